"""Guided sampling on the GPU (hqt_set_guidance, guidance=, guidance_scale=).

Every image of a guided call is two rows of one pass, one per condition; guide_logits_kernel writes g = l_pos + (s - 1) (l_pos - l_neg) over both rows between
the head GEMM and the sampler, and both rows draw with one Philox key.  What is checked:

 * the kernel bit for bit against three float32 numpy operations (tests/guidance_ref.py::mix), in every precision, eager and graphed, on every depth head:
   with all levels forced the model sees the same inputs with and without the table, so the dumped rows of the two calls are related by ``mix`` exactly;
 * scale 1 draws what no table draws;
 * an EXACT free run against the oracle drawing from the mixed rows.  A logit error e per row becomes at most (|s| + |s - 1|) e in the guided row, so a draw
   is decided when its winner / runner-up ratio of p / q is at least exp(2 (|s| + |s - 1|) e / T) (guidance_ref.safe_ratio) with the project's EXACT logit
   tolerance e = 2e-4.  The noise seeds below were picked on the CPU, with the oracle alone, so that every draw clears that ratio; each test asserts it
   before it compares.  Seeds and the smallest ratio they give (oracle, CPU):
       class, plain            seed 100: ratio 1.005734 (needed 1.001201)
       class, top-k            seed 100: ratio 1.013280 (needed 1.001001)
       class, top-k + top-p    seed 101: ratio 1.007708 (needed 1.001144)
       class, prefix of 3      seed 200: ratio 1.007653 (needed 1.001001)
       text, [PAD] negative    seed 300: ratio 1.002717 (needed 1.001001)
 * FAST: guided logits within (|s| + |s - 1|) x the FAST teacher-forced gate of the tiny class model (0.15, tests/test_gpu_parity.py), by the triangle
   inequality; draws identical wherever the ratio clears the same formula with that tolerance;
 * log-probabilities, merged passes, and every refusal."""
import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.models import HQTransformerStage2
from hqtransformer_amd.pipeline import InflightSampler
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.text import PAD_ID, pad_caption
from oracle import hqt_oracle as O
from oracle.hqt_oracle import OracleStage2
from tests.guidance_ref import guided_oracle, level_of_draw, mix, safe_ratio
from tests.helpers import gate, load, stage2_from_fixture
from tests.prefix_ref import oracle_complete
from tests.test_gpu_logprobs import check_own, engine_s2, l3_noise, np_, synth_engine

pytestmark = pytest.mark.gpu
PRECISIONS = [PRECISION_EXACT, PRECISION_SPLIT, PRECISION_FAST]
LOGIT_TOL = 2e-4                 # the project's EXACT logit gate
FAST_GATE = 0.15                 # tests/test_gpu_parity.py::test_fast_precision_teacher_forced: FAST against EXACT on the tiny class model, teacher-forced
SCALES = (1.5, 2.0)
# three sampler settings: (top_k, top_p, temperature), each per level
SETTINGS = {'plain': ((None, None), (None, None), (1.0, 1.0)), 'topk': ((50, 20), (None, None), (0.8, 1.2)), 'topp': ((50, 20), (0.9, 0.8), (0.7, 1.3))}
# picked on the CPU with the oracle alone (free_run_case / prefix_case / text_case below under guided_oracle): (noise seed, smallest ratio it gives)
SEEDS = {'plain': (100, 1.005734), 'topk': (100, 1.01328), 'topp': (101, 1.007708), 'prefix': (200, 1.007653), 'text': (300, 1.002717)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------- 1. / 2. the kernel, bit for bit
def forced_case(levels, B, n, V, pairs, seed):
    """Forced codes of every level and explicit noise; the two rows of a pair get the same of both (what hqt.h asks of the caller)."""
    rng = np.random.default_rng([seed, 0x6d1])
    draws = (4 ** levels - 1) // 3
    force = [rng.integers(0, V, (B, n) + ((4 ** l,) if l else ())) for l in range(levels)]
    noise = np.maximum(rng.standard_exponential((n, draws, B, V), dtype=np.float32), np.float32(1e-30))
    for pos, neg in pairs:
        noise[:, :, neg] = noise[:, :, pos]
        for f in force:
            f[neg] = f[pos]
    return [torch.from_numpy(f) for f in force], torch.from_numpy(noise)


def run(eng, levels, B, cond, n, **kw):
    """(codes [B, n, draws], logits [n, draws, B, V]) of a call with return_logits, whatever the level count."""
    force = kw.pop('force')
    if levels == 3:
        out = eng.sample3(B, cond, n, force=force, return_logits=True, **kw)
    else:
        out = eng.sample(B, cond, n, force_top=force[0], force_bot=force[1], return_logits=True, **kw)
    eng.range_check()
    torch.cuda.synchronize()
    codes = np.concatenate([np_(c).reshape(B, n, -1) for c in out[:levels]], axis=2)
    return codes, np_(out[levels])


def check_identity(what, L, G, codes, plain_codes, pairs, scales, B):
    """G[pos] == G[neg] == mix(L[pos], L[neg], s_level) and G[other rows] == L, bitwise, for every position and draw; equal codes within a pair."""
    draws = L.shape[1]
    paired = set()
    for pos, neg in pairs:
        paired |= {pos, neg}
        for d in range(draws):
            want = mix(L[:, d, pos], L[:, d, neg], scales[level_of_draw(d)])
            assert (bits(G[:, d, pos]) == bits(want)).all(), f'{what}: row {pos} draw {d} is not the mixed row'
            assert (bits(G[:, d, neg]) == bits(want)).all(), f'{what}: row {neg} draw {d} is not the mixed row'
        assert (codes[pos] == codes[neg]).all(), f'{what}: rows {pos} and {neg} drew different codes'
    for b in set(range(B)) - paired:
        assert (bits(G[:, :, b]) == bits(L[:, :, b])).all(), f'{what}: row {b} is in no pair and was touched'
        assert (codes[b] == plain_codes[b]).all(), f'{what}: row {b} is in no pair and drew other codes'


def kernel_identity(eng, levels, V, precisions, scale_sets, n=4, seed=3, what=''):
    B, pairs = 5, [(0, 3), (4, 1)]                   # a pair with pos_row > neg_row, and row 2 in no pair
    cond = torch.tensor([1, 2, 3, 4, 5])
    force, noise = forced_case(levels, B, n, V, pairs, seed)
    for precision in precisions:
        for graph in (False, True):
            kw = dict(precision=precision, noise=noise, force=list(force), use_graph=graph)
            plain_codes, L = run(eng, levels, B, cond, n, **kw)
            for scales in scale_sets if graph else scale_sets[:1]:       # other values of the same size replay the same graph
                codes, G = run(eng, levels, B, cond, n, guidance=[(p, q, scales) for p, q in pairs], **kw)
                check_identity(f'{what} V={V} precision={precision} graph={graph} scales={scales}', L, G, codes, plain_codes, pairs, scales, B)
                assert any((bits(G[:, d, 0]) != bits(L[:, d, 0])).any() for d in range(L.shape[1]) if scales[level_of_draw(d)] != 1.0), \
                    'the guided rows equal the unguided ones: the case shows nothing'


@pytest.mark.parametrize('V', [516, 8192, 16384])
def test_kernel_bit_for_bit_two_levels(V):
    """V = 516: 129 float4 groups (a tail inside the first round of the 256 threads); 8192 / 16384: 8 / 16 groups per thread.  The engine refuses any V that
    is not a multiple of 4, so there is no such case.  FAST on this root handle with 5 rows takes the persistent launch."""
    spec, eng = synth_engine(V)
    kernel_identity(eng, 2, V, PRECISIONS, [(1.0, 2.5), (0.0, -1.0)], what='synthetic')


@pytest.mark.parametrize('name', ['g7_l3_tiny_cls.npz', 'g7_l3_tiny_cls_top2mid2bot.npz'])
def test_kernel_bit_for_bit_three_levels(name):
    """Sub-steps of 1, 4 and 16 rows per sample ('parallel-add'), and 21 one-row sub-steps ('top2mid2bot'), three different scales."""
    fx = load(name)
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 8)
    kernel_identity(eng, 3, spec.vocab_top, PRECISIONS, [(1.5, 0.5, 3.0), (-1.0, 2.0, 0.0)], n=3, what=name)


def test_kernel_bit_for_bit_bidirectional():
    fx = load('g13_tiny_cls_bidirectional.npz')
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 8)
    kernel_identity(eng, 2, spec.vocab_top, PRECISIONS, [(1.0, 2.5), (0.0, -1.0)], what='bidirectional')


# ------------------------------------------------------------------------------- 3. scale 1
@pytest.fixture(scope='module')
def g4():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    return fx, spec, weights, engine_s2(spec, weights, 8, max_prefix=3)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_scale_one_is_no_guidance(g4, precision):
    fx, spec, weights, eng = g4
    n, steps, seed = 4, 8, 41
    cond = torch.tensor([7, 1, 2, 3, 4, 4, 5, 6])
    kw = dict(precision=precision, top_k=(50, 20), temperature=(0.8, 1.2))
    for graph in (False, True):
        guided = eng.sample(2 * n, cond, steps, seed=seed, guidance=[(i, n + i, 1.0) for i in range(n)], use_graph=graph, **kw)
        # the same 2 n-row pass without a table, the negative rows given their positive rows' keys
        plain = eng.sample(2 * n, cond, steps, row_seeds=[seed] * (2 * n), row_offsets=list(range(n)) * 2, use_graph=graph, **kw)
        eng.range_check()
        torch.cuda.synchronize()
        for g, p in zip(guided, plain):
            assert torch.equal(g[:n], p[:n]), f'precision={precision} graph={graph}: scale 1 changed a draw of a positive row'
            assert torch.equal(g[n:], g[:n]), 'the negative rows did not draw their positive rows\' codes'


# ------------------------------------------------------------------------------- 4. EXACT free run against the oracle
N_PAIRS, STEPS = 4, 8


def class_cond():
    return np.array([7, 1, 2, 3, 4, 4, 5, 6], np.int64)           # positives, then the class each is pushed away from


def free_run_case(orc, key, seed):
    """The oracle's guided free run of 2 N_PAIRS rows: (codes_top, codes_bot, noise of the N_PAIRS positive rows, smallest ratio)."""
    tk, tp, T = SETTINGS[key]
    noise = synth.exp_noise(seed, STEPS, N_PAIRS, orc.s.vocab_top)
    with guided_oracle(N_PAIRS, SCALES) as sink:
        ct, cb = orc.sample(class_cond(), 2 * N_PAIRS, STEPS, np.concatenate([noise, noise], axis=2), tk, tp, T)
    assert len(sink) == 5 * STEPS
    return ct, cb, noise, min(sink)


def prefix_case(orc, seed, P=3):
    tk, tp, T = SETTINGS['topk']
    rng = np.random.default_rng([seed, 0x51ed])
    prefix = [rng.integers(0, orc.s.vocab_top, (N_PAIRS, P)), rng.integers(0, orc.s.vocab_top, (N_PAIRS, P, 4))]
    noise = synth.exp_noise(seed, STEPS, N_PAIRS, orc.s.vocab_top)
    with guided_oracle(N_PAIRS, SCALES):
        ct, cb, _, margin = oracle_complete(orc, class_cond(), 2 * N_PAIRS, STEPS, np.concatenate([noise, noise], axis=2), P,
                                            [np.concatenate([p, p]) for p in prefix], tk, tp, T)
    return ct, cb, noise, margin, prefix


def text_case(orc, txt, seed):
    tk, tp, T = SETTINGS['topk']
    n = txt.shape[0]
    noise = synth.exp_noise(seed, STEPS, n, orc.s.vocab_top)
    cond = np.concatenate([txt, np_(pad_caption(n, txt.shape[1]))])
    with guided_oracle(n, SCALES) as sink:
        ct, cb = orc.sample(cond, 2 * n, STEPS, np.concatenate([noise, noise], axis=2), tk, tp, T)
    return ct, cb, noise, min(sink)


def text_prompts(fx, spec):
    return synth.text_ids(int(fx['text_seed']), 3, spec.ctx_len_txt, spec.vocab_txt)


def guided_call(eng, cond, noise, key, **kw):
    tk, tp, T = SETTINGS[key]
    n = noise.shape[2]
    noise2 = torch.from_numpy(np.concatenate([noise, noise], axis=2))
    return eng.sample(2 * n, torch.from_numpy(cond), STEPS, precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=noise2,
                      guidance=[(i, n + i, SCALES) for i in range(n)], **kw)


def assert_safe(what, ratio, key):
    need = safe_ratio(SCALES, LOGIT_TOL, SETTINGS[key][2])
    print(f'{what}: smallest winner / runner-up ratio {ratio:.6f}, needed {need:.6f}')
    assert ratio >= need, f'{what}: the oracle\'s run is not well-conditioned (ratio {ratio} < {need}): pick another noise seed'


@pytest.mark.parametrize('key', ['plain', 'topk', 'topp'])
def test_free_run_matches_the_oracle(g4, key):
    fx, spec, weights, eng = g4
    ct, cb, noise, ratio = free_run_case(OracleStage2(spec, weights), key, SEEDS[key][0])
    assert_safe(f'class, {key}', ratio, key)
    for graph in (False, True):
        got_t, got_b = guided_call(eng, class_cond(), noise, key, use_graph=graph)
        torch.cuda.synchronize()
        assert (np_(got_t) == ct).all() and (np_(got_b) == cb).all(), f'{key} graph={graph}: codes differ from the oracle\'s guided run'
    assert (ct[:N_PAIRS] == ct[N_PAIRS:]).all() and (cb[:N_PAIRS] == cb[N_PAIRS:]).all()


def test_free_run_with_a_prefix_matches_the_oracle(g4):
    fx, spec, weights, eng = g4
    ct, cb, noise, ratio, prefix = prefix_case(OracleStage2(spec, weights), SEEDS['prefix'][0])
    assert_safe('class, prefix of 3', ratio, 'topk')
    got_t, got_b = guided_call(eng, class_cond(), noise, 'topk', prefix=[torch.from_numpy(np.concatenate([p, p])) for p in prefix])
    torch.cuda.synchronize()
    assert (np_(got_t) == ct).all() and (np_(got_b) == cb).all()


def test_text_model_defaults_to_the_pad_caption():
    """Through the sampling surface: ``guidance_scale`` alone on a text model pairs every prompt with the all-[PAD] caption and returns the prompts' rows."""
    fx = load('g3_tiny_txt.npz')
    spec, weights = stage2_from_fixture(fx)
    txt = text_prompts(fx, spec)
    ct, cb, noise, ratio = text_case(OracleStage2(spec, weights), txt, SEEDS['text'][0])
    assert_safe('text, [PAD] negative', ratio, 'topk')
    st2 = HQTransformerStage2(spec)
    st2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    st2.to('cuda')
    tk, tp, T = SETTINGS['topk']
    got_t, got_b = sampling_ihqgpt(st2, 1, torch.from_numpy(txt), top_k_top=tk[0], top_k_bot=tk[1], softmax_temperature=list(T), use_fp16=False,
                                   is_tqdm=False, max_seq_len=STEPS, noise=torch.from_numpy(noise), guidance_scale=SCALES)
    torch.cuda.synchronize()
    n = txt.shape[0]
    assert tuple(got_t.shape) == (n, STEPS) and tuple(got_b.shape) == (n, STEPS, 4)
    assert (np_(got_t) == ct[:n]).all() and (np_(got_b) == cb[:n]).all()
    assert PAD_ID < spec.vocab_txt


# ------------------------------------------------------------------------------- 5. FAST
def test_fast_guided_logits_and_draws(g4):
    fx, spec, weights, eng = g4
    key = 'topk'
    tk, tp, T = SETTINGS[key]
    n = N_PAIRS
    ct, cb, noise, _ = free_run_case(OracleStage2(spec, weights), key, SEEDS[key][0])
    kw = dict(force_top=torch.from_numpy(ct), force_bot=torch.from_numpy(cb), return_logits=True)
    ex = guided_call(eng, class_cond(), noise, key, use_graph=False, **kw)
    growth = [abs(s) + abs(s - 1.0) for s in SCALES]
    noise2 = np.concatenate([noise, noise], axis=2)
    for graph in (False, True):
        fa = eng.sample(2 * n, torch.from_numpy(class_cond()), STEPS, precision=PRECISION_FAST, top_k=tk, top_p=tp, temperature=T,
                        noise=torch.from_numpy(noise2), guidance=[(i, n + i, SCALES) for i in range(n)], use_graph=graph, **kw)
        eng.range_check()
        torch.cuda.synchronize()
        Ge, Gf = np_(ex[2]), np_(fa[2])
        codes_f = np.concatenate([np_(fa[0])[..., None], np_(fa[1])], axis=2)      # [2 n, steps, 5]
        compared = total = 0
        for d in range(5):
            lv = level_of_draw(d)
            gate(f'tiny_cls.guided_fast_logits(level={lv},draw={d},graph={graph})', np.abs(Gf[:, d] - Ge[:, d]).max(), growth[lv] * FAST_GATE)
            need = float(np.exp(2.0 * growth[lv] * FAST_GATE / T[lv]))
            for step in range(STEPS):
                idx, pr = O.sample_filtered(Ge[step, d], noise2[step, d], T[lv], tk[lv], tp[lv])
                part = np.partition(pr / noise2[step, d], -2, axis=-1)
                safe = part[:, -1] >= need * part[:, -2]
                assert (codes_f[safe, step, d] == idx[safe]).all(), f'graph={graph}: a well-conditioned FAST draw (step {step}, draw {d}) differs'
                compared, total = compared + int(safe.sum()), total + safe.size
        print(f'graph={graph}: {compared} of {total} draws clear the FAST ratio and were compared')
        assert compared > 0
        assert torch.equal(fa[0][:n], fa[0][n:]) and torch.equal(fa[1][:n], fa[1][n:])


# ------------------------------------------------------------------------------- 6. log-probabilities
@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_FAST])
def test_logprobs_score_the_code_under_the_guided_row(g4, precision):
    fx, spec, weights, eng = g4
    n = N_PAIRS
    for graph in (False, True):
        out = eng.sample(2 * n, torch.from_numpy(class_cond()), STEPS, precision=precision, seed=61, top_k=(50, 20), temperature=(0.8, 1.2),
                         guidance=[(i, n + i, SCALES) for i in range(n)], return_logits=True, return_logprobs=True, use_graph=graph)
        eng.range_check()
        torch.cuda.synchronize()
        check_own(out, 2, f'guided precision={precision} graph={graph}')
        assert torch.equal(out[3][:n], out[3][n:]), 'the two rows of a pair report different log-probabilities'
        assert (bits(np_(out[2])[:, :, :n]) == bits(np_(out[2])[:, :, n:])).all()


# ------------------------------------------------------------------------------- 7. merged passes
def test_merged_pass_mixes_guided_and_unguided_steps():
    import os
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = ImageGPT2(load_config(os.path.join(root, 'configs', 'tiny-cls.yaml')), seed=5).to('cuda').eval()
    n = 64                                           # a merged pass decodes what it samples: all 64 positions of the tiny model's images
    kw = dict(max_seq_len=n, use_fp16=False, top_k_top=50, top_k_bot=20)
    pipe = InflightSampler(model, lanes=1, merge=2)
    p0 = pipe.submit(3, torch.tensor([5, 6, 7]), seed=71, guidance_scale=SCALES, neg_cond=9, precision='exact', **kw)
    p1 = pipe.submit(2, 3, seed=72, sample_offset=64, precision='exact', **kw)
    pipe.drain()
    torch.cuda.synchronize()
    r0, r1 = p0.get(), p1.get()
    assert tuple(r0[0].shape) == (3, n) and tuple(r1[0].shape) == (2, n) and r0[2].shape[0] == 3 and r1[2].shape[0] == 2
    a = sampling_ihqgpt(model.stage2, 3, torch.tensor([5, 6, 7]), seed=71, guidance_scale=SCALES, neg_cond=9, is_tqdm=False, **kw)
    b = sampling_ihqgpt(model.stage2, 2, 3, seed=72, sample_offset=64, is_tqdm=False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a[0], r0[0]) and torch.equal(a[1], r0[1]), 'the guided step of a merged pass differs from its separate call'
    assert torch.equal(b[0], r1[0]) and torch.equal(b[1], r1[1]), 'the unguided step of a merged pass differs from its separate call'
    plain = sampling_ihqgpt(model.stage2, 3, torch.tensor([5, 6, 7]), seed=71, is_tqdm=False, **kw)
    assert not torch.equal(plain[0], a[0]), 'guidance changed nothing: the case shows nothing'


# ------------------------------------------------------------------------------- 8. what is refused
def test_refusals_and_nothing_left_staged(g4):
    fx, spec, weights, eng = g4
    B, steps = 4, 4
    cond = torch.tensor([7, 1, 2, 3])
    kw = dict(precision=PRECISION_EXACT, seed=81, use_graph=False)
    want = eng.sample(B, cond, steps, **kw)
    torch.cuda.synchronize()
    same = ((1.0, 1.0), (None, None), (None, None))
    cases = [
        (dict(guidance=[(0, 4, 2.0)]), r'rows \(0, 4\) outside \[0, B=4\)'),
        (dict(guidance=[(-1, 2, 2.0)]), r'rows \(-1, 2\) outside \[0, B=4\)'),
        (dict(guidance=[(1, 1, 2.0)]), r'pos_row == neg_row == 1'),
        (dict(guidance=[(0, 1, 2.0), (2, 1, 2.0)]), r'row 1 appears in more than one pair'),
        (dict(guidance=[(0, 1, (2.0, float('inf')))]), r'scale\[1\] is not finite'),
        (dict(guidance=[(0, 1, (float('nan'), 1.0))]), r'scale\[0\] is not finite'),
        (dict(guidance=[(0, 1, 2.0)], row_samplers=[same, ((0.5, 1.0), (None, None), (None, None)), same, same]), r'different sampler settings'),
        (dict(guidance=[(0, 1, 2.0)], row_seeds=[81, 82, 81, 81], row_offsets=[0, 0, 2, 3]), r'different keys'),
        (dict(guidance=[(0, 1, 2.0)], row_seeds=[81] * 4, row_offsets=[0, 1, 2, 3]), r'different keys'),
    ]
    for extra, message in cases:
        call = dict(kw)
        if 'row_seeds' in extra:
            call.pop('seed')
        with pytest.raises(_lib.HqtError, match=message) as err:
            eng.sample(B, cond, steps, **call, **extra)
        assert err.value.code == -1                  # HQT_ERR_INVALID
        # a failed call leaves nothing staged: the next plain call draws what it always drew
        got = eng.sample(B, cond, steps, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f'after "{message}": a table was left staged'
    # more pairs than rows could hold is refused when the table is staged
    with pytest.raises(_lib.HqtError, match=r'n_pairs=5 outside \[0, max_batch / 2 = 4\]'):
        eng.sample(B, cond, steps, guidance=[(0, 1, 2.0)] * 5, **kw)
    # the same keys given explicitly are accepted, and give what the implicit ones give
    a = eng.sample(B, cond, steps, guidance=[(0, 1, 2.0)], **kw)
    b = eng.sample(B, cond, steps, guidance=[(0, 1, 2.0)], row_seeds=[81] * 4, row_offsets=[0, 0, 2, 3], precision=PRECISION_EXACT, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0][0], a[0][1])


def test_unconditional_model_is_refused():
    fx = load('g3_tiny_reduce_uncond.npz')
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 4)
    want = eng.sample(4, None, 4, precision=PRECISION_EXACT, seed=5, use_graph=False)
    with pytest.raises(_lib.HqtError, match='HQT_COND_NONE'):
        eng.sample(4, None, 4, precision=PRECISION_EXACT, seed=5, use_graph=False, guidance=[(0, 1, 2.0)])
    got = eng.sample(4, None, 4, precision=PRECISION_EXACT, seed=5, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
