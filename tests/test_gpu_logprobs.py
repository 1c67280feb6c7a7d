"""Log-probabilities of sampled codes (hqt_set_logprob_out, return_logprobs=) on the GPU.

The kernel computes, in fp32, l[code] - max(l) - log(sum exp(l - max(l))) over the raw logits row of a draw: two passes, IEEE expf / logf, 256 threads per row,
per thread a pairwise tree over its float4 groups, the wave's butterfly, then the four wave sums.  Against an fp64 log-softmax of the SAME fp32 row the bound is

    tol(l) = 2^-24 * (32 + 4 * max|l|)

4 max|l|: one rounding each in l - max and in the two final subtractions (operands up to 2 max|l|); 32: one ulp of expf, a reduction tree over at most 16384
terms (here 14 levels deep: 2 within a float4, up to 4 over a thread's groups, 6 in the wave, 2 over the waves -- no deeper than the 256-lane strided sum +
pairwise tree the constant was derived for), logf, and the ulp of a log-sum <= 9.7.  The bound is taken per row, from that row's own max|l|.  Every test prints
its largest error / bound ratio before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.pipeline import InflightSampler, sample_best_of, score_codes, sequence_logprob
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from tests.helpers import load, stage2_from_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 2e-4                 # the project's EXACT logit gate against the reference's fixtures
FAST_LOGIT_GATE = 0.06           # ... and its FAST teacher-forced one
PRECISIONS = [PRECISION_EXACT, PRECISION_SPLIT, PRECISION_FAST]


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_steps=None, max_prefix=0):
    e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img, max_prefix=max_prefix)
    e.load(stage2=weights)
    e.finalize()
    return e


def np_(t):
    return t.detach().cpu().numpy()


def l3_noise(seed, n, B, V):
    return np.maximum(np.random.default_rng(seed).standard_exponential((n, 21, B, V), dtype=np.float32), np.float32(1e-30))


def all_codes(codes):
    """Code levels [B, n], [B, n, 4][, [B, n, 16]] -> int64 [B, n, draws] in draw order."""
    B, n = codes[0].shape
    return np.concatenate([(np_(c) if torch.is_tensor(c) else np.asarray(c)).reshape(B, n, -1) for c in codes], axis=2)


def reference(logits, codes):
    """fp64 log-softmax of fp32 rows [n, draws, B, V] at codes [B, n, draws] -> (log-probabilities, tol of every row), both [B, n, draws]."""
    l = np.asarray(logits, np.float32).astype(np.float64)
    m = l.max(-1)
    lse = m + np.log(np.exp(l - m[..., None]).sum(-1))
    picked = np.take_along_axis(l, codes.transpose(1, 2, 0)[..., None], -1)[..., 0]
    tol = 2.0 ** -24 * (32.0 + 4.0 * np.abs(l).max(-1))
    return (picked - lse).transpose(2, 0, 1), tol.transpose(2, 0, 1)


def check_own(out, levels, what):
    """out = (*codes, logits, logprobs) of ONE call: the log-probabilities against the fp64 log-softmax of that call's own dumped rows at its own codes."""
    codes, lg, lp = out[:levels], out[levels], out[levels + 1]
    want, tol = reference(np_(lg), all_codes(codes))
    got = np_(lp)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.isfinite(got).all(), f'{what}: a log-probability is not finite'
    ratio = (np.abs(got.astype(np.float64) - want) / tol).max()
    print(f'{what}: largest error / bound {ratio:.3f} (largest |logit| {np.abs(np_(lg)).max():.2f}, log-probabilities in [{got.min():.3f}, {got.max():.3f}])')
    assert ratio <= 1.0, f'{what}: error {ratio:.3f} x the bound'
    assert (got <= 0.0).all()


@pytest.fixture(scope='module')
def g4():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    return fx, spec, weights, engine_s2(spec, weights, 8)


_SYNTH = {}


def synth_engine(V):
    """1-layer D = 64 models (the shape of test_gpu_row_samplers.py::full_vocab) at the vocabularies where the kernel changes its path: 516 (129 float4 groups: a
    tail inside the first round of the 256 threads), 8192 (8 groups per thread) and 16384 (16: the largest vocabulary the engine takes)."""
    if V not in _SYNTH:
        spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=V, vocab_bot=V, vocab_txt=64,
                          ctx_len_img=16, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
        _SYNTH[V] = (spec, engine_s2(spec, synth.stage2_weights(spec, 51, 'fixture'), 8))
    return _SYNTH[V]


# ------------------------------------------------------------------------------- 1. against the reference's fixture
@pytest.mark.parametrize('si', [0, 1, 2])
@pytest.mark.parametrize('graph', [False, True])
def test_fixture_logits_give_these_logprobs(g4, si, graph):
    fx, spec, weights, eng = g4
    tk, tp, T = json.loads(str(fx['settings']))[si]
    B, n = int(fx['B']), int(fx['n_steps'])
    noise = synth.exp_noise(int(fx['noise_seed']), n, B, spec.vocab_top)
    ct, cb, lp = eng.sample(B, torch.full((B,), 7), n, precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=torch.from_numpy(noise),
                            return_logprobs=True, use_graph=graph)
    torch.cuda.synchronize()
    assert (np_(ct) == fx[f'codes_top_{si}']).all() and (np_(cb) == fx[f'codes_bot_{si}']).all()      # the rows line up
    keep = fx['keep_steps']
    scale = np.array([T[0]] + [T[1]] * 4, np.float32)[None, :, None, None]
    raw = fx[f'logits_{si}'] * scale                          # the fixture keeps post-temperature logits
    codes = all_codes([fx[f'codes_top_{si}'], fx[f'codes_bot_{si}']])[:, keep]
    want, tol = reference(raw, codes)
    got = np_(lp)[:, keep]
    bound = 2.0 * LOGIT_TOL * max(T) + tol                    # log-softmax moves at most twice the sup-norm change of its row
    ratio = (np.abs(got - want) / bound).max()
    print(f'settings {si} graph={graph}: largest error / bound {ratio:.4f}; expected in [{want.min():.3f}, {want.max():.3f}], max |logit| {np.abs(raw).max():.2f}')
    assert ratio <= 1.0
    assert np.isfinite(np_(lp)).all() and (np_(lp) <= 0).all()


# ------------------------------------------------------------------------------- 2. against the call's own logits
CUT = dict(top_k=(50, 20), top_p=(0.9, 0.8), temperature=(0.7, 1.3))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_own_logits_tiny(g4, precision):
    fx, spec, weights, eng = g4
    B, n = 4, 8
    for graph in (False, True):
        out = eng.sample(B, torch.tensor([7, 1, 2, 3]), n, precision=precision, seed=21, return_logits=True, return_logprobs=True, use_graph=graph, **CUT)
        eng.range_check()
        torch.cuda.synchronize()
        check_own(out, 2, f'tiny V=512 precision={precision} graph={graph}')


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('V', [516, 8192, 16384])
def test_own_logits_synthetic(V, precision):
    spec, eng = synth_engine(V)
    B, n = 5, 4
    cut = dict(CUT) if V <= 8192 else dict(top_k=(50, 20), temperature=(0.7, 1.3))       # top-p needs V <= 8192
    for graph in (False, True):
        out = eng.sample(B, torch.tensor([1, 2, 3, 4, 5]), n, precision=precision, seed=22, return_logits=True, return_logprobs=True, use_graph=graph, **cut)
        eng.range_check()
        torch.cuda.synchronize()
        check_own(out, 2, f'synthetic V={V} precision={precision} graph={graph}')
    # cut-offs and temperature do not enter the value: a call that draws differently scores the codes IT drew from the same kind of row
    out = eng.sample(B, torch.tensor([1, 2, 3, 4, 5]), n, precision=precision, seed=22, return_logits=True, return_logprobs=True)
    eng.range_check()
    torch.cuda.synchronize()
    check_own(out, 2, f'synthetic V={V} precision={precision} no cut-off')


# ------------------------------------------------------------------------------- 3. every head and conditioning kind
@pytest.mark.parametrize('name', ['g7_l3_tiny_cls.npz', 'g7_l3_tiny_cls_top2mid2bot.npz'])
def test_three_levels(name):
    """21 draws per position; 'top2mid2bot': 21 one-token sub-steps, each writing one slot of a 4- or 16-wide code group (out_stride / out_slot)."""
    fx = load(name)
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 4)
    B, n = int(fx['B']), 6
    tk, tp, T = json.loads(str(fx['settings']))[-1]
    cond = torch.full((B,), int(fx['cond']) if 'cond' in fx.files else 7)
    for precision, kw in ((PRECISION_EXACT, dict(noise=torch.from_numpy(l3_noise(8, n, B, spec.vocab_top)))), (PRECISION_FAST, dict(seed=23))):
        for graph in (False, True):
            out = eng.sample3(B, cond, n, precision=precision, top_k=tk, top_p=tp, temperature=T, return_logits=True, return_logprobs=True, use_graph=graph, **kw)
            eng.range_check()
            torch.cuda.synchronize()
            assert tuple(out[-1].shape) == (B, n, 21)
            check_own(out, 3, f'{name} precision={precision} graph={graph}')


def test_bidirectional_head():
    fx = load('g13_tiny_cls_bidirectional.npz')
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 4)
    B, n = int(fx['B']), 6
    tk, tp, T = json.loads(str(fx['settings']))[0]
    for precision in (PRECISION_EXACT, PRECISION_FAST):
        for graph in (False, True):
            out = eng.sample(B, torch.full((B,), int(fx['cond'])), n, precision=precision, top_k=tk, top_p=tp, temperature=T, seed=24,
                             return_logits=True, return_logprobs=True, use_graph=graph)
            eng.range_check()
            torch.cuda.synchronize()
            check_own(out, 2, f'bidirectional precision={precision} graph={graph}')


def test_text_conditioning():
    fx = load('g3_tiny_txt.npz')
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 4)
    B, n = int(fx['B']), 6
    txt = torch.from_numpy(synth.text_ids(int(fx['text_seed']), B, spec.ctx_len_txt, spec.vocab_txt))
    for precision in (PRECISION_EXACT, PRECISION_FAST):
        for graph in (False, True):
            out = eng.sample(B, txt, n, precision=precision, seed=25, return_logits=True, return_logprobs=True, use_graph=graph, **CUT)
            eng.range_check()
            torch.cuda.synchronize()
            check_own(out, 2, f'text precision={precision} graph={graph}')          # position 0 is drawn by the prompt's prefill pass


def test_row_samplers(g4):
    fx, spec, weights, eng = g4
    B, n = 4, 6
    rows = [((1.0, 1.0), (None, None), (None, None)), ((0.7, 1.3), (50, 20), (0.9, 0.8)), ((1.0, 0.9), (5, 5), (None, None)), ((0.7, 1.3), (50, 20), (0.9, 0.8))]
    for precision in (PRECISION_EXACT, PRECISION_FAST):
        out = eng.sample(B, torch.tensor([7, 1, 2, 3]), n, precision=precision, seed=26, row_samplers=rows, return_logits=True, return_logprobs=True)
        eng.range_check()
        torch.cuda.synchronize()
        check_own(out, 2, f'row table precision={precision}')


# ------------------------------------------------------------------------------- 4. forcing
def test_given_top_code_scores_the_given_code(g4):
    fx, spec, weights, eng = g4
    B = int(fx['B'])
    noise = synth.exp_noise(int(fx['noise_seed']), 64, B, spec.vocab_top)[:8]
    ct, cb, lp = eng.sample(B, torch.full((B,), 3), 8, precision=PRECISION_EXACT, noise=torch.from_numpy(noise.copy()),
                            force_top=torch.from_numpy(fx['given_top']), return_logprobs=True, use_graph=False)
    torch.cuda.synchronize()
    assert (np_(cb) == fx['given_codes_bot']).all()
    assert (np_(ct) != fx['given_top']).any(), 'every drawn top code equals the given one: the case cannot tell which of the two is scored'
    # draw 0: the GIVEN top code (the one fed forward), not the drawn one; draws 1-4: the drawn bottom codes, which are the fixture's
    want, tol = reference(fx['given_logits'], all_codes([fx['given_top'], fx['given_codes_bot']]))
    bound = 2.0 * LOGIT_TOL * 1.0 + tol
    ratio = (np.abs(np_(lp) - want) / bound).max()
    print(f'given_top: largest error / bound {ratio:.4f}')
    assert ratio <= 1.0
    drawn, _ = reference(fx['given_logits'], all_codes([np_(ct), fx['given_codes_bot']]))
    differ = np_(ct) != fx['given_top']
    assert (np.abs(np_(lp)[..., 0] - drawn[..., 0])[differ] > bound[..., 0][differ]).any(), 'draw 0 reads like the score of the DRAWN code'


@pytest.fixture(scope='module')
def tiny_model():
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to('cuda').eval()


def test_score_codes_returns_the_free_runs_logprobs(tiny_model):
    st2 = tiny_model.stage2
    B, n = 4, 8
    cond = torch.tensor([417, 3, 99, 7])
    ct, cb, lp = sampling_ihqgpt(st2, num_candidates=B, cond=cond, use_fp16=False, is_tqdm=False, max_seq_len=n, seed=31, top_k_top=50, top_k_bot=20,
                                 softmax_temperature=[0.8, 1.2], return_logprobs=True)
    got = score_codes(st2, [ct, cb], cond, precision='exact')
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, n, 5) and got.dtype == torch.float32
    assert torch.equal(got, lp), f'EXACT: the scored codes differ from their free run by {(got - lp).abs().max().item()}'       # same logits, same codes: same bits
    # sum = the sequence score; a host copy of the codes scores the same
    assert torch.equal(sequence_logprob(got), sequence_logprob(lp))
    assert torch.equal(score_codes(st2, [ct.cpu(), cb.cpu()], cond, precision='exact', use_graph=False), lp)
    # FAST: the free run's own logits against the teacher-forced ones, within the project's FAST logit gate on either side of the log-softmax
    eng = st2.engine(B, n)
    fct, fcb, flg, flp = eng.sample(B, cond, n, precision=PRECISION_FAST, seed=32, return_logits=True, return_logprobs=True)
    fgot = score_codes(st2, [fct, fcb], cond, precision='fast')
    st2.range_check()
    torch.cuda.synchronize()
    _, tol = reference(np_(flg), all_codes([fct, fcb]))
    err = np.abs(np_(fgot).astype(np.float64) - np_(flp))
    print(f'FAST: scored vs free run, largest difference {err.max():.3e}')
    assert (err <= 2 * FAST_LOGIT_GATE + tol).all()


# ------------------------------------------------------------------------------- 5. prefix
def test_prefix_positions_are_nan_and_the_rest_is_the_free_run(g4):
    fx, spec, weights, _ = g4
    eng = engine_s2(spec, weights, 4, max_prefix=3)
    B, n, P = 4, 8, 3
    cond = torch.tensor([7, 1, 2, 3])
    kw = dict(precision=PRECISION_EXACT, seed=41, top_k=(50, 20), temperature=(0.9, 1.1))
    ct, cb, lp = eng.sample(B, cond, n, return_logprobs=True, **kw)
    for graph in (False, True):
        pt, pb, plp = eng.sample(B, cond, n, prefix=[ct[:, :P].clone(), cb[:, :P].clone()], return_logprobs=True, use_graph=graph, **kw)
        torch.cuda.synchronize()
        assert torch.equal(pt, ct) and torch.equal(pb, cb)
        assert torch.isnan(plp[:, :P]).all(), 'positions below the prefix must read NaN'
        assert torch.isfinite(plp[:, P:]).all()
        print(f'prefix graph={graph}: largest difference from the free run {(plp[:, P:] - lp[:, P:]).abs().max().item():.3e}')
        assert torch.equal(plp[:, P:], lp[:, P:]), 'EXACT: the completion scores differ from the free run that produced the prefix'
        assert torch.isnan(sequence_logprob(plp)).all() and torch.isfinite(sequence_logprob(plp[:, P:])).all()


# ------------------------------------------------------------------------------- 6. nothing else moved
@pytest.mark.parametrize('precision', PRECISIONS)
def test_codes_do_not_change_and_the_launches_are_counted(precision):
    spec, eng = synth_engine(8192)                # FAST, 5 rows on a root handle: the persistent launch up to the top logits
    B, n = 5, 4
    cond = torch.tensor([1, 2, 3, 4, 5])
    kw = dict(precision=precision, seed=51, top_k=(2048, 100), temperature=(0.95, 0.8))
    for graph in (False, True):
        plain = eng.sample(B, cond, n, use_graph=graph, **kw)
        a = eng.sample(B, cond, n, use_graph=graph, return_logprobs=True, **kw)
        b = eng.sample(B, cond, n, use_graph=graph, return_logprobs=True, **kw)
        again = eng.sample(B, cond, n, use_graph=graph, **kw)
        eng.range_check()
        torch.cuda.synchronize()
        assert len(plain) == 2 and len(a) == 3 and len(again) == 2
        for x in (a, b, again):
            assert torch.equal(x[0], plain[0]) and torch.equal(x[1], plain[1]), f'precision {precision} graph={graph}: the codes moved'
        assert torch.equal(a[2], b[2]), 'two identical calls must return the same bits'
    for want_lp, count in ((False, 0), (True, 5 * n)):
        eng.timing_reset()
        eng.timing(True)
        out = eng.sample(B, cond, n, use_graph=False, return_logprobs=want_lp, **kw)
        torch.cuda.synchronize()
        rep = eng.timing_report()
        eng.timing(False)
        assert rep.get('code_logprob', (0,))[0] == count, {k: v[0] for k, v in rep.items()}
        assert torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])
        if precision == PRECISION_FAST:
            assert rep.get('persist_position', (0,))[0] == n, {k: v[0] for k, v in rep.items()}
        if want_lp:
            assert torch.equal(out[2], a[2]), 'eager under timing and graph replay must agree bit for bit'


def test_three_levels_launch_21_per_position():
    fx = load('g7_l3_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 4)
    B, n = 3, 3
    eng.timing(True)
    out = eng.sample3(B, torch.full((B,), 7), n, precision=PRECISION_EXACT, seed=52, use_graph=False, return_logprobs=True)
    torch.cuda.synchronize()
    rep = eng.timing_report()
    eng.timing(False)
    assert rep.get('code_logprob', (0,))[0] == 21 * n, {k: v[0] for k, v in rep.items()}
    assert torch.isfinite(out[-1]).all()


def test_the_staged_pointer_is_taken_once(g4):
    fx, spec, weights, eng = g4
    B, n = 4, 4
    cond = torch.tensor([7, 1, 2, 3])
    POISON = -12345.0
    buf = torch.full((B, n, 5), POISON, dtype=torch.float32, device=dev())
    _lib.check(eng.lib.hqt_set_logprob_out(eng.h, buf.data_ptr()))
    a = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61)               # takes the staged pointer
    torch.cuda.synchronize()
    assert (buf != POISON).all() and torch.isfinite(buf).all()
    want = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61, return_logprobs=True)
    torch.cuda.synchronize()
    assert torch.equal(buf, want[2]) and torch.equal(a[0], want[0])
    buf.fill_(POISON)
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61)                   # nothing staged: nothing written
    torch.cuda.synchronize()
    assert (buf == POISON).all(), 'a call without a staged pointer wrote log-probabilities'
    # NULL clears; a refused call takes the pointer with it; a lane has its own
    _lib.check(eng.lib.hqt_set_logprob_out(eng.h, buf.data_ptr()))
    _lib.check(eng.lib.hqt_set_logprob_out(eng.h, None))
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61)
    _lib.check(eng.lib.hqt_set_logprob_out(eng.h, buf.data_ptr()))
    with pytest.raises(_lib.HqtError):
        eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61, temperature=(0.0, 1.0))
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61)
    lane = eng.clone()
    _lib.check(eng.lib.hqt_set_logprob_out(eng.h, buf.data_ptr()))
    lane.sample(B, cond, n, precision=PRECISION_EXACT, seed=61)
    torch.cuda.synchronize()
    assert (buf == POISON).all()
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=61)                   # ... and the root's stays for the root's next call
    torch.cuda.synchronize()
    assert torch.equal(buf, want[2])
    lane.close()


# ------------------------------------------------------------------------------- 7. merged pass
def test_merged_pass_gives_the_asking_step_its_rows(tiny_model):
    model = tiny_model
    B, n = 3, 64                                 # a merged pass decodes what it samples: all 64 positions of the tiny model's images
    pipe = InflightSampler(model, lanes=1, merge=2)
    kw = dict(max_seq_len=n, use_fp16=False, precision='exact', top_k_top=50, top_k_bot=20)
    p0 = pipe.submit(B, 5, seed=71, **kw)
    p1 = pipe.submit(B, 9, seed=72, sample_offset=64, return_logprobs=True, **kw)
    pipe.drain()
    torch.cuda.synchronize()
    r0, r1 = p0.get(), p1.get()
    assert len(r0) == 4 and isinstance(r0[3], torch.cuda.Event)                   # what it is today
    assert len(r1) == 5 and tuple(r1[4].shape) == (B, n, 5) and r1[4].dtype == torch.float32
    # the step's separate call with its own logits: the merged rows hold the log-softmax of those rows at the step's codes
    eng = model.stage2.engine(2 * B, n)
    ct, cb, lg, lp = eng.sample(B, torch.full((B,), 9), n, precision=PRECISION_EXACT, top_k=(50, 20), seed=72, sample_offset=64,
                                return_logits=True, return_logprobs=True)
    torch.cuda.synchronize()
    assert torch.equal(ct, r1[0]) and torch.equal(cb, r1[1])
    check_own((r1[0], r1[1], lg, r1[4]), 2, 'merged pass, asking step')
    print(f'merged rows vs the separate call: largest difference {(r1[4] - lp).abs().max().item():.3e}')


# ------------------------------------------------------------------------------- 8. sample_best_of
def test_best_of_keeps_what_a_host_argsort_picks(tiny_model):
    st2 = tiny_model.stage2
    G, C, K, n = 2, 6, 2, 8
    classes = torch.tensor([5, 9])
    kw = dict(use_fp16=False, max_seq_len=n, seed=81, top_k_top=100, top_k_bot=100, softmax_temperature=[1.0, 0.9])
    codes, scores = sample_best_of(st2, classes, C, K, **kw)
    # the same call, unranked (group-major rows: class g repeated C times)
    ct, cb, lp = sampling_ihqgpt(st2, num_candidates=G * C, cond=classes.repeat_interleave(C), is_tqdm=False, return_logprobs=True, **kw)
    torch.cuda.synchronize()
    sums = np_(lp).astype(np.float64).sum(axis=(1, 2)).reshape(G, C)
    order = np.argsort(-sums, axis=1, kind='stable')[:, :K]
    flat = (order + np.arange(G)[:, None] * C).reshape(-1)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (G, K)
    assert [tuple(c.shape) for c in codes] == [(G * K, n), (G * K, n, 4)]
    assert (np_(codes[0]) == np_(ct)[flat]).all() and (np_(codes[1]) == np_(cb)[flat]).all()
    got = np_(scores)
    assert (np.diff(got, axis=1) <= 0).all(), 'scores must come best first'
    assert np.abs(got - np.take_along_axis(sums, order, 1)).max() <= 1e-9
    assert len(set(sums.reshape(-1).tolist())) > 1, 'every candidate scored the same: the ranking shows nothing'
