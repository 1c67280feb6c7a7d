"""Completion from a code prefix on a text-conditional model: the prompt and the prefix are ONE causal body pass of ctx_len_txt + P rows per
sample (embed_text_kernel + embed_prefix_kernel behind it), position P is drawn from its last row, the rest are ordinary decode steps.  In
FAST precision at head size 64 that pass takes attention_prefill_tiled_kernel (one wave per 32-query tile, online softmax) from 65 rows on.

Bars: EXACT / SPLIT codes of every position >= P bit for bit -- against the reference's own text fixture and, for prefixes the model did not
draw, against the unchanged oracle by iteration (tests/prefix_ref.py) on seeds whose oracle-only margin is recorded below; logits of positions
P and P + 1 within the project's 2e-4; FAST teacher-forced logits inside the 0.15 gate test_causal_prefill_on_the_matrix_cores_vs_oracle holds
the same model to, on a NaN-poisoned workspace.  The fixture has 12 positions: of P in {1, 8, 31, 32, 33, 63} those <= 11 run."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O
from tests.helpers import gate, load, stage2_from_fixture
from tests.prefix_ref import oracle_complete, random_prefix_case

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
FAST_BAR = 0.15
PS = (1, 8, 31, 32, 33, 63)
HOOK = 'HQT_PREFILL_TILED'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_prefix, poison=False):
    if poison:                       # every workspace buffer starts as NaN: a row no kernel wrote shows up
        os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        e = Engine(spec, None, dev(), max_batch, spec.ctx_len_img, max_prefix=max_prefix)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    e.load(stage2=weights)
    e.finalize()
    return e


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------- 1. pinned to the reference's own output
def test_completion_of_the_text_fixture_prefix_is_the_fixture():
    """Prefix = the fixture's own codes of positions < P: the prefix comes back verbatim, every code of positions >= P equals the fixture's,
    eager and graph, and the logits of positions P and P + 1 are within 2e-4 of the fixture's where it kept them, of the oracle's
    teacher-forced logits and of this engine's own free run -- which is first shown to be the fixture."""
    fx = load('g3_tiny_txt.npz')
    spec, weights = stage2_from_fixture(fx)
    B, n = int(fx['B']), int(fx['n_steps'])
    noise = synth.exp_noise(int(fx['noise_seed']), n, B, spec.vocab_top)
    txt = synth.text_ids(int(fx['text_seed']), B, spec.ctx_len_txt, spec.vocab_txt)
    codes = [fx['codes_top'], fx['codes_bot']]
    kept = {int(s): fx['logits'][i] for i, s in enumerate(fx['keep_steps'])}
    kw = dict(precision=PRECISION_EXACT, noise=t_(noise), return_logits=True)
    ft, fb, free_lg = engine_s2(spec, weights, B, max_prefix=0).sample(B, t_(txt), n, use_graph=False, **kw)
    assert (np_(ft) == codes[0]).all() and (np_(fb) == codes[1]).all()         # the premise, restated: the free run is the fixture
    free_lg = np_(free_lg)
    orc_lg = O.OracleStage2(spec, weights).sample(txt, B, n, noise, force_top=codes[0].copy(), force_bot=codes[1].copy(), return_logits=True)[2]
    # the prefix calls get a NaN-poisoned engine to themselves, shortest prefix first: every longer prefill reaches rows nothing wrote before
    eng = engine_s2(spec, weights, B, max_prefix=n - 1, poison=True)
    ran = []
    for P in [P for P in PS if P <= n - 1]:
        prefix = [t_(c[:, :P]) for c in codes]
        for graph in (False, True):
            ct, cb, lg = eng.sample(B, t_(txt), n, use_graph=graph, prefix=prefix, **kw)
            torch.cuda.synchronize()
            for l, (g, c) in enumerate(zip((ct, cb), codes)):
                assert (np_(g)[:, :P] == c[:, :P]).all(), f'P={P} level {l}: the prefix did not come back verbatim'
                assert (np_(g)[:, P:] == c[:, P:]).all(), f'P={P} graph={graph} level {l}: completion differs from the reference'
            lg = np_(lg)
            assert np.isfinite(lg[P:]).all()
            for p in (P, P + 1):
                if p >= n:
                    continue
                if p in kept:
                    err = np.abs(lg[p] - kept[p]).max()
                    assert err <= LOGIT_TOL, f'P={P} position {p}: {err} from the fixture'
                for what, ref in (('the oracle', orc_lg), ('the free run', free_lg)):
                    err = np.abs(lg[p] - ref[p]).max()
                    print(f'P={P} graph={graph} position {p}: {err} from {what}')
                    assert err <= LOGIT_TOL, f'P={P} position {p}: {err} from {what}'
        ran.append(P)
    assert ran == [1, 8]


# ------------------------------------------------------------------------------- 2. a prefix the model did not draw itself
# (spec key, B, n, P, seed): seeds picked on the CPU with the oracle alone (tests/prefix_ref.py: oracle_complete; text ids synth.text_ids(seed)); the
# margin is the oracle's smallest winner / runner-up ratio of p / q over ALL compared draws, recorded here and asserted: >= 1.00009, so no
# position is excluded.
RANDOM_CASES = {'tiny': ('tiny', 5, 12, 6, 700, 1.0043059587478638),
                'head-2': ('head', 2, 6, 3, 800, 1.0541102886199951),
                'head-17': ('head', 17, 6, 3, 800, 1.0064095258712769)}
TINY_SET = ((50, 20), (None, 0.9), (1.0, 0.8))
HEAD_SET = ((None, 64), (None, 0.9), (1.0, 0.9))


def _random_spec(kind):
    if kind == 'tiny':
        return stage2_from_fixture(load('g3_tiny_txt.npz')) + (TINY_SET,)
    spec = Stage2Spec(embed_dim=1536, n_layers=1, n_heads=24, n_layers_depth=1, vocab_top=512, vocab_bot=512, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=0, cond=2, embedding=0)          # the ImageNet head geometry, text-conditional
    return spec, synth.stage2_weights(spec, 91, 'fixture'), HEAD_SET


@pytest.mark.parametrize('case', sorted(RANDOM_CASES))
def test_completion_of_a_random_prefix_to_a_prompt_vs_oracle(case):
    kind, B, n, P, seed, recorded = RANDOM_CASES[case]
    spec, weights, (tk, tp, T) = _random_spec(kind)
    _, prefix, noise = random_prefix_case(spec, B, n, P, seed)
    txt = synth.text_ids(seed, B, spec.ctx_len_txt, spec.vocab_txt)
    wt, wb, wl, margin = oracle_complete(O.OracleStage2(spec, weights), txt, B, n, noise, P, prefix, tk, tp, T)
    print(f'{case}: oracle margin {margin!r} (recorded {recorded!r})')
    assert margin >= 1.00009 and abs(margin - recorded) <= 1e-6 * recorded
    eng = engine_s2(spec, weights, B, max_prefix=P, poison=True)
    for prec in (PRECISION_EXACT, PRECISION_SPLIT):
        for graph in (False, True):
            ct, cb, lg = eng.sample(B, t_(txt), n, precision=prec, top_k=tk, top_p=tp, temperature=T, noise=t_(noise), return_logits=True,
                                    use_graph=graph, prefix=[t_(prefix[0]), t_(prefix[1])])
            eng.range_check()
            assert (np_(ct) == wt).all() and (np_(cb) == wb).all(), f'precision {prec} graph={graph}: codes differ from the oracle'
            err = np.abs(np_(lg)[P:] - wl[P:]).max()
            print(f'{case}: precision {prec} graph={graph} logit error {err}')
            assert err <= LOGIT_TOL


# ------------------------------------------------------------------------------- 3. FAST: the tiled kernel
def _mfma_spec(T):
    """test_causal_prefill_on_the_matrix_cores_vs_oracle's model: head size 64, two body layers (a wrong attention row anywhere changes the logits)."""
    spec = Stage2Spec(embed_dim=128, n_layers=2, n_heads=2, n_layers_depth=1, vocab_top=256, vocab_bot=256, vocab_txt=512,
                      ctx_len_img=64, ctx_len_txt=T, n_classes=0, cond=2, embedding=0)
    return spec, synth.stage2_weights(spec, 501 + T, 'fixture')


@pytest.mark.parametrize('T,P', [(64, 1), (64, 32), (64, 33), (64, 63), (16, 20)])
def test_fast_prompt_and_prefix_prefill_teacher_forced_vs_oracle(T, P):
    """T + P = 65 (the first row of the third tile), 96 (a full third tile), 97 (the first row of the fourth), 127 (the longest with T = 64) rows
    per sample through attention_prefill_tiled_kernel, and 36 rows through attention_prefill_mfma_kernel with the new row stride; B = 5, so the
    last workgroup has idle waves.  Teacher-forced on the oracle's codes, on a poisoned workspace; logits of positions P and P + 1 finite and
    inside the 0.15 the project already holds this model to (set at about twice its measured value, not derived anew); two graph runs bit-identical.
    HQT_RECORD_GATES=profiles/text_prefix_fast_gates.txt records the measured values."""
    spec, weights = _mfma_spec(T)
    B, n = 5, min(P + 2, 64)
    _, prefix, noise = random_prefix_case(spec, B, n, P, 900 + T + P)
    txt = synth.text_ids(903, B, T, spec.vocab_txt)
    rng = np.random.default_rng(T + P)
    ft = np.concatenate([prefix[0], rng.integers(0, spec.vocab_top, (B, n - P))], axis=1)
    fb = np.concatenate([prefix[1], rng.integers(0, spec.vocab_top, (B, n - P, 4))], axis=1)
    want = O.OracleStage2(spec, weights).sample(txt, B, n, noise, force_top=ft, force_bot=fb, return_logits=True)[2]
    eng = engine_s2(spec, weights, B, max_prefix=P, poison=True)
    runs = []
    for graph in (False, True, True):
        _, _, lf = eng.sample(B, t_(txt), n, precision=PRECISION_FAST, noise=t_(noise), force_top=t_(ft), force_bot=t_(fb), return_logits=True,
                              use_graph=graph, prefix=[t_(prefix[0]), t_(prefix[1])])
        eng.range_check()
        assert bool(torch.isfinite(lf[P:P + 2]).all())
        gate(f'text_prefix.fast_logits(T={T},P={P},graph={graph})', np.abs(np_(lf)[P:P + 2] - want[P:P + 2]).max(), FAST_BAR)
        runs.append(lf)
    assert torch.equal(runs[1], runs[2]), 'two graph runs differ'


# ------------------------------------------------------------------------------- 4. the tiled kernel against the one-wave kernel
@pytest.mark.parametrize('T', [20, 32, 33, 48, 64])
def test_tiled_prefill_against_the_one_wave_prefill(T):
    """The text prefill without a prefix (4 < T <= 64: attention_prefill_mfma_kernel by default) once more through the tiled kernel, with the
    per-launch hook HQT_PREFILL_TILED, on one engine in one process: each path inside the 0.15 gate against the oracle; the difference between
    the two is printed.  Without the hook a second call is bit-identical to the first: the default dispatch does not depend on the hook's history."""
    assert HOOK not in os.environ
    spec, weights = _mfma_spec(T)
    B, n = 5, 3
    noise = synth.exp_noise(502, n, B, spec.vocab_top)
    txt = synth.text_ids(503, B, T, spec.vocab_txt)
    want = O.OracleStage2(spec, weights).sample(txt, B, n, noise, return_logits=True)
    eng = engine_s2(spec, weights, B, max_prefix=0, poison=True)
    kw = dict(precision=PRECISION_FAST, noise=t_(noise), force_top=t_(want[0]), force_bot=t_(want[1]), return_logits=True)

    def run():
        lf = eng.sample(B, t_(txt), n, **kw)[2]
        eng.range_check()
        assert bool(torch.isfinite(lf).all())
        return lf
    first, second = run(), run()
    assert torch.equal(first, second)
    os.environ[HOOK] = '1'
    try:
        tiled = run()
    finally:
        del os.environ[HOOK]
    assert torch.equal(run(), first), 'the default dispatch changed after the hook was used'
    gate(f'text_prefix.one_wave_logits(T={T})', np.abs(np_(first) - want[2]).max(), FAST_BAR)
    gate(f'text_prefix.tiled_logits(T={T})', np.abs(np_(tiled) - want[2]).max(), FAST_BAR)
    print(f'T={T}: largest logit difference tiled vs one-wave prefill {float((tiled - first).abs().max())}')


# ------------------------------------------------------------------------------- 5. surface
def _tiny_model():
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-txt.yaml')), seed=5).to(dev())


def test_complete_images_to_a_prompt_keeps_the_rows_and_decodes_its_codes():
    from hqtransformer_amd.pipeline import complete_images, decode_codes
    from hqtransformer_amd.sampling import rearrange_levels
    model = _tiny_model()
    spec = model.stage2.spec
    R = model.stage1.spec.resolution
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 3, R, R)).astype(np.float32)).to(dev())
    txt = t_(synth.text_ids(4, 3, spec.ctx_len_txt, spec.vocab_txt))
    grids = model.stage1.code_grids(x)
    K = int(grids[0].shape[-1])
    for keep in (1, K - 1):
        px, codes = complete_images(model, x, keep, cond=txt, seed=11, use_fp16=False, top_k_top=50, top_k_bot=50)
        model.stage1.range_check()
        assert px.shape == (3, 3, R, R) and float(px.min()) >= 0.0 and float(px.max()) <= 1.0
        for l, (g, own) in enumerate(zip(rearrange_levels(codes, K), grids)):
            assert torch.equal(g[:, :keep << l], own[:, :keep << l]), f'level {l}: kept rows differ from get_codes'
            assert g.shape == own.shape
        assert torch.equal(px, decode_codes(model.stage1, codes))


def test_txt2img_driver_option_writes_the_usual_files(tmp_path):
    from hqtransformer_amd import sampling_hqmodel_txt2img
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.spec import stage1_spec_from_config, stage2_spec_from_config
    cfg_path = os.path.join(ROOT, 'configs', 'tiny-txt.yaml')
    cfg = load_config(cfg_path)
    R, K = stage1_spec_from_config(cfg).resolution, int(round(stage2_spec_from_config(cfg).ctx_len_img ** 0.5))
    src = tmp_path / 'images.npy'
    np.save(src, np.random.default_rng(1).uniform(0, 1, (2, 3, R, R)).astype(np.float32))
    out = tmp_path / 'out'
    sampling_hqmodel_txt2img.main(['-r', str(out), '-m', cfg_path, '--batch_size', '2', '--synthetic-prompts', '3', '--top-k', '64',
                                   '--top-resolution', str(K), '--complete-from', str(src), '--keep-rows', '2'])
    for batch, rows in ((1, 2), (2, 1)):                 # three prompts: a batch of two and the shorter last one
        with open(out / f'samples_({batch}_2).pkl', 'rb') as fp:
            px = pickle.load(fp)
        assert px.dtype == np.float32 and px.shape == (rows, 3, R, R) and px.min() >= 0.0 and px.max() <= 1.0
    with pytest.raises(SystemExit):
        sampling_hqmodel_txt2img.main(['-r', str(out), '-m', cfg_path, '--synthetic-prompts', '3', '--complete-from', str(src)])


@pytest.fixture(scope='module')
def tiny_txt():
    fx = load('g3_tiny_txt.npz')
    spec, weights = stage2_from_fixture(fx)
    return spec, weights, engine_s2(spec, weights, 8, max_prefix=20)


def test_a_text_handle_without_max_prefix_allocates_what_it_did_and_refuses_a_prefix(tiny_txt):
    spec, weights, eng = tiny_txt
    plain = Engine(spec, None, dev(), 8, spec.ctx_len_img)
    again = Engine(spec, None, dev(), 8, spec.ctx_len_img, max_prefix=0)
    big = Engine(spec, None, dev(), 8, spec.ctx_len_img, max_prefix=20)
    assert plain.max_prefix == 0 and again.workspace_bytes() == plain.workspace_bytes() < big.workspace_bytes()
    print(f'workspace bytes: max_prefix 0 -> {plain.workspace_bytes()}, 20 -> {big.workspace_bytes()}')
    assert big.lib.hqt_set_max_prefix(big.h, 0) == 0 and big.workspace_bytes() == plain.workspace_bytes()       # and back: nothing is left behind
    plain.load(stage2=weights)
    plain.finalize()
    txt = torch.zeros((2, spec.ctx_len_txt), dtype=torch.int64)
    prefix = [torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 4, 4), dtype=torch.int64)]
    with pytest.raises(ValueError, match='max_prefix=0'):
        plain.sample(2, txt, 16, prefix=prefix)
    # the library's own refusals
    o = _lib.hqt_sample_opts()
    o.precision, o.n_steps, o.temperature_top, o.temperature_bot = PRECISION_EXACT, 16, 1.0, 1.0
    cond = txt.to(dev())
    pt, pb = prefix[0].to(dev()), prefix[1].to(dev())
    ot, ob = torch.zeros((2, 16), dtype=torch.int64, device=dev()), torch.zeros((2, 16, 4), dtype=torch.int64, device=dev())

    def call(e, P):
        return e.lib.hqt_sample_prefix(e.h, 2, cond.data_ptr(), C.byref(o), None, P, pt.data_ptr(), pb.data_ptr(), None, None, None, ot.data_ptr(), ob.data_ptr(), None)
    assert call(plain, 4) == -1 and b'hqt_set_max_prefix' in plain.lib.hqt_last_error()
    assert call(eng, 4) == 0
    torch.cuda.synchronize()
    # one pass holds at most 16384 rows: 1024 * (16 + 1) is refused, 1024 * 16 without a prefix is what it was
    wide = Engine(spec, None, dev(), 1024, spec.ctx_len_img)
    assert wide.lib.hqt_set_max_prefix(wide.h, 1) == -1 and b'16384' in wide.lib.hqt_last_error()


def test_philox_shards_with_a_prefix_on_a_text_model(tiny_txt):
    spec, weights, eng = tiny_txt
    n, P = 24, 9
    txt = t_(synth.text_ids(21, 5, spec.ctx_len_txt, spec.vocab_txt))
    rng = np.random.default_rng(77)
    prefix = [t_(rng.integers(0, spec.vocab_top, (5, P))), t_(rng.integers(0, spec.vocab_top, (5, P, 4)))]
    kw = dict(precision=PRECISION_EXACT, seed=4321, top_k=(100, 60))
    full = eng.sample(5, txt, n, prefix=prefix, **kw)
    a = eng.sample(3, txt[:3], n, prefix=[p[:3] for p in prefix], **kw)
    b = eng.sample(2, txt[3:], n, prefix=[p[3:] for p in prefix], sample_offset=3, **kw)
    for l in range(2):
        assert torch.equal(full[l], torch.cat([a[l], b[l]])), 'ragged 3 + 2 rows differ from 5'
        assert torch.equal(full[l][:, :P], prefix[l].to(full[l].device))
    # the same keys as a free run: teacher-forcing the whole completed sequence through the free entry point redraws it
    redo = eng.sample(5, txt, n, force_top=full[0], force_bot=full[1], **kw)
    assert torch.equal(redo[0][:, P:], full[0][:, P:]) and torch.equal(redo[1][:, P:], full[1][:, P:])
