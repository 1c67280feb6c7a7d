"""One-pass scoring on the GPU (hqt_score, Engine.score, score_codes(one_pass=True), ImageGPT2.forward, score_images).

Tolerances.  |d logprob| <= |d l_code| + |d lse| <= 2 max|d l|: with the project's EXACT logit gate of 2e-4 against reference fixtures the
log-probability bound is 4e-4 (score_ref.LOGPROB_TOL), the logits bound 2e-4.  One pass against the stepwise path, both EXACT: each side is within
4e-4 of exact arithmetic, so 8e-4.  FAST: see test_fast_on_a_poisoned_workspace."""
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import HQTransformerStage2
from hqtransformer_amd.pipeline import score_codes, score_images, sequence_logprob
from hqtransformer_amd.sampling import global_to_sequence_index
from hqtransformer_amd.spec import Stage2Spec
from tests.helpers import gate
from tests.score_ref import G15, LOGIT_TOL, LOGPROB_TOL, g15

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# largest |logprob - G15 logprob| of the stepwise FAST score_codes (the only way before hqt_score; its launch sequence is unchanged) on the fixture's own
# B = 2, n = 64: profiles/score_fast_gates.txt.  The FAST one-pass gate is twice that, the project's usual margin: its GEMMs are other tile kernels
# that reorder the bf16 accumulations.
STEPWISE_FAST_ERR = {'tiny_cls': 0.0591, 'tiny_txt': 0.0643}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def make_engine(spec, weights, max_batch, max_prefix, score_chunk=0, poison=False, **kw):
    if poison:                       # every workspace buffer starts as NaN: a row no kernel wrote shows up
        os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        e = Engine(spec, None, dev(), max_batch, spec.ctx_len_img, max_prefix=max_prefix, score_chunk=score_chunk, **kw)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    e.load(stage2=weights)
    e.finalize()
    return e


_CASES, _ENGINES = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = g15(name)
    return _CASES[name]


def fixture_engine(name, chunk):
    """One engine per (fixture, chunk), shared by the tests of this module: max_batch = 2, so the default chunk is 2 pairs (64 chunks of the 128)."""
    if (name, chunk) not in _ENGINES:
        fx, spec, weights, cond, codes = case(name)
        _ENGINES[(name, chunk)] = make_engine(spec, weights, 2, int(fx['n_steps']) - 1, chunk)
    return _ENGINES[(name, chunk)]


def score(eng, cond, codes, precision, return_logits=False):
    out = eng.score(int(codes[0].shape[0]), None if cond is None else t_(cond), [t_(c) for c in codes], precision=precision, return_logits=return_logits)
    eng.range_check()
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------- 1. the reference's forward
@pytest.mark.parametrize('chunk', [0, 48])         # 48: chunks of 48 + 48 + 32 pairs -- a ragged last one, and one that straddles the sample boundary (the text row map)
@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT])
@pytest.mark.parametrize('name', G15)
def test_fixture_logprobs_and_logits(name, precision, chunk):
    fx, spec, weights, cond, codes = case(name)
    lp, logits = score(fixture_engine(name, chunk), cond, codes, precision, return_logits=True)
    keep = fx['keep_steps']
    err = np.abs(np_(lp) - fx['logprob']).max()
    errs = [np.abs(np_(logits[0]) - fx['logits_top']).max()] + [np.abs(np_(logits[l])[:, keep] - fx[f'logits{l}']).max() for l in range(1, spec.levels)]
    print(f'{name} precision {precision} chunk {chunk}: logprob error {err:.2e} (bound {LOGPROB_TOL}), logits errors {[f"{e:.2e}" for e in errs]} (bound {LOGIT_TOL})')
    assert np.isfinite(np_(lp)).all() and np_(lp).shape == fx['logprob'].shape
    assert err <= LOGPROB_TOL
    assert max(errs) <= LOGIT_TOL


# ------------------------------------------------------------------------------- 2. chunk invariance
@pytest.mark.parametrize('name', G15)
def test_exact_logprobs_do_not_depend_on_the_chunk(name):
    """EXACT: k-ordered GEMM chains at every row count, LayerNorm and attention per row -- chunks of 2, 48 and 128 pairs give the same bits."""
    fx, spec, weights, cond, codes = case(name)
    got = [score(fixture_engine(name, chunk), cond, codes, PRECISION_EXACT, return_logits=True) for chunk in (0, 48, 128)]
    for lp, logits in got[1:]:
        assert torch.equal(lp, got[0][0])
        assert all(torch.equal(a, b) for a, b in zip(logits, got[0][1]))


# ------------------------------------------------------------------------------- 3. short and odd shapes
def stepwise(eng, cond, codes, precision):
    B, n = codes[0].shape
    force = [t_(c) for c in codes]
    out = (eng.sample3(B, t_(cond), n, force=force, precision=precision, seed=0, return_logprobs=True) if len(codes) == 3 else
           eng.sample(B, t_(cond), n, force_top=force[0], force_bot=force[1], precision=precision, seed=0, return_logprobs=True))
    eng.range_check()
    torch.cuda.synchronize()
    return out[-1]


@pytest.mark.parametrize('n', [5, 1])
def test_short_sequences_equal_the_stepwise_score(n):
    fx, spec, weights, _, _ = case('tiny_cls')
    eng = make_engine(spec, weights, 3, 4)           # max_steps = ctx_len_img = 64; n = 1 would need no prefix room
    rng = np.random.default_rng(70 + n)
    B = 3
    codes = [rng.integers(0, spec.vocab_top, (B, n)), rng.integers(0, spec.vocab_top, (B, n, 4))]
    cond = np.array([7, 1, 9])
    one = np_(score(eng, cond, codes, PRECISION_EXACT))
    step = np_(stepwise(eng, cond, codes, PRECISION_EXACT))
    err = np.abs(one - step).max()
    print(f'B=3 n={n}: one pass vs stepwise, EXACT: {err:.2e}')
    assert one.shape == (B, n, 5) and np.isfinite(one).all() and err <= 2 * LOGPROB_TOL


def test_a_vocabulary_with_a_tail_equals_the_stepwise_score():
    """V = 516: 129 float4 groups, a tail inside the first round of the 256 threads (the model of tests/test_gpu_logprobs.py::synth_engine)."""
    V, B, n = 516, 3, 8
    spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=V, vocab_bot=V, vocab_txt=64,
                      ctx_len_img=16, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    eng = make_engine(spec, synth.stage2_weights(spec, 51, 'fixture'), 8, n - 1, 5)      # chunks of 5 pairs: 24 = 4 x 5 + 4
    rng = np.random.default_rng(71)
    codes = [rng.integers(0, V, (B, n)), rng.integers(0, V, (B, n, 4))]
    codes[0][0, 0], codes[1][0, 0, 0] = V - 1, V - 1                                       # the last code of the tail group
    cond = np.array([0, 4, 9])
    one = np_(score(eng, cond, codes, PRECISION_EXACT))
    step = np_(stepwise(eng, cond, codes, PRECISION_EXACT))
    err = np.abs(one - step).max()
    print(f'V=516 B=3 n=8: one pass vs stepwise, EXACT: {err:.2e}')
    assert np.isfinite(one).all() and err <= 2 * LOGPROB_TOL


# ------------------------------------------------------------------------------- 4. bidirectional, through the Python surface
def stage2_model(spec, weights):
    st2 = HQTransformerStage2(spec)
    st2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    return st2.to('cuda')


def test_one_pass_scores_the_bidirectional_head_and_stepwise_still_refuses():
    fx, spec, weights, cond, codes = case('tiny_cls_bidirectional')
    st2 = stage2_model(spec, weights)
    with pytest.raises(ValueError, match='bidirectional'):
        score_codes(st2, [t_(c) for c in codes], t_(cond), precision='exact')
    lp = score_codes(st2, [t_(c) for c in codes], t_(cond), precision='exact', one_pass=True, score_chunk=48)
    st2.range_check()
    assert st2.engine(2, 64).max_prefix == 63 and st2.engine(2, 64).score_chunk == 48
    err = np.abs(np_(lp) - fx['logprob']).max()
    print(f'bidirectional through score_codes(one_pass=True): {err:.2e}')
    assert err <= LOGPROB_TOL
    nll = -sequence_logprob(lp)
    assert nll.dtype == torch.float64 and np.allclose(np_(nll), -fx['logprob'].astype(np.float64).sum((1, 2)), atol=64 * 5 * LOGPROB_TOL)


# ------------------------------------------------------------------------------- 5. FAST
@pytest.mark.parametrize('name', ['tiny_cls', 'tiny_txt'])
def test_fast_on_a_poisoned_workspace(name):
    """B = 3 on a NaN-poisoned workspace: row counts that are no multiple of 32 (text: 16 + 63 = 79 rows per sample, the tiled prefill attention);
    every value finite, and the error against the EXACT one-pass values within twice what the stepwise FAST path shows against the reference."""
    fx, spec, weights, cond, codes = case(name)
    pick = [0, 1, 0]
    cond3, codes3 = cond[pick], [c[pick] for c in codes]
    if spec.cond == 1:
        cond3 = np.array([7, 2, 5])
    eng = make_engine(spec, weights, 3, 63, 40, poison=True)          # chunks of 40 pairs: 192 = 4 x 40 + 32
    exact = np_(score(eng, cond3, codes3, PRECISION_EXACT))
    fast, logits = score(eng, cond3, codes3, PRECISION_FAST, return_logits=True)
    fast = np_(fast)
    assert np.isfinite(exact).all() and np.isfinite(fast).all() and all(bool(torch.isfinite(l).all()) for l in logits)
    err = np.abs(fast - exact).max()
    print(f'{name}: FAST one pass vs EXACT one pass: {err:.4f}; stepwise FAST vs the reference: {STEPWISE_FAST_ERR[name]}')
    gate(f'score.fast_logprob({name},B=3,n=64,chunk=40)', err, 2.0 * STEPWISE_FAST_ERR[name])
    assert torch.equal(t_(fast), score(eng, cond3, codes3, PRECISION_FAST).cpu()), 'two identical calls must return the same bits'


# ------------------------------------------------------------------------------- 6. state
def test_sampling_is_unmoved_by_a_score_and_lanes_agree():
    fx, spec, weights, cond, codes = case('tiny_cls')
    eng = fixture_engine('tiny_cls', 48)
    B, n = 2, 64
    kw = dict(precision=PRECISION_FAST, seed=17, top_k=(50, 50), use_graph=True, return_logprobs=True)
    before = eng.sample(B, t_(cond), n, **kw)
    lp0 = score(eng, cond, codes, PRECISION_EXACT)
    after = eng.sample(B, t_(cond), n, **kw)
    eng.range_check()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, after)), 'a graphed sampling call drew other codes after hqt_score'
    lane = eng.clone()
    assert lane.score_chunk == 48
    assert torch.equal(score(lane, cond, codes, PRECISION_EXACT), lp0), 'lane 1 scores other bits than lane 0'


@pytest.mark.parametrize('name,chunk,chunks', [('tiny_cls', 48, 3), ('l3_tiny_cls', 0, 64), ('tiny_cls_bidirectional', 48, 3)])
def test_timing_counts_one_logprob_launch_per_chunk_and_sub_step(name, chunk, chunks):
    fx, spec, weights, cond, codes = case(name)
    eng = fixture_engine(name, chunk)
    eng.timing_reset()
    eng.timing(True)
    lp = score(eng, cond, codes, PRECISION_EXACT)
    rep = eng.timing_report()
    eng.timing(False)
    counts = {k: v[0] for k, v in rep.items() if not k.startswith('variant:')}
    assert counts.get('score_logprob') == chunks * spec.levels, counts
    assert counts.get('score_depth_input') == chunks and 'sampler' not in counts and 'code_logprob' not in counts, counts
    assert torch.equal(lp, score(eng, cond, codes, PRECISION_EXACT)), 'eager under timing and without must agree bit for bit'


# ------------------------------------------------------------------------------- 7. refusals
def raw_score(eng, B, cond, codes, n, precision=PRECISION_EXACT, logprobs='alloc'):
    import ctypes as C
    lp = torch.empty((B, n, 21), dtype=torch.float32, device=dev()) if logprobs == 'alloc' else logprobs
    cs = [c.to(dev()) for c in codes]
    cp = (C.c_void_p * 3)(*[c.data_ptr() for c in cs])
    cond = None if cond is None else cond.to(dev())
    rc = eng.lib.hqt_score(eng.h, B, None if cond is None else cond.data_ptr(), cp, n, precision, None if lp is None else lp.data_ptr(), None, None)
    torch.cuda.synchronize()
    return rc, eng.lib.hqt_last_error().decode()


def test_refusals_name_their_cause():
    fx, spec, weights, cond, codes = case('tiny_cls')
    B, n = 2, 8
    top, bot = t_(codes[0][:, :n]), t_(codes[1][:, :n])
    c = t_(cond)
    small = make_engine(spec, weights, 2, 3)
    rc, msg = raw_score(small, B, c, [top, bot], n)
    assert rc == -3 and 'hqt_set_max_prefix' in msg and 'max_prefix >= 7' in msg, (rc, msg)
    rc, msg = raw_score(small, B, c, [top[:, :4], bot[:, :4]], 4, logprobs=None)
    assert rc == -1 and 'logprobs is NULL' in msg, (rc, msg)
    # a staged table / buffer belongs to a sampling call: cleared, refused, and the next call runs
    buf = torch.zeros((B, 4, 5), dtype=torch.float32, device=dev())
    _lib.check(small.lib.hqt_set_logprob_out(small.h, buf.data_ptr()))
    rc, msg = raw_score(small, B, c, [top[:, :4], bot[:, :4]], 4)
    assert rc == -3 and 'staged' in msg and 'hqt_set_logprob_out' in msg, (rc, msg)
    rc, msg = raw_score(small, B, c, [top[:, :4], bot[:, :4]], 4)
    assert rc == 0, (rc, msg)
    assert float(buf.abs().max()) == 0.0
    # pairs x Tdepth beyond one pass: 4097 x 4 rows
    e = Engine(spec, None, dev(), 2, spec.ctx_len_img)
    with pytest.raises(_lib.HqtError, match=r'4097 \* 4 exceeds the 16384 rows') as ei:
        _lib.check(e.lib.hqt_set_score_chunk(e.h, 4097))
    assert ei.value.code == -1
    _lib.check(e.lib.hqt_set_score_chunk(e.h, 4096))
    e.close()
    with pytest.raises(_lib.HqtError, match='between hqt_create and hqt_finalize_weights'):
        _lib.check(small.lib.hqt_set_score_chunk(small.h, 8))
    # a FAST-only replica: layout_check refuses what it refuses for hqt_sample (SPLIT); EXACT runs from the fp32 tensors as received, as it does there
    lean = make_engine(spec, weights, 2, n - 1, ar_layouts=_lib.LAYOUT_FAST)
    rc, msg = raw_score(lean, B, c, [top, bot], n, precision=PRECISION_SPLIT)
    assert rc == -3 and 'HQT_LAYOUT_SPLIT' in msg, (rc, msg)
    full = make_engine(spec, weights, 2, n - 1)
    assert torch.equal(score(lean, cond, [codes[0][:, :n], codes[1][:, :n]], PRECISION_EXACT), score(full, cond, [codes[0][:, :n], codes[1][:, :n]], PRECISION_EXACT))
    # heads and conditionings the one pass is not built for
    l3 = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=64, vocab_bot=64, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                    n_classes=10, cond=1, embedding=0, levels=3, depth_decoding='top2mid2bot')
    e = make_engine(l3, synth.stage2_weights(l3, 5, 'fixture'), 2, 3)
    z = [torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 4, 4), dtype=torch.int64), torch.zeros((2, 4, 16), dtype=torch.int64)]
    rc, msg = raw_score(e, 2, torch.zeros(2, dtype=torch.int64), z, 4)
    assert rc == -1 and 'top2mid2bot' in msg, (rc, msg)
    l3t = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=64, vocab_bot=64, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                     n_classes=0, cond=2, embedding=0, levels=3)
    e = make_engine(l3t, synth.stage2_weights(l3t, 5, 'fixture'), 2, 0)
    rc, msg = raw_score(e, 2, torch.zeros((2, 16), dtype=torch.int64), [t[:, :1] for t in z], 1)
    assert rc == -1 and 'text conditioning with three code levels' in msg, (rc, msg)


def test_without_a_chunk_the_workspace_is_what_it_was():
    fx, spec, weights, cond, codes = case('tiny_cls')
    plain = Engine(spec, None, dev(), 2, spec.ctx_len_img, max_prefix=63)
    small = Engine(spec, None, dev(), 2, spec.ctx_len_img, max_prefix=63, score_chunk=2)       # no more than max_batch pairs: nothing to grow
    big = Engine(spec, None, dev(), 2, spec.ctx_len_img, max_prefix=63, score_chunk=128)
    assert plain.workspace_bytes() == small.workspace_bytes() < big.workspace_bytes()
    for e in (plain, small, big):
        e.close()


# ------------------------------------------------------------------------------- 8. surface
def test_forward_returns_the_reference_layout():
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    fx, spec, weights, cond, codes = case('tiny_cls')
    model = ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5)
    model.stage2 = stage2_model(spec, weights)
    idx = global_to_sequence_index(64)
    bot = torch.empty((2, 256), dtype=torch.int64)
    bot[:, idx.reshape(-1)] = t_(codes[1]).reshape(2, -1)
    lt, lb = model((t_(codes[0]), bot), t_(cond))
    torch.cuda.synchronize()
    assert lt.shape == (2, 64, 512) and lb.shape == (2, 256, 512)
    keep = fx['keep_steps']
    seq = np_(lb)[:, idx.reshape(-1).numpy()].reshape(2, 64, 4, 512)
    errs = np.abs(np_(lt) - fx['logits_top']).max(), np.abs(seq[:, keep] - fx['logits1']).max()
    print(f'forward vs the reference: top {errs[0]:.2e}, bottom {errs[1]:.2e}')
    assert max(errs) <= LOGIT_TOL
    # the log-softmax of what forward returns, at the codes in ITS layout, is the fixture's logprob
    lsm = torch.log_softmax(lb.double(), -1).gather(2, bot.to(lb.device)[..., None])[..., 0]
    assert np.abs(np_(lsm)[:, idx.reshape(-1).numpy()].reshape(2, 64, 4) - fx['logprob'][:, :, 1:]).max() <= LOGPROB_TOL


def test_score_images_scores_the_codes_of_get_codes():
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import grids_to_sequences
    model = ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to(dev())
    R = model.stage1.spec.resolution
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 3, R, R)).astype(np.float32)).to(dev())
    score_, codes = score_images(model, x, 2, precision='exact', score_chunk=20)
    flat = model.stage1.get_codes(x)
    K = int(round(codes[0].shape[1] ** 0.5))
    want_codes = grids_to_sequences([f.reshape(3, K << l, K << l) for l, f in enumerate(flat)])
    assert all(torch.equal(a, b) for a, b in zip(codes, want_codes))
    want = sequence_logprob(score_codes(model.stage2, want_codes, 2, precision='exact', one_pass=True))
    model.stage2.range_check()
    assert score_.dtype == torch.float64 and score_.shape == (3,) and torch.equal(score_, want) and bool((score_ < 0).all())
