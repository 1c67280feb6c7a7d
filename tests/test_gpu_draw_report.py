"""The draw report on the GPU (hqt_set_draw_report, report_out= / return_report=): entropy, rank and top-N of the row behind every draw.

Reference: tests/draw_report_ref.py on fp32 rows that are upstream of the kernel under test -- rows injected through the heads (tests/sampler_rows.py: the
logits ARE the chosen row, bit for bit) or the call's own logits_out.  The order and the rank are integers and are compared exactly, with no case excluded; the
entropy is held to the derived gate of 2e-4 (draw_report_ref.ENTROPY_GATE); top_logprobs are pinned BIT FOR BIT to the log-probabilities of a second call that
feeds those codes forward with only hqt_set_logprob_out staged.

The row with -0.0 next to +0.0 cannot come out of a head: every term of a dot product is added to a +0.0 accumulator, and +0.0 + -0.0 is +0.0 (products
that underflow to -0.0 fare no better: tried on the device, the logits come back +0.0).  That row is therefore handed to the kernels themselves:
launch_score_report and launch_score_logprob of libhqt.so, the launchers hqt_score calls, on a tensor of rows (test_negative_zero_next_to_positive_zero).
score_report_kernel and draw_report_kernel share one body (report_row), which every other test here reaches through the sampling calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import DrawReport, Engine
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.pipeline import RollingSampler, SamplingSession, score_images, uncertainty_map
from hqtransformer_amd.sampling import sampling_ihqgpt
from tests import draw_report_ref as R
from tests import sampler_rows as SR
from tests.helpers import load, stage2_from_fixture
from tests.score_ref import LOGPROB_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, UNSET = float('nan'), -7                # what the buffers hold before a call: an entry nobody wrote keeps it


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return torch.from_numpy(np.array(a))


def engine_s2(spec, weights, max_batch, max_steps=None, max_prefix=0):
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # every workspace buffer starts as NaN: a row no kernel wrote shows up
    try:
        e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img, max_prefix=max_prefix)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    e.load(stage2=weights)
    e.finalize()
    return e


def buffers(B, n, draws, top_n, entropy=True, rank=True):
    """A DrawReport of sentinel-filled device tensors."""
    shp = (B, n, draws)
    return DrawReport(torch.full(shp, NAN, dtype=torch.float32, device=dev()) if entropy else None,
                      torch.full(shp, UNSET, dtype=torch.int32, device=dev()) if rank else None,
                      torch.full(shp + (top_n,), UNSET, dtype=torch.int32, device=dev()) if top_n else None,
                      torch.full(shp + (top_n,), NAN, dtype=torch.float32, device=dev()) if top_n else None)


def host(rep):
    return tuple(None if f is None else np_(f) for f in rep)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def same_report(a, b):
    return all((x is None and y is None) or same_bits(np_(x), np_(y)) for x, y in zip(a, b))


def all_codes(codes):
    B, n = codes[0].shape
    return np.concatenate([np_(c).reshape(B, n, -1) for c in codes], axis=2)


def untouched(rep, index):
    """The entries rep[...][index] still hold the sentinels."""
    return all(f is None or bool((torch.isnan(f[index]) if f.dtype == torch.float32 else f[index] == UNSET).all()) for f in rep)


def written(rep, index):
    return all(f is None or bool((torch.isfinite(f[index]) if f.dtype == torch.float32 else f[index] >= 0).all()) for f in rep)


# ------------------------------------------------------------------------------- 1. injected rows, EXACT
INJECTED = [(V, pair) for V in R.VOCABS for pair in R.PAIRS]


@pytest.mark.parametrize('V,pair', INJECTED, ids=[f'V{V}-{a}-{b}' for V, (a, b) in INJECTED])
def test_injected_rows_exact(V, pair):
    B, n, N = 3, 2, 16
    rows = [R.family_row(V, name) for name in pair]
    spec, base = SR.base_weights(V)
    eng = engine_s2(spec, SR.inject(base, *rows), B, n)
    try:
        cond = t_(SR.cond(B))
        rep = buffers(B, n, 5, N)
        ct, cb, lg, lp = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=5, return_logits=True, return_logprobs=True, report_out=rep, use_graph=False)
        eng.range_check()
        torch.cuda.synchronize()
        lg = np_(lg)
        assert same_bits(lg[:, 0], np.broadcast_to(rows[0], lg[:, 0].shape)), 'the top logits are not the injected row (sign bits included)'
        assert same_bits(lg[:, 1:], np.broadcast_to(rows[1], lg[:, 1:].shape)), 'the bottom logits are not the injected row (sign bits included)'
        got = host(rep)
        codes = all_codes([ct, cb])
        R.check_rows(lg, codes, got, N, f'V={V} {pair}')
        for level, name in enumerate(pair):
            draws = slice(0, 1) if level == 0 else slice(1, 5)
            if name == 'const':
                assert (got[2][:, :, draws] == np.arange(N)).all() and (got[1][:, :, draws] == codes[:, :, draws]).all()
        inside = got[1] < N                         # where the code is among the top N its log-probability is that entry, bit for bit
        pick = np.take_along_axis(got[3], np.minimum(got[1], N - 1)[..., None], -1)[..., 0]
        assert (pick.view(np.uint32)[inside] == np_(lp).view(np.uint32)[inside]).all()
        for j in (0, N - 1):                        # a second call that feeds top_codes[j] forward, with only the log-probability buffer staged
            force_top = torch.from_numpy(got[2][:, :, 0, j].astype(np.int64))
            force_bot = torch.from_numpy(got[2][:, :, 1:, j].astype(np.int64))
            forced = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=5, force_top=force_top, force_bot=force_bot, return_logprobs=True, use_graph=False)
            torch.cuda.synchronize()
            assert same_bits(np_(forced[2]), got[3][..., j]), f'top_logprobs[..., {j}] are not the log-probabilities of the call that forces those codes'
    finally:
        eng.close()


def launcher(name, argtypes):
    """A C++ launcher of libhqt.so (csrc/kernels.h) by its name: the symbol is looked up in the library's dynamic table."""
    nm = subprocess.run(['nm', '-D', _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    found = re.findall(rf'\bT (_Z\d+{name}\S+)', nm)
    assert len(found) == 1, f'{name}: {found}'
    fn = getattr(_lib.load(), found[0])
    fn.restype, fn.argtypes = C.c_int, argtypes
    return fn


@pytest.mark.parametrize('V', R.VOCABS)
def test_negative_zero_next_to_positive_zero(V):
    """-0.0 and +0.0 tie and the lower index wins, in the order and in the rank; the kernels get the row directly (see the module text).  Two pairs of four slots
    at draws 1 .. 4 of pairs 1 and 2 of a [3, 5] report: what lies outside stays on the sentinel."""
    report = launcher('launch_score_report', [C.c_void_p, C.c_void_p, C.POINTER(_lib.hqt_draw_report)] + [C.c_int] * 6 + [C.c_void_p])
    logprob = launcher('launch_score_logprob', [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p])
    N, pair0, pairs, slots, draw0, draws = 16, 1, 2, 4, 1, 5
    row = R.zeros_row(V)
    zeros = np.flatnonzero(row == 0)
    assert np.signbit(row[zeros]).any() and not np.signbit(row[zeros]).all()
    logits = torch.from_numpy(np.broadcast_to(row, (pairs * slots, V)).copy()).to(dev())
    given = np.array([0, 1, int(zeros[-1]), int(zeros[-2]), 6, V - 3, 3, 2])[:pairs * slots]      # both zeros, first and last index, and entries below them
    codes = torch.from_numpy(given.astype(np.int64)).to(dev())
    rep = buffers(pair0 + pairs, 1, draws, N)
    r = _lib.hqt_draw_report()
    r.entropy, r.rank, r.top_n, r.top_codes, r.top_logprobs = rep.entropy.data_ptr(), rep.rank.data_ptr(), N, rep.top_codes.data_ptr(), rep.top_logprobs.data_ptr()
    stream = torch.cuda.current_stream(dev()).cuda_stream
    with torch.cuda.device(dev()):
        assert report(logits.data_ptr(), codes.data_ptr(), C.byref(r), pair0, pairs, V, slots, draw0, draws, stream) == 0
    torch.cuda.synchronize()
    assert untouched(rep, (0,)) and untouched(rep, (slice(None), slice(None), 0)) and written(rep, (slice(pair0, None), slice(None), slice(draw0, None)))
    got = tuple(f[pair0:, :, draw0:] for f in host(rep))                # [pairs, 1, slots(, N)]
    lg = np_(logits).reshape(pairs, slots, 1, V).transpose(2, 1, 0, 3)   # -> [n = 1, draws = slots, B = pairs, V]
    R.check_rows(lg, given.reshape(pairs, 1, slots), got, N, f'V={V}: -0.0 next to +0.0')
    want = sorted(zeros.tolist())[:N]
    assert (got[2][..., :len(want)] == np.array(want)).all(), 'the zeros of both signs come in index order'
    assert [int(v) for v in got[1].reshape(-1)[:4]] == [0, 1, len(zeros) - 1, len(zeros) - 2]
    for j in (0, N - 1):                         # the log-probability kernel at top_codes[j]: the same bits
        forced = torch.from_numpy(got[2][..., j].reshape(-1).astype(np.int64)).to(dev())
        lp = torch.full((pair0 + pairs, 1, draws), NAN, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            assert logprob(logits.data_ptr(), forced.data_ptr(), lp[pair0:].data_ptr(), pairs, V, slots, draw0, draws, stream) == 0
        torch.cuda.synchronize()
        assert same_bits(np_(lp[pair0:, :, draw0:]), got[3][..., j])


# ------------------------------------------------------------------------------- 2. FAST and SPLIT on the reference's tiny model
@pytest.fixture(scope='module')
def g4():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    return fx, spec, weights, engine_s2(spec, weights, 8, max_prefix=7)


CUT = dict(top_k=(50, 20), top_p=(0.9, 0.8), temperature=(0.7, 1.3))


@pytest.mark.parametrize('precision', [PRECISION_FAST, PRECISION_SPLIT], ids=['fast', 'split'])
def test_own_logits_fast_and_split(g4, precision):
    fx, spec, weights, eng = g4
    B, n, N = 4, 6, 16
    for graph in (False, True):
        rep = buffers(B, n, 5, N)
        ct, cb, lg = eng.sample(B, torch.tensor([7, 1, 2, 3]), n, precision=precision, seed=21, return_logits=True, report_out=rep, use_graph=graph, **CUT)
        eng.range_check()
        torch.cuda.synchronize()
        R.check_rows(np_(lg), all_codes([ct, cb]), host(rep), N, f'g4 precision {precision} graph={graph}')


# ------------------------------------------------------------------------------- 3. nothing changes for others
@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_FAST], ids=['exact', 'fast'])
def test_nothing_changes_for_others(g4, precision):
    fx, spec, weights, eng = g4
    B, n, N = 4, 5, 16
    cond = torch.tensor([7, 1, 2, 3])
    kw = dict(precision=precision, seed=33, **CUT)
    plain = eng.sample(B, cond, n, return_logprobs=True, **kw)
    reps = {}
    for graph in (False, True):
        rep = buffers(B, n, 5, N)
        both = eng.sample(B, cond, n, return_logprobs=True, report_out=rep, use_graph=graph, **kw)
        alone = buffers(B, n, 5, N)
        only = eng.sample(B, cond, n, report_out=alone, use_graph=graph, **kw)
        torch.cuda.synchronize()
        assert torch.equal(both[0], plain[0]) and torch.equal(both[1], plain[1]) and torch.equal(only[0], plain[0]) and torch.equal(only[1], plain[1]), 'the codes moved'
        assert same_bits(np_(both[2]), np_(plain[2])), 'the log-probabilities changed their bits next to a report'
        assert same_report(rep, alone)
        reps[graph] = rep
    assert same_report(reps[False], reps[True]), 'eager and graph replay must give the same report bits'
    # a subset of the fields: the others are simply not written
    part = buffers(B, n, 5, 0, entropy=False)
    eng.sample(B, cond, n, report_out=part, **kw)
    torch.cuda.synchronize()
    assert same_bits(np_(part.rank), np_(reps[True].rank))
    for staged, want in ((True, (5 * n, 0)), (False, (0, 0))):
        eng.timing_reset()
        eng.timing(True)
        out = eng.sample(B, cond, n, use_graph=False, return_logprobs=staged, report_out=buffers(B, n, 5, N) if staged else None, **kw)
        torch.cuda.synchronize()
        slots = eng.timing_report()
        eng.timing(False)
        counts = {k: v[0] for k, v in slots.items()}
        assert (counts.get('draw_report', 0), counts.get('code_logprob', 0)) == want, counts
        if not staged:
            assert 'draw_report' not in counts or counts['draw_report'] == 0
        assert torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])


# ------------------------------------------------------------------------------- 4. written only where it belongs
def test_a_prefix_call_leaves_the_prefix_positions_alone(g4):
    fx, spec, weights, eng = g4
    B, n, P, N = 3, 6, 2, 4
    cond = torch.tensor([7, 1, 2])
    kw = dict(precision=PRECISION_EXACT, seed=41, **CUT)
    full = buffers(B, n, 5, N)
    ct, cb = eng.sample(B, cond, n, report_out=full, **kw)
    rep = buffers(B, n, 5, N)
    pt, pb = eng.sample(B, cond, n, prefix=[ct[:, :P].clone(), cb[:, :P].clone()], report_out=rep, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pt, ct) and torch.equal(pb, cb)
    assert untouched(rep, (slice(None), slice(0, P))) and written(rep, (slice(None), slice(P, n)))
    assert all(same_bits(np_(a[:, P:]), np_(b[:, P:])) for a, b in zip(rep, full)), 'EXACT: the completion reports what the free run reports'


def test_a_rolling_call_writes_live_rows_only_and_a_staggered_request_equals_the_plain_call(g4):
    fx, spec, weights, eng = g4
    S, n, N = 3, 5, 16
    cls, seeds, offs = [3, 7, 1], [1001, 2002, 3003], [0, 11, 5]
    kw = dict(precision=PRECISION_EXACT, **CUT)
    # the plain call of the same batch: every slot's request in its slot
    want = buffers(S, n, 5, N)
    plain = eng.sample(S, torch.tensor(cls), n, row_seeds=seeds, row_offsets=offs, return_logprobs=True, report_out=want, **kw)
    torch.cuda.synchronize()
    codes = [torch.full((S, n), -1, dtype=torch.int64, device=dev()), torch.full((S, n, 4), -1, dtype=torch.int64, device=dev())]
    lp = torch.full((S, n, 5), NAN, dtype=torch.float32, device=dev())
    rep = buffers(S, n, 5, N)
    roll = dict(out=codes, logprobs_out=lp, report_out=rep, row_seeds=seeds, row_offsets=offs, **kw)
    # slot 0 joins alone and runs two positions; then slot 2 joins at 0 while slot 0 is mid-image and slot 1 stays empty
    eng.sample(S, torch.tensor(cls), n, row_positions=([0, -1, -1], 2), **roll)
    torch.cuda.synchronize()
    assert untouched(rep, (slice(1, 3),)) and untouched(rep, (0, slice(2, n))) and written(rep, (0, slice(0, 2)))
    eng.sample(S, torch.tensor(cls), n, row_positions=([2, -1, 0], 3), **roll)
    torch.cuda.synchronize()
    assert untouched(rep, (1,)), 'the idle slot was written'
    assert written(rep, (0,)) and written(rep, (2, slice(0, 3))) and untouched(rep, (2, slice(3, n)))
    eng.sample(S, torch.tensor(cls), n, row_positions=([-1, -1, 3], 2), **roll)
    torch.cuda.synchronize()
    assert untouched(rep, (1,)) and written(rep, (2,))
    for s in (0, 2):
        assert torch.equal(codes[0][s], plain[0][s]) and torch.equal(codes[1][s], plain[1][s]) and same_bits(np_(lp[s]), np_(plain[2][s]))
        assert all(same_bits(np_(a[s]), np_(b[s])) for a, b in zip(rep, want)), f'the staggered request in slot {s} reports other bits than the plain call'


# ------------------------------------------------------------------------------- 5. compositions
def test_a_guidance_pair_reports_the_guided_row_in_both_rows(g4):
    fx, spec, weights, eng = g4
    B, n, N = 4, 4, 16
    cond = torch.tensor([7, 1, 2, 3])
    rep = buffers(B, n, 5, N)
    ct, cb, lg, lp = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=51, guidance=[(0, 2, 2.5)], return_logits=True, return_logprobs=True,
                                report_out=rep, **CUT)
    torch.cuda.synchronize()
    assert torch.equal(ct[0], ct[2]) and torch.equal(cb[0], cb[2])
    assert all(same_bits(np_(f[0]), np_(f[2])) for f in rep), 'both rows of a pair carry the same report'
    assert same_bits(np_(lg[:, :, 0]), np_(lg[:, :, 2]))
    R.check_rows(np_(lg), all_codes([ct, cb]), host(rep), N, 'guided pair (0, 2) and two plain rows')


def test_a_keep_table(g4):
    fx, spec, weights, eng = g4
    B, n, N = 3, 6, 8
    cond = torch.tensor([7, 1, 2])
    rng = np.random.default_rng(52)
    kept = [t_(rng.integers(0, spec.vocab_top, (B, n))), t_(rng.integers(0, spec.vocab_top, (B, n, 4)))]
    mask = np.zeros((B, n), bool)
    mask[:, 0] = True                            # a leading run all rows share: the prefill, not reported (as with a prefix)
    mask[0, 2], mask[1, 3:5], mask[2, 5] = True, True, True
    rep = buffers(B, n, 5, N)
    ct, cb, lg, lp = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=53, keep=(t_(mask), kept), return_logits=True, return_logprobs=True, report_out=rep, **CUT)
    torch.cuda.synchronize()
    assert untouched(rep, (slice(None), 0)) and written(rep, (slice(None), slice(1, n)))
    sel = torch.from_numpy(mask)
    assert torch.equal(ct.cpu()[sel], kept[0][sel]) and torch.equal(cb.cpu()[sel], kept[1][sel])
    got = tuple(f[:, 1:] for f in host(rep))
    R.check_rows(np_(lg)[1:], all_codes([ct, cb])[:, 1:], got, N, 'keep table: kept positions are ranked at the kept code')
    inside = got[1] < N
    pick = np.take_along_axis(got[3], np.minimum(got[1], N - 1)[..., None], -1)[..., 0]
    assert (pick.view(np.uint32)[inside] == np_(lp)[:, 1:].view(np.uint32)[inside]).all()


@pytest.mark.parametrize('name,draws', [('g7_l3_tiny_cls.npz', 21), ('g13_tiny_cls_bidirectional.npz', 5)])
def test_three_levels_and_the_bidirectional_head(name, draws):
    fx = load(name)
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 3)
    B, n, N = 3, 3, 16
    cond = torch.tensor([7, 1, 2])
    rep = buffers(B, n, draws, N)
    kw = dict(precision=PRECISION_EXACT, seed=54, return_logits=True, return_logprobs=True, report_out=rep)
    out = eng.sample3(B, cond, n, **kw) if spec.levels == 3 else eng.sample(B, cond, n, **kw)
    eng.timing(True)
    again = buffers(B, n, draws, N)
    kw['report_out'] = again
    (eng.sample3 if spec.levels == 3 else eng.sample)(B, cond, n, use_graph=False, **kw)
    torch.cuda.synchronize()
    counts = {k: v[0] for k, v in eng.timing_report().items()}
    eng.timing(False)
    assert counts.get('draw_report', 0) == draws * n and counts.get('code_logprob', 0) == 0, counts
    assert same_report(rep, again)
    codes = all_codes(out[:spec.levels])
    got = host(rep)
    R.check_rows(np_(out[spec.levels]), codes, got, N, name)
    inside = got[1] < N
    pick = np.take_along_axis(got[3], np.minimum(got[1], N - 1)[..., None], -1)[..., 0]
    assert (pick.view(np.uint32)[inside] == np_(out[-1]).view(np.uint32)[inside]).all()
    eng.close()


def test_one_row(g4):
    fx, spec, weights, eng = g4
    n, N = 4, 16
    rep = buffers(1, n, 5, N)
    ct, cb, lg = eng.sample(1, torch.tensor([7]), n, precision=PRECISION_FAST, seed=55, return_logits=True, report_out=rep)
    eng.range_check()
    torch.cuda.synchronize()
    R.check_rows(np_(lg), all_codes([ct, cb]), host(rep), N, 'B = 1')


# ------------------------------------------------------------------------------- 6. hqt_score
def test_score_takes_a_staged_report(g4):
    fx, spec, weights, eng = g4
    B, n, N = 3, 8, 16
    V = spec.vocab_top
    rng = np.random.default_rng(61)
    codes = [t_(rng.integers(0, V, (B, n))), t_(rng.integers(0, V, (B, n, 4)))]
    cond = torch.tensor([7, 1, 9])
    rep = buffers(B, n, 5, N)
    lp, logits = eng.score(B, cond, codes, precision=PRECISION_EXACT, return_logits=True, report_out=rep)
    eng.range_check()
    torch.cuda.synchronize()
    lg = np.concatenate([np_(logits[0])[:, :, None], np_(logits[1])], axis=2).transpose(1, 2, 0, 3)        # [B, n, 5, V] -> [n, 5, B, V]
    got = host(rep)
    R.check_rows(lg, all_codes(codes), got, N, 'hqt_score, EXACT')
    inside = got[1] < N
    pick = np.take_along_axis(got[3], np.minimum(got[1], N - 1)[..., None], -1)[..., 0]
    assert (pick.view(np.uint32)[inside] == np_(lp).view(np.uint32)[inside]).all(), 'the report and score_logprob read one row with one arithmetic'
    assert same_bits(np_(lp), np_(eng.score(B, cond, codes, precision=PRECISION_EXACT))), 'the log-probabilities do not change next to a report'
    # against the stepwise forced sampling call.  Both sides are within the project's EXACT logit gate of exact arithmetic, so their rows differ by at most
    # d = 2 * 2e-4: a log-probability -- the largest one, top_logprobs[..., 0], too -- moves by at most 2 d = 2 * LOGPROB_TOL (tests/test_gpu_score.py); the
    # entropy H = -sum p log p by at most sum |dp| |log p| + sum p |dlog p| <= 2 d (H + 1) <= 2 d (1 + ln V).
    step = buffers(B, n, 5, N)
    slp = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=0, force_top=codes[0], force_bot=codes[1], return_logprobs=True, report_out=step)[-1]
    torch.cuda.synchronize()
    e_lp = np.abs(np_(lp) - np_(slp)).max()
    e_top = np.abs(got[3][..., 0] - np_(step.top_logprobs)[..., 0]).max()
    e_h = np.abs(got[0] - np_(step.entropy)).max()
    print(f'one pass vs stepwise: logprob {e_lp:.2e}, top logprob {e_top:.2e} (bound {2 * LOGPROB_TOL}), entropy {e_h:.2e} (bound {2 * LOGPROB_TOL * (1 + np.log(V)):.2e})')
    assert e_lp <= 2 * LOGPROB_TOL and e_top <= 2 * LOGPROB_TOL and e_h <= 2 * LOGPROB_TOL * (1 + np.log(V))
    # FAST, against its own logits
    rep = buffers(B, n, 5, N)
    lp, logits = eng.score(B, cond, codes, precision=PRECISION_FAST, return_logits=True, report_out=rep)
    torch.cuda.synchronize()
    lg = np.concatenate([np_(logits[0])[:, :, None], np_(logits[1])], axis=2).transpose(1, 2, 0, 3)
    R.check_rows(lg, all_codes(codes), host(rep), N, 'hqt_score, FAST')
    # what it refuses today stays refused, and takes the report with it
    rep = buffers(B, n, 5, N)
    r, _ = stage(eng, rep)
    table = (_lib.hqt_row_sampler * B)()
    _lib.check(eng.lib.hqt_set_row_samplers(eng.h, B, table))
    with pytest.raises(_lib.HqtError, match='row-sampler table') as err:
        eng.score(B, cond, codes, precision=PRECISION_EXACT)
    assert err.value.code == -3                  # HQT_ERR_STATE
    eng.score(B, cond, codes, precision=PRECISION_EXACT)
    torch.cuda.synchronize()
    assert untouched(rep, ()), 'a refused hqt_score left the report staged'


# ------------------------------------------------------------------------------- 7. errors
def stage(eng, rep, top_n=None):
    r = _lib.hqt_draw_report()
    r.entropy, r.rank = (None if f is None else f.data_ptr() for f in (rep.entropy, rep.rank))
    r.top_n = (0 if rep.top_codes is None else int(rep.top_codes.shape[-1])) if top_n is None else top_n
    r.top_codes, r.top_logprobs = (None if f is None else f.data_ptr() for f in (rep.top_codes, rep.top_logprobs))
    return r, eng.lib.hqt_set_draw_report(eng.h, _lib.C.byref(r))


def test_errors(g4):
    fx, spec, weights, eng = g4
    B, n = 2, 3
    cond = torch.tensor([7, 1])
    rep = buffers(B, n, 5, 16)
    last = lambda: eng.lib.hqt_last_error().decode()
    assert stage(eng, rep, 17)[1] == -1 and 'top_n=17 outside [0, HQT_REPORT_MAX_TOP = 16]' in last()
    assert stage(eng, rep, -1)[1] == -1 and 'top_n=-1 outside' in last()
    assert stage(eng, rep._replace(top_codes=None), 16)[1] == -1 and 'top_codes is NULL' in last()
    assert stage(eng, rep._replace(top_logprobs=None), 16)[1] == -1 and 'top_logprobs is NULL' in last()
    assert stage(eng, rep, 0)[1] == -1 and 'top_codes is set and top_n is 0' in last()
    assert stage(eng, rep._replace(top_codes=None), 0)[1] == -1 and 'top_logprobs is set and top_n is 0' in last()
    assert eng.lib.hqt_set_draw_report(None, None) == -1 and 'null handle' in last()
    # none of the refused structs stayed staged
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=71)
    torch.cuda.synchronize()
    assert untouched(rep, ())
    # NULL and an empty struct clear
    assert stage(eng, rep)[1] == 0 and eng.lib.hqt_set_draw_report(eng.h, None) == 0
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=71)
    assert stage(eng, rep)[1] == 0 and stage(eng, DrawReport(None, None, None, None))[1] == 0
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=71)
    torch.cuda.synchronize()
    assert untouched(rep, ())
    # a staged report is gone after a failed call
    assert stage(eng, rep)[1] == 0
    with pytest.raises(_lib.HqtError):
        eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=71, temperature=(0.0, 1.0))
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=71)
    torch.cuda.synchronize()
    assert untouched(rep, ())
    # a lane has its own
    lane = eng.clone()
    assert stage(eng, rep)[1] == 0
    lane.sample(B, cond, n, precision=PRECISION_EXACT, seed=71)
    torch.cuda.synchronize()
    assert untouched(rep, ())
    eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=71)
    torch.cuda.synchronize()
    assert written(rep, ())
    lane.close()
    eng.range_check()


def test_top_n_above_the_vocabulary_is_refused_by_the_taking_call():
    spec, weights = SR.base_weights(100)
    from dataclasses import replace
    small = replace(spec, vocab_top=8, vocab_bot=8)
    from hqtransformer_amd import synth
    eng = engine_s2(small, synth.stage2_weights(small, 7, 'fixture'), 2, 4, max_prefix=3)
    B, n = 2, 3
    cond = t_(SR.cond(B))
    rep = buffers(B, n, 5, 16)
    assert stage(eng, rep)[1] == 0               # staging cannot know the vocabulary of the taking call
    with pytest.raises(_lib.HqtError, match=r'top_n=16, this model\'s vocabulary has 8 codes') as err:
        eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=72)
    assert err.value.code == -1
    assert stage(eng, rep)[1] == 0
    codes = [torch.zeros((B, n), dtype=torch.int64), torch.zeros((B, n, 4), dtype=torch.int64)]
    with pytest.raises(_lib.HqtError, match='top_n=16'):
        eng.score(B, cond, codes, precision=PRECISION_EXACT)
    with pytest.raises(ValueError, match='N=16 alternatives, the vocabulary has 8 codes'):
        eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=72, report_out=rep)
    ok = buffers(B, n, 5, 8)
    ct, cb, lg = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=72, return_logits=True, report_out=ok)
    torch.cuda.synchronize()
    assert untouched(rep, ())
    R.check_rows(np_(lg), all_codes([ct, cb]), host(ok), 8, 'V = 8, top_n = 8: the whole row in order')
    assert (np.sort(np_(ok.top_codes), axis=-1) == np.arange(8)).all()
    eng.range_check()
    eng.close()


# ------------------------------------------------------------------------------- 8. Python end to end
@pytest.fixture(scope='module')
def tiny_model():
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to('cuda').eval()


def test_sampling_ihqgpt_returns_the_report_behind_the_logprobs(tiny_model):
    st2 = tiny_model.stage2
    B, n = 3, 6
    cond = torch.tensor([417, 3, 99])
    kw = dict(num_candidates=B, cond=cond, use_fp16=False, is_tqdm=False, max_seq_len=n, seed=81, top_k_top=50, top_k_bot=20)
    ct, cb, lp, rep = sampling_ihqgpt(st2, return_logprobs=True, return_report=5, **kw)
    plain = sampling_ihqgpt(st2, return_logprobs=True, **kw)
    torch.cuda.synchronize()
    assert isinstance(rep, DrawReport) and tuple(rep.top_codes.shape) == (B, n, 5, 5) and rep.rank.dtype == torch.int32
    assert torch.equal(ct, plain[0]) and torch.equal(cb, plain[1]) and torch.equal(lp, plain[2])
    eng = st2.engine(B, n)
    _, _, lg = eng.sample(B, cond, n, precision=PRECISION_EXACT, force_top=ct, force_bot=cb, return_logits=True)
    torch.cuda.synchronize()
    R.check_rows(np_(lg), all_codes([ct, cb]), host(rep), 5, 'sampling_ihqgpt(return_report=5)')
    ct0, cb0, rep0 = sampling_ihqgpt(st2, return_report=0, **kw)
    assert rep0.top_codes is None and rep0.top_logprobs is None and same_bits(np_(rep0.entropy), np_(rep.entropy)) and torch.equal(rep0.rank, rep.rank)
    # a guided call returns the positive half of the report
    out = sampling_ihqgpt(st2, return_report=2, guidance_scale=2.0, neg_cond=5, **kw)
    assert tuple(out[-1].entropy.shape) == (B, n, 5) and bool(torch.isfinite(out[-1].entropy).all())
    st2.range_check()


def test_rolling_sampler_returns_each_requests_slice(tiny_model):
    st2 = tiny_model.stage2
    n = 4
    reqs = [(417, 1001, 0), (3, 2002, 11), (99, 3003, 5)]
    roll = RollingSampler(st2, 3, n, precision='exact', return_logprobs=True, return_report=0)
    tickets = [roll.submit(reqs[0][0], seed=reqs[0][1], sample_offset=reqs[0][2])]
    done = roll.step(2)                          # request 0 stands at position 2 when the other two join at 0
    tickets += [roll.submit(c, seed=s, sample_offset=o) for c, s, o in reqs[1:]]
    done += roll.step(1)
    assert roll.live == 3 and not done
    done += roll.drain(1)
    torch.cuda.synchronize()
    assert sorted(d[0] for d in done) == tickets
    for ticket, codes, lp, rep in done:
        c, s, o = reqs[ticket]
        want = sampling_ihqgpt(st2, 1, c, use_fp16=False, is_tqdm=False, max_seq_len=n, seed=s, sample_offset=o, return_logprobs=True, return_report=0)
        torch.cuda.synchronize()
        assert torch.equal(codes[0], want[0][0]) and torch.equal(codes[1], want[1][0])
        assert tuple(rep.entropy.shape) == (n, 5) and rep.top_codes is None
        assert same_bits(np_(rep.entropy), np_(want[3].entropy[0])) and torch.equal(rep.rank, want[3].rank[0]), f'request {ticket}'
    st2.range_check()


def test_a_session_remaps_the_report_with_its_rows(tiny_model):
    st2 = tiny_model.stage2
    B, n = 3, 6
    cond = torch.tensor([417, 3, 99])
    kw = dict(seed=83, precision='exact', top_k_top=50, top_k_bot=20)
    st2.engine(4, n)                             # room for the four rows the mapping below leaves
    ref = SamplingSession(st2, B, cond, n, return_logprobs=True, return_report=3, **kw)
    ref.finish()
    s = SamplingSession(st2, B, cond, n, return_logprobs=True, return_report=3, **kw)
    s.advance(2)
    s.select([2, 2, 0, 0])                        # row 1 is dropped, rows 2 and 0 are duplicated (they keep their keys: they go on drawing the same codes)
    codes = s.finish()
    torch.cuda.synchronize()
    for j, src in enumerate([2, 2, 0, 0]):
        assert torch.equal(codes[0][j], ref.codes[0][src]) and torch.equal(codes[1][j], ref.codes[1][src])
        assert all(same_bits(np_(a[j]), np_(b[src])) for a, b in zip(s.report, ref.report)), f'row {j} (from {src})'
    assert tuple(s.report.top_codes.shape) == (4, n, 5, 3) and written(s.report, ())
    st2.range_check()


def test_score_images_with_a_report_and_the_map(tiny_model):
    model = tiny_model
    res = model.stage1.spec.resolution
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, 3, res, res)).astype(np.float32)).to(dev())
    score, codes, rep = score_images(model, x, 2, precision='exact', report=1)
    plain, codes2 = score_images(model, x, 2, precision='exact')
    torch.cuda.synchronize()
    assert torch.equal(score, plain) and all(torch.equal(a, b) for a, b in zip(codes, codes2))
    n = int(codes[0].shape[1])
    K = int(round(n ** 0.5))
    assert tuple(rep.top_codes.shape) == (2, n, 5, 1) and written(rep, ())
    maps = uncertainty_map(rep.entropy, 2)
    assert [tuple(m.shape) for m in maps] == [(2, K, K), (2, 2 * K, 2 * K)]
    assert 0.0 <= float(maps[1].min()) and float(maps[1].max()) <= np.log(model.stage2.spec.vocab_top) + R.ENTROPY_GATE
    assert maps[0][1, 3, 5] == rep.entropy[1, 3 * K + 5, 0] and maps[1][1, 2 * 3 + 1, 2 * 5] == rep.entropy[1, 3 * K + 5, 1 + 2]
    # where the image's own code is the most likely one its rank is 0 and its log-probability the top one
    first = rep.rank == 0
    lp = model.stage2.engine(2, n).score(2, torch.tensor([2, 2]), codes, precision=PRECISION_EXACT)
    torch.cuda.synchronize()
    assert torch.equal(rep.top_logprobs[..., 0][first], lp[first]) and bool((rep.top_codes[..., 0][first] == torch.cat([c.reshape(2, n, -1) for c in codes], 2)[first]).all())
    # the stepwise path reports too
    s2, _, rep2 = score_images(model, x, 2, precision='exact', report=1, one_pass=False)
    torch.cuda.synchronize()
    assert float((rep2.entropy - rep.entropy).abs().max()) <= 2 * LOGPROB_TOL * (1 + np.log(model.stage2.spec.vocab_top))
    model.stage2.range_check()


def test_merged_steps_get_their_rows_of_the_report(tiny_model):
    from hqtransformer_amd.pipeline import InflightSampler
    model = tiny_model
    B, n = 2, 64                                 # a merged pass decodes what it samples: all 64 positions of the tiny model's images
    pipe = InflightSampler(model, lanes=1, merge=2)
    kw = dict(max_seq_len=n, use_fp16=False, precision='exact', top_k_top=50, top_k_bot=20, return_report=2)
    p0 = pipe.submit(B, 5, seed=91, **kw)
    p1 = pipe.submit(B, 9, seed=92, sample_offset=64, return_logprobs=True, **kw)
    pipe.drain()
    torch.cuda.synchronize()
    r0, r1 = p0.get(), p1.get()
    assert len(r0) == 5 and len(r1) == 6 and isinstance(r0[4], DrawReport) and isinstance(r1[5], DrawReport)
    for r, cls, seed, off in ((r0, 5, 91, 0), (r1, 9, 92, 64)):
        want = sampling_ihqgpt(model.stage2, B, cls, use_fp16=False, is_tqdm=False, max_seq_len=n, seed=seed, sample_offset=off, top_k_top=50, top_k_bot=20,
                               return_report=2)
        torch.cuda.synchronize()
        assert torch.equal(r[0], want[0]) and torch.equal(r[1], want[1])
        assert tuple(r[-1].top_codes.shape) == (B, n, 5, 2) and same_report(r[-1], want[2]), 'EXACT: a row reports the same bits in a merged pass and alone'
    model.stage2.range_check()


def test_the_class_driver_writes_report_npz(tmp_path):
    from hqtransformer_amd import sampling_hqmodel
    args = ['-r', str(tmp_path), '-m', os.path.join(ROOT, 'configs', 'tiny-cls.yaml'), '--num-classes', '2', '--samples-per-class', '2', '--batch-size', '2',
            '--decode-precision', 'exact', '--seed', '3']
    sampling_hqmodel.main(args + ['--report-top', '4'])
    with_report = {f: open(os.path.join(tmp_path, f), 'rb').read() for f in sorted(os.listdir(tmp_path)) if f != 'report.npz'}
    rep = np.load(os.path.join(tmp_path, 'report.npz'))
    assert sorted(rep.files) == ['entropy', 'rank', 'top_codes', 'top_logprobs']
    assert rep['entropy'].shape == (4, 64, 5) and rep['top_codes'].shape == (4, 64, 5, 4) and rep['rank'].dtype == np.int32
    assert np.isfinite(rep['entropy']).all() and (rep['rank'] >= 0).all() and (np.diff(rep['top_logprobs'], axis=-1) <= 0).all()
    plain = tmp_path / 'plain'
    sampling_hqmodel.main(['-r', str(plain)] + args[2:])
    assert sorted(os.listdir(plain)) == sorted(with_report), 'without the flag there is no report.npz and nothing else changes'
    for f, data in with_report.items():
        assert open(os.path.join(plain, f), 'rb').read() == data, f'{f} differs without --report-top'
