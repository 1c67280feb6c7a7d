"""The three-level and bidirectional depth heads off the grid their fixtures sit on (tests/offgrid_depth_cases.py: which model reaches which kernel),
through the C ABI and against the CPU oracle.  EXACT and SPLIT: codes of every level bit-identical, logits within 2e-4 (the bar include/hqt.h promises
for every accepted config); FAST: teacher-forced on the oracle's codes, every logit finite and max |logits - oracle| inside a gate of twice the figure
measured on the MI355X (profiles/offgrid_depth_fast_gates.txt), never above the suite's blanket 0.15.  Every engine starts on a NaN-poisoned workspace.
The attention kernel of every depth sub-step is read from the engine's counters ('variant:attn_<kernel>:depth') and held to the host's prediction
(tests/test_offgrid_depth_host.py); the GEMM variants are asserted where the case was written for one."""
import ctypes as C
import os
import time
from collections import Counter

import numpy as np
import pytest
import torch

from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from tests import offgrid_depth_cases as DC
from tests.helpers import gate
from tests.score_ref import LOGPROB_TOL, log_softmax_at

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
FAST_BLANKET = 0.15               # fixture-weight models with logits of standard deviation about 3 (the oracle's here: 3.0 .. 3.2)
SCORED = ('LA', 'LC', 'BB')       # cases that also run the one-pass score, on engines of their own (score chunk 7, and one chunk for all pairs)
BOTH_CHAINS = ('LD', 'LF', 'BC', 'BD')      # FAST with the persistent body and with the launch chain
SCORE_CHUNK = 7                   # divides neither B n = 15 (LA), 10 (LC) nor 134 (BB)

# FAST gates: max |logits - oracle| measured on the MI355X per (case, persistent switch), as recorded in profiles/offgrid_depth_fast_gates.txt.  The
# limit is twice that, rounded up to 0.01, and never above the blanket bound.  A gate without an entry has not been measured: the test fails and names it.
# The figures are the recorded ones rounded up to four decimals.  Eager and graph returned the same figure everywhere, and so did the persistent body
# and the launch chain (LD, LF, BC, BD: the largest error sits in the depth head, which is the launch chain in both).  Figures above 0.075 (their
# doubled limit is cut off at 0.15) are the level of this model family at logits up to |l| = 15 (a bf16 ulp there is 0.0625), as in
# tests/test_gpu_offgrid_stage2.py; BB's 0.108 is the largest here: 335 rows x 1000 logits behind one unmasked depth pass.  The four mutations this
# file was tried against (a wrong table slice, row map, few-query bound, a dropped softmax rescale) moved the EXACT logits by 1.9 .. 14.8.
FAST_MEASURED = {
    ('LA', None): 0.0918, ('LB', None): 0.0737, ('LC', None): 0.0666, ('LD', True): 0.0757, ('LD', False): 0.0757, ('LE', None): 0.0911,
    ('LF', True): 0.0632, ('LF', False): 0.0632, ('LG', None): 0.0813, ('BA', None): 0.0925, ('BB', None): 0.1083, ('BC', True): 0.0635,
    ('BC', False): 0.0635, ('BD', True): 0.0776, ('BD', False): 0.0776, ('BE', None): 0.0767,
}
FAST_LIMITS = {k: min(float(np.ceil(200.0 * m - 1e-9)) / 100.0, FAST_BLANKET) for k, m in FAST_MEASURED.items()}


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return None if a is None else torch.from_numpy(np.array(a))          # a copy: the shared oracle arrays are read-only


_ENGINES = {}


def engine(name, score_chunk=0):
    """One engine per model (LF / LD, BC and the like differ in their head, so every case is a model of its own), shared by the tests of this module;
    score_chunk: an engine with room for the one-pass score in chunks of that many pairs."""
    spec, weights, cond, noise, B, n, settings = DC.inputs(name)
    if (name, score_chunk) not in _ENGINES:
        assert torch.cuda.is_available(), 'these tests need the MI355X'
        os.environ['HQT_POISON_WORKSPACE'] = '1'          # every workspace buffer starts as NaN: a row no kernel wrote shows up
        try:
            e = Engine(spec, None, torch.device('cuda:0'), B, n, max_prefix=n - 1 if score_chunk else 0, score_chunk=score_chunk)
        finally:
            del os.environ['HQT_POISON_WORKSPACE']
        e.load(stage2=weights)
        e.finalize()
        _ENGINES[(name, score_chunk)] = e
    return _ENGINES[(name, score_chunk)]


def variants(eng):
    return {k: v[0] for k, v in eng.timing_report().items() if k.startswith('variant:') and v[0] > 0}      # (a reset keeps the slots of earlier calls, at 0)


def timed(eng, fn):
    """fn() eagerly under the engine's counters -> (its result, the variants it counted)."""
    eng.timing_reset()
    eng.timing(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        v = variants(eng)
    finally:
        eng.timing(False)
    return out, v


def sample(eng, name, precision, graph, B=None, force=None):
    """The case's call -> (codes per level, logits [n, draws, B, V]); B: its first B rows alone, with the same per-row noise."""
    spec, weights, cond, noise, B0, n, settings = DC.inputs(name)
    if B is not None:
        cond, noise = (None if cond is None else cond[:B]), noise[:, :, :B]
    kw = dict(precision=precision, noise=t_(noise), return_logits=True, use_graph=graph, **settings)
    if DC.is_bidir(name):
        if force is not None:
            kw.update(force_top=t_(force[0]), force_bot=t_(force[1]))
        out = eng.sample(B or B0, t_(cond), n, **kw)
    else:
        if force is not None:
            kw.update(force=[t_(f) for f in force])
        out = eng.sample3(B or B0, t_(cond), n, **kw)
    return [np_(c) for c in out[:-1]], np_(out[-1])


# (case, precision) -> (variant prefixes that must have been counted, prefixes that must not).  LA / BA: K = 48 has neither the fp32 matrix path
# (K % 32) nor packed bf16 weights (3 D % 32); only fc2 (K = 192) is on the grid.  LB: 272 rows at level 2 are above the fp32 matrix path's 256, beside
# the 17 and 68 rows of levels 0 and 1 that take it.  LB / BB in FAST: the blocks are packed (D % 32 == 0), the head (V % 32 != 0) is not, and goes to
# the plain MFMA kernel.  BB's one depth pass defers its LayerNorm whatever the heads are, and bidir_head_ln hands them two unpacked operands.  LB's
# stream_gemm_dln launches are its BODY's (persist_program_ok takes K % 64 == 0 only, so at D = 96 the body is the launch chain): its depth blocks
# run the packed streaming GEMM behind a LayerNorm launch, because deferred LayerNorm needs the folded weights of the sub-step's head as well (dln_of
# in run_position) -- DESIGN.md records this against the expectation written from reading.
_BLOCK48 = ('gemm_qkv', 'gemm_proj', 'gemm_fc1', 'gemm_head')
EXPECT = {
    ('LB', PRECISION_EXACT): (['variant:gemm_generic_f32:gemm_qkv', 'variant:exact_mfma:gemm_qkv', 'variant:exact_mfma:gemm_head', 'variant:gemm_generic_f32:gemm_head'], []),
    ('LB', PRECISION_FAST): (['variant:stream_gemm_dln:gemm_qkv', 'variant:stream_gemm_dln:gemm_fc1', 'variant:stream_gemm:gemm_qkv', 'variant:stream_gemm:gemm_fc1',
                              'variant:mfma_gemm:gemm_head'],
                             ['variant:stream_gemm:gemm_head', 'variant:stream_gemm_dln:gemm_head', 'variant:gemm_generic']),
    ('BB', PRECISION_FAST): (['variant:stream_gemm_dln:gemm_qkv', 'variant:stream_gemm_dln:gemm_fc1', 'variant:mfma_gemm:gemm_head'],
                             ['variant:stream_gemm:gemm_head', 'variant:stream_gemm_dln:gemm_head', 'variant:gemm_generic']),
}
for _c in ('LA', 'BA'):
    EXPECT[(_c, PRECISION_EXACT)] = ([f'variant:gemm_generic_f32:{t}' for t in _BLOCK48] + ['variant:exact_mfma:gemm_fc2'], [f'variant:exact_mfma:{t}' for t in _BLOCK48])
    EXPECT[(_c, PRECISION_SPLIT)] = ([f'variant:gemm_generic_f32:{t}' for t in _BLOCK48], ['variant:split_gemm'])
    EXPECT[(_c, PRECISION_FAST)] = ([f'variant:gemm_generic_bf16:{t}' for t in _BLOCK48] + ['variant:mfma_gemm:gemm_fc2'], ['variant:stream_gemm', 'variant:tile_gemm', 'variant:persist'])


def variant_problems(name, precision, v, B=None):
    """The attention kernels counted for the depth head against the host's prediction (every sub-step, every depth layer, every position), and the GEMMs
    the case was written for."""
    spec, _, n = DC.CASES[name]
    want = Counter(f'variant:attn_{k}:depth' for k in DC.predicted_attention(name, precision == PRECISION_FAST, B) if k)
    want = {k: c * n * spec.n_layers_depth for k, c in want.items()}
    got = {k: c for k, c in v.items() if k.startswith('variant:attn_') and k.endswith(':depth')}
    out = [] if got == want else [f'depth attention: counted {got}, predicted {want}']
    need, never = EXPECT.get((name, precision), ([], []))
    out += [f'{p} was not counted' for p in need if not any(k.startswith(p) for k in v)]
    return out + [f'{k} was counted' for p in never for k in v if k.startswith(p)]


def run_exact_or_split(name, precision):
    """The free run of a case in EXACT (eager, counted, and from the graph) or SPLIT (eager) -> one record per run."""
    codes, lg, _ = DC.oracle(name)
    eng = engine(name)
    recs = []
    for graph in ((False, True) if precision == PRECISION_EXACT else (False,)):
        t0 = time.perf_counter()
        (got, lgot), v = timed(eng, lambda: sample(eng, name, precision, False)) if not graph else (sample(eng, name, precision, True), None)
        eng.range_check()
        torch.cuda.synchronize()
        finite = bool(np.isfinite(lgot).all())
        rec = dict(case=name, precision=precision, graph=graph, codes_equal=[bool((g == c).all()) for g, c in zip(got, codes)], finite=finite,
                   logit_err=float(np.abs(lgot - lg).max()) if finite else float('nan'), seconds=round(time.perf_counter() - t0, 2))
        if v is not None:
            rec['variants'] = v
            rec['variant_problems'] = variant_problems(name, precision, v)
        print(rec)
        recs.append(rec)
    return recs


def run_fast(name, persist=None):
    """Teacher-forced FAST on the oracle's codes, eager (counted) and from the graph; persist: True / False sets the switch for the call (restored after)."""
    codes, lg, _ = DC.oracle(name)
    eng = engine(name)
    recs = []
    if persist is not None:
        eng.set_persist(persist)
    try:
        for graph in (False, True):
            t0 = time.perf_counter()
            call = lambda: sample(eng, name, PRECISION_FAST, graph, force=codes)
            (got, lf), v = timed(eng, call) if not graph else (call(), None)
            eng.range_check()
            torch.cuda.synchronize()
            finite = bool(np.isfinite(lf).all())
            rec = dict(case=name, precision=PRECISION_FAST, graph=graph, persist=persist, finite=finite,
                       logit_err=float(np.abs(lf - lg).max()) if finite else float('nan'),
                       agree=float(np.mean([(g == c).mean() for g, c in zip(got, codes)])), seconds=round(time.perf_counter() - t0, 2))
            if v is not None:
                rec['variants'] = v
                rec['variant_problems'] = variant_problems(name, PRECISION_FAST, v)
                rec['persistent'] = sorted(k for k in v if k.startswith('variant:persist'))
            print(rec)
            recs.append(rec)
    finally:
        if persist is not None:
            eng.set_persist(True)
    return recs


def gate_name(rec):
    tail = '' if rec['persist'] is None else f',persist={rec["persist"]}'
    return f'offgrid_depth.fast_logits({rec["case"]},graph={rec["graph"]}{tail})'


def score_logits_want(lg):
    """The oracle's logits [n, draws, B, V] in the layout hqt_score returns them: [B, n, V], [B, n, 4, V](, [B, n, 16, V])."""
    out = [lg[:, 0].transpose(1, 0, 2), lg[:, 1:5].transpose(2, 0, 1, 3)]
    return out + ([lg[:, 5:21].transpose(2, 0, 1, 3)] if lg.shape[1] == 21 else [])


def run_score(name, precision, chunk):
    spec, weights, cond, noise, B, n, settings = DC.inputs(name)
    codes, lg, _ = DC.oracle(name)
    eng = engine(name, chunk)
    lp, logits = eng.score(B, t_(cond), [t_(c) for c in codes], precision=precision, return_logits=True)
    eng.range_check()
    torch.cuda.synchronize()
    rec = dict(case=name, precision=precision, chunk=chunk, finite=bool(torch.isfinite(lp).all()),
               logprob_err=float(np.abs(np_(lp) - log_softmax_at(lg, codes)).max()),
               logit_err=float(max(np.abs(np_(g) - w).max() for g, w in zip(logits, score_logits_want(lg)))))
    print(rec)
    return rec, lp, logits


# ------------------------------------------------------------------------------- EXACT and SPLIT
@pytest.mark.parametrize('name', list(DC.CASES))
def test_exact_codes_and_logits_vs_oracle(name):
    for rec in run_exact_or_split(name, PRECISION_EXACT):
        assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL, rec
        assert all(rec['codes_equal']), rec
        assert not rec.get('variant_problems'), rec


@pytest.mark.parametrize('name', [c for c in DC.CASES if c != 'LG'])
def test_split_codes_and_logits_vs_oracle(name):
    for rec in run_exact_or_split(name, PRECISION_SPLIT):
        assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL, rec
        assert all(rec['codes_equal']), rec
        assert not rec.get('variant_problems'), rec


# ------------------------------------------------------------------------------- FAST
@pytest.mark.parametrize('name,persist', [(c, None) for c in DC.CASES if c not in BOTH_CHAINS] + [(c, p) for c in BOTH_CHAINS for p in (True, False)])
def test_fast_teacher_forced_logits_vs_oracle(name, persist):
    for rec in run_fast(name, persist):
        assert rec['finite'], rec
        assert (name, persist) in FAST_LIMITS, f'{gate_name(rec)}: no measured limit (profiles/offgrid_depth_fast_gates.txt); this run: {rec["logit_err"]:.4f}'
        gate(gate_name(rec), rec['logit_err'], FAST_LIMITS[(name, persist)])
        assert not rec.get('variant_problems'), rec
        if persist is False:
            assert not rec.get('persistent'), rec


# ------------------------------------------------------------------------------- one-pass score
@pytest.mark.parametrize('name', SCORED)
def test_one_pass_score_vs_oracle(name):
    """hqt_score on the oracle's codes: score_depth_embed_l2_kernel without (LA) and with (LC) the [V, 4 D] tables, score_depth_input_kernel under the
    bidirectional row map (BB); chunks of 7 pairs -- a ragged last one -- and one chunk for all B n pairs.  EXACT: the two chunkings give the same bits."""
    B, n = DC.CASES[name][1:]
    assert (B * n) % SCORE_CHUNK
    exact = []
    for precision in (PRECISION_EXACT, PRECISION_SPLIT):
        for chunk in (SCORE_CHUNK, B * n):
            rec, lp, logits = run_score(name, precision, chunk)
            assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL and rec['logprob_err'] <= LOGPROB_TOL, rec
            if precision == PRECISION_EXACT:
                exact.append((lp, logits))
    assert torch.equal(exact[0][0], exact[1][0]) and all(torch.equal(a, b) for a, b in zip(exact[0][1], exact[1][1])), f'{name}: EXACT scores depend on the chunk'


def test_one_pass_score_still_refuses_top2mid2bot():
    codes, _, _ = DC.oracle('LF')
    B, n = DC.CASES['LF'][1:]
    eng = engine('LF')
    with pytest.raises(ValueError, match="'top2mid2bot' depth head runs 21 causal sub-steps"):
        eng.score(B, t_(DC.inputs('LF')[2]), [t_(c) for c in codes])
    dev = torch.device('cuda:0')
    cs = [t_(c).to(dev) for c in codes]
    lp = torch.empty((B, n, 21), dtype=torch.float32, device=dev)
    cond = t_(DC.inputs('LF')[2]).to(dev)
    rc = eng.lib.hqt_score(eng.h, B, cond.data_ptr(), (C.c_void_p * 3)(*[c.data_ptr() for c in cs]), n, PRECISION_EXACT, lp.data_ptr(), None, None)
    torch.cuda.synchronize()
    msg = eng.lib.hqt_last_error().decode()
    assert rc == -1 and "the 'top2mid2bot' depth head (21 causal sub-steps per position) is not built for the one-pass score" in msg, (rc, msg)


# ------------------------------------------------------------------------------- batch composition
@pytest.mark.parametrize('name', ['LE', 'BB'])
def test_exact_rows_do_not_depend_on_the_batch_they_sit_in(name):
    """The first five rows alone, with the same per-row noise, draw the codes they draw inside B = 67: attention.hip promises one kernel per row count
    in EXACT, the GEMM chains are k-ordered at every row count, LayerNorm and the sampler work per row."""
    codes, lg, _ = DC.oracle(name)
    eng = engine(name)
    full, lfull = sample(eng, name, PRECISION_EXACT, False)
    (five, lfive), v = timed(eng, lambda: sample(eng, name, PRECISION_EXACT, False, B=5))
    eng.range_check()
    rec = dict(case=name, rows=5, codes_equal_in_batch=[bool((a == b[:5]).all()) for a, b in zip(five, full)],
               codes_equal_oracle=[bool((a == c[:5]).all()) for a, c in zip(five, codes)], logit_err=float(np.abs(lfive - lg[:, :, :5]).max()),
               logit_diff_in_batch=float(np.abs(lfive - lfull[:, :, :5]).max()), variant_problems=variant_problems(name, PRECISION_EXACT, v, B=5))
    print(rec)
    assert all(rec['codes_equal_in_batch']) and all(rec['codes_equal_oracle']), rec
    assert rec['logit_err'] <= LOGIT_TOL, rec
    assert not [p for p in rec['variant_problems'] if p.startswith('depth attention')], rec
