"""Stage 2 off the grid the rest of the suite runs (tests/offgrid_cases.py: which model reaches which kernel), through the C ABI and against the CPU
oracle.  EXACT and SPLIT: codes bit-identical, logits within 2e-4 (the bar include/hqt.h promises for every accepted config); FAST: teacher-forced
on the oracle's codes, every logit finite and max |logits - oracle| inside a gate of about twice the figure measured on the MI355X
(profiles/offgrid_fast_gates.txt), never above the suite's blanket 0.15.  Every engine starts on a NaN-poisoned workspace.  The kernel variants each
call took are read from the engine's counters and asserted where the case was written for one."""
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from tests import offgrid_cases as OG
from tests.helpers import gate
from tests.score_ref import LOGPROB_TOL, log_softmax_at
from tests.test_gpu_logprobs import check_own

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
FAST_BLANKET = 0.15               # fixture-weight models with logits of standard deviation about 3 (the oracle's here: 3.0 .. 3.3)
SCORED = ('A', 'C')               # cases that also run the one-pass score: the engine is created with room for the prefix
LOGPROBS = ('A', 'B')             # ... that also return log-probabilities (and every row of the vocabulary sweep)
BOTH_CHAINS = ('C', 'D', 'F')     # FAST with the persistent program and with the launch chain
SWEEP = [r for r in OG.ROWS if r.startswith('V')]

# FAST gates: max |logits - oracle| measured on the MI355X per (case, persistent switch) -- eager and graph returned the same bits everywhere --
# as recorded in profiles/offgrid_fast_gates.txt.  The limit is twice that, rounded up to 0.01, and never above the blanket bound.  Figures above
# 0.075 (A, B, C, D chain, E, F, V1000-cut, V16384: their doubled limit is cut off at 0.15) are the level of this model family, not of an off-grid
# kernel: F and G run only kernels the grid runs too (0.074 .. 0.077), tests/test_gpu_timed_schedule.py records 0.077 at the same logit standard
# deviation, and a bf16 ulp at the largest logits here (|l| up to 15.6) is 0.0625.  A kernel that is wrong shows as > 1.6 (a K loop 16 short, a
# missing online-softmax rescale).  A gate without an entry has not been measured: the test fails and names it.
FAST_MEASURED = {
    ('A', None): 0.0787, ('B', None): 0.0862, ('C', True): 0.0892, ('C', False): 0.0835, ('D', True): 0.0733,
    ('D', False): 0.0845, ('E', None): 0.0758, ('F', True): 0.0751, ('F', False): 0.0765, ('G', None): 0.0741,
    ('V100-plain', None): 0.0688, ('V100-cut', None): 0.0541, ('V260-plain', None): 0.0663, ('V260-cut', None): 0.0656, ('V1000-plain', None): 0.0608,
    ('V1000-cut', None): 0.0821, ('V1500-plain', None): 0.0633, ('V1500-cut', None): 0.0640, ('V5000-plain', None): 0.0738, ('V5000-cut', None): 0.0697,
    ('V16384-plain', None): 0.0834, ('V16384-cut', None): 0.0773,
}
FAST_LIMITS = {k: min(float(np.ceil(200.0 * m - 1e-9)) / 100.0, FAST_BLANKET) for k, m in FAST_MEASURED.items()}


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return None if a is None else torch.from_numpy(np.array(a))          # a copy: the shared oracle arrays are read-only


_ENGINES = {}


def engine(name):
    """One engine per model, shared by the tests of this module (the plain and the cut row of a vocabulary share theirs)."""
    spec, weights, cond, noise, B, n, settings = OG.inputs(name)
    key = name.split('-')[0]
    if key not in _ENGINES:
        assert torch.cuda.is_available(), 'these tests need the MI355X'
        os.environ['HQT_POISON_WORKSPACE'] = '1'          # every workspace buffer starts as NaN: a row no kernel wrote shows up
        try:
            e = Engine(spec, None, torch.device('cuda:0'), B, n, max_prefix=n - 1 if name in SCORED else 0)
        finally:
            del os.environ['HQT_POISON_WORKSPACE']
        e.load(stage2=weights)
        e.finalize()
        _ENGINES[key] = e
    return _ENGINES[key]


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


# (case, precision) -> (variant prefixes that must have been counted, prefixes that must not).  A: K = 48 has neither the fp32 matrix path
# (K % 32) nor packed bf16 weights (3 D % 32); only fc2 (K = 192) is on the grid.  B: the body is packed and normalises in its GEMMs, the head
# (V % 32 != 0) is not packed; its 320-row depth sub-step is above the fp32 matrix path's 256 rows, and in SPLIT only fc2 (K = 384) is a multiple of 64.
# E: as A at K = 80, fc2 at K = 320.  D and the sweep: a head with V % 32 != 0 behind a packed body.
_BLOCK48 = ('gemm_qkv', 'gemm_proj', 'gemm_fc1', 'gemm_head')
EXPECT = {
    ('A', PRECISION_EXACT): ([f'variant:gemm_generic_f32:{t}' for t in _BLOCK48] + ['variant:exact_mfma:gemm_fc2'], [f'variant:exact_mfma:{t}' for t in _BLOCK48]),
    ('A', PRECISION_SPLIT): ([f'variant:gemm_generic_f32:{t}' for t in _BLOCK48], ['variant:split_gemm']),
    ('A', PRECISION_FAST): ([f'variant:gemm_generic_bf16:{t}' for t in _BLOCK48] + ['variant:mfma_gemm:gemm_fc2'], ['variant:stream_gemm', 'variant:tile_gemm', 'variant:persist']),
    ('B', PRECISION_EXACT): (['variant:gemm_generic_f32:gemm_qkv', 'variant:exact_mfma:gemm_qkv', 'variant:exact_mfma:gemm_head'], []),
    ('B', PRECISION_SPLIT): (['variant:split_gemm', 'variant:gemm_generic_f32:gemm_qkv'], []),
    ('B', PRECISION_FAST): (['variant:stream_gemm_dln:gemm_qkv', 'variant:stream_gemm_dln:gemm_fc1', 'variant:mfma_gemm:gemm_head'],
                            ['variant:stream_gemm:gemm_head', 'variant:stream_gemm_dln:gemm_head', 'variant:tile_gemm', 'variant:gemm_generic']),
    ('D', PRECISION_FAST): (['variant:mfma_gemm:gemm_head'], ['variant:stream_gemm:gemm_head', 'variant:stream_gemm_dln:gemm_head', 'variant:gemm_generic']),
    ('E', PRECISION_EXACT): ([f'variant:gemm_generic_f32:{t}' for t in _BLOCK48] + ['variant:exact_mfma:gemm_fc2', 'variant:gemm_generic_f32:gemm_fc2'],
                             [f'variant:exact_mfma:{t}' for t in _BLOCK48]),
    ('E', PRECISION_SPLIT): (['variant:split_gemm', 'variant:gemm_generic_f32:gemm_qkv'], []),
    ('E', PRECISION_FAST): ([f'variant:gemm_generic_bf16:{t}' for t in _BLOCK48] + ['variant:mfma_gemm:gemm_fc2'], ['variant:stream_gemm', 'variant:tile_gemm']),
}
for _V in OG.SWEEP_V:
    for _kind in ('plain', 'cut'):
        EXPECT[(f'V{_V}-{_kind}', PRECISION_EXACT)] = (['variant:exact_mfma:gemm_head'], ['variant:gemm_generic'])
        if _V % 32:
            EXPECT[(f'V{_V}-{_kind}', PRECISION_FAST)] = (['variant:mfma_gemm:gemm_head'], ['variant:stream_gemm:gemm_head', 'variant:stream_gemm_dln:gemm_head', 'variant:gemm_generic'])


def variant_problems(name, precision, v):
    need, never = EXPECT.get((name, precision), ([], []))
    out = [f'{p} was not counted' for p in need if not any(k.startswith(p) for k in v)]
    return out + [f'{k} was counted' for p in never for k in v if k.startswith(p)]


def run_exact_or_split(name, precision):
    """The free run of a row in EXACT or SPLIT, eager (counted) and from the graph -> one record per run: codes equal, largest logit error, variants."""
    spec, weights, cond, noise, B, n, settings = OG.inputs(name)
    ct, cb, lg, _ = OG.oracle(name)
    eng = engine(name)
    want_lp = name in LOGPROBS or name in SWEEP
    graphs = (False, True) if precision == PRECISION_EXACT or name in ('B', 'E') else (False,)
    recs = []
    for graph in graphs:
        call = lambda: eng.sample(B, t_(cond), n, precision=precision, noise=t_(noise), return_logits=True, return_logprobs=want_lp, use_graph=graph, **settings)
        out, v = timed(eng, call) if not graph else (call(), None)
        eng.range_check()
        torch.cuda.synchronize()
        rec = dict(case=name, precision=precision, graph=graph, codes_equal=bool((np_(out[0]) == ct).all() and (np_(out[1]) == cb).all()),
                   finite=bool(torch.isfinite(out[2]).all()), logit_err=float(np.abs(np_(out[2]) - lg).max()))
        if v is not None:
            rec['variants'] = v
            rec['variant_problems'] = variant_problems(name, precision, v)
        print(rec)
        if want_lp and rec['finite']:
            check_own(out, 2, f'{name} precision={precision} graph={graph}')
        recs.append(rec)
    return recs


def run_fast(name, persist=None):
    """Teacher-forced FAST on the oracle's codes, eager (counted) and from the graph; persist: True / False sets the switch for the call (restored after)."""
    spec, weights, cond, noise, B, n, settings = OG.inputs(name)
    ct, cb, lg, _ = OG.oracle(name)
    eng = engine(name)
    recs = []
    if persist is not None:
        eng.set_persist(persist)
    try:
        for graph in (False, True):
            call = lambda: eng.sample(B, t_(cond), n, precision=PRECISION_FAST, noise=t_(noise), force_top=t_(ct), force_bot=t_(cb), return_logits=True,
                                      use_graph=graph, **settings)
            out, v = timed(eng, call) if not graph else (call(), None)
            eng.range_check()
            torch.cuda.synchronize()
            lf = np_(out[2])
            rec = dict(case=name, precision=PRECISION_FAST, graph=graph, persist=persist, finite=bool(np.isfinite(lf).all()),
                       logit_err=float(np.abs(lf - lg).max()) if np.isfinite(lf).all() else float('nan'),
                       agree=float(((np_(out[0]) == ct).mean() + 4 * (np_(out[1]) == cb).mean()) / 5))
            if v is not None:
                rec['variants'] = v
                rec['variant_problems'] = variant_problems(name, PRECISION_FAST, v)
                # the persistent program declines a shape it has no phases for (persist_build): recorded, not a failure
                rec['persistent'] = any(k.startswith('variant:persist') for k in v)
            print(rec)
            recs.append(rec)
    finally:
        if persist is not None:
            eng.set_persist(True)
    return recs


def gate_name(rec):
    tail = '' if rec['persist'] is None else f',persist={rec["persist"]}'
    return f'offgrid.fast_logits({rec["case"]},graph={rec["graph"]}{tail})'


def run_score(name, precision):
    spec, weights, cond, noise, B, n, settings = OG.inputs(name)
    ct, cb, lg, _ = OG.oracle(name)
    eng = engine(name)
    lp, logits = eng.score(B, t_(cond), [t_(ct), t_(cb)], precision=precision, return_logits=True)
    eng.range_check()
    torch.cuda.synchronize()
    want_lp = log_softmax_at(lg, [ct, cb])
    rec = dict(case=name, precision=precision, finite=bool(torch.isfinite(lp).all()),
               logprob_err=float(np.abs(np_(lp) - want_lp).max()),
               logit_err=float(max(np.abs(np_(logits[0]) - lg[:, 0].transpose(1, 0, 2)).max(), np.abs(np_(logits[1]) - lg[:, 1:].transpose(2, 0, 1, 3)).max())))
    print(rec)
    return rec


# ------------------------------------------------------------------------------- EXACT and SPLIT
@pytest.mark.parametrize('name', list(OG.ROWS))
def test_exact_codes_and_logits_vs_oracle(name):
    for rec in run_exact_or_split(name, PRECISION_EXACT):
        assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL, rec
        assert rec['codes_equal'], rec
        assert not rec.get('variant_problems'), rec


@pytest.mark.parametrize('name', [r for r in OG.ROWS if r != 'G'])
def test_split_codes_and_logits_vs_oracle(name):
    for rec in run_exact_or_split(name, PRECISION_SPLIT):
        assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL, rec
        assert rec['codes_equal'], rec
        assert not rec.get('variant_problems'), rec


# ------------------------------------------------------------------------------- FAST
@pytest.mark.parametrize('name,persist', [(r, None) for r in OG.ROWS if r not in BOTH_CHAINS] + [(r, p) for r in BOTH_CHAINS for p in (True, False)])
def test_fast_teacher_forced_logits_vs_oracle(name, persist):
    for rec in run_fast(name, persist):
        assert rec['finite'], rec
        assert (name, persist) in FAST_LIMITS, f'{gate_name(rec)}: no measured limit (profiles/offgrid_fast_gates.txt)'
        gate(gate_name(rec), rec['logit_err'], FAST_LIMITS[(name, persist)])
        assert not rec.get('variant_problems'), rec
        if persist is False:
            assert not rec.get('persistent', False), rec


# ------------------------------------------------------------------------------- one-pass score
@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT])
@pytest.mark.parametrize('name', SCORED)
def test_one_pass_score_vs_oracle(name, precision):
    """hqt_score on the oracle's codes: the body pass runs causal multi-query attention at head sizes 16 and 256, the score kernels at V = 100."""
    rec = run_score(name, precision)
    assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL and rec['logprob_err'] <= LOGPROB_TOL, rec
