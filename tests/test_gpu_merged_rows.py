"""Merged passes at ragged row counts, one case per branch of the tile GEMMs' plan (tests/merged_rows_cases.py: which model reaches which geometry, split-K
factor and tile order; tests/test_tile_plan_host.py proves the reach on the real plan function), through the C ABI and against the CPU oracle.  Every engine
starts on a NaN-poisoned workspace and runs under the throughput policy, eager under the variant counters and then from the graph.

EXACT and SPLIT: codes bit-identical, logits within 2e-4, all finite, range_check clean; SPLIT served every launch above 256 rows on split_gemm_kernel.
FAST: teacher-forced on the oracle's codes; every logit finite -- a call holds fewer rows than packed_mb rounds up to and the pad rows are NaN, so this also
says that no pad row leaked into a real one --; the counted variants are exactly the case's record (tag, geometry suffix, splitkS per GEMM).  The tile
kernels' bf16 error is not gated by a figure of their own: a second engine created under HQT_NO_TILE_GEMM runs the same call on the streaming kernels
(separate code, gated since before the tile kernels existed), and tile max |error| <= 1.5 x streaming max, tile mean |error| <= 1.1 x streaming mean, both
paths under the suite's blanket 0.15.  (The project's one joint measurement, at 2048 rows: 0.077 / 0.0105 tile against 0.081 / 0.0105 streaming; the maximum
over a few million logits is a noisy extreme, the mean is stable and a lost or doubled product term moves it by far more than 10 %.)  The recorded run:
profiles/merged_rows_fast_gates.txt."""
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd._lib import POLICY_THROUGHPUT, PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from tests import merged_rows_cases as MR
from tests.helpers import gate

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
FAST_BLANKET = 0.15
MAX_RATIO, MEAN_RATIO = 1.5, 1.1


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return torch.from_numpy(np.array(a))          # a copy: the shared oracle arrays are read-only


_ENGINES = {}


def engine(name, streaming=False):
    """One poisoned engine per (case, GEMM family), shared by the tests of this module; streaming: created under HQT_NO_TILE_GEMM."""
    spec, weights, cond, noise, B, n = MR.inputs(name)
    if (name, streaming) not in _ENGINES:
        assert torch.cuda.is_available(), 'these tests need the MI355X'
        os.environ['HQT_POISON_WORKSPACE'] = '1'          # every workspace buffer starts as NaN: a row no kernel wrote shows up
        if streaming:
            os.environ['HQT_NO_TILE_GEMM'] = '1'
        try:
            e = Engine(spec, None, torch.device('cuda:0'), B, n)
        finally:
            del os.environ['HQT_POISON_WORKSPACE']
            os.environ.pop('HQT_NO_TILE_GEMM', None)
        e.load(stage2=weights)
        e.finalize()
        e.set_policy(POLICY_THROUGHPUT)
        _ENGINES[(name, streaming)] = e
    return _ENGINES[(name, streaming)]


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


def gemm_variants(v):
    return {k: c for k, c in v.items() if k.split(':')[-1].startswith('gemm_') and k.split(':')[-1] != 'gemm_combine'}


def run_exact_or_split(name, precision):
    """The free run of a case, eager (counted) and from the graph -> one record per run."""
    spec, weights, cond, noise, B, n = MR.inputs(name)
    ct, cb, lg, _ = MR.oracle(name)
    eng = engine(name)
    recs = []
    for graph in (False, True):
        call = lambda: eng.sample(B, t_(cond), n, precision=precision, noise=t_(noise), return_logits=True, use_graph=graph)
        out, v = timed(eng, call) if not graph else (call(), None)
        eng.range_check()
        torch.cuda.synchronize()
        got = np_(out[2])
        rec = dict(case=name, precision=precision, graph=graph, codes_equal=bool((np_(out[0]) == ct).all() and (np_(out[1]) == cb).all()),
                   finite=bool(np.isfinite(got).all()), logit_err=float(np.abs(got - lg).max()))
        if v is not None:
            rec['variants'] = gemm_variants(v)
        print(rec)
        recs.append(rec)
    return recs


@pytest.mark.parametrize('name', list(MR.CASES))
def test_exact_codes_and_logits_vs_oracle(name):
    for rec in run_exact_or_split(name, PRECISION_EXACT):
        assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL, rec
        assert rec['codes_equal'], rec


@pytest.mark.parametrize('name', list(MR.CASES))
def test_split_codes_and_logits_vs_oracle(name):
    spec, B = MR.CASES[name]
    # SPLIT runs the EXACT launch sequence (a full qkv GEMM in depth sub-step 0 too): per position 4 + 5 + 5 nn.Linear launches, those above 256 rows on
    # the fp16 hi / lo matrix path
    above = sum(k * (rows > 256) for k, rows in ((4, B), (5, B), (5, 4 * B)))
    for rec in run_exact_or_split(name, PRECISION_SPLIT):
        assert rec['finite'] and rec['logit_err'] <= LOGIT_TOL, rec
        assert rec['codes_equal'], rec
        if 'variants' in rec:
            v = rec['variants']
            split = {k: c for k, c in v.items() if k.startswith('variant:split_gemm')}
            assert sum(split.values()) == above * MR.N_POSITIONS, rec
            print(f'{name}: K-slice counts of the SPLIT launches: { {k: c for k, c in split.items() if "kslices" in k} }')


def run_fast(name, streaming):
    """Teacher-forced FAST on the oracle's codes, eager (counted) and from the graph, on the tile kernels or (streaming) on the engine without them."""
    spec, weights, cond, noise, B, n = MR.inputs(name)
    ct, cb, lg, _ = MR.oracle(name)
    eng = engine(name, streaming)
    recs = []
    for graph in (False, True):
        call = lambda: eng.sample(B, t_(cond), n, precision=PRECISION_FAST, noise=t_(noise), force_top=t_(ct), force_bot=t_(cb), return_logits=True, use_graph=graph)
        out, v = timed(eng, call) if not graph else (call(), None)
        eng.range_check()
        torch.cuda.synchronize()
        lf = np_(out[2])
        finite = bool(np.isfinite(lf).all())
        err = np.abs(lf.astype(np.float64) - lg) if finite else None
        rec = dict(case=name, streaming=streaming, graph=graph, finite=finite, rows_nonfinite=int((~np.isfinite(lf)).any(axis=(0, 1, 3)).sum()),
                   max_err=float(err.max()) if finite else float('nan'), mean_err=float(err.mean()) if finite else float('nan'))
        if v is not None:
            rec['variants'] = gemm_variants(v)
        print(rec)
        recs.append(rec)
    return recs


@pytest.mark.parametrize('name', list(MR.CASES))
def test_fast_tile_kernels_vs_oracle_and_vs_the_streaming_kernels(name):
    tile, stream = run_fast(name, False), run_fast(name, True)
    assert all(r['finite'] for r in tile), tile
    assert all(r['finite'] for r in stream), stream                      # the streaming kernels at ragged rows above 256 are part of what this checks
    assert tile[0]['variants'] == MR.expected_fast_variants(name), tile[0]['variants']
    assert not any(k.startswith('variant:tile_gemm') for k in stream[0]['variants']) and sum(stream[0]['variants'].values()) == 14 * MR.N_POSITIONS, stream[0]['variants']
    for t, s in zip(tile, stream):
        tag = f'merged_rows.fast_logits({name},graph={t["graph"]})'
        gate(f'{tag}.streaming_max', s['max_err'], FAST_BLANKET)
        gate(f'{tag}.streaming_mean', s['mean_err'], FAST_BLANKET)
        gate(f'{tag}.tile_max', t['max_err'], min(MAX_RATIO * s['max_err'], FAST_BLANKET))
        gate(f'{tag}.tile_mean', t['mean_err'], MEAN_RATIO * s['mean_err'])
