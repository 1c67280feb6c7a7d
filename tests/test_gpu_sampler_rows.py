"""The sampler kernels on injected rows (tests/sampler_rows.py: the rows, the noise, the table, and which kernel path each case takes), through
Engine.sample and against oracle.hqt_oracle.sample_filtered.  Every call asserts first that the dumped logits ARE the injected rows, bit for bit.

1. kept-set readout, EXACT and SPLIT: probe noise names one token per draw; it wins iff it was kept.  Top-k membership is exact arithmetic: every
   probe counts.  A top-p probe counts if the reference gives the same winner under p (1 -+ 2^-20) (device and host expf need not agree to the last
   ulp); on the block rows (no libm in their probabilities) every probe counts.
2. random-noise draws, EXACT and SPLIT, eager and graph: codes equal the reference's on every well-conditioned draw (winner / runner-up >= 1.00001
   under p and p (1 -+ 2^-20)); at most 1 % of a case's draws may be excluded.
3. tie rule, all three precisions: two candidates with bit-equal ratios, the lower index wins -- in one float4, across lanes, waves, strides of one
   thread, with the lower index in the higher wave; FAST without a cut runs sampler_plain_fast_kernel<2 | 4 | 8>, with one sampler_kernel<.., true>.
4. the reference's own known answers (tests/golden/g1_sampler.npz: 6 rows x 6 settings, V = 512, a multiple of 4: no padding) through the EXACT
   kernel with the fixture's noise.  (Its rows are arbitrary fp32 values, which only EXACT's fp32 weights carry bit for bit.)
5. FAST: top-k membership by probe is exact at T in {0.5, 1} (the reciprocal is exact); top-p membership is asserted where the reference agrees with
   itself under p (1 -+ 2^-12) (derived: __expf's argument error at |x| ~ 80 is about 2^-18 relative); random-noise draws are gated at >= 99 %
   identical (helpers.gate; measured: profiles/sampler_rows_fast_gates.txt).
6. log-probabilities on the same rows against the fp64 log-softmax within tests/test_gpu_logprobs.py's bound 2^-24 (32 + 4 max|l|) -- and, since
   max|l| = 1e30 makes that bound empty on the rows with "never" entries, also with max|l| taken over the entries within 200 of the maximum (all
   others contribute exp(..) = 0 exactly on both sides, whatever their rounding).
7. the zero question: -0.0 behind the temperature division, where the reference's `logits < kth` treats the two zeros as equal."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from tests import sampler_rows as SR
from tests.helpers import gate, load
from tests.test_gpu_logprobs import all_codes, check_own, reference as logprob_reference

pytestmark = pytest.mark.gpu
VARIANT = {PRECISION_EXACT: 'f32', PRECISION_SPLIT: 'split', PRECISION_FAST: 'bf16'}
PNAME = {PRECISION_EXACT: 'exact', PRECISION_SPLIT: 'split', PRECISION_FAST: 'fast'}
ROWSET_IDS = [f'V{V}-{name}' for V, name in SR.ROWSETS]
DRAW_ROWSETS = [(V, name) for V, name in SR.ROWSETS if name in SR.DRAW_SETTINGS]
MAX_N = 4
FAST_DRAWS_BAR = 0.99


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return torch.from_numpy(np.array(a))              # a copy: the shared arrays are read-only


_ENGINES = {}


def engine_of(key, spec, weights, batch=SR.B):
    if key not in _ENGINES:
        assert torch.cuda.is_available(), 'these tests need the MI355X'
        os.environ['HQT_POISON_WORKSPACE'] = '1'      # every workspace buffer starts as NaN: a row no kernel wrote shows up
        try:
            e = Engine(spec, None, torch.device('cuda:0'), batch, MAX_N)
        finally:
            del os.environ['HQT_POISON_WORKSPACE']
        e.load(stage2=weights)
        e.finalize()
        _ENGINES[key] = e
    return _ENGINES[key]


def engine(V, name, variant):
    return engine_of((V, name, variant), *SR.model(V, name, variant))


def sampler_kw(setting):
    if 'table' in setting:
        return dict(row_samplers=SR.row_samplers(setting))
    return dict(top_k=setting['top_k'], top_p=setting['top_p'], temperature=setting['temperature'])


def run(eng, rows, n, noise, setting, precision, graph=False, batch=SR.B, **kw):
    """One call on an injected engine -> (codes_top, codes_bot[, logprobs]) as numpy, after the precondition: the logits are the injected rows."""
    out = eng.sample(batch, t_(SR.cond(batch)), n, precision=precision, noise=t_(noise), return_logits=True, use_graph=graph, **sampler_kw(setting), **kw)
    eng.range_check()
    torch.cuda.synchronize()
    lg = np_(out[2])
    assert lg.shape == (n, 5, batch, len(rows[0]))
    assert (lg[:, 0].view(np.uint32) == rows[0].view(np.uint32)).all(), 'the top logits are not the injected row'
    assert (lg[:, 1:].view(np.uint32) == rows[1].view(np.uint32)).all(), 'the bottom logits are not the injected row'
    return out


def mismatches(got, want, ok):
    bad = ok & (got != want)
    return [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(bad)[:8]], int(bad.sum())


def setting_of(V, name, sn):
    return dict(SR.ROWSETS[(V, name)][2])[sn]


# ------------------------------------------------------------------------------- 1. kept-set readout
def readout(V, name, precision, eps, counts):
    """Every setting of a row set under probe noise.  counts(level values) -> whether that level's probes are asserted."""
    variant = VARIANT[precision]
    rows, eng = SR.rows(V, name, variant), engine(V, name, variant)
    problems, asserted, total = [], 0, 0
    for sn, setting in SR.ROWSETS[(V, name)][2]:
        n, noise, want_t, want_b, ok_t, ok_b = SR.probe_case(V, name, variant, setting, eps, exact_blocks=precision != PRECISION_FAST)
        for s, members in SR.groups_of(setting):
            for level, ok in enumerate((ok_t, ok_b)):
                if not counts(*SR.level_values(s, level)):
                    ok[members] = False
        out = run(eng, rows, n, noise, setting, precision)
        for what, got, want, ok in (('top', np_(out[0]), want_t, ok_t), ('bottom', np_(out[1]), want_b, ok_b)):
            some, count = mismatches(got, want, ok)
            asserted, total = asserted + int(ok.sum()), total + ok.size
            if count:
                problems.append(f'{sn} {what}: {count} of {int(ok.sum())} probes differ; (index, got, reference): {some}')
    print(f'V{V}-{name} {PNAME[precision]}: {asserted} of {total} probes asserted, {len(problems)} problems')
    assert asserted > 0
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT], ids=['exact', 'split'])
@pytest.mark.parametrize('V,name', list(SR.ROWSETS), ids=ROWSET_IDS)
def test_kept_set_by_probe(V, name, precision):
    readout(V, name, precision, SR.EPS_EXACT, lambda T, k, p: True)


# ------------------------------------------------------------------------------- 2. random-noise draws
@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT], ids=['exact', 'split'])
@pytest.mark.parametrize('V,name', DRAW_ROWSETS, ids=[f'V{V}-{name}' for V, name in DRAW_ROWSETS])
def test_random_draws_equal_the_reference(V, name, precision):
    variant = VARIANT[precision]
    rows, eng = SR.rows(V, name, variant), engine(V, name, variant)
    problems = []
    for sn in SR.DRAW_SETTINGS[name]:
        if sn not in dict(SR.ROWSETS[(V, name)][2]):
            continue
        setting = setting_of(V, name, sn)
        noise, want_t, want_b, ok_t, ok_b = SR.draw_case(V, name, variant, setting, SR.EPS_EXACT)
        excluded = 1.0 - (ok_t.sum() + ok_b.sum()) / (ok_t.size + ok_b.size)
        assert excluded <= SR.MAX_EXCLUDED, f'{sn}: {excluded:.4f} of the draws are ill-conditioned'
        for graph in (False, True):
            out = run(eng, rows, SR.DRAW_N, noise, setting, precision, graph)
            for what, got, want, ok in (('top', np_(out[0]), want_t, ok_t), ('bottom', np_(out[1]), want_b, ok_b)):
                some, count = mismatches(got, want, ok)
                if count:
                    problems.append(f'{sn} graph={graph} {what}: {count} of {int(ok.sum())} draws differ; (index, got, reference): {some}')
    assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT, PRECISION_FAST], ids=['exact', 'split', 'fast'])
@pytest.mark.parametrize('V', SR.VOCABS)
def test_lower_index_wins_a_tie(V, precision):
    spec, w = SR.base_weights(V)
    row = SR.row_of(V, ('const',))
    eng = engine_of((V, 'const'), spec, SR.inject(w, row, row))
    pairs = SR.tie_pairs(V)
    assert len(pairs) <= SR.B
    q, want = SR.tie_noise(V, pairs, 5 * SR.B)
    noise, want = q.reshape(1, 5, SR.B, V), want.reshape(5, SR.B)
    problems = []
    for what, setting in (('no cut', SR._set()), ('top-k', SR._set(top_k=(V // 2, V // 2))),
                          ('table', SR._table(SR._set(), SR._set(top_k=(V // 2, V // 2)), SR._set(temperature=(0.5, 0.5))))):
        for graph in (False, True):
            out = run(eng, (row, row), 1, noise, setting, precision, graph)
            got = np.concatenate([np_(out[0]).reshape(SR.B, 1), np_(out[1]).reshape(SR.B, 4)], 1).T        # [5, B]
            for d, b in np.argwhere(got != want):
                problems.append(f'{what} graph={graph} draw {d}: candidates {pairs[(d * SR.B + b) % len(pairs)]}, winner {got[d, b]}')
    assert not problems, '\n'.join(problems[:20])


# ------------------------------------------------------------------------------- 4. the reference's known answers
def test_reference_known_answers():
    fx = load('g1_sampler.npz')
    cases = json.loads(str(fx['cases']))
    logits, q = fx['logits'], fx['noise']
    V = logits.shape[1]
    spec, w = SR.base_weights(V)
    problems = []
    for a in range(0, len(logits), 2):
        rows = (np.ascontiguousarray(logits[a]), np.ascontiguousarray(logits[a + 1]))
        eng = engine_of((V, 'g1', a), spec, SR.inject(w, *rows))
        noise = np.ones((1, 5, SR.B, V), np.float32)
        noise[0, 0], noise[0, 1:] = q[a], q[a + 1]
        for ci, (k, p, T) in enumerate(cases):
            for graph in (False, True):
                out = run(eng, rows, 1, noise, SR._set((k, k), (p, p), (T, T)), PRECISION_EXACT, graph)
                want = fx[f'index_{ci}']
                if not ((np_(out[0]) == want[a]).all() and (np_(out[1]) == want[a + 1]).all()):
                    problems.append(f'rows {a}, {a + 1} case {ci} {(k, p, T)} graph={graph}: drew {np_(out[0])[0, 0]}, {np_(out[1])[0, 0]}, the reference {want[a]}, {want[a + 1]}')
    assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------- 5. FAST
@pytest.mark.parametrize('V,name', list(SR.ROWSETS), ids=ROWSET_IDS)
def test_fast_kept_set_by_probe(V, name):
    readout(V, name, PRECISION_FAST, SR.EPS_FAST, lambda T, k, p: bool(p) or T in (0.5, 1.0))


@pytest.mark.parametrize('V,name', DRAW_ROWSETS, ids=[f'V{V}-{name}' for V, name in DRAW_ROWSETS])
def test_fast_random_draws_agree(V, name):
    rows, eng = SR.rows(V, name, 'bf16'), engine(V, name, 'bf16')
    for sn in SR.DRAW_SETTINGS[name]:
        if sn not in dict(SR.ROWSETS[(V, name)][2]):
            continue
        setting = setting_of(V, name, sn)
        noise, want_t, want_b, _, _ = SR.draw_case(V, name, 'bf16', setting, 0.0)
        for graph in (False, True):
            out = run(eng, rows, SR.DRAW_N, noise, setting, PRECISION_FAST, graph)
            same = ((np_(out[0]) == want_t).sum() + (np_(out[1]) == want_b).sum()) / (want_t.size + want_b.size)
            gate(f'sampler_rows.fast_draws(V{V}-{name},{sn},graph={graph})', same, FAST_DRAWS_BAR, '>=')


# ------------------------------------------------------------------------------- 6. log-probabilities
@pytest.mark.parametrize('V,name', list(SR.ROWSETS), ids=ROWSET_IDS)
def test_logprobs_on_the_rows(V, name):
    rows, eng = SR.rows(V, name, 'f32'), engine(V, name, 'f32')
    out = run(eng, rows, SR.DRAW_N, SR.draw_noise(V), SR._set(), PRECISION_EXACT, return_logprobs=True)
    check_own(out, 2, f'V{V}-{name}')
    # the same bound with max|l| over the entries that contribute: "never" entries add exp(..) = 0 exactly on both sides
    codes = all_codes(out[:2])
    want, _ = logprob_reference(np_(out[2]), codes)
    tol = np.empty(5)
    for d, row in enumerate((rows[0],) + (rows[1],) * 4):
        tol[d] = 2.0 ** -24 * (32.0 + 4.0 * np.abs(row[row >= row.max() - 200.0]).max())
    ratio = (np.abs(np_(out[3]).astype(np.float64) - want) / tol).max()
    print(f'V{V}-{name}: largest error / bound over the contributing entries {ratio:.3f}')
    assert ratio <= 1.0


# ------------------------------------------------------------------------------- 7. the zero question
ZERO_V, ZERO_K = 100, 8
ZERO_CASES = {'denormal': (np.float32(-1e-45), 2.0), 'normal': (np.float32(-1e-38), 1e10)}      # tiny negative logit / temperature -> -0.0


def zero_row(tiny):
    """ZERO_K zeros (the k-th largest is +0.0), eight tiny negative logits whose quotient by the temperature underflows to -0.0, "never" elsewhere."""
    row = np.full(ZERO_V, SR.NEVER, np.float32)
    row[[0, 5, 17, 33, 64, 65, 98, 99]] = 0.0
    row[[1, 4, 16, 34, 63, 66, 96, 97]] = tiny
    return row


@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT, PRECISION_FAST], ids=['exact', 'split', 'fast'])
@pytest.mark.parametrize('case', list(ZERO_CASES))
def test_negative_zero_behind_the_temperature(case, precision):
    """The reference masks `logits < kth`: -0.0 < +0.0 is false, so a logit that became -0.0 stays in the top-k set when the k-th largest is +0.0.
    The kernels' radix key orders -0.0 below +0.0; they canonicalise the zero first.  The reference is evaluated on the logits the call dumped: the
    denormal travels through EXACT's head GEMM only (SPLIT's fp16 planes and FAST's bf16 weights cannot carry it; the normal one they can)."""
    tiny, T = ZERO_CASES[case]
    variant = VARIANT[precision]
    row = SR.ROUND[variant](zero_row(tiny)) + np.float32(0.0)
    spec, w = SR.base_weights(ZERO_V)
    eng = engine_of(('zero', case, variant), spec, SR.inject(w, row, row))
    tiny_at = np.flatnonzero(zero_row(tiny) == tiny)
    q, tok = SR.probe_noise(ZERO_V, list(tiny_at) + [0, 5, 99, 2], 5 * SR.B)
    noise = q.reshape(1, 5, SR.B, ZERO_V)
    setting = SR._set(top_k=(ZERO_K, ZERO_K), temperature=(T, T))
    out = eng.sample(SR.B, t_(SR.cond()), 1, precision=precision, noise=t_(noise), return_logits=True, use_graph=False, **sampler_kw(setting))
    eng.range_check()
    torch.cuda.synchronize()
    lg = np_(out[2])
    assert (lg == lg[0, 0, 0]).all(), 'every draw sees the same row'
    dumped = lg[0, 0, 0]
    carried = bool((dumped.view(np.uint32) == row.view(np.uint32)).all())
    quotient = (dumped / np.float32(T)).astype(np.float32)
    print(f'{case} {PNAME[precision]}: injected row carried bit for bit: {carried}; dumped tiny logits {dumped[tiny_at][:2]}, '
          f'host quotient is -0.0 at {int(np.signbit(quotient[tiny_at]).sum())} of {len(tiny_at)}')
    if case == 'normal' or precision == PRECISION_EXACT:
        assert carried
    want, _ = SR.ref_draws(dumped, q, T, ZERO_K, None)
    got = np.concatenate([np_(out[0]).reshape(SR.B, 1), np_(out[1]).reshape(SR.B, 4)], 1).T.reshape(-1)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f'probe of token {tok[bad][:8]}: drew {got[bad][:8]}, the reference {want[bad][:8]}'
    if carried and case == 'normal':
        assert (want[np.isin(tok, tiny_at)] == tok[np.isin(tok, tiny_at)]).all(), 'the reference keeps the -0.0 tokens'
