"""Shared by tests/test_draw_report_host.py and tests/test_gpu_draw_report.py: what hqt_set_draw_report reports, restated in numpy from a given fp32 logits
row -- the order (logit descending, index ascending, float compares), the rank of a code, the entropy and the log-probabilities in fp64 -- and a float32
emulation of the kernel's entropy formula H = logf(S) - T / S in its reduction order (256 threads, float4 groups t, t + 256, ...: per group (x + y) + (z + w),
per thread a pairwise tree over its groups, the xor butterfly of the 64 lanes, the four wave sums as (w0 + w1) + (w2 + w3)).

ENTROPY GATE (derived, not measured).  With H = log S - T / S: |T / S| <= H + |log S| <= 2 ln 16384 ~ 19.4; S and T each carry a few ulp of expf plus a
pairwise tree of depth <= 14, about 20 * 2^-24 relative; so the absolute error stays below about 5e-5 and the gate is 2e-4 absolute against the fp64 value.
The host test holds the emulation to a quarter of it on every row family the GPU test injects."""
import numpy as np

from tests import sampler_rows as SR

F32 = np.float32
ENTROPY_GATE = 2e-4
VOCABS = (100, 1000, 4096, 8192, 16384)
MAX_TOP = 16
# the rows the GPU test feeds the kernels; 'zeros' is the row with -0.0 next to +0.0 (zeros_row).  PAIRS: the (top family, bottom family) of one injected
# model -- all but 'zeros', which no head can return (a dot product adds +0.0 to a -0.0 term): that row goes to the kernel directly
FAMILIES = {'const': ('const',), 'quant': ('quant',), 'tierun': ('tierun', 5), 'block': ('block', 32), 'heavy': ('heavy',), 'steep': ('steep',),
            'zeros': ('zeros',)}
PAIRS = (('const', 'tierun'), ('quant', 'block'), ('heavy', 'steep'))


def zeros_row(V):
    """-0.0 next to +0.0 at the top of the row: both zeros at indices inside one float4, in neighbouring ones, in two groups of one thread, first and last index;
    everything else is negative, so the top-16 is decided among the zeros by index alone."""
    rng = np.random.default_rng([912, V])
    row = -(1.0 + np.round(8.0 * rng.random(V)) / 4.0).astype(F32)
    minus = [0, 2, 5, 64, V - 1] + ([1024 + 1] if V > 1030 else [])
    plus = [1, 3, 4, 65, V - 2] + ([1024] if V > 1030 else [])
    row[plus] = F32(0.0)
    row[minus] = F32(-0.0)
    assert np.signbit(row[minus]).all() and not np.signbit(row[plus]).any()
    row.setflags(write=False)
    return row


def family_row(V, name):
    if name == 'zeros':
        return zeros_row(V)
    fam = FAMILIES[name]
    if name == 'block':
        fam = ('block', min(32, V))
    return SR.row_of(V, fam, 'f32')


def order(row):
    """Indices by (value descending, index ascending): -0.0 and +0.0 compare equal, so the lower index comes first."""
    row = np.asarray(row, F32)
    assert not np.isnan(row).any()
    return np.argsort(-row, kind='stable')


def rank(row, c):
    row = np.asarray(row, F32)
    return int((row > row[c]).sum() + (row[:c] == row[c]).sum())


def ranks(row, codes):
    return np.array([rank(row, int(c)) for c in np.asarray(codes).reshape(-1)], np.int32).reshape(np.shape(codes))


def entropy64(row):
    l = np.asarray(row, F32).astype(np.float64)
    d = l - l.max()
    e = np.exp(d)
    S = e.sum()
    return float(np.log(S) - (e * d).sum() / S)


def logprobs64(row):
    l = np.asarray(row, F32).astype(np.float64)
    d = l - l.max()
    return d - np.log(np.exp(d).sum())


def g4_of(V):
    return 4 if V <= 4096 else 8 if V <= 8192 else 16


def entropy32(row):
    """The kernel's formula in float32, in its order of operations (numpy's float32 exp / log stand in for IEEE expf / logf)."""
    row = np.asarray(row, F32)
    V, G4 = len(row), g4_of(len(row))
    assert V % 4 == 0 and V <= 1024 * G4
    m = row.max()
    pad = np.zeros(1024 * G4, F32)
    valid = np.zeros(1024 * G4, bool)
    pad[:V], valid[:V] = row, True
    d = (pad - m).astype(F32).reshape(G4, 256, 4)                 # element (k, tid, e) is index 4 (tid + 256 k) + e
    valid = valid.reshape(G4, 256, 4)
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        e = np.where(valid, np.exp(d, dtype=F32), F32(0.0)).astype(F32)
        p = np.where(valid, (e * d).astype(F32), F32(0.0)).astype(F32)

    def reduce(x):
        x = ((x[..., 0] + x[..., 1]).astype(F32) + (x[..., 2] + x[..., 3]).astype(F32)).astype(F32)        # [G4, 256]
        w = 1
        while w < G4:
            x[0::2 * w] = (x[0::2 * w] + x[w::2 * w]).astype(F32)
            w *= 2
        lanes = x[0].reshape(4, 64).copy()
        off = 32
        while off:
            lanes = (lanes + lanes[:, np.arange(64) ^ off]).astype(F32)
            off >>= 1
        ws = lanes[:, 0]
        return F32(F32(ws[0] + ws[1]) + F32(ws[2] + ws[3]))
    S, T = reduce(e), reduce(p)
    return float(F32(np.log(S, dtype=F32)) - F32(T / S))


def check_rows(logits, codes, report, top_n, what, gate=ENTROPY_GATE):
    """A report against the rows it was computed from.  logits fp32 [n, draws, B, V] (the layout of logits_out), codes int [B, n, draws] (the fed-forward
    codes), report = (entropy, rank, top_codes, top_logprobs) as numpy [B, n, draws(, top_n)].  Order and rank are exact; the entropy is within the gate of
    the fp64 value; top_logprobs within the log-probability bound of tests/test_gpu_logprobs.py (their BITS are pinned elsewhere, against forced calls).
    Returns the largest entropy error."""
    entropy, rk, tc, tl = report
    n, draws, B, V = logits.shape
    worst = 0.0
    for t in range(n):
        for d in range(draws):
            for b in range(B):
                row, c = logits[t, d, b], int(codes[b, t, d])
                o = order(row)
                assert rk[b, t, d] == rank(row, c), f'{what}: rank at (b={b}, t={t}, draw={d}): {rk[b, t, d]}, reference {rank(row, c)}'
                if top_n:
                    assert (tc[b, t, d] == o[:top_n]).all(), f'{what}: top codes at (b={b}, t={t}, draw={d}): {tc[b, t, d].tolist()}, reference {o[:top_n].tolist()}'
                    lp = logprobs64(row)[o[:top_n]]
                    tol = 2.0 ** -24 * (32.0 + 4.0 * float(np.abs(row.astype(np.float64)).max()))
                    assert np.abs(tl[b, t, d].astype(np.float64) - lp).max() <= tol, f'{what}: top log-probabilities at (b={b}, t={t}, draw={d})'
                    if rk[b, t, d] < top_n:
                        assert tc[b, t, d, rk[b, t, d]] == c
                err = abs(float(entropy[b, t, d]) - entropy64(row))
                worst = max(worst, err)
    print(f'{what}: largest entropy error {worst:.3e} (gate {gate})')
    assert worst <= gate, f'{what}: entropy error {worst:.3e} above the gate {gate}'
    return worst
