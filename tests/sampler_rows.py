"""Shared by tests/test_sampler_rows_host.py and tests/test_gpu_sampler_rows.py: chosen logits rows and chosen noise for the sampler kernels of
csrc/kernels.hip (sampler_kernel<256|1024, exact|fast-math>, sampler_plain_fast_kernel<2|4|8>), fed through the public ABI.

INJECTION.  The heads have no bias and each has its own LayerNorm: with ln_X.weight = 0, ln_X.bias = e_0 and head_X.weight = row (x) e_0 every logits
row of head X, for every sample and position, IS `row`, bit for bit -- the LayerNorm output is exactly e_0 and the dot product adds exact zeros.  One
D = 64, 1 + 1 layer model (offgrid_cases.sweep_spec) carries two rows, one per head (a ROWSET).  Injected values are finite (0 * inf is NaN): NEVER =
-1e30 stands for "never".  FAST keeps its weights in bf16 and SPLIT as fp16 hi + lo / 2048 planes, so a FAST engine gets the 'bf16' variant of a row
set and a SPLIT engine the 'split' one: the same families built on the bf16 grid, or on 22 significant bits inside the fp16 range (-60000 is "never" there).  Every GPU test asserts `return_logits` == the injected rows before it concludes anything.

NOISE.  The explicit noise input makes the kept set observable: q = 1 everywhere but q[j] = 2^-100 lets token j win if and only if it was kept with
a non-zero probability, else the head wins (probe_noise).  Equal logits under equal noise give bit-equal ratios in every precision: q = 1 at two
indices and 2 elsewhere on a constant row makes exactly those two the candidates, and the lower index has to win (tie_noise).

REFERENCE.  oracle.hqt_oracle.sample_filtered (cutoff_topk_logits, cutoff_topp_probs inside it) on the injected row; nothing of it is restated
here.  It is evaluated on the row once per setting (its second result, the probabilities) and the draw of every noise row is argmax(p / q), the line
tests/test_oracle_golden.py::test_multinomial_is_argmax_p_over_q pins; the host tests hold that shortcut against sample_filtered's own index.  The
reference raises for top_k > V (torch.topk); the kernels cut nothing from top_k >= V on, which is what top_k = V gives in the reference, so that is
the expectation for V + 1 too.

ROW FAMILIES (row_of): heavy (Cauchy x 3), flat (sigma 1e-3), steep (sigma 30), quant (quarters: many exact ties), block (m zeros among NEVER: every
probability is exactly 1 / m), ulp (the k-th and (k+1)-th largest differ by `gap` ulps: gap 1, 2^10 and 2^18 let the radix select decide in its
fourth, third and second pass, block's 0 against -1e30 in the first), tierun (the k-th value shared by a run of equal entries at index 0, V - 1 and
on both sides of multiples of 4, 64, 256 and 1024), const (all equal: the tie rows).  m is a power of two (every prefix sum of 1 / m is exact), or
3 * 2^a ('block3': 1 / m is rounded once, by an IEEE division, and every prefix j * fl(1 / m) is exact in double, so the cut at p = fl32(j * fl(1 / m))
is decided by exact arithmetic on both sides, with no libm in it -- and sits where a prefix accumulated in fp32 rounds differently)."""
import functools
import math

import numpy as np

from oracle.hqt_oracle import OracleStage2, cutoff_topk_logits, cutoff_topp_probs, sample_filtered, softmax
from tests import offgrid_cases as OG

F32 = np.float32
NEVER = F32(-1e30)
SPLIT_MAX = 60000.0               # SPLIT carries weights as fp16 planes: its rows stay inside the fp16 range, and -60000 is its "never"
B = 64
VOCABS = (100, 1000, 2048, 3000, 4096, 8192, 16384)
TOP_P_MAX_V = 8192                # hqt_sample refuses top-p above
EPS_EXACT = 2.0 ** -20            # a top-p probe / draw counts if it holds under p (1 -+ this): device and host expf need not agree to the last ulp
EPS_FAST = 2.0 ** -12             # FAST: __expf's argument error at |x| ~ 80 is about 2^-18 relative; 40 x margin
MIN_REL_P = 2.0 ** -60            # probe tokens: zero, or at least this share of the largest probability (the ratio p / 2^-100 can neither tie nor overflow)
PROBE_Q = F32(2.0 ** -100)
MAX_PROBES = 128                  # per level of a case: two positions of the top draw, one of the four bottom draws
MIN_MARGIN = OG.MIN_MARGIN
MAX_EXCLUDED = 0.01               # share of a case's random draws that may be ill-conditioned
WEIGHT_SEED = 910


def bf16_round(a):
    """fp32 -> the nearest bf16 value (ties to even), as fp32."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split_planes(a):
    """split2 of csrc/split_device.h, put together again: fp16(x) + fp16((x - fp16(x)) * 2048) / 2048, in fp32."""
    a = np.ascontiguousarray(a, F32)
    hi = a.astype(np.float16).astype(F32)
    return hi + ((a - hi) * F32(2048.0)).astype(np.float16).astype(F32) / F32(2048.0)


def split_round(a):
    """fp32 -> a value inside the fp16 range that SPLIT's fp16 hi + lo / 2048 planes carry exactly: 22 significant bits where fp16(x) is a normal number."""
    return split_planes(split_planes(np.clip(a, -SPLIT_MAX, SPLIT_MAX)))


ROUND = {'f32': lambda a: np.asarray(a, F32), 'bf16': bf16_round, 'split': split_round}
ULP = {'f32': lambda n: n, 'split': lambda n: 4 * n, 'bf16': lambda n: min(n, 64) << 16}      # (bf16: at most 64 of its ulps, half a binade)


def step_down(x, ulps, variant):
    """The positive float `ulps` units in the last place of the variant's grid below x."""
    u = np.array([x], F32).view(np.uint32)
    assert x > 0
    return (u - np.uint32(ULP[variant](ulps))).view(F32)[0]


def pow2_below(V):
    return 1 << (V - 1).bit_length() - 1


def tierun_indices(V):
    idx = {0, V - 1}
    for m in (4, 64, 256, 1024):
        if m < V:
            idx |= {m - 1, m}
    return np.array(sorted(idx))


@functools.lru_cache(maxsize=None)
def row_of(V, family, variant='f32'):
    """The row of a family spec (name, *parameters), fp32 [V], read-only.  variant: 'f32' any fp32 value (EXACT), 'bf16' values FAST's bf16 weights carry,
    'split' values SPLIT's fp16 hi / lo planes carry."""
    name, args = family[0], family[1:]
    rng = np.random.default_rng([WEIGHT_SEED, V, sum(map(ord, name))] + [int(a) for a in args])
    rnd = ROUND[variant]
    if name == 'heavy':
        row = rnd(3.0 * rng.standard_cauchy(V))
    elif name == 'flat':
        row = rnd(1e-3 * rng.standard_normal(V))
    elif name == 'steep':
        row = rnd(30.0 * rng.standard_normal(V))
    elif name == 'quant':
        row = rnd(np.round(8.0 * rng.standard_normal(V)) / 4.0)            # quarters up to |l| ~ 8: exact in bf16 too
    elif name == 'const':
        row = np.full(V, 0.5, F32)
    elif name == 'block':                                                  # (m[, another placement]): m zeros, index 0 and V - 1 among them
        m = args[0]
        assert 2 <= m <= V
        at = np.concatenate([[0, V - 1], 1 + rng.permutation(V - 2)[:m - 2]])
        row = np.full(V, NEVER, F32)
        row[at] = 0.0
    elif name == 'ulp':                                                    # (k, gap)
        k, gap = args
        s = np.sort(rnd(8.0 + 2.0 * rng.standard_normal(V)))[::-1].copy()
        assert 1 <= k < V and s[k - 1] > 1.0
        y = step_down(s[k - 1], gap, variant)
        s[k:] = np.minimum(s[k:], y)
        s[k] = y
        row = s[rng.permutation(V)]
    elif name == 'tierun':                                                 # (k,): k >= 2; the run holds the (k - 1)-th .. largest
        k, = args
        at = tierun_indices(V)
        row = rnd(2.0 * rng.standard_normal(V))
        rest = np.setdiff1d(np.arange(V), at)
        s = np.sort(row[rest])[::-1]
        assert 2 <= k <= len(rest)
        x = s[k - 2]                                                       # at most k - 2 entries above the run, which holds the k-th largest with >= 1 other entry
        row[at] = x
    else:
        raise KeyError(name)
    row = rnd(np.ascontiguousarray(row, F32)) + F32(0.0)                       # (-0.0 cannot be injected: the dot product adds +0.0 to it)
    assert np.isfinite(row).all() and (rnd(row) == row).all() and (variant != 'split' or (split_planes(row) == row).all())
    row.setflags(write=False)
    return row


# ----------------------------------------------------------------------------- the table
def _set(top_k=(None, None), top_p=(None, None), temperature=(1.0, 1.0)):
    return dict(top_k=tuple(top_k), top_p=tuple(top_p), temperature=tuple(temperature))


def _table(*groups):
    """A row-sampler table: sample b takes groups[b % len(groups)]."""
    return dict(table=tuple(groups))


def _rowsets(V):
    """name -> (top family, bottom family, [(setting name, setting)])."""
    k3, m, top_p = V // 3, pow2_below(V), V <= TOP_P_MAX_V
    m3 = 3 * pow2_below(V // 3 + 1) if V >= 12 else 3                      # the largest 3 * 2^a <= V
    c3 = float(F32(1.0) / F32(m3))
    generic = [('plain', _set(temperature=(1.0, 0.7))),
               ('k', _set(top_k=(k3, 2), temperature=(1.0, 1.3))),
               ('k-edge', _set(top_k=(1, V - 1), temperature=(0.5, 1.0))),
               ('k-over', _set(top_k=(V, V + 1)))]
    if top_p:
        generic += [('p', _set(top_p=(0.9, 0.5), temperature=(1.0, 0.7))),
                    ('p-edge', _set(top_p=(1.0, 1e-6))),
                    ('p-wide', _set(top_p=(0.999, 0.999), temperature=(1.3, 0.5))),
                    ('kp', _set(top_k=(k3, k3), top_p=(0.999, 0.9), temperature=(0.5, 1.3))),
                    ('table', _table(_set(), _set(top_k=(k3, 2), temperature=(1.0, 1.3)), _set(top_p=(0.9, 0.5), temperature=(1.0, 0.7))))]
    else:
        generic += [('table', _table(_set(), _set(top_k=(k3, 2), temperature=(1.0, 1.3)), _set(top_k=(1, V - 1), temperature=(0.5, 1.0))))]
    block = [('k', _set(top_k=(m // 2, k3)))]
    if top_p:
        block += [('p-quarter', _set(top_k=(None, k3 + 1), top_p=(0.25, None))),
                  ('p-one', _set(top_k=(None, k3 - 1), top_p=(1.0, 0.9))),
                  ('p-last', _set(top_k=(None, k3), top_p=((m - 1) / m, 0.999))),
                  ('p-first', _set(top_k=(None, k3), top_p=(1.0 / m, 0.5), temperature=(0.5, 0.5))),
                  ('table', _table(_set(top_k=(m // 2, k3)), _set(top_k=(None, k3), top_p=(0.25, 0.9)), _set(top_k=(None, k3 + 1))))]
    else:
        block += [('k-more', _set(top_k=(m - 1, k3 + 1))), ('k-less', _set(top_k=(2, k3 - 1), temperature=(0.5, 0.5))),
                  ('table', _table(_set(top_k=(m // 2, k3)), _set(top_k=(1, k3 + 1)), _set()))]
    ties = [('k', _set(top_k=(k3, k3))), ('k-off', _set(top_k=(k3 - 1, k3 + 1))), ('k-half', _set(top_k=(k3, k3), temperature=(0.5, 0.5)))]
    if top_p:
        ties += [('kp', _set(top_k=(k3, k3), top_p=(0.9, 0.9))),
                 ('table', _table(_set(top_k=(k3, k3)), _set(), _set(top_k=(k3, k3), top_p=(0.9, 0.5))))]
    else:
        ties += [('table', _table(_set(top_k=(k3, k3)), _set(), _set(top_k=(k3 - 1, k3 + 1))))]
    sets = {'hf': (('heavy',), ('flat',), generic),
            'sq': (('steep',), ('quant',), generic),
            'bu': (('block', m), ('ulp', k3, 1), block),
            'tg': (('tierun', k3), ('ulp', k3, 1 << (10 if VOCABS.index(V) % 2 else 18)), ties)}
    if top_p:
        # prefixes of fl(1 / m3): p = fl32(j c) for several j, on both levels (the bottom row is the same block at another place)
        js = [j for j in (3, m3 // 7, m3 // 3 + 1, m3 // 2 + 5, m3 - m3 // 5, m3 - 1) if 1 <= j < m3]
        ps = [float(F32(np.float64(c3) * j)) for j in js]
        block3 = [(f'p{a}', _set(top_p=(ps[a], ps[a + 1]))) for a in range(0, len(ps) - 1, 2)]
        block3 += [(f'q{a}', _set(top_p=(ps[a + 1], ps[a]))) for a in range(0, len(ps) - 1, 2)]
        sets['b3'] = (('block', m3), ('block', m3, 1), block3)
    return sets


ROWSETS = {(V, name): rs for V in VOCABS for name, rs in _rowsets(V).items()}
EXACT_BLOCKS = ('block',)         # families whose probabilities involve no libm: no top-p probe of theirs is excluded


def setting_of(setting, b):
    """The (top_k, top_p, temperature) pairs sample b draws with."""
    return setting['table'][b % len(setting['table'])] if 'table' in setting else setting


def row_samplers(setting, batch=B):
    """Engine.sample's row_samplers argument of a table setting, else None."""
    if 'table' not in setting:
        return None
    return [(s['temperature'], s['top_k'], s['top_p']) for s in (setting_of(setting, b) for b in range(batch))]


def groups_of(setting, batch=B):
    """[(setting, the samples that draw with it)]."""
    if 'table' not in setting:
        return [(setting, np.arange(batch))]
    n = len(setting['table'])
    return [(setting['table'][g], np.arange(g, batch, n)) for g in range(n)]


def rows(V, name, variant):
    top, bot, _ = ROWSETS[(V, name)]
    return row_of(V, top, variant), row_of(V, bot, variant)


def inject(weights, row_top, row_bot):
    """A copy of stage-2 weights whose two heads return the given rows whatever their input."""
    w = {k: np.array(v, F32) for k, v in weights.items()}
    for head, row in (('top', row_top), ('bot', row_bot)):
        w[f'ln_{head}.weight'][:] = 0.0
        w[f'ln_{head}.bias'][:] = 0.0
        w[f'ln_{head}.bias'][0] = 1.0
        w[f'head_{head}.weight'][:] = 0.0
        w[f'head_{head}.weight'][:, 0] = row
    return w


@functools.lru_cache(maxsize=None)
def base_weights(V):
    from hqtransformer_amd import synth
    spec = OG.sweep_spec(V)
    return spec, synth.stage2_weights(spec, WEIGHT_SEED, 'fixture')


def model(V, name, variant):
    """(spec, weights with the row set injected)."""
    spec, w = base_weights(V)
    return spec, inject(w, *rows(V, name, variant))


def cond(batch=B):
    return np.arange(batch) % 10


# ----------------------------------------------------------------------------- the reference
def eff_k(k, V):
    return None if not k or k >= V else int(k)


def ref_probs(row, T, k, p):
    """sample_filtered's probabilities of one row [V] under (temperature, top_k, top_p)."""
    V = len(row)
    return sample_filtered(row[None], np.ones((1, V), F32), T, eff_k(k, V), p or None)[1][0]


def ref_draws(row, q, T, k, p):
    """The reference's draws of one row under the noise rows q [..., V] -> (codes [...], winner / runner-up ratio [...])."""
    ratio = ref_probs(row, T, k, p) / q
    part = np.partition(ratio, -2, axis=-1)
    with np.errstate(over='ignore'):
        return np.argmax(ratio, axis=-1).astype(np.int64), part[..., -1] / np.maximum(part[..., -2], F32(1e-38))


def perturbed(p, eps):
    return [None] if not p else [p, p * (1.0 - eps), p * (1.0 + eps)]


def robust_draws(row, q, T, k, p, eps, margin=1.0):
    """(codes, ok): ok where the same code wins, by at least `margin`, under p and under p (1 -+ eps)."""
    code, ok = None, None
    for pp in perturbed(p, eps):
        c, mg = ref_draws(row, q, T, k, pp)
        good = mg >= margin
        code, ok = (c, good) if code is None else (code, ok & good & (c == code))
    return code, ok


def level_values(setting, level):
    return setting['temperature'][level], setting['top_k'][level], setting['top_p'][level]


# ----------------------------------------------------------------------------- probes
def probe_tokens(row, T, k, p):
    """Tokens whose membership in the kept set a case reads out: ranks k - 3 .. k + 3 of the top-k order, every member of the tie run at the
    threshold, sorted positions first - 3 .. first + 3 of the top-p cut, the head, the last non-zero token, indices 0 and V - 1."""
    V = len(row)
    k = eff_k(k, V)
    lg = (row / F32(T)).astype(F32)
    pr = softmax(cutoff_topk_logits(lg[None], k))[0]
    by_p = np.argsort(-pr, kind='stable')
    cnt = int((pr > 0).sum())
    toks = [0, V - 1, int(by_p[0]), int(by_p[cnt - 1])]
    if k:
        by_l = np.argsort(-lg, kind='stable')
        toks += [int(by_l[r]) for r in range(max(k - 4, 0), min(k + 3, V))]
    if p:
        kept = cutoff_topp_probs(pr[None], p)[0] > 0
        first = int(kept[by_p[:cnt]].sum()) - 1                            # the last kept sorted position
        toks += [int(by_p[r]) for r in range(max(first - 3, 0), min(first + 4, cnt))]
    if k:
        toks += [int(i) for i in np.flatnonzero(lg == lg[by_l[k - 1]])]
    toks = list(dict.fromkeys(toks))[:MAX_PROBES]                          # (a block row's run of thousands is read as far as the pass has room)
    # a probe is zero in the reference (the head has to win) or far above the underflow range
    final = ref_probs(row, T, k, p)
    return [t for t in toks if final[t] == 0 or final[t] >= MIN_REL_P * final.max()]


def probe_noise(V, tokens, rows_):
    """[rows_, V]: row r probes tokens[r % len(tokens)] -> (noise, the token of every row)."""
    tok = np.array([tokens[r % len(tokens)] for r in range(rows_)])
    q = np.ones((rows_, V), F32)
    q[np.arange(rows_), tok] = PROBE_Q
    return q, tok


def probe_case(V, name, variant, setting, eps, batch=B, exact_blocks=True):
    """The probe pass of a case: (n, noise [n, 5, B, V], want codes_top [B, n], want codes_bot [B, n, 4], counted masks of the same shapes).
    Sample b of group g probes that group's tokens; position t and, on the bottom level, draw d continue the list.  exact_blocks: no probe of a block row
    is excluded (EXACT and SPLIT, whose expf(0), sum and division are exact there; FAST's reciprocal is not)."""
    r_top, r_bot = rows(V, name, variant)
    top_fam, bot_fam, _ = ROWSETS[(V, name)]
    plans, n = [], 1
    for s, members in groups_of(setting, batch):
        per = []
        for level, (row, draws) in enumerate(((r_top, 1), (r_bot, 4))):
            T, k, p = level_values(s, level)
            toks = probe_tokens(row, T, k, p)
            n = max(n, min(4, math.ceil(len(toks) / (len(members) * draws))))
            per.append(toks)
        plans.append((s, members, per))
    noise = np.ones((n, 5, batch, V), F32)
    want_t, want_b = np.zeros((batch, n), np.int64), np.zeros((batch, n, 4), np.int64)
    ok_t, ok_b = np.zeros((batch, n), bool), np.zeros((batch, n, 4), bool)
    for s, members, per in plans:
        for level, (row, fam, draws) in enumerate(((r_top, top_fam, 1), (r_bot, bot_fam, 4))):
            T, k, p = level_values(s, level)
            q, _ = probe_noise(V, per[level], n * draws * len(members))
            exact = exact_blocks and fam[0] in EXACT_BLOCKS and math.log2(T).is_integer()
            code, ok = robust_draws(row, q, T, k, p, 0.0 if exact else eps)
            q, code, ok = (a.reshape((n, draws, len(members)) + a.shape[1:]) for a in (q, code, ok))
            noise[:, level:level + draws][:, :, members] = q
            if level == 0:
                want_t[members], ok_t[members] = code[:, 0].T, ok[:, 0].T
            else:
                want_b[members], ok_b[members] = code.transpose(2, 0, 1), ok.transpose(2, 0, 1)
    return n, noise, want_t, want_b, ok_t, ok_b


# ----------------------------------------------------------------------------- random draws
DRAW_SETTINGS = {'hf': ('plain', 'k', 'k-edge', 'p', 'p-edge', 'kp', 'table'), 'sq': ('plain', 'k', 'k-edge', 'p', 'p-edge', 'kp', 'table')}
DRAW_N, NOISE_SEED = 2, 911


def draw_cases():
    """(V, row set, setting name) of the random-noise draws: the four random families under seven settings."""
    return [(V, name, sn) for (V, name), (_, _, settings) in ROWSETS.items() if name in DRAW_SETTINGS
            for sn, _ in settings if sn in DRAW_SETTINGS[name]]


@functools.lru_cache(maxsize=None)
def draw_noise(V):
    from hqtransformer_amd import synth
    q = synth.exp_noise(NOISE_SEED, DRAW_N, B, V)
    q.setflags(write=False)
    return q


def draw_case(V, name, variant, setting, eps, margin=MIN_MARGIN):
    """The random-noise pass of a case: (noise [n, 5, B, V], want top [B, n], want bot [B, n, 4], well-conditioned masks of the same shapes)."""
    r_top, r_bot = rows(V, name, variant)
    noise = draw_noise(V)
    want_t, want_b = np.zeros((B, DRAW_N), np.int64), np.zeros((B, DRAW_N, 4), np.int64)
    ok_t, ok_b = np.zeros((B, DRAW_N), bool), np.zeros((B, DRAW_N, 4), bool)
    for s, members in groups_of(setting):
        T, k, p = level_values(s, 0)
        code, ok = robust_draws(r_top, noise[:, 0][:, members], T, k, p, eps, margin)
        want_t[members], ok_t[members] = code.T, ok.T
        T, k, p = level_values(s, 1)
        code, ok = robust_draws(r_bot, noise[:, 1:][:, :, members], T, k, p, eps, margin)
        want_b[members], ok_b[members] = code.transpose(2, 0, 1), ok.transpose(2, 0, 1)
    return noise, want_t, want_b, ok_t, ok_b


# ----------------------------------------------------------------------------- ties
def tie_pairs(V):
    """Index pairs (i < j) whose candidates sit in one float4, in neighbouring float4s, lanes 63 | 64, two groups of one thread of the plain kernel
    (256 threads x float4), two strides of one thread of the general kernel (NT threads x float4: i, i + 4 NT; and i, i + NT, which are two threads),
    a LOWER index in a HIGHER lane or wave than its partner (the reductions must compare indices, not arrival order), first and last index."""
    NT = 256 if V < 4096 else 1024
    pairs = {(0, 1), (1, 2), (2, 3), (0, 3), (3, 4), (63 * 4 + 3, 64 * 4), (0, V - 1), (V - 2, V - 1), (5, 5 + NT), (2, 2 + 4 * NT)}
    for S in (4 * 256, 4 * 1024):
        pairs |= {(0, S), (5, S + 5), (4, S), (256, S), (260, S + 4), (S - 1, S), (S - 4 + 1, 2 * S - 2), (4 * 65 + 1, S + 4 * 3 + 2)}
    return sorted((i, j) for i, j in pairs if 0 <= i < j < V)


def tie_noise(V, pairs, rows_):
    q = np.full((rows_, V), 2.0, F32)
    want = np.zeros(rows_, np.int64)
    for r in range(rows_):
        i, j = pairs[r % len(pairs)]
        q[r, i] = q[r, j] = 1.0
        want[r] = i
    return q, want


# ----------------------------------------------------------------------------- which code path a case takes (restated as data)
def sort_class(row, T, k, p):
    """(threads per row, sort path) of sampler_kernel's top-p branch for a row, None without top-p: NT = 256 below V = 4096, else 1024; cnt = non-zero
    probabilities behind top-k; n2e = max(256, next power of two >= cnt); registers with one or two elements per thread while n2e <= 2 NT, else LDS."""
    if not p:
        return None
    V = len(row)
    NT = 256 if V < 4096 else 1024
    cnt = int((ref_probs(row, T, k, None) > 0).sum())
    n2e = 256
    while n2e < cnt:
        n2e <<= 1
    return NT, ('regs1' if n2e <= NT else 'regs2') if n2e <= 2 * NT else 'lds'


def f2ord(x):
    """The radix select's order-preserving key of fp32 values (csrc/kernels.hip)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def radix_pass(row, T, k):
    """The pass (1 .. 4) of the 4 x 8-bit radix select in which the k-th largest value parts from the largest value it masks: the two keys agree in
    their top 8 (pass - 1) bits and differ in the next 8.  None without an effective top-k or when nothing is masked."""
    V = len(row)
    k = eff_k(k, V)
    if not k:
        return None
    lg = np.sort((row / F32(T)).astype(F32))[::-1]
    below = lg[lg < lg[k - 1]]
    if not len(below):
        return None
    a, b = (int(v) for v in f2ord(np.array([lg[k - 1], below[0]], F32)))
    return next(ps for ps in (1, 2, 3, 4) if (a >> (32 - 8 * ps)) != (b >> (32 - 8 * ps)))


def plain_g4(V):
    """sampler_plain_fast_kernel's float4 groups per thread for a FAST row without a cut-off, None where launch_sampler keeps the general kernel."""
    if V % 4 or not 1024 <= V <= 8192:
        return None
    return 2 if V <= 2048 else 4 if V <= 4096 else 8


def is_plain(s, level, V):
    T, k, p = level_values(s, level)
    return not eff_k(k, V) and not p


def dispatch_form(setting, V):
    """'one': a uniform call, one launch per draw; 'two': a row table at a vocabulary the plain kernel takes -- FAST launches both kernels over all rows."""
    return 'two' if 'table' in setting and plain_g4(V) else 'one'


def all_cases():
    """(V, row set name, setting name, setting) of the whole table."""
    return [(V, name, sn, s) for (V, name), (_, _, settings) in ROWSETS.items() for sn, s in settings]


def oracle_rows(V, name, variant, batch=2, n=1):
    """The logits the CPU oracle's model returns with the row set injected: [n, 5, batch, V]."""
    spec, w = model(V, name, variant)
    noise = np.ones((n, 5, batch, V), F32)
    return OracleStage2(spec, w).sample(cond(batch), batch, n, noise, return_logits=True)[2]
