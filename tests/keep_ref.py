"""Test infrastructure of the keep-mask tests: what a call with kept positions must return, from the unchanged oracle (oracle/hqt_oracle.py) by
iteration -- ``oracle_complete`` of tests/prefix_ref.py with a mask in place of a prefix length."""
import numpy as np

from oracle import hqt_oracle as O


def leading_run(mask, max_prefix):
    """L of a keep table, restated: the smallest count of leading ones over the rows, clipped to min(max_prefix, n - 1)."""
    mask = np.asarray(mask).astype(bool)
    runs = [int(np.argmin(r)) if not r.all() else mask.shape[1] for r in mask]
    return min(min(runs), int(max_prefix), mask.shape[1] - 1)


def oracle_keep(orc, cond, B, n, noise, mask, kept, top_k=(None, None), top_p=(None, None), temperature=(1.0, 1.0)):
    """Codes of a two-level run that keeps ``kept`` = (top [B, n], bot [B, n, 4]) where ``mask`` [B, n] is set and draws every other position as a free
    run would draw it had its earlier positions produced the same codes: for p = 0 .. n - 1 the oracle runs p + 1 teacher-forced positions, once for
    the top draw and once -- with the top code that is fed forward forced -- for the four bottom draws; a kept (b, p) takes the kept codes in place of
    the draws.  Returns (codes_top [B, n], codes_bot [B, n, 4], raw logits [n, 5, B, V], smallest winner / runner-up ratio of p / q over ALL draws,
    those a kept position discards included: no position is excluded)."""
    mask = np.asarray(mask).astype(bool)
    ct, cb = np.zeros((B, n), np.int64), np.zeros((B, n, 4), np.int64)
    logits = np.zeros((n, 5, B, orc.s.vocab_top), np.float32)
    margins = []
    for p in range(n):
        O.MARGIN_SINK = sink = []
        try:
            t, _ = orc.sample(cond, B, p + 1, noise[:p + 1], top_k, top_p, temperature, force_top=ct[:, :p + 1].copy(), force_bot=cb[:, :p + 1].copy())
            margins.append(sink[-5])                 # the top draw of position p (five draws per position, in order)
            ct[:, p] = np.where(mask[:, p], kept[0][:, p], t[:, p])
            del sink[:]
            _, b2, lg = orc.sample(cond, B, p + 1, noise[:p + 1], top_k, top_p, temperature, force_top=ct[:, :p + 1].copy(),
                                   force_bot=cb[:, :p + 1].copy(), return_logits=True)
            margins.extend(sink[-4:])
        finally:
            O.MARGIN_SINK = None
        cb[:, p] = np.where(mask[:, p, None], kept[1][:, p], b2[:, p])
        logits[p] = lg[p]
    return ct, cb, logits, float(min(margins))


def scattered_mask(B, n, runs, extra=()):
    """Mask [B, n]: row b keeps its first runs[b] positions, plus the cells of ``extra`` = ((row, (positions ...)), ...)."""
    mask = np.zeros((B, n), bool)
    for b, r in enumerate(runs):
        mask[b, :r] = True
    for b, cells in extra:
        mask[b, list(cells)] = True
    return mask


# the case of the issue, picked on the CPU with the oracle alone: g4_tiny_cls, B = 5, n = 12, TINY_SET, synth.exp_noise(700, ...)
KEEP_SEED = 700
KEEP_RUNS = (0, 3, 6, 3, 11)
KEEP_RUNS_L2 = (2, 3, 6, 3, 11)                      # the same case with a shared leading run of 2
KEEP_EXTRA = ((0, (2, 5, 6)), (1, (7, 9)), (3, (4, 10, 11)))
TINY_SET = ((50, 20), (None, 0.9), (1.0, 0.8))


def tiny_keep_case(spec, runs=KEEP_RUNS, B=5, n=12):
    """(cond, mask, kept codes, noise) of the recorded case."""
    from hqtransformer_amd import synth
    rng = np.random.default_rng([KEEP_SEED, 0x6b65])
    cond = (np.arange(B) % spec.n_classes).astype(np.int64)
    kept = (rng.integers(0, spec.vocab_top, (B, n)), rng.integers(0, spec.vocab_top, (B, n, 4)))
    return cond, scattered_mask(B, n, runs, KEEP_EXTRA), kept, synth.exp_noise(KEEP_SEED, n, B, spec.vocab_top)
