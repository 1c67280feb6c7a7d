"""Test infrastructure of the guided-sampling tests (never the product): the guided logits row in numpy float32, and the unchanged oracle
(oracle/hqt_oracle.py) made to draw from it."""
import contextlib

import numpy as np

from oracle import hqt_oracle as O

F32 = np.float32


def mix(l_pos, l_neg, s):
    """g = l_pos + (s - 1) (l_pos - l_neg): s - 1, the difference, the product and the sum each rounded to float32 on their own (numpy never
    contracts into an FMA) -- what guide_logits_kernel computes with __fsub_rn / __fmul_rn / __fadd_rn, bit for bit."""
    l_pos, l_neg = np.asarray(l_pos, F32), np.asarray(l_neg, F32)
    sm1 = F32(s) - F32(1.0)
    d = (l_pos - l_neg).astype(F32)
    m = (sm1 * d).astype(F32)
    return (l_pos + m).astype(F32)


def level_of_draw(d: int) -> int:
    """Code level of draw d of a position (draw order top, 4 x middle / bottom[, 16 x bottom])."""
    return 0 if d == 0 else (1 if d < 5 else 2)


def safe_ratio(scales, e: float, temperature) -> float:
    """Winner / runner-up ratio of p / q above which a draw cannot be changed by a logit error of at most ``e`` per row: the guided row moves by at most
    (|s| + |s - 1|) e, a log-ratio of two entries by twice that, over the temperature.  The largest over the levels."""
    return max(float(np.exp(2.0 * (abs(s) + abs(s - 1.0)) * e / float(T))) for s, T in zip(scales, temperature))


@contextlib.contextmanager
def guided_oracle(n: int, scales, draws: int = 5):
    """For the length of the block, ``oracle.hqt_oracle.sample_filtered`` draws BOTH halves of a 2 n-row run (positives, then negatives, ``noise``
    duplicated by the caller) from the mixed rows; the oracle's own files stay as they are.  The oracle calls it once per draw, in draw order, ``draws``
    (5 or 21) per position: the level of a call follows from its count.  Yields the list the oracle's own MARGIN_SINK fills: the smallest winner /
    runner-up ratio of every draw."""
    orig, calls, sink = O.sample_filtered, [0], []

    def wrapped(logits, q, temperature, top_k, top_p):
        lv = level_of_draw(calls[0] % draws)
        calls[0] += 1
        assert logits.shape[0] == 2 * n, f'expected {2 * n} rows (positives, then negatives), got {logits.shape}'
        g = mix(logits[:n], logits[n:], scales[lv])
        return orig(np.concatenate([g, g]), q, temperature, top_k, top_p)

    old_sink = O.MARGIN_SINK
    O.sample_filtered, O.MARGIN_SINK = wrapped, sink
    try:
        yield sink
    finally:
        O.sample_filtered, O.MARGIN_SINK = orig, old_sink
