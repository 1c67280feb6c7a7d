"""Test infrastructure of the prefix-completion tests: the expected completion of a code prefix from the unchanged oracle
(oracle/hqt_oracle.py), by iteration -- the oracle has no prefix argument, only teacher forcing of a whole run."""
import numpy as np

from oracle import hqt_oracle as O


def oracle_complete(orc, cond, B, n, noise, P, prefix, top_k=(None, None), top_p=(None, None), temperature=(1.0, 1.0)):
    """Codes of positions P .. n - 1 as a free run would draw them had its first P positions produced ``prefix`` = (top [B, P], bot [B, P, 4]):
    for p = P .. n - 1 the oracle runs p + 1 teacher-forced positions and its draw at p is taken.  The oracle feeds force_top[:, p] to the
    bottom draws of position p itself, so every position takes two runs: one for the top draw, one -- with that top code forced, which is what
    a free run feeds -- for the four bottom draws.  Returns (codes_top [B, n], codes_bot [B, n, 4], logits [n, 5, B, V] (rows >= P filled),
    smallest winner / runner-up ratio of p / q over the compared draws)."""
    ct, cb = np.zeros((B, n), np.int64), np.zeros((B, n, 4), np.int64)
    ct[:, :P], cb[:, :P] = prefix
    logits = np.zeros((n, 5, B, orc.s.vocab_top), np.float32)
    margins = []
    for p in range(P, n):
        O.MARGIN_SINK = sink = []
        try:
            t, _ = orc.sample(cond, B, p + 1, noise[:p + 1], top_k, top_p, temperature, force_top=ct[:, :p + 1].copy(), force_bot=cb[:, :p + 1].copy())
            margins.append(sink[-5])                 # the top draw of position p (five draws per position, in order)
            ct[:, p] = t[:, p]
            del sink[:]
            t2, b2, lg = orc.sample(cond, B, p + 1, noise[:p + 1], top_k, top_p, temperature, force_top=ct[:, :p + 1].copy(),
                                    force_bot=cb[:, :p + 1].copy(), return_logits=True)
            margins.extend(sink[-4:])
        finally:
            O.MARGIN_SINK = None
        assert (t2[:, p] == ct[:, p]).all()
        cb[:, p] = b2[:, p]
        logits[p] = lg[p]
    return ct, cb, logits, float(min(margins))


def random_prefix_case(spec, B, n, P, seed):
    """Seeded inputs of a completion the model did not draw itself: class ids, uniform random prefix codes, explicit Exp(1) noise."""
    from hqtransformer_amd import synth
    rng = np.random.default_rng([seed, 0x51ed])
    cond = (np.arange(B) % spec.n_classes).astype(np.int64) if spec.cond == 1 else None
    prefix = (rng.integers(0, spec.vocab_top, (B, P)), rng.integers(0, spec.vocab_top, (B, P, 4)))
    return cond, prefix, synth.exp_noise(seed, n, B, spec.vocab_top)
