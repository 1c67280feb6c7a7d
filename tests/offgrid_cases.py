"""Shared by tests/test_offgrid_host.py and tests/test_gpu_offgrid_stage2.py: stage-2 models hqt_create accepts (embed_dim a multiple of 16 and of
n_heads, head size a power of two in [8, 256], vocabulary a multiple of 4 up to 16384) that lie OFF the grid every other test, fixture and released
config sits on (embed_dim in {64, 128, 256, 1024, 1536}, head size 32 / 64, V in {64, 256, 512, 1024, 8192}, at most 64 + 3 cached keys) -- shapes at
which the dispatchers of csrc/engine.hip pick kernels nothing else runs.  Every case: synth.stage2_weights(spec, 900, 'fixture'), synth.exp_noise(901, ...),
synth.text_ids(902, ...) or class b % n_classes, and the CPU oracle (oracle/hqt_oracle.py) as the checker.

case  reaches
A     D 48 / head size 16, V 100: fp32 and bf16 gemm_tile_kernel at K = 48 (no k-quarter order, no packed weights), a head with N % 16 != 0, a sampler
      row of fewer than 256 entries
B     D 96 / head size 8, V 1000, 80 samples: one lane per key row in attention; packed body + deferred LayerNorm into an UNPACKED head (V % 32 != 0)
      with a ragged N tile; depth sub-step 1 has 320 rows (EXACT: the tile kernel; SPLIT: above 256 rows with qkv_D % 64 != 0)
C     D 256 / head size 256, 40 positions: 16 keys per online-softmax group, so three groups; depth sub-step 1 (5 keys) is beyond the few-query
      kernel's bound at this head size and runs attention_kernel with Tq = 4
D     D 256 / head size 128, V 516, 23 text tokens + 48 positions: 32 keys per group, 71 keys; a prefill of 23 rows at a head size the MFMA prefill
      does not take; a vocabulary with a tail
E     D 80 / head size 16, V 260, unconditional, 'reduce' embedding, 67 samples: K = 80 generic and K = 320 mfma_gemm with an 80-column tile; 268-row
      depth sub-step; ragged batch
F     D 128 / head size 64 (the production head size), 64 text tokens + 64 positions: the second key group filled completely (65 .. 128 keys)
G     F's model at 256 samples: attention_heads8_kernel (FAST, B >= 256) walking past 64 keys

SWEEP: D 64 / 2 heads / 1 + 1 layers at V in {100, 260, 1000, 1500, 5000, 16384}, each plain (no cut-off, T = 1) and cut (top-k, top-p, temperature:
the sampler's sort padded to a power of two, 256 threads per row below V = 4096 and 1024 from there; top-p is refused above V = 8192)."""
import numpy as np

from hqtransformer_amd import synth
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O

WEIGHT_SEED, NOISE_SEED, TEXT_SEED = 900, 901, 902
MIN_MARGIN = 1.00001              # tests/test_gpu_timed_schedule.py: below this a draw is decided by the summation order of any fp32 implementation
SETTINGS = dict(top_k=(None, 20), top_p=(None, 0.9), temperature=(1.0, 0.9))
PLAIN = dict(top_k=(None, None), top_p=(None, None), temperature=(1.0, 1.0))


def _spec(D, heads, layers, depth, V, ctx_img, **kw):
    base = dict(embed_dim=D, n_layers=layers, n_heads=heads, n_layers_depth=depth, vocab_top=V, vocab_bot=V, vocab_txt=64, ctx_len_img=ctx_img,
                ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    base.update(kw)
    return Stage2Spec(**base)


_F = dict(vocab_txt=512, ctx_len_txt=64, cond=2)
# name -> (spec, B, n)
CASES = {
    'A': (_spec(48, 3, 2, 2, 100, 24), 5, 24),
    'B': (_spec(96, 12, 2, 1, 1000, 16), 80, 3),
    'C': (_spec(256, 1, 2, 1, 256, 40), 5, 40),
    'D': (_spec(256, 2, 2, 1, 516, 48, vocab_txt=100, ctx_len_txt=23, cond=2), 5, 48),
    'E': (_spec(80, 5, 2, 2, 260, 16, cond=0, embedding=1), 67, 4),
    'F': (_spec(128, 2, 2, 1, 256, 64, **_F), 5, 64),
    'G': (_spec(128, 2, 2, 1, 256, 64, **_F), 256, 3),
}
SWEEP_V = (100, 260, 1000, 1500, 5000, 16384)
SWEEP_B, SWEEP_N = 3, 3


def sweep_settings(V, cut):
    if not cut:
        return dict(PLAIN)
    return dict(top_k=(V // 3, 37), top_p=(0.95, 0.9) if V <= 8192 else (None, None), temperature=(0.95, 0.8))


def sweep_spec(V):
    return _spec(64, 2, 1, 1, V, 16)


def all_rows():
    """Every row of the table: (id, spec, B, n, sampler settings)."""
    rows = [(name, spec, B, n, dict(SETTINGS)) for name, (spec, B, n) in CASES.items()]
    for V in SWEEP_V:
        for cut in (False, True):
            rows.append((f'V{V}-{"cut" if cut else "plain"}', sweep_spec(V), SWEEP_B, SWEEP_N, sweep_settings(V, cut)))
    return rows


ROWS = {r[0]: r for r in all_rows()}
_INPUTS, _WANT = {}, {}


def inputs(name):
    """(spec, weights, cond, noise, B, n, settings) of a row; cond is None for the unconditional model."""
    if name not in _INPUTS:
        _, spec, B, n, settings = ROWS[name]
        weights = synth.stage2_weights(spec, WEIGHT_SEED, 'fixture')
        noise = synth.exp_noise(NOISE_SEED, n, B, spec.vocab_top)
        if spec.cond == 2:
            cond = synth.text_ids(TEXT_SEED, B, spec.ctx_len_txt, spec.vocab_txt)
        else:
            cond = np.arange(B) % spec.n_classes if spec.cond == 1 else None
        _INPUTS[name] = (spec, weights, cond, noise, B, n, settings)
    return _INPUTS[name]


def oracle(name):
    """The oracle's free run of a row, computed once: (codes_top [B, n], codes_bot [B, n, 4], raw logits [n, 5, B, V], closest winner / runner-up
    ratio of p / q over all its draws).  Callers must not write into the arrays."""
    if name not in _WANT:
        spec, weights, cond, noise, B, n, settings = inputs(name)
        old, O.MARGIN_SINK = O.MARGIN_SINK, []
        try:
            ct, cb, lg = O.OracleStage2(spec, weights).sample(cond, B, n, noise, settings['top_k'], settings['top_p'], settings['temperature'],
                                                              return_logits=True)
            margin = min(O.MARGIN_SINK)
        finally:
            O.MARGIN_SINK = old
        for a in (ct, cb, lg):
            a.setflags(write=False)
        _WANT[name] = (ct, cb, lg, margin)
    return _WANT[name]
