"""Shared test helpers: fixture loading and oracle construction (the oracle is the checker, never the product)."""
import json
import os

import numpy as np

from hqtransformer_amd import synth
from hqtransformer_amd.spec import Stage1Spec, Stage2Spec
from oracle.hqt_oracle import OracleStage1, OracleStage2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def stage2_from_fixture(fx):
    spec = Stage2Spec(**json.loads(str(fx['spec'])))
    weights = synth.stage2_weights(spec, int(fx['weight_seed']), 'fixture')
    return spec, weights


def stage1_from_fixture(fx):
    spec = Stage1Spec(**json.loads(str(fx['spec'])))
    weights = synth.stage1_weights(spec, int(fx['weight_seed']), 'fixture')
    return spec, weights


def oracle_stage2(fx):
    spec, weights = stage2_from_fixture(fx)
    return spec, weights, OracleStage2(spec, weights)


def oracle_stage1(fx):
    spec, weights = stage1_from_fixture(fx)
    return spec, weights, OracleStage1(spec, weights)


def gate(name: str, value: float, limit: float, op: str = '<=') -> None:
    """Assert ``value op limit`` for a FAST-precision tolerance gate.  With HQT_RECORD_GATES=<file> the measured value is
    appended to that JSON-lines file too (profiles/r02_fast_gates.txt is kept from such a run): the gates are set at about twice the
    measured figure, so a regression of the bf16 path shows up long before it reaches the old blanket 0.1 / 0.15 bounds."""
    value, limit = float(value), float(limit)
    path = os.environ.get('HQT_RECORD_GATES')
    if path:
        with open(path, 'a') as fp:
            fp.write(json.dumps({'gate': name, 'measured': value, 'limit': limit, 'op': op}) + '\n')
    ok = value <= limit if op == '<=' else value >= limit
    assert ok, f'{name}: measured {value} violates {op} {limit}'


def _synth_images(seed, B, R):
    r = np.random.default_rng([seed, 78])
    yy, xx = np.meshgrid(np.linspace(0, 1, R, dtype=np.float32), np.linspace(0, 1, R, dtype=np.float32), indexing='ij')
    img = np.zeros((B, 3, R, R), np.float32)
    for b in range(B):
        for c in range(3):
            for _ in range(4):
                fx_, fy_, ph = r.uniform(0.5, 6.0), r.uniform(0.5, 6.0), r.uniform(0, 2 * np.pi)
                img[b, c] += r.uniform(0.1, 0.4) * np.sin(2 * np.pi * (fx_ * xx + fy_ * yy) + ph).astype(np.float32)
    return np.clip(img + 0.05 * r.standard_normal(img.shape).astype(np.float32), -1.0, 1.0).astype(np.float32)


def _excess_distance(resid, emb, codes):
    """float64 d(z, e[code]) - min_n d(z, e[n]) per row: 0 where the code is the nearest one."""
    z = np.ascontiguousarray(resid.transpose(0, 2, 3, 1)).reshape(-1, resid.shape[1]).astype(np.float64)
    e = emb.astype(np.float64)
    d = (z ** 2).sum(1, keepdims=True) + (e ** 2).sum(1)[None] - 2 * z @ e.T
    return d[np.arange(len(z)), codes.reshape(-1)] - d.min(1)


def _codebooks(spec, weights):
    if spec.code_levels == 3:
        return [weights[f'quantizers.{l}.embedding'] for l in range(3)]
    return [weights['quantize_t.embedding'], weights['quantize_b.embedding']]


def philox_exp_noise(row_seeds, global_rows, n_steps: int, V: int, draws: int = 5) -> np.ndarray:
    """The Exp(1) noise libhqt's sampler generates in-kernel (csrc/kernels.hip, sampler_kernel): Philox4x32-10 with key = the
    row's 64-bit seed, counter = (vocabulary index // 4, step * draws + draw, global row lo, global row hi), lane v % 4 of the
    output, q = -log((float(r >> 9) + 0.5) * 2^-23) in fp32 (23 random bits: the sum is exact and u < 1, so q > 0 always).  The RNG is this build's own design (the reference draws from
    torch's global generator), so this restatement is test infrastructure: it lets the oracle replay what a Philox-driven call
    drew.  Returns [n_steps, draws, B, V] fp32."""
    seeds = np.asarray(row_seeds, np.uint64)
    rows = np.asarray(global_rows, np.int64).astype(np.uint64)
    B = len(seeds)
    V4 = (V + 3) // 4
    M32 = np.uint64(0xFFFFFFFF)
    out = np.empty((n_steps, draws, B, V4 * 4), np.float32)
    c0_init = np.broadcast_to(np.arange(V4, dtype=np.uint64)[None, :], (B, V4))
    for step in range(n_steps):
        for d in range(draws):
            c0 = c0_init.copy()
            c1 = np.full((B, V4), step * draws + d, np.uint64)
            c2 = np.broadcast_to((rows & M32)[:, None], (B, V4)).copy()
            c3 = np.broadcast_to((rows >> np.uint64(32))[:, None], (B, V4)).copy()
            k0 = np.broadcast_to((seeds & M32)[:, None], (B, V4)).copy()
            k1 = np.broadcast_to((seeds >> np.uint64(32))[:, None], (B, V4)).copy()
            for _ in range(10):
                p0 = np.uint64(0xD2511F53) * c0
                p1 = np.uint64(0xCD9E8D57) * c2
                hi0, lo0 = p0 >> np.uint64(32), p0 & M32
                hi1, lo1 = p1 >> np.uint64(32), p1 & M32
                c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
                k0 = (k0 + np.uint64(0x9E3779B9)) & M32
                k1 = (k1 + np.uint64(0xBB67AE85)) & M32
            r = np.stack([c0, c1, c2, c3], axis=-1).reshape(B, V4 * 4)
            u = ((r >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
            out[step, d] = -np.log(u, dtype=np.float32)
    return out[..., :V]
