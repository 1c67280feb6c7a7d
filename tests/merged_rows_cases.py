"""Shared by tests/test_tile_plan_host.py and tests/test_gpu_merged_rows.py: merged passes at RAGGED row counts, one case per branch of the tile GEMMs' plan
(csrc/tile_plan.h: five geometries, split-K with S in {1, 2, 3, 4, 6, 8}, two tile orders, bands with a short last one) that the multiples of 128 rows of
tests/test_gpu_timed_schedule.py never take.  Every case: one body and one depth layer, heads of 64, n = 2 positions (the second reads a cache of more than
one key), V = 1024 except R1; synth.stage2_weights(spec, 910, 'fixture'), synth.exp_noise(NOISE_SEED[case], ...), class b % n_classes, no cut-offs, and the CPU
oracle (oracle/hqt_oracle.py) as the checker.  These are the smallest shapes that still reach the branch.

A pass of B samples launches its GEMMs at B rows in the body and in depth sub-step 0 and at 4 B rows in depth sub-step 1.  What each case reaches (the
plan's own words: tests/test_tile_plan_host.py prints them from the real function and holds EXPECTED_PLANS below against it):

case  model, B               body / sub-step 0 rows   sub-step 1 rows   reaches
R1    D 1536, V 8192, B 650  650                      2600              body qkv on loader waves with a 10-row last tile; the k/v GEMM of sub-step 0 (N = 2 D) on 8-wave
                                                                        64 x 128 tiles, 11 row tiles, ragged; fc2 split-K 8; 21 row tiles in depth (bands 7, 7, 7); the
                                                                        benchmark's own head (V = 8192) at ragged rows; fc2 of sub-step 1 on loader waves without split-K
R2    D 1536, B 830          830                      3320              fc2 split-K 6 (S does not divide 8: the other tile order); 26 row tiles of 128 in depth, bands 7, 7, 7, 5;
                                                                        proj on 13 row tiles of 64 (bands 7 + 6)
R3    D 1536, B 415          415 (streaming kernels)  1660              13 row tiles of 128, bands 7 + 6; fc2 split-K 3; a 415-row streaming body
R4    D 1536, B 1000         1000                     4000              fc2 on 8-wave 64 x 128 tiles through the t64 window; proj on 8-wave tiles
R5    D 1024, B 500          500 (streaming)          2000              the plain 128 x 128 geometry with S = 4 (tiles % 64 == 0); 16 row tiles, the last with 80 rows
R6    D 768, B 330           330 (streaming)          1320              fc2 split-K 8 at N = 768 (resid_combine_kernel<S, 256> with N < 1024); proj on 64 x 64 tiles, 21 row
                                                                        tiles, ragged
R7    D 896, B 660           660                      2640              split-K 2 (K / 16 = 224 divides by 4 only); S = 4 on loader waves and proj on 64 x 64 tiles at ragged rows
R8    D 256, B 200           200 (streaming)          800               the 4-wave 64 x 128 geometry (K = 256), 13 row tiles of 64, bands 7 + 6; the plain 128 x 128 geometry with
                                                                        only 8 stages (proj); fc2 (K = 1024) on 64 x 64 tiles

The table is as it was first written down: the real plan function agreed with every row, no case had to move."""
import collections

import numpy as np

from hqtransformer_amd import synth
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O

WEIGHT_SEED = 910
N_POSITIONS = 2
# csrc/tile_plan.h: geometries, the plan's ways out, the store modes (restated: the host test compiles the header and would not start if an enum moved
# without this file, since every EXPECTED_PLANS row would stop matching)
TG_128, TG_64X128, TG_64X128_W8, TG_64X64, TG_128_PC, TG_COUNT = 0, 1, 2, 3, 4, 5
(TB_NOT_TAKEN, TB_NARROW_64X64, TB_LOADERS, TB_W8, TB_W4, TB_NARROW_W8, TB_WIDE_LOADERS, TB_WIDE_W8, TB_WIDE_S4_LOADERS, TB_WIDE_S4, TB_WIDE_LARGEST_S, TB_PLAIN,
 TB_COUNT) = range(13)
STORES = dict(rows=0, qkv=2, packed=3, resid=4)
TILE_NAME = {TG_128: '128x128', TG_64X128: '64x128', TG_64X128_W8: '64x128w8', TG_64X64: '64x64', TG_128_PC: '128x128pc'}
Plan = collections.namedtuple('Plan', 'geom bm bn S branch')


def _spec(D, V):
    return Stage2Spec(embed_dim=D, n_layers=1, n_heads=D // 64, n_layers_depth=1, vocab_top=V, vocab_bot=V, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                      n_classes=10, cond=1, embedding=0)


# name -> (spec, B); the noise seed of a case is changed, never the margin bound, if one of its draws is ill-conditioned
CASES = {
    'R1': (_spec(1536, 8192), 650),
    'R2': (_spec(1536, 1024), 830),
    'R3': (_spec(1536, 1024), 415),
    'R4': (_spec(1536, 1024), 1000),
    'R5': (_spec(1024, 1024), 500),
    'R6': (_spec(768, 1024), 330),
    'R7': (_spec(896, 1024), 660),
    'R8': (_spec(256, 1024), 200),
}
NOISE_SEED = {name: 911 for name in CASES}

PHASES = ('body', 'depth0', 'depth1')
TAG = dict(qkv='gemm_qkv', kv='gemm_qkv', proj='gemm_proj', fc1='gemm_fc1', fc2='gemm_fc2', head='gemm_head')


def launches(D, V, B):
    """The nn.Linear launches of one position of a FAST pass of B samples: {(gemm, phase): (rows, N, K, store mode, deferred LayerNorm)} -- the transformer
    block of the body, of depth sub-step 0 (one key: only [key; value] of the fused weight, N = 2 D) and of sub-step 1 (4 rows per sample), a head behind each
    depth sub-step."""
    out = {}
    for phase, M in zip(PHASES, (B, B, 4 * B)):
        out[('kv' if phase == 'depth0' else 'qkv', phase)] = (M, 2 * D if phase == 'depth0' else 3 * D, D, 'qkv', True)
        out[('proj', phase)] = (M, D, D, 'resid', False)
        out[('fc1', phase)] = (M, 4 * D, D, 'packed', True)
        out[('fc2', phase)] = (M, D, 4 * D, 'resid', False)
        if phase != 'body':
            out[('head', phase)] = (M, V, D, 'rows', True)
    return out


def all_launches():
    return {name: launches(spec.embed_dim, spec.vocab_top, B) for name, (spec, B) in CASES.items()}


def timed_schedule_launches():
    """The shapes tests/test_gpu_timed_schedule.py runs (all multiples of 128 rows): counted when the host test asks whether every way out of the plan is taken."""
    return {f'timed{B}': launches(D, V, B) for D, V, B in ((1536, 8192, 512), (1536, 8192, 640), (1536, 8192, 2048), (512, 1024, 1280))}


def bands(TM):
    """Heights of the row-tile bands tile_of walks (held against the real function by tests/test_tile_plan_host.py::test_tile_of_bands)."""
    nb = 1 if TM <= 12 else (TM + 7) // 8
    GM = -(-TM // nb)
    return [min(GM, TM - first) for first in range(0, TM, GM)]


_S = (-1, 1)          # not the tile kernels': below 512 rows (the streaming kernels)
_BODY_STREAM = {(g, ph): _S for ph in ('body', 'depth0') for g in ('kv' if ph == 'depth0' else 'qkv', 'proj', 'fc1', 'fc2')} | {('head', 'depth0'): _S}
# case -> {(gemm, phase): (geometry, S)}: the record the host test holds against the real plan and the GPU test against the engine's counters
EXPECTED_PLANS = {
    'R1': {('qkv', 'body'): (4, 1), ('proj', 'body'): (2, 1), ('fc1', 'body'): (0, 1), ('fc2', 'body'): (0, 8),
           ('kv', 'depth0'): (2, 1), ('proj', 'depth0'): (2, 1), ('fc1', 'depth0'): (0, 1), ('fc2', 'depth0'): (0, 8), ('head', 'depth0'): (0, 1),
           ('qkv', 'depth1'): (0, 1), ('proj', 'depth1'): (2, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (4, 1), ('head', 'depth1'): (0, 1)},
    'R2': {('qkv', 'body'): (4, 1), ('proj', 'body'): (2, 1), ('fc1', 'body'): (0, 1), ('fc2', 'body'): (0, 6),
           ('kv', 'depth0'): (4, 1), ('proj', 'depth0'): (2, 1), ('fc1', 'depth0'): (0, 1), ('fc2', 'depth0'): (0, 6), ('head', 'depth0'): (2, 1),
           ('qkv', 'depth1'): (0, 1), ('proj', 'depth1'): (0, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (0, 1), ('head', 'depth1'): (4, 1)},
    'R3': {**_BODY_STREAM,
           ('qkv', 'depth1'): (0, 1), ('proj', 'depth1'): (2, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (0, 3), ('head', 'depth1'): (2, 1)},
    'R4': {('qkv', 'body'): (0, 1), ('proj', 'body'): (2, 1), ('fc1', 'body'): (0, 1), ('fc2', 'body'): (2, 1),
           ('kv', 'depth0'): (4, 1), ('proj', 'depth0'): (2, 1), ('fc1', 'depth0'): (0, 1), ('fc2', 'depth0'): (2, 1), ('head', 'depth0'): (2, 1),
           ('qkv', 'depth1'): (0, 1), ('proj', 'depth1'): (0, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (0, 1), ('head', 'depth1'): (4, 1)},
    'R5': {**_BODY_STREAM,
           ('qkv', 'depth1'): (0, 1), ('proj', 'depth1'): (2, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (0, 4), ('head', 'depth1'): (2, 1)},
    'R6': {**_BODY_STREAM,
           ('qkv', 'depth1'): (4, 1), ('proj', 'depth1'): (3, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (0, 8), ('head', 'depth1'): (2, 1)},
    'R7': {('qkv', 'body'): (2, 1), ('proj', 'body'): (3, 1), ('fc1', 'body'): (4, 1), ('fc2', 'body'): (4, 4),
           ('kv', 'depth0'): (2, 1), ('proj', 'depth0'): (3, 1), ('fc1', 'depth0'): (4, 1), ('fc2', 'depth0'): (4, 4), ('head', 'depth0'): (2, 1),
           ('qkv', 'depth1'): (0, 1), ('proj', 'depth1'): (2, 1), ('fc1', 'depth1'): (0, 1), ('fc2', 'depth1'): (0, 2), ('head', 'depth1'): (4, 1)},
    'R8': {**_BODY_STREAM,
           ('qkv', 'depth1'): (1, 1), ('proj', 'depth1'): (0, 1), ('fc1', 'depth1'): (1, 1), ('fc2', 'depth1'): (3, 1), ('head', 'depth1'): (1, 1)},
}


def expected_fast_variants(name, n=N_POSITIONS):
    """The GEMM counters a FAST pass of n positions must show for a case, from EXPECTED_PLANS: {variant: launches}.  A launch the plan does not take is the
    streaming kernel's (these models pack every weight)."""
    spec, B = CASES[name]
    want = collections.Counter()
    for (gemm, phase), (M, N, K, store, dln) in launches(spec.embed_dim, spec.vocab_top, B).items():
        geom, S = EXPECTED_PLANS[name][(gemm, phase)]
        if geom < 0:
            want[f'variant:stream_gemm{"_dln" if dln else ""}:{TAG[gemm]}'] += n
        elif S > 1:
            want[f'variant:tile_gemm_{TILE_NAME[geom]}_splitk{S}:{TAG[gemm]}'] += n
        else:
            want[f'variant:tile_gemm_{TILE_NAME[geom]}{"_dln" if dln else ""}:{TAG[gemm]}'] += n
    return dict(want)


_INPUTS, _WANT = {}, {}


def inputs(name):
    """(spec, weights, cond, noise, B, n) of a case."""
    if name not in _INPUTS:
        spec, B = CASES[name]
        weights = synth.stage2_weights(spec, WEIGHT_SEED, 'fixture')
        noise = synth.exp_noise(NOISE_SEED[name], N_POSITIONS, B, spec.vocab_top)
        _INPUTS[name] = (spec, weights, np.arange(B) % spec.n_classes, noise, B, N_POSITIONS)
    return _INPUTS[name]


def oracle(name):
    """The oracle's free run of a case, computed once: (codes_top [B, n], codes_bot [B, n, 4], raw logits [n, 5, B, V], closest winner / runner-up ratio of
    p / q over all its draws).  Callers must not write into the arrays."""
    if name not in _WANT:
        spec, weights, cond, noise, B, n = inputs(name)
        old, O.MARGIN_SINK = O.MARGIN_SINK, []
        try:
            ct, cb, lg = O.OracleStage2(spec, weights).sample(cond, B, n, noise, return_logits=True)
            margin = min(O.MARGIN_SINK)
        finally:
            O.MARGIN_SINK = old
        for a in (ct, cb, lg):
            a.setflags(write=False)
        _WANT[name] = (ct, cb, lg, margin)
    return _WANT[name]
