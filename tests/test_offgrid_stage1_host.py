"""The off-grid stage-1 case table (tests/offgrid_stage1_cases.py) on the CPU: every spec builds and is off the grid in what its row says, the fp32
oracle is a good enough checker at these shapes (within 1e-5 of an fp64 run of the same graph: a tenth of the 1e-4 pixel bar the GPU tests hold the
kernels to), the large-mean cases have large group means, the encode inputs have few argmin near-ties, and the dispatch conditions restated as data
predict the kernels each case is there to reach (tests/test_gpu_offgrid_stage1.py compares the engine's own report with the same prediction)."""
import numpy as np
import pytest

from hqtransformer_amd.spec import stage1_encoder_param_shapes, stage1_param_shapes
from oracle import hqt_oracle as O
from tests import offgrid_stage1_cases as S1
from tests.helpers import _codebooks

REFERENCE_TOL = 1e-5


@pytest.mark.parametrize('name', list(S1.CASES))
def test_spec_builds_and_the_fp32_oracle_is_within_1e5_of_its_fp64_run(name):
    spec, weights, codes = S1.inputs(name)
    assert spec.ch % 32 == 0 and spec.resolution % 2 ** len(spec.ch_mult) == 0
    shapes = stage1_param_shapes(spec)
    assert list(shapes) == list(weights) and all(weights[k].shape == tuple(s) for k, s in shapes.items())
    z_res, grids = S1.GRIDS[name]
    assert spec.z_res == z_res and [c.shape for c in codes] == [(S1.N_IMAGES, g, g) for g in grids]
    assert grids[-1] == z_res and all(2 * a == b for a, b in zip(grids, grids[1:])) and len(grids) == spec.code_levels
    want = S1.want(name)
    assert want.shape == (S1.N_IMAGES, 3, spec.resolution, spec.resolution) and want.dtype == np.float32 and np.isfinite(want).all()
    f64 = S1.oracle_decode_f64(spec, weights, codes)
    assert f64.dtype == np.float64 and O.F32 is np.float32
    err = np.abs(want - f64).max()
    print(f'{name}: fp32 oracle vs fp64 run {err:.2e}, pixel std {want.std():.3f}, max |pixel| {np.abs(want).max():.2f}')
    assert err <= REFERENCE_TOL, err


@pytest.mark.parametrize('name', S1.LARGE_MEAN)
def test_large_mean_cases_have_large_group_means(name):
    """A spy on oracle.group_norm: at least 8 GroupNorms of the shifted weights see |mean| / std >= 25 in some (image, group) -- where variance as
    E[x^2] - mean^2 from fp32 sums has lost three digits -- while the unshifted weights stay at or below 2.5 and the pixels stay O(1)."""
    spec, weights, codes = S1.inputs(name)
    seen = []
    real = O.group_norm

    def spy(x, g, b, groups=32, eps=1e-6):
        xg = x.reshape(x.shape[0], groups, -1).astype(np.float64)
        seen.append(float((np.abs(xg.mean(-1)) / xg.std(-1)).max()))
        return real(x, g, b, groups, eps)

    O.group_norm = spy
    try:
        px = S1.oracle_decode(spec, weights, codes)
        shifted, seen = seen, []
        base = dict(weights)
        for k in S1.SHIFTED:
            base[k] = (weights[k] - np.float32(S1.BIAS_SHIFT)).astype(np.float32)
        S1.oracle_decode(spec, base, codes)
        plain = seen
    finally:
        O.group_norm = real
    n_gn = sum(r.op == 'gn' for r in S1.plan(name))
    assert len(shifted) == len(plain) == n_gn == 16
    big = [v for v in shifted if v >= 25.0]
    print(f'{name}: |mean| / std per GroupNorm {[round(v, 1) for v in shifted]}; unshifted max {max(plain):.2f}; max |pixel| {np.abs(px).max():.2f}')
    assert len(big) >= 8, shifted
    assert max(plain) <= 2.5 and np.abs(px).max() <= 5.0                     # unshifted: a tenth of the threshold at most


@pytest.mark.parametrize('name', S1.ENCODE)
def test_encode_inputs_have_few_argmin_near_ties(name):
    """The GPU test lets a code differ from the oracle's only where the oracle's own fp64 distance gap is <= 1e-4, and lets at most 1 % of the codes
    use that: here, fewer than 1 % of the oracle's quantiser inputs have a runner-up that close."""
    spec, weights, x, want = S1.encode_inputs(name)
    shapes = dict(stage1_param_shapes(spec))
    shapes.update(stage1_encoder_param_shapes(spec))
    assert set(shapes) == set(weights) and x.shape == (S1.N_IMAGES, 3, spec.resolution, spec.resolution)
    cbs = _codebooks(spec, weights)
    for l in range(2):
        resid = want['resid'][l]
        z = np.ascontiguousarray(resid.transpose(0, 2, 3, 1)).reshape(-1, resid.shape[1]).astype(np.float64)
        e = cbs[l].astype(np.float64)
        d = np.partition((z ** 2).sum(1, keepdims=True) + (e ** 2).sum(1)[None] - 2 * z @ e.T, 1, axis=1)
        frac = float(np.mean(d[:, 1] - d[:, 0] <= 1e-4))
        print(f'{name} level {l}: {len(z)} vectors, near-ties {frac:.4f}, smallest gap {np.min(d[:, 1] - d[:, 0]):.2e}')
        assert frac < 0.01, (l, frac)
        assert want['codes'][l].shape == (S1.N_IMAGES, resid.shape[2], resid.shape[3])


def _rows(name, **kw):
    return [r for r in S1.plan(name) if all(getattr(r, k) == v for k, v in kw.items())]


def test_every_case_is_off_the_grid_in_what_its_row_says():
    """The documented shape conditions per launch site, as data: each case crosses the ones it is named for."""
    on_grid = lambda r: r.c64 and r.h8 and r.w16 and r.k64 and (r.nchw or (r.cpg_pow2 and r.fixed_map)) and r.res & (r.res - 1) == 0
    assert all(on_grid(r) for r in S1.plan('M64'))                          # the wide config of tests/test_gpu_split.py crosses none of them
    for name in S1.PLAIN:
        assert not all(on_grid(r) for r in S1.plan(name)), name
    # A: 192 channels keep every conv % 64, but no GroupNorm at 192 has a power-of-two group or the fixed thread mapping
    a = S1.plan('A')
    assert all(r.c64 and r.h8 and r.w16 and r.k64 for r in a if r.op != 'gn')
    assert {r.cin for r in a if r.op == 'gn'} == {64, 192}
    assert all(r.cpg_pow2 == r.fixed_map == (r.cin == 64) for r in a if r.op == 'gn')
    assert all(r.cout % 128 for r in a if r.op == 'conv3')                   # never the ring kernel's whole 128-channel tiles
    # B: 96-wide layers are not % 64, 192-wide ones are; K = 48 at post_quant and conv_in
    b = S1.plan('B')
    assert [(r.layer, r.K, r.k64, r.k32) for r in b[:2]] == [('post_quant_conv_b', 48, False, False), ('decoder.conv_in', 432, False, False)]
    assert {r.cin: r.c64 for r in b if r.op == 'conv3' and r.layer != 'decoder.conv_in'} == {96: False, 192: True}
    assert b[-1].layer == 'decoder.conv_out' and b[-1].cin == 96 and b[-1].w16
    # C: nothing % 64, five channels per group, K = 1440
    c = S1.plan('C')
    assert not any(r.c64 for r in c if r.op in ('conv3', 'conv1')) and not any(r.cpg_pow2 or r.fixed_map for r in c if r.op == 'gn')
    assert {r.K for r in c if r.op == 'conv3' and r.cin == 160} == {1440} and not any(r.k64 for r in c if r.op in ('conv3', 'conv1'))
    # D: 24 (W % 16 != 0), 48, 96; attention products at hw = 576 stay % 64
    d = S1.plan('D')
    assert sorted({r.res for r in d}) == [24, 48, 96] and all(r.c64 for r in d if r.op != 'gn')
    assert all(r.h8 and r.w16 == (r.res != 24) for r in d)
    assert [(r.K, r.k64) for r in d if r.op == 'attn'] == [(128, True), (576, True)] * 3 and S1.N_IMAGES * 576 % 128
    # E: 20 (H % 8 != 0), 40 (H % 8 == 0, W % 16 != 0), 80; attention K = 400 is neither % 64 nor % 32
    e = S1.plan('E')
    assert sorted({r.res for r in e}) == [20, 40, 80]
    assert {r.res: (r.h8, r.w16) for r in e} == {20: (False, False), 40: (True, False), 80: (True, True)}
    assert [(r.K, r.k64, r.k32) for r in e if r.op == 'attn'] == [(128, True, True), (400, False, False)] * 3 and S1.N_IMAGES * 400 % 128
    # F: no final upsampling; 128-channel convs at 48 (whole ring tiles), 24 falls back
    f = S1.plan('F')
    assert sorted({r.res for r in f}) == [24, 48] and sum(r.up for r in f) == 1 and f[-1].res == 48
    assert any(r.op == 'conv3' and r.res == 48 and r.cout == 128 and r.w16 for r in f)
    # G: three levels 20 -> 160, conv_out with M = 3 * 160 * 160 >= 4096 and H % 16 == 0
    g = S1.plan('G')
    assert sorted({r.res for r in g}) == [20, 40, 80, 160] and g[-1].res == 160 and S1.N_IMAGES * 160 * 160 >= 4096
    # H: three code levels, K = 16 into post_quant
    h = S1.plan('H')
    assert h[0].K == 16 and not h[0].k32 and h[1:] == d[1:]


def test_predicted_kernels_per_case():
    """What the restated conditions predict for the kernels each case is there to reach (the GPU test holds the engine's report against the same
    function, so a wrong restatement fails there, not silently)."""
    v = lambda name, prec: S1.variants(name, prec)
    for name in S1.CASES:                                                     # EXACT: the fp32 kernels and the two-pass statistics, nothing else
        ex = v(name, 'exact')
        assert all(k.startswith(('variant:gemm_generic_f32:', 'variant:gn_stats_two_pass:')) for k in ex), (name, ex)
        assert ex['variant:gn_stats_two_pass:gn'] == sum(r.op == 'gn' for r in S1.plan(name))
        for prec in ('split', 'fast'):                                        # every conv / product / GroupNorm is counted exactly once
            got = v(name, prec)
            rows = S1.plan(name)
            n_conv = sum(c for k, c in got.items() if not k.endswith((':gn', ':attn_gemm')) and 'planes_out' not in k)
            assert n_conv == sum(r.op in ('conv3', 'conv1') for r in rows), (name, prec, got)
            assert sum(c for k, c in got.items() if k.endswith(':attn_gemm')) == sum(r.op == 'attn' for r in rows)
            assert sum(c for k, c in got.items() if k.endswith(':gn')) == sum(r.op == 'gn' for r in rows)
    a = v('A', 'split')
    assert not any('gemm_generic_f32' in k for k in a) and 'variant:gn_stats_two_pass:gn' not in a
    gn192 = len(_rows('A', op='gn', cin=192))
    # every 192-wide GroupNorm takes the pass; of the 64-wide ones, those behind a SPLIT 3x3 conv with 64 outputs take its tile statistics
    assert a['variant:gn_stats_pass:gn'] >= gn192 and a['variant:gn_stats_tiles:gn'] + a['variant:gn_stats_pass:gn'] == 16
    assert a['variant:gn_stats_pass:gn'] == gn192 and a['variant:gn_stats_tiles:gn'] == len(_rows('A', op='gn', cin=64)) == 4
    assert a['variant:conv_out_direct:conv_out'] == 1
    b = v('B', 'split')
    n96 = len([r for r in S1.plan('B') if r.op == 'conv3' and r.cin == 96 and r.tag == 'conv3x3'])
    assert b['variant:gemm_generic_f32:conv3x3'] == n96 + 1                   # + conv_in (Cin = 48)
    assert b['variant:split_conv3:conv3x3'] == len([r for r in S1.plan('B') if r.op == 'conv3' and r.cin == 192])
    assert b['variant:conv_out_direct:conv_out'] == 1 and b['variant:gemm_generic_f32:conv1x1'] >= 1
    c = v('C', 'split')
    # (the one SPLIT kernel C does reach: softmax x v with K = hw = 64; q k^T has K = 160)
    assert [k for k in c if ':split_' in k] == ['variant:split_gemm:attn_gemm'] and c['variant:split_gemm:attn_gemm'] == 3
    assert not any('halo_conv' in k for k in v('C', 'fast')) and c['variant:gn_stats_pass:gn'] == 1      # conv_out_direct's statistics at 160
    d = v('D', 'split')
    assert d['variant:gemm_generic_f32:conv3x3'] == len(_rows('D', op='conv3', res=24))
    assert d['variant:split_conv3:conv3x3'] == len(_rows('D', op='conv3', tag='conv3x3', res=48)) + len(_rows('D', op='conv3', tag='conv3x3', res=96))
    assert d["variant:split_gemm:attn_gemm"] == 6 and d['variant:split_gemm:conv1x1'] == len(_rows('D', op='conv1'))
    e = v('E', 'split')
    assert e["variant:split_gemm:attn_gemm"] == 3 and e["variant:gemm_generic_f32:attn_gemm"] == 3      # q k^T (K = 128) stays; softmax v (K = 400) falls back
    ef = v('E', 'fast')
    assert ef["variant:mfma_gemm:attn_gemm"] == 3 and ef["variant:gemm_generic_bf16:attn_gemm"] == 3
    assert e['variant:split_conv3:conv3x3'] == len(_rows('E', op='conv3', tag='conv3x3', res=80))
    f = v('F', 'split')
    assert f.get('variant:conv3x3_planes_out:conv3x3', 0) == 0 and f['variant:split_conv3:conv3x3'] == len(_rows('F', op='conv3', tag='conv3x3', res=48))
    assert v('G', 'fast')['variant:halo_conv:conv_out'] == 1
    assert v('H', 'split')['variant:gemm_generic_f32:conv1x1'] == 1 and v('H', 'fast')['variant:gemm_generic_bf16:conv1x1'] == 1
    m = v('M64', 'split')                                                     # on the grid: matrix cores and tile statistics wherever a 3x3 conv produced the tensor
    assert not any('gemm_generic_f32' in k for k in m) and m['variant:gn_stats_pass:gn'] == 2 and m['variant:gn_stats_tiles:gn'] == 14
    assert v('M_A', 'split') == a
