"""Shared by tests/test_offgrid_stage1_host.py and tests/test_gpu_offgrid_stage1.py: HQ-VAE decoders / encoders hqt_create accepts (ch % 32 == 0, any
ch_mult, any resolution the level count divides) that lie OFF the grid every other stage-1 test sits on (resolutions 8 .. 1024 powers of two, ch in
{32, 64, 128} x {1, 2, 4}: 1, 2, 4, 8 or 16 channels per GroupNorm group, every feature-map edge a power of two) -- shapes at which the dispatchers of
csrc/engine.hip (s1_norm, s1_plain, s1_conv, the attention products, decode_chunk's conv_out branch) pick kernels nothing else runs.  Every case:
num_res_blocks 1, n_embed 256, synth.stage1_weights(spec, seed, 'fixture'), 3 images of random codes, the CPU oracle (oracle/hqt_oracle.py) as checker.

case  off the grid in
A     192 channels (6 per group): every conv stays % 64 (matrix cores in SPLIT and FAST) while every statistics / apply / operand pass at 192 is the
      generic one (C / 8 = 24 does not divide 256); N = 192 % 128 != 0: the LDS-resident SPLIT conv, not the ring kernel
B     96 channels (3 per group) fall back inside SPLIT, 192 do not; K = 48 at post_quant_conv and conv_in; conv_out_direct at Cin = 96
C     160 channels (5 per group), K = 1440, no channel count % 64: every conv of SPLIT falls back (the one SPLIT kernel left is softmax x v, K = hw = 64)
D     maps of 24, 48, 96: at 24 W % 16 != 0 -- the 3x3 convs fall back while the 1x1 convs and the attention products (hw = 576) do not; M = 1728
E     maps of 20, 40, 80: at 20 H % 8 != 0, hw = 400 (attention K % 64 != 0, K % 32 != 0, softmax rows of 400); at 40 H % 8 == 0 but W % 16 != 0
F     no final upsampling (use_init_downsample False): ring kernels at 48 (N = 128), 24 falls back
G     three levels 20 -> 160: FAST's narrow conv_out (M >= 4096) with 16-row halo tiles at H = 160
H     D with three code levels at embed_dim 16: quant_gather3 and the three-level entry at a 6 / 12 / 24 code pyramid, post_quant K = 16
M64   the wide config of tests/test_gpu_split.py, M_A = case A: +30 on four conv biases -> |group mean| / std of 28 .. 58 at eight of the sixteen GroupNorms
      (variance as E[x^2] - mean^2 from fp32 partial sums cancels there), pixels still O(1)

variants(name, precision) restates the dispatch conditions as data (plan(name): one row per conv / GEMM / statistics pass with the documented
predicates evaluated) and predicts the `variant:*` counters of one timed decode; the GPU test compares the engine's report with it."""
from collections import Counter, namedtuple

import numpy as np

from hqtransformer_amd import synth
from hqtransformer_amd.spec import Stage1Spec, decoder_plan
from oracle import hqt_oracle as O
from tests.helpers import _synth_images

N_IMAGES = 3
BIAS_SHIFT = 30.0
SHIFTED = ('decoder.conv_in.bias', 'decoder.mid.block_1.conv1.bias', 'decoder.mid.attn_1.proj_out.bias', 'decoder.up.1.upsample.conv.bias')


def _spec(ch, ch_mult, attn, resolution, z=64, E=32, **kw):
    return Stage1Spec(ch=ch, ch_mult=list(ch_mult), num_res_blocks=1, attn_resolutions=list(attn), resolution=resolution, z_channels=z, embed_dim=E,
                      n_embed=256, **kw)


# name -> (spec, weight seed, code seed, bias shift)
CASES = {
    'A': (_spec(64, [1, 3], [16], 64), 911, 912, 0.0),
    'B': (_spec(96, [1, 2], [16], 64, z=48, E=24), 913, 914, 0.0),
    'C': (_spec(160, [1, 1], [8], 32, z=32, E=16), 915, 916, 0.0),
    'D': (_spec(64, [1, 2], [24], 96), 917, 918, 0.0),
    'E': (_spec(64, [1, 2], [20], 80), 919, 920, 0.0),
    'F': (_spec(128, [1, 2], [24], 48, use_init_downsample=False), 921, 922, 0.0),
    'G': (_spec(64, [1, 1, 2], [20], 160), 923, 924, 0.0),
    'H': (_spec(64, [1, 2], [24], 96, E=16, code_levels=3), 925, 926, 0.0),
    'M64': (_spec(64, [1, 2], [16], 64), 927, 928, BIAS_SHIFT),
    'M_A': (_spec(64, [1, 3], [16], 64), 911, 912, BIAS_SHIFT),
}
PLAIN = tuple(n for n in CASES if not n.startswith('M'))
LARGE_MEAN = ('M64', 'M_A')
# z_res and the code grids (coarse -> fine) of each case
GRIDS = {'A': (16, (8, 16)), 'B': (16, (8, 16)), 'C': (8, (4, 8)), 'D': (24, (12, 24)), 'E': (20, (10, 20)), 'F': (24, (12, 24)),
         'G': (20, (10, 20)), 'H': (24, (6, 12, 24)), 'M64': (16, (8, 16)), 'M_A': (16, (8, 16))}
ENCODE = ('A', 'D', 'E')
ENCODE_IMAGE_SEED = {'A': 931, 'D': 932, 'E': 933}

_INPUTS, _WANT, _ENC = {}, {}, {}


def inputs(name):
    """(spec, weights, codes): codes is the list of int64 grids [3, r_l, r_l], coarse -> fine."""
    if name not in _INPUTS:
        spec, wseed, cseed, shift = CASES[name]
        weights = synth.stage1_weights(spec, wseed, 'fixture')
        if shift:
            for k in SHIFTED:
                weights[k] = (weights[k] + np.float32(shift)).astype(np.float32)
        r = np.random.default_rng(cseed)
        codes = [r.integers(0, spec.n_embed, (N_IMAGES, g, g)) for g in GRIDS[name][1]]
        _INPUTS[name] = (spec, weights, codes)
    return _INPUTS[name]


def oracle_decode(spec, weights, codes):
    o = O.OracleStage1(spec, weights)
    return o.decode_codes3(codes) if spec.code_levels == 3 else o.decode_code(codes[0], codes[1])


def oracle_decode_f64(spec, weights, codes):
    """The same oracle graph in fp64: its module-level F32 is np.float64 for the call (weights, im2col buffers, casts)."""
    old, O.F32 = O.F32, np.float64
    try:
        return oracle_decode(spec, weights, codes)
    finally:
        O.F32 = old


def want(name):
    """The oracle's pixels of a case, computed once.  Callers must not write into the array."""
    if name not in _WANT:
        px = oracle_decode(*inputs(name))
        px.setflags(write=False)
        _WANT[name] = px
    return _WANT[name]


def encode_inputs(name):
    """(spec, weights with the encoder, images [3, 3, R, R], the oracle's encode of them), computed once."""
    if name not in _ENC:
        spec, wseed, _, _ = CASES[name]
        weights = synth.stage1_weights(spec, wseed, 'fixture', encoder=True)
        x = _synth_images(ENCODE_IMAGE_SEED[name], N_IMAGES, spec.resolution)
        _ENC[name] = (spec, weights, x, O.OracleStage1(spec, weights).encode(x))
    return _ENC[name]


# ------------------------------------------------------------------------------------------ the dispatch conditions as data
# One row per launch site of a decode, in execution order.  op: 'conv3' | 'conv1' | 'attn' (a product of two activation tensors) | 'gn'.
# tag: the timing slot tag of the site.  res: output map edge; K: reduction length; the booleans are the documented shape conditions.
Row = namedtuple('Row', 'op tag layer res cin cout K c64 h8 w16 k64 k32 cpg_pow2 fixed_map src dst up nchw resid')


def _pow2_group(C):                 # conv_halo_stats_ok: channels per group a power of two <= 64 dividing 128
    cpg = C // 32
    return C % 32 == 0 and cpg <= 64 and cpg & (cpg - 1) == 0 and 128 % cpg == 0


def _fixed_map(C):                  # gn_fixed_ok / sp_fixed_ok: C / 8 divides 256
    return C % 8 == 0 and C // 8 <= 256 and 256 % (C // 8) == 0


def _row(op, tag, layer, res, cin, cout, K, src, dst, up=False, nchw=False, resid=False):
    gnC = cin if op == 'gn' else cout
    return Row(op, tag, layer, res, cin, cout, K, cin % 64 == 0, res % 8 == 0, res % 16 == 0, K % 64 == 0, K % 32 == 0, _pow2_group(gnC), _fixed_map(gnC),
               src, dst, up, nchw, resid)


def plan(name):
    """The decode of a case as rows: a Python restatement of build_decoder_plan + decode_chunk + s1_layer (csrc/engine.hip).  src / dst name the
    rotating activation buffers the way the engine swaps them, so 'which conv produced the tensor this GroupNorm reads' is data too."""
    spec = CASES[name][0]
    rows = []
    E = spec.embed_dim
    cur, t1, t2 = 'act0', 'act1', 'act2'
    kq = E if spec.code_levels == 3 else 2 * E
    rows.append(_row('conv1', 'conv1x1', 'post_quant_conv_b', spec.z_res, kq, spec.z_channels, kq, 'quant', cur))
    for l in decoder_plan(spec):
        res, hw = l.res, l.res * l.res
        if l.kind in ('conv3', 'upconv'):
            ro = 2 * res if l.kind == 'upconv' else res
            rows.append(_row('conv3', 'conv3x3', l.name, ro, l.cin, l.cout, 9 * l.cin, cur, t1, up=l.kind == 'upconv'))
            cur, t1 = t1, cur
        elif l.kind == 'res':
            rows.append(_row('gn', 'gn', l.name + '.norm1', res, l.cin, l.cin, hw, cur, None))
            rows.append(_row('conv3', 'conv3x3', l.name + '.conv1', res, l.cin, l.cout, 9 * l.cin, cur, t1))
            outbuf = t2
            if l.cin != l.cout:
                rows.append(_row('conv1', 'conv1x1', l.name + '.nin_shortcut', res, l.cin, l.cout, l.cin, cur, t2))
                outbuf = cur
            rows.append(_row('gn', 'gn', l.name + '.norm2', res, l.cout, l.cout, hw, t1, None))
            rows.append(_row('conv3', 'conv3x3', l.name + '.conv2', res, l.cout, l.cout, 9 * l.cout, t1, outbuf, resid=True))
            if outbuf == t2:
                cur, t2 = t2, cur
        elif l.kind == 'attn':
            C = l.cin
            rows.append(_row('gn', 'gn', l.name + '.norm', res, C, C, hw, cur, None))
            for c in 'qkv':
                rows.append(_row('conv1', 'conv1x1', f'{l.name}.{c}', res, C, C, C, cur, 'a' + c, nchw=c == 'v'))
            rows.append(_row('attn', 'attn_gemm', l.name + '.qk', res, C, hw, C, 'aq', 'as'))
            rows.append(_row('attn', 'attn_gemm', l.name + '.sv', res, hw, C, hw, 'as', 'ao'))
            rows.append(_row('conv1', 'conv1x1', l.name + '.proj_out', res, C, C, C, 'ao', t1, resid=True))
            cur, t1 = t1, cur
        else:
            rows.append(_row('gn', 'gn', 'decoder.norm_out', res, l.cin, l.cin, hw, cur, None))
            rows.append(_row('conv3', 'conv_out', 'decoder.conv_out', res, l.cin, l.cout, 9 * l.cin, cur, 'out', nchw=True))
    return rows


def _split_conv_ok(r):
    """split_conv3_ok (3x3: Cin % 64, H % 8, W % 16; the NCHW store up to 32 channels) / split_gemm_ok (1x1: K % 64)."""
    if r.op == 'conv3':
        return r.c64 and r.h8 and r.w16 and (r.cout <= 32 if r.nchw else r.cout % 8 == 0)
    return r.k64


def variants(name, precision, n_images=N_IMAGES):
    """The `variant:*` counters of ONE timed decode of n_images images of the case (one chunk), predicted from plan(name): {slot name: launches}.
    precision: 'exact' | 'split' | 'fast'.  Only FAST looks at the number of images: its halo-tile kernel wants a grid that fills the chip."""
    rows = plan(name)
    n = Counter()
    ready = None                    # the buffer whose producing 3x3 conv left per-tile statistics (S1Ctx::gn_ready)
    M_of = lambda r: n_images * r.res * r.res
    i = 0
    while i < len(rows):
        r = rows[i]
        if r.op == 'gn':
            conv = rows[i + 1]
            if precision == 'exact':
                n['variant:gn_stats_two_pass:gn'] += 1
            elif precision == 'fast':
                n['variant:gn_stats_tiles:gn' if ready == r.src else 'variant:gn_stats_pass:gn'] += 1
            elif conv.tag == 'conv_out' and conv.cin % 32 == 0 and conv.res % 16 == 0:       # conv_out_direct_ok: statistics, then ONE fp32 kernel
                n['variant:gn_stats_tiles:gn' if ready == r.src else 'variant:gn_stats_pass:gn'] += 1
                n['variant:conv_out_direct:conv_out'] += 1
                i += 2
                continue
            elif _split_conv_ok(conv):
                n['variant:gn_stats_tiles:gn' if ready == r.src else 'variant:gn_stats_pass:gn'] += 1
            else:
                n['variant:gn_stats_two_pass:gn'] += 1
            i += 1
            continue
        if ready == r.dst:
            ready = None            # the tensor is being overwritten
        if r.op == 'attn':
            if precision == 'fast':
                kern = 'mfma_gemm' if r.k32 else 'gemm_generic_bf16'
            elif precision == 'split':
                kern = 'split_gemm' if r.k64 else 'gemm_generic_f32'
            else:
                kern = 'gemm_generic_f32'
            n[f'variant:{kern}:attn_gemm'] += 1
        elif precision == 'exact':
            n[f'variant:gemm_generic_f32:{r.tag}'] += 1
        elif precision == 'split':
            if not _split_conv_ok(r):
                n[f'variant:gemm_generic_f32:{r.tag}'] += 1
            elif r.op == 'conv1':
                n[f'variant:split_gemm:{r.tag}'] += 1
            else:
                n[f'variant:split_conv3:{r.tag}'] += 1
                if not r.nchw and r.cpg_pow2:
                    ready = r.dst
                # a ResnetBlock in front of an upsampling conv emits the operand planes itself when both take the ring kernel (N % 128 == 0)
                nxt = rows[i + 1] if i + 1 < len(rows) else None
                if r.resid and nxt is not None and nxt.up and nxt.cin == r.cout and _split_conv_ok(nxt) and r.cout % 128 == 0:
                    n['variant:conv3x3_planes_out:conv3x3'] += 1
        else:                        # FAST: mfma_gemm_ok (K % 32, Cin % 32); the halo-tile kernel for big or narrow 3x3 shapes
            if not (r.k32 and r.cin % 32 == 0):
                n[f'variant:gemm_generic_bf16:{r.tag}'] += 1
            else:
                M, N = M_of(r), r.cout
                narrow = N < 32 and M >= 4096 and r.k64 and r.c64
                big = narrow or (N >= 128 and M >= 128 and ((M + 127) // 128) * ((N + 127) // 128) >= 96)
                halo = big and r.op == 'conv3' and r.c64 and r.h8 and r.w16 and (not r.resid if r.nchw else N % 8 == 0)
                n[f'variant:{"halo_conv" if halo else "mfma_gemm"}:{r.tag}'] += 1
                if halo and not r.nchw and r.cpg_pow2:
                    ready = r.dst
        i += 1
    return dict(n)
