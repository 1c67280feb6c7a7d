"""The 'conv2' and 'nearest' HQ-VAE variants (``hqt_config.s1_resample``) on the MI355X, through the C ABI (``Engine``) and through
``HQVAEStage1``, against the reference's own outputs (tests/golden/g14_resample_*.npz, tools/gen_golden_resample.py).

Bars: EXACT and SPLIT pixels and fp32 tensors within 1e-4, EXACT codes bit-identical (the fixtures sit >= 4e-4 from any argmin
tie), SPLIT / FAST codes the exact nearest ones of the device's own quantiser input.  FAST decode shares every kernel after the
lookup with the pixelshuffle model, so its bar is the one tests/test_gpu_parity.py::test_decode_fast_tolerance uses for this shape.
"""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT, HqtError
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.sampling import rearrange_codes, sampling_ihqgpt
from hqtransformer_amd.spec import Stage1Spec
from oracle import hqt_oracle as O
from tests.helpers import gate, load, stage1_from_fixture, stage2_from_fixture
from tests.resample_ref import ResampleOracle

pytestmark = pytest.mark.gpu
PIXEL_TOL = 1e-4
VARIANTS = ('conv2', 'nearest')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HQT_ERR_STATE, HQT_ERR_SHAPE, HQT_ERR_MISSING_WEIGHT = -3, -5, -6


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def np_(t):
    return t.detach().cpu().numpy()


def engine_s1(spec, weights, max_batch):
    e = Engine(None, spec, dev(), max_batch)
    e.load(stage1=weights)
    e.finalize()
    return e


def fixture(variant):
    fx = load(f'g14_resample_{variant}.npz')
    spec = Stage1Spec(**json.loads(str(fx['spec'])))
    return fx, spec, synth.stage1_weights(spec, int(fx['weight_seed']), 'fixture', encoder=True)


def _excess_distance(resid, emb, codes):
    """float64 d(z, e[code]) - min_n d(z, e[n]) per row: 0 where the code is the nearest one."""
    z = np.ascontiguousarray(resid.transpose(0, 2, 3, 1)).reshape(-1, resid.shape[1]).astype(np.float64)
    e = emb.astype(np.float64)
    d = (z ** 2).sum(1, keepdims=True) + (e ** 2).sum(1)[None] - 2 * z @ e.T
    return d[np.arange(len(z)), codes.reshape(-1)] - d.min(1)


def _seq(ct, cb):
    """code grids -> the sampler's [B, (r/2)^2], [B, (r/2)^2, 4] (the inverse of sampling_hqmodel.py:119-120)"""
    B, rt = ct.shape[0], ct.shape[1]
    return ct.reshape(B, rt * rt), cb.reshape(B, rt, 2, rt, 2).permute(0, 1, 3, 2, 4).reshape(B, rt * rt, 4)


@pytest.mark.parametrize('precision', [PRECISION_EXACT, PRECISION_SPLIT], ids=['exact', 'split'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_decode_vs_reference_fixture(variant, precision):
    """hqt_decode and hqt_decode_seq, three code combinations.  The bottom-only decode of 'conv2' carries upsample_t.bias (the
    reference runs upsample_t over a zero quant_t, generator.py:339-342, 316)."""
    fx, spec, weights = fixture(variant)
    eng = engine_s1(spec, {k: v for k, v in weights.items() if not k.startswith(('encoder.', 'quant_conv_b.', 'down_t.'))}, 2)
    assert not eng.has_encoder
    ct, cb = torch.from_numpy(fx['code_t']), torch.from_numpy(fx['code_b'])
    st, sb = _seq(ct, cb)
    cases = (('pixels', ct, cb, st, sb), ('pixels_top_only', ct[:1], None, st[:1], None), ('pixels_bot_only', None, cb[:1], None, sb[:1]))
    for name, t, b, t_seq, b_seq in cases:
        px = np_(eng.decode(t, b, precision=precision))
        err = np.abs(px - fx[name]).max()
        print(f'{variant} precision {precision} {name}: max |diff| {err:.3g}')
        assert err <= PIXEL_TOL, name
        px_seq = np_(eng.decode(t_seq, b_seq, precision=precision, seq_layout=True))
        assert np.array_equal(px_seq, px), name          # the rearranges are pure addressing
    clamped = np_(eng.decode(ct, cb, precision=precision, clamp01=True))
    np.testing.assert_allclose(clamped, O.postprocess(fx['pixels']), atol=PIXEL_TOL)
    eng.range_check()                                    # SPLIT: hqt_range_check == HQT_OK (raises otherwise); a no-op for EXACT


@pytest.mark.parametrize('variant', VARIANTS)
def test_encode_exact_vs_reference_fixture(variant):
    fx, spec, weights = fixture(variant)
    B, E, r = int(fx['B']), spec.embed_dim, spec.z_res
    eng = engine_s1(spec, weights, B)
    assert eng.has_encoder
    o = eng.encode(torch.from_numpy(fx['images']), precision=PRECISION_EXACT, want_quant=True, want_resid=True, want_recon=True, want_diff=True)
    assert tuple(o['quant'][0].shape) == (B, E, r // 2, r // 2) and tuple(o['resid'][0].shape) == (B, E, r // 2, r // 2)
    for l in range(2):
        for key in ('resid', 'quant'):
            err = np.abs(np_(o[key][l]) - fx[f'{key}_{l}']).max()
            print(f'{variant} exact {key}_{l}: max |diff| {err:.3g}')
            assert err <= PIXEL_TOL, (key, l)
        assert np.array_equal(np_(o['codes'][l]).reshape(-1), fx[f'enc_code_{l}'].reshape(-1)), l
        assert abs(float(o['diff'][l]) - float(fx[f'diff_{l}'])) <= 1e-4 * float(fx[f'diff_{l}']), l
    assert np.abs(np_(o['recon']) - fx['recon']).max() <= PIXEL_TOL
    rec = eng.decode(o['codes'][0], o['codes'][1], precision=PRECISION_EXACT)
    assert np.abs(np_(rec) - fx['reconstruction']).max() <= PIXEL_TOL
    # a smaller batch than max_batch, and the same rows again: nothing depends on what an earlier call left in the workspace
    o1 = eng.encode(torch.from_numpy(fx['images'][1:2]), precision=PRECISION_EXACT)
    assert np.array_equal(np_(o1['codes'][0]), np_(o['codes'][0])[1:2]) and np.array_equal(np_(o1['codes'][1]), np_(o['codes'][1])[1:2])


@pytest.mark.parametrize('precision', [PRECISION_SPLIT, PRECISION_FAST], ids=['split', 'fast'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_encode_split_and_fast_pick_the_nearest_code(variant, precision):
    """down_t, upsample_t and the distance GEMM stay fp32 in every precision: every chosen code is the exact nearest one of the
    device's own quantiser input (0 up to 1e-4 ties)."""
    fx, spec, weights = fixture(variant)
    eng = engine_s1(spec, weights, int(fx['B']))
    o = eng.encode(torch.from_numpy(fx['images']), precision=precision, want_resid=True, want_quant=True)
    eng.range_check()
    cbs = [weights['quantize_t.embedding'], weights['quantize_b.embedding']]
    for l in range(2):
        resid, codes = np_(o['resid'][l]), np_(o['codes'][l])
        assert np.isfinite(resid).all()
        excess = _excess_distance(resid, cbs[l], codes).max()
        print(f'{variant} precision {precision} level {l}: excess distance {excess:.3g}, '
              f'code agreement with the fp32 reference {(codes.reshape(-1) == fx[f"enc_code_{l}"].reshape(-1)).mean():.3f}')
        assert excess <= 1e-4, l
    if precision == PRECISION_SPLIT:                    # fp32-accurate: the tensors themselves stay within the bar
        for l in range(2):
            assert np.abs(np_(o['resid'][l]) - fx[f'resid_{l}']).max() <= PIXEL_TOL, l


def test_fast_decode_error_next_to_the_pixelshuffle_model():
    """FAST decode error of the two variants and of the pixelshuffle model of the same shape (g5_decode_64), measured in one run.
    The variants share every kernel after the lookup, so all three meet the bars test_decode_fast_tolerance sets for this shape."""
    cases = [('pixelshuffle', load('g5_decode_64.npz'))] + [(v, load(f'g14_resample_{v}.npz')) for v in VARIANTS]
    for name, fx in cases:
        spec, weights = stage1_from_fixture(fx)
        eng = engine_s1(spec, weights, 2)
        px = np_(eng.decode(torch.from_numpy(fx['code_t']), torch.from_numpy(fx['code_b']), precision=PRECISION_FAST))
        d = np.abs(px - fx['pixels'])
        print(f'FAST decode {name}: max {d.max():.4g} mean {d.mean():.4g} (pixel span {fx["pixels"].max() - fx["pixels"].min():.3g})')
        gate(f'resample.decode_fast.{name}.max', d.max(), 0.06)
        gate(f'resample.decode_fast.{name}.mean', d.mean(), 1e-2)


def test_error_paths():
    fx, spec, weights = fixture('conv2')
    E = spec.embed_dim
    # conv2 without upsample_t.*: decode needs it, so finalize fails
    eng = Engine(None, spec, dev(), 1)
    eng.load(stage1={k: v for k, v in weights.items() if not k.startswith('upsample_t.')})
    with pytest.raises(HqtError, match='upsample_t') as ei:
        eng.finalize()
    assert ei.value.code == HQT_ERR_MISSING_WEIGHT
    eng.close()
    # conv2 without down_t.*: decodes, but hqt_encode returns HQT_ERR_STATE
    eng = engine_s1(spec, {k: v for k, v in weights.items() if not k.startswith('down_t.')}, 1)
    assert not eng.has_encoder
    px = np_(eng.decode(torch.from_numpy(fx['code_t'][:1]), torch.from_numpy(fx['code_b'][:1]), precision=PRECISION_EXACT))
    assert np.abs(px - fx['pixels'][:1]).max() <= PIXEL_TOL
    with pytest.raises(HqtError, match='down_t') as ei:
        eng.encode(torch.from_numpy(fx['images'][:1]))
    assert ei.value.code == HQT_ERR_STATE
    eng.close()
    # a pixelshuffle-shaped [n_embed, 4E] top codebook on a conv2 handle
    bad = dict(weights)
    bad['quantize_t.embedding'] = np.zeros((spec.n_embed, 4 * E), np.float32)
    eng = Engine(None, spec, dev(), 1)
    eng.load(stage1=bad)
    with pytest.raises(HqtError, match='quantize_t') as ei:
        eng.finalize()
    assert ei.value.code == HQT_ERR_SHAPE
    eng.close()


@pytest.mark.parametrize('variant', VARIANTS)
def test_surface_encode_decode_roundtrip(variant):
    """HQVAEStage1.encode / get_codes / forward / decode_code with the fixture's weights (default precision: SPLIT)."""
    fx, spec, weights = fixture(variant)
    from hqtransformer_amd.models import HQVAEStage1
    m = HQVAEStage1(spec)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    m.to('cuda')
    x = torch.from_numpy(fx['images'])
    quant_t, quant_b, diff_t, diff_b, (code_t, code_b, h_b) = m.encode(x, precision='exact')
    assert np.array_equal(np_(code_t), fx['enc_code_0'].reshape(-1)) and np.array_equal(np_(code_b), fx['enc_code_1'].reshape(-1))
    assert np.abs(np_(quant_t) - fx['quant_0']).max() <= PIXEL_TOL and np.abs(np_(quant_b) - fx['quant_1']).max() <= PIXEL_TOL
    assert np.abs(np_(h_b) - fx['resid_1']).max() <= PIXEL_TOL
    gt, gb = m.get_codes(x, precision='exact')
    assert np.array_equal(np_(gt), np_(code_t)) and np.array_equal(np_(gb), np_(code_b))
    assert np.abs(np_(m(x, precision='exact')) - fx['reconstruction']).max() <= PIXEL_TOL
    px = m.decode_code(torch.from_numpy(fx['code_t']), torch.from_numpy(fx['code_b']))          # SPLIT, range-checked
    assert np.abs(np_(px) - fx['pixels']).max() <= PIXEL_TOL
    assert np.abs(np_(m.decode_code(None, torch.from_numpy(fx['code_b'][:1]))) - fx['pixels_bot_only']).max() <= PIXEL_TOL


@pytest.mark.parametrize('variant', VARIANTS)
def test_tiny_config_end_to_end(variant):
    """sampling_ihqgpt + decode_code from configs/tiny-cls-<variant>.yaml: stage 2 is untouched, so under G4's noise and weights the codes
    are G4's; the pixels equal the numpy restatement on those codes."""
    fx = load('g4_tiny_cls.npz')
    s2, w2 = stage2_from_fixture(fx)
    cfg = load_config(os.path.join(ROOT, 'configs', f'tiny-cls-{variant}.yaml'), [f'stage2.hparams.n_classes={s2.n_classes}'])
    m = ImageGPT2(cfg, seed=5)
    assert m.stage1.spec.resample == variant
    m.stage2.load_state_dict({k: torch.from_numpy(v) for k, v in w2.items()})
    m.to('cuda').eval()
    B, n = int(fx['B']), int(fx['n_steps'])
    noise = synth.exp_noise(int(fx['noise_seed']), n, B, s2.vocab_top)
    ct, cb = sampling_ihqgpt(m.stage2, num_candidates=B, cond=7, use_fp16=False, is_tqdm=False, max_seq_len=n, noise=torch.from_numpy(noise))
    assert np.array_equal(np_(ct), fx['codes_top_0']) and np.array_equal(np_(cb), fx['codes_bot_0'])
    gt, gb = rearrange_codes(ct, cb, 8)
    w1 = {k: v.numpy() for k, v in m.stage1.state_dict().items()}
    want = ResampleOracle(m.stage1.spec, w1).decode_code(np_(gt), np_(gb))
    for prec in ('exact', 'split'):
        assert np.abs(np_(m.stage1.decode_code(gt, gb, precision=prec)) - want).max() <= PIXEL_TOL, prec
    assert np.abs(np_(m.stage1.decode_sequences(ct, cb, precision='exact')) - want).max() <= PIXEL_TOL
