"""The 'conv2' and 'nearest' HQ-VAE variants (``stage1.hparams_aux.upsample``; generator.py:193-242), host side: configuration,
refusals, state-dict shapes, and the numpy restatement of tests/resample_ref.py against the reference's own outputs
(tests/golden/g14_resample_*.npz, tools/gen_golden_resample.py).  The GPU side: tests/test_gpu_resample.py."""
import json
import os

import numpy as np
import pytest

from hqtransformer_amd import synth
from hqtransformer_amd._lib import ABI_VERSION, RESAMPLE_CONV2, RESAMPLE_NEAREST, RESAMPLE_PIXELSHUFFLE
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import make_config
from hqtransformer_amd.spec import (STAGE1_RESAMPLES, Stage1Spec, stage1_encoder_param_shapes, stage1_is_encoder_key, stage1_param_shapes,
                                    stage1_spec_from_config)
from tests.helpers import load
from tests.resample_ref import ResampleOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4          # the project's bar for fp32 tensors and pixels
VARIANTS = ('conv2', 'nearest')


def cfg_path(name):
    return os.path.join(ROOT, 'configs', name)


@pytest.mark.parametrize('variant', VARIANTS)
def test_new_configs_load(variant):
    assert ABI_VERSION == 9 and STAGE1_RESAMPLES == ('pixelshuffle', 'nearest', 'conv2')
    want = {'conv2': RESAMPLE_CONV2, 'nearest': RESAMPLE_NEAREST}[variant]
    for name in (f'imagenet-12l-{variant}.yaml', f'tiny-cls-{variant}.yaml'):
        s1 = stage1_spec_from_config(load_config(cfg_path(name)))
        assert s1.resample == variant and s1.code_levels == 2
        assert make_config(None, s1, 2, 1).s1_resample == want
        base = stage1_spec_from_config(load_config(cfg_path(name.replace(f'-{variant}', ''))))
        assert base.resample == 'pixelshuffle' and make_config(None, base, 2, 1).s1_resample == RESAMPLE_PIXELSHUFFLE
        assert {k: v for k, v in s1.__dict__.items() if k != 'resample'} == {k: v for k, v in base.__dict__.items() if k != 'resample'}
    # the override route, and nearest2 == nearest (generator.py:203-212: an empty kernel-size suffix means 2)
    over = stage1_spec_from_config(load_config(cfg_path('tiny-cls.yaml'), [f'stage1.hparams_aux.upsample={variant}']))
    assert over == stage1_spec_from_config(load_config(cfg_path(f'tiny-cls-{variant}.yaml')))
    assert stage1_spec_from_config(load_config(cfg_path('tiny-cls.yaml'), ['stage1.hparams_aux.upsample=nearest2'])).resample == 'nearest'


def test_spec_json_of_older_fixtures_still_loads():
    spec = Stage1Spec(**json.loads(str(load('g5_decode_64.npz')['spec'])))
    assert spec.resample == 'pixelshuffle'


@pytest.mark.parametrize('cfg_name,overrides', [
    ('tiny-cls.yaml', ['stage1.hparams_aux.upsample=conv4']),
    ('tiny-cls.yaml', ['stage1.hparams_aux.upsample=nearest4']),
    ('tiny-cls.yaml', ['stage1.hparams_aux.upsample=pixelshuffle4']),
    ('tiny-cls.yaml', ['stage1.hparams_aux.upsample=null']),
    ('tiny-cls-conv2.yaml', ['stage1.hparams_aux.decoding_type=add']),
    ('tiny-l3.yaml', ['stage1.hparams_aux.upsample=conv2']),                    # stage1.type hqvae: three levels
    ('tiny-l3.yaml', ['stage1.hparams_aux.upsample=nearest']),
])
def test_variants_that_are_refused(cfg_name, overrides):
    cfg = load_config(cfg_path(cfg_name), overrides)
    with pytest.raises(NotImplementedError, match='pixelshuffle.*nearest.*conv2'):
        stage1_spec_from_config(cfg)


@pytest.mark.parametrize('variant', VARIANTS)
def test_state_dict_matches_the_reference_fixture(variant):
    fx = load(f'g14_resample_{variant}.npz')
    spec = Stage1Spec(**json.loads(str(fx['spec'])))
    assert spec.resample == variant
    want = {k: tuple(v) for k, v in json.loads(str(fx['param_shapes'])).items()}
    mine = dict(stage1_param_shapes(spec))
    enc = dict(stage1_encoder_param_shapes(spec))
    assert not set(mine) & set(enc)
    mine.update(enc)
    assert {k: tuple(v) for k, v in mine.items()} == want
    assert mine['quantize_t.embedding'] == (spec.n_embed, spec.embed_dim)
    assert all(stage1_is_encoder_key(k) for k in enc) and not any(stage1_is_encoder_key(k) for k in stage1_param_shapes(spec))
    assert ('down_t.weight' in enc) == (variant == 'conv2') and ('upsample_t.weight' in stage1_param_shapes(spec)) == (variant == 'conv2')


@pytest.fixture(scope='module', params=VARIANTS)
def case(request):
    fx = load(f'g14_resample_{request.param}.npz')
    spec = Stage1Spec(**json.loads(str(fx['spec'])))
    weights = synth.stage1_weights(spec, int(fx['weight_seed']), 'fixture', encoder=True)
    return request.param, fx, spec, ResampleOracle(spec, weights)


def test_fixture_is_well_conditioned(case):
    _, fx, _, _ = case
    assert fx['margins'].min() >= 4e-4          # the condition tools/gen_golden_resample.py picked the weight seed by


def test_numpy_decode_vs_reference(case):
    variant, fx, spec, orc = case
    ct, cb = fx['code_t'], fx['code_b']
    for name, got in (('pixels', orc.decode_code(ct, cb)), ('pixels_top_only', orc.decode_code(ct[:1], None)),
                      ('pixels_bot_only', orc.decode_code(None, cb[:1]))):
        err = np.abs(got - fx[name]).max()
        print(f'{variant} {name}: max |diff| {err:.3g}')
        assert err <= TOL, name
    if variant == 'conv2':
        # the missing top level carries upsample_t.bias: decoding with a zero contribution instead is visibly different
        E, r = spec.embed_dim, spec.z_res
        qb = orc.w['quantize_b.embedding'][cb[:1]].transpose(0, 3, 1, 2)
        no_bias = orc.decoder(orc._conv('post_quant_conv_b', np.concatenate([np.zeros((1, E, r, r), np.float32), qb], axis=1)))
        assert np.abs(no_bias - fx['pixels_bot_only']).max() > 100 * TOL


def test_numpy_encode_vs_reference(case):
    variant, fx, spec, orc = case
    o = orc.encode(fx['images'])
    assert np.abs(o['h'] - fx['h']).max() <= TOL
    for l in range(2):
        assert np.array_equal(o['codes'][l].reshape(-1), fx[f'enc_code_{l}'].reshape(-1)), l
        for key in ('resid', 'quant'):
            err = np.abs(o[key][l] - fx[f'{key}_{l}']).max()
            print(f'{variant} {key}_{l}: max |diff| {err:.3g}')
            assert err <= TOL, (key, l)
        assert abs(float(o['diff'][l]) - float(fx[f'diff_{l}'])) <= 1e-4 * float(fx[f'diff_{l}']), l
    assert o['resid'][0].shape == (int(fx['B']), spec.embed_dim, spec.z_res // 2, spec.z_res // 2)
    assert np.abs(o['recon'] - fx['recon']).max() <= TOL
    assert np.abs(orc.decode(o['quant'][0], o['quant'][1]) - fx['reconstruction']).max() <= TOL
