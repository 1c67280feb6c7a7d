"""The bidirectional depth head of the two-level model (iHQGPT model_type 'bidirectional4', hierarchical_ar.py:791-878): configuration,
state-dict shapes and refusals, host side only (the GPU side: tests/test_gpu_bidirectional.py)."""
import json
import os
import types

import pytest

from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import make_config
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.spec import DEPTH_DECODINGS, Stage2Spec, stage2_param_shapes, stage2_spec_from_config
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'imagenet-12l-bidirectional.yaml')
TINY = os.path.join(ROOT, 'configs', 'tiny-cls.yaml')


def test_bidirectional_config_loads_as_depth_decoding_4():
    s2 = stage2_spec_from_config(load_config(CFG))
    assert s2.depth_decoding == 'bidirectional' and s2.levels == 2 and DEPTH_DECODINGS.index('bidirectional') == 4
    assert make_config(s2, None, 4, 64).depth_decoding == 4
    # same tensors as the 'parallel' model of the same size: a checkpoint of either loads by the same names
    par = stage2_spec_from_config(load_config(os.path.join(ROOT, 'configs', 'imagenet-12l.yaml')))
    assert par.depth_decoding == 'parallel-add' and make_config(par, None, 4, 64).depth_decoding == 0
    assert stage2_param_shapes(s2) == stage2_param_shapes(par)
    for t in ('hq-transformer/bidirectional', 'hq-transformer/bidirectional4'):
        assert stage2_spec_from_config(load_config(TINY, [f'stage2.type={t}'])).depth_decoding == 'bidirectional'


def test_bidirectional_state_dict_matches_the_reference_fixture():
    fx = load('g13_tiny_cls_bidirectional.npz')
    for key in ('spec', 'reduce_spec'):
        spec = Stage2Spec(**json.loads(str(fx[key])))
        assert spec.depth_decoding == 'bidirectional'
        if key == 'spec':
            want = {k: tuple(v) for k, v in json.loads(str(fx['param_shapes'])).items()}
            assert {k: tuple(v) for k, v in stage2_param_shapes(spec).items()} == want


@pytest.mark.parametrize('cfg_name,overrides', [
    ('tiny-cls.yaml', ['stage2.type=hq-transformer/bidirectional16']),          # only bot_win = 2 (ratio_bot2top 4)
    ('tiny-cls.yaml', ['stage2.type=hq-transformer/top2bot']),
    ('tiny-cls.yaml', ['stage2.type=hq-transformer']),                          # = top2bot
    ('tiny-txt.yaml', ['stage2.type=hq-transformer/bidirectional4']),           # text conditioning
    ('tiny-l3.yaml', ['stage2.decoding_type=bidirectional']),                   # three levels
])
def test_bidirectional_variants_that_are_refused(cfg_name, overrides):
    cfg = load_config(os.path.join(ROOT, 'configs', cfg_name), overrides)
    with pytest.raises(NotImplementedError):
        stage2_spec_from_config(cfg)


def test_given_top_code_is_refused_by_the_bidirectional_head():
    spec = stage2_spec_from_config(load_config(TINY, ['stage2.type=hq-transformer/bidirectional4']))

    def no_engine(*a, **k):
        raise AssertionError('the refusal must come before any engine is built')
    model = types.SimpleNamespace(spec=spec, use_txt_cond=False, use_cls_cond=True, engine=no_engine)
    with pytest.raises(ValueError, match='given_top_code'):
        sampling_ihqgpt(model, 2, 3, given_top_code=[[1, 2]], max_seq_len=2)
