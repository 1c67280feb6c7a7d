"""Completion from a code prefix on a text-conditional model (the prompt and the prefix share one prefill), the parts that need no GPU:
``check_prefix(text_prefix=True)``, the refusals that remain -- each before any engine is built -- and the prefix ``complete_images`` cuts for
text prompts.  The GPU side: tests/test_gpu_text_prefix.py."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import Engine, check_prefix
from hqtransformer_amd.pipeline import complete_images, grids_to_sequences
from hqtransformer_amd.sampling import sampling_hqtransformer, sampling_ihqgpt
from hqtransformer_amd.spec import stage2_spec_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spec_of(name):
    return stage2_spec_from_config(load_config(os.path.join(ROOT, 'configs', name), []))


def no_engine(*a, **k):
    raise AssertionError('the refusal must come before any engine is built')


def model_of(spec, engine=no_engine):
    return types.SimpleNamespace(spec=spec, use_txt_cond=spec.cond == 2, use_cls_cond=spec.cond == 1, engine=engine)


def prefix_of(spec, B, P, fill=1):
    return [torch.full((B, P) + ((4 ** l,) if l else ()), fill, dtype=torch.int64) for l in range(spec.levels)]


def test_check_prefix_takes_a_text_spec_on_request_only():
    spec = spec_of('tiny-txt.yaml')
    assert spec.cond == 2 and spec.levels == 2
    good = prefix_of(spec, 2, 4)
    with pytest.raises(ValueError, match='text conditioning'):                      # the default: today's refusal
        check_prefix(spec, 2, 16, good)
    with pytest.raises(ValueError, match='text_prefix=True'):
        check_prefix(spec, 2, 16, good, text_prefix=False)
    levels = check_prefix(spec, 2, 16, good, text_prefix=True)
    assert [tuple(l.shape) for l in levels] == [(2, 4), (2, 4, 4)] and all(torch.equal(a, b) for a, b in zip(levels, good))
    assert check_prefix(spec, 2, 16, None, text_prefix=True) is None
    # a class model does not care about the flag
    cls = spec_of('tiny-cls.yaml')
    assert check_prefix(cls, 2, 16, prefix_of(cls, 2, 4), text_prefix=True)[0].shape == (2, 4)


def test_text_prefixes_get_the_checks_of_class_models():
    spec = spec_of('tiny-txt.yaml')
    good = prefix_of(spec, 2, 4)
    for P, n in ((8, 8), (9, 8), (64, 64)):                                        # P >= n_steps
        with pytest.raises(ValueError, match='n_steps - 1'):
            check_prefix(spec, 2, n, prefix_of(spec, 2, P), text_prefix=True)
    with pytest.raises(ValueError, match='n_steps - 1'):
        check_prefix(spec, 2, 8, [p[:, :0] for p in good], text_prefix=True)
    with pytest.raises(ValueError, match='max_prefix=3'):
        check_prefix(spec, 2, 16, good, max_prefix=3, text_prefix=True)
    bad = [good[:-1], good + [good[-1]], good[0], [good[0], good[1][:, :3]], [good[0], good[1][..., :3]], [g[:1] for g in good],
           [g.float() for g in good]]
    for prefix in bad:
        with pytest.raises(ValueError):
            check_prefix(spec, 2, 16, prefix, text_prefix=True)
    for level in range(2):
        for value in (-1, spec.vocab_top):
            prefix = prefix_of(spec, 2, 4)
            prefix[level].view(-1)[3] = value
            with pytest.raises(IndexError, match=f'prefix\\[{level}\\]'):
                check_prefix(spec, 2, 16, prefix, text_prefix=True)
    # the sampler forwards the flag: the same refusals through sampling_ihqgpt, before any engine is built
    txt = torch.zeros((2, spec.ctx_len_txt), dtype=torch.int64)
    with pytest.raises(ValueError, match='n_steps - 1'):
        sampling_ihqgpt(model_of(spec), 1, txt, max_seq_len=4, prefix_codes=good, text_prefix=True)
    with pytest.raises(ValueError, match='text conditioning'):
        sampling_ihqgpt(model_of(spec), 1, txt, max_seq_len=16, prefix_codes=good)


def test_the_remaining_refusals_name_what_is_built():
    txt2 = spec_of('tiny-txt.yaml')
    # stage2_spec_from_config refuses the bidirectional head with text itself; a spec built by hand reaches check_prefix
    bidir = dataclasses.replace(txt2, depth_decoding='bidirectional')
    with pytest.raises(ValueError, match="'parallel' depth head"):
        check_prefix(bidir, 2, 16, prefix_of(bidir, 2, 4), text_prefix=True)
    l3 = dataclasses.replace(spec_of('tiny-l3.yaml'), cond=2, ctx_len_txt=16, vocab_txt=64)
    assert l3.levels == 3
    with pytest.raises(ValueError, match='two code levels'):
        check_prefix(l3, 2, 16, prefix_of(l3, 2, 4), text_prefix=True)
    txt = torch.zeros((2, 16), dtype=torch.int64)
    with pytest.raises(ValueError, match='text conditioning'):                      # the three-level sampler has no flag to forward
        sampling_hqtransformer(model_of(l3), 1, txt, max_seq_len=16, prefix_codes=prefix_of(l3, 2, 4))
    with pytest.raises(ValueError, match="'parallel' depth head"):
        sampling_ihqgpt(model_of(bidir), 1, txt, max_seq_len=16, prefix_codes=prefix_of(bidir, 2, 4), text_prefix=True)


def test_a_text_engine_without_room_refuses_before_the_library_is_touched():
    spec = spec_of('tiny-txt.yaml')
    eng = Engine.__new__(Engine)                     # no handle, no library: the check sits in front of both
    eng.s2, eng.max_prefix, eng.device, eng.lib, eng.h = spec, 0, torch.device('cuda:0'), None, None
    with pytest.raises(ValueError, match='max_prefix=0'):
        eng.sample(2, torch.zeros((2, spec.ctx_len_txt), dtype=torch.int64), 16, prefix=prefix_of(spec, 2, 5))


class _Stop(Exception):
    pass


def _stub_model(spec, grids, seen):
    """A model whose stage 1 returns ``grids`` and whose stage-2 engine records what the sampler hands it."""
    def engine(batch, n_steps, lane=0, max_prefix=0):
        seen['engine'] = (batch, n_steps, max_prefix)

        def sample(B, cond, n, **kw):
            seen['cond'], seen['prefix'] = cond, kw['prefix']
            raise _Stop
        return types.SimpleNamespace(sample=sample)
    stage2 = model_of(spec, engine)
    stage1 = types.SimpleNamespace(code_grids=lambda images, precision=None: grids)
    return types.SimpleNamespace(stage1=stage1, stage2=stage2)


@pytest.mark.parametrize('keep', [1, 5, 7])
def test_complete_images_cuts_the_same_prefix_for_text_as_for_class(keep):
    B, K = 3, 8
    rng = np.random.default_rng(keep)
    grids = [torch.from_numpy(rng.integers(0, 512, (B, K << l, K << l))) for l in range(2)]
    images = torch.zeros((B, 3, 64, 64))
    got = {}
    for name, cond in (('tiny-cls.yaml', 2), ('tiny-txt.yaml', torch.from_numpy(rng.integers(0, 300, (B, 16))))):
        spec, seen = spec_of(name), {}
        with pytest.raises(_Stop):
            complete_images(_stub_model(spec, grids, seen), images, keep, cond=cond, seed=1)
        assert seen['engine'] == (B, K * K, keep * K)            # room for the prefix that was asked
        got[name] = seen
    want = [s[:, :keep * K] for s in grids_to_sequences(grids)]
    for name, seen in got.items():
        assert all(torch.equal(a, b) for a, b in zip(seen['prefix'], want)), name
    assert tuple(got['tiny-txt.yaml']['cond'].shape) == (B, 16) and tuple(got['tiny-cls.yaml']['cond'].shape) == (B,)
