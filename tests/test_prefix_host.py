"""Completion from a code prefix (hqt_sample_prefix, hqt_set_max_prefix), the parts that need no GPU: the ABI additions, the refusals -- each
before any engine is built --, the merged-pass rule (one prefix length per pass) and the grid <-> sequence rearranges ``complete_images``
cuts the prefix with.  The GPU side: tests/test_gpu_prefix.py."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import Engine, check_prefix
from hqtransformer_amd.pipeline import Pending, _Step, check_mergeable, grids_to_sequences
from hqtransformer_amd.sampling import rearrange_levels, sampling_hqtransformer, sampling_ihqgpt
from hqtransformer_amd.spec import stage2_spec_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg(name, overrides=()):
    return load_config(os.path.join(ROOT, 'configs', name), list(overrides))


def no_engine(*a, **k):
    raise AssertionError('the refusal must come before any engine is built')


def model_of(spec):
    return types.SimpleNamespace(spec=spec, use_txt_cond=spec.cond == 2, use_cls_cond=spec.cond == 1, engine=no_engine)


def prefix_of(spec, B, P, fill=1):
    return [torch.full((B, P) + ((4 ** l,) if l else ()), fill, dtype=torch.int64) for l in range(spec.levels)]


def test_three_entry_points_are_added_and_no_struct_or_version_changes():
    """The feature adds entry points only: hqt_config, the option structs and the ABI version stay what they were (a caller built against
    the header of before keeps working), so max_prefix is set through hqt_set_max_prefix and is no field of hqt_config."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "hqt.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(hqt_config));', '  printf("s1_resample %zu\\n", offsetof(hqt_config, s1_resample));',
             '  printf("abi %d\\n", HQT_ABI_VERSION);', '  return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'l.c'), os.path.join(d, 'l')
        with open(src, 'w') as fp:
            fp.write('\n'.join(lines))
        subprocess.run(['gcc', '-o', exe, src], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    want = {k: int(v) for k, v in (l.split() for l in out.strip().splitlines())}
    assert want['abi'] == _lib.ABI_VERSION
    assert want['size'] == want['s1_resample'] + 4 == C.sizeof(_lib.hqt_config)       # s1_resample is still the last field
    assert _lib.hqt_config._fields_[-1][0] == 's1_resample' and not hasattr(_lib.hqt_config, 'max_prefix')
    for name, n_args in (('hqt_set_max_prefix', 2), ('hqt_sample_prefix', 14), ('hqt_sample_prefix_l3', 17)):
        assert name in _lib.exported_symbols() and len(_lib.SYMBOLS[name][1]) == n_args
    # hqt_sample keeps its signature
    assert len(_lib.SYMBOLS['hqt_sample'][1]) == 11 and len(_lib.SYMBOLS['hqt_sample_l3'][1]) == 13


def test_entry_points_are_exported_and_refuse_null():
    _lib.build()
    lib = _lib.load()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    names = {l.split()[-1] for l in nm.splitlines() if l.strip()}
    assert {'hqt_set_max_prefix', 'hqt_sample_prefix', 'hqt_sample_prefix_l3'} <= names
    assert lib.hqt_set_max_prefix(None, 4) == -1 and b'null' in lib.hqt_last_error()
    assert lib.hqt_sample_prefix(None, 1, None, None, None, 1, None, None, None, None, None, None, None, None) == -1
    assert b'null' in lib.hqt_last_error()
    assert lib.hqt_sample_prefix_l3(None, 1, None, None, None, 1, None, None, None, None, None, None, None, None, None, None, None) == -1


@pytest.mark.parametrize('name', ['tiny-cls.yaml', 'tiny-l3.yaml'])
def test_prefix_length_outside_the_run_is_refused(name):
    spec = stage2_spec_from_config(cfg(name))
    sampler = sampling_hqtransformer if spec.levels == 3 else sampling_ihqgpt
    for P, n in ((8, 8), (9, 8), (64, 64)):                                        # P >= n_steps
        with pytest.raises(ValueError, match='n_steps - 1'):
            sampler(model_of(spec), 2, 3, max_seq_len=n, prefix_codes=prefix_of(spec, 2, P))
    with pytest.raises(ValueError, match='n_steps - 1'):                              # an empty prefix is no prefix: pass None
        sampler(model_of(spec), 2, 3, max_seq_len=8, prefix_codes=[p[:, :0] for p in prefix_of(spec, 2, 1)])


def test_prefix_longer_than_max_prefix_is_refused_before_the_library_is_touched():
    spec = stage2_spec_from_config(cfg('tiny-cls.yaml'))
    with pytest.raises(ValueError, match='max_prefix=4'):
        check_prefix(spec, 2, 16, prefix_of(spec, 2, 5), max_prefix=4)
    assert check_prefix(spec, 2, 16, prefix_of(spec, 2, 4), max_prefix=4)[0].shape == (2, 4)
    eng = Engine.__new__(Engine)                     # no handle, no library: the check sits in front of both
    eng.s2, eng.max_prefix, eng.device, eng.lib, eng.h = spec, 0, torch.device('cuda:0'), None, None
    with pytest.raises(ValueError, match='max_prefix=0'):
        eng.sample(2, torch.zeros(2, dtype=torch.int64), 16, prefix=prefix_of(spec, 2, 5))


@pytest.mark.parametrize('name', ['tiny-cls.yaml', 'tiny-l3.yaml'])
def test_wrong_shapes_and_level_counts_are_refused(name):
    spec = stage2_spec_from_config(cfg(name))
    sampler = sampling_hqtransformer if spec.levels == 3 else sampling_ihqgpt
    good = prefix_of(spec, 2, 4)
    bad = [good[:-1],                                                      # a level missing
           good + [good[-1]],                                              # one too many
           good[0],                                                        # a bare tensor, not the list of levels
           [good[0]] + [g[:, :3] for g in good[1:]],                       # levels that disagree on P
           [good[0]] + [g[..., :3] for g in good[1:]],                     # wrong codes per position
           [g[:1] for g in good],                                          # wrong batch
           [g.float() for g in good]]                                      # not integer codes
    for prefix in bad:
        with pytest.raises(ValueError):
            sampler(model_of(spec), 2, 3, max_seq_len=16, prefix_codes=prefix)


@pytest.mark.parametrize('name', ['tiny-cls.yaml', 'tiny-l3.yaml'])
def test_out_of_vocabulary_codes_raise_index_error(name):
    spec = stage2_spec_from_config(cfg(name))
    sampler = sampling_hqtransformer if spec.levels == 3 else sampling_ihqgpt
    for level in range(spec.levels):
        for value in (-1, spec.vocab_top):
            prefix = prefix_of(spec, 2, 4)
            prefix[level].view(-1)[3] = value
            with pytest.raises(IndexError, match=f'prefix\\[{level}\\]'):
                sampler(model_of(spec), 2, 3, max_seq_len=16, prefix_codes=prefix)


def test_text_conditional_models_are_refused():
    spec = stage2_spec_from_config(cfg('tiny-txt.yaml'))
    txt = torch.zeros((2, spec.ctx_len_txt), dtype=torch.int64)
    with pytest.raises(ValueError, match='text conditioning'):
        sampling_ihqgpt(model_of(spec), 2, txt, max_seq_len=16, prefix_codes=prefix_of(spec, 2, 4))


def test_without_a_prefix_the_engine_is_asked_for_no_prefix_room():
    spec = stage2_spec_from_config(cfg('tiny-cls.yaml'))
    seen = {}

    class Stop(Exception):
        pass

    def engine(batch, n_steps, lane=0, max_prefix=0):
        seen['max_prefix'] = max_prefix
        raise Stop
    model = types.SimpleNamespace(spec=spec, use_txt_cond=False, use_cls_cond=True, engine=engine)
    with pytest.raises(Stop):
        sampling_ihqgpt(model, 2, 3, max_seq_len=16)
    assert seen['max_prefix'] == 0
    with pytest.raises(Stop):
        sampling_ihqgpt(model, 2, 3, max_seq_len=16, prefix_codes=prefix_of(spec, 2, 4))
    assert seen['max_prefix'] == 4                   # room for the prefix that was asked, not for every one the model could take


def _step(n, prefix=None, **kw):
    if prefix is not None:
        kw['prefix_codes'] = prefix
    return _Step(Pending(), n, 3, 1, 16, True, None, True, True, None, True, kw)


def test_a_merged_pass_has_one_prefix_length():
    spec = stage2_spec_from_config(cfg('tiny-cls.yaml'))
    a, b = _step(2, prefix_of(spec, 2, 4, fill=1)), _step(3, prefix_of(spec, 3, 4, fill=2))
    check_mergeable(b, a)                            # same P, different codes and sizes: one pass
    assert a.prefix_len() == 4 and _step(2).prefix_len() == 0
    for other in (_step(2, prefix_of(spec, 2, 5)), _step(2)):
        with pytest.raises(ValueError, match='prefix length'):
            check_mergeable(other, a)
        with pytest.raises(ValueError, match='prefix length'):
            check_mergeable(a, other)
    with pytest.raises(ValueError, match='must share max_seq_len'):          # the older rule still speaks for itself
        check_mergeable(_step(2, prefix_of(spec, 2, 4), top_k_top=5), a)
    check_mergeable(_step(2, prefix_of(spec, 2, 4), top_k_top=5), a, mixed_samplers=True)


@pytest.mark.parametrize('levels', [2, 3])
def test_grid_and_sequence_layouts_are_inverse_and_rows_are_prefixes(levels):
    B, K = 2, 4
    rng = np.random.default_rng(levels)
    seqs = [torch.from_numpy(rng.integers(0, 99, (B, K * K) + ((4 ** l,) if l else ()))) for l in range(levels)]
    grids = rearrange_levels(seqs, K)
    back = grids_to_sequences(list(grids))
    assert all(torch.equal(a, b) for a, b in zip(seqs, back))
    # the first keep_rows rows of the top grid are the first keep_rows * K positions, and on level l the first keep_rows << l grid rows
    for keep in (1, 3):
        cut = [s[:, :keep * K] for s in back]
        for l, (g, c) in enumerate(zip(grids, cut)):
            rows = g[:, :keep << l]                  # [B, keep << l, K << l]
            k = 2 ** l
            want = rows.reshape(B, keep, k, K, k).permute(0, 1, 3, 2, 4).reshape(B, keep * K, k * k)
            assert torch.equal(c.reshape(B, keep * K, k * k), want)
