"""Shared prompts (hqt_set_prompt_groups, prompt_groups=, share_prompts=), the parts that need no GPU: the header and the binding, the deduplication
helper, the row layout of a guided pass and every refusal the Python surface raises before it reaches an engine."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.engine import Engine, check_prompt_groups
from hqtransformer_amd.pipeline import InflightSampler, sample_best_of
from hqtransformer_amd.sampling import guided_cond, prompt_groups_of, sampling_hqtransformer, sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16


def spec_of(**kw):
    base = dict(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=64, ctx_len_txt=T,
                n_classes=0, cond=2, embedding=0)
    base.update(kw)
    return Stage2Spec(**base)


def no_engine(*a, **k):
    raise AssertionError('the refusal must come before any engine is built')


def model_of(spec, engine=no_engine):
    return types.SimpleNamespace(spec=spec, use_txt_cond=spec.cond == 2, use_cls_cond=spec.cond == 1, engine=engine)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f'the library was reached ({name}) before the arguments were validated')


def engine_stub(spec, max_batch=8):
    """An Engine without a handle: whatever touches the library fails the test."""
    e = Engine.__new__(Engine)
    e.lib, e.h, e.s2, e.s1, e.device = _NoLibrary(), None, spec, None, torch.device('cuda:0')
    e.max_batch, e.max_steps, e.max_prefix, e.finalized = max_batch, spec.ctx_len_img, 0, True
    return e


def prompts(*rows):
    """Hand-made prompts: row i is T copies of rows[i]."""
    return torch.tensor([[r] * T for r in rows], dtype=torch.int64)


def test_the_header_declares_the_entry_point_and_it_is_bound():
    with open(os.path.join(ROOT, 'include', 'hqt.h')) as fp:
        header = fp.read()
    assert re.search(r'int hqt_set_prompt_groups\(hqt_handle\* h, int B, int n_groups, const int32_t\* group_of_row\);', header)
    assert 'a sampling call allocates nothing' in header
    assert 'hqt_set_prompt_groups' in _lib.SYMBOLS and len(_lib.SYMBOLS['hqt_set_prompt_groups'][1]) == 4
    assert _lib.ABI_VERSION == 9 and '#define HQT_ABI_VERSION 9' in header
    lib = _lib.load()
    assert 'hqt_set_prompt_groups' in _lib.exported_symbols() and lib.hqt_abi_version() == 9
    table = np.zeros(4, np.int32)
    assert lib.hqt_set_prompt_groups(None, 4, 1, table.ctypes.data_as(C.c_void_p)) == -1 and b'null handle' in lib.hqt_last_error()


def test_prompt_groups_of_numbers_groups_in_order_of_first_appearance():
    cond = prompts(7, 3, 3, 9, 7, 3)
    uniq, group = prompt_groups_of(cond)
    assert group.dtype == torch.int32 and group.tolist() == [0, 1, 1, 2, 0, 1]
    assert torch.equal(uniq, prompts(7, 3, 9))
    assert torch.equal(uniq[group.long()], cond)                         # the inverse reproduces cond
    # rows that differ in one token only are different prompts
    near = cond.clone()
    near[2, T - 1] = 4
    uniq, group = prompt_groups_of(near)
    assert group.tolist() == [0, 1, 2, 3, 0, 1] and torch.equal(uniq[group.long()], near)
    uniq, group = prompt_groups_of(prompts(5, 5, 5, 5))                  # all rows equal
    assert uniq.shape == (1, T) and group.tolist() == [0, 0, 0, 0]
    uniq, group = prompt_groups_of(prompts(4, 2, 8))                     # all rows distinct: the identity
    assert torch.equal(uniq, prompts(4, 2, 8)) and group.tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match='prompt_groups_of'):
        prompt_groups_of(torch.zeros(T, dtype=torch.int64))


def test_all_negative_rows_of_a_guided_pass_are_one_group():
    model = model_of(spec_of())
    cond = prompts(7, 3, 9)
    rows = guided_cond(model, 3, cond, None)                             # positives, then the all-[PAD] caption per image
    uniq, group = prompt_groups_of(rows)
    assert rows.shape == (6, T) and uniq.shape == (4, T)
    assert group.tolist() == [0, 1, 2, 3, 3, 3]
    # a caption that repeats among the positives shares its group too; one negative prompt given for all
    rows = guided_cond(model, 3, prompts(7, 3, 7), prompts(1))
    assert prompt_groups_of(rows)[1].tolist() == [0, 1, 0, 2, 2, 2]


def test_check_prompt_groups_refuses_by_name():
    spec = spec_of()
    cond = prompts(7, 3, 9)
    table, G = check_prompt_groups(spec, 5, cond, torch.tensor([2, 0, 0, 1, 2]), 8)
    assert G == 3 and table.dtype == np.int32 and table.flags['C_CONTIGUOUS'] and table.tolist() == [2, 0, 0, 1, 2]
    assert check_prompt_groups(spec, 5, cond, None, 8) is None
    with pytest.raises(ValueError, match='not text-conditional'):
        check_prompt_groups(spec_of(cond=1, n_classes=10), 2, torch.zeros(2, dtype=torch.int64), [0, 1], 8)
    with pytest.raises(ValueError, match=r'B=9 outside \[1, max_batch=8\]'):
        check_prompt_groups(spec, 9, cond, [0] * 9, 8)
    with pytest.raises(ValueError, match=r'n_groups=3 exceeds B=2'):
        check_prompt_groups(spec, 2, cond, [0, 1], 8)
    with pytest.raises(ValueError, match=r'index outside \[0, n_groups=3\)'):
        check_prompt_groups(spec, 4, cond, [0, 1, 3, 2], 8)
    with pytest.raises(ValueError, match=r'index outside \[0, n_groups=3\)'):
        check_prompt_groups(spec, 4, cond, [0, -1, 1, 2], 8)
    with pytest.raises(ValueError, match=r'expected shape \(4,\)'):
        check_prompt_groups(spec, 4, cond, [0, 1, 2], 8)
    with pytest.raises(ValueError, match='expected integers'):
        check_prompt_groups(spec, 3, cond, torch.tensor([0.0, 1.0, 2.0]), 8)
    with pytest.raises(ValueError, match=r'expected shape \(G, 16\)'):
        check_prompt_groups(spec, 3, cond[:, :8], [0, 1, 2], 8)
    with pytest.raises(ValueError, match='prefix or keep'):
        check_prompt_groups(spec, 3, cond, [0, 1, 2], 8, prefix=[torch.zeros((3, 2), dtype=torch.int64)])
    with pytest.raises(ValueError, match='prefix or keep'):
        check_prompt_groups(spec, 3, cond, [0, 1, 2], 8, keep=(torch.zeros((3, 64), dtype=torch.bool), []))


def test_engine_sample_validates_before_any_call_into_the_library():
    spec = spec_of()
    eng = engine_stub(spec)
    cond = prompts(7, 3, 9)
    with pytest.raises(ValueError, match=r'index outside \[0, n_groups=3\)'):
        eng.sample(4, cond, 8, prompt_groups=[0, 1, 2, 5])
    with pytest.raises(ValueError, match=r'n_groups=3 exceeds B=2'):
        eng.sample(2, cond, 8, prompt_groups=[0, 1])
    with pytest.raises(ValueError, match=r'B=9 outside'):
        eng.sample(9, cond, 8, prompt_groups=[0] * 9)
    with pytest.raises(ValueError, match='prefix or keep'):
        eng.sample(3, cond, 8, prompt_groups=[0, 1, 2], prefix=[torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2, 4), dtype=torch.int64)])
    l3 = engine_stub(spec_of(levels=3))
    with pytest.raises(ValueError, match=r'index outside \[0, n_groups=3\)'):
        l3.sample3(3, cond, 8, prompt_groups=[0, 1, 3])
    with pytest.raises(ValueError, match='not text-conditional'):
        engine_stub(spec_of(cond=1, n_classes=10)).sample(2, torch.zeros(2, dtype=torch.int64), 8, prompt_groups=[0, 1])


def test_share_prompts_with_a_prefix_or_a_keep_table_names_the_two():
    spec = spec_of()
    model = model_of(spec)
    cond = prompts(7, 7, 3)
    prefix = [torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2, 4), dtype=torch.int64)]
    with pytest.raises(ValueError, match='share_prompts together with prefix_codes or keep_mask'):
        sampling_ihqgpt(model, 1, cond, max_seq_len=8, prefix_codes=prefix, text_prefix=True, share_prompts=True)
    mask = torch.zeros((3, 8), dtype=torch.bool)
    kept = [torch.zeros((3, 8), dtype=torch.int64), torch.zeros((3, 8, 4), dtype=torch.int64)]
    with pytest.raises(ValueError, match='share_prompts together with prefix_codes or keep_mask'):
        sampling_ihqgpt(model, 1, cond, max_seq_len=8, keep_mask=mask, kept_codes=kept, share_prompts=True)
    with pytest.raises(ValueError, match='share_prompts together with prefix_codes or keep_mask'):       # also under guidance, whose rows are doubled first
        sampling_ihqgpt(model, 1, cond, max_seq_len=8, keep_mask=mask, kept_codes=kept, share_prompts=True, guidance_scale=2.0)
    with pytest.raises(ValueError, match='share_prompts together with prefix_codes or keep_mask'):
        sample_best_of(model, cond, 2, 1, share_prompts=True, max_seq_len=8,
                       prefix_codes=[p.repeat_interleave(2, dim=0) for p in prefix], text_prefix=True)
    l3 = model_of(spec_of(levels=3))
    with pytest.raises(ValueError, match='share_prompts together with prefix_codes or keep_mask'):
        sampling_hqtransformer(l3, 1, cond, max_seq_len=8, keep_mask=mask, kept_codes=kept + [torch.zeros((3, 8, 16), dtype=torch.int64)], share_prompts=True)
    with pytest.raises(ValueError, match='share_prompts needs a text-conditional model'):
        sampling_ihqgpt(model_of(spec_of(cond=1, n_classes=10)), 2, 3, max_seq_len=8, share_prompts=True)
    with pytest.raises(ValueError, match='share_prompts together with mixed_prefixes'):
        InflightSampler(types.SimpleNamespace(stage2=model), lanes=1, merge=2, mixed_prefixes=True, share_prompts=True)


def test_share_prompts_hands_the_engine_the_deduplicated_prompts():
    """The surface stages what prompt_groups_of returns -- for a guided call over the rows as the pass runs them -- and passes nothing new when it is off."""
    spec = spec_of()
    calls = []

    class Recorder:
        def sample(self, B, cond, n, **kw):
            calls.append((B, cond, kw))
            out = (torch.zeros((B, n), dtype=torch.int64), torch.zeros((B, n, 4), dtype=torch.int64))
            return out + ((torch.zeros((B, n, 5)),) if kw.get('return_logprobs') else ())

    model = model_of(spec, engine=lambda *a, **k: Recorder())
    cond = prompts(7, 3, 7)
    sampling_ihqgpt(model, 1, cond, max_seq_len=8, seed=1)
    assert 'prompt_groups' not in calls[-1][2] and torch.equal(calls[-1][1], cond)
    sampling_ihqgpt(model, 1, cond, max_seq_len=8, seed=1, share_prompts=True)
    B, c, kw = calls[-1]
    assert B == 3 and torch.equal(c, prompts(7, 3)) and kw['prompt_groups'].tolist() == [0, 1, 0]
    out = sampling_ihqgpt(model, 1, cond, max_seq_len=8, seed=1, share_prompts=True, guidance_scale=1.5)
    B, c, kw = calls[-1]
    assert B == 6 and c.shape == (3, T) and kw['prompt_groups'].tolist() == [0, 1, 0, 2, 2, 2] and len(kw['guidance']) == 3
    assert out[0].shape == (3, 8)                                        # the positive half comes back
    sample_best_of(model, prompts(7, 3), 4, 2, share_prompts=True, max_seq_len=8, seed=1)
    B, c, kw = calls[-1]
    assert B == 8 and torch.equal(c, prompts(7, 3)) and kw['prompt_groups'].tolist() == [0] * 4 + [1] * 4
