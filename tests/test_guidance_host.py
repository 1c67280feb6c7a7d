"""Host side of guided sampling (hqt_set_guidance, guidance_scale=): the reference arithmetic, the doubled batch and the pair tables the Python
layer builds, and what it refuses.  No library call, no GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import check_guided_rows, guide_pair_table
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.pipeline import _Step, Pending, check_guided_step, check_mergeable, step_guidance
from hqtransformer_amd.sampling import (_twice, _twice_rows, guidance_scales, guided_cond, guided_pairs, negative_cond, sampling_hqtransformer,
                                        sampling_ihqgpt)
from hqtransformer_amd.text import PAD_ID, pad_caption
from tests.guidance_ref import level_of_draw, mix, safe_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(seed, shape=(3, 516)):
    r = np.random.default_rng(seed)
    return (3.0 * r.standard_normal(shape)).astype(np.float32), (3.0 * r.standard_normal(shape)).astype(np.float32)


# ------------------------------------------------------------------------------------ the reference arithmetic
def test_mix_scale_one_is_the_positive_row_bit_for_bit():
    lp, ln = rows(1)
    assert mix(lp, ln, 1.0).dtype == np.float32
    assert (mix(lp, ln, 1.0).view(np.uint32) == lp.view(np.uint32)).all()


def test_mix_scale_zero_and_the_three_roundings():
    lp, ln = rows(2)
    d = (lp - ln).astype(np.float32)
    assert (mix(lp, ln, 0.0).view(np.uint32) == (lp - d).astype(np.float32).view(np.uint32)).all()
    # every operation is rounded on its own: the float64 expression rounded once differs somewhere, the float32 chain never
    s = 2.5
    chain = (lp + (np.float32(s - 1.0) * d).astype(np.float32)).astype(np.float32)
    assert (mix(lp, ln, s).view(np.uint32) == chain.view(np.uint32)).all()
    once = (lp.astype(np.float64) + (s - 1.0) * (lp.astype(np.float64) - ln.astype(np.float64))).astype(np.float32)
    assert (mix(lp, ln, s) != once).any(), 'the case cannot tell three roundings from one'
    assert np.abs(mix(lp, ln, s) - once).max() <= 4 * np.spacing(np.abs(once).max())


def test_levels_of_draws_and_the_safe_ratio():
    assert [level_of_draw(d) for d in (0, 1, 4, 5, 20)] == [0, 1, 1, 2, 2]
    assert safe_ratio((1.0, 1.0), 2e-4, (1.0, 1.0)) == pytest.approx(np.exp(4e-4))
    assert safe_ratio((1.5, 2.0), 2e-4, (1.0, 0.5)) == pytest.approx(np.exp(2 * 3.0 * 2e-4 / 0.5))
    assert safe_ratio((0.0, -1.0), 2e-4, (1.0, 1.0)) == pytest.approx(np.exp(2 * 3.0 * 2e-4))


# ------------------------------------------------------------------------------------ the ABI
def test_pair_struct_is_20_bytes_on_both_sides():
    assert C.sizeof(_lib.hqt_guide_pair) == 20
    hdr = open(os.path.join(ROOT, 'include', 'hqt.h')).read()
    m = re.search(r'typedef struct \{ int32_t pos_row, neg_row; float scale\[3\]; \} hqt_guide_pair;\s*/\* 20 bytes \*/', hdr)
    assert m, 'include/hqt.h does not declare hqt_guide_pair as the ctypes mirror lays it out'
    assert re.search(r'int hqt_set_guidance\(hqt_handle\* h, int n_pairs, const hqt_guide_pair\* pairs\);', hdr)
    eng = open(os.path.join(ROOT, 'hqtransformer_amd', 'csrc', 'engine.hip')).read()
    assert 'sizeof(hqt_guide_pair) == 20 && sizeof(GuidePair) == sizeof(hqt_guide_pair)' in eng
    assert [f[0] for f in _lib.hqt_guide_pair._fields_] == ['pos_row', 'neg_row', 'scale']
    assert _lib.hqt_guide_pair.pos_row.offset == 0 and _lib.hqt_guide_pair.neg_row.offset == 4 and _lib.hqt_guide_pair.scale.offset == 8
    assert _lib.SYMBOLS['hqt_set_guidance'][1][1:] == [C.c_int, C.POINTER(_lib.hqt_guide_pair)]


def test_pair_table():
    t = guide_pair_table(2, [(0, 3, (1.0, 2.5)), (4, 1, 2.0)])
    assert len(t) == 2 and C.sizeof(t) == 40
    assert (t[0].pos_row, t[0].neg_row, list(t[0].scale)) == (0, 3, [1.0, 2.5, 1.0])           # a level the model lacks: no guidance
    assert (t[1].pos_row, t[1].neg_row, list(t[1].scale)) == (4, 1, [2.0, 2.0, 1.0])
    assert list(guide_pair_table(3, [(1, 0, (0.5, 1.5, -1.0))])[0].scale) == [0.5, 1.5, -1.0]
    with pytest.raises(ValueError, match='one scale or 2'):
        guide_pair_table(2, [(0, 1, (1.0, 2.0, 3.0))])
    with pytest.raises(ValueError, match=r'\(pos_row, neg_row, scale\)'):
        guide_pair_table(2, [(0, 1)])


# ------------------------------------------------------------------------------------ the doubled batch
def test_scales_and_pairs():
    assert guidance_scales(2, None) is None
    assert guidance_scales(2, 3) == (3.0, 3.0) and guidance_scales(3, [1, 2.5, 0]) == (1.0, 2.5, 0.0)
    with pytest.raises(ValueError, match='one per code level'):
        guidance_scales(3, [1.0, 2.0])
    assert guided_pairs(3, (1.5, 2.0)) == [(0, 3, (1.5, 2.0)), (1, 4, (1.5, 2.0)), (2, 5, (1.5, 2.0))]
    assert guided_pairs(2, (2.0,) * 3, lo=4) == [(4, 6, (2.0,) * 3), (5, 7, (2.0,) * 3)]


def test_per_row_inputs_are_repeated_for_the_negative_half():
    noise = torch.arange(2 * 5 * 3 * 4, dtype=torch.float32).reshape(2, 5, 3, 4)
    n2 = _twice(noise, 2)
    assert tuple(n2.shape) == (2, 5, 6, 4) and torch.equal(n2[:, :, :3], noise) and torch.equal(n2[:, :, 3:], noise)
    p = torch.arange(6).reshape(3, 2)
    assert torch.equal(_twice(p), torch.cat([p, p])) and _twice(None) is None
    assert _twice_rows([7, 8]) == [7, 8, 7, 8] and _twice_rows(None) is None


def fake(cond, levels=2, n_classes=10, ctx=4):
    return SimpleNamespace(use_txt_cond=cond == 2, use_cls_cond=cond == 1, spec=SimpleNamespace(levels=levels, n_classes=n_classes, ctx_len_txt=ctx))


def test_conditions_of_the_doubled_batch():
    cls = guided_cond(fake(1), 3, torch.tensor([1, 2, 3]), 9)
    assert cls.tolist() == [1, 2, 3, 9, 9, 9]
    assert guided_cond(fake(1), 3, torch.tensor([1, 2, 3]), [4, 5, 6]).tolist() == [1, 2, 3, 4, 5, 6]
    txt = torch.arange(1, 9).reshape(2, 4)
    got = guided_cond(fake(2), 2, txt, None)                   # text: the all-[PAD] caption by default
    assert got.dtype == torch.int64 and torch.equal(got[:2], txt) and torch.equal(got[2:], torch.full((2, 4), PAD_ID))
    assert torch.equal(pad_caption(2, 4), torch.full((2, 4), PAD_ID, dtype=torch.int64)) and pad_caption(1, 3, 7).tolist() == [[7, 7, 7]]
    one = guided_cond(fake(2), 2, txt, torch.tensor([5, 6, 7, 8]))      # one negative prompt for all
    assert torch.equal(one[2:], torch.tensor([[5, 6, 7, 8]] * 2))


def test_what_is_refused():
    with pytest.raises(ValueError, match='needs neg_cond'):
        guided_cond(fake(1), 2, torch.tensor([1, 2]), None)
    with pytest.raises(ValueError, match='conditional model'):
        guided_cond(fake(0), 2, None, None)
    with pytest.raises(ValueError, match='one condition or 3'):
        guided_cond(fake(1), 3, torch.tensor([1, 2, 3]), [4, 5])
    with pytest.raises(IndexError):
        guided_cond(fake(1), 2, torch.tensor([1, 2]), 10)


@pytest.fixture(scope='module')
def tiny_models():
    return {name: ImageGPT2(load_config(os.path.join(ROOT, 'configs', f'{name}.yaml')), seed=5).eval() for name in ('tiny-cls', 'tiny-l3')}


def test_samplers_refuse_before_an_engine_is_built(tiny_models):
    """The models are on the CPU: whatever got past these checks would fail for want of a GPU, with another error."""
    st2 = tiny_models['tiny-cls'].stage2
    with pytest.raises(ValueError, match='needs neg_cond'):
        sampling_ihqgpt(st2, 2, 3, guidance_scale=2.0, max_seq_len=4)
    with pytest.raises(ValueError, match='one per code level'):
        sampling_ihqgpt(st2, 2, 3, guidance_scale=[1.0, 2.0, 3.0], neg_cond=4, max_seq_len=4)
    with pytest.raises(ValueError, match='neg_cond comes with guidance_scale'):
        sampling_ihqgpt(st2, 2, 3, neg_cond=4, max_seq_len=4)
    with pytest.raises(ValueError, match='not both'):
        sampling_ihqgpt(st2, 2, 3, guidance_scale=2.0, neg_cond=4, guidance=[(0, 1, 2.0)], max_seq_len=4)
    st3 = tiny_models['tiny-l3'].stage2
    with pytest.raises(ValueError, match='needs neg_cond' if st3.use_cls_cond else 'conditional model'):
        sampling_hqtransformer(st3, 2, 3, guidance_scale=2.0, max_seq_len=4)
    # an unconditional model has no second condition
    uncond = SimpleNamespace(use_txt_cond=False, use_cls_cond=False, spec=st2.spec)
    with pytest.raises(ValueError, match='conditional model'):
        sampling_ihqgpt(uncond, 2, None, guidance_scale=2.0, max_seq_len=4)


def test_engine_names_the_doubling_when_the_rows_do_not_fit():
    check_guided_rows(4, 2, 4)
    with pytest.raises(ValueError, match=r'two rows of one pass.*batch=4 rows for 2 pairs exceed max_batch=2'):
        check_guided_rows(4, 2, 2)


def test_a_bad_guided_step_is_refused_when_it_is_submitted():
    """``InflightSampler.submit`` runs this before it queues the step: the queue and every Pending handed out stay as they were."""
    check_guided_step(fake(1), 3, dict(top_k_top=5))
    check_guided_step(fake(1), 3, dict(guidance_scale=2.0, neg_cond=[1, 2, 3]))
    check_guided_step(fake(2), 2, dict(guidance_scale=[1.0, 2.0]))
    assert negative_cond(fake(1), 2, 7).tolist() == [7, 7]
    for model, n, kw, message in ((fake(1), 3, dict(guidance_scale=2.0), 'needs neg_cond'), (fake(1), 3, dict(guidance_scale=2.0, neg_cond=[1, 2]), 'one condition or 3'),
                                  (fake(1), 3, dict(guidance_scale=[1.0, 2.0, 3.0], neg_cond=1), 'one per code level'), (fake(0), 3, dict(guidance_scale=2.0), 'conditional model'),
                                  (fake(1), 3, dict(neg_cond=4), 'neg_cond comes with guidance_scale')):
        with pytest.raises(ValueError, match=message):
            check_guided_step(model, n, kw)


# ------------------------------------------------------------------------------------ merged passes
def test_pair_tables_of_merged_steps():
    # three steps of 2, 3 and 1 rows; the first and the last guided: their negative rows follow the 6 rows of all steps
    pairs, mirrors = step_guidance(2, [2, 3, 1], [dict(guidance_scale=2.0, neg_cond=5), dict(top_k_top=5), dict(guidance_scale=[1.5, 0.5])])
    assert pairs == [(0, 6, (2.0, 2.0)), (1, 7, (2.0, 2.0)), (5, 8, (1.5, 0.5))]
    assert mirrors == [0, 1, 5]
    assert step_guidance(3, [4, 4], [{}, {}]) == ([], [])
    pairs, mirrors = step_guidance(3, [1, 2], [{}, dict(guidance_scale=(1.0, 2.0, 3.0))])
    assert pairs == [(1, 3, (1.0, 2.0, 3.0)), (2, 4, (1.0, 2.0, 3.0))] and mirrors == [1, 2]
    with pytest.raises(ValueError, match='neg_cond comes with guidance_scale'):
        step_guidance(2, [1], [dict(neg_cond=3)])
    # every row of the table is named once, inside the pass
    named = [r for p in pairs for r in p[:2]]
    assert len(set(named)) == len(named) and max(named) < 3 + len(mirrors)


def test_guided_and_unguided_steps_merge():
    def step(**kw):
        return _Step(Pending(), 4, 7, 1, 8, False, None, True, True, None, True, kw)
    check_mergeable(step(guidance_scale=2.0, neg_cond=3), step())
    check_mergeable(step(guidance_scale=2.0, neg_cond=3), step(guidance_scale=[1.0, 3.0], neg_cond=5))
    with pytest.raises(ValueError, match='must share'):
        check_mergeable(step(guidance_scale=2.0, neg_cond=3, top_k_top=5), step())
