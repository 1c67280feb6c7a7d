"""Kept positions (hqt_set_keep_mask), the parts that need no GPU: the recorded oracle case, the rule for the leading run L, the window plan of
``sample_canvas``, the keep table of a pass with mixed prefixes, the refusals of the Python surface -- each before any engine is built -- and the ABI
addition.  The GPU side: tests/test_gpu_keep.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import check_keep, keep_leading_run
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.pipeline import (Pending, _Step, box_keep_mask, canvas_keep_masks, canvas_windows, check_mergeable, step_keep_table)
from hqtransformer_amd.sampling import sampling_hqtransformer, sampling_ihqgpt
from hqtransformer_amd.spec import stage2_spec_from_config
from oracle import hqt_oracle as O
from tests import keep_ref as K
from tests.helpers import load, stage2_from_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg(name):
    return load_config(os.path.join(ROOT, 'configs', name))


# ------------------------------------------------------------------------------- the reference by iteration
@pytest.mark.parametrize('runs', [K.KEEP_RUNS, K.KEEP_RUNS_L2])
def test_the_recorded_case_is_well_conditioned_and_keeps_what_it_is_given(runs):
    """g4_tiny_cls, B = 5, n = 12, TINY_SET, exp_noise(700): margin 1.0049 over ALL draws with either set of leading runs (recorded, 1e-6 relative)."""
    spec, weights = stage2_from_fixture(load('g4_tiny_cls.npz'))
    cond, mask, kept, noise = K.tiny_keep_case(spec, runs)
    ct, cb, logits, margin = K.oracle_keep(O.OracleStage2(spec, weights), cond, 5, 12, noise, mask, kept, *K.TINY_SET)
    print(f'runs {runs}: oracle margin {margin!r}')
    recorded = 1.0049023628234863
    assert margin >= 1.00009 and abs(margin - recorded) <= 1e-6 * recorded
    assert (ct[mask] == kept[0][mask]).all() and (cb[mask] == kept[1][mask]).all()
    assert np.isfinite(logits).all() and mask.sum() == {K.KEEP_RUNS: 31, K.KEEP_RUNS_L2: 33}[runs]
    # a position that is not kept is a free draw: forcing the whole result through the plain oracle redraws it
    t, b = O.OracleStage2(spec, weights).sample(cond, 5, 12, noise, *K.TINY_SET, force_top=ct.copy(), force_bot=cb.copy())
    assert (t[~mask] == ct[~mask]).all() and (b[~mask] == cb[~mask]).all()


# ------------------------------------------------------------------------------- L
def test_the_leading_run_is_the_shortest_one_clipped():
    mask = K.scattered_mask(5, 12, K.KEEP_RUNS_L2, K.KEEP_EXTRA)       # row 0: positions 0, 1 and its extra cell 2 -> a run of 3
    assert [keep_leading_run(mask, m) for m in (0, 1, 2, 3, 11, 63)] == [0, 1, 2, 3, 3, 3]
    assert [K.leading_run(mask, m) for m in (0, 1, 2, 3, 11, 63)] == [0, 1, 2, 3, 3, 3]
    assert keep_leading_run(K.scattered_mask(5, 12, K.KEEP_RUNS, K.KEEP_EXTRA), 63) == 0             # one row leads with nothing
    full = np.ones((3, 12), bool)
    assert keep_leading_run(full, 63) == 11 and keep_leading_run(full, 4) == 4                      # n_steps - 1: the last position is a decode step
    assert keep_leading_run(np.ones((2, 1), bool), 63) == 0
    assert keep_leading_run(full, 63, text_l3=True) == 0                                            # no prefix prefill there
    assert keep_leading_run(torch.from_numpy(full), 63) == 11
    with pytest.raises(ValueError, match='keep mask'):
        keep_leading_run(np.ones((12,), bool), 3)


# ------------------------------------------------------------------------------- the Python surface refuses before an engine is built
def test_check_keep_shapes_dtypes_and_the_vocabulary():
    spec = stage2_spec_from_config(cfg('tiny-cls.yaml'))
    B, n, V = 3, 8, spec.vocab_top
    mask = np.zeros((B, n), bool)
    mask[1, 2] = True
    codes = [torch.zeros((B, n), dtype=torch.int64), torch.zeros((B, n, 4), dtype=torch.int64)]
    m, levels = check_keep(spec, B, n, (mask, codes))
    assert m.dtype == np.uint8 and m.flags['C_CONTIGUOUS'] and m.sum() == 1 and len(levels) == 2
    assert check_keep(spec, B, n, None) is None
    codes[0][0, 0] = V + 7                           # outside the vocabulary where nothing is kept: never read
    check_keep(spec, B, n, (mask, codes))
    codes[1][1, 2, 3] = V
    with pytest.raises(IndexError, match=r'kept codes\[1\]'):
        check_keep(spec, B, n, (mask, codes))
    codes[1][1, 2, 3] = 0
    for bad, word in (((mask[:, :4], codes), 'keep mask'), ((mask.astype(np.float32), codes), 'keep mask'), ((mask, codes[:1]), 'code levels'),
                      ((mask, [codes[0], codes[1][:, :, :2]]), r'kept codes\[1\]'), ((mask, [codes[0], codes[1].float()]), 'integer codes'), (mask, 'expected')):
        with pytest.raises(ValueError, match=word):
            check_keep(spec, B, n, bad)


def test_the_samplers_refuse_a_bad_table_before_any_engine_is_built():
    model = ImageGPT2(cfg('tiny-cls.yaml'), seed=1)          # on the CPU: anything that reaches an engine raises HqtLibraryError
    spec = model.stage2.spec
    B, n = 2, 16
    mask = torch.zeros((B, n), dtype=torch.bool)
    mask[:, :3] = True
    codes = [torch.zeros((B, n), dtype=torch.int64), torch.zeros((B, n, 4), dtype=torch.int64)]
    kw = dict(max_seq_len=n, seed=1)
    with pytest.raises(ValueError, match='come together'):
        sampling_ihqgpt(model.stage2, B, 3, keep_mask=mask, **kw)
    with pytest.raises(ValueError, match='leading run'):
        sampling_ihqgpt(model.stage2, B, 3, keep_mask=mask, kept_codes=codes, prefix_codes=[c[:, :3] for c in codes], **kw)
    with pytest.raises(ValueError, match='given_top_code'):
        sampling_ihqgpt(model.stage2, B, 3, keep_mask=mask, kept_codes=codes, given_top_code=codes[0], **kw)
    codes[0][1, 1] = spec.vocab_top
    with pytest.raises(IndexError):
        sampling_ihqgpt(model.stage2, B, 3, keep_mask=mask, kept_codes=codes, **kw)
    codes[0][1, 1] = 0
    with pytest.raises(_lib.HqtLibraryError):                # a good table goes on to the engine
        sampling_ihqgpt(model.stage2, B, 3, keep_mask=mask, kept_codes=codes, **kw)
    l3 = ImageGPT2(cfg('tiny-l3.yaml'), seed=1)
    with pytest.raises(ValueError, match='code levels'):
        sampling_hqtransformer(l3.stage2, B, 3, keep_mask=mask, kept_codes=codes, **kw)


# ------------------------------------------------------------------------------- canvases and boxes
@pytest.mark.parametrize('G,w,s', [(16, 8, 4), (16, 8, 2), (12, 8, 1), (8, 8, 3), (20, 8, 6), (11, 4, 7)])
def test_canvas_windows_draw_every_cell_exactly_once(G, w, s):
    if (G - w) % s or not 1 <= s < w:
        with pytest.raises(ValueError, match='canvas_windows'):
            canvas_windows(G, w, s)
        return
    wins = canvas_windows(G, w, s)
    steps = list(range(0, G - w + 1, s))
    assert wins == [(oy, ox) for oy in steps for ox in steps] and len(wins) == len(steps) ** 2
    drawn = np.zeros((G, G), int)
    plan = canvas_keep_masks(G, w, s)
    assert [(oy, ox) for oy, ox, _ in plan] == wins
    for oy, ox, keep in plan:
        keep = keep.numpy()
        want = np.zeros((w, w), bool)                # rows < w - s when a window above was drawn, columns < w - s when one to the left was
        if oy > 0:
            want[:w - s] = True
        if ox > 0:
            want[:, :w - s] = True
        assert (keep == want).all(), (oy, ox)
        drawn[oy:oy + w, ox:ox + w] += ~keep
    assert (drawn == 1).all()                        # every canvas cell is owned by exactly one window


def test_canvas_windows_refuses_what_does_not_tile():
    assert len(canvas_windows(16, 8, 4)) == 9
    for bad in ((16, 8, 8), (16, 8, 0), (16, 8, 3), (6, 8, 1), (16, 8, 9)):
        with pytest.raises(ValueError, match='canvas_windows'):
            canvas_windows(*bad)


def test_box_keep_mask_keeps_everything_outside_the_box():
    m = box_keep_mask(8, (2, 5, 1, 4)).reshape(8, 8)
    assert int((~m).sum()) == 9 and not bool(m[2:5, 1:4].any()) and bool(m[:2].all()) and bool(m[:, 4:].all())
    assert not bool(box_keep_mask(8, (0, 8, 0, 8)).any())
    for bad in ((2, 2, 1, 4), (-1, 3, 0, 2), (0, 9, 0, 2), (0, 2, 5, 4)):
        with pytest.raises(ValueError, match='box='):
            box_keep_mask(8, bad)


# ------------------------------------------------------------------------------- merged passes
def _step(n, prefix=None, **kw):
    if prefix is not None:
        kw['prefix_codes'] = prefix
    return _Step(Pending(), n, 3, 1, 16, True, None, True, True, None, True, kw)


def _prefix(B, P, fill, levels=2):
    return [torch.full((B, P) + ((4 ** l,) if l else ()), fill + l, dtype=torch.int64) for l in range(levels)]


def test_the_default_rule_still_refuses_and_mixed_prefixes_merges():
    a, b, c = _step(2, _prefix(2, 4, 1)), _step(3, _prefix(3, 5, 2)), _step(2)
    for x, y in ((b, a), (c, a), (a, c)):
        with pytest.raises(ValueError, match=r'steps merged into one pass must share the prefix length: this step has P=\d, the pass P=\d '
                                             r'\(a merged pass has one prefill; flush\(\) first to start a new pass\)'):
            check_mergeable(x, y)
        check_mergeable(x, y, mixed_prefixes=True)
    with pytest.raises(ValueError, match='must share max_seq_len'):        # everything else is still shared
        check_mergeable(_step(2, _prefix(2, 4, 1), top_k_top=5), c, mixed_prefixes=True)
    check_mergeable(_step(2, _prefix(2, 4, 1), top_k_top=5), c, mixed_samplers=True, mixed_prefixes=True)


@pytest.mark.parametrize('levels', [2, 3])
def test_the_merged_keep_table_holds_every_steps_own_prefix(levels):
    sizes, Ps, n = (2, 3, 1), (0, 5, 9), 16
    kws = [dict() if P == 0 else dict(prefix_codes=_prefix(b, P, 10 * (i + 1), levels), top_k_top=5) for i, (b, P) in enumerate(zip(sizes, Ps))]
    mask, codes = step_keep_table(levels, sizes, n, kws)
    assert mask.shape == (6, n) and mask.dtype == torch.bool and [tuple(c.shape) for c in codes] == [(6, n), (6, n, 4), (6, n, 16)][:levels]
    assert mask.sum(1).tolist() == [0, 0, 5, 5, 5, 9]
    assert all(bool(mask[r, :p].all()) and not bool(mask[r, p:].any()) for r, p in enumerate([0, 0, 5, 5, 5, 9]))
    for l, c in enumerate(codes):
        assert bool((c[2:5, :5] == 20 + l).all()) and bool((c[5:, :9] == 30 + l).all()) and bool((c[~mask] == 0).all())
    assert keep_leading_run(mask, 15) == 0           # the pass's L is the shortest prefix
    m2, _ = step_keep_table(levels, sizes[1:], n, kws[1:])
    assert keep_leading_run(m2, 15) == 5 and keep_leading_run(m2, 3) == 3
    with pytest.raises(ValueError, match='prefix_codes'):
        step_keep_table(levels, (2,), n, [dict(prefix_codes=_prefix(2, n, 1, levels))])


# ------------------------------------------------------------------------------- ABI
def test_the_entry_point_is_exported_and_refuses_a_null_handle():
    lib = _lib.load()
    assert 'hqt_set_keep_mask' in _lib.exported_symbols() and lib.hqt_abi_version() == 9
    mask = np.ones((1, 4), np.uint8)
    assert lib.hqt_set_keep_mask(None, 1, 4, mask.ctypes.data_as(C.c_void_p), None) == -1
    assert b'null handle' in lib.hqt_last_error()
