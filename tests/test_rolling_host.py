"""Rolling passes (hqt_set_row_positions): what can be checked without a GPU -- the slot bookkeeping of pipeline.RollingSampler against a fake engine that
records its calls, the argument checks that raise before any engine call, and the new symbol in the built library with the argument errors that need no device."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.engine import Engine, check_row_positions
from hqtransformer_amd.pipeline import RollingSampler
from hqtransformer_amd.spec import Stage2Spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spec_of(**kw):
    base = dict(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=64, ctx_len_txt=16,
                n_classes=10, cond=1, embedding=0)
    base.update(kw)
    return Stage2Spec(**base)


class FakeEngine:
    """Engine.sample as far as a rolling sampler can tell: the call is recorded, and every position a row draws holds, on every level, the code
    (seed + offset + position) % 512 of the key its slot carried in that call -- so a result names the request that drew it.  It also keeps the record the
    library keeps, and refuses a slot that neither joins, stays empty nor continues where it stands."""
    device, max_batch = torch.device('cpu'), 16

    def __init__(self):
        self.calls, self.next = [], None

    def sample(self, B, cond, n, *, out, logprobs_out, row_seeds, row_offsets, row_samplers, row_positions, **kw):
        pos, k = row_positions
        assert len(pos) == len(row_seeds) == len(row_offsets) == len(row_samplers) == B == out[0].shape[0] and (cond is None or len(cond) == B)
        want = self.next or [-1] * B
        for b, p in enumerate(pos):
            assert p in (-1, 0, want[b]), f'slot {b} at position {p}: the pass has it at {want[b]}'
        self.calls.append(dict(pos=list(pos), k=k, cond=None if cond is None else cond.tolist(), seeds=list(row_seeds), offsets=list(row_offsets),
                               samplers=list(row_samplers), kw=kw))
        for b, p in enumerate(pos):
            for t in range(p, min(p + k, n)) if p >= 0 else ():
                for o in out:
                    o[b, t] = (row_seeds[b] + row_offsets[b] + t) % 512
                if logprobs_out is not None:
                    logprobs_out[b, t] = -float(row_seeds[b] % 10) - 0.01 * t
        self.next = [-1 if p < 0 or p + k >= n else p + k for p in pos]


def stage2_stub(spec, eng=None):
    return types.SimpleNamespace(spec=spec, use_cls_cond=spec.cond == 1, use_txt_cond=spec.cond == 2, engine=lambda *a, **k: eng)


def codes_of(seed, offset, n):
    return [(seed + offset + t) % 512 for t in range(n)]


def test_admission_order_slot_reuse_and_the_positions_of_every_call():
    eng = FakeEngine()
    rs = RollingSampler(stage2_stub(spec_of(), eng), 3, 4, precision='exact', return_logprobs=True)
    tickets = [rs.submit(cls, seed=100 + 7 * cls, sample_offset=cls, top_k_top=10 + cls) for cls in (1, 2)]
    assert tickets == [0, 1] and rs.live == 0 and rs.step() == []            # position 0 of both: nothing finishes
    assert eng.calls[0]['pos'] == [0, 0, -1] and eng.calls[0]['cond'] == [1, 2, 0] and eng.calls[0]['k'] == 1
    assert eng.calls[0]['seeds'][:2] == [107, 114] and eng.calls[0]['offsets'][:2] == [1, 2]
    assert [s[1][0] for s in eng.calls[0]['samplers'][:2]] == [11, 12]       # each slot carries its request's sampler settings
    assert eng.calls[0]['kw']['precision'] == _lib.PRECISION_EXACT and eng.calls[0]['kw']['seed'] == 0
    assert rs.step() == []
    for cls in (3, 4, 5):                                                     # three more than there are free slots: one joins now, two wait
        tickets.append(rs.submit(cls, seed=100 + 7 * cls, sample_offset=cls))
    assert rs.step() == [] and eng.calls[2]['pos'] == [2, 2, 0] and eng.calls[2]['cond'] == [1, 2, 3]
    done = rs.step()                                                          # the first two draw position 3 = n - 1
    assert eng.calls[3]['pos'] == [3, 3, 1] and [d[0] for d in done] == [0, 1]
    for (ticket, codes, lp), cls in zip(done, (1, 2)):
        assert [tuple(c.shape) for c in codes] == [(4,), (4, 4)] and tuple(lp.shape) == (4, 5)
        assert codes[0].tolist() == codes_of(100 + 7 * cls, cls, 4) and bool((codes[1] == codes[0][:, None]).all())
        assert bool(torch.isfinite(lp).all())
    assert rs.pos == [-1, -1, 2] and rs.free == [0, 1]
    done = rs.step()                                                          # the freed slots are reused in submission order, lowest slot first
    assert eng.calls[4]['pos'] == [0, 0, 2] and eng.calls[4]['cond'] == [4, 5, 3] and done == []
    done = rs.drain()
    assert [d[0] for d in done] == [2, 3, 4] and not rs.queue and rs.live == 0
    assert [c['pos'] for c in eng.calls[5:]] == [[1, 1, 3], [2, 2, -1], [3, 3, -1]]
    for (ticket, codes, lp), cls in zip(done, (3, 4, 5)):
        assert codes[0].tolist() == codes_of(100 + 7 * cls, cls, 4)
    n_calls = len(eng.calls)
    assert rs.step() == [] and rs.drain() == [] and len(eng.calls) == n_calls   # nothing queued or live: no engine call


def test_a_request_that_finishes_mid_call_frees_its_slot_for_the_next_call():
    eng = FakeEngine()
    rs = RollingSampler(stage2_stub(spec_of(), eng), 2, 5)
    a = rs.submit(1, seed=11)
    assert rs.step(2) == [] and rs.step(2) == [] and rs.pos == [4, -1]        # one position left
    b = rs.submit(2, seed=22)
    done = rs.step(2)                                                         # k = 2: a draws position 4 in the first step and idles in the second
    assert eng.calls[-1]['pos'] == [4, 0] and eng.calls[-1]['k'] == 2
    assert [d[0] for d in done] == [a] and len(done[0]) == 2 and done[0][1][0].tolist() == codes_of(11, 0, 5)
    assert rs.pos == [-1, 2] and rs.free == [0]
    c = rs.submit(3, seed=33)
    done = rs.drain(2)
    assert [d[0] for d in done] == [b, c]
    assert [cl['pos'] for cl in eng.calls[3:]] == [[0, 2], [2, 4], [4, -1]]
    assert done[1][1][0].tolist() == codes_of(33, 0, 5)
    with pytest.raises(ValueError, match='1 <= k <= n = 5'):
        rs.step(6)


def test_drain_terminates_with_more_requests_than_slots_and_any_k():
    for k in (1, 2, 3, 7):
        eng = FakeEngine()
        rs = RollingSampler(stage2_stub(spec_of(cond=0), eng), 2, 7)
        tickets = [rs.submit(None, seed=5 * i) for i in range(5)]
        done = rs.drain(k)
        assert sorted(d[0] for d in done) == tickets and len(eng.calls) <= 5 * 7
        for ticket, codes in done:
            assert codes[0].tolist() == codes_of(5 * ticket, 0, 7)
        assert all(c['cond'] is None for c in eng.calls)


def test_text_models_and_bad_requests_are_refused_before_an_engine_is_asked_for():
    def no_engine(*a, **k):
        raise AssertionError('an engine was built before the arguments were validated')
    st = stage2_stub(spec_of(cond=2))
    st.engine = no_engine
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill'):
        RollingSampler(st, 3, 8)
    st = stage2_stub(spec_of())
    st.engine = no_engine
    with pytest.raises(ValueError, match='at least one slot'):
        RollingSampler(st, 0, 8)
    with pytest.raises(ValueError, match='ctx_len_img=64'):
        RollingSampler(st, 2, 65)
    rs = RollingSampler(stage2_stub(spec_of(), FakeEngine()), 2, 8)
    with pytest.raises(ValueError, match=r'class id in \[0, 10\)'):
        rs.submit(10, seed=1)
    with pytest.raises(ValueError, match='class id'):
        rs.submit(None, seed=1)
    with pytest.raises(TypeError, match='guidance_scale'):
        rs.submit(1, seed=1, guidance_scale=2.0)
    with pytest.raises(ValueError, match='takes None'):
        RollingSampler(stage2_stub(spec_of(cond=0), FakeEngine()), 2, 8).submit(3, seed=1)


def test_row_positions_are_checked_on_the_host():
    assert check_row_positions(1, 3, 8, None) is None
    pos, k = check_row_positions(1, 3, 8, ([4, -1, 0], 2))
    assert pos.dtype == np.int32 and pos.tolist() == [4, -1, 0] and pos.flags['C_CONTIGUOUS'] and k == 2
    assert check_row_positions(0, 2, 8, (torch.tensor([7, 0]), 8))[0].tolist() == [7, 0]
    with pytest.raises(ValueError, match='text-conditional'):
        check_row_positions(2, 3, 8, ([0, 0, 0], 1))
    for bad, match in ((([0, 0], 1), 'one integer per row'), (([0.0, 1.0, 2.0], 1), 'one integer per row'), (([0, 8, 0], 1), r'pos\[1\]=8 outside \[-1, n_steps - 1 = 7\]'),
                       (([0, -2, 0], 1), r'pos\[1\]=-2'), (([0, 0, 0], 0), r'k=0 outside \[1, n_steps = 8\]'), (([0, 0, 0], 9), 'k=9'), (([0, 0, 0], True), 'k=True'),
                       ([0, 0, 0], r'expected \(pos, k\)')):
        with pytest.raises(ValueError, match=match):
            check_row_positions(1, 3, 8, bad)
    for what in ('prefix', 'keep', 'prompt_groups', 'segment'):
        with pytest.raises(ValueError, match=f'row_positions together with {what}'):
            check_row_positions(1, 3, 8, ([0, 0, 0], 1), **{what: object()})
    # Engine.sample raises before it touches the library: this "engine" has none
    eng = Engine.__new__(Engine)
    eng.s2, eng.device, eng.max_batch, eng.max_prefix = spec_of(), torch.device('cpu'), 4, 0
    with pytest.raises(ValueError, match='pass the tensors the pass lives in'):
        eng.sample(2, torch.zeros(2, dtype=torch.int64), 8, row_positions=([0, 0], 1))
    with pytest.raises(ValueError, match=r'pos\[0\]=9'):
        eng.sample(2, torch.zeros(2, dtype=torch.int64), 8, row_positions=([9, 0], 1))


def test_the_built_library_exports_the_entry_point_and_checks_its_arguments_without_a_device():
    assert _lib.SYMBOLS['hqt_set_row_positions'] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int])
    with open(os.path.join(ROOT, 'include', 'hqt.h')) as fp:
        header = fp.read()
    assert 'int hqt_set_row_positions(hqt_handle* h, int B, const int32_t* pos, int k);' in header
    assert _lib.ABI_VERSION == 9 and '#define HQT_ABI_VERSION 9' in header       # an entry point only: the structs and the version stay
    lib = _lib.load()                                # raises HqtLibraryError when the built library lacks a symbol of the table
    pos = (C.c_int32 * 2)(0, -1)
    assert lib.hqt_set_row_positions(None, 2, pos, 1) == -1 and b'null handle' in lib.hqt_last_error()
    assert lib.hqt_set_row_positions(None, 0, None, 0) == -1                      # ... also where the call would only clear
    # a NULL handle is refused by the taking entry points before they read anything else
    assert lib.hqt_sample(None, 2, None, None, None, None, None, None, None, None, None) == -1
