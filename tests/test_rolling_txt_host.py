"""Rolling passes on text-conditional models (hqt_set_max_joins): what can be checked without a GPU -- the slot bookkeeping of pipeline.RollingSampler against a
fake engine that keeps the TEXT record rule (a row that joins in a call draws position 0 in its prompt prefill, in front of the k steps: it advances by 1 + k),
the argument checks that raise before any engine call, and the new symbol in the built library with the argument errors that need no device."""
import ctypes as C
import os

import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.engine import Engine, check_row_positions
from hqtransformer_amd.pipeline import RollingSampler
from tests.test_rolling_host import codes_of, spec_of, stage2_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, VT = 16, 64                                   # ctx_len_txt and vocab_txt of spec_of


class FakeTextEngine:
    """Engine.sample as far as a rolling sampler of a text model can tell.  The call is recorded; every position a row draws holds, on every level, the code
    (seed + offset + position) % 512 of the key its slot carried in that call, so a result names the request that drew it.  A row at position 0 draws
    [0, 1 + k), every other [pos, pos + k), clipped at n; the engine keeps the record the library keeps under that rule and refuses a slot that neither joins,
    stays empty nor continues where it stands, more joining rows than `max_joins`, and a cond that is not [B, ctx_len_txt]."""
    device, max_batch = torch.device('cpu'), 16

    def __init__(self, max_joins):
        self.calls, self.next, self.max_joins = [], None, max_joins

    def sample(self, B, cond, n, *, out, logprobs_out, row_seeds, row_offsets, row_samplers, row_positions, **kw):
        pos, k = row_positions
        assert len(pos) == len(row_seeds) == len(row_offsets) == len(row_samplers) == B == out[0].shape[0]
        assert tuple(cond.shape) == (B, T) and cond.dtype == torch.int64
        assert sum(p == 0 for p in pos) <= self.max_joins, f'{pos}: more than max_joins = {self.max_joins} rows join'
        want = self.next or [-1] * B
        for b, p in enumerate(pos):
            assert p in (-1, 0, want[b]), f'slot {b} at position {p}: the pass has it at {want[b]}'
        self.calls.append(dict(pos=list(pos), k=k, cond=cond.tolist(), seeds=list(row_seeds), offsets=list(row_offsets)))
        self.next = []
        for b, p in enumerate(pos):
            stop = -1 if p < 0 else min(p + k + (1 if p == 0 else 0), n)
            for t in range(p, stop):
                for o in out:
                    o[b, t] = (row_seeds[b] + row_offsets[b] + t) % 512
            self.next.append(stop if 0 <= stop < n else -1)


def prompt_of(i):
    return [(3 * i + t) % VT for t in range(T)]


def text_sampler(slots, n, max_joins, **kw):
    eng = FakeTextEngine(max_joins)
    return RollingSampler(stage2_stub(spec_of(cond=2), eng), slots, n, max_joins=max_joins, **kw), eng


def test_a_joiner_stands_at_1_plus_k_after_its_call_and_everyone_else_at_pos_plus_k():
    rs, eng = text_sampler(3, 8, 3)
    a = rs.submit(prompt_of(0), seed=100)
    assert rs.step(2) == [] and eng.calls[0]['pos'] == [0, -1, -1] and rs.pos == [3, -1, -1]          # the join drew 0, the steps 1 and 2
    b = rs.submit(torch.tensor(prompt_of(1)), seed=200, sample_offset=5)
    assert rs.step(2) == [] and eng.calls[1]['pos'] == [3, 0, -1] and rs.pos == [5, 3, -1]            # a continues by k, b joins by 1 + k
    assert eng.calls[1]['cond'][0] == prompt_of(0) and eng.calls[1]['cond'][1] == prompt_of(1) and eng.calls[1]['cond'][2] == [0] * T
    assert eng.calls[1]['seeds'][:2] == [100, 200] and eng.calls[1]['offsets'][:2] == [0, 5]
    assert rs.step(1) == [] and rs.pos == [6, 4, -1]
    done = rs.step(2)                                                                                 # a draws 6 and 7
    assert [d[0] for d in done] == [a] and done[0][1][0].tolist() == codes_of(100, 0, 8) and rs.pos == [-1, 6, -1] and rs.free == [0, 2]
    done = rs.drain(3)
    assert [d[0] for d in done] == [b] and done[0][1][0].tolist() == codes_of(200, 5, 8) and rs.live == 0
    assert [tuple(c.shape) for c in done[0][1]] == [(8,), (8, 4)]


def test_at_most_max_joins_requests_are_admitted_per_step():
    rs, eng = text_sampler(4, 6, 2)
    tickets = [rs.submit(prompt_of(i), seed=10 * i) for i in range(5)]
    assert rs.step() == [] and eng.calls[0]['pos'] == [0, 0, -1, -1] and len(rs.queue) == 3           # four free slots, two joins
    assert rs.step() == [] and eng.calls[1]['pos'] == [2, 2, 0, 0] and len(rs.queue) == 1
    assert rs.step() == [] and eng.calls[2]['pos'] == [3, 3, 2, 2] and len(rs.queue) == 1             # no free slot: the fifth waits
    done = rs.drain()
    assert sorted(d[0] for d in done) == tickets
    assert all(sum(p == 0 for p in c['pos']) <= 2 for c in eng.calls)
    for ticket, codes in done:
        assert codes[0].tolist() == codes_of(10 * ticket, 0, 6)


def test_a_request_that_finishes_in_its_joining_call_is_returned_by_that_step():
    for n, k in ((1, 1), (2, 1), (3, 2), (4, 4), (5, 4)):                                             # n <= 1 + k
        rs, eng = text_sampler(2, n, 1)
        a = rs.submit(prompt_of(1), seed=7)
        done = rs.step(k)
        assert [d[0] for d in done] == [a] and done[0][1][0].tolist() == codes_of(7, 0, n), (n, k)
        assert rs.pos == [-1, -1] and rs.free == [0, 1] and eng.next == [-1, -1]
        b = rs.submit(prompt_of(2), seed=9)                                                           # the slot is reused behind the finished row
        assert [d[0] for d in rs.step(k)] == [b] and eng.calls[1]['pos'] == [0, -1]
    rs, eng = text_sampler(2, 4, 1)                                                                   # n = 2 + k: one position is left
    rs.submit(prompt_of(1), seed=7)
    assert rs.step(2) == [] and rs.pos == [3, -1]


def test_drain_terminates_and_each_request_names_its_own_key():
    n = 7
    for k in (1, 2, 3, n):
        for max_joins in (1, 2):
            rs, eng = text_sampler(2, n, max_joins)
            tickets = [rs.submit(prompt_of(i), seed=5 * i, sample_offset=i) for i in range(5)]
            done = rs.drain(k)
            assert sorted(d[0] for d in done) == tickets and len(eng.calls) <= 5 * n
            for ticket, codes in done:
                assert codes[0].tolist() == codes_of(5 * ticket, ticket, n) and bool((codes[1] == codes[0][:, None]).all())
            assert rs.drain(k) == [] and rs.live == 0 and not rs.queue


def test_row_positions_on_a_text_model_need_max_joins_and_respect_it():
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill.*max_joins'):
        check_row_positions(2, 3, 8, ([0, 0, 0], 1))
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill'):
        check_row_positions(2, 3, 8, ([0, 0, 0], 1), max_joins=0)
    pos, k = check_row_positions(2, 3, 8, ([0, 4, 0], 2), max_joins=2)
    assert pos.tolist() == [0, 4, 0] and k == 2
    with pytest.raises(ValueError, match=r'3 rows join at position 0 .*max_joins=2'):
        check_row_positions(2, 3, 8, ([0, 0, 0], 1), max_joins=2)
    assert check_row_positions(2, 3, 8, ([5, -1, 3], 1), max_joins=1)[0].tolist() == [5, -1, 3]       # nobody joins
    for what in ('prefix', 'keep', 'prompt_groups', 'segment'):
        with pytest.raises(ValueError, match=f'row_positions together with {what}'):
            check_row_positions(2, 3, 8, ([0, 0, 0], 1), max_joins=3, **{what: object()})
    assert check_row_positions(1, 3, 8, ([0, 0, 0], 1))[0].tolist() == [0, 0, 0]                      # any other model: max_joins is not read
    # Engine.sample raises before it touches the library: this "engine" has none
    eng = Engine.__new__(Engine)
    eng.s2, eng.device, eng.max_batch, eng.max_prefix, eng.max_joins = spec_of(cond=2), torch.device('cpu'), 4, 0, 0
    cond = torch.zeros(2, T, dtype=torch.int64)
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill'):
        eng.sample(2, cond, 8, row_positions=([0, 0], 1))
    eng.max_joins = 1
    with pytest.raises(ValueError, match=r'2 rows join at position 0 .*max_joins=1'):
        eng.sample(2, cond, 8, row_positions=([0, 0], 1))
    with pytest.raises(ValueError, match='pass the tensors the pass lives in'):
        eng.sample(2, cond, 8, row_positions=([0, -1], 1))


def test_a_text_stub_is_refused_without_max_joins_before_an_engine_is_asked_for():
    def no_engine(*a, **k):
        raise AssertionError('an engine was built before the arguments were validated')
    st = stage2_stub(spec_of(cond=2))
    st.engine = no_engine
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill.*max_joins'):
        RollingSampler(st, 3, 8)
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill'):
        RollingSampler(st, 3, 8, max_joins=0)
    for bad in (4, -1, True):
        with pytest.raises(ValueError, match=r'max_joins=.* outside \[1, slots = 3\]'):
            RollingSampler(st, 3, 8, max_joins=bad)
    st = stage2_stub(spec_of())
    st.engine = no_engine
    with pytest.raises(ValueError, match='only a text-conditional model'):
        RollingSampler(st, 3, 8, max_joins=2)


def test_submit_checks_the_prompt():
    asked = []

    def engine(*a, **k):
        asked.append((a, k))
        return FakeTextEngine(2)
    st = stage2_stub(spec_of(cond=2))
    st.engine = engine
    rs = RollingSampler(st, 3, 8, max_joins=2)
    assert asked == [((3, 8, 0), {'max_joins': 2})]                                                   # the engine is asked for the staging of the joins
    for bad, match in ((None, 'one prompt of ctx_len_txt = 16'), (prompt_of(0)[:-1], r'shape \(15,\)'), ([prompt_of(0)], r'shape \(1, 16\)'),
                       ([0.5] * T, 'float'), (3, r'shape \(\)'), ([0] * (T - 1) + [VT], r'span \[0, 64\].*vocab_txt = 64'), ([-1] + [0] * (T - 1), r'span \[-1, 0\]')):
        with pytest.raises(ValueError, match=match):
            rs.submit(bad, seed=1)
    assert not rs.queue
    with pytest.raises(TypeError, match='guidance_scale'):
        rs.submit(prompt_of(0), seed=1, guidance_scale=2.0)
    assert rs.submit(prompt_of(0), seed=1) == 0 and rs.queue[0][1] == prompt_of(0)


def test_the_built_library_exports_the_entry_point_and_checks_its_arguments_without_a_device():
    assert _lib.SYMBOLS['hqt_set_max_joins'] == (C.c_int, [C.c_void_p, C.c_int])
    with open(os.path.join(ROOT, 'include', 'hqt.h')) as fp:
        header = fp.read()
    assert 'int hqt_set_max_joins(hqt_handle* h, int max_joins);' in header
    assert _lib.ABI_VERSION == 9 and '#define HQT_ABI_VERSION 9' in header       # an entry point only: the structs and the version stay
    lib = _lib.load()                                # raises HqtLibraryError when the built library lacks a symbol of the table
    assert lib.hqt_set_max_joins(None, 1) == -1 and b'null handle' in lib.hqt_last_error()
    assert lib.hqt_set_max_joins(None, 0) == -1
