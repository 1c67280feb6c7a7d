"""Kept positions in rolling passes (hqt_set_join_run; RollingSampler(join_run=), submit(keep_mask=, kept_codes=)): what can be checked without a GPU -- the
host check of a rolling call with a keep table, the admission by shared leading run and the position rule L + 1 + k of pipeline.RollingSampler against a fake
engine that keeps the record the library keeps, the validation of masks and codes, and the new symbol in the built library and the header."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.engine import check_row_positions
from hqtransformer_amd.pipeline import RollingSampler
from tests.test_rolling_host import spec_of, stage2_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeKeepEngine:
    """Engine.sample / set_join_run as far as a rolling sampler can tell.  It applies the library's rule to the table it is given: the rows at position 0 share
    L = min(their smallest leading run of ones, max_run, n - 1); a join phase runs on a text model or where L > 0 and moves them on by L + 1 + k, every other row
    moves by k; a kept cell inside the span a row passes holds the kept code, a drawn one 1000 + position; a slot that neither joins, stays empty nor continues
    where the record has it is refused."""
    device = torch.device('cpu')

    def __init__(self, max_prefix, text=False):
        self.max_prefix, self.text, self.calls, self.next, self.join_run = int(max_prefix), text, [], None, None

    def set_join_run(self, max_joins, max_run):
        assert 0 <= max_run <= self.max_prefix and self.next is None
        self.join_run = (int(max_joins), int(max_run))

    def sample(self, B, cond, n, *, out, row_positions, keep=None, **kw):
        pos, k = row_positions
        want = self.next or [-1] * B
        for b, p in enumerate(pos):
            assert p in (-1, 0, want[b]), f'slot {b} at position {p}: the pass has it at {want[b]}'
        assert keep is not None and self.join_run is not None
        mask, kept = np.asarray(keep[0]).astype(bool), keep[1]
        assert mask.shape == (B, n)
        joiners = [b for b, p in enumerate(pos) if p == 0]
        L = min([self.join_run[1], n - 1] + [n if mask[b].all() else int(np.argmin(mask[b])) for b in joiners]) if joiners else 0
        assert sum(p == 0 for p in pos) <= self.join_run[0]
        phase = bool(joiners) and (self.text or L > 0)
        self.calls.append(dict(pos=list(pos), k=k, L=L, phase=phase))
        nxt = []
        for b, p in enumerate(pos):
            if p < 0:
                nxt.append(-1)
                continue
            to = min(p + k + (L + 1 if phase and p == 0 else 0), n)
            for t in range(p, to):
                for lv, o in enumerate(out):
                    o[b, t] = kept[lv][b, t] if mask[b, t] else 1000 + t
            nxt.append(to if to < n else -1)
        self.next = nxt if any(q >= 0 for q in nxt) else None


def request(n, run, extra=(), base=0):
    m = np.zeros(n, bool)
    m[:run] = True
    m[list(extra)] = True
    return m, [torch.arange(n) + base, (torch.arange(n) + base)[:, None].repeat(1, 4)]


def test_check_row_positions_takes_keep_only_with_the_flag():
    keep = object()
    pos, k = check_row_positions(1, 3, 8, ([4, -1, 0], 2), keep=keep, rolling_keep=True)
    assert pos.tolist() == [4, -1, 0] and k == 2
    with pytest.raises(ValueError, match='row_positions together with keep is not built'):
        check_row_positions(1, 3, 8, ([4, -1, 0], 2), keep=keep)
    with pytest.raises(ValueError, match='row_positions together with keep is not built'):
        check_row_positions(1, 3, 8, ([4, -1, 0], 2), keep=keep, rolling_keep=False)
    for what in ('prefix', 'prompt_groups', 'segment'):                      # these stay refused, opted in or not
        with pytest.raises(ValueError, match=f'row_positions together with {what}'):
            check_row_positions(1, 3, 8, ([0, 0, 0], 1), rolling_keep=True, **{what: object()})
    with pytest.raises(ValueError, match='text-conditional'):               # a text model still needs max_joins
        check_row_positions(2, 3, 8, ([0, 0, 0], 1), keep=keep, rolling_keep=True)


def test_admission_by_shared_run_and_the_position_rule():
    n = 8
    eng = FakeKeepEngine(max_prefix=3)
    rs = RollingSampler(stage2_stub(spec_of(), eng), 4, n, precision='exact', join_run=3)
    assert eng.join_run == (4, 3)
    # runs 2, 2, 5 (clipped to 3), 0: the head decides; the first request whose clipped run differs waits one call -- and then decides the next
    a = rs.submit(1, seed=1, keep_mask=request(n, 2, (6,))[0], kept_codes=request(n, 2, (6,))[1])
    b = rs.submit(2, seed=2, keep_mask=request(n, 2, base=100)[0], kept_codes=request(n, 2, base=100)[1])
    c = rs.submit(3, seed=3, keep_mask=request(n, 5, base=200)[0], kept_codes=request(n, 5, base=200)[1])
    d = rs.submit(4, seed=4)
    assert rs.step(2) == []
    assert eng.calls[0] == dict(pos=[0, 0, -1, -1], k=2, L=2, phase=True) and rs.pos == [5, 5, -1, -1] and [q[0] for q in rs.queue] == [c, d]
    done = rs.step(2)                                                         # c joins alone (run 3): 3 + 1 + 2; a and b draw positions 5, 6
    assert eng.calls[1] == dict(pos=[5, 5, 0, -1], k=2, L=3, phase=True) and rs.pos == [7, 7, 6, -1] and done == [] and [q[0] for q in rs.queue] == [d]
    done = rs.step(2)                                                         # d joins without a run: no join phase, it advances by k
    assert eng.calls[2] == dict(pos=[7, 7, 6, 0], k=2, L=0, phase=False) and rs.pos == [-1, -1, -1, 2]
    assert [t[0] for t in done] == [a, b, c]
    got = {t[0]: t[1] for t in done}
    assert got[a][0].tolist() == [0, 1, 1002, 1003, 1004, 1005, 6, 1007]      # kept cells verbatim, run and interior; the rest drawn
    assert got[b][0].tolist() == [100, 101] + [1000 + t for t in range(2, n)]
    assert got[c][0].tolist() == [200, 201, 202, 203, 204] + [1005, 1006, 1007] and bool((got[c][1] == got[c][0][:, None]).all())
    done = rs.drain(3)
    assert [t[0] for t in done] == [d] and done[0][1][0].tolist() == [1000 + t for t in range(n)]
    assert [cl['pos'] for cl in eng.calls[3:]] == [[-1, -1, -1, 2], [-1, -1, -1, 5]] and rs.live == 0 and not rs.keep_mask.any()


def test_join_run_zero_makes_every_kept_position_a_step_and_text_joins_advance_by_one_more():
    n = 5
    eng = FakeKeepEngine(max_prefix=0)
    rs = RollingSampler(stage2_stub(spec_of(cond=0), eng), 2, n, join_run=0)
    m, codes = request(n, 3)
    rs.submit(None, seed=1, keep_mask=m, kept_codes=codes)
    rs.submit(None, seed=2)                                                   # both runs clip to 0: they join together
    assert rs.step(2) == [] and eng.calls[0] == dict(pos=[0, 0], k=2, L=0, phase=False) and rs.pos == [2, 2]
    done = rs.drain(2)
    assert done[0][1][0].tolist() == [0, 1, 2, 1003, 1004] and done[1][1][0].tolist() == [1000 + t for t in range(n)]
    # a text model: the join phase runs for every joiner, L + 1 + k with L = 1 here
    eng = FakeKeepEngine(max_prefix=1, text=True)
    rs = RollingSampler(stage2_stub(spec_of(cond=2), eng), 2, n, max_joins=2, join_run=1)
    assert eng.join_run == (2, 1)
    m, codes = request(n, 4)
    rs.submit([1] * 16, seed=1, keep_mask=m, kept_codes=codes)
    rs.submit([2] * 16, seed=2)                                               # run 0 differs from the head's clipped run 1: it waits
    assert rs.step(1) == [] and eng.calls[0] == dict(pos=[0, -1], k=1, L=1, phase=True) and rs.pos == [3, -1]
    assert rs.step(1) == [] and eng.calls[1] == dict(pos=[3, 0], k=1, L=0, phase=True) and rs.pos == [4, 2]


def test_masks_and_codes_are_validated_before_anything_is_queued():
    n = 6
    with pytest.raises(ValueError, match='join_run=3 exceeds max_prefix=2'):
        RollingSampler(stage2_stub(spec_of(), FakeKeepEngine(max_prefix=2)), 2, n, join_run=3)
    with pytest.raises(ValueError, match=r'join_run=6 outside \[0, n - 1 = 5\]'):
        RollingSampler(stage2_stub(spec_of(), FakeKeepEngine(max_prefix=8)), 2, n, join_run=6)
    plain = RollingSampler(stage2_stub(spec_of(), FakeKeepEngine(max_prefix=2)), 2, n)
    m, codes = request(n, 2)
    with pytest.raises(ValueError, match='join_run=R'):
        plain.submit(1, seed=1, keep_mask=m, kept_codes=codes)
    rs = RollingSampler(stage2_stub(spec_of(), FakeKeepEngine(max_prefix=2)), 2, n, join_run=2)
    with pytest.raises(ValueError, match='come together'):
        rs.submit(1, seed=1, keep_mask=m)
    with pytest.raises(ValueError, match=r'keep_mask: expected bool of shape \(6,\)'):
        rs.submit(1, seed=1, keep_mask=np.zeros(5, bool), kept_codes=codes)
    with pytest.raises(ValueError, match=r'keep_mask: expected bool'):
        rs.submit(1, seed=1, keep_mask=np.zeros(n, np.float32), kept_codes=codes)
    with pytest.raises(ValueError, match='2 code levels as one list'):
        rs.submit(1, seed=1, keep_mask=m, kept_codes=codes[:1])
    with pytest.raises(ValueError, match=r'kept_codes\[1\]: expected integer codes of shape \(6, 4\)'):
        rs.submit(1, seed=1, keep_mask=m, kept_codes=[codes[0], codes[1][:, :3]])
    with pytest.raises(ValueError, match=r'kept_codes\[0\]: expected integer codes'):
        rs.submit(1, seed=1, keep_mask=m, kept_codes=[codes[0].float(), codes[1]])
    bad = [codes[0].clone(), codes[1].clone()]
    bad[1][1, 2] = 512
    with pytest.raises(IndexError, match=r'kept_codes\[1\]: index out of range'):
        rs.submit(1, seed=1, keep_mask=m, kept_codes=bad)
    bad[1][1, 2], bad[0][4] = 0, -3                                           # outside the mask nothing is read
    assert rs.submit(1, seed=1, keep_mask=m, kept_codes=bad) == 0 and len(rs.queue) == 1
    rs3 = RollingSampler(stage2_stub(spec_of(levels=3), FakeKeepEngine(max_prefix=2)), 2, n, join_run=2)
    with pytest.raises(ValueError, match=r'kept_codes\[2\]: expected integer codes of shape \(6, 16\)'):
        rs3.submit(1, seed=1, keep_mask=m, kept_codes=codes + [torch.zeros(n, 4, dtype=torch.int64)])
    with pytest.raises(ValueError, match='three code levels'):               # text with three levels: only join_run=0
        RollingSampler(stage2_stub(spec_of(cond=2, levels=3), FakeKeepEngine(max_prefix=2, text=True)), 2, n, max_joins=2, join_run=1)


def test_the_built_library_exports_the_entry_point_and_refuses_a_null_handle():
    assert _lib.SYMBOLS['hqt_set_join_run'] == (C.c_int, [C.c_void_p, C.c_int, C.c_int])
    with open(os.path.join(ROOT, 'include', 'hqt.h')) as fp:
        header = fp.read()
    assert 'int hqt_set_join_run(hqt_handle* h, int max_joins, int max_run);' in header
    assert _lib.ABI_VERSION == 9 and '#define HQT_ABI_VERSION 9' in header       # an entry point only: the structs and the version stay
    lib = _lib.load()                                # raises HqtLibraryError when the built library lacks a symbol of the table
    assert lib.hqt_set_join_run(None, 1, 0) == -1 and b'null handle' in lib.hqt_last_error()
