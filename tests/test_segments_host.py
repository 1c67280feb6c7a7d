"""Paused passes (hqt_set_segment, hqt_select_rows): what can be checked without a GPU -- the binding table against the header, argument checks that
raise before any engine call, and the bookkeeping of pipeline.SamplingSession / sample_best_of(prune=) / HQTransformerStage2.sampling_step against a stub engine."""
import os
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, pipeline
from hqtransformer_amd.engine import Engine, check_segment, check_select_rows
from hqtransformer_amd.pipeline import SamplingSession, check_prune, prune_survivors, rank_candidates, sample_best_of
from hqtransformer_amd.spec import Stage2Spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spec_of(**kw):
    base = dict(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=64, ctx_len_txt=16,
                n_classes=10, cond=1, embedding=0)
    base.update(kw)
    return Stage2Spec(**base)


def test_binding_table_and_header_hold_both_symbols():
    assert _lib.SYMBOLS['hqt_set_segment'] == (_lib.C.c_int, [_lib.C.c_void_p, _lib.C.c_int, _lib.C.c_int])
    assert len(_lib.SYMBOLS['hqt_select_rows'][1]) == 4
    with open(os.path.join(ROOT, 'include', 'hqt.h')) as fp:
        header = fp.read()
    assert 'int hqt_set_segment(hqt_handle* h, int start, int stop);' in header
    assert 'int hqt_select_rows(hqt_handle* h, int B_new, const int32_t* rows_from, void* stream);' in header
    assert _lib.ABI_VERSION == 9 and '#define HQT_ABI_VERSION 9' in header       # entry points only: the structs and the version stay


def test_segment_arguments_are_checked_on_the_host():
    assert check_segment(8, None) is None and check_segment(8, (0, 8)) == (0, 8) and check_segment(8, [3, 4]) == (3, 4)
    for bad in ((2, 2), (3, 2), (-1, 2), (0, 9)):
        with pytest.raises(ValueError, match='0 <= start < stop <= n_steps = 8'):
            check_segment(8, bad)
    for bad in (3, (1,), (0, 1, 2), (0.0, 2), (True, 2)):
        with pytest.raises(ValueError, match='segment'):
            check_segment(8, bad)
    with pytest.raises(ValueError, match='prefix'):
        check_segment(8, (0, 2), prefix=[torch.zeros((1, 1))])
    with pytest.raises(ValueError, match='keep'):
        check_segment(8, (0, 2), keep=(None, None))
    with pytest.raises(ValueError, match='starts at 0'):
        check_segment(8, (2, 4), prompt_groups=[0, 0])
    assert check_segment(8, (0, 4), prompt_groups=[0, 0]) == (0, 4)
    # Engine.sample raises before it touches the library: this "engine" has none
    eng = Engine.__new__(Engine)
    eng.s2, eng.device, eng.max_batch, eng.max_prefix = spec_of(), torch.device('cpu'), 4, 0
    with pytest.raises(ValueError, match='0 <= start < stop'):
        eng.sample(2, torch.zeros(2, dtype=torch.int64), 8, segment=(4, 4))
    with pytest.raises(ValueError, match='reads the codes of position 1 from out'):
        eng.sample(2, torch.zeros(2, dtype=torch.int64), 8, segment=(2, 4))
    with pytest.raises(ValueError, match='three code tensors'):
        eng.sample3(2, torch.zeros(2, dtype=torch.int64), 8, out=[torch.zeros((2, 8))])


def test_select_rows_arguments_are_checked_on_the_host():
    got = check_select_rows([3, 3, 0], 4, 8)
    assert got.dtype == np.int32 and got.tolist() == [3, 3, 0] and got.flags['C_CONTIGUOUS']
    assert check_select_rows(torch.tensor([1, 0]), None, 2).tolist() == [1, 0]
    with pytest.raises(ValueError, match=r'outside \[0, B=4\)'):
        check_select_rows([0, 4], 4, 8)
    with pytest.raises(ValueError, match='outside'):
        check_select_rows([-1], None, 8)
    with pytest.raises(ValueError, match='exceeds max_batch=2'):
        check_select_rows([0, 0, 0], 4, 2)
    with pytest.raises(ValueError, match='integers'):
        check_select_rows([0.0, 1.0], 4, 8)
    for bad in ([], [[0, 1]]):
        with pytest.raises(ValueError, match='one-dimensional'):
            check_select_rows(bad, 4, 8)


def test_prune_arguments_are_checked_on_the_host():
    assert check_prune([(16, 4), (32, 2)], 8, 1, 64) == [(16, 4), (32, 2)]
    for bad, match in (([], 'expected a list'), ([(16,)], 'entries'), ([(16, 4), (16, 2)], 'ascend'), ([(0, 4)], 'ascend'), ([(64, 4)], 'ascend'),
                       ([(16, 8)], 'descend'), ([(16, 4), (32, 4)], 'descend'), ([(16, 1)], 'keep=2')):
        with pytest.raises(ValueError, match=match):
            check_prune(bad, 8, 2, 64)
    st = stage2_stub(spec_of())
    with pytest.raises(ValueError, match='ascend'):                              # ... before an engine is asked for
        sample_best_of(st, 3, 8, 1, prune=[(9, 4)], max_seq_len=8)
    st.engine = lambda *a, **k: (_ for _ in ()).throw(AssertionError('an engine was built before the arguments were validated'))
    for k, v in (('prefix_codes', [torch.zeros((8, 1))]), ('keep_mask', torch.ones((8, 8))), ('guidance_scale', 2.0)):
        with pytest.raises(ValueError, match=f'prune together with {k}'):
            sample_best_of(st, 3, 8, 1, prune=[(4, 4)], max_seq_len=8, **{k: v})


# ------------------------------------------------------------------------------- a stub engine: codes and log-probabilities that name the key that drew them
class StubEngine:
    """Engine.sample / select_rows as far as a session can tell: position t of a row keyed (seed, offset) holds the code (seed + offset + t) % 512 on every
    level and the log-probability -(seed % 10) - 0.01 t in every draw."""
    device, max_batch = torch.device('cpu'), 16

    def __init__(self):
        self.calls, self.paused, self.fed = [], None, []

    def sample(self, B, cond, n, *, out, segment, logprobs_out, row_seeds, row_offsets, **kw):
        start, stop = segment
        assert (start == 0) == (self.paused is None), 'a continuation needs the paused pass, a first segment none'
        assert start == 0 or self.paused == (B, start)
        assert len(row_seeds) == len(row_offsets) == B == out[0].shape[0] and (cond is None or len(cond) == B)
        for b in range(B):
            for t in range(start, stop):
                for o in out:
                    o[b, t] = (row_seeds[b] + row_offsets[b] + t) % 512
                if logprobs_out is not None:
                    logprobs_out[b, t] = -(row_seeds[b] % 10) - 0.01 * t
        # what a forced top level feeds: its codes at the positions drawn, and at start - 1 (where the engine reads the previous codes of a forced level);
        # without one, the previous top codes are those of `out`
        ft = kw.get('force_top')
        self.fed.append((None if start == 0 else (out[0] if ft is None else ft)[:, start - 1].tolist(), None if ft is None else ft[:, start:stop].tolist()))
        self.paused = (B, stop) if stop < n else None
        self.calls.append(('sample', B, segment, dict(kw), None if cond is None else torch.as_tensor(cond).tolist()))

    def select_rows(self, table, paused_batch=None):
        assert self.paused is not None and paused_batch == self.paused[0] and max(table) < paused_batch
        self.paused = (len(table), self.paused[1])
        self.calls.append(('select', [int(r) for r in table]))
        return len(table)


def stage2_stub(spec, eng=None):
    return types.SimpleNamespace(spec=spec, use_cls_cond=spec.cond == 1, use_txt_cond=spec.cond == 2, engine=lambda *a, **k: eng)


def test_session_keys_codes_and_conditions_follow_their_rows_through_select():
    eng = StubEngine()
    s = SamplingSession(stage2_stub(spec_of(), eng), 4, torch.tensor([1, 2, 3, 4]), 6, seed=100, sample_offset=10, return_logprobs=True, top_k_top=50)
    assert (s.position, s.done, s.row_seeds, s.row_offsets) == (0, False, [100] * 4, [10, 11, 12, 13])
    so_far = s.advance(2, softmax_temperature=[0.5, 2.0])
    assert s.position == 2 and [tuple(c.shape) for c in so_far] == [(4, 2), (4, 2, 4)]
    call = eng.calls[-1]
    assert call[2] == (0, 2) and call[3]['top_k'] == (50, None) and call[3]['temperature'] == (0.5, 2.0) and call[3]['seed'] == 0
    s.select([3, 3, 0], row_seeds=[100, 7, 100], row_offsets=[13, 0, 10])         # a fork with a key of its own, and a survivor
    assert eng.calls[-1] == ('select', [3, 3, 0])
    assert (s.B, s.row_seeds, s.row_offsets, s.cond.tolist()) == (3, [100, 7, 100], [13, 0, 10], [4, 4, 1])
    assert s.codes[0][:, :2].tolist() == [[113, 114], [113, 114], [110, 111]] and torch.isnan(s.logprobs[:, 2:]).all()
    s.advance(1)
    assert eng.calls[-1][1:3] == (3, (2, 3)) and eng.calls[-1][3]['temperature'] == (1.0, 1.0) and eng.calls[-1][4] == [4, 4, 1]
    s.select([2, 0])                                                             # keys travel with their rows
    assert (s.row_seeds, s.row_offsets) == ([100, 100], [10, 13])
    codes = s.finish()
    assert s.done and s.position == 6 and codes[0].tolist() == [[110, 111, 112, 113, 114, 115], [113, 114, 115, 116, 117, 118]]
    assert codes[1][1, 5].tolist() == [118] * 4 and not torch.isnan(s.logprobs).any()
    with pytest.raises(ValueError, match='finished'):
        s.advance(1)
    with pytest.raises(ValueError, match='finished'):
        s.select([0])
    assert s.finish() is codes


def test_session_refuses_bad_arguments_before_the_engine_sees_them():
    eng = StubEngine()
    st = stage2_stub(spec_of(), eng)
    with pytest.raises(TypeError, match='unexpected keywords'):
        SamplingSession(st, 2, 3, 6, prefix_codes=[None])
    with pytest.raises(ValueError, match='ctx_len_img'):
        SamplingSession(st, 2, 3, 65)
    with pytest.raises(ValueError, match='come together'):
        SamplingSession(st, 2, 3, 6, row_seeds=[1, 2])
    with pytest.raises(ValueError, match='share_prompts'):
        SamplingSession(st, 2, 3, 6, share_prompts=True)
    s = SamplingSession(st, 2, 3, 6, seed=1)
    for k in (0, 7, -1):
        with pytest.raises(ValueError, match='remaining positions'):
            s.advance(k)
    with pytest.raises(TypeError, match='unexpected keywords'):
        s.advance(1, seed=3)
    s.advance(3)
    for bad in ([2], [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]):
        with pytest.raises(ValueError, match='rows_from'):
            s.select(bad)
    with pytest.raises(ValueError, match='one per new row'):
        s.select([0, 1, 1], row_seeds=[1, 2], row_offsets=[0, 1])
    assert eng.calls == [('sample', 2, (0, 3), eng.calls[0][3], [3, 3])]          # none of the refused calls reached the engine


def test_select_gathers_the_row_table_and_asks_for_new_guidance_pairs():
    eng = StubEngine()
    rows = [((1.0, 1.0), (10 + b, None), (None, None)) for b in range(4)]
    s = SamplingSession(stage2_stub(spec_of(), eng), 4, 3, 6, seed=1, row_samplers=rows, guidance=[(0, 1, 2.0), (2, 3, 2.0)])
    s.advance(2)
    with pytest.raises(ValueError, match='guidance pairs name rows by index'):
        s.select([2, 3])
    assert eng.calls[-1][0] == 'sample' and s.B == 4                            # refused before anything moved
    s.select([3, 2, 2], guidance=[(1, 2, 1.5)])
    s.advance(1)
    assert eng.calls[-1][3]['row_samplers'] == [rows[3], rows[2], rows[2]] and eng.calls[-1][3]['guidance'] == [(1, 2, 1.5)]
    s.select([0], guidance=[])
    s.advance(1)
    assert eng.calls[-1][3]['row_samplers'] == [rows[3]] and eng.calls[-1][3]['guidance'] is None


def shim_model(eng):
    from hqtransformer_amd.models import HQTransformerStage2
    spec = spec_of()
    st = HQTransformerStage2.__new__(HQTransformerStage2)
    st.spec, st.use_cls_cond, st.use_txt_cond = spec, True, False
    st.engine = lambda *a, **k: eng
    return st


def test_sampling_step_shim_finds_its_session_and_obeys_the_loops_codes():
    eng = StubEngine()
    st = shim_model(eng)
    cond = torch.tensor([1, 2])
    with pytest.raises(ValueError, match='not its embedding'):
        st.sampling_step(sos=torch.zeros((2, 1, 128)))
    kw = dict(seed=100, max_seq_len=3, top_k_top=7, softmax_temperature=[0.5, 1.0])
    top, bot, presents = st.sampling_step(sos=cond, codes_t=None, codes_b=None, pos_codes=None, past=None, **kw)
    assert tuple(top.shape) == (2, 1) and tuple(bot.shape) == (2, 1, 4) and top[:, 0].tolist() == [100, 101]
    assert len(presents) == 1 and len(st._step_sessions) == 1
    session = next(iter(st._step_sessions.values()))
    assert eng.calls[-1][2] == (0, 1) and eng.calls[-1][3]['top_k'] == (7, None) and eng.calls[-1][3]['temperature'] == (0.5, 1.0)
    past = [torch.stack(presents).clone().detach()]                            # what the reference's loop keeps
    # the loop hands back ALTERED codes: they are written at position 0 before position 1 is drawn, and the step finds its session through `past`
    top, bot, presents = st.sampling_step(sos=cond, codes_t=torch.tensor([[7], [8]]), codes_b=torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]]), past=past, **kw)
    assert session.position == 2 and session.codes[0][:, 0].tolist() == [7, 8] and session.codes[1][1, 0].tolist() == [5, 6, 7, 8]
    assert eng.calls[-1][2] == (1, 2) and eng.fed[-1] == ([7, 8], None) and top[:, 0].tolist() == [101, 102]
    past.append(torch.stack(presents).clone().detach())
    with pytest.raises(ValueError, match='does not belong to a running session'):
        st.sampling_step(sos=cond, past=[torch.tensor([[12345]])], **kw)
    # a given top code: fed forward at this position, the DRAWN code of the position before it still in front of it, and returned as the reference returns it
    top, bot, presents = st.sampling_step(sos=cond, codes_t=top, codes_b=bot[:, 0], past=past, given_top_code=torch.tensor([40, 41]), **kw)
    assert eng.fed[-1] == ([101, 102], [[40], [41]]) and top[:, 0].tolist() == [40, 41] and session.codes[0].tolist() == [[7, 101, 40], [8, 102, 41]]
    assert bot[:, 0, 0].tolist() == [102, 103]
    # done: dropped, and its `past` names nothing any more
    assert session.done and st._step_sessions == {}
    with pytest.raises(ValueError, match='does not belong to a running session'):
        st.sampling_step(sos=cond, past=past, **kw)
    # a loop abandoned half way is forgotten when the next one begins (one paused pass per lane)
    _, _, p1 = st.sampling_step(sos=cond, past=None, **kw)
    eng.paused = None                                                          # (the engine: a segment from 0 ends the paused pass)
    _, _, p2 = st.sampling_step(sos=cond, past=None, **kw)
    assert len(st._step_sessions) == 1 and int(p1[0]) != int(p2[0])
    with pytest.raises(ValueError, match='does not belong to a running session'):
        st.sampling_step(sos=cond, past=[torch.stack(p1)], **kw)
    # the given code travels in ONE tensor per session: the engine sees one pointer at every position
    eng2 = StubEngine()
    st2 = shim_model(eng2)
    _, _, p = st2.sampling_step(sos=cond, past=None, given_top_code=torch.tensor([1, 2]), **kw)
    st2.sampling_step(sos=cond, past=[torch.stack(p)], given_top_code=torch.tensor([3, 4]), **kw)
    assert eng2.calls[0][3]['force_top'] is eng2.calls[1][3]['force_top'] and eng2.fed[-1] == ([1, 2], [[3], [4]])


def test_prune_survivors_and_the_tie_rule():
    scores = torch.tensor([[-3.0, -1.0, -1.0, -2.0], [-5.0, -5.0, -5.0, -5.0]], dtype=torch.float64)
    assert rank_candidates(scores, 2).tolist() == [[1, 2], [0, 1]]                  # ties to the lower candidate index
    assert prune_survivors(scores, 3).tolist() == [[1, 2, 3], [0, 1, 2]]            # ... and the survivors in candidate order
    assert prune_survivors(torch.tensor([[-1.0, -9.0, -1.0, -1.0]], dtype=torch.float64), 2).tolist() == [[0, 2]]


def test_pruned_best_of_selects_group_major_survivors(monkeypatch):
    """Two classes, 4 candidates each; the stub scores a row by its seed, so per-row seeds make candidate c of both groups score -(c' % 10) per entry."""
    eng = StubEngine()
    st = stage2_stub(spec_of(), eng)
    # scores per entry: candidates 0..3 of group 0 -> -3, -1, -1, -2; of group 1 -> -2, -2, -0, -9
    seeds = [3, 1, 11, 2, 2, 12, 0, 9]
    codes, scores = sample_best_of(st, torch.tensor([5, 9]), 4, 1, prune=[(2, 2)], max_seq_len=4, row_seeds=seeds, row_offsets=list(range(8)))
    selects = [c for c in eng.calls if c[0] == 'select']
    assert selects == [('select', [1, 2, 4 + 0, 4 + 2])]                            # group-major; the tie in group 0 keeps candidates 1 and 2, in group 1 the lower of 0 and 1
    assert [c[1:3] for c in eng.calls if c[0] == 'sample'] == [(8, (0, 2)), (4, (2, 4))]
    assert eng.calls[-1][4] == [5, 5, 9, 9]
    # final ranking: group 0 ties again (seeds 1 and 11) -> the lower candidate, row keyed (1, 1); group 1 -> seed 0, row keyed (0, 6)
    assert codes[0].tolist() == [[2, 3, 4, 5], [6, 7, 8, 9]] and tuple(codes[1].shape) == (2, 4, 4)
    want = torch.tensor([[-(1.0 * 20 + 0.01 * 5 * 6)], [-(0.01 * 5 * 6)]], dtype=torch.float64)
    assert scores.dtype == torch.float64 and torch.allclose(scores, want, atol=1e-5)


def test_prune_none_never_touches_the_session_path(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('prune=None built a session')
    monkeypatch.setattr(pipeline, 'SamplingSession', boom)
    monkeypatch.setattr(pipeline, '_best_of_pruned', boom)
    seen = {}

    def fake_sample_codes(stage2, num, cond, **kw):
        seen.update(kw, num=num)
        return [torch.zeros((num, 4), dtype=torch.int64), torch.zeros((num, 4, 4), dtype=torch.int64), torch.zeros((num, 4, 5))]
    monkeypatch.setattr(pipeline, 'sample_codes', fake_sample_codes)
    codes, scores = sample_best_of(stage2_stub(spec_of()), torch.tensor([5, 9]), 3, 2, max_seq_len=4, seed=1)
    assert seen == dict(num=6, return_logprobs=True, max_seq_len=4, seed=1) and tuple(scores.shape) == (2, 2) and tuple(codes[0].shape) == (4, 4)
