"""Rolling passes on the GPU (hqt_set_row_positions; row_positions=, pipeline.RollingSampler): rows of ONE pass at different positions.

A row of a rolling pass draws what a PLAIN call of the same B draws for it: Philox keys are (seed, global row, absolute position, draw, chunk), every buffer is
indexed by absolute position, and a row's arithmetic depends on its own position alone.  The bars are therefore equalities -- codes, raw logits rows and
log-probabilities, bit for bit -- and the reference of a request is never the rolling path: it is a plain call of the same B with the request's condition and key
in the same slot.  FAST references run with HQT_SWITCH_PERSIST 0: a rolling call takes the launch chain, and the persistent launch sums in another order.
Every engine starts from a NaN-poisoned workspace, and the buffers of a rolling pass start as -1 / NaN: what no request drew must still be -1 / NaN at the end."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import HQTransformerStage2
from hqtransformer_amd.pipeline import RollingSampler
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from tests.helpers import load, stage2_from_fixture

pytestmark = pytest.mark.gpu
PRECISIONS = {'exact': PRECISION_EXACT, 'fast': PRECISION_FAST, 'split': PRECISION_SPLIT}
SLOTS, N = 3, 5


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_steps=None):
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # every workspace buffer starts as NaN / -1: a row no kernel wrote shows up
    try:
        e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img)
        e.load(stage2=weights)
        e.finalize()
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    return e


def sample_any(eng, L, B, cond, n, force=None, **kw):
    if L == 3:
        return eng.sample3(B, cond, n, force=force, **kw)
    force = force or (None, None)
    return eng.sample(B, cond, n, force_top=force[0], force_bot=force[1], **kw)


def plain(eng, L, B, cond, n, **kw):
    """One plain call -> (codes list, logits [n, draws, B, V], logprobs [B, n, draws])."""
    out = sample_any(eng, L, B, cond, n, return_logits=True, return_logprobs=True, **kw)
    return list(out[:L]), out[L], out[L + 1]


class Pass:
    """The buffers a rolling pass lives in, poisoned: codes -1, logits and log-probabilities NaN."""

    def __init__(self, L, B, n, V):
        self.L, self.B, self.n = L, B, n
        draws = (4 ** L - 1) // 3
        self.codes = [torch.full((B, n) + ((4 ** l,) if l else ()), -1, dtype=torch.int64, device=dev()) for l in range(L)]
        self.logits = torch.full((n, draws, B, V), float('nan'), dtype=torch.float32, device=dev())
        self.logprobs = torch.full((B, n, draws), float('nan'), dtype=torch.float32, device=dev())

    def call(self, eng, cond, pos, k, **kw):
        sample_any(eng, self.L, self.B, cond, self.n, out=self.codes, logits_out=self.logits, logprobs_out=self.logprobs, row_positions=(list(pos), k), **kw)

    def row(self, b):
        return [c[b].clone() for c in self.codes], self.logits[:, :, b].clone(), self.logprobs[b].clone()

    def clear(self, b):
        for c in self.codes:
            c[b] = -1
        self.logits[:, :, b] = float('nan')
        self.logprobs[b] = float('nan')

    def untouched_from(self, b, t):
        """Positions >= t of slot b hold what the pass started with."""
        return (all(bool((c[b, t:] == -1).all()) for c in self.codes) and bool(torch.isnan(self.logits[t:, :, b]).all())
                and bool(torch.isnan(self.logprobs[b, t:]).all()))


def row_of(want, b):
    return [c[b] for c in want[0]], want[1][:, :, b], want[2][b]


def same_row(got, want):
    return all(torch.equal(x, y) for x, y in zip(got[0], want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


# ------------------------------------------------------------------------------- 1. a staggered pass equals the plain calls
_FIXTURES = {}
FIXTURES = ['g4_tiny_cls', 'g3_tiny_reduce_uncond', 'g13_tiny_cls_bidirectional', 'g7_l3_tiny_cls', 'g7_l3_tiny_cls_top2mid2bot']
# five requests with their own class, seed and global row offset; `join`: the first call that may admit them
REQUESTS = [dict(cls=3, seed=1001, offset=0, join=0), dict(cls=7, seed=2002, offset=11, join=0), dict(cls=1, seed=3003, offset=5, join=2),
            dict(cls=9, seed=4004, offset=2, join=3), dict(cls=4, seed=5005, offset=40, join=3)]


def fixture_case(name):
    if name not in _FIXTURES:
        fx = load(name + '.npz')
        spec, weights = stage2_from_fixture(fx)
        tk, tp, T = json.loads(str(fx['settings']))[-1] if 'settings' in fx.files else ((None,) * spec.levels, (None,) * spec.levels, (1.0,) * spec.levels)
        _FIXTURES[name] = (spec, engine_s2(spec, weights, SLOTS), dict(top_k=tk, top_p=tp, temperature=T), {})
    return _FIXTURES[name]


def reference(eng, spec, req, kw, cache, tag):
    """The plain call of SLOTS rows that holds the request in EVERY slot (its class, its key): row s is the reference of the request in slot s.  Computed once per
    (precision, graph) and shared; FAST: on the launch chain."""
    key = (tag, req['seed'])
    if key not in cache:
        cond = torch.full((SLOTS,), req['cls'] % spec.n_classes) if spec.cond == 1 else None
        eng.set_persist(False)
        try:
            cache[key] = plain(eng, spec.levels, SLOTS, cond, N, row_seeds=[req['seed']] * SLOTS, row_offsets=[req['offset']] * SLOTS, **kw)
        finally:
            eng.set_persist(True)
        assert bool(torch.isfinite(cache[key][1]).all()) and bool(torch.isfinite(cache[key][2]).all())
    return cache[key]


def run_staggered(eng, spec, k, kw, refs):
    """Two requests join at call 0, one at call 2, the rest as slots free up; `k` steps per call.  Returns the positions that shared a call."""
    L = spec.levels
    p = Pass(L, SLOTS, N, spec.vocab_top)
    pos, who = [-1] * SLOTS, [None] * SLOTS
    cls, seeds, offs = [0] * SLOTS, [0] * SLOTS, [0] * SLOTS
    waiting, finished, shared, call = list(range(len(REQUESTS))), [], [], 0
    while waiting or any(q >= 0 for q in pos):
        for s in range(SLOTS):
            if pos[s] < 0 and waiting and REQUESTS[waiting[0]]['join'] <= call:
                who[s] = waiting.pop(0)
                r = REQUESTS[who[s]]
                pos[s], cls[s], seeds[s], offs[s] = 0, r['cls'] % max(spec.n_classes, 1), r['seed'], r['offset']
        shared.append(tuple(pos))
        cond = torch.tensor(cls) if spec.cond == 1 else None
        p.call(eng, cond, pos, k, row_seeds=seeds, row_offsets=offs, **kw)
        for s in range(SLOTS):
            if pos[s] < 0:
                assert p.untouched_from(s, 0), f'call {call}: the empty slot {s} was written'
                continue
            nxt = pos[s] + k
            assert p.untouched_from(s, min(nxt, N)), f'call {call}: slot {s} was written beyond position {min(nxt, N) - 1}'
            if nxt >= N:                             # finished (k = 2: possibly in the first step of the call, idle in the second)
                got = p.row(s)
                assert same_row(got, row_of(refs(REQUESTS[who[s]]), s)), f'call {call}: request {who[s]} in slot {s} differs from its plain call'
                finished.append(who[s])
                p.clear(s)
                pos[s], who[s] = -1, None
            else:
                pos[s] = nxt
        call += 1
        assert call < 40
    assert sorted(finished) == list(range(len(REQUESTS)))
    assert all(p.untouched_from(s, 0) for s in range(SLOTS)), 'an entry no request drew was written'
    return shared


@pytest.mark.parametrize('precision', sorted(PRECISIONS))
@pytest.mark.parametrize('name', FIXTURES)
def test_a_staggered_pass_equals_the_plain_calls_bit_for_bit(name, precision):
    spec, eng, cut, cache = fixture_case(name)
    for graph in (False, True):
        kw = dict(precision=PRECISIONS[precision], use_graph=graph, **cut)
        # (the references first: a plain call on the engine ends its rolling pass)
        refs = {req['seed']: reference(eng, spec, req, kw, cache, (precision, graph)) for req in REQUESTS}
        for k in (1, 2):
            shared = run_staggered(eng, spec, k, kw, lambda req: refs[req['seed']])
            # the schedule is what the test is about: rows at different positions share a step, and a slot is reused behind a finished row
            assert any(len({q for q in ps if q >= 0}) > 1 for ps in shared) and len(shared) > (N + k - 1) // k
    eng.range_check()


# ------------------------------------------------------------------------------- 2. per-row samplers and forced levels
def test_rows_at_different_positions_keep_their_own_samplers_and_forced_codes():
    spec, eng, cut, _ = fixture_case('g4_tiny_cls')
    L, V = spec.levels, spec.vocab_top
    table = [((1.3, 0.7), (20, 11), (0.6, 0.95)), ((0.8, 1.1), (None, 64), (None, 0.9)), ((1.0, 1.0), (None, None), (None, None))]
    cond, seeds, offs = torch.tensor([2, 5, 0]), [71, 72, 73], [3, 9, 0]
    force_top = torch.from_numpy(np.random.default_rng(5).integers(0, V, (SLOTS, N)))
    for graph in (False, True):
        base = dict(precision=PRECISION_EXACT, use_graph=graph, row_seeds=seeds, row_offsets=offs, row_samplers=table)
        p = Pass(L, SLOTS, N, V)
        p.call(eng, cond, [0, -1, -1], 2, **base)                                # slot 0: positions 0, 1
        force_top[0, :2] = p.codes[0][0, :2].cpu()                               # (a forced level reads the code of position pos - 1 from force_*: the draw)
        p.call(eng, cond, [2, 0, -1], 1, force=(force_top, None), **base)        # slots 0 and 1 at positions 2 and 0, the top level forced
        # out_* holds the DRAW of a forced level, and the next call reads the codes of the position in front of it from out_*: a caller that wants the pass
        # to go on from the forced code puts it there, as a segmented pass would (hqt_set_segment)
        drawn = (p.codes[0][0, 2].clone(), p.codes[0][1, 0].clone())
        p.codes[0][0, 2], p.codes[0][1, 0] = force_top[0, 2], force_top[1, 0]
        p.call(eng, cond, [3, 1, -1], N, **base)                                 # both to their end
        assert p.untouched_from(2, 0)
        # the plain call of a row: the top code fed forward is the forced one at the position the forced call drew, the row's own draw everywhere else
        feed = p.codes[0].clone()
        feed[2] = 0
        p.codes[0][0, 2], p.codes[0][1, 0] = drawn
        want = plain(eng, L, SLOTS, cond, N, force=(feed, None), **base)
        for s in (0, 1):
            assert same_row(p.row(s), row_of(want, s)), f'graph={graph}: slot {s} differs from its plain call'
        assert not torch.equal(p.codes[0][0], p.codes[0][1])
    eng.range_check()


# ------------------------------------------------------------------------------- 3. a guided pair in a rolling pass
def test_a_guided_pair_rolls_with_a_third_row_elsewhere():
    spec, eng, cut, _ = fixture_case('g4_tiny_cls')
    L, V = spec.levels, spec.vocab_top
    cond, seeds, offs = torch.tensor([2, 8, 5]), [81, 81, 83], [4, 4, 0]
    pairs = [(0, 1, (2.5, 1.5))]
    for graph in (False, True):
        base = dict(precision=PRECISION_EXACT, use_graph=graph, row_seeds=seeds, row_offsets=offs, **cut)
        p = Pass(L, SLOTS, N, V)
        p.call(eng, cond, [-1, -1, 0], 2, **base)                                # the third row: positions 0, 1
        p.call(eng, cond, [0, 0, 2], 1, guidance=pairs, **base)                  # the pair joins at 0 beside a row at 2
        p.call(eng, cond, [1, 1, 3], N, guidance=pairs, **base)
        want = plain(eng, L, SLOTS, cond, N, guidance=pairs, **base)
        for s in range(SLOTS):
            assert same_row(p.row(s), row_of(want, s)), f'graph={graph}: slot {s} differs from the plain guided call'
        assert all(torch.equal(c[0], c[1]) for c in p.codes)
    eng.range_check()


# ------------------------------------------------------------------------------- 4. both body attention kernels
SPEC_H64 = dict(embed_dim=128, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                n_classes=10, cond=1, embedding=0)          # head size 64, as tests/test_gpu_attention_paths.py


@pytest.mark.parametrize('B,kernel', [(256, 'heads8'), (5, 'generic')])
def test_both_body_attention_kernels_take_per_row_positions(B, kernel):
    spec = Stage2Spec(**SPEC_H64)
    eng = engine_s2(spec, synth.stage2_weights(spec, 301, 'fixture'), B, max_steps=N)
    cond = torch.from_numpy(np.arange(B) % spec.n_classes)
    seeds, offs = [500 + (b % 7) for b in range(B)], [3 * b for b in range(B)]
    base = dict(precision=PRECISION_FAST, row_seeds=seeds, row_offsets=offs)
    group = [b % 3 for b in range(B)]                        # neighbouring rows -- lane groups of one wave -- stand at different positions
    p = Pass(2, B, N, spec.vocab_top)
    p.call(eng, cond, [0 if g == 0 else -1 for g in group], N - 2, use_graph=True, **base)
    p.call(eng, cond, [N - 2 if g == 0 else (0 if g == 1 else -1) for g in group], 1, use_graph=True, **base)
    eng.timing(True)                                         # a timed pass runs eagerly and reports the kernel variants it launched
    eng.timing_reset()
    p.call(eng, cond, [N - 1 if g == 0 else (1 if g == 1 else 0) for g in group], 1, use_graph=False, **base)      # positions n - 1, 1 and 0 in one step
    report = eng.timing_report()
    eng.timing(False)
    ran = {name: v[0] for name, v in report.items() if name.startswith('variant:attn_') and name.endswith(':body') and v[0]}
    assert ran == {f'variant:attn_{kernel}:body': spec.n_layers}, ran
    assert not any('persist' in name and v[0] for name, v in report.items()), 'a rolling call took the persistent launch'
    p.call(eng, cond, [-1 if g == 0 else (2 if g == 1 else 1) for g in group], N, use_graph=True, **base)
    eng.set_persist(False)
    want = plain(eng, 2, B, cond, N, use_graph=True, **base)
    for what, got, ref in (('codes_top', p.codes[0], want[0][0]), ('codes_bot', p.codes[1], want[0][1]), ('logits', p.logits, want[1]), ('logprobs', p.logprobs, want[2])):
        assert torch.equal(got, ref), f'{kernel}: {what} of the rolling pass differ from the plain FAST call of {B} rows'
    eng.range_check()
    eng.close()


# ------------------------------------------------------------------------------- 5. errors
def raises(eng, code, match, fn):
    with pytest.raises(_lib.HqtError, match=match) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def test_errors_name_their_cause_and_keep_the_pass():
    spec, eng, cut, _ = fixture_case('g4_tiny_cls')
    L, V = spec.levels, spec.vocab_top
    cond = torch.tensor([1, 2, 3])
    base = dict(precision=PRECISION_EXACT, seed=9)
    INVALID, STATE = -1, -3
    p = Pass(L, SLOTS, N, V)
    p.call(eng, cond, [-1, -1, -1], 1, **base)               # a first call of empty slots only: legal, draws nothing
    assert all(p.untouched_from(s, 0) for s in range(SLOTS))
    p.call(eng, cond, [0, -1, 0], 2, **base)
    raises(eng, STATE, 'row 0 continues at position 3, but the slot stands at position 2', lambda: p.call(eng, cond, [3, -1, 2], 1, **base))
    raises(eng, STATE, 'row 1 continues at position 2, but the slot is empty', lambda: p.call(eng, cond, [2, 2, 2], 1, **base))
    p.call(eng, cond, [2, 0, 2], 1, **base)                  # the failed calls kept the pass
    raises(eng, STATE, 'rolling pass has B=3, this call has B=2',
           lambda: Pass(L, 2, N, V).call(eng, cond[:2], [3, 1], 1, **base))
    raises(eng, STATE, 'rolling pass has n_steps=5, this call has n_steps=4',
           lambda: Pass(L, SLOTS, 4, V).call(eng, cond, [3, 1, 3], 1, **base))
    raises(eng, STATE, 'rolling pass runs in precision 0, this call asks for precision 1',
           lambda: p.call(eng, cond, [3, 1, 3], 1, precision=PRECISION_FAST, seed=9))
    raises(eng, STATE, 'rolling pass', lambda: eng.select_rows([0, 1]))
    # what the host surface refuses first is also refused by the library: staged by hand, taken by the next call
    lib, h = eng.lib, eng.h
    stream = _lib.C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)

    def staged(pos, k=1):
        arr = (_lib.C.c_int32 * len(pos))(*pos)
        _lib.check(lib.hqt_set_row_positions(h, len(pos), arr, k))

    def taken(**kw):
        sample_any(eng, L, SLOTS, cond, N, out=p.codes, **{**base, **kw})

    staged([3, 1, 3])
    _lib.check(lib.hqt_set_segment(h, 0, 2))
    raises(eng, INVALID, 'together with a staged segment', taken)
    staged([3, 1, 3])
    raises(eng, INVALID, 'together with a staged keep table', lambda: taken(keep=(torch.zeros((SLOTS, N), dtype=torch.bool), [c.clamp(min=0) for c in p.codes])))
    staged([3, 1])
    raises(eng, INVALID, 'staged a table of B=2, this call has B=3', taken)
    staged([3, 1, 3], k=N + 1)
    raises(eng, INVALID, r'k=6 outside \[1, n_steps = 5\]', taken)
    with pytest.raises(_lib.HqtError, match=r'pos\[1\]=-2 outside') as ei:
        staged([0, -2, 0])
    assert ei.value.code == INVALID
    with pytest.raises(_lib.HqtError, match=r'B=4 outside \[1, max_batch=3\]') as ei:
        staged([0, 0, 0, 0])
    assert ei.value.code == INVALID
    raises(eng, INVALID, 'rows 0 and 1 stand at different positions', lambda: p.call(eng, cond, [3, 1, 3], 1, guidance=[(0, 1, 2.0)], row_seeds=[5, 5, 6], row_offsets=[0, 0, 0],
                                                                                       precision=PRECISION_EXACT))
    raises(eng, INVALID, 'exactly one of rows 0 and 1 is an empty slot', lambda: p.call(eng, cond, [3, -1, 3], 1, guidance=[(0, 1, 2.0)], row_seeds=[5, 5, 6], row_offsets=[0, 0, 0],
                                                                                        precision=PRECISION_EXACT))
    p.call(eng, cond, [3, 1, 3], 1, **base)                  # none of them ended the pass
    # a plain call writes the body cache: the pass is over
    sample_any(eng, L, SLOTS, cond, N, **base)
    raises(eng, STATE, 'row 0 continues at position 4, and this handle holds no rolling pass', lambda: p.call(eng, cond, [4, 2, 4], 1, **base))
    p.call(eng, cond, [0, -1, 0], 1, **base)                 # ... and a new one begins with joins
    eng.range_check()


def test_text_handles_and_prefix_entry_points_are_refused():
    fx = load('g3_tiny_txt.npz')
    spec, weights = stage2_from_fixture(fx)
    eng = engine_s2(spec, weights, 2)
    arr = (_lib.C.c_int32 * 2)(0, 0)
    with pytest.raises(_lib.HqtError, match='text-conditional handle is not built .*prompt prefill') as ei:
        _lib.check(eng.lib.hqt_set_row_positions(eng.h, 2, arr, 1))
    assert ei.value.code == -1
    eng.close()
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        eng = Engine(spec, None, dev(), 2, spec.ctx_len_img, max_prefix=2)
        eng.load(stage2=weights)
        eng.finalize()
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    _lib.check(eng.lib.hqt_set_row_positions(eng.h, 2, arr, 1))
    prefix = [torch.zeros((2, 1), dtype=torch.int64), torch.zeros((2, 1, 4), dtype=torch.int64)]
    with pytest.raises(_lib.HqtError, match='taken by a prefix entry point') as ei:
        eng.sample(2, torch.tensor([1, 2]), N, precision=PRECISION_EXACT, prefix=prefix)
    assert ei.value.code == -1
    out = eng.sample(2, torch.tensor([1, 2]), N, precision=PRECISION_EXACT, prefix=prefix)      # ... which cleared the table: a plain prefix call
    assert bool((out[0] >= 0).all())
    eng.close()


# ------------------------------------------------------------------------------- 6. RollingSampler end to end
def test_rolling_sampler_returns_what_each_request_draws_alone():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    st2 = HQTransformerStage2(spec)
    st2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    st2 = st2.to('cuda')
    n = 6
    reqs = [dict(cond=(3 * i + 1) % spec.n_classes, seed=900 + 13 * i) for i in range(7)]
    kws = [dict(top_k_top=40 + i, top_k_bot=20, softmax_temperature=[1.0, 0.9]) if i % 2 else {} for i in range(7)]
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # (the model builds its engine when the sampler asks for one)
    try:
        rs = RollingSampler(st2, 3, n, precision='exact', return_logprobs=True)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    tickets = [rs.submit(r['cond'], r['seed'], **kw) for r, kw in zip(reqs[:4], kws)]
    done = rs.step() + rs.step(2)
    tickets += [rs.submit(r['cond'], r['seed'], **kw) for r, kw in zip(reqs[4:], kws[4:])]
    done += rs.drain()
    assert sorted(d[0] for d in done) == tickets == list(range(7))
    for ticket, codes, lp in done:
        r = reqs[ticket]
        want = sampling_ihqgpt(st2, 1, r['cond'], max_seq_len=n, seed=r['seed'], precision='exact', is_tqdm=False, **kws[ticket])
        assert torch.equal(codes[0], want[0][0]) and torch.equal(codes[1], want[1][0]), f'request {ticket} differs from its own call'
        assert tuple(lp.shape) == (n, 5) and bool(torch.isfinite(lp).all())
    st2.range_check()
