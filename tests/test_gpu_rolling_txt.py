"""Rolling passes of text-conditional models on the GPU (hqt_set_max_joins; Engine(max_joins=), pipeline.RollingSampler(max_joins=)).

A row that joins a text pass draws position 0 in a prompt prefill of its own -- the join phase, in front of the k steps of its call -- and then stands behind its
prompt like a row of a plain call; it advances by 1 + k in that call, every other row by k.  As in tests/test_gpu_rolling.py the bars are equalities, bit for bit,
of codes, raw logits rows and log-probabilities, and the reference of a request is never the rolling path: it is a plain call of the same B on a SECOND engine (a
plain call on the engine of the pass would end the pass).  In EXACT it is the unshared call that holds the request's prompt and key in every slot.  In FAST and
SPLIT a prefill over fewer rows may be served by other GEMM kernels, so the reference of a join is the plain call that prefills the same prompts: prompt_groups
whose groups are the joiners in ascending slot order (FAST: on the launch chain, which a rolling call takes).
Every engine starts from a NaN-poisoned workspace, and the buffers of a pass start as -1 / NaN: what no request drew must still be -1 / NaN after every call."""
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_rolling as R
from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT
from hqtransformer_amd.engine import Engine, new_draw_report
from hqtransformer_amd.models import HQTransformerStage2
from hqtransformer_amd.pipeline import RollingSampler
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from hqtransformer_amd.text import pad_caption
from tests.test_gpu_text_prefix import _random_spec

pytestmark = pytest.mark.gpu
SLOTS, N, JOINS = 3, 5, 2
dev, Pass, plain, sample_any, same_row, row_of, raises = R.dev, R.Pass, R.plain, R.sample_any, R.same_row, R.row_of, R.raises
# five requests with their own prompt (row i of PROMPTS), seed and global row offset; `join`: the first call that may admit them
REQUESTS = [dict(seed=1001, offset=0, join=0), dict(seed=2002, offset=11, join=0), dict(seed=3003, offset=5, join=2),
            dict(seed=4004, offset=2, join=3), dict(seed=5005, offset=40, join=3)]


def engine_txt(spec, weights, max_batch, max_joins=0, max_steps=None):
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # every workspace buffer starts as NaN / -1: a row no kernel wrote shows up
    try:
        e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img, max_joins=max_joins)
        e.load(stage2=weights)
        e.finalize()
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    return e


def prompts_of(spec, seed=1800, n=len(REQUESTS)):
    return torch.from_numpy(synth.text_ids(seed, n, spec.ctx_len_txt, spec.vocab_txt))


_CASES = {}


def case(kind):
    """(spec, the rolling engine with max_joins = JOINS, the engine of the plain references, sampler cut-offs, prompts, reference cache), built once per model."""
    if kind not in _CASES:
        if kind == 'tiny':
            spec, weights, (tk, tp, T) = _random_spec('tiny')
            cut = dict(top_k=tk, top_p=tp, temperature=T)
        else:                                        # three code levels with text: the model of test_three_level_shared_call_is_the_unshared_call_exact
            spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=64, vocab_bot=64, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                              n_classes=0, cond=2, embedding=0, levels=3)
            weights, cut = synth.stage2_weights(spec, 5, 'fixture'), dict(top_k=(50, 40, 30))
        _CASES[kind] = (spec, engine_txt(spec, weights, SLOTS, JOINS), engine_txt(spec, weights, SLOTS), cut, prompts_of(spec), {})
    return _CASES[kind]


def moved(pos, k):
    """Where a slot stands behind a call of k steps it entered at `pos`: a joiner drew position 0 in front of the steps."""
    return pos + k + (1 if pos == 0 else 0)


def run_staggered(eng, spec, prompts, k, kw, ref_row):
    """Two requests join at call 0, one at call 2, the rest as slots free up; `k` steps per call.  `ref_row(request, slot, joiners)`: the reference row of a
    request that joined in `slot` in a call whose joiners were `joiners` = ((slot, request), ...) in ascending slot order.  Returns the positions of every call."""
    L, T = spec.levels, spec.ctx_len_txt
    p = Pass(L, SLOTS, N, spec.vocab_top)
    pos, who, event = [-1] * SLOTS, [None] * SLOTS, [None] * SLOTS
    cond, seeds, offs = torch.zeros((SLOTS, T), dtype=torch.int64), [0] * SLOTS, [0] * SLOTS
    waiting, finished, shared, call = list(range(len(REQUESTS))), [], [], 0
    while waiting or any(q >= 0 for q in pos):
        joiners = []
        for s in range(SLOTS):
            if pos[s] < 0 and waiting and REQUESTS[waiting[0]]['join'] <= call and len(joiners) < JOINS:
                who[s] = waiting.pop(0)
                r = REQUESTS[who[s]]
                pos[s], seeds[s], offs[s] = 0, r['seed'], r['offset']
                cond[s] = prompts[who[s]]
                joiners.append((s, who[s]))
        for s, _ in joiners:
            event[s] = tuple(joiners)
        shared.append(tuple(pos))
        p.call(eng, cond.clone(), pos, k, row_seeds=seeds, row_offsets=offs, **kw)
        for s in range(SLOTS):
            if pos[s] < 0:
                assert p.untouched_from(s, 0), f'call {call}: the empty slot {s} was written'
                continue
            nxt = moved(pos[s], k)
            assert p.untouched_from(s, min(nxt, N)), f'call {call}: slot {s} was written beyond position {min(nxt, N) - 1}'
            if nxt >= N:                             # finished (possibly before the last step of the call: idle from there on)
                assert same_row(p.row(s), ref_row(who[s], s, event[s])), f'call {call}: request {who[s]} in slot {s} differs from its plain call'
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


def unshared_reference(ref, spec, prompts, cache, kw, tag):
    """EXACT: the plain unshared call of SLOTS rows that holds the request's prompt and key in every slot (row s for slot s), once per request."""
    def ref_row(q, s, joiners):
        if (tag, q) not in cache:
            r = REQUESTS[q]
            cache[(tag, q)] = plain(ref, spec.levels, SLOTS, prompts[q].expand(SLOTS, -1).contiguous(), N, row_seeds=[r['seed']] * SLOTS,
                                    row_offsets=[r['offset']] * SLOTS, **kw)
            assert bool(torch.isfinite(cache[(tag, q)][1]).all()) and bool(torch.isfinite(cache[(tag, q)][2]).all())
        return row_of(cache[(tag, q)], s)
    return ref_row


def assert_staggered(shared, k):
    # the schedule is what the test is about: rows at different positions share a step, and a slot is reused behind a finished row
    assert any(len({q for q in ps if q >= 0}) > 1 for ps in shared) and len(shared) > (N + k - 1) // k
    assert any(0 in ps and any(q > 0 for q in ps) for ps in shared), 'no row joined beside a row that is mid-image'
    assert any(ps.count(0) == 2 for ps in shared) and any(ps.count(0) == 1 for ps in shared)


# ------------------------------------------------------------------------------- 1., 3. EXACT: a staggered pass equals the plain unshared calls
@pytest.mark.parametrize('kind', ['tiny', 'l3'])
def test_a_staggered_text_pass_equals_the_plain_unshared_calls_exact(kind):
    spec, eng, ref, cut, prompts, cache = case(kind)
    for graph in (False, True):
        kw = dict(precision=PRECISION_EXACT, use_graph=graph, **cut)
        ref_row = unshared_reference(ref, spec, prompts, cache, kw, ('exact', graph))
        for k in (1, 2):
            assert_staggered(run_staggered(eng, spec, prompts, k, kw, ref_row), k)
    eng.range_check()


# ------------------------------------------------------------------------------- 2. FAST and SPLIT: the plain call that prefills the same prompts
@pytest.mark.parametrize('precision', ['fast', 'split'])
def test_a_staggered_text_pass_equals_the_plain_calls_that_prefill_the_same_prompts(precision):
    spec, eng, ref, cut, prompts, cache = case('tiny')
    ref.set_persist(False)                           # a rolling call takes the launch chain, and the persistent launch sums in another order
    try:
        for graph in (False, True):
            kw = dict(precision=R.PRECISIONS[precision], use_graph=graph, **cut)

            def ref_row(q, s, joiners):
                key = (precision, graph, joiners)
                if key not in cache:                 # the joiners are groups 0 .. J - 1 with their keys in their slots; every other row: group 0, any key
                    groups, seeds, offs = [0] * SLOTS, [7] * SLOTS, [0] * SLOTS
                    for g, (slot, req) in enumerate(joiners):
                        groups[slot], seeds[slot], offs[slot] = g, REQUESTS[req]['seed'], REQUESTS[req]['offset']
                    cond = torch.stack([prompts[req] for _, req in joiners])
                    cache[key] = plain(ref, spec.levels, SLOTS, cond, N, row_seeds=seeds, row_offsets=offs, prompt_groups=groups, **kw)
                    assert bool(torch.isfinite(cache[key][1]).all()) and bool(torch.isfinite(cache[key][2]).all())
                return row_of(cache[key], s)
            for k in (1, 2):
                assert_staggered(run_staggered(eng, spec, prompts, k, kw, ref_row), k)
    finally:
        ref.set_persist(True)
    eng.range_check()


# ------------------------------------------------------------------------------- 4. a guided pair joins beside a row that is mid-image
def test_a_guided_pair_joins_a_text_pass_beside_a_row_that_is_mid_image():
    spec, eng, ref, cut, prompts, _ = case('tiny')
    L, V, T = spec.levels, spec.vocab_top, spec.ctx_len_txt
    cond = torch.stack([prompts[0], pad_caption(1, T)[0], prompts[1]])               # the pair: a prompt and the all-PAD negative prompt
    seeds, offs, pairs = [81, 81, 83], [4, 4, 0], [(0, 1, (2.5, 1.5))]
    for graph in (False, True):
        base = dict(precision=PRECISION_EXACT, use_graph=graph, row_seeds=seeds, row_offsets=offs, **cut)
        p = Pass(L, SLOTS, N, V)
        p.call(eng, cond, [-1, -1, 0], 1, **base)                                # the third row joins alone: positions 0, 1
        assert p.untouched_from(2, 2) and p.untouched_from(0, 0) and p.untouched_from(1, 0)
        p.call(eng, cond, [0, 0, 2], 1, guidance=pairs, **base)                  # the pair joins (0, 1) beside a row at 2
        assert p.untouched_from(0, 2) and p.untouched_from(1, 2) and p.untouched_from(2, 3)
        p.call(eng, cond, [2, 2, 3], N, guidance=pairs, **base)
        want = plain(ref, L, SLOTS, cond, N, guidance=pairs, **base)
        for s in range(SLOTS):
            assert same_row(p.row(s), row_of(want, s)), f'graph={graph}: slot {s} differs from the plain guided call'
        assert all(torch.equal(c[0], c[1]) for c in p.codes) and not torch.equal(p.codes[0][0], p.codes[0][2])
    eng.range_check()


# ------------------------------------------------------------------------------- 5. per-row samplers, a forced level and the draw report
def test_rows_of_a_text_pass_keep_their_samplers_forced_codes_and_report():
    spec, eng, ref, _, prompts, _ = case('tiny')
    L, V, draws, top_n = spec.levels, spec.vocab_top, 5, 3
    table = [((1.3, 0.7), (20, 11), (0.6, 0.95)), ((0.8, 1.1), (None, 64), (None, 0.9)), ((1.0, 1.0), (None, None), (None, None))]
    cond, seeds, offs = prompts[:SLOTS].clone(), [71, 72, 73], [3, 9, 0]
    force_top = torch.from_numpy(np.random.default_rng(5).integers(0, V, (SLOTS, N)))
    for graph in (False, True):
        base = dict(precision=PRECISION_EXACT, use_graph=graph, row_seeds=seeds, row_offsets=offs, row_samplers=table)
        p, rep = Pass(L, SLOTS, N, V), new_draw_report(SLOTS, N, draws, top_n, dev())
        p.call(eng, cond, [0, -1, -1], 2, report_out=rep, **base)                # slot 0: position 0 in the join phase, then 1 and 2
        assert bool((rep.rank[0, :3] >= 0).all()) and bool((rep.rank[0, 3:] == -1).all()) and bool((rep.rank[1:] == -1).all())
        force_top[0, :3] = p.codes[0][0, :3].cpu()                               # (a forced level reads the code of position pos - 1 from force_*: the draw)
        p.call(eng, cond, [3, 0, -1], 1, force=(force_top, None), report_out=rep, **base)      # slot 0 at 3; slot 1 joins: 0 in the join phase, then 1; top level forced
        # out_* holds the DRAW of a forced level, and the next call reads the codes of the position in front of it from out_*: a caller that wants the pass
        # to go on from the forced code puts it there, as a segmented pass would (hqt_set_segment)
        at = [(0, 3), (1, 0), (1, 1)]
        drawn = [p.codes[0][s, t].clone() for s, t in at]
        for s, t in at:
            p.codes[0][s, t] = force_top[s, t]
        p.call(eng, cond, [4, 2, -1], N, report_out=rep, **base)                 # both to their end
        assert p.untouched_from(2, 0) and bool((rep.rank[2] == -1).all()) and bool(torch.isnan(rep.entropy[2]).all())
        # the plain call of a row: the top code fed forward is the forced one at the positions the forced call drew, the row's own draw everywhere else
        feed = p.codes[0].clone()
        feed[2] = 0
        for (s, t), d in zip(at, drawn):
            p.codes[0][s, t] = d
        want_rep = new_draw_report(SLOTS, N, draws, top_n, dev())
        want = plain(ref, L, SLOTS, cond, N, force=(feed, None), report_out=want_rep, **base)
        for s in (0, 1):
            assert same_row(p.row(s), row_of(want, s)), f'graph={graph}: slot {s} differs from its plain call'
            for f, g in zip(rep, want_rep):
                assert torch.equal(f[s], g[s]) or (f.is_floating_point() and torch.equal(torch.nan_to_num(f[s], nan=-7.0), torch.nan_to_num(g[s], nan=-7.0))), \
                    f'graph={graph}: the draw report of slot {s} differs from its plain call'
        assert not torch.equal(p.codes[0][0], p.codes[0][1])
    eng.range_check()


# ------------------------------------------------------------------------------- 6. sizing and refusals
def test_sizing_refusals_and_the_plain_call_behind_a_pass():
    spec, weights, (tk, tp, T) = _random_spec('tiny')
    cut = dict(top_k=tk, top_p=tp, temperature=T)
    L, V, Tt, D = spec.levels, spec.vocab_top, spec.ctx_len_txt, spec.embed_dim
    INVALID, STATE = -1, -3
    eng = engine_txt(spec, weights, SLOTS)
    prompts = prompts_of(spec)
    cond = prompts[:SLOTS].clone()
    base = dict(precision=PRECISION_EXACT, seed=9, **cut)
    before_plain = plain(eng, L, SLOTS, cond, N, **base)
    # a text handle that never sized its joins is refused as it always was, by the library and on the host
    arr = (_lib.C.c_int32 * SLOTS)(0, 0, -1)
    with pytest.raises(_lib.HqtError, match='text-conditional handle is not built .*prompt prefill.*hqt_set_max_joins') as ei:
        _lib.check(eng.lib.hqt_set_row_positions(eng.h, SLOTS, arr, 1))
    assert ei.value.code == INVALID
    with pytest.raises(ValueError, match='text-conditional model is not built .*prompt prefill'):
        Pass(L, SLOTS, N, V).call(eng, cond, [0, 0, -1], 1, **base)
    for bad in (-1, SLOTS + 1):
        with pytest.raises(_lib.HqtError, match=rf'max_joins={bad} outside \[0, max_batch={SLOTS}\]') as ei:
            eng.set_max_joins(bad)
        assert ei.value.code == INVALID and eng.max_joins == 0
    # the call grows the workspace once, by the staging of JOINS prompts and the gathered rows; later calls allocate nothing
    torch.cuda.synchronize()
    sizes = [eng.workspace_bytes()]
    eng.set_max_joins(JOINS)
    sizes.append(eng.workspace_bytes())
    assert sizes[1] - sizes[0] == JOINS * 2 * spec.n_layers * Tt * D * 4 + SLOTS * D * 4, sizes
    eng.set_max_joins(1)                                                         # smaller: nothing shrinks, and one row may join per call
    raises(eng, INVALID, r'2 rows join at position 0 .*max_joins=1', lambda: sample_staged(eng, L, cond, [0, 0, -1], 1, base))
    eng.set_max_joins(JOINS)
    assert eng.workspace_bytes() == sizes[1]
    p = Pass(L, SLOTS, N, V)
    p.call(eng, cond, [0, -1, 0], 1, **base)
    torch.cuda.synchronize()
    assert eng.workspace_bytes() == sizes[1]
    # the host refuses too many joiners first; staged by hand the library does, naming both numbers -- and keeps the pass
    with pytest.raises(ValueError, match=r'3 rows join at position 0 .*max_joins=2'):
        p.call(eng, cond, [0, 0, 0], 1, **base)
    raises(eng, INVALID, r'3 rows join at position 0 .*max_joins=2', lambda: sample_staged(eng, L, cond, [0, 0, 0], 1, base, out=p.codes))
    raises(eng, STATE, 'hqt_set_max_joins: this handle holds a rolling pass', lambda: eng.set_max_joins(3))
    raises(eng, STATE, 'hqt_set_max_joins: this handle holds a rolling pass', lambda: eng.set_max_joins(0))
    raises(eng, STATE, 'row 0 continues at position 1, but the slot stands at position 2', lambda: p.call(eng, cond, [1, -1, 2], 1, **base))
    raises(eng, STATE, 'rolling pass', lambda: eng.select_rows([0, 1]))
    stage_positions(eng, [2, -1, 2], 1)
    _lib.check(eng.lib.hqt_set_prompt_groups(eng.h, SLOTS, 1, (_lib.C.c_int32 * SLOTS)(0, 0, 0)))
    raises(eng, INVALID, 'together with a staged prompt-group table', lambda: sample_any(eng, L, SLOTS, cond, N, out=p.codes, **base))
    stage_positions(eng, [2, -1, 2], 1)
    _lib.check(eng.lib.hqt_set_segment(eng.h, 0, 2))
    raises(eng, INVALID, 'together with a staged segment', lambda: sample_any(eng, L, SLOTS, cond, N, out=p.codes, **base))
    stage_positions(eng, [2, -1, 2], 1)
    raises(eng, INVALID, 'together with a staged keep table',
           lambda: sample_any(eng, L, SLOTS, cond, N, out=p.codes, keep=(torch.zeros((SLOTS, N), dtype=torch.bool), [c.clamp(min=0) for c in p.codes]), **base))
    p.call(eng, cond, [2, 0, 2], N, **base)                                      # none of them ended the pass: the record was kept; slot 1 joins now
    torch.cuda.synchronize()
    assert eng.workspace_bytes() == sizes[1]
    for s in range(SLOTS):                                                       # (seed=9: the implicit keys of the plain call, row s)
        assert same_row(p.row(s), row_of(before_plain, s)), f'slot {s} differs from the plain call'
    # the pass is over (every slot finished): sizing is free again, and a plain call draws what it drew before the handle ever rolled
    eng.set_max_joins(JOINS)
    after_plain = plain(eng, L, SLOTS, cond, N, **base)
    assert all(torch.equal(a, b) for a, b in zip(after_plain[0], before_plain[0])) and torch.equal(after_plain[1], before_plain[1]) and torch.equal(after_plain[2], before_plain[2])
    assert eng.workspace_bytes() == sizes[1]
    eng.set_max_joins(0)                                                         # off again: refused as before, nothing freed
    with pytest.raises(_lib.HqtError, match='text-conditional handle is not built .*prompt prefill') as ei:
        _lib.check(eng.lib.hqt_set_row_positions(eng.h, SLOTS, arr, 1))
    assert ei.value.code == INVALID and eng.workspace_bytes() == sizes[1]
    eng.range_check()
    eng.close()
    # a handle that is not text-conditional has nothing to size
    fx = R.load('g4_tiny_cls.npz')
    cspec, cweights = R.stage2_from_fixture(fx)
    ceng = R.engine_s2(cspec, cweights, 2)
    with pytest.raises(_lib.HqtError, match='hqt_set_max_joins: the handle is not text-conditional') as ei:
        ceng.set_max_joins(1)
    assert ei.value.code == INVALID
    ceng.close()


def stage_positions(eng, pos, k):
    arr = (_lib.C.c_int32 * len(pos))(*pos)
    _lib.check(eng.lib.hqt_set_row_positions(eng.h, len(pos), arr, k))


def sample_staged(eng, L, cond, pos, k, base, out=None):
    """A rolling call whose table goes to the library by hand, past the checks of the host surface."""
    stage_positions(eng, pos, k)
    out = out or Pass(L, SLOTS, N, eng.s2.vocab_top).codes
    sample_any(eng, L, SLOTS, cond, N, out=out, **base)


# ------------------------------------------------------------------------------- 7. RollingSampler end to end
def test_rolling_sampler_returns_what_each_text_request_draws_alone():
    spec, weights, _ = _random_spec('tiny')
    st2 = HQTransformerStage2(spec)
    st2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    st2 = st2.to('cuda')
    n = 6
    prompts = prompts_of(spec, 1900, 7)
    reqs = [dict(cond=prompts[i], seed=900 + 13 * i) for i in range(7)]
    kws = [dict(top_k_top=40 + i, top_k_bot=20, softmax_temperature=[1.0, 0.9]) if i % 2 else {} for i in range(7)]
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # (the model builds its engine when the sampler asks for one)
    try:
        rs = RollingSampler(st2, 3, n, max_joins=2, precision='exact', return_logprobs=True)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    tickets = [rs.submit(r['cond'], r['seed'], **kw) for r, kw in zip(reqs[:4], kws)]
    done = rs.step()
    assert rs.pos == [2, 2, -1] and len(rs.queue) == 2                             # two joins per call: the third slot stays free for the next one
    done += rs.step(2)
    assert rs.pos == [4, 4, 3]
    tickets += [rs.submit(r['cond'], r['seed'], **kw) for r, kw in zip(reqs[4:], kws[4:])]
    done += rs.drain()
    assert sorted(d[0] for d in done) == tickets == list(range(7))
    for ticket, codes, lp in done:
        r = reqs[ticket]
        want = sampling_ihqgpt(st2, 1, r['cond'][None], max_seq_len=n, seed=r['seed'], precision='exact', is_tqdm=False, **kws[ticket])
        assert torch.equal(codes[0], want[0][0]) and torch.equal(codes[1], want[1][0]), f'request {ticket} differs from its own call'
        assert tuple(lp.shape) == (n, 5) and bool(torch.isfinite(lp).all())
    st2.range_check()
