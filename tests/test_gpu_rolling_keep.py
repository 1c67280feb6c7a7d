"""Kept positions in rolling passes on the GPU (hqt_set_join_run; Engine(join_run=), RollingSampler(join_run=), submit(keep_mask=, kept_codes=)).

A rolling call that takes a keep table scatters, per row, the kept codes of the span the row passes in the call; a kept position is an ordinary step whose draw
is discarded; the rows that join prefill the leading kept run L they share (clipped to max_run and n - 1) in the call's join phase and advance by L + 1 + k.  As
in tests/test_gpu_rolling.py the bars are equalities -- codes, raw logits rows and log-probabilities, bit for bit -- and the reference of a request is never the
rolling path: it is the plain ``keep=`` call of SLOTS rows with the request in every slot, on a SECOND engine whose max_prefix is the L of the call the request
joined in (so the plain call prefills exactly that run).  Rows of positions < L are written by neither side: the comparison starts at L, and the rolling pass must
still hold its poison there.  FAST / SPLIT references run with the persistent launch off: a rolling call takes the launch chain.
Every engine starts from a NaN-poisoned workspace, and the buffers of a pass start as -1 / NaN: what no request drew must still be -1 / NaN at the end."""
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_rolling as R
from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import HQTransformerStage2
from hqtransformer_amd.pipeline import RollingSampler
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O
from tests.helpers import gate, load, stage2_from_fixture
from tests.keep_ref import scattered_mask
from tests.test_gpu_text_prefix import _random_spec

pytestmark = pytest.mark.gpu
SLOTS, N = 3, 6                                      # the smallest sizes that leave a run, a kept interior cell and two draws
dev, Pass, plain, sample_any, raises = R.dev, R.Pass, R.plain, R.sample_any, R.raises
PRECISIONS = R.PRECISIONS
INVALID, STATE = -1, -3
# five requests: leading runs 2, 2, 0, 3 and 6 (fully kept) plus scattered interior cells; `join`: the first call that may admit them.  The two run-2 requests
# join together at call 0, the run-0 request at call 2 beside them, the last two -- runs 3 and 6, clipped to the handle's max_run -- into the slots they free
REQUESTS = [dict(cls=3, seed=1001, offset=0, join=0, run=2, extra=(4,)), dict(cls=7, seed=2002, offset=11, join=0, run=2, extra=()),
            dict(cls=1, seed=3003, offset=5, join=2, run=0, extra=(1, 3)), dict(cls=9, seed=4004, offset=2, join=3, run=3, extra=(5,)),
            dict(cls=4, seed=5005, offset=40, join=3, run=6, extra=())]


def engine_of(spec, weights, max_batch, max_prefix=0, **kw):
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # every workspace buffer starts as NaN / -1: a row no kernel wrote shows up
    try:
        e = Engine(spec, None, dev(), max_batch, spec.ctx_len_img, max_prefix=max_prefix, **kw)
        e.load(stage2=weights)
        e.finalize()
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    return e


def request_table(spec, q):
    """(mask [N] bool, kept codes per level [N(, 4 | 16)]) of request q: its own codes everywhere, read where the mask is set."""
    r = REQUESTS[q]
    rng = np.random.default_rng([r['seed'], 0x6b70])
    mask = scattered_mask(1, N, (r['run'],), ((0, r['extra']),))[0]
    return mask, [torch.from_numpy(rng.integers(0, spec.vocab_top, (N,) + ((4 ** l,) if l else ()))) for l in range(spec.levels)]


def clipped(run, max_run):
    return min(run, max_run, N - 1)


def compare_from(got, want, L, what):
    """A finished row of the pass against its plain keep call: codes everywhere (positions < L hold the kept codes on both sides), logits rows and
    log-probabilities from position L on, bit for bit; below L the pass still holds its poison."""
    assert all(torch.equal(x, y) for x, y in zip(got[0], want[0])), f'{what}: codes differ'
    assert torch.equal(got[1][L:], want[1][L:]) and bool(torch.isfinite(got[1][L:]).all()), f'{what}: logits rows differ'
    assert torch.equal(got[2][L:], want[2][L:]) and bool(torch.isfinite(got[2][L:]).all()), f'{what}: log-probabilities differ'
    assert bool(torch.isnan(got[1][:L]).all()) and bool(torch.isnan(got[2][:L]).all()), f'{what}: a row of a prefilled position was written'


def run_staggered(eng, spec, k, kw, max_run, ref_row, cond_of, text=False, max_joins=SLOTS):
    """Two requests join at call 0, one at call 2, the rest as slots free up; `k` steps per call, every call with the keep table of the slots.  `ref_row(q, slot,
    L)`: the reference row of request q that joined in `slot` in a call whose join run was L.  Returns per call (positions, join run, join phase ran)."""
    L_, V = spec.levels, spec.vocab_top
    p = Pass(L_, SLOTS, N, V)
    pos, who, joined_L = [-1] * SLOTS, [None] * SLOTS, [0] * SLOTS
    seeds, offs = [0] * SLOTS, [0] * SLOTS
    cond = cond_of(None, None)
    # an empty slot's rows of the table are never read: all ones over codes that would be seen if they were
    mask = np.ones((SLOTS, N), bool)
    kept = [torch.full((SLOTS, N) + ((4 ** l,) if l else ()), V - 1, dtype=torch.int64) for l in range(L_)]
    waiting, finished, calls, call = list(range(len(REQUESTS))), [], [], 0
    while waiting or any(q >= 0 for q in pos):
        joiners = []
        for s in range(SLOTS):
            if pos[s] < 0 and waiting and REQUESTS[waiting[0]]['join'] <= call and len(joiners) < max_joins:
                who[s] = waiting.pop(0)
                r = REQUESTS[who[s]]
                pos[s], seeds[s], offs[s] = 0, r['seed'], r['offset']
                cond = cond_of(cond, (s, who[s]))
                m, codes = request_table(spec, who[s])
                mask[s] = m
                for dst, src in zip(kept, codes):
                    dst[s] = src
                joiners.append(s)
        # the rule of the header, restated: the rows that join share the smallest leading run among them, clipped; the join phase runs on a text handle or where L > 0
        L = min(clipped(REQUESTS[who[s]]['run'], max_run) for s in joiners) if joiners else 0
        phase = bool(joiners) and (text or L > 0)
        for s in joiners:
            joined_L[s] = L
        calls.append((tuple(pos), L, phase))
        p.call(eng, None if cond is None else cond.clone(), pos, k, row_seeds=seeds, row_offsets=offs, keep=(torch.from_numpy(mask.copy()), [t.clone() for t in kept]), **kw)
        for s in range(SLOTS):
            if pos[s] < 0:
                assert p.untouched_from(s, 0), f'call {call}: the empty slot {s} was written'
                continue
            nxt = pos[s] + k + (L + 1 if phase and pos[s] == 0 else 0)
            assert p.untouched_from(s, min(nxt, N)), f'call {call}: slot {s} was written beyond position {min(nxt, N) - 1}'
            if nxt >= N:
                compare_from(p.row(s), ref_row(who[s], s, joined_L[s]), joined_L[s], f'call {call}: request {who[s]} in slot {s} (join run {joined_L[s]})')
                m, codes = request_table(spec, who[s])
                for got, want in zip(p.row(s)[0], codes):                    # kept cells are returned verbatim
                    assert torch.equal(got.cpu()[torch.from_numpy(m)], want[torch.from_numpy(m)])
                finished.append(who[s])
                p.clear(s)
                pos[s], who[s] = -1, None
                mask[s] = True
                for dst in kept:
                    dst[s] = V - 1
            else:
                pos[s] = nxt
        call += 1
        assert call < 40
    assert sorted(finished) == list(range(len(REQUESTS)))
    assert all(p.untouched_from(s, 0) for s in range(SLOTS)), 'an entry no request drew was written'
    return calls


def assert_schedule(calls, max_run, text=False):
    """The schedule did what the test is about."""
    assert any(len({q for q in ps if q >= 0}) > 1 for ps, _, _ in calls), 'no two rows at different positions shared a call'
    assert sum(ps.count(0) for ps, _, _ in calls) == len(REQUESTS) > SLOTS, 'no slot was reused'
    if max_run or text:
        assert any(ps.count(0) == 2 and phase for ps, _, phase in calls), 'no two joiners shared a join phase'
    if max_run:
        assert any(L == 2 and phase and any(q > 0 for q in ps) for ps, L, phase in calls), 'no run-2 joiner entered beside a row that is mid-image'
        assert any(0 in ps and L == 0 for ps, L, _ in calls), 'no row joined without a run'
    else:
        assert all(L == 0 for _, L, _ in calls)


def keep_reference(refs, spec, cache, kw, tag, cond_rows):
    """The plain keep= call of SLOTS rows that holds request q -- condition, key, mask and kept codes -- in EVERY slot (row s for slot s), on the engine whose
    max_prefix is the join run L; once per (request, L)."""
    def ref_row(q, s, L):
        if (tag, q, L) not in cache:
            r = REQUESTS[q]
            m, codes = request_table(spec, q)
            ref = refs[L]
            ref.set_persist(False)
            try:
                cache[(tag, q, L)] = plain(ref, spec.levels, SLOTS, cond_rows(q), N, row_seeds=[r['seed']] * SLOTS, row_offsets=[r['offset']] * SLOTS,
                                           keep=(torch.from_numpy(np.tile(m, (SLOTS, 1))), [c.unsqueeze(0).expand((SLOTS,) + tuple(c.shape)).contiguous() for c in codes]), **kw)
            finally:
                ref.set_persist(True)
        return R.row_of(cache[(tag, q, L)], s)
    return ref_row


# ------------------------------------------------------------------------------- 1. EXACT, staggered
_FIXTURES = {}
FIXTURES = R.FIXTURES


def fixture_case(name):
    """(spec, the rolling engine with max_prefix 2, the reference engines by max_prefix, sampler cut-offs, reference cache), built once per fixture."""
    if name not in _FIXTURES:
        fx = load(name + '.npz')
        spec, weights = stage2_from_fixture(fx)
        cut = R.fixture_case(name)[2]
        _FIXTURES[name] = (spec, engine_of(spec, weights, SLOTS, 2), {L: engine_of(spec, weights, SLOTS, L) for L in (0, 2)}, cut, {})
    return _FIXTURES[name]


def class_cond(spec):
    def cond_of(cond, join):
        if spec.cond != 1:
            return None
        cond = torch.zeros(SLOTS, dtype=torch.int64) if cond is None else cond
        if join is not None:
            cond[join[0]] = REQUESTS[join[1]]['cls'] % spec.n_classes
        return cond

    def cond_rows(q):
        return torch.full((SLOTS,), REQUESTS[q]['cls'] % spec.n_classes) if spec.cond == 1 else None
    return cond_of, cond_rows


@pytest.mark.parametrize('max_run', [0, 2])
@pytest.mark.parametrize('name', FIXTURES)
def test_a_staggered_pass_with_kept_cells_equals_the_plain_keep_calls_exact(name, max_run):
    spec, eng, refs, cut, cache = fixture_case(name)
    cond_of, cond_rows = class_cond(spec)
    eng.set_join_run(SLOTS, max_run)
    for graph in (False, True):
        kw = dict(precision=PRECISION_EXACT, use_graph=graph, **cut)
        ref_row = keep_reference(refs, spec, cache, kw, ('exact', graph), cond_rows)
        for k in (1, 2):
            assert_schedule(run_staggered(eng, spec, k, kw, max_run, ref_row, cond_of), max_run)
    eng.range_check()


# ------------------------------------------------------------------------------- 2. FAST and SPLIT, max_run = 0: every kept position is a step on both sides
@pytest.mark.parametrize('precision', ['fast', 'split'])
@pytest.mark.parametrize('name', ['g4_tiny_cls', 'g7_l3_tiny_cls'])
def test_a_staggered_pass_without_a_join_run_equals_the_plain_keep_calls(name, precision):
    spec, eng, refs, cut, cache = fixture_case(name)
    cond_of, cond_rows = class_cond(spec)
    eng.set_join_run(SLOTS, 0)
    for graph in (False, True):
        kw = dict(precision=PRECISIONS[precision], use_graph=graph, **cut)
        ref_row = keep_reference(refs, spec, cache, kw, (precision, graph), cond_rows)
        for k in (1, 2):
            assert_schedule(run_staggered(eng, spec, k, kw, 0, ref_row, cond_of), 0)
    eng.range_check()


# ------------------------------------------------------------------------------- 3. FAST and SPLIT: a join phase over the rows of a plain prefill
@pytest.mark.parametrize('precision', ['fast', 'split'])
def test_a_join_phase_over_all_rows_equals_the_plain_keep_call(precision):
    spec, eng, refs, cut, _ = fixture_case('g4_tiny_cls')
    eng.set_join_run(SLOTS, 2)
    who = (0, 1, 3)                                  # runs 2, 2, 3: the call's join run is 2
    cond = torch.tensor([REQUESTS[q]['cls'] % spec.n_classes for q in who])
    seeds, offs = [REQUESTS[q]['seed'] for q in who], [REQUESTS[q]['offset'] for q in who]
    tables = [request_table(spec, q) for q in who]
    keep = (torch.from_numpy(np.stack([t[0] for t in tables])), [torch.stack([t[1][l] for t in tables]) for l in range(spec.levels)])
    ref = refs[2]
    ref.set_persist(False)
    try:
        for graph in (False, True):
            kw = dict(precision=PRECISIONS[precision], use_graph=graph, row_seeds=seeds, row_offsets=offs, **cut)
            want = plain(ref, spec.levels, SLOTS, cond, N, keep=keep, **kw)
            p = Pass(spec.levels, SLOTS, N, spec.vocab_top)
            p.call(eng, cond, [0] * SLOTS, 1, keep=keep, **kw)              # the join phase draws position 2, the step position 3
            assert all(p.untouched_from(s, 4) for s in range(SLOTS)) and bool((p.codes[0][:, :4] >= 0).all())
            p.call(eng, cond, [4] * SLOTS, 2, keep=keep, **kw)
            for s in range(SLOTS):
                compare_from(p.row(s), R.row_of(want, s), 2, f'graph={graph}: slot {s}')
    finally:
        ref.set_persist(True)
    eng.range_check()


# ------------------------------------------------------------------------------- 4. FAST: a staggered join prefill against the oracle
def test_fast_join_prefill_teacher_forced_vs_oracle():
    """Fully kept rows (L = min(R, N - 1) = 3) that join one after another: logits_out[L:] of each against the oracle's teacher-forced logits, inside the bar of
    tests/test_gpu_prefix.py::test_fast_prefill_teacher_forced_vs_oracle for this model (0.15, the FAST gate of the text-prefill test of the same size); two runs
    bit-identical."""
    spec = Stage2Spec(embed_dim=128, n_layers=2, n_heads=2, n_layers_depth=1, vocab_top=256, vocab_bot=256, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    weights = synth.stage2_weights(spec, 501, 'fixture')
    Rr, V = 3, spec.vocab_top
    rng = np.random.default_rng(4100)
    cond = np.array([2, 7, 5])
    ft, fb = rng.integers(0, V, (SLOTS, N)), rng.integers(0, V, (SLOTS, N, 4))
    noise = synth.exp_noise(41, N, SLOTS, V)
    want = O.OracleStage2(spec, weights).sample(cond, SLOTS, N, noise, force_top=ft, force_bot=fb, return_logits=True)[2]      # [N, 5, SLOTS, V]
    eng = engine_of(spec, weights, SLOTS, Rr, join_run=(SLOTS, Rr))
    keep = (torch.ones((SLOTS, N), dtype=torch.bool), [torch.from_numpy(ft), torch.from_numpy(fb)])
    runs = []
    for graph in (False, True, True):
        p = Pass(2, SLOTS, N, V)
        kw = dict(precision=PRECISION_FAST, use_graph=graph, noise=torch.from_numpy(noise), keep=keep)
        p.call(eng, torch.from_numpy(cond), [0, -1, -1], 1, **kw)           # slot 0 joins alone: positions 0 .. 4
        p.call(eng, torch.from_numpy(cond), [5, 0, -1], 1, **kw)            # slot 1 joins beside its last step
        p.call(eng, torch.from_numpy(cond), [-1, 5, 0], 1, **kw)
        p.call(eng, torch.from_numpy(cond), [-1, -1, 5], 1, **kw)
        eng.range_check()
        lf = p.logits.cpu().numpy()
        assert np.isnan(lf[:Rr]).all() and np.isfinite(lf[Rr:]).all()
        assert torch.equal(p.codes[0].cpu(), keep[1][0]) and torch.equal(p.codes[1].cpu(), keep[1][1])
        gate(f'rolling_keep.fast_join_logits(tiny64,graph={graph})', np.abs(lf[Rr:] - want[Rr:]).max(), 0.15)
        runs.append(p.logits.clone())
    assert torch.equal(runs[1][Rr:], runs[2][Rr:]), 'two runs differ'


# ------------------------------------------------------------------------------- 5. text
_TEXT = {}


def text_case():
    if not _TEXT:
        spec, weights, (tk, tp, T) = _random_spec('tiny')
        prompts = torch.from_numpy(synth.text_ids(1800, len(REQUESTS), spec.ctx_len_txt, spec.vocab_txt))
        _TEXT['c'] = (spec, engine_of(spec, weights, SLOTS, 2, join_run=(2, 2)), {L: engine_of(spec, weights, SLOTS, L) for L in (0, 2)},
                      dict(top_k=tk, top_p=tp, temperature=T), prompts, {})
    return _TEXT['c']


def test_a_staggered_text_pass_with_kept_cells_equals_the_plain_unshared_keep_calls_exact():
    spec, eng, refs, cut, prompts, cache = text_case()
    assert eng.max_joins == 2 and eng.join_run == (2, 2)                     # on a text engine the call is also set_max_joins

    def cond_of(cond, join):
        cond = torch.zeros((SLOTS, spec.ctx_len_txt), dtype=torch.int64) if cond is None else cond
        if join is not None:
            cond[join[0]] = prompts[join[1]]
        return cond

    for graph in (False, True):
        kw = dict(precision=PRECISION_EXACT, use_graph=graph, **cut)
        ref_row = keep_reference(refs, spec, cache, kw, ('exact', graph), lambda q: prompts[q].expand(SLOTS, -1).contiguous())
        for k in (1, 2):
            assert_schedule(run_staggered(eng, spec, k, kw, 2, ref_row, cond_of, text=True, max_joins=2), 2, text=True)
    eng.range_check()


def test_a_guided_pair_with_a_shared_run_joins_a_text_pass():
    from hqtransformer_amd.text import pad_caption
    spec, eng, refs, cut, prompts, _ = text_case()
    L_, V, T = spec.levels, spec.vocab_top, spec.ctx_len_txt
    cond = torch.stack([prompts[0], pad_caption(1, T)[0], prompts[1]])               # the pair: a prompt and the all-PAD negative prompt
    seeds, offs, pairs = [81, 81, 83], [4, 4, 0], [(0, 1, (2.5, 1.5))]
    rng = np.random.default_rng(77)
    mask = scattered_mask(SLOTS, N, (2, 2, 0), ((0, (4,)), (1, (4,))))              # both rows of the pair keep the same cells
    kept = [torch.from_numpy(rng.integers(0, V, (SLOTS, N) + ((4 ** l,) if l else ()))) for l in range(L_)]
    for t in kept:
        t[1] = t[0]
    keep = (torch.from_numpy(mask), kept)
    for graph in (False, True):
        base = dict(precision=PRECISION_EXACT, use_graph=graph, row_seeds=seeds, row_offsets=offs, keep=keep, **cut)
        p = Pass(L_, SLOTS, N, V)
        p.call(eng, cond, [-1, -1, 0], 1, **base)                                # the third row joins alone, without a run: positions 0, 1
        assert p.untouched_from(2, 2) and p.untouched_from(0, 0) and p.untouched_from(1, 0)
        p.call(eng, cond, [0, 0, 2], 1, guidance=pairs, **base)                  # the pair joins with its run of 2 beside a row at 2: positions 0 .. 3
        assert p.untouched_from(0, 4) and p.untouched_from(1, 4) and p.untouched_from(2, 3)
        p.call(eng, cond, [4, 4, 3], N, guidance=pairs, **base)
        # the plain guided keep call that equals it prefills no run over ALL rows (row 2 has none): the pair's rows on the max_prefix = 2 engine need a call of their own
        want0 = plain(refs[0], L_, SLOTS, cond, N, guidance=pairs, **base)
        want2 = plain(refs[2], L_, 2, cond[:2], N, guidance=[(0, 1, (2.5, 1.5))], **{**base, 'row_seeds': seeds[:2], 'row_offsets': offs[:2],
                                                                                    'keep': (keep[0][:2], [t[:2] for t in kept])})
        compare_from(p.row(2), R.row_of(want0, 2), 0, f'graph={graph}: the row beside the pair')
        for s in (0, 1):
            compare_from(p.row(s), R.row_of(want2, s), 2, f'graph={graph}: row {s} of the pair')
        assert all(torch.equal(c[0], c[1]) for c in p.codes)
    eng.range_check()


# ------------------------------------------------------------------------------- 6. sizing and refusals
def test_sizing_refusals_and_the_pass_they_leave_intact():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    cut = R.fixture_case('g4_tiny_cls')[2]
    eng = engine_of(spec, weights, SLOTS, 2)
    L_, V, D = spec.levels, spec.vocab_top, spec.embed_dim
    cond = torch.tensor([1, 2, 3])
    base = dict(precision=PRECISION_EXACT, seed=9, **cut)
    keep = (torch.from_numpy(scattered_mask(SLOTS, N, (2, 2, 3))), [torch.zeros((SLOTS, N) + ((4 ** l,) if l else ()), dtype=torch.int64) for l in range(L_)])
    before = sample_any(eng, L_, SLOTS, cond, N, **base)
    # a handle that never opted in refuses, on the host surface and in the library, with the message it always had
    p = Pass(L_, SLOTS, N, V)
    with pytest.raises(ValueError, match='row_positions together with keep is not built'):
        p.call(eng, cond, [0, 0, -1], 1, keep=keep, **base)
    arr = (_lib.C.c_int32 * SLOTS)(0, 0, -1)
    _lib.check(eng.lib.hqt_set_row_positions(eng.h, SLOTS, arr, 1))
    raises(eng, INVALID, 'hqt_set_row_positions together with a staged keep table', lambda: sample_any(eng, L_, SLOTS, cond, N, out=p.codes, keep=keep, **base))
    # the workspace: nothing without a run; with one, K and V of [n_layers][J][1 + R][D] at 4 bytes and the gathered rows [max_batch][D], once
    ws = eng.lib.hqt_workspace_bytes(eng.h)
    eng.set_join_run(SLOTS, 0)
    assert eng.lib.hqt_workspace_bytes(eng.h) == ws
    eng.set_join_run(2, 2)
    grown = 2 * spec.n_layers * 2 * (1 + 2) * D * 4 + SLOTS * D * 4
    assert eng.lib.hqt_workspace_bytes(eng.h) == ws + grown
    eng.set_join_run(2, 1)                                                       # a smaller need reuses the staging
    eng.set_join_run(0, 0)                                                       # switching off frees nothing ...
    assert eng.lib.hqt_workspace_bytes(eng.h) == ws + grown
    with pytest.raises(ValueError, match='row_positions together with keep is not built'):
        p.call(eng, cond, [0, 0, -1], 1, keep=keep, **base)                      # ... and the combination is refused again
    eng.set_join_run(2, 2)
    assert eng.lib.hqt_workspace_bytes(eng.h) == ws + grown
    for bad, match in (((SLOTS + 1, 0), r'max_joins=4 outside \[0, max_batch=3\]'), ((-1, 0), 'max_joins=-1'), ((2, 3), r'max_run=3 outside \[0, max_prefix=2\]'), ((2, -1), 'max_run=-1')):
        raises(eng, INVALID, match, lambda: eng.set_join_run(*bad))
    assert eng.join_run == (2, 2)
    # the taking call's refusals name their cause and keep the pass
    p.call(eng, cond, [0, 0, -1], 1, keep=keep, **base)                          # a pass: rows 0 and 1 behind their run at position 4
    assert eng.lib.hqt_workspace_bytes(eng.h) == ws + grown                      # calls allocate nothing
    raises(eng, STATE, 'hqt_set_join_run: this handle holds a rolling pass', lambda: eng.set_join_run(2, 1))
    raises(eng, INVALID, '3 rows join at position 0 in this call, .*max_joins=2', lambda: Pass(L_, SLOTS, N, V).call(eng, cond, [0, 0, 0], 1, keep=keep, **base))
    dev_codes = [t.to(dev()) for t in keep[1]]

    def staged_keep(B):
        kp = (_lib.C.c_void_p * 3)(*[t.data_ptr() for t in dev_codes[:L_]], *([None] * (3 - L_)))
        m = np.ascontiguousarray(np.zeros((B, N), np.uint8))
        _lib.check(eng.lib.hqt_set_keep_mask(eng.h, B, N, m.ctypes.data_as(_lib.C.c_void_p), kp))

    arr2 = (_lib.C.c_int32 * SLOTS)(4, 4, -1)
    staged_keep(2)
    _lib.check(eng.lib.hqt_set_row_positions(eng.h, SLOTS, arr2, 1))
    raises(eng, INVALID, 'hqt_set_keep_mask staged a table of B=2, n_steps=6, this call has B=3, n_steps=6', lambda: sample_any(eng, L_, SLOTS, cond, N, out=p.codes, **base))
    raises(eng, INVALID, 'force_top together with a keep table is not built', lambda: _forced(eng, L_, cond, p, keep, base))
    arr0 = (_lib.C.c_int32 * SLOTS)(4, 4, -1)
    kp0 = (_lib.C.c_void_p * 3)(dev_codes[0].data_ptr(), None, None)          # a level pointer is NULL
    _lib.check(eng.lib.hqt_set_keep_mask(eng.h, SLOTS, N, np.zeros((SLOTS, N), np.uint8).ctypes.data_as(_lib.C.c_void_p), kp0))
    _lib.check(eng.lib.hqt_set_row_positions(eng.h, SLOTS, arr0, 1))
    raises(eng, INVALID, 'kept codes of level 1 are NULL', lambda: sample_any(eng, L_, SLOTS, cond, N, out=p.codes, **base))
    p.call(eng, cond, [4, 4, 0], 2, keep=keep, **base)                           # none of them ended the pass; row 2 joins with its run clipped to 2
    assert p.untouched_from(2, 5) and bool((p.codes[0][2, :5] >= 0).all()) and bool(torch.isnan(p.logprobs[2, :2]).all()) and bool(torch.isfinite(p.logprobs[2, 2:5]).all())
    assert bool((p.codes[0][:2] >= 0).all())
    # a text handle with three code levels prefills no run
    spec3 = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=64, vocab_bot=64, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                       n_classes=0, cond=2, embedding=0, levels=3)
    e3 = engine_of(spec3, synth.stage2_weights(spec3, 5, 'fixture'), 2)
    raises(e3, INVALID, 'max_run=1', lambda: e3.set_join_run(2, 1))              # (max_prefix is 0 there: text with three levels takes none)
    w3 = e3.lib.hqt_workspace_bytes(e3.h)
    e3.set_join_run(2, 0)
    assert e3.lib.hqt_workspace_bytes(e3.h) == w3 + 2 * spec3.n_layers * 2 * spec3.ctx_len_txt * spec3.embed_dim * 4 + 2 * spec3.embed_dim * 4 and e3.max_joins == 2
    e3.close()
    # a plain call after the pass draws what it drew before the handle ever rolled
    after = sample_any(eng, L_, SLOTS, cond, N, **base)
    assert all(torch.equal(a, b) for a, b in zip(before[:L_], after[:L_]))
    eng.range_check()
    eng.close()


def _forced(eng, L_, cond, p, keep, base):
    """force_* together with a table, staged by hand (the host surface refuses it first)."""
    arr = (_lib.C.c_int32 * SLOTS)(4, 4, -1)
    dev_codes = [t.to(dev()) for t in keep[1]]
    kp = (_lib.C.c_void_p * 3)(*[t.data_ptr() for t in dev_codes], *([None] * (3 - L_)))
    m = np.ascontiguousarray(keep[0].numpy().astype(np.uint8))
    _lib.check(eng.lib.hqt_set_keep_mask(eng.h, SLOTS, N, m.ctypes.data_as(_lib.C.c_void_p), kp))
    _lib.check(eng.lib.hqt_set_row_positions(eng.h, SLOTS, arr, 1))
    sample_any(eng, L_, SLOTS, cond, N, out=p.codes, force=(torch.zeros((SLOTS, N), dtype=torch.int64), None), **base)


# ------------------------------------------------------------------------------- 7. RollingSampler end to end
def test_rolling_sampler_returns_what_each_request_draws_alone_around_its_kept_cells():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    st2 = HQTransformerStage2(spec)
    st2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    st2 = st2.to('cuda')
    n = 6
    rng = np.random.default_rng(31)
    reqs = [dict(cond=(3 * i + 1) % spec.n_classes, seed=900 + 13 * i) for i in range(7)]
    runs, extras = (0, 2, 2, None, 4, 6, None), ((3,), (), (5,), None, (), (), None)     # None: a plain request
    tables = [None if r is None else (scattered_mask(1, n, (r,), ((0, e),))[0], [torch.from_numpy(rng.integers(0, spec.vocab_top, (n,))),
                                                                               torch.from_numpy(rng.integers(0, spec.vocab_top, (n, 4)))]) for r, e in zip(runs, extras)]
    os.environ['HQT_POISON_WORKSPACE'] = '1'         # (the model builds its engine when the sampler asks for one)
    try:
        rs = RollingSampler(st2, 3, n, precision='exact', join_run=2)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)

    def submit(i):
        kw = {} if tables[i] is None else dict(keep_mask=tables[i][0], kept_codes=tables[i][1])
        return rs.submit(reqs[i]['cond'], reqs[i]['seed'], **kw)
    tickets = [submit(i) for i in range(4)]
    done = rs.step() + rs.step(2)
    tickets += [submit(i) for i in range(4, 7)]
    done += rs.drain()
    assert sorted(d[0] for d in done) == tickets == list(range(7))
    for ticket, codes in done:
        r, kw = reqs[ticket], {}
        if tables[ticket] is not None:
            m, kc = tables[ticket]
            kw = dict(keep_mask=torch.from_numpy(m)[None], kept_codes=[c[None] for c in kc])
            for got, want in zip(codes, kc):
                assert torch.equal(got.cpu()[torch.from_numpy(m)], want[torch.from_numpy(m)]), f'request {ticket}: a kept cell was not returned verbatim'
        want = sampling_ihqgpt(st2, 1, r['cond'], max_seq_len=n, seed=r['seed'], precision='exact', is_tqdm=False, **kw)
        assert torch.equal(codes[0], want[0][0]) and torch.equal(codes[1], want[1][0]), f'request {ticket} differs from its own call'
    st2.range_check()


# ------------------------------------------------------------------------------- 8. complete_images / regenerate_region through a rolling pass
def test_complete_images_and_regenerate_region_through_a_rolling_pass_return_the_plain_calls_codes():
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import complete_images, decode_codes, regenerate_region
    model = ImageGPT2(load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'tiny-cls.yaml')), seed=5).to(dev())
    Rs = model.stage1.spec.resolution
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 3, Rs, Rs)).astype(np.float32)).to(dev())
    K = int(model.stage1.code_grids(x)[0].shape[-1])
    cut = dict(top_k_top=50, top_k_bot=50)
    os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        rs = RollingSampler(model.stage2, 2, K * K, precision='exact', join_run=16)       # two slots for three images: one waits for a slot
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    px, codes = complete_images(model, x, 3, cond=2, seed=11, rolling=rs, steps_per_call=7, **cut)       # 24 kept positions: 16 prefilled, 8 forced steps
    box = (0, 3, 1, 4)                                                                     # a box in the top rows: a leading run of one cell
    px2, codes2 = regenerate_region(model, x, box, cond=torch.tensor([2, 3, 4]), seed=12, rolling=rs, **cut)
    assert rs.live == 0 and not rs.queue
    model.stage2.range_check()
    with pytest.raises(ValueError, match='belong to the RollingSampler'):
        complete_images(model, x, 3, cond=2, seed=11, rolling=rs, use_fp16=False)
    with pytest.raises(ValueError, match='the pass has n=32 positions, the images have 64'):
        complete_images(model, x, 3, cond=2, rolling=RollingSampler(model.stage2, 2, 32, precision='exact', join_run=16))
    # (the plain calls last: they may rebuild the engine the pass lived on)
    wpx, want = complete_images(model, x, 3, cond=2, seed=11, use_fp16=False, **cut)
    wpx2, want2 = regenerate_region(model, x, box, cond=torch.tensor([2, 3, 4]), seed=12, use_fp16=False, **cut)
    assert all(torch.equal(a, b) for a, b in zip(codes, want)) and all(torch.equal(a, b) for a, b in zip(codes2, want2))
    assert torch.equal(px, decode_codes(model.stage1, codes)) and torch.equal(px, wpx) and torch.equal(px2, wpx2)
