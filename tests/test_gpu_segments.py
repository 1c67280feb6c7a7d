"""Paused passes on the GPU (hqt_set_segment, hqt_select_rows; segment=, Engine.select_rows, pipeline.SamplingSession, sample_best_of(prune=),
HQTransformerStage2.sampling_step).

A pass that stops behind a position and goes on later draws what ONE call draws: Philox keys are (seed, global row, absolute position, draw, chunk), and
between two positions a row's whole state is its body K/V rows, the step state and the codes in the caller's buffers.  The bars are therefore equalities:
codes, raw logits and log-probabilities of all segments together against the whole call, bit for bit, in every precision, eager and replayed.  Where the
rows of a paused pass are re-mapped (kv_gather_rows_kernel) row j must go on as the row it came from -- and every engine of those tests starts from a
NaN-poisoned workspace, so a cache row the gather did not write shows up."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.pipeline import SamplingSession, sample_best_of, sequence_logprob
from hqtransformer_amd.sampling import sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from tests.helpers import load, stage2_from_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 2e-4                 # the project's EXACT logit gate (tests/test_gpu_logprobs.py)
PRECISIONS = {'exact': PRECISION_EXACT, 'fast': PRECISION_FAST, 'split': PRECISION_SPLIT}
N = 6                            # positions of the segmented passes: the first N of every fixture's run


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def np_(t):
    return t.detach().cpu().numpy()


def engine_s2(spec, weights, max_batch, max_steps=None, max_prefix=0, poison=False):
    if poison:                       # every workspace buffer starts as NaN / -1: a row no kernel wrote shows up
        os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img, max_prefix=max_prefix)
        e.load(stage2=weights)
        e.finalize()
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    return e


def sample_any(eng, L, B, cond, n, force=None, **kw):
    """Engine.sample / sample3 behind one signature: returns the tuple they return (codes first); ``force``: one entry per level."""
    if L == 3:
        return eng.sample3(B, cond, n, force=force, **kw)
    force = force or (None, None)
    return eng.sample(B, cond, n, force_top=force[0], force_bot=force[1], **kw)


def whole(eng, L, B, cond, n, **kw):
    """One plain call -> (codes list, logits [n, draws, B, V], logprobs [B, n, draws])."""
    out = sample_any(eng, L, B, cond, n, return_logits=True, return_logprobs=True, **kw)
    return list(out[:L]), out[L], out[L + 1]


def segmented(eng, L, B, cond, n, plan, V, per_segment=None, **kw):
    """The pass as the segments of ``plan`` into poisoned full-length buffers (codes -1, logits and log-probabilities NaN); ``per_segment[i]``: keywords of
    segment i in place of those of ``kw``."""
    draws = (4 ** L - 1) // 3
    outs = [torch.full((B, n) + ((4 ** l,) if l else ()), -1, dtype=torch.int64, device=dev()) for l in range(L)]
    lg = torch.full((n, draws, B, V), float('nan'), dtype=torch.float32, device=dev())
    lp = torch.full((B, n, draws), float('nan'), dtype=torch.float32, device=dev())
    for i, seg in enumerate(plan):
        sample_any(eng, L, B, cond, n, out=outs, segment=seg, logits_out=lg, logprobs_out=lp, **{**kw, **((per_segment or {}).get(i, {}))})
    return outs, lg, lp


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def plans(n):
    return {'every position': [(t, t + 1) for t in range(n)], 'first | rest': [(0, 1), (1, n)], 'all but one | last': [(0, n - 1), (n - 1, n)]}


# ------------------------------------------------------------------------------- 1. a segmented pass equals the whole call
def _l3_noise(seed, n, B, V):
    return np.maximum(np.random.default_rng([seed, 0x9e3779b9]).standard_exponential((n, 21, B, V), dtype=np.float32), np.float32(1e-30))


_FIXTURES = {}


def fixture_case(name):
    """(fixture, spec, engine, levels, B, cond, fixture noise of the first N positions, sampler settings), built once per fixture and shared."""
    if name not in _FIXTURES:
        fx = load(name + '.npz')
        spec, weights = stage2_from_fixture(fx)
        B, L = int(fx['B']), spec.levels
        full = int(fx['n_steps'])
        if spec.cond == 2:
            cond = torch.from_numpy(synth.text_ids(int(fx['text_seed']), B, spec.ctx_len_txt, spec.vocab_txt))
        else:
            cond = torch.full((B,), int(fx['cond']) if 'cond' in fx.files else 7)
        noise = (_l3_noise if L == 3 else synth.exp_noise)(int(fx['noise_seed']), full, B, spec.vocab_top)[:N].copy()
        tk, tp, T = json.loads(str(fx['settings']))[-1] if 'settings' in fx.files else ((None, None), (None, None), (1.0, 1.0))
        eng = engine_s2(spec, weights, B, poison=True)
        _FIXTURES[name] = (fx, spec, eng, L, B, cond, torch.from_numpy(noise), dict(top_k=tk, top_p=tp, temperature=T))
    return _FIXTURES[name]


FIXTURES = ['g4_tiny_cls', 'g3_tiny_txt', 'g7_l3_tiny_cls', 'g7_l3_tiny_cls_top2mid2bot', 'g13_tiny_cls_bidirectional']


@pytest.mark.parametrize('precision', sorted(PRECISIONS))
@pytest.mark.parametrize('name', FIXTURES)
def test_segments_equal_the_whole_call_bit_for_bit(name, precision):
    fx, spec, eng, L, B, cond, noise, cut = fixture_case(name)
    prec = PRECISIONS[precision]
    for graph in (False, True):
        for source in ('fixture noise', 'philox'):
            kw = dict(precision=prec, use_graph=graph, **cut, **(dict(noise=noise) if source == 'fixture noise' else dict(seed=404)))
            want = whole(eng, L, B, cond, N, **kw)
            if name == 'g4_tiny_cls' and precision == 'exact' and source == 'fixture noise':      # these are the reference's codes
                si = len(json.loads(str(fx['settings']))) - 1
                assert (np_(want[0][0]) == fx[f'codes_top_{si}'][:, :N]).all() and (np_(want[0][1]) == fx[f'codes_bot_{si}'][:, :N]).all()
            assert bool(torch.isfinite(want[1]).all()) and bool(torch.isfinite(want[2]).all())
            for what, plan in plans(N).items():
                got = segmented(eng, L, B, cond, N, plan, spec.vocab_top, **kw)
                assert same(got, want), f'{name} {precision} graph={graph} {source}, {what}: the segmented pass differs from the whole call'
    eng.range_check()


def test_segments_on_the_launch_chain_equal_the_whole_call():
    """FAST with up to 64 rows takes the persistent launch by default (the cases above); HQT_SWITCH_PERSIST = 0: the launch chain."""
    fx, spec, eng, L, B, cond, noise, cut = fixture_case('g4_tiny_cls')
    eng.set_persist(False)
    try:
        for graph in (False, True):
            kw = dict(precision=PRECISION_FAST, use_graph=graph, seed=405, **cut)
            want = whole(eng, L, B, cond, N, **kw)
            for what, plan in plans(N).items():
                assert same(segmented(eng, L, B, cond, N, plan, spec.vocab_top, **kw), want), f'launch chain, graph={graph}, {what}'
    finally:
        eng.set_persist(True)
    eng.range_check()


# ------------------------------------------------------------------------------- 2. settings that change between segments
@pytest.mark.parametrize('precision', ['exact', 'fast'])
def test_settings_may_change_between_segments(precision):
    fx, spec, eng, L, B, cond, noise, cut = fixture_case('g4_tiny_cls')
    prec, k = PRECISIONS[precision], 2
    s1 = dict(top_k=(64, 32), top_p=(0.9, 0.8), temperature=(0.95, 0.9))
    rows = [((1.3, 0.7), (20 + 3 * b, 11), (0.6, 0.95)) for b in range(B)]             # S2: another temperature, top-k and top-p, as a row table
    s2 = dict(row_samplers=rows)
    for graph in (False, True):
        base = dict(precision=prec, use_graph=graph, seed=77)
        a = whole(eng, L, B, cond, N, **base, **s1)
        r = segmented(eng, L, B, cond, N, [(0, k), (k, N)], spec.vocab_top, per_segment={0: s1, 1: s2}, **base)
        for x, y in zip(r[0], a[0]):
            assert torch.equal(x[:, :k], y[:, :k])
        assert torch.equal(r[1][:k], a[1][:k]) and torch.equal(r[2][:, :k], a[2][:, :k])
        # a whole call under S2 that is forced to the segmented result still writes its own draws: from k on they are the segmented pass's
        w = whole(eng, L, B, cond, N, force=[c.clone() for c in r[0]], **base, **s2)
        for x, y in zip(w[0], r[0]):
            assert torch.equal(x[:, k:], y[:, k:]), f'{precision} graph={graph}: positions from {k} on are not the draws of S2'
        assert torch.equal(w[1][k:], r[1][k:]) and torch.equal(w[2][:, k:], r[2][:, k:])
        assert not all(torch.equal(x[:, k:], y[:, k:]) for x, y in zip(r[0], a[0])), 'S2 drew what S1 draws: the change shows nothing'
    eng.range_check()


# ------------------------------------------------------------------------------- 3. select_rows
MAPPINGS = {'identity': [0, 1, 2, 3, 4], 'swap': [1, 0, 2, 3, 4], 'rotation': [1, 2, 3, 4, 0], 'all from row 0': [0, 0, 0, 0, 0], '5 -> 3': [4, 0, 2],
            '5 -> 7 with duplicates': [3, 3, 0, 4, 1, 1, 2]}
_GATHER = {}


def gather_engine(D, text):
    """max_batch 7, two body layers, on a poisoned workspace: cache rows are 2 D bytes (FAST) or 4 D (EXACT), i.e. 160 / 320 at D = 80, 512 / 1024 at 256."""
    if (D, text) not in _GATHER:
        spec = Stage2Spec(embed_dim=D, n_layers=2, n_heads=5 if D == 80 else 4, n_layers_depth=1, vocab_top=256, vocab_bot=256, vocab_txt=64,
                          ctx_len_img=16, ctx_len_txt=6, n_classes=10, cond=2 if text else 1, embedding=0)
        _GATHER[(D, text)] = (spec, engine_s2(spec, synth.stage2_weights(spec, 311, 'fixture'), 7, max_steps=5, poison=True))
    return _GATHER[(D, text)]


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('text', [False, True], ids=['class', 'text'])
@pytest.mark.parametrize('D', [80, 256])
def test_selected_rows_go_on_as_the_rows_they_came_from(D, text, precision):
    spec, eng = gather_engine(D, text)
    prec, B, n = PRECISIONS[precision], 5, 5
    cond = torch.from_numpy(synth.text_ids(312, B, spec.ctx_len_txt, spec.vocab_txt)) if text else torch.tensor([3, 1, 4, 1, 5])
    seeds, offs = [900 + 7 * b for b in range(B)], [10 * b + 1 for b in range(B)]
    cut = dict(top_k=(100, 50), top_p=(None, None), temperature=(1.0, 0.9))
    a_codes, _, _ = whole(eng, 2, B, cond, n, precision=prec, row_seeds=seeds, row_offsets=offs, **cut)
    assert len({tuple(np_(a_codes[1])[b].reshape(-1).tolist()) for b in range(B)}) == B, 'rows of the whole call coincide: a wrong row would not show'
    for p in (1, n - 1):
        for what, rows_from in MAPPINGS.items():
            idx = torch.tensor(rows_from, device=dev())
            # ---- the rows keep their keys: row j goes on as row rows_from[j] of the whole call
            outs = [torch.full_like(c, -1) for c in a_codes]
            eng.sample(B, cond, n, precision=prec, row_seeds=seeds, row_offsets=offs, out=outs, segment=(0, p), **cut)
            assert eng.select_rows(rows_from, B) == len(rows_from)
            outs = [c.index_select(0, idx) for c in outs]
            keys = dict(row_seeds=[seeds[r] for r in rows_from], row_offsets=[offs[r] for r in rows_from])
            eng.sample(len(rows_from), cond[rows_from], n, precision=prec, out=outs, segment=(p, n), **keys, **cut)
            for got, want in zip(outs, a_codes):
                assert torch.equal(got, want.index_select(0, idx)), f'D={D} text={text} {precision}, pause at {p}, {what}: a row does not go on as its source row'
            if precision != 'exact':
                continue
            # ---- new keys (EXACT: codes do not depend on the row count of a pass): the plain whole call forced to the source row's codes below the
            # pause -- and, from there on, to what the continuation drew -- carries the new key and draws the same codes
            outs = [torch.full_like(c, -1) for c in a_codes]
            eng.sample(B, cond, n, precision=prec, row_seeds=seeds, row_offsets=offs, out=outs, segment=(0, p), **cut)
            eng.select_rows(rows_from)
            outs = [c.index_select(0, idx) for c in outs]
            fresh = dict(row_seeds=[5000 + j for j in range(len(rows_from))], row_offsets=[j for j in range(len(rows_from))])
            eng.sample(len(rows_from), cond[rows_from], n, precision=prec, out=outs, segment=(p, n), **fresh, **cut)
            w = eng.sample(len(rows_from), cond[rows_from], n, precision=prec, force_top=outs[0].clone(), force_bot=outs[1].clone(), **fresh, **cut)
            for got, want in zip(outs, w[:2]):
                assert torch.equal(got[:, p:], want[:, p:]), f'D={D} text={text}, pause at {p}, {what}: forked rows with new keys differ from the forced whole call'
                assert torch.equal(got[:, :p], a_codes[0 if got.dim() == 2 else 1].index_select(0, idx)[:, :p])
    eng.range_check()


# ------------------------------------------------------------------------------- 4. state and refusals
def test_state_and_refusals():
    fx, spec, weights = (lambda fx: (fx,) + stage2_from_fixture(fx))(load('g4_tiny_cls.npz'))
    eng = engine_s2(spec, weights, 4, max_prefix=3)
    B, n = 4, 6
    cond = torch.full((B,), 7)
    kw = dict(precision=PRECISION_EXACT, seed=3)
    outs = [torch.zeros((B, n), dtype=torch.int64, device=dev()), torch.zeros((B, n, 4), dtype=torch.int64, device=dev())]

    def refused(code, match, fn):
        with pytest.raises(_lib.HqtError, match=match) as e:
            fn()
        assert e.value.code == code, f'{e.value}: expected status {code}'

    def stage(start, stop):
        _lib.check(eng.lib.hqt_set_segment(eng.h, start, stop))

    cont = lambda **over: eng.sample(**{**dict(batch=B, cond=cond, n_steps=n, out=outs, segment=(2, n), **kw), **over})      # noqa: E731
    rows = np.array([0, 1, 2, 3], np.int32)
    select = lambda table, count=None: _lib.check(eng.lib.hqt_select_rows(eng.h, len(table) if count is None else count,      # noqa: E731
                                                                          table.ctypes.data, None))
    assert eng.lib.hqt_set_segment(None, 0, 1) == -1
    refused(-3, 'holds none', cont)                                                  # a continuation without a paused pass
    refused(-3, 'no paused pass', lambda: select(rows))
    eng.sample(B, cond, n, out=outs, segment=(0, 2), **kw)
    refused(-3, r'B=4, this call has B=3', lambda: cont(batch=3, cond=cond[:3], out=[o[:3].contiguous() for o in outs]))
    refused(-3, r'n_steps=6, this call has n_steps=5', lambda: cont(n_steps=5, out=[o[:, :5].contiguous() for o in outs], segment=(2, 5)))
    refused(-3, 'precision 0, this call asks for precision 1', lambda: cont(precision=PRECISION_FAST))
    refused(-3, 'stands at position 2, this segment has start=3', lambda: cont(segment=(3, n)))
    refused(-1, r'rows_from\[1\]=4 outside', lambda: select(np.array([0, 4], np.int32)))
    refused(-1, 'B_new=5 outside', lambda: select(np.zeros(5, np.int32)))
    refused(-1, 'B_new=0 outside', lambda: select(rows, 0))
    # bounds of a segment, a staged keep table, a prefix entry point: HQT_ERR_INVALID, checked at the taking call (the host checks are bypassed)
    for start, stop in ((2, 2), (-1, 2), (2, n + 1)):
        stage(start, stop)
        refused(-1, 'a segment needs', lambda: eng.sample(B, cond, n, out=outs, **kw))
    stage(2, n)
    refused(-1, 'keep table', lambda: eng.sample(B, cond, n, keep=(np.ones((B, n), bool), [o.clone() for o in outs]), **kw))
    stage(0, 2)
    refused(-1, 'prefix entry point', lambda: eng.sample(B, cond, n, prefix=[o[:, :2].contiguous() for o in outs], **kw))
    # ... none of which ended the paused pass, and each of which took its segment with it: the pass goes on and equals the whole call
    cont()
    want = eng.sample(B, cond, n, **kw)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])
    refused(-3, 'holds none', cont)                                                  # finished: the record is cleared
    # a plain call, and hqt_score, end a paused pass
    for ender in (lambda: eng.sample(B, cond, n, **kw), lambda: eng.score(B, cond, [want[0][:, :3].contiguous(), want[1][:, :3].contiguous()], precision=PRECISION_EXACT)):
        eng.sample(B, cond, n, out=outs, segment=(0, 2), **kw)
        ender()
        refused(-3, 'holds none', cont)
    # a staged segment is cleared by a failing call: the next plain call runs all positions, and reproduces the reference's fixture
    stage(0, 1)
    refused(-1, 'temperatures', lambda: eng.sample(B, cond, n, temperature=(0.0, 1.0), **kw))
    full = int(fx['n_steps'])
    noise = torch.from_numpy(synth.exp_noise(int(fx['noise_seed']), full, B, spec.vocab_top))
    tk, tp, T = json.loads(str(fx['settings']))[1]
    ct, cb = eng.sample(B, cond, full, precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=noise)
    assert (np_(ct) == fx['codes_top_1']).all() and (np_(cb) == fx['codes_bot_1']).all()


# ------------------------------------------------------------------------------- 5. pruned best-of, 6. the sampling_step shim
@pytest.fixture(scope='module')
def tiny_model():
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to('cuda').eval()


def test_pruned_best_of_keeps_the_unpruned_calls_candidates(tiny_model):
    st2 = tiny_model.stage2
    G, C, K, n = 2, 4, 1, 6
    classes = torch.tensor([5, 9])
    kw = dict(use_fp16=False, max_seq_len=n, seed=81, top_k_top=100, top_k_bot=100, softmax_temperature=[1.0, 0.9])
    codes, scores = sample_best_of(st2, classes, C, K, prune=[(2, 2)], **kw)
    ct, cb, lg, lp = st2.engine(G * C, n).sample(G * C, classes.repeat_interleave(C), n, precision=PRECISION_EXACT, top_k=(100, 100), temperature=(1.0, 0.9), seed=81,
                                                 return_logits=True, return_logprobs=True)
    torch.cuda.synchronize()
    lp64 = np_(lp).astype(np.float64)
    early, sums = lp64[:, :2].sum(axis=(1, 2)).reshape(G, C), lp64.sum(axis=(1, 2)).reshape(G, C)
    assert len(set(sums.reshape(-1).tolist())) > 1 and len(set(early.reshape(-1).tolist())) > 1, 'every candidate scored the same: the ranking shows nothing'
    alive = np.sort(np.argsort(-early, axis=1, kind='stable')[:, :2], axis=1)            # the two survivors of every group at position 2, by candidate index
    best = np.take_along_axis(alive, np.argsort(-np.take_along_axis(sums, alive, 1), axis=1, kind='stable')[:, :K], 1)
    flat = (best + np.arange(G)[:, None] * C).reshape(-1)
    assert (np_(codes[0]) == np_(ct)[flat]).all() and (np_(codes[1]) == np_(cb)[flat]).all(), 'survivors drew other codes than in the unpruned call'
    # per entry 2 LOGIT_TOL + tol(row) (tests/test_gpu_logprobs.py: a log-softmax moves at most twice the sup-norm change of its row), summed over the entries
    tol = 2.0 ** -24 * (32.0 + 4.0 * np.abs(np_(lg)).max(-1)).transpose(2, 0, 1)         # [B, n, draws]
    bound = (2.0 * LOGIT_TOL + tol).sum(axis=(1, 2))[flat].reshape(G, K)
    got = np_(scores)
    err = np.abs(got - np.take_along_axis(sums, best, 1))
    print(f'pruned vs unpruned scores: largest error {err.max():.3e}, bound {bound.min():.3e}')
    assert scores.dtype == torch.float64 and got.shape == (G, K) and (err <= bound).all()
    # keep = 2: both survivors of every group come back, best first, with the unpruned call's codes and scores
    codes2, scores2 = sample_best_of(st2, classes, C, 2, prune=[(2, 2)], **kw)
    order = np.take_along_axis(alive, np.argsort(-np.take_along_axis(sums, alive, 1), axis=1, kind='stable'), 1)
    flat2 = (order + np.arange(G)[:, None] * C).reshape(-1)
    got2 = np_(scores2)
    assert got2.shape == (G, 2) and (np.diff(got2, axis=1) <= 0).all(), 'scores must come best first'
    assert (np_(codes2[0]) == np_(ct)[flat2]).all() and (np_(codes2[1]) == np_(cb)[flat2]).all()
    bound2 = (2.0 * LOGIT_TOL + tol).sum(axis=(1, 2))[flat2].reshape(G, 2)
    assert (np.abs(got2 - np.take_along_axis(sums, order, 1)) <= bound2).all() and (got2[:, :1] == got).all()


def test_sampling_step_loop_returns_the_codes_of_sampling_ihqgpt(tiny_model):
    st2 = tiny_model.stage2
    B, n = 3, 5
    cond = torch.tensor([417, 3, 99])
    kw = dict(use_fp16=False, top_k_top=50, top_k_bot=20, softmax_temperature=[0.8, 1.2])
    want = sampling_ihqgpt(st2, num_candidates=B, cond=cond, is_tqdm=False, max_seq_len=n, seed=31, **kw)
    codes_top, codes_bot, past = None, None, None
    for cnt in range(n):                                                            # the loop of hqvae/utils/sampling.py:194-235
        _top = None if codes_top is None else codes_top.clone().detach()[:, cnt - 1:cnt]
        _bot = None if codes_bot is None else codes_bot.clone().detach()[:, cnt - 1, :]
        code_top, code_bot, present = st2.sampling_step(sos=cond, codes_t=_top, codes_b=_bot, pos_codes=None, past=past, model_stage1=None,
                                                        given_top_code=None, seed=31, max_seq_len=n, **kw)
        present = torch.stack(present).clone().detach()
        past = [present] if past is None else past + [present]
        codes_top = code_top if codes_top is None else torch.cat([codes_top, code_top], axis=1)
        codes_bot = code_bot if codes_bot is None else torch.cat([codes_bot, code_bot], axis=1)
    torch.cuda.synchronize()
    assert torch.equal(codes_top, want[0]) and torch.equal(codes_bot, want[1])
    # given_top_code at every position: the given code is fed forward and returned (hierarchical_ar.py:768-774); the bottom codes are those of
    # sampling_ihqgpt with the same given codes, whose codes_top holds the discarded draws
    given = torch.tensor([[11, 22, 33, 44, 55], [5, 4, 3, 2, 1], [500, 400, 300, 200, 100]])
    want_g = sampling_ihqgpt(st2, num_candidates=B, cond=cond, is_tqdm=False, max_seq_len=n, seed=31, given_top_code=given, **kw)
    codes_top, codes_bot, past = None, None, None
    for cnt in range(n):
        _top = None if codes_top is None else codes_top.clone().detach()[:, cnt - 1:cnt]
        _bot = None if codes_bot is None else codes_bot.clone().detach()[:, cnt - 1, :]
        code_top, code_bot, present = st2.sampling_step(sos=cond, codes_t=_top, codes_b=_bot, pos_codes=None, past=past, given_top_code=given[:, cnt],
                                                        seed=31, max_seq_len=n, **kw)
        present = torch.stack(present).clone().detach()
        past = [present] if past is None else past + [present]
        codes_top = code_top if codes_top is None else torch.cat([codes_top, code_top], axis=1)
        codes_bot = code_bot if codes_bot is None else torch.cat([codes_bot, code_bot], axis=1)
    torch.cuda.synchronize()
    assert torch.equal(codes_top.cpu(), given) and torch.equal(codes_bot, want_g[1])
    assert not torch.equal(want_g[1], want[1]), 'the given codes changed nothing: the comparison shows nothing'
    # a session is the same pass with its state in the open
    s = SamplingSession(st2, B, cond, n, seed=31, return_logprobs=True, **kw)
    s.advance(2)
    assert s.position == 2 and not s.done
    got = s.finish()
    assert s.done and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(torch.isfinite(sequence_logprob(s.logprobs)).all())
