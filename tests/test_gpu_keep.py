"""Kept positions (hqt_set_keep_mask): any (row, position) cells of the code grid are held fixed and the rest is drawn around them -- the
kept codes are scattered into the handle's code buffers (copy_kept_kernel), the sampler kernels leave those entries alone, the leading run
all rows share goes through the prefix prefill.

Bars: EXACT / SPLIT codes bit for bit against the unchanged oracle by iteration (tests/keep_ref.py) on seeds whose oracle-only margin is recorded
below (>= 1.00009, asserted to 1e-6 relative, no position excluded), logits of positions >= L within the project's 2e-4, on a NaN-poisoned
workspace; a uniform mask against the ``prefix=`` call, and a replay through plain ``force_*``, bit for bit (the same kernels at the same B).
The recorded tiny case with leading runs (2, 3, 6, 3, 11) has L = 3, not 2: its extra cell (row 0, position 2) extends row 0's run; L = 2 is
what it gets from an engine with max_prefix = 2 (the clip)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine, keep_leading_run
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O
from tests import keep_ref as K
from tests.helpers import load, stage2_from_fixture

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_SET = ((None, 64), (None, 0.9), (1.0, 0.9))


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_prefix, poison=False):
    if poison:                       # every workspace buffer starts as NaN / -1 / mask 0xFF: a read of something no kernel wrote shows up
        os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        e = Engine(spec, None, dev(), max_batch, spec.ctx_len_img, max_prefix=max_prefix)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    e.load(stage2=weights)
    e.finalize()
    return e


def np_(t):
    return t.detach().cpu().numpy()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def l3_noise(seed, n, B, V):
    return np.maximum(np.random.default_rng([seed, 0x9e3779b9]).standard_exponential((n, 21, B, V), dtype=np.float32), np.float32(1e-30))


# ------------------------------------------------------------------------------- 1. against the oracle
# name -> (model, leading runs, recorded oracle margin): seeds picked on the CPU with the oracle alone (tests/keep_ref.py: oracle_keep); the margin is the
# oracle's smallest winner / runner-up ratio of p / q over ALL draws.  'head*': the ImageNet head geometry of test_gpu_prefix.py, B = 64, n = 6, row b
# leading with (lead +) b % 4 kept positions and every third row keeping position 4 as well.
ORACLE_CASES = {'tiny': ('tiny', K.KEEP_RUNS, 1.0049023628234863),
                'tiny-lead': ('tiny', K.KEEP_RUNS_L2, 1.0049023628234863),
                'head': ('head', 0, 1.0002846717834473),
                'head-lead': ('head', 1, 1.000744342803955)}
HEAD_SEED = 800


def _head_spec():
    spec = Stage2Spec(embed_dim=1536, n_layers=1, n_heads=24, n_layers_depth=1, vocab_top=512, vocab_bot=512, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    return spec, synth.stage2_weights(spec, 91, 'fixture')


@functools.lru_cache(maxsize=None)
def _oracle_case(case):
    """(spec, weights, settings, cond, mask, kept, noise, expected codes_top, codes_bot, logits, margin): the oracle's answer, computed once."""
    kind, runs, _ = ORACLE_CASES[case]
    if kind == 'tiny':
        spec, weights = stage2_from_fixture(load('g4_tiny_cls.npz'))
        sets = K.TINY_SET
        cond, mask, kept, noise = K.tiny_keep_case(spec, runs)
    else:
        spec, weights = _head_spec()
        sets, B, n = HEAD_SET, 64, 6
        rng = np.random.default_rng([HEAD_SEED, 0x6b65])
        cond = (np.arange(B) % spec.n_classes).astype(np.int64)
        kept = (rng.integers(0, spec.vocab_top, (B, n)), rng.integers(0, spec.vocab_top, (B, n, 4)))
        mask = K.scattered_mask(B, n, [runs + b % 4 for b in range(B)], [(b, (4,)) for b in range(0, B, 3)])
        noise = synth.exp_noise(HEAD_SEED, n, B, spec.vocab_top)
    B, n = mask.shape
    want = K.oracle_keep(O.OracleStage2(spec, weights), cond, B, n, noise, mask, kept, *sets)
    return (spec, weights, sets, cond, mask, kept, noise) + want


@pytest.mark.parametrize('max_prefix', [0, 2, 11])
@pytest.mark.parametrize('case', sorted(ORACLE_CASES))
def test_kept_positions_vs_oracle(case, max_prefix):
    spec, weights, (tk, tp, T), cond, mask, kept, noise, wt, wb, wl, margin = _oracle_case(case)
    recorded = ORACLE_CASES[case][2]
    print(f'{case}: oracle margin {margin!r} (recorded {recorded!r})')
    assert margin >= 1.00009 and abs(margin - recorded) <= 1e-6 * recorded
    B, n = mask.shape
    max_prefix = min(max_prefix, n - 1)
    L = K.leading_run(mask, max_prefix)
    assert L == keep_leading_run(mask, max_prefix) == {'tiny': 0, 'tiny-lead': min(3, max_prefix), 'head': 0, 'head-lead': min(1, max_prefix)}[case]
    assert (wt[mask] == kept[0][mask]).all() and (wb[mask] == kept[1][mask]).all()
    eng = engine_s2(spec, weights, B, max_prefix=max_prefix, poison=True)
    for prec in (PRECISION_EXACT, PRECISION_SPLIT):
        for graph in (False, True):
            ct, cb, lg = eng.sample(B, t_(cond), n, precision=prec, top_k=tk, top_p=tp, temperature=T, noise=t_(noise), return_logits=True,
                                    use_graph=graph, keep=(mask, [t_(kept[0]), t_(kept[1])]))
            eng.range_check()
            assert (np_(ct) == wt).all() and (np_(cb) == wb).all(), f'precision {prec} graph={graph}: codes differ from the oracle'
            err = np.abs(np_(lg)[L:] - wl[L:]).max()
            print(f'{case}: max_prefix {max_prefix} (L = {L}) precision {prec} graph={graph} logit error {err}')
            assert err <= LOGIT_TOL


# ------------------------------------------------------------------------------- 2. a uniform mask is a prefix; a replay through plain forcing
@pytest.fixture(scope='module')
def tiny():
    spec, weights = stage2_from_fixture(load('g4_tiny_cls.npz'))
    return spec, weights, engine_s2(spec, weights, 10, max_prefix=63), engine_s2(spec, weights, 10, max_prefix=0)


def _random_codes(spec, B, n, seed, levels=2):
    rng = np.random.default_rng(seed)
    return [t_(rng.integers(0, spec.vocab_top, (B, n) + ((4 ** l,) if l else ()))) for l in range(levels)]


@pytest.mark.parametrize('prec', [PRECISION_EXACT, PRECISION_FAST])
def test_a_uniform_mask_is_the_prefix_call_bit_for_bit(tiny, prec):
    spec, weights, eng, _ = tiny
    B, n, P = 5, 24, 9
    cond = torch.arange(B) % spec.n_classes
    codes = _random_codes(spec, B, n, 77)
    mask = np.zeros((B, n), bool)
    mask[:, :P] = True
    kw = dict(precision=prec, seed=4321, top_k=(100, 60), return_logits=True, return_logprobs=True)
    for graph in (False, True):
        want = eng.sample(B, cond, n, prefix=[c[:, :P] for c in codes], use_graph=graph, **kw)
        got = eng.sample(B, cond, n, keep=(mask, codes), use_graph=graph, **kw)
        eng.range_check()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(got[0][:, :P].cpu(), codes[0][:, :P]) and torch.equal(got[1][:, :P].cpu(), codes[1][:, :P])
        assert torch.equal(got[2], want[2]), 'logits differ from the prefix call'
        assert bool(torch.isnan(got[3][:, :P]).all()) and torch.equal(got[3][:, P:], want[3][:, P:])


def _replay_model(kind):
    if kind == 'l3':
        return stage2_from_fixture(load('g7_l3_tiny_cls.npz'))
    if kind == 'head':               # D = 1536: FAST passes of up to 64 rows on a root handle run a position as the persistent launch
        return _head_spec()
    if kind == 'plain1024':          # a vocabulary the register-resident FAST sampler takes (1024 <= V <= 8192, no cut-off)
        spec = Stage2Spec(embed_dim=128, n_layers=2, n_heads=2, n_layers_depth=1, vocab_top=1024, vocab_bot=1024, vocab_txt=64,
                          ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
        return spec, synth.stage2_weights(spec, 507, 'fixture')
    return stage2_from_fixture(load('g4_tiny_cls.npz'))


@pytest.mark.parametrize('kind', ['l2', 'l3', 'plain1024', 'head'])
@pytest.mark.parametrize('prec', [PRECISION_EXACT, PRECISION_SPLIT, PRECISION_FAST])
def test_replay_through_plain_forcing_redraws_every_code_that_was_not_kept(kind, prec):
    """max_prefix = 0: every position is a decode step.  The result, fed back through plain force_*, is redrawn at every position that was not kept;
    logits and log-probabilities (of the fed-forward code: at a kept position the kept one) are bit-identical everywhere."""
    spec, weights = _replay_model(kind)
    levels = spec.levels
    B, n = 5, 12
    eng = engine_s2(spec, weights, B, max_prefix=0, poison=True)
    fn = eng.sample3 if levels == 3 else eng.sample
    cond = torch.arange(B) % spec.n_classes
    codes = _random_codes(spec, B, n, 78, levels)
    mask = K.scattered_mask(B, n, K.KEEP_RUNS, K.KEEP_EXTRA)
    kw = dict(precision=prec, seed=99, return_logits=True, return_logprobs=True)
    if kind == 'plain1024':
        kw.update(temperature=(1.0, 0.9))
    else:
        kw.update(dict(top_k=(50, 20, 20), top_p=(None, 0.9, None), temperature=(1.0, 0.8, 0.9)) if levels == 3 else dict(top_k=(50, 20), top_p=(None, 0.9), temperature=(1.0, 0.8)))
    for graph in (False, True):
        got = fn(B, cond, n, keep=(mask, codes), use_graph=graph, **kw)
        forced = dict(force=list(got[:levels])) if levels == 3 else dict(force_top=got[0], force_bot=got[1])
        redo = fn(B, cond, n, use_graph=graph, **forced, **kw)
        eng.range_check()
        m = torch.from_numpy(mask)
        for l in range(levels):
            assert torch.equal(got[l].cpu()[m], codes[l][m]), f'level {l}: a kept code did not come back'
            assert torch.equal(redo[l].cpu()[~m], got[l].cpu()[~m]), f'level {l}: the replay draws other codes'
        assert torch.equal(redo[levels], got[levels]), 'logits differ'
        assert bool(torch.isfinite(got[levels + 1]).all()) and torch.equal(redo[levels + 1], got[levels + 1]), 'log-probabilities differ'


# ------------------------------------------------------------------------------- 3. the reference's own fixtures
KEEP_FIXTURES = ['g7_l3_tiny_cls.npz', 'g7_l3_tiny_cls_parallel.npz', 'g7_l3_tiny_cls_parallel_reduce.npz', 'g7_l3_tiny_cls_top2mid2bot.npz',
                 'g13_tiny_cls_bidirectional.npz', 'g3_tiny_txt.npz']


@pytest.mark.parametrize('name', KEEP_FIXTURES)
def test_keeping_the_fixtures_own_codes_gives_the_fixture(name):
    """The fixture's own codes kept on a scattered mask (and on one with a leading run all rows share, through the prefill -- the text fixture: together
    with the prompt): every position that is not kept is drawn as the reference drew it."""
    import json
    fx = load(name)
    spec, weights = stage2_from_fixture(fx)
    B, n, L = int(fx['B']), int(fx['n_steps']), spec.levels
    if name == 'g3_tiny_txt.npz':
        codes, tk, tp, T = [fx['codes_top'], fx['codes_bot']], (None, None), (None, None), (1.0, 1.0)
        cond = synth.text_ids(int(fx['text_seed']), B, spec.ctx_len_txt, spec.vocab_txt)
    else:
        tk, tp, T = json.loads(str(fx['settings']))[0]
        codes = [fx[f'codes{i}_0'] for i in range(3)] if L == 3 else [fx['codes_top_0'], fx['codes_bot_0']]
        cond = np.full((B,), int(fx['cond']) if 'cond' in fx.files else 7, np.int64)
    noise = l3_noise(int(fx['noise_seed']), n, B, spec.vocab_top) if L == 3 else synth.exp_noise(int(fx['noise_seed']), n, B, spec.vocab_top)
    eng = engine_s2(spec, weights, B, max_prefix=n - 1, poison=True)
    fn = eng.sample3 if L == 3 else eng.sample
    kw = dict(precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=t_(noise))
    free = fn(B, t_(cond), n, use_graph=False, **kw)
    assert all((np_(a) == b).all() for a, b in zip(free, codes))               # the premise, restated: the free run is the fixture
    scattered = np.random.default_rng(len(name)).random((B, n)) < 0.4
    scattered[0, 0] = False
    lead = scattered.copy()
    lead[:, :2] = True
    assert keep_leading_run(scattered, n - 1) == 0 and keep_leading_run(lead, n - 1) >= 2
    # kept codes elsewhere are never read: poison them (a value outside the vocabulary would be clamped into it and change the result)
    for mask in (scattered, lead):
        given = [t_(np.where(mask.reshape(B, n, *([1] * (c.ndim - 2))), c, spec.vocab_top + 5)) for c in codes]
        for graph in (False, True):
            got = fn(B, t_(cond), n, use_graph=graph, keep=(mask, given), **kw)
            torch.cuda.synchronize()
            for l, (g, c) in enumerate(zip(got, codes)):
                assert (np_(g) == c).all(), f'{name} graph={graph} level {l}: differs from the fixture'


# ------------------------------------------------------------------------------- 4. row tables, shards, lanes, guidance
def test_philox_shards_row_tables_lanes_and_guided_pairs_with_kept_positions(tiny):
    spec, weights, eng, flat = tiny
    B, n = 5, 12
    cond = torch.arange(B) % spec.n_classes
    codes = _random_codes(spec, B, n, 79)
    mask = K.scattered_mask(B, n, K.KEEP_RUNS_L2, K.KEEP_EXTRA)
    kw = dict(precision=PRECISION_EXACT, seed=4321, top_k=(100, 60))
    for e in (eng, flat):                            # with the prefill (L = 3) and without
        full = e.sample(B, cond, n, keep=(mask, codes), **kw)
        a = e.sample(3, cond[:3], n, keep=(mask[:3], [c[:3] for c in codes]), **kw)
        b = e.sample(2, cond[3:], n, keep=(mask[3:], [c[3:] for c in codes]), sample_offset=3, **kw)
        for l in range(2):
            assert torch.equal(full[l], torch.cat([a[l], b[l]])), 'ragged 3 + 2 rows differ from 5'
        lane = e.clone()
        got = lane.sample(B, cond, n, keep=(mask, codes), **kw)
        assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1]), 'a lane draws other codes'
    assert all(torch.equal(x, y) for x, y in zip(eng.sample(B, cond, n, keep=(mask, codes), **kw), flat.sample(B, cond, n, keep=(mask, codes), **kw)))
    # per-row sampler settings: row b draws what it draws in a call that has its settings for every row
    sets = [((1.0, 0.8), (50, 20), (None, 0.9)), ((0.7, 1.3), (None, None), (None, None))]
    mixed = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=4321, row_samplers=[sets[i % 2] for i in range(B)], keep=(mask, codes))
    for i, (T, k, p) in enumerate(sets):
        one = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=4321, temperature=T, top_k=k, top_p=p, keep=(mask, codes))
        for l in range(2):
            assert torch.equal(mixed[l][i::2], one[l][i::2])
    # a guided pair whose rows keep the same positions: scale 1 draws the positive row's own logits, so both rows are the unguided row
    full = eng.sample(B, cond, n, keep=(mask, codes), **kw)
    twice = (np.concatenate([mask, mask]), [torch.cat([c, c]) for c in codes])
    pairs = [(i, B + i, 1.0) for i in range(B)]
    neg = torch.cat([cond, (cond + 3) % spec.n_classes])
    g = eng.sample(2 * B, neg, n, keep=twice, guidance=pairs, **kw)
    for l in range(2):
        assert torch.equal(g[l][:B], full[l]) and torch.equal(g[l][B:], full[l])
    g2 = eng.sample(2 * B, neg, n, keep=twice, guidance=[(i, B + i, 3.0) for i in range(B)], **kw)
    m = torch.from_numpy(mask)
    assert torch.equal(g2[0][:B], g2[0][B:]) and torch.equal(g2[0][:B].cpu()[m], codes[0][m]) and not torch.equal(g2[0][:B], full[0])
    # ... and one whose rows keep different positions is refused, by name
    other = twice[0].copy()
    other[B + 1, n - 1] ^= True
    with pytest.raises(_lib.HqtError, match='keep table'):
        eng.sample(2 * B, neg, n, keep=(other, twice[1]), guidance=pairs, **kw)
    again = eng.sample(B, cond, n, keep=(mask, codes), **kw)
    assert torch.equal(again[0], full[0]) and torch.equal(again[1], full[1])


# ------------------------------------------------------------------------------- 5. every error path clears the table
def test_every_error_path_names_its_cause_and_leaves_no_table_behind(tiny):
    spec, weights, eng, _ = tiny
    lib, d = eng.lib, dev()
    B, n = 4, 10
    o = _lib.hqt_sample_opts()
    o.precision, o.n_steps, o.temperature_top, o.temperature_bot, o.seed = PRECISION_EXACT, n, 1.0, 1.0, 5
    cond = (torch.arange(B) % spec.n_classes).to(d)
    ct, cb = torch.zeros((B, n), dtype=torch.int64, device=d), torch.zeros((B, n, 4), dtype=torch.int64, device=d)
    kt, kb = (c.to(d) for c in _random_codes(spec, B, n, 80))
    mask = np.ascontiguousarray(K.scattered_mask(B, n, (0, 3, 6, 3), ((0, (2, 5)),)).astype(np.uint8))

    def stage(b=B, steps=n, top=kt, m=mask):
        ptrs = (C.c_void_p * 3)(top.data_ptr() if top is not None else None, kb.data_ptr(), None)
        return lib.hqt_set_keep_mask(eng.h, b, steps, m.ctypes.data_as(C.c_void_p) if m is not None else None, ptrs)

    def plain(force_top=None, b=B, prefix=0):
        if prefix:
            return lib.hqt_sample_prefix(eng.h, b, cond.data_ptr(), C.byref(o), None, prefix, kt.data_ptr(), kb.data_ptr(), None, None, None, ct.data_ptr(), cb.data_ptr(), None)
        return lib.hqt_sample(eng.h, b, cond.data_ptr(), C.byref(o), None, force_top, None, None, ct.data_ptr(), cb.data_ptr(), None)

    def drawn():
        assert plain() == 0
        torch.cuda.synchronize()
        return ct.clone(), cb.clone()
    base = drawn()
    assert stage() == 0 and plain() == 0             # the table works ...
    torch.cuda.synchronize()
    m = torch.from_numpy(mask.astype(bool))
    assert torch.equal(ct.cpu()[m], kt.cpu()[m]) and torch.equal(cb.cpu()[m], kb.cpu()[m]) and not torch.equal(ct, base[0])
    assert all(torch.equal(x, y) for x, y in zip(drawn(), base))       # ... for one call
    assert lib.hqt_set_keep_mask(None, B, n, mask.ctypes.data_as(C.c_void_p), None) == -1 and b'null handle' in lib.hqt_last_error()
    failures = [
        (lambda: stage(b=B - 1, m=mask[:B - 1]), lambda: plain(), b'B='),                    # another B than the call's
        (lambda: stage(steps=n - 1, m=np.ascontiguousarray(mask[:, :n - 1])), lambda: plain(), b'n_steps='),
        (lambda: stage(top=None), lambda: plain(), b'level 0 are NULL'),
        (lambda: stage(), lambda: plain(force_top=kt.data_ptr()), b'force_top'),
        (lambda: stage(), lambda: plain(prefix=3), b'prefix entry point'),
    ]
    for set_table, call, word in failures:
        assert set_table() == 0
        assert call() == -1 and word in lib.hqt_last_error(), lib.hqt_last_error()
        assert all(torch.equal(x, y) for x, y in zip(drawn(), base)), f'{word}: the table outlived the call that refused it'
    # B == 0 or a NULL mask clears
    for clear in (lambda: stage(b=0), lambda: stage(m=None)):
        assert stage() == 0 and clear() == 0
        assert all(torch.equal(x, y) for x, y in zip(drawn(), base))
    # out of range is refused when staged
    assert stage(b=eng.max_batch + 1) == -1 and stage(steps=spec.ctx_len_img + 1) == -1
    assert all(torch.equal(x, y) for x, y in zip(drawn(), base))


# ------------------------------------------------------------------------------- 6. the surface: merged passes, regions, canvases
def _tiny_model(name='tiny-cls.yaml'):
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', name)), seed=5).to(dev())


def test_steps_with_different_prefix_lengths_run_in_one_pass():
    from hqtransformer_amd.pipeline import InflightSampler, sample_codes
    model = _tiny_model()
    spec = model.stage2.spec
    n, sizes, Ps = 64, (2, 3, 2), (0, 5, 9)
    rng = np.random.default_rng(6)
    steps = [dict(cond=int(i + 1), seed=200 + i,
                  **({} if P == 0 else dict(prefix_codes=[t_(rng.integers(0, spec.vocab_top, (b, P))), t_(rng.integers(0, spec.vocab_top, (b, P, 4)))])))
             for i, (b, P) in enumerate(zip(sizes, Ps))]
    common = dict(max_seq_len=n, use_fp16=False, top_k_top=80, top_k_bot=80)
    sampler = InflightSampler(model, lanes=1, merge=3, mixed_prefixes=True)
    launched = sampler.k
    pend = [sampler.submit(b, s['cond'], seed=s['seed'], **{k: v for k, v in s.items() if k == 'prefix_codes'}, **common) for b, s in zip(sizes, steps)]
    assert sampler.k == launched + 1 and not sampler._queue, 'the three steps did not run as one pass'
    sampler.drain()
    for p, b, s, P in zip(pend, sizes, steps, Ps):
        ct, cb, px, _ = p.get()
        want = sample_codes(model.stage2, b, s['cond'], seed=s['seed'], **{k: v for k, v in s.items() if k == 'prefix_codes'}, **common)
        assert torch.equal(ct, want[0]) and torch.equal(cb, want[1]), f'P={P}: the merged step differs from its own call'
        if P:
            assert torch.equal(ct[:, :P].cpu(), s['prefix_codes'][0]) and torch.equal(cb[:, :P].cpu(), s['prefix_codes'][1])
        assert px.shape[0] == b
    # the default keeps its rule
    strict = InflightSampler(model, lanes=1, merge=3)
    strict.submit(2, 1, seed=1, **common)
    with pytest.raises(ValueError, match='prefix length'):
        strict.submit(2, 1, seed=1, prefix_codes=[p[:2] for p in steps[1]['prefix_codes']], **common)
    strict.drain()


def test_regenerate_region_keeps_everything_outside_the_box():
    from hqtransformer_amd.pipeline import box_keep_mask, decode_codes, grids_to_sequences, regenerate_region, sample_codes
    from hqtransformer_amd.sampling import rearrange_levels
    model = _tiny_model()
    R = model.stage1.spec.resolution
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 3, R, R)).astype(np.float32)).to(dev())
    grids = list(model.stage1.code_grids(x))
    K_ = int(grids[0].shape[-1])
    box = (2, 5, 1, 4)
    px, codes = regenerate_region(model, x, box, cond=2, seed=11, use_fp16=False, top_k_top=50, top_k_bot=50)
    model.stage1.range_check()
    assert px.shape == (3, 3, R, R) and float(px.min()) >= 0.0 and float(px.max()) <= 1.0
    for l, (g, own) in enumerate(zip(rearrange_levels(codes, K_), grids)):
        inside = torch.zeros_like(own, dtype=torch.bool)
        inside[:, box[0] << l:box[1] << l, box[2] << l:box[3] << l] = True
        assert torch.equal(g[~inside], own[~inside]), f'level {l}: a cell outside the box changed'
    assert not torch.equal(rearrange_levels(codes, K_)[0], grids[0]), 'nothing was drawn'
    mask = box_keep_mask(K_, box).unsqueeze(0).expand(3, K_ * K_)
    want = sample_codes(model.stage2, 3, 2, seed=11, use_fp16=False, top_k_top=50, top_k_bot=50, max_seq_len=K_ * K_, keep_mask=mask,
                        kept_codes=grids_to_sequences(grids))
    assert all(torch.equal(a, b) for a, b in zip(codes, want))
    assert torch.equal(px, decode_codes(model.stage1, codes))
    with pytest.raises(ValueError, match='box='):
        regenerate_region(model, x, (2, 2, 1, 4), cond=2)


def test_sample_canvas_windows_replay_and_the_scaled_decoder_vs_oracle():
    """tiny-cls, B = 2, a 16 x 16 canvas of 8 x 8 windows with stride 4: 9 windows.  Every window, replayed through plain forcing with seed + k, redraws
    the cells it owns; a second run is identical; the canvas decodes through ``at_resolution(128)`` within the project's 1e-4 of the oracle's decoder
    under the scaled spec."""
    import dataclasses
    from hqtransformer_amd.pipeline import canvas_keep_masks, grids_to_sequences, sample_canvas
    model = _tiny_model()
    B, G, s, seed = 2, 16, 4, 40
    cond = torch.tensor([1, 5])
    grids, px = sample_canvas(model, cond, grid=G, stride=s, seed=seed, use_fp16=False, decode_precision='exact')
    again, px2 = sample_canvas(model, cond, grid=G, stride=s, seed=seed, use_fp16=False, decode_precision='exact')
    assert [tuple(g.shape) for g in grids] == [(B, G, G), (B, 2 * G, 2 * G)]
    assert all(torch.equal(a, b) for a, b in zip(grids, again)) and torch.equal(px, px2), 'a second run differs'
    plan = canvas_keep_masks(G, 8, s)
    assert len(plan) == 9
    eng = model.stage2.engine(B, 64)
    for k, (oy, ox, keep) in enumerate(plan):
        window = grids_to_sequences([g[:, oy << l:(oy + 8) << l, ox << l:(ox + 8) << l] for l, g in enumerate(grids)])
        redo = eng.sample(B, cond, 64, precision=PRECISION_EXACT, seed=seed + k, force_top=window[0], force_bot=window[1])
        own = (~keep).reshape(-1).to(dev())
        assert bool(own.any())
        assert torch.equal(redo[0][:, own], window[0][:, own]) and torch.equal(redo[1][:, own], window[1][:, own]), f'window {k}: the replay draws other codes'
    # pixels: the same weights under the spec scaled by G / w
    s1 = model.stage1
    big = s1.at_resolution(128)
    assert big is s1.at_resolution(128) and big.spec.resolution == 128 and big.spec.z_res == 2 * G
    assert big.spec == dataclasses.replace(s1.spec, resolution=128, attn_resolutions=[2 * a for a in s1.spec.attn_resolutions]) and s1.at_resolution(64) is s1
    assert px.shape == (B, 3, 128, 128)
    ref = O.OracleStage1(big.spec, {k: v.numpy() for k, v in s1.state_dict().items()}).decode_code(np_(grids[0]), np_(grids[1]))
    err = float(np.abs(np_(px) - np.clip(0.5 * ref + 0.5, 0.0, 1.0)).max())
    raw = float(np.abs(np_(big.decode_code(grids, precision='exact')) - ref).max())
    split = float(np.abs(np_(big.decode_code(grids, precision='split')) - ref).max())
    print(f'canvas decode at 128: pixel error {err} (clamped), {raw} (EXACT), {split} (SPLIT)')
    assert err <= 1e-4 and raw <= 1e-4 and split <= 1e-4
    with pytest.raises(ValueError, match='at_resolution'):
        s1.at_resolution(90)


def test_driver_canvas_options_write_the_usual_files(tmp_path):
    import pickle
    from hqtransformer_amd import sampling_hqmodel
    cfg_path = os.path.join(ROOT, 'configs', 'tiny-cls.yaml')
    out = tmp_path / 'out'
    sampling_hqmodel.main(['-r', str(out), '-m', cfg_path, '--batch-size', '2', '--num-classes', '2', '--samples-per-class', '2', '--top-k', '64',
                           '--top-resolution', '8', '--canvas-grid', '12', '--canvas-stride', '4'])
    for cls in (1, 2):
        with open(out / f'samples_({cls}_0).pkl', 'rb') as fp:
            px = pickle.load(fp)
        assert px.dtype == np.float32 and px.shape == (2, 3, 96, 96) and px.min() >= 0.0 and px.max() <= 1.0
        tg = np.load(out / f'targets_({cls}_0).npz')['targets']
        assert (tg == cls - 1).all() and tg.shape == (2,)
    for bad in (['--canvas-grid', '12'], ['--canvas-grid', '12', '--canvas-stride', '3']):
        with pytest.raises(SystemExit):
            sampling_hqmodel.main(['-r', str(out), '-m', cfg_path, '--top-resolution', '8'] + bad)
