"""Completion from a code prefix (hqt_sample_prefix / hqt_sample_prefix_l3): the prefix runs through the body in ONE causal pass
(embed_prefix_kernel + the prefill of the text path), position P is drawn from its last row, the rest are ordinary decode steps.

Bars: EXACT / SPLIT codes of every position >= P bit for bit -- against the reference's own fixtures (their recorded smallest
winner / runner-up ratio is >= 1.00007 and the existing fixture tests already hold EXACT to them bit for bit, so an fp32-accurate prefill
must as well) and, for prefixes the model did not draw, against the unchanged oracle by iteration (tests/prefix_ref.py) on seeds whose
oracle-only margin is recorded below; logits of positions P and P + 1 within the project's 2e-4; FAST teacher-forced logits inside the
gates the text-prefill tests use at the same model sizes (0.15 tiny, 0.1 at D = 1536), on a NaN-poisoned workspace.
Fixtures shorter than 64 positions take the P of {1, 8, 31, 32, 33, 63} that leave a position to draw (P <= n_steps - 1)."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O
from tests.helpers import gate, load, stage2_from_fixture
from tests.prefix_ref import oracle_complete, random_prefix_case

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
PS = (1, 8, 31, 32, 33, 63)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_prefix, poison=False):
    if poison:                       # every workspace buffer starts as NaN: a row no kernel wrote shows up
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


# ------------------------------------------------------------------------------- 1. pinned to the reference's own output
def _fixture_case(name, si):
    """(spec, weights, B, n, cond, noise, settings, codes per level, {step: post-temperature logits}, temperature per draw)."""
    fx = load(name)
    spec, weights = stage2_from_fixture(fx)
    B, n = int(fx['B']), int(fx['n_steps'])
    L = spec.levels
    if name == 'g3_tiny_reduce_uncond.npz':
        k, p, T = int(fx['top_k']), float(fx['top_p']), [float(t) for t in fx['temps']]
        settings, codes, logits = ((k, k), (p, p), T), [fx['codes_top'], fx['codes_bot']], fx['logits']
    else:
        settings = json.loads(str(fx['settings']))[si]
        codes = [fx[f'codes{i}_{si}'] for i in range(3)] if L == 3 else [fx[f'codes_top_{si}'], fx[f'codes_bot_{si}']]
        logits = fx[f'logits_{si}']
    cond = None if spec.cond == 0 else np.full((B,), int(fx['cond']) if 'cond' in fx.files else 7, np.int64)
    noise = l3_noise(int(fx['noise_seed']), n, B, spec.vocab_top) if L == 3 else synth.exp_noise(int(fx['noise_seed']), n, B, spec.vocab_top)
    T = settings[2]
    if spec.depth_decoding == 'bidirectional':       # all five draws use temperature[0]
        scale = np.full((5,), T[0], np.float32)
    else:                                            # the two-level fixtures log post-temperature logits, the three-level ones raw logits
        scale = np.ones((21,), np.float32) if L == 3 else np.array([T[0]] + [T[1]] * 4, np.float32)
    kept = {int(s): logits[i] for i, s in enumerate(fx['keep_steps'])}
    return spec, weights, B, n, cond, noise, settings, codes, kept, scale


def _sample(eng, spec, B, cond, n, **kw):
    fn = eng.sample3 if spec.levels == 3 else eng.sample
    out = fn(B, None if cond is None else t_(cond), n, **kw)
    return list(out[:spec.levels]), (out[spec.levels] if kw.get('return_logits') else None)


FIXTURES = [('g4_tiny_cls.npz', 0), ('g4_tiny_cls.npz', 1), ('g4_tiny_cls.npz', 2), ('g3_tiny_reduce_uncond.npz', 0),
            ('g13_tiny_cls_bidirectional.npz', 0), ('g13_tiny_cls_bidirectional.npz', 1), ('g7_l3_tiny_cls.npz', 0), ('g7_l3_tiny_cls.npz', 1),
            ('g7_l3_tiny_cls_parallel.npz', 0), ('g7_l3_tiny_cls_parallel_reduce.npz', 0), ('g7_l3_tiny_cls_top2mid2bot.npz', 0)]


@pytest.mark.parametrize('name,si', FIXTURES)
def test_completion_of_the_fixture_prefix_is_the_fixture(name, si):
    """Prefix = the fixture's own codes of positions < P: every code of positions >= P must equal the fixture's, eager and graph, and
    the logits of positions P and P + 1 the fixture's where it kept them (2e-4), else those of this engine's free EXACT run -- which the
    existing fixture tests hold to the reference -- and, where the oracle restates the head (every one but the bidirectional), the oracle's."""
    spec, weights, B, n, cond, noise, (tk, tp, T), codes, kept, scale = _fixture_case(name, si)
    # the prefix calls get a NaN-poisoned engine to themselves, shortest prefix first: every longer prefill reaches rows nothing wrote before
    eng = engine_s2(spec, weights, B, max_prefix=n - 1, poison=True)
    kw = dict(precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=t_(noise), return_logits=True)
    free, free_lg = _sample(engine_s2(spec, weights, B, max_prefix=0), spec, B, cond, n, use_graph=False, **kw)
    assert all((np_(a) == b).all() for a, b in zip(free, codes))           # the premise, restated: the free run is the fixture
    free_lg = np_(free_lg)
    orc_lg = None
    if spec.depth_decoding != 'bidirectional':
        orc = (O.OracleStage2L3 if spec.levels == 3 else O.OracleStage2)(spec, weights)
        forced = dict(force=[c.copy() for c in codes]) if spec.levels == 3 else dict(force_top=codes[0].copy(), force_bot=codes[1].copy())
        orc_lg = orc.sample(cond, B, n, noise, tk, tp, T, return_logits=True, **forced)[-1]
    ran = []
    for P in [P for P in PS if P <= n - 1]:
        prefix = [t_(c[:, :P]) for c in codes]
        for graph in (False, True):
            got, lg = _sample(eng, spec, B, cond, n, use_graph=graph, prefix=prefix, **kw)
            torch.cuda.synchronize()
            for l, (g, c) in enumerate(zip(got, codes)):
                assert (np_(g)[:, :P] == c[:, :P]).all(), f'P={P} level {l}: the prefix did not come back verbatim'
                assert (np_(g)[:, P:] == c[:, P:]).all(), f'P={P} graph={graph} level {l}: completion differs from the reference'
            lg = np_(lg)
            assert np.isfinite(lg[P:]).all()
            for p in (P, P + 1):
                if p >= n:
                    continue
                if p in kept:
                    err = np.abs(lg[p] / scale[:, None, None] - kept[p]).max()
                    assert err <= LOGIT_TOL, f'P={P} position {p}: {err} from the fixture'
                if orc_lg is not None:
                    err = np.abs(lg[p] - orc_lg[p]).max()
                    assert err <= LOGIT_TOL, f'P={P} position {p}: {err} from the oracle'
                err = np.abs(lg[p] - free_lg[p]).max()
                assert err <= LOGIT_TOL, f'P={P} position {p}: {err} from the free run'
        ran.append(P)
    assert ran, 'no prefix length fits this fixture'


# ------------------------------------------------------------------------------- 2. a prefix the model did not draw itself
# (spec key, B, n, P, seed): seeds picked on the CPU with the oracle alone (tests/prefix_ref.py: oracle_complete); the margin is the oracle's smallest
# winner / runner-up ratio of p / q over ALL compared draws, recorded here and asserted: >= 1.00009, so no position is excluded.
RANDOM_CASES = {'tiny': ('tiny', 5, 12, 6, 700, 1.0485467910766602),
                'head-2': ('head', 2, 6, 3, 800, 1.00098717212677),
                'head-64': ('head', 64, 6, 3, 800, 1.004356026649475)}
TINY_SET = ((50, 20), (None, 0.9), (1.0, 0.8))
HEAD_SET = ((None, 64), (None, 0.9), (1.0, 0.9))


def _random_spec(kind):
    if kind == 'tiny':
        return stage2_from_fixture(load('g4_tiny_cls.npz')) + (TINY_SET,)
    spec = Stage2Spec(embed_dim=1536, n_layers=1, n_heads=24, n_layers_depth=1, vocab_top=512, vocab_bot=512, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)         # test_imagenet_head_geometry_vs_oracle's
    return spec, synth.stage2_weights(spec, 91, 'fixture'), HEAD_SET


@pytest.mark.parametrize('case', sorted(RANDOM_CASES))
def test_completion_of_a_random_prefix_vs_oracle(case):
    kind, B, n, P, seed, recorded = RANDOM_CASES[case]
    spec, weights, (tk, tp, T) = _random_spec(kind)
    cond, prefix, noise = random_prefix_case(spec, B, n, P, seed)
    wt, wb, wl, margin = oracle_complete(O.OracleStage2(spec, weights), cond, B, n, noise, P, prefix, tk, tp, T)
    print(f'{case}: oracle margin {margin!r} (recorded {recorded!r})')
    assert margin >= 1.00009 and abs(margin - recorded) <= 1e-6 * recorded
    eng = engine_s2(spec, weights, B, max_prefix=P, poison=True)
    for prec in (PRECISION_EXACT, PRECISION_SPLIT):
        for graph in (False, True):
            ct, cb, lg = eng.sample(B, t_(cond), n, precision=prec, top_k=tk, top_p=tp, temperature=T, noise=t_(noise), return_logits=True,
                                    use_graph=graph, prefix=[t_(prefix[0]), t_(prefix[1])])
            eng.range_check()
            assert (np_(ct) == wt).all() and (np_(cb) == wb).all(), f'precision {prec} graph={graph}: codes differ from the oracle'
            err = np.abs(np_(lg)[P:] - wl[P:]).max()
            print(f'{case}: precision {prec} graph={graph} logit error {err}')
            assert err <= LOGIT_TOL


# ------------------------------------------------------------------------------- 3. FAST
@pytest.mark.parametrize('rows', [2, 20, 33, 48, 64])
@pytest.mark.parametrize('kind,B,bar', [('tiny64', 5, 0.15), ('head', 2, 0.1), ('head', 17, 0.1), ('head', 64, 0.1)])
def test_fast_prefill_teacher_forced_vs_oracle(kind, B, bar, rows):
    """P + 1 = ``rows`` body rows per sample through the bf16 prefill on a poisoned workspace: head size 64 (the matrix-core attention from 5
    rows on), row counts that are no multiple of 32 (B (P + 1) = 10 .. 4096).  Teacher-forced on the oracle's codes; logits of positions P and
    P + 1 inside the gate of the text-prefill test of the same size; two runs bit-identical.  HQT_RECORD_GATES=profiles/prefix_fast_gates.txt
    records the measured values (no such record is kept yet: it is written by the first run on an MI355X)."""
    P = rows - 1
    n = min(P + 2, 64)
    if kind == 'tiny64':                             # test_causal_prefill_on_the_matrix_cores_vs_oracle's model, class-conditional
        spec = Stage2Spec(embed_dim=128, n_layers=2, n_heads=2, n_layers_depth=1, vocab_top=256, vocab_bot=256, vocab_txt=64,
                          ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
        weights = synth.stage2_weights(spec, 501 + rows, 'fixture')
    else:
        spec, weights, _ = _random_spec('head')
    cond, prefix, noise = random_prefix_case(spec, B, n, P, 900 + rows)
    rng = np.random.default_rng(rows)
    ft = np.concatenate([prefix[0], rng.integers(0, spec.vocab_top, (B, n - P))], axis=1)
    fb = np.concatenate([prefix[1], rng.integers(0, spec.vocab_top, (B, n - P, 4))], axis=1)
    want = O.OracleStage2(spec, weights).sample(cond, B, n, noise, force_top=ft, force_bot=fb, return_logits=True)[2]
    eng = engine_s2(spec, weights, B, max_prefix=P, poison=True)
    runs = []
    for graph in (False, True, True):
        _, _, lf = eng.sample(B, t_(cond), n, precision=PRECISION_FAST, noise=t_(noise), force_top=t_(ft), force_bot=t_(fb), return_logits=True,
                              use_graph=graph, prefix=[t_(prefix[0]), t_(prefix[1])])
        eng.range_check()
        assert bool(torch.isfinite(lf[P:]).all())
        gate(f'prefix_prefill.fast_logits({kind},B={B},rows={rows},graph={graph})', np.abs(np_(lf)[P:] - want[P:]).max(), bar)
        runs.append(lf)
    assert torch.equal(runs[1], runs[2]), 'two runs differ'


# ------------------------------------------------------------------------------- 4. invariants
@pytest.fixture(scope='module')
def tiny():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    return fx, spec, weights, engine_s2(spec, weights, 8, max_prefix=63)


def test_a_handle_without_max_prefix_allocates_what_it_did_and_refuses_a_prefix(tiny):
    fx, spec, weights, eng = tiny
    plain = Engine(spec, None, dev(), 8, spec.ctx_len_img)
    # workspaces as hqt_create sizes them (no weights loaded: nothing else is counted).  max_prefix = 0 is the handle of before the field: what
    # grows with max_prefix are exactly the buffers sized by the rows of the widest body pass, so 0 costs nothing and 63 must cost something
    again = Engine(spec, None, dev(), 8, spec.ctx_len_img, max_prefix=0)
    one = Engine(spec, None, dev(), 8, spec.ctx_len_img, max_prefix=1)      # 2 rows per sample < the 4 depth rows that already size it
    big = Engine(spec, None, dev(), 8, spec.ctx_len_img, max_prefix=63)
    assert plain.max_prefix == 0 and again.workspace_bytes() == plain.workspace_bytes() == one.workspace_bytes() < big.workspace_bytes()
    print(f'workspace bytes: max_prefix 0 -> {plain.workspace_bytes()}, 63 -> {big.workspace_bytes()}')
    plain.load(stage2=weights)
    plain.finalize()
    # the library's own refusals (the Python surface refuses earlier: tests/test_prefix_host.py)
    import ctypes as C
    o = _lib.hqt_sample_opts()
    o.precision, o.n_steps, o.temperature_top, o.temperature_bot = PRECISION_EXACT, 16, 1.0, 1.0
    cond = torch.zeros(2, dtype=torch.int64, device=dev())
    pt, pb = torch.zeros((2, 20), dtype=torch.int64, device=dev()), torch.zeros((2, 20, 4), dtype=torch.int64, device=dev())
    ot, ob = torch.zeros((2, 16), dtype=torch.int64, device=dev()), torch.zeros((2, 16, 4), dtype=torch.int64, device=dev())

    def call(e, P):
        return e.lib.hqt_sample_prefix(e.h, 2, cond.data_ptr(), C.byref(o), None, P, pt.data_ptr(), pb.data_ptr(), None, None, None, ot.data_ptr(), ob.data_ptr(), None)
    assert call(plain, 4) == -1 and b'hqt_set_max_prefix' in plain.lib.hqt_last_error()
    for P in (0, -3, 16, 17):
        assert call(eng, P) == -1 and b'n_steps - 1' in eng.lib.hqt_last_error()
    assert eng.lib.hqt_sample_prefix(eng.h, 2, cond.data_ptr(), C.byref(o), None, 4, None, pb.data_ptr(), None, None, None, ot.data_ptr(), ob.data_ptr(), None) == -1
    assert call(eng, 4) == 0
    torch.cuda.synchronize()
    # hqt_set_max_prefix: range, and only before the weights are finalized
    fresh = Engine(spec, None, dev(), 8, spec.ctx_len_img)
    for bad in (-1, 64):                             # > max_steps - 1
        assert fresh.lib.hqt_set_max_prefix(fresh.h, bad) == -1 and b'max_prefix' in fresh.lib.hqt_last_error()
    assert fresh.lib.hqt_set_max_prefix(fresh.h, 63) == 0 and fresh.workspace_bytes() == big.workspace_bytes()
    assert fresh.lib.hqt_set_max_prefix(fresh.h, 0) == 0 and fresh.workspace_bytes() == plain.workspace_bytes()      # and back: nothing is left behind
    assert eng.lib.hqt_set_max_prefix(eng.h, 8) == -3 and b'hqt_finalize_weights' in eng.lib.hqt_last_error()


def test_philox_shards_rows_tables_and_lanes_with_a_prefix(tiny):
    fx, spec, weights, eng = tiny
    n, P = 24, 9
    cond = torch.arange(5) % spec.n_classes
    rng = np.random.default_rng(77)
    prefix = [t_(rng.integers(0, spec.vocab_top, (5, P))), t_(rng.integers(0, spec.vocab_top, (5, P, 4)))]
    kw = dict(precision=PRECISION_EXACT, seed=4321, top_k=(100, 60))
    full = eng.sample(5, cond, n, prefix=prefix, **kw)
    a = eng.sample(3, cond[:3], n, prefix=[p[:3] for p in prefix], **kw)
    b = eng.sample(2, cond[3:], n, prefix=[p[3:] for p in prefix], sample_offset=3, **kw)
    for l in range(2):
        assert torch.equal(full[l], torch.cat([a[l], b[l]])), 'ragged 3 + 2 rows differ from 5'
        assert torch.equal(full[l][:, :P], prefix[l].to(full[l].device))
    # the same keys as a free run: teacher-forcing the whole completed sequence through the free entry point redraws it
    redo = eng.sample(5, cond, n, force_top=full[0], force_bot=full[1], **kw)
    assert torch.equal(redo[0][:, P:], full[0][:, P:]) and torch.equal(redo[1][:, P:], full[1][:, P:])
    # per-row tables: row b with its own settings draws what it draws in a call that has them for every row
    sets = [((1.0, 0.8), (50, 20), (None, 0.9)), ((0.7, 1.3), (None, None), (None, None))]
    rows = [sets[i % 2] for i in range(5)]
    mixed = eng.sample(5, cond, n, precision=PRECISION_EXACT, seed=4321, row_samplers=rows, prefix=prefix)
    for i, (T, k, p) in enumerate(sets):
        one = eng.sample(5, cond, n, precision=PRECISION_EXACT, seed=4321, temperature=T, top_k=k, top_p=p, prefix=prefix)
        for l in range(2):
            assert torch.equal(mixed[l][i::2], one[l][i::2])
    # a lane inherits max_prefix and draws the same
    lane = eng.clone()
    assert lane.max_prefix == eng.max_prefix and lane.workspace_bytes() > 0
    got = lane.sample(5, cond, n, prefix=prefix, **kw)
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
    # given_top_code keeps its meaning behind the prefix
    given = t_(rng.integers(0, spec.vocab_top, (5, n)))
    g = eng.sample(5, cond, n, force_top=given, prefix=prefix, **kw)
    want = eng.sample(5, cond, n, force_top=torch.cat([prefix[0], given[:, P:]], 1), force_bot=torch.cat([prefix[1], g[1][:, P:].cpu()], 1), **kw)
    assert torch.equal(g[1][:, P:], want[1][:, P:]) and torch.equal(g[0][:, P:], want[0][:, P:])


def _tiny_model(name):
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', name)), seed=5).to(dev())


def test_merged_pass_with_one_prefix_length_equals_the_separate_calls():
    from hqtransformer_amd.pipeline import InflightSampler, sample_codes
    model = _tiny_model('tiny-cls.yaml')
    spec = model.stage2.spec
    n, P, sizes = 64, 5, (3, 2)                      # the whole 8 x 8 grid: a merged step decodes what it samples
    rng = np.random.default_rng(5)
    steps = [dict(cond=int(i + 1), seed=100 + i, prefix_codes=[t_(rng.integers(0, spec.vocab_top, (b, P))), t_(rng.integers(0, spec.vocab_top, (b, P, 4)))])
             for i, b in enumerate(sizes)]
    sampler = InflightSampler(model, lanes=1, merge=2)
    pend = [sampler.submit(b, s['cond'], seed=s['seed'], max_seq_len=n, use_fp16=False, prefix_codes=s['prefix_codes'], top_k_top=80, top_k_bot=80)
            for b, s in zip(sizes, steps)]
    # the pass above is full and gone; a step without a prefix now waits alone, and a step WITH one may not join it
    lone = sampler.submit(2, 1, seed=1, max_seq_len=n, use_fp16=False, top_k_top=80, top_k_bot=80)
    with pytest.raises(ValueError, match='prefix length'):
        sampler.submit(2, 1, seed=1, max_seq_len=n, use_fp16=False, top_k_top=80, top_k_bot=80, prefix_codes=steps[1]['prefix_codes'])
    sampler.drain()                                  # the refused step was never queued: the lone one runs as a pass of its own
    assert lone.get()[0].shape == (2, n)
    for p, b, s in zip(pend, sizes, steps):
        ct, cb, px, _ = p.get()
        want = sample_codes(model.stage2, b, s['cond'], seed=s['seed'], max_seq_len=n, use_fp16=False, prefix_codes=s['prefix_codes'], top_k_top=80, top_k_bot=80)
        assert torch.equal(ct, want[0]) and torch.equal(cb, want[1])
        assert torch.equal(ct[:, :P].cpu(), s['prefix_codes'][0])


# ------------------------------------------------------------------------------- 6. surface
@pytest.mark.parametrize('name', ['tiny-cls.yaml', 'tiny-l3.yaml'])
def test_complete_images_keeps_the_rows_and_decodes_its_codes(name):
    from hqtransformer_amd.pipeline import complete_images, decode_codes
    from hqtransformer_amd.sampling import rearrange_levels
    model = _tiny_model(name)
    R = model.stage1.spec.resolution
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 3, R, R)).astype(np.float32)).to(dev())
    grids = model.stage1.code_grids(x)
    K = int(grids[0].shape[-1])
    extra = dict(top_k=[50] * 3) if model.stage2.spec.levels == 3 else dict(top_k_top=50, top_k_bot=50)
    for keep in (1, K - 1):
        px, codes = complete_images(model, x, keep, cond=2, seed=11, use_fp16=False, **extra)
        model.stage1.range_check()
        assert px.shape == (3, 3, R, R) and float(px.min()) >= 0.0 and float(px.max()) <= 1.0
        for l, (g, own) in enumerate(zip(rearrange_levels(codes, K), grids)):
            assert torch.equal(g[:, :keep << l], own[:, :keep << l]), f'level {l}: kept rows differ from get_codes'
            assert g.shape == own.shape
        assert torch.equal(px, decode_codes(model.stage1, codes))
    flat = model.stage1.get_codes(x)
    assert all(torch.equal(f, g.reshape(-1)) for f, g in zip(flat, grids))
    with pytest.raises(ValueError, match='keep_rows'):
        complete_images(model, x, K, cond=2)


def test_driver_option_writes_the_usual_files(tmp_path):
    import pickle
    from hqtransformer_amd import sampling_hqmodel
    cfg_path = os.path.join(ROOT, 'configs', 'tiny-cls.yaml')
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.spec import stage1_spec_from_config, stage2_spec_from_config
    cfg = load_config(cfg_path)
    R, K = stage1_spec_from_config(cfg).resolution, int(round(stage2_spec_from_config(cfg).ctx_len_img ** 0.5))
    src = tmp_path / 'images.npy'
    np.save(src, np.random.default_rng(1).uniform(0, 1, (3, 3, R, R)).astype(np.float32))
    out = tmp_path / 'out'
    sampling_hqmodel.main(['-r', str(out), '-m', cfg_path, '--batch-size', '2', '--num-classes', '2', '--samples-per-class', '2', '--top-k', '64',
                           '--top-resolution', str(K), '--complete-from', str(src), '--keep-rows', '1'])
    for cls in (1, 2):
        with open(out / f'samples_({cls}_0).pkl', 'rb') as fp:
            px = pickle.load(fp)
        assert px.dtype == np.float32 and px.shape == (2, 3, R, R) and px.min() >= 0.0 and px.max() <= 1.0
        tg = np.load(out / f'targets_({cls}_0).npz')['targets']
        assert tg.dtype == np.int64 and (tg == cls - 1).all() and tg.shape == (2,)
    with pytest.raises(SystemExit):
        sampling_hqmodel.main(['-r', str(out), '-m', cfg_path, '--complete-from', str(src)])
