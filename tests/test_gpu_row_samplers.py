"""Per-row sampler settings (hqt_set_row_samplers) on the GPU.  Rows of a pass are independent, so the property throughout is: row b of a
mixed call equals, bit for bit and on every code level, row b of a UNIFORM call with the same B, the same noise or seed, the same precision
and that row's settings for every row.  EXACT on tiny-cls is additionally held against the CPU oracle (run once per settings group on the
whole batch).  Every row of every case is compared."""
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
from hqtransformer_amd.sampling import sampling_hqtransformer, sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O
from tests.helpers import load, stage2_from_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_steps=None):
    e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img)
    e.load(stage2=weights)
    e.finalize()
    return e


def np_(t):
    return t.detach().cpu().numpy()


def entry(group):
    """(top_k, top_p, temperature) per level, the argument order of Engine.sample -> a row_samplers entry."""
    tk, tp, T = group
    return (tuple(T), tuple(tk), tuple(tp))


def table_of(groups, assign):
    return [entry(groups[g]) for g in assign]


def assert_rows(got, uniform, assign, what):
    """got: the mixed call's code tensors (one per level); uniform[g]: those of the uniform call with group g's settings."""
    for lv, g_lv in enumerate(got):
        g_lv = np_(g_lv)
        for b, g in enumerate(assign):
            want = np_(uniform[g][lv])[b]
            assert (g_lv[b] == want).all(), f'{what}: row {b} (settings group {g}) differs on level {lv}'


# none; top-k alone; top-k + top-p with two temperatures
GROUPS2 = [((None, None), (None, None), (1.0, 1.0)), ((5, 5), (None, None), (1.0, 1.0)), ((50, 50), (0.9, 0.9), (0.7, 1.3))]


@pytest.fixture(scope='module')
def tiny_model():
    return ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to('cuda').eval()


@pytest.fixture(scope='module')
def g4():
    fx = load('g4_tiny_cls.npz')
    spec, weights = stage2_from_fixture(fx)
    return spec, engine_s2(spec, weights, 8)


@pytest.mark.parametrize('graph', [False, True])
def test_exact_mixed_rows_vs_oracle(tiny_model, graph):
    s2 = tiny_model.stage2.spec
    w2 = {k: v.numpy() for k, v in tiny_model.stage2.state_dict().items()}
    B, n = 6, 24
    assign = [0, 1, 2, 2, 0, 1]
    noise = synth.exp_noise(31, n, B, s2.vocab_top)
    cond = np.array([417, 3, 99, 512, 7, 0])
    oracle = O.OracleStage2(s2, w2)
    want = [oracle.sample(cond, B, n, noise, tk, tp, T) for tk, tp, T in GROUPS2]
    ct, cb = sampling_ihqgpt(tiny_model.stage2, num_candidates=B, cond=torch.from_numpy(cond), use_fp16=False, is_tqdm=False, max_seq_len=n,
                             noise=torch.from_numpy(noise), use_graph=graph, row_samplers=table_of(GROUPS2, assign),
                             top_k_top=3, softmax_temperature=[2.0, 2.0])          # the scalars are ignored while a table is staged
    torch.cuda.synchronize()
    for b, g in enumerate(assign):
        assert (np_(ct)[b] == want[g][0][b]).all(), f'row {b} (group {g}): top codes differ from the oracle'
        assert (np_(cb)[b] == want[g][1][b]).all(), f'row {b} (group {g}): bottom codes differ from the oracle'


def test_graph_replays_changed_values_and_the_table_is_taken_once(g4):
    spec, eng = g4
    B, n = 6, 16
    noise = torch.from_numpy(synth.exp_noise(32, n, B, spec.vocab_top))
    cond = torch.tensor([7, 1, 2, 3, 4, 5])

    def run(graph, **kw):
        out = eng.sample(B, cond, n, precision=PRECISION_EXACT, noise=noise, use_graph=graph, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    uniform = [run(False, top_k=tk, top_p=tp, temperature=T) for tk, tp, T in GROUPS2]
    a1, a2 = [0, 1, 2, 0, 1, 2], [2, 2, 1, 0, 0, 1]
    assert_rows(run(True, row_samplers=table_of(GROUPS2, a1)), uniform, a1, 'first graph call')
    assert_rows(run(True, row_samplers=table_of(GROUPS2, a2)), uniform, a2, 'second graph call (same graph, other values)')
    # no table staged: the scalars again, for every row -- the table of the call before is gone
    tk, tp, T = GROUPS2[1]
    assert_rows(run(True, top_k=tk, top_p=tp, temperature=T), uniform, [1] * B, 'call without a table')
    assert_rows(run(False, row_samplers=table_of(GROUPS2, a2)), uniform, a2, 'eager call')


GROUPS3 = [((None, None, None), (None, None, None), (1.0, 1.0, 1.0)), ((5, 7, 9), (None, None, None), (1.0, 0.9, 0.8)),
           ((50, 50, 20), (0.9, None, 0.8), (0.7, 1.3, 1.1))]


def test_three_levels_parallel_add():
    m = ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-l3.yaml')), seed=9).to('cuda').eval()
    s2 = m.stage2.spec
    B, n = 5, 16
    assign = [2, 0, 1, 0, 2]
    noise = torch.from_numpy(np.maximum(np.random.default_rng(6).standard_exponential((n, 21, B, s2.vocab_top), dtype=np.float32), np.float32(1e-30)))

    def run(graph, **kw):
        out = sampling_hqtransformer(m.stage2, num_candidates=B, cond=torch.tensor([1, 2, 3, 4, 5]), use_fp16=False, is_tqdm=False, max_seq_len=n,
                                     noise=noise, use_graph=graph, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    uniform = [run(False, top_k=list(tk), top_p=list(tp), softmax_temperature=list(T)) for tk, tp, T in GROUPS3]
    for graph in (False, True):
        got = run(graph, row_samplers=table_of(GROUPS3, assign))
        assert [tuple(t.shape) for t in got] == [(B, n), (B, n, 4), (B, n, 16)]
        assert_rows(got, uniform, assign, f'tiny-l3 (graph={graph})')


def resized(fx, vocab):
    """The fixture's model at another vocabulary (synthetic weights of the fixture's seed).  At 1024 entries a FAST pass has both sampler kernels to
    choose from, so a row table makes it dispatch by row; at the fixture's own 512 only the general kernel runs."""
    spec = json.loads(str(fx['spec']))
    spec.update(vocab_top=vocab, vocab_bot=vocab)
    spec = Stage2Spec(**spec)
    return spec, synth.stage2_weights(spec, int(fx['weight_seed']), 'fixture')


@pytest.mark.parametrize('vocab', [512, 1024])
def test_three_levels_top2mid2bot_head(vocab):
    """The causal head of 21 one-token sub-steps: every draw writes ONE slot of a 4- or 16-wide code group (out_stride / out_slot).  With 1024
    entries the FAST rows are dispatched between the two kernels, each of which has to honour the slot."""
    fx = load('g7_l3_tiny_cls_top2mid2bot.npz')
    spec, weights = resized(fx, vocab)
    eng = engine_s2(spec, weights, 4)
    B, n = 4, int(fx['n_steps'])
    assign = [1, 2, 0, 2]
    cond = torch.full((B,), int(fx['cond']))
    for precision, kw in ((PRECISION_EXACT, dict(noise=torch.from_numpy(np.maximum(np.random.default_rng(8).standard_exponential(
            (n, 21, B, spec.vocab_top), dtype=np.float32), np.float32(1e-30))))), (PRECISION_FAST, dict(seed=77))):
        def run(graph, **s):
            out = eng.sample3(B, cond, n, precision=precision, use_graph=graph, **kw, **s)
            torch.cuda.synchronize()
            return [t.clone() for t in out]
        uniform = [run(False, top_k=tk, top_p=tp, temperature=T) for tk, tp, T in GROUPS3]
        assert any(not torch.equal(uniform[0][lv], uniform[1][lv]) for lv in range(3)), 'the settings groups draw the same codes: the case shows nothing'
        for graph in (False, True):
            assert_rows(run(graph, row_samplers=table_of(GROUPS3, assign)), uniform, assign, f'top2mid2bot (V={vocab}, precision={precision}, graph={graph})')
    eng.range_check()


@pytest.mark.parametrize('vocab,precision', [(512, PRECISION_EXACT), (1024, PRECISION_EXACT), (1024, PRECISION_FAST)])
def test_bidirectional_head_keeps_its_mapping_per_row(vocab, precision):
    """All five draws of the bidirectional head use temperature[0], top_k[1], top_p[1]: the other three values of a row must not matter.  With 1024
    entries in FAST the rows are dispatched between the two kernels, by top_k[1] / top_p[1] for every draw."""
    fx = load('g13_tiny_cls_bidirectional.npz')
    spec, weights = resized(fx, vocab)
    eng = engine_s2(spec, weights, 8)
    B, n = 6, 16
    assign = [0, 2, 1, 1, 2, 0]
    kw = dict(noise=torch.from_numpy(synth.exp_noise(33, n, B, spec.vocab_top))) if precision == PRECISION_EXACT else dict(seed=78)
    cond = torch.full((B,), int(fx['cond']))
    used = [(1.0, None, None), (0.8, 7, None), (1.3, 50, 0.9)]                # (temperature[0], top_k[1], top_p[1]) per group

    def run(graph, **s):
        out = eng.sample(B, cond, n, precision=precision, use_graph=graph, **kw, **s)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    uniform = [run(False, top_k=(None, k), top_p=(None, p), temperature=(t, 1.0)) for t, k, p in used]
    assert any(not torch.equal(uniform[0][lv], uniform[1][lv]) for lv in range(2)), 'the settings groups draw the same codes: the case shows nothing'
    # the table fills the unused places with values that would change the draws if they were read
    table = [((used[g][0], 5.0), (2, used[g][1]), (0.3, used[g][2])) for g in assign]
    for graph in (False, True):
        assert_rows(run(graph, row_samplers=table), uniform, assign, f'bidirectional (V={vocab}, precision={precision}, graph={graph})')
    eng.range_check()


@pytest.fixture(scope='module')
def full_vocab():
    """The model of test_full_vocabulary_sampler_vs_oracle (V = 8192: the 1024-thread general kernel, and in FAST the register-resident one)."""
    spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=8192, vocab_bot=8192, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    return spec, engine_s2(spec, synth.stage2_weights(spec, 51, 'fixture'), 256)


# plain rows (FAST: the register-resident kernel), the quality mode, and a row with top-p (99 KB of LDS in the general kernel)
GROUPS_V = [((None, None), (None, None), (1.0, 1.0)), ((2048, 2048), (None, None), (0.95, 0.95)), ((2048, 100), (1.0, 0.9), (0.95, 0.8))]


@pytest.mark.parametrize('precision', [PRECISION_FAST, PRECISION_SPLIT])
@pytest.mark.parametrize('B', [48, 256])
def test_fast_and_split_at_the_full_vocabulary(full_vocab, precision, B):
    spec, eng = full_vocab
    n = 3
    r = np.random.default_rng(B)
    assign = [int(v) for v in r.choice([0, 0, 1, 1, 1, 2], B)]
    assign[:6] = [0, 1, 2, 1, 0, 1]
    cond = torch.from_numpy(r.integers(0, spec.n_classes, B))

    def run(**s):
        out = eng.sample(B, cond, n, precision=precision, seed=1234, sample_offset=5, **s)
        eng.range_check()
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    uniform = [run(top_k=tk, top_p=tp, temperature=T) for tk, tp, T in GROUPS_V]
    assert any(not torch.equal(uniform[0][0], u[0]) for u in uniform[1:]), 'the settings groups draw the same codes: the case shows nothing'
    assert_rows(run(row_samplers=table_of(GROUPS_V, assign)), uniform, assign, f'V=8192 (precision={precision}, B={B})')
    # without a top-p row the general kernel is launched with its small LDS: another graph, the same draws
    assign2 = [g if g != 2 else 1 for g in assign]
    assert_rows(run(row_samplers=table_of(GROUPS_V, assign2)), uniform, assign2, f'V=8192 without top-p (precision={precision}, B={B})')
    if precision == PRECISION_FAST and B <= 64:
        # a root handle, FAST, up to 64 samples: every position of the mixed call above was ONE persistent launch with the sampler launches behind it --
        # shown on an eager call under the timing report, which names the kernels of a pass (test_gpu_persist.py does the same)
        eng.timing_reset()
        eng.timing(True)
        got = run(use_graph=False, row_samplers=table_of(GROUPS_V, assign))
        rep = eng.timing_report()
        eng.timing(False)
        assert rep.get('persist_position', (0,))[0] == n, {k: v[0] for k, v in rep.items()}
        assert_rows(got, uniform, assign, f'V=8192 eager under timing (precision={precision}, B={B})')


def test_mixed_inflight_steps_draw_what_the_separate_calls_draw(tiny_model):
    from hqtransformer_amd.pipeline import InflightSampler
    model = tiny_model
    B, n = 3, 64
    steps = [(5, 11, 0, dict()),                                             # (class id, seed, sample_offset, sampler settings)
             (2, 12, 64, dict(top_k_top=100, top_p_top=0.95, top_k_bot=None, top_p_bot=None, softmax_temperature=[1.0, 0.9])),
             (9, 13, 7, dict(top_k_top=5, top_k_bot=50, top_p_bot=0.9, softmax_temperature=[0.7, 1.3]))]
    sep = []
    for cls, seed, off, kw in steps:
        ct, cb = sampling_ihqgpt(model.stage2, num_candidates=B, cond=cls, use_fp16=False, is_tqdm=False, max_seq_len=n, seed=seed, sample_offset=off, **kw)
        px = model.stage1.decode_sequences(ct, cb, precision='exact', clamp01=True)
        sep.append((ct.clone(), cb.clone(), px.clone()))
    pipe = InflightSampler(model, lanes=1, merge=3, mixed_samplers=True)
    pend = [pipe.submit(B, cls, seed=seed, max_seq_len=n, use_fp16=False, precision='exact', sample_offset=off, **kw) for cls, seed, off, kw in steps]
    pipe.drain()
    torch.cuda.synchronize()
    for i, (p, (ct, cb, px)) in enumerate(zip(pend, sep)):
        mct, mcb, mpx, _ = p.get()
        assert torch.equal(mct, ct) and torch.equal(mcb, cb), f'step {i}: mixed EXACT codes differ from the separate call'
        assert torch.equal(mpx, px), f'step {i}: pixels differ'
    # a mixed queue still refuses a step that differs in anything else, and keeps what is queued
    pipe = InflightSampler(model, lanes=1, merge=3, mixed_samplers=True)
    a = pipe.submit(B, 5, seed=11, max_seq_len=n, use_fp16=False, precision='exact')
    with pytest.raises(ValueError):
        pipe.submit(B, 5, seed=11, max_seq_len=32, use_fp16=False, precision='exact', top_k_top=5)
    pipe.drain()
    torch.cuda.synchronize()
    assert torch.equal(a.get()[0], sep[0][0])
    # the default: the same submissions are refused, in the words the surface has always used
    pipe = InflightSampler(model, lanes=1, merge=3)
    pipe.submit(B, steps[0][0], seed=11, max_seq_len=n, use_fp16=False, precision='exact', **steps[0][3])
    with pytest.raises(ValueError, match='steps merged into one pass must share max_seq_len, precision and sampler settings'):
        pipe.submit(B, steps[1][0], seed=12, max_seq_len=n, use_fp16=False, precision='exact', sample_offset=64, **steps[1][3])
    pipe.drain()


def test_refusals_leave_the_handle_usable(g4):
    spec, eng = g4
    B, n = 4, 8
    cond = torch.tensor([1, 2, 3, 4])

    def run(**kw):
        out = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=9, use_graph=False, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    tk, tp, T = GROUPS2[2]
    want = run(top_k=tk, top_p=tp, temperature=T)
    ok = entry(GROUPS2[2])
    # n != B
    with pytest.raises(_lib.HqtError) as e:
        run(row_samplers=[ok] * (B - 1))
    assert e.value.code == -1
    # the refused call took the table with it: this one runs on its scalars
    assert_rows(run(top_k=tk, top_p=tp, temperature=T), [want], [0] * B, 'after n != B')
    # a temperature <= 0 (on a level the model has)
    for bad in (0.0, -1.0):
        with pytest.raises(_lib.HqtError) as e:
            run(row_samplers=[ok, ok, ((0.7, bad), (50, 50), (0.9, 0.9)), ok])
        assert e.value.code == -1
    # index 2 is ignored by a two-level model
    rows = (_lib.hqt_row_sampler * B)()
    for b in range(B):
        rows[b].temperature[:] = [T[0], T[1], -5.0]
        rows[b].top_k[:] = [tk[0], tk[1], 3]
        rows[b].top_p[:] = [tp[0], tp[1], 0.1]
    _lib.check(eng.lib.hqt_set_row_samplers(eng.h, B, rows))
    assert_rows(run(), [want], [0] * B, 'table with a wild third level')
    # staging and clearing again (n = 0 / NULL): nothing is staged for the next call
    _lib.check(eng.lib.hqt_set_row_samplers(eng.h, B - 1, rows))
    _lib.check(eng.lib.hqt_set_row_samplers(eng.h, 0, None))
    assert_rows(run(top_k=tk, top_p=tp, temperature=T), [want], [0] * B, 'after clearing')
    # a lane has its own table: one staged on the root is not seen by the clone, and stays for the root's next call
    lane = eng.clone()
    _lib.check(eng.lib.hqt_set_row_samplers(eng.h, B - 1, rows))
    out = lane.sample(B, cond, n, precision=PRECISION_EXACT, seed=9, use_graph=False, top_k=tk, top_p=tp, temperature=T)
    torch.cuda.synchronize()
    assert_rows(out, [want], [0] * B, 'lane')
    with pytest.raises(_lib.HqtError):
        run()
    lane.close()


def test_top_p_row_above_8192_entries_is_refused():
    spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=16384, vocab_bot=16384, vocab_txt=64,
                      ctx_len_img=16, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    eng = engine_s2(spec, synth.stage2_weights(spec, 53, 'fixture'), 4)
    B, n = 3, 2
    cond = torch.tensor([1, 2, 3])

    def run(**kw):
        out = eng.sample(B, cond, n, precision=PRECISION_EXACT, seed=4, use_graph=False, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    groups = [((None, None), (None, None), (1.0, 1.0)), ((100, 100), (None, None), (0.9, 0.9))]
    uniform = [run(top_k=tk, top_p=tp, temperature=T) for tk, tp, T in groups]
    with pytest.raises(_lib.HqtError) as e:
        run(row_samplers=[entry(groups[0]), ((1.0, 1.0), (100, 100), (None, 0.9)), entry(groups[1])])
    assert e.value.code == -1 and 'top-p' in str(e.value)
    assign = [1, 0, 1]
    assert_rows(run(row_samplers=table_of(groups, assign)), uniform, assign, 'V=16384 after the refusal')
