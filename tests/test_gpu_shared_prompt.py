"""Shared prompts on the GPU (hqt_set_prompt_groups, prompt_groups=, share_prompts=): the text prefill runs over the G distinct prompts of a pass into a
staging buffer, prompt_fanout_kernel copies every row's K/V into its cache slot and gathers the last prompt row of x, the depth head draws position 0 over
the B rows, and the decode steps are those of an unshared call.

Bars: EXACT / SPLIT against the unchanged oracle on the EXPANDED prompts -- codes bit for bit, logits of every position within the project's 2e-4, on seeds
whose oracle-only margin is recorded below and asserted --; EXACT bit for bit against the unshared call on the same handle; FAST teacher-forced logits inside
the 0.15 gate the text tests already hold these models to.  Every engine here starts from a NaN-poisoned workspace: a cache row or an x row the fan-out did not
write shows up."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_text_prefix as TP
from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.models import HQTransformerStage2
from hqtransformer_amd.sampling import prompt_groups_of, sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from oracle import hqt_oracle as O
from tests.helpers import gate

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
FAST_BAR = 0.15
dev, np_, engine_s2 = TP.dev, TP.np_, TP.engine_s2


def t_(a):
    return torch.from_numpy(np.array(a))                                  # a copy: the shared reference arrays are read-only


G5 = [2, 0, 0, 1, 2]                                                      # non-monotone, G = 3
G17 = [3, 1, 0, 2, 2, 0, 1, 3, 3, 3, 0, 1, 2, 0, 0, 1, 2]                 # an odd row count, G = 4
# (spec key, group table, n, seed, margin): seeds picked on the CPU with the oracle alone (a free run over the expanded prompts, text ids
# synth.text_ids(seed, G)); the margin is the oracle's smallest winner / runner-up ratio of p / q over ALL draws of the run, recorded here and asserted:
# >= 1.00009 (the bar of test_gpu_text_prefix.RANDOM_CASES), so no position is excluded.
ORACLE_CASES = {'tiny': ('tiny', G5, 6, 1204, 1.0160129070281982),
                'head': ('head', G17, 4, 1301, 1.0092179775238037)}


@functools.lru_cache(maxsize=None)
def oracle_case(case):
    """(spec, weights, sampler settings, unique prompts [G, T], noise, oracle codes_top, codes_bot, logits [n, 5, B, V], margin): computed once, read-only."""
    kind, groups, n, seed, _ = ORACLE_CASES[case]
    spec, weights, (tk, tp, T) = TP._random_spec(kind)
    B, G = len(groups), max(groups) + 1
    uniq = synth.text_ids(seed, G, spec.ctx_len_txt, spec.vocab_txt)
    noise = synth.exp_noise(seed, n, B, spec.vocab_top)
    O.MARGIN_SINK = sink = []
    try:
        wt, wb, wl = O.OracleStage2(spec, weights).sample(uniq[groups], B, n, noise, tk, tp, T, return_logits=True)
    finally:
        O.MARGIN_SINK = None
    assert len(sink) == 5 * n
    for a in (uniq, noise, wt, wb, wl):
        a.setflags(write=False)
    return spec, weights, (tk, tp, T), uniq, noise, wt, wb, wl, float(min(sink))


# ------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize('case', sorted(ORACLE_CASES))
def test_shared_prefill_vs_oracle_on_the_expanded_prompts(case):
    _, groups, n, _, recorded = ORACLE_CASES[case]
    spec, weights, (tk, tp, T), uniq, noise, wt, wb, wl, margin = oracle_case(case)
    print(f'{case}: oracle margin {margin!r} (recorded {recorded!r})')
    assert margin >= 1.00009 and abs(margin - recorded) <= 1e-6 * recorded
    B = len(groups)
    eng = engine_s2(spec, weights, B, 0, poison=True)
    for prec in (PRECISION_EXACT, PRECISION_SPLIT):
        for graph in (False, True):
            ct, cb, lg = eng.sample(B, t_(uniq), n, precision=prec, top_k=tk, top_p=tp, temperature=T, noise=t_(noise), return_logits=True,
                                    use_graph=graph, prompt_groups=groups)
            eng.range_check()
            assert (np_(ct) == wt).all() and (np_(cb) == wb).all(), f'precision {prec} graph={graph}: codes differ from the oracle'
            err = np.abs(np_(lg) - wl).max()
            print(f'{case}: precision {prec} graph={graph} logit error {err}')
            assert err <= LOGIT_TOL


# ------------------------------------------------------------------------------- 2. EXACT: the unshared call, bit for bit
@pytest.fixture(scope='module')
def tiny_pair():
    """The tiny case on one poisoned handle with its unshared EXACT result (codes_top, codes_bot, logits), shared by the tests below and left unchanged."""
    spec, weights, (tk, tp, T), uniq, noise, *_ = oracle_case('tiny')
    eng = engine_s2(spec, weights, 5, 8, poison=True)                    # (max_prefix 8: the refusal of a table with a prefix needs room for one)
    kw = dict(precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=t_(noise), return_logits=True)
    full = t_(uniq[G5])
    plain = eng.sample(5, full, 6, **kw)                                 # (the first call of a handle binds its persistent chain)
    before = eng.workspace_bytes()
    assert same(eng.sample(5, full, 6, **kw), plain)
    torch.cuda.synchronize()
    assert eng.workspace_bytes() == before                               # a call without a table allocates nothing for the feature
    return spec, weights, eng, kw, full, plain


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_exact_shared_call_is_the_unshared_call_bit_for_bit(tiny_pair):
    spec, _, eng, kw, full, plain = tiny_pair
    uniq3, g3 = prompt_groups_of(full)
    assert g3.tolist() == [0, 1, 1, 2, 0]                                # first-appearance order: another table for the same rows than G5
    tables = {'G=1': (full[:1], [0] * 5), 'G=B': (full, [0, 1, 2, 3, 4]), 'G=3': (uniq3, g3), 'G=3, as picked': (t_(oracle_case('tiny')[3]), G5)}
    for name, (cond, groups) in tables.items():
        want = plain if name != 'G=1' else eng.sample(5, full[:1].expand(5, -1), 6, **kw)
        for graph in (False, True):
            got = eng.sample(5, cond, 6, use_graph=graph, prompt_groups=groups, **kw)
            assert same(got, want), f'{name} graph={graph}: the shared call differs from the unshared one'
            assert bool(torch.isfinite(got[2]).all())
    # the table belonged to its call: the next call without one prefills every row of a [B, T] cond again
    assert same(eng.sample(5, full, 6, **kw), plain)


# ------------------------------------------------------------------------------- 3. FAST, teacher-forced on the oracle's codes
@pytest.mark.parametrize('kind,groups', [('mfma', [1, 0, 0, 1, 0]), ('tiny', G5)])
def test_fast_shared_prefill_teacher_forced_vs_oracle(kind, groups):
    """Position 0 reads the gathered x, position 1 the fanned-out K/V of every layer (mfma: two body layers, the one-wave MFMA prefill over G = 2 samples).
    The prefill of fewer rows may be served by other GEMM kernels than the unshared one's: the difference is recorded, equality is not claimed.
    HQT_RECORD_GATES=<file> records the measured values."""
    spec, weights = TP._mfma_spec(64) if kind == 'mfma' else TP._random_spec('tiny')[:2]
    B, G, n = 5, max(groups) + 1, 3
    uniq = synth.text_ids(1400, G, spec.ctx_len_txt, spec.vocab_txt)
    noise = synth.exp_noise(1401, n, B, spec.vocab_top)
    ft, fb, want = O.OracleStage2(spec, weights).sample(uniq[groups], B, n, noise, return_logits=True)
    eng = engine_s2(spec, weights, B, 0, poison=True)
    kw = dict(precision=PRECISION_FAST, noise=t_(noise), force_top=t_(ft), force_bot=t_(fb), return_logits=True)
    runs = []
    for graph in (False, True, True):
        lf = eng.sample(B, t_(uniq), n, use_graph=graph, prompt_groups=groups, **kw)[2]
        eng.range_check()
        assert bool(torch.isfinite(lf[:2]).all())
        gate(f'shared_prompt.fast_logits({kind},graph={graph})', np.abs(np_(lf)[:2] - want[:2]).max(), FAST_BAR)
        runs.append(lf)
    assert torch.equal(runs[1], runs[2]), 'two graph runs differ'
    unshared = eng.sample(B, t_(uniq[groups]), n, use_graph=False, **kw)[2]
    eng.range_check()
    gate(f'shared_prompt.fast_shared_vs_unshared({kind})', float((runs[0] - unshared).abs().max()), 0.0, op='>=')       # recorded, not gated: a difference is never negative


# ------------------------------------------------------------------------------- 4. the staging buffer grows
def test_a_larger_table_grows_the_staging_buffer(tiny_pair):
    spec, weights, _, kw, full, plain = tiny_pair
    eng = engine_s2(spec, weights, 5, 0, poison=True)
    pair = torch.cat([full[:1], full[3:4]])                              # two prompts
    want = eng.sample(5, pair[[0, 0, 0, 1, 1]], 6, **kw)
    torch.cuda.synchronize()
    sizes = [eng.workspace_bytes()]
    got = eng.sample(5, pair, 6, prompt_groups=[0, 0, 0, 1, 1], **kw)
    torch.cuda.synchronize()
    sizes.append(eng.workspace_bytes())
    assert same(got, want)
    assert same(eng.sample(5, full, 6, prompt_groups=[0, 1, 2, 3, 4], **kw), plain)      # G = 5 after G = 2
    torch.cuda.synchronize()
    sizes.append(eng.workspace_bytes())
    assert same(eng.sample(5, pair, 6, prompt_groups=[0, 0, 0, 1, 1], **kw), want)       # and back: the larger buffer serves the smaller table
    assert eng.workspace_bytes() == sizes[2]
    per_prompt = 2 * spec.n_layers * spec.ctx_len_txt * spec.embed_dim * 4
    assert sizes[1] - sizes[0] == 2 * per_prompt + 5 * spec.embed_dim * 4 and sizes[2] - sizes[1] == 3 * per_prompt, sizes


# ------------------------------------------------------------------------------- 5., 6. the sampling surface
@pytest.fixture(scope='module')
def tiny_model(tiny_pair):
    spec, weights = tiny_pair[:2]
    st2 = HQTransformerStage2(spec)
    st2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    st2 = st2.to('cuda')
    os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        st2.engine(12, 6)                                                # every call below fits this engine
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    return spec, st2


def test_merged_pass_with_shared_prompts_equals_step_at_a_time_exact(tiny_model):
    """Three steps (own captions, Philox seed and row offset each) as ONE pass of 12 rows that prefills its 4 distinct captions once: in EXACT every row
    draws what it draws in its own unshared call (the pattern of test_merged_pass_equals_step_at_a_time_exact), and the pass launches ONE fan-out."""
    spec, st2 = tiny_model
    B, n = 4, 6
    caps = t_(synth.text_ids(1500, 4, spec.ctx_len_txt, spec.vocab_txt))            # a, b, c, d
    steps = [([0, 0, 1, 0], 11, 0), ([2, 2, 2, 2], 12, 64), ([1, 3, 0, 0], 13, 7)]  # (captions, seed, sample_offset)
    kw = dict(precision='exact', max_seq_len=n, top_k_top=50, top_k_bot=20, softmax_temperature=[1.1, 0.8], is_tqdm=False)
    sep = [sampling_ihqgpt(st2, 1, caps[c], seed=s, sample_offset=o, use_graph=False, **kw) for c, s, o in steps]
    cond = torch.cat([caps[c] for c, _, _ in steps])
    assert prompt_groups_of(cond)[0].shape[0] == 4
    seeds = [s for _, s, _ in steps for _ in range(B)]
    offs = [o + b for _, _, o in steps for b in range(B)]
    eng = st2.engine(12, n)
    for graph in (False, True):
        mt, mb = sampling_ihqgpt(st2, 1, cond, row_seeds=seeds, row_offsets=offs, use_graph=graph, share_prompts=True, **kw)
        for i, (ct, cb) in enumerate(sep):
            assert torch.equal(mt[i * B:(i + 1) * B], ct) and torch.equal(mb[i * B:(i + 1) * B], cb), f'merged step {i} (graph={graph})'
    eng.timing_reset()
    eng.timing(True)
    try:
        mt, mb = sampling_ihqgpt(st2, 1, cond, row_seeds=seeds, row_offsets=offs, share_prompts=True, **kw)
        torch.cuda.synchronize()
    finally:
        eng.timing(False)
    report = eng.timing_report()
    assert report['prompt_fanout'][0] == 1, report.get('prompt_fanout')
    assert torch.equal(mt[:B], sep[0][0])
    eng.timing_reset()


def test_guided_call_with_shared_prompts_equals_the_unshared_one_exact(tiny_model):
    spec, st2 = tiny_model
    n = 6
    cond = t_(synth.text_ids(1600, 3, spec.ctx_len_txt, spec.vocab_txt))
    kw = dict(precision='exact', max_seq_len=n, seed=5, guidance_scale=2.0, return_logprobs=True, top_k_top=50, top_k_bot=20, is_tqdm=False)
    want = sampling_ihqgpt(st2, 1, cond, **kw)
    eng = st2.engine(6, n)
    staged = []
    inner = eng.sample

    def spy(batch, c, *a, **k):
        staged.append((batch, tuple(c.shape), k.get('prompt_groups')))
        return inner(batch, c, *a, **k)
    eng.sample = spy
    try:
        got = sampling_ihqgpt(st2, 1, cond, share_prompts=True, **kw)
    finally:
        del eng.sample
    assert same(got, want) and bool(torch.isfinite(got[2]).all())
    batch, shape, groups = staged[-1]
    assert batch == 6 and shape == (4, spec.ctx_len_txt) and groups.tolist() == [0, 1, 2, 3, 3, 3]      # the three negative rows are one group


# ------------------------------------------------------------------------------- 7. three code levels
def test_three_level_shared_call_is_the_unshared_call_exact():
    """hqt_sample_l3 takes the table as hqt_sample does.  The reference has no three-level text fixture: this is self-consistency only -- the shared call
    against the unshared one on the same handle --, not a comparison with the reference."""
    spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=64, vocab_bot=64, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                      n_classes=0, cond=2, embedding=0, levels=3)
    eng = engine_s2(spec, synth.stage2_weights(spec, 5, 'fixture'), 3, 0, poison=True)
    uniq = t_(synth.text_ids(1700, 2, spec.ctx_len_txt, spec.vocab_txt))
    groups = [1, 0, 1]
    kw = dict(precision=PRECISION_EXACT, seed=9, top_k=(50, 40, 30), return_logits=True)
    want = eng.sample3(3, uniq[groups], 3, **kw)
    for graph in (False, True):
        got = eng.sample3(3, uniq, 3, use_graph=graph, prompt_groups=groups, **kw)
        assert same(got, want), f'graph={graph}'
        assert bool(torch.isfinite(got[3]).all())


# ------------------------------------------------------------------------------- 8. refusals through the C ABI
def test_the_library_refuses_by_name_and_the_handle_stays_usable(tiny_pair):
    spec, _, eng, _, full, _ = tiny_pair
    lib, B, n = eng.lib, 5, 6
    cond = full.to(dev())
    out = [torch.zeros((B, n), dtype=torch.int64, device=dev()), torch.zeros((B, n, 4), dtype=torch.int64, device=dev())]
    o = _lib.hqt_sample_opts()
    o.precision, o.n_steps, o.temperature_top, o.temperature_bot, o.seed = PRECISION_EXACT, n, 1.0, 1.0, 77

    def stage(table, b=None, g=None, e=eng):
        a = np.ascontiguousarray(table, dtype=np.int32)
        with torch.cuda.device(dev()):
            return lib.hqt_set_prompt_groups(e.h, len(a) if b is None else b, max(table) + 1 if g is None else g, a.ctypes.data_as(C.c_void_p))

    def sample(b=B):
        with torch.cuda.device(dev()):
            rc = lib.hqt_sample(eng.h, b, cond.data_ptr(), C.byref(o), None, None, None, None, out[0].data_ptr(), out[1].data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    def plain_again(what):
        assert sample() == 0, lib.hqt_last_error()
        assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1]), f'after {what}: the plain call changed'

    assert sample() == 0
    first = [t.clone() for t in out]
    # a handle that is not text-conditional (refused before anything else is looked at: no weights needed)
    cls = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=64, vocab_bot=64, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
                     n_classes=10, cond=1, embedding=0)
    ce = Engine(cls, None, dev(), 4, cls.ctx_len_img)
    assert stage([0, 0], e=ce) == -1 and b'not text-conditional' in lib.hqt_last_error()
    ce.close()
    # the table itself
    assert stage([0, 1, 2, 7, 0], g=3) == -1 and b'group_of_row[3]=7 outside [0, n_groups=3)' in lib.hqt_last_error()
    assert stage([0, 1, -1, 0, 0], g=2) == -1 and b'group_of_row[2]=-1' in lib.hqt_last_error()
    assert stage([0] * 5, b=0) == -1 and b'B=0 outside [1, max_batch=5]' in lib.hqt_last_error()
    assert stage([0] * 5, b=6) == -1 and b'B=6 outside' in lib.hqt_last_error()
    assert stage([0] * 5, g=0) == -1 and b'n_groups=0 outside' in lib.hqt_last_error()
    assert stage([0, 1], g=3) == -1 and b'n_groups=3 exceeds B=2' in lib.hqt_last_error()
    plain_again('refused tables')
    # a table of another B than the call's: refused, and gone with the call
    assert stage([0, 1, 1, 0]) == 0
    assert sample() == -1 and b'staged a table of B=4, this call has B=5' in lib.hqt_last_error()
    plain_again('a B mismatch')
    # a table together with a code prefix
    assert stage(G5) == 0
    pt, pb = torch.zeros((B, 2), dtype=torch.int64, device=dev()), torch.zeros((B, 2, 4), dtype=torch.int64, device=dev())
    with torch.cuda.device(dev()):
        rc = lib.hqt_sample_prefix(eng.h, B, cond.data_ptr(), C.byref(o), None, 2, pt.data_ptr(), pb.data_ptr(), None, None, None, out[0].data_ptr(), out[1].data_ptr(), None)
    assert rc == -1 and b'hqt_set_prompt_groups together with a code prefix' in lib.hqt_last_error()
    plain_again('a table with a prefix')
    # ... and together with a keep table whose rows share a leading run
    assert stage(G5) == 0
    mask = np.zeros((B, n), np.uint8)
    mask[:, :2] = 1
    kept = (C.c_void_p * 3)(first[0].data_ptr(), first[1].data_ptr(), None)
    assert lib.hqt_set_keep_mask(eng.h, B, n, mask.ctypes.data_as(C.c_void_p), kept) == 0
    assert sample() == -1 and b'prefix_len=2' in lib.hqt_last_error() and b'hqt_set_prompt_groups' in lib.hqt_last_error()
    plain_again('a table with a kept leading run')
    # hqt_score clears a staged table and says so
    assert stage(G5) == 0
    with torch.cuda.device(dev()):
        rc = lib.hqt_score(eng.h, B, cond.data_ptr(), None, n, PRECISION_EXACT, None, None, None)
    assert rc == -3 and b'hqt_set_prompt_groups' in lib.hqt_last_error()
    plain_again('hqt_score')


# ------------------------------------------------------------------------------- 9. the pipeline and the driver
def test_inflight_sampler_shares_prompts_across_the_steps_of_a_pass():
    """InflightSampler(share_prompts=True): three steps of four captions each run as ONE pass that prefills its distinct captions once; in EXACT every step
    receives the codes and pixels it receives from a sampler that does not share."""
    from hqtransformer_amd.pipeline import InflightSampler
    model = TP._tiny_model()
    spec = model.stage2.spec
    n = spec.ctx_len_img
    caps = t_(synth.text_ids(1800, 4, spec.ctx_len_txt, spec.vocab_txt))
    steps = [([0, 0, 1, 0], 21, 0), ([2, 2, 2, 2], 22, 64), ([1, 3, 0, 0], 23, 7)]
    res = {}
    for share in (False, True):
        pipe = InflightSampler(model, lanes=1, merge=3, share_prompts=share)
        pend = [pipe.submit(4, caps[c], seed=s, sample_offset=o, max_seq_len=n, use_fp16=False, precision='exact', top_k_top=50, top_k_bot=20)
                for c, s, o in steps]
        pipe.drain()
        torch.cuda.synchronize()
        res[share] = [p.get()[:3] for p in pend]
    for i, (a, b) in enumerate(zip(res[False], res[True])):
        assert same(a, b), f'step {i}: the sharing sampler returned other codes or pixels'
    # a step cannot opt out of what its pass does: the setting travels with the sampler keywords, which merged steps must share
    pipe = InflightSampler(model, lanes=1, merge=3, share_prompts=True)
    pipe.submit(4, caps[[0, 0, 1, 0]], seed=1, max_seq_len=n, use_fp16=False)
    with pytest.raises(ValueError, match='merged into one pass must share'):
        pipe.submit(4, caps[[0, 0, 1, 0]], seed=2, max_seq_len=n, use_fp16=False, share_prompts=False)
    pipe.drain()


def test_txt2img_driver_share_prompts_writes_the_usual_files(tmp_path):
    """--share-prompts with --best-of and --guidance-scale: the driver's usual pickles.  The driver samples in FAST, where the prefill of fewer rows may be
    served by other GEMM kernels, so equality with the unshared run is printed, not asserted (EXACT equality: the tests above)."""
    import pickle

    from hqtransformer_amd import sampling_hqmodel_txt2img
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.spec import stage1_spec_from_config, stage2_spec_from_config
    cfg_path = os.path.join(TP.ROOT, 'configs', 'tiny-txt.yaml')
    cfg = load_config(cfg_path)
    R, K = stage1_spec_from_config(cfg).resolution, int(round(stage2_spec_from_config(cfg).ctx_len_img ** 0.5))
    outs = {}
    for share in (False, True):
        out = tmp_path / f'share_{share}'
        sampling_hqmodel_txt2img.main(['-r', str(out), '-m', cfg_path, '--batch_size', '2', '--synthetic-prompts', '3', '--top-k', '64', '--top-resolution', str(K),
                                       '--best-of', '3', '--guidance-scale', '1.5'] + (['--share-prompts'] if share else []))
        outs[share] = []
        for batch, rows in ((1, 2), (2, 1)):                 # three prompts: a batch of two and the shorter last one
            with open(out / f'samples_({batch}_2).pkl', 'rb') as fp:
                px = pickle.load(fp)
            assert px.dtype == np.float32 and px.shape == (rows, 3, R, R) and px.min() >= 0.0 and px.max() <= 1.0
            outs[share].append(px)
    print('shared run equals the unshared one:', all((a == b).all() for a, b in zip(outs[False], outs[True])))
    src = tmp_path / 'images.npy'
    np.save(src, np.zeros((1, 3, R, R), np.float32))
    with pytest.raises(SystemExit, match='--share-prompts and --complete-from'):
        sampling_hqmodel_txt2img.main(['-r', str(tmp_path / 'x'), '-m', cfg_path, '--synthetic-prompts', '2', '--share-prompts', '--complete-from', str(src),
                                       '--keep-rows', '2'])
