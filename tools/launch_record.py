#!/usr/bin/env python
"""Launch record of the engine: which kernels served a fixed list of calls, and a hash of what they returned.

A refactor of the host side (csrc/engine.hip) must leave both unchanged.  ``--out FILE`` runs the cases on cuda:0 and writes a JSON
record: per case the launch counts of every timing slot (the ``variant:*`` slots included) from one un-graphed pass with timing on,
and a SHA-256 of every array the call returned.  ``--compare A B`` exits 0 iff two records are equal, and names what differs.

    python tools/launch_record.py --out profiles/launch_record_parent.json        # on the parent build
    python tools/launch_record.py --out profiles/launch_record.json               # on this tree
    python tools/launch_record.py --compare profiles/launch_record_parent.json profiles/launch_record.json

Cases: tiny class-conditional, text (prefill), three-level ('parallel-add', 'top2mid2bot') and bidirectional models through
sample / sample3 in EXACT, SPLIT and FAST, persist on and off, eager and graph; one merged pass of 640 rows under the throughput
policy (tiled GEMM, split-K combine, K-sliced SPLIT GEMM); decode and encode in the three precisions on a stage 1 with attention, an
upsampling conv and a nin_shortcut (planes-out, conv_out-direct, the halo conv's fused statistics), one decode with HQT_NO_FUSED_GN=1.

The ``staged/*`` cases (``staged_cases``) cover the calls that stage something on the handle first -- code prefixes, kept positions, row samplers (six calls
back to back through the four-slot pinned ring), guidance, shared prompts, segments with ``select_rows``, rolling passes (``row_positions``: a slot that joins late, rows that end at different calls, a call
over empty slots alone; on a text engine with ``max_joins`` the join phase with two, one and no joiner), draw reports -- and ``score``, on the tiny spec;
``staged/refusals/*`` record the code and text of refused raw-ABI calls (a wrong table, or two tables staged together: which test speaks first) and the
hash of a plain call behind each.

The ``surface/*`` cases record hashes only, with fixed seeds, of what the Python surface above the engine returns on the tiny configs:
``sampling_ihqgpt`` (class / text / bidirectional; every form of ``cond``, ``given_top_code``, ``row_seeds``, 'split', a seed drawn from
torch's generator), ``sampling_hqtransformer``, ``decode_code`` / ``decode_sequences`` (two and three levels, a level missing) and
``InflightSampler`` (3 lanes unmerged, 2 lanes x merge 4; every step's codes and pixels).  A refactor of that surface must leave them unchanged.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRECISIONS = ('exact', 'split', 'fast')


def digest(t) -> str:
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def timed(eng, call):
    """One un-graphed pass with timing on: (launch counts per slot, hashes of the returned arrays)."""
    import torch
    eng.timing(True)
    eng.timing_reset()
    out = call()
    torch.cuda.synchronize()
    counts = {k: v[0] for k, v in sorted(eng.timing_report().items()) if v[0]}
    eng.timing(False)
    eng.range_check()
    return counts, out


def flat(out):
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in (out[k] if isinstance(out[k], (list, tuple)) else [out[k]])]
    return list(out) if isinstance(out, (list, tuple)) else [out]


def sample_cases(rec, name, spec, seed, B, n, policy=None, persist=(True, False)):
    import numpy as np
    import torch
    from hqtransformer_amd import _lib, synth
    from hqtransformer_amd.engine import Engine
    eng = Engine(spec, None, torch.device('cuda:0'), B, spec.ctx_len_img)
    eng.load(stage2=synth.stage2_weights(spec, seed, 'fixture'))
    eng.finalize()
    if policy is not None:
        eng.set_policy(policy)
    draws = 21 if spec.levels == 3 else 5
    noise = torch.from_numpy(np.maximum(np.random.default_rng([seed, 1]).standard_exponential((n, draws, B, spec.vocab_top), dtype=np.float32),
                                        np.float32(1e-30)))
    cond = None
    if spec.cond == 1:
        cond = torch.from_numpy((np.arange(B) * 7) % spec.n_classes)
    elif spec.cond == 2:
        cond = torch.from_numpy(synth.text_ids(seed, B, spec.ctx_len_txt, spec.vocab_txt))
    fn = eng.sample3 if spec.levels == 3 else eng.sample
    for prec in PRECISIONS:
        for on in persist:
            eng.set_persist(on)
            kw = dict(precision=_lib.PRECISIONS[prec], noise=noise, return_logits=True)
            counts, out = timed(eng, lambda: fn(B, cond, n, use_graph=False, **kw))
            graph = fn(B, cond, n, use_graph=True, **kw)
            torch.cuda.synchronize()
            eng.range_check()
            rec[f'{name}/{prec}/persist={int(on)}'] = {'launches': counts, 'eager': [digest(t) for t in flat(out)],
                                                      'graph': [digest(t) for t in flat(graph)]}
    eng.close()


def stage1_cases(rec):
    import numpy as np
    import torch
    from hqtransformer_amd import _lib, synth
    from hqtransformer_amd.engine import Engine
    from hqtransformer_amd.spec import Stage1Spec
    spec = Stage1Spec(ch=128, ch_mult=[1, 1, 2], num_res_blocks=1, attn_resolutions=[16], resolution=128, z_channels=64, embed_dim=32,
                      n_embed=256, use_init_downsample=True)
    B = 3
    eng = Engine(None, spec, torch.device('cuda:0'), B)
    eng.load(stage1=synth.stage1_weights(spec, 41, 'fixture', encoder=True))
    eng.finalize()
    r = np.random.default_rng(42)
    ct = torch.from_numpy(r.integers(0, spec.n_embed, (B, spec.z_res // 2, spec.z_res // 2)))
    cb = torch.from_numpy(r.integers(0, spec.n_embed, (B, spec.z_res, spec.z_res)))
    img = torch.from_numpy(r.uniform(-1, 1, (B, 3, spec.resolution, spec.resolution)).astype(np.float32))
    for prec in PRECISIONS:
        p = _lib.PRECISIONS[prec]
        counts, out = timed(eng, lambda: eng.decode(ct, cb, precision=p))
        rec[f'stage1/decode/{prec}'] = {'launches': counts, 'eager': [digest(t) for t in flat(out)]}
        counts, out = timed(eng, lambda: eng.encode(img, precision=p, want_quant=True, want_resid=True, want_recon=True, want_diff=True))
        rec[f'stage1/encode/{prec}'] = {'launches': counts, 'eager': [digest(t) for t in flat(out)]}
    os.environ['HQT_NO_FUSED_GN'] = '1'                   # read per launch: the halo conv leaves no statistics, a pass computes them
    try:
        counts, out = timed(eng, lambda: eng.decode(ct, cb, precision=_lib.PRECISION_FAST))
    finally:
        del os.environ['HQT_NO_FUSED_GN']
    rec['stage1/decode/fast/no_fused_gn'] = {'launches': counts, 'eager': [digest(t) for t in flat(out)]}
    eng.close()


def surface_cases(rec):
    import torch
    from hqtransformer_amd import synth
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import InflightSampler
    from hqtransformer_amd.sampling import rearrange_codes, rearrange_codes3, sampling_hqtransformer, sampling_ihqgpt

    def model(name, *overrides, seed):
        return ImageGPT2(load_config(os.path.join(ROOT, 'configs', name), list(overrides)), seed=seed).to('cuda').eval()

    def put(case, tensors):
        torch.cuda.synchronize()
        rec['surface/' + case] = {'hashes': [None if t is None else digest(t) for t in tensors]}

    B = 3
    cls, txt, l3 = model('tiny-cls.yaml', seed=3), model('tiny-txt.yaml', seed=4), model('tiny-l3.yaml', seed=9)
    bidir = model('tiny-cls.yaml', 'stage2.type=hq-transformer/bidirectional4', seed=5)
    prompts = torch.from_numpy(synth.text_ids(6, B, txt.stage2.spec.ctx_len_txt, txt.stage2.spec.vocab_txt))
    quality = dict(top_k_top=100, top_p_top=0.9, top_k_bot=50, top_p_bot=None, softmax_temperature=[1.0, 0.9])
    for name, m, cond in (('class', cls, 7), ('text', txt, prompts), ('bidirectional', bidir, 7)):
        for fp16 in (False, True):
            put(f'ihqgpt/{name}/fp16={int(fp16)}', sampling_ihqgpt(m.stage2, B, cond, use_fp16=fp16, is_tqdm=False, max_seq_len=64, seed=21, **quality))
        put(f'ihqgpt/{name}/split', sampling_ihqgpt(m.stage2, B, cond, is_tqdm=False, max_seq_len=16, seed=22, precision='split'))
        torch.manual_seed(23)                     # seed=None: one draw from torch's generator per call
        put(f'ihqgpt/{name}/torch_seed', [*sampling_ihqgpt(m.stage2, B, cond, is_tqdm=False, max_seq_len=16),
                                          *sampling_ihqgpt(m.stage2, B, cond, is_tqdm=False, max_seq_len=16), torch.randint(0, 2 ** 62, (1,))])
    for form, cond in (('one', torch.tensor([7])), ('each', torch.tensor([1, 5, 9]))):
        put(f'ihqgpt/class/cond={form}', sampling_ihqgpt(cls.stage2, B, cond, use_fp16=False, is_tqdm=False, max_seq_len=16, seed=24))
    given = torch.arange(16).reshape(1, 16) % 7
    put('ihqgpt/class/given_top_code', sampling_ihqgpt(cls.stage2, B, 7, use_fp16=False, is_tqdm=False, max_seq_len=16, seed=25, given_top_code=given))
    put('ihqgpt/class/row_seeds', sampling_ihqgpt(cls.stage2, B, torch.tensor([1, 5, 9]), use_fp16=False, is_tqdm=False, max_seq_len=16,
                                                 seed=29, row_seeds=[31, 32, 31], row_offsets=[0, 4, 2]))
    codes2 = sampling_ihqgpt(cls.stage2, B, 7, use_fp16=False, is_tqdm=False, max_seq_len=64, seed=26)
    for fp16 in (False, True):
        put(f'hqtransformer/fp16={int(fp16)}', sampling_hqtransformer(l3.stage2, B, 123, top_k=[100, 50, None], top_p=[0.9, None, None],
                                                                     softmax_temperature=[1.0, 0.9, 0.8], use_fp16=fp16, is_tqdm=False, max_seq_len=16, seed=27))
    codes3 = sampling_hqtransformer(l3.stage2, B, 123, use_fp16=False, is_tqdm=False, max_seq_len=16, seed=28)
    grids2, grids3 = rearrange_codes(*codes2, 8), list(rearrange_codes3(codes3, 4))
    for prec in PRECISIONS:
        put(f'decode/l2/{prec}', [cls.stage1.decode_code(*grids2, precision=prec), cls.stage1.decode_code(None, grids2[1], precision=prec),
                                  cls.stage1.decode_code(grids2[0], None, precision=prec, clamp01=True),
                                  cls.stage1.decode_sequences(*codes2, precision=prec), cls.stage1.decode_sequences(codes2[0], None, precision=prec, clamp01=True)])
        put(f'decode/l3/{prec}', [l3.stage1.decode_code(grids3, precision=prec), l3.stage1.decode_code([None, grids3[1], grids3[2]], precision=prec),
                                  l3.stage1.decode_code([grids3[0], None, None], precision=prec, clamp01=True),
                                  l3.stage1.decode_sequences(codes3, precision=prec), l3.stage1.decode_sequences([codes3[0], codes3[1], None], precision=prec, clamp01=True)])
        cls.stage1.range_check()
        l3.stage1.range_check()
    l3_quality = dict(top_k=[100, 50, None], top_p=[0.9, None, None], softmax_temperature=[1.0, 0.9, 0.8])
    for name, m, n_pos, conds, kw in (('class', cls, 64, [3, torch.tensor([4]), torch.tensor([1, 5, 9]), 6, 8], quality),
                                      ('l3', l3, 16, [3, torch.tensor([4]), torch.tensor([1, 5, 9]), 6, 8], l3_quality),
                                      ('text', txt, 64, [prompts.roll(k, 0) for k in range(5)], quality)):
        for lanes, merge in ((3, 1), (2, 4)):
            for fp16 in (False, True):
                pipe = InflightSampler(m, lanes=lanes, merge=merge)
                steps = [pipe.submit(B, c, seed=40 + k, max_seq_len=n_pos, use_fp16=fp16, sample_offset=k, **kw) for k, c in enumerate(conds)]
                pipe.drain()
                out = []
                for st in steps:
                    ct, cb, px, _ = st.get() if merge > 1 else st
                    out += [ct, *(cb if isinstance(cb, (list, tuple)) else [cb]), px]
                put(f'inflight/{name}/lanes={lanes}/merge={merge}/fp16={int(fp16)}', out)
                pipe.release(B, n_pos)


def flat_all(out):
    """Every tensor of a nest of lists / tuples, in order."""
    return [t for o in out for t in flat_all(o)] if isinstance(out, (list, tuple)) else [out]


def staged_cases(rec, tiny):
    """``staged/*``: the calls that stage something on the handle first (row samplers, log-probabilities, guidance, prefixes, kept positions, shared prompts,
    segments with select_rows, rolling passes, draw reports) and ``score``, on the tiny spec with B = 4, n = 6, max_prefix = 5 and score_chunk = 5 (24 pairs: chunks of 5, 5, 5, 5, 4).
    Draws are keyed (no ``noise``): the per-row keys travel with the tables.  ``staged/refusals/*``: refused raw-ABI calls, their code and text, and
    the hash of a plain call behind each -- nothing was left staged."""
    import ctypes as C
    import numpy as np
    import torch
    from hqtransformer_amd import _lib, synth
    from hqtransformer_amd.engine import Engine, guide_pair_table, row_sampler_table
    from hqtransformer_amd.spec import Stage2Spec
    dev = torch.device('cuda:0')
    B, n, P, V = 4, 6, 2, tiny['vocab_top']
    specs = {'class': Stage2Spec(**tiny), 'text': Stage2Spec(**dict(tiny, cond=2, n_classes=0)),
             'l3_parallel_add': Stage2Spec(**tiny, levels=3, depth_decoding='parallel-add'), 'bidirectional': Stage2Spec(**tiny, depth_decoding='bidirectional')}
    specs['text_joins'] = specs['text']              # the text model on an engine of its own, built with max_joins = 2 (rolling passes; 'text' stays without)
    engines = {}

    def engine(model):
        if model not in engines:
            spec = specs[model]
            eng = engines[model] = Engine(spec, None, dev, B, spec.ctx_len_img, max_prefix=5, score_chunk=5, max_joins=2 if model == 'text_joins' else 0)
            eng.load(stage2=synth.stage2_weights(spec, 60 + len(engines), 'fixture'))
            eng.finalize()
        return engines[model]

    def cond_of(model, rows=B):
        spec = specs[model]
        if spec.cond == 2:
            return torch.from_numpy(synth.text_ids(71, rows, spec.ctx_len_txt, spec.vocab_txt))
        return torch.from_numpy((np.arange(rows) * 7) % spec.n_classes)

    def codes_of(model, seed):
        r = np.random.default_rng([seed, 2])
        return [torch.from_numpy(r.integers(0, V, (B, n) + ((4 ** l,) if l else ()))) for l in range(specs[model].levels)]

    def put(case, model, call, precs=('exact', 'fast'), graph=True, persist=None):
        """``call(precision, use_graph)`` -> tensors: launch counts and hashes of the eager pass, hashes of the graphed one."""
        eng = engine(model)
        for prec in precs:
            for on in (True,) if persist is None else persist:
                eng.set_persist(on)
                counts, out = timed(eng, lambda: call(_lib.PRECISIONS[prec], False))
                entry = {'launches': counts, 'eager': [digest(t) for t in flat_all(out)]}
                if graph:
                    out = call(_lib.PRECISIONS[prec], True)
                    torch.cuda.synchronize()
                    eng.range_check()
                    entry['graph'] = [digest(t) for t in flat_all(out)]
                rec[f'staged/{case}/{model}/{prec}' + ('' if persist is None else f'/persist={int(on)}')] = entry
        eng.set_persist(True)

    def fn_of(model):
        return engine(model).sample3 if specs[model].levels == 3 else engine(model).sample

    for model in ('class', 'text', 'l3_parallel_add'):
        prefix = [c[:, :P].contiguous() for c in codes_of(model, 81)]
        put('prefix', model, lambda p, g, m=model, px=prefix: fn_of(m)(B, cond_of(m), n, precision=p, use_graph=g, seed=82, prefix=px,
                                                                       return_logits=True, return_logprobs=True))
    # every row keeps position 0 (the shared leading run: the prefix prefill); beyond it the rows differ
    mask = np.zeros((B, n), dtype=bool)
    mask[:, 0] = True
    mask[0, 3] = mask[1, 4] = mask[2, 2] = mask[2, 5] = True
    for model in ('class', 'l3_parallel_add'):
        put('keep', model, lambda p, g, m=model: fn_of(m)(B, cond_of(m), n, precision=p, use_graph=g, seed=83, keep=(mask, codes_of(m, 84)), return_logits=True))
    pairs = [(0, 2, 1.5), (1, 3, 2.0)]
    paired = [0, 1, 0, 1]                            # both rows of a pair keep the same positions and codes
    put('keep_guided', 'class', lambda p, g: fn_of('class')(B, cond_of('class'), n, precision=p, use_graph=g, seed=85, guidance=pairs,
                                                             keep=(mask[paired], [c[paired].contiguous() for c in codes_of('class', 84)])))
    table = [((1.0, 0.9), (100, 50), None), ((0.8, 1.0), (None, 20), None), ((1.0, 1.0), None, (0.9, None)), ((1.1, 0.7), (10, None), None)]
    put('row_samplers', 'class', lambda p, g: fn_of('class')(B, cond_of('class'), n, precision=p, use_graph=g, seed=86, row_samplers=table), precs=('exact',))
    put('row_samplers', 'class', lambda p, g: fn_of('class')(B, cond_of('class'), n, precision=p, use_graph=g, seed=86, row_samplers=table), precs=('fast',),
        persist=(True, False))
    put('row_samplers', 'bidirectional', lambda p, g: fn_of('bidirectional')(B, cond_of('bidirectional'), n, precision=p, use_graph=g, seed=87, row_samplers=table))
    # six calls, four ring slots, no synchronisation in between: the fifth and sixth rewrite a slot behind a copy that may still be pending
    put('ring', 'class', lambda p, g: [fn_of('class')(B, cond_of('class'), n, precision=p, use_graph=g, seed=90 + k, row_samplers=table[k % B:] + table[:k % B],
                                                      row_seeds=[90 + k] * B, row_offsets=[(b + k) % B for b in range(B)]) for k in range(6)])
    put('guidance', 'class', lambda p, g: fn_of('class')(B, cond_of('class'), n, precision=p, use_graph=g, seed=88, guidance=pairs, return_logprobs=True))
    groups = torch.tensor([0, 1, 1, 0])
    put('prompt_groups', 'text', lambda p, g: fn_of('text')(B, cond_of('text', 2), n, precision=p, use_graph=g, seed=89, prompt_groups=groups))

    def segments(model, p, g):
        spec, eng, draws = specs[model], engine(model), 5
        shared = dict(prompt_groups=groups) if spec.cond == 2 else {}
        cond = cond_of(model, 2) if shared else cond_of(model)
        outs = [torch.zeros((B, n) + ((4 ** l,) if l else ()), dtype=torch.int64, device=dev) for l in range(spec.levels)]
        lg, lp = torch.zeros((n, draws, B, V), device=dev), torch.zeros((B, n, draws), device=dev)
        kw = dict(precision=p, use_graph=g, seed=91)
        eng.sample(B, cond, n, segment=(0, 2), out=outs, logits_out=lg, logprobs_out=lp, **shared, **kw)
        eng.sample(B, cond[groups] if shared else cond, n, segment=(2, 4), out=outs, logits_out=lg, logprobs_out=lp, **kw)
        rows = [2, 0, 0]
        eng.select_rows(rows, paused_batch=B)
        outs3, lg3, lp3 = [o[rows].contiguous() for o in outs], lg[:, :, rows].contiguous(), lp[rows].contiguous()
        eng.sample(len(rows), (cond[groups] if shared else cond)[rows], n, segment=(4, 6), out=outs3, logits_out=lg3, logprobs_out=lp3,
                   row_seeds=[91] * len(rows), row_offsets=rows, **kw)
        return [outs, lg, lp, outs3, lg3, lp3]
    for model in ('class', 'text'):
        put('segments', model, lambda p, g, m=model: segments(m, p, g))
    for model in ('class', 'text', 'bidirectional', 'l3_parallel_add'):
        put('score', model, lambda p, g, m=model: [engine(m).score(B, cond_of(m), [c[:, :k].contiguous() for c in codes_of(m, 92)], precision=p, return_logits=True)
                                                   for k in (n, 1)], graph=False)

    def rolling(case, model, tables, seed):
        """A rolling pass (``row_positions``) of k = 2 steps per call on one set of ``out`` tensors, one call per table: a launch dict per call (and their sum, which
        ``check_coverage`` reads) and the hash of ``out`` after every call, eager and graphed."""
        eng, spec = engine(model), specs[model]

        def calls(p, g, each):
            outs = [torch.zeros((B, n) + ((4 ** l,) if l else ()), dtype=torch.int64, device=dev) for l in range(spec.levels)]
            lp = torch.zeros((B, n, (4 ** spec.levels - 1) // 3), device=dev)
            seen = []
            for pos in tables:
                each(lambda: fn_of(model)(B, cond_of(model), n, precision=p, use_graph=g, seed=seed, out=outs, logprobs_out=lp, row_positions=(pos, 2)))
                torch.cuda.synchronize()
                seen += [digest(t) for t in outs + [lp]]
            return seen
        for prec in ('exact', 'fast'):
            per_call = []
            eager = calls(_lib.PRECISIONS[prec], False, lambda call: per_call.append(timed(eng, call)[0]))
            graph = calls(_lib.PRECISIONS[prec], True, lambda call: call())
            eng.range_check()
            total = {}
            for counts in per_call:
                for slot, v in counts.items():
                    total[slot] = total.get(slot, 0) + v
            rec[f'staged/{case}/{model}/{prec}'] = {'launches': total, 'launches_per_call': per_call, 'eager': eager, 'graph': graph}

    # a slot joins late (slot 2, in call 2), rows end at different calls (slots 0, 1, 3 in call 3; slot 2 is left at position 4), and a call over empty slots alone
    for k, model in enumerate(('class', 'l3_parallel_add', 'bidirectional')):
        rolling('rolling', model, [[0, 0, -1, 0], [2, 2, 0, 2], [4, 4, 2, 4], [-1, -1, -1, -1]], 94 + k)
    # text, max_joins = 2: a joiner draws position 0 in its prompt prefill and then the k steps, so it stands at 1 + k = 3 behind its first call.  Two joiners; ONE
    # joiner next to two continuing rows; no joiner (slots 0 and 1 draw their last position, 5, in the first step and idle in the second)
    # and a last call in which slot 2 draws position 5: the pass is over, as behind the all-empty call above (the next precision begins a pass of its own)
    rolling('rolling_txt', 'text_joins', [[0, 0, -1, -1], [3, 3, 0, -1], [5, 5, 3, -1], [-1, -1, 5, -1]], 97)

    def report(model, p, g, score=False):
        from hqtransformer_amd.engine import new_draw_report
        eng, draws = engine(model), 5
        if score:
            rep = new_draw_report(B, n, draws, 3, dev)
            return [eng.score(B, cond_of(model), codes_of(model, 92), precision=p, report_out=rep), list(rep)]
        reps = [new_draw_report(B, n, draws, 3, dev) for _ in range(2)]
        return [eng.sample(B, cond_of(model), n, precision=p, use_graph=g, seed=98, report_out=reps[0]), list(reps[0]),
                eng.sample(B, cond_of(model), n, precision=p, use_graph=g, seed=98, report_out=reps[1], return_logprobs=True), list(reps[1])]
    for model in ('class', 'bidirectional'):
        put('report', model, lambda p, g, m=model: report(m, p, g))
    put('report_score', 'class', lambda p, g: report('class', p, g, score=True), graph=False)

    # ---- refusals, through the C ABI: what the Python surface checks first never reaches the library
    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def raw_sample(eng, model, rows=B, prefix_len=None, opts=True, force_top=False):
        o = _lib.hqt_sample_opts()
        o.precision, o.n_steps, o.temperature_top, o.temperature_bot, o.seed = _lib.PRECISION_EXACT, n, 1.0, 1.0, 5
        cond = cond_of(model, rows).to(dev)
        outs = [torch.zeros((rows, n), dtype=torch.int64, device=dev), torch.zeros((rows, n, 4), dtype=torch.int64, device=dev)]
        forced = torch.zeros((rows, n), dtype=torch.int64, device=dev)
        head = [eng.h, rows, ptr(cond), C.byref(o) if opts else None, None]
        tail = [ptr(forced) if force_top else None, None, None, ptr(outs[0]), ptr(outs[1]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)]
        if prefix_len is None:
            return eng.lib.hqt_sample(*head, *tail)
        px = [torch.zeros((rows, prefix_len), dtype=torch.int64, device=dev), torch.zeros((rows, prefix_len, 4), dtype=torch.int64, device=dev)]
        return eng.lib.hqt_sample_prefix(*head, prefix_len, ptr(px[0]), ptr(px[1]), *tail)

    def raw_score(eng, model):
        codes = [c.to(dev) for c in codes_of(model, 92)]
        cond, lp = cond_of(model).to(dev), torch.zeros((B, n, 5), device=dev)
        return eng.lib.hqt_score(eng.h, B, ptr(cond), (C.c_void_p * 3)(*[c.data_ptr() for c in codes]), n, _lib.PRECISION_EXACT, ptr(lp), None,
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def set_rows(eng, rows, entries=table):
        t = row_sampler_table(2, entries[:rows])
        return eng.lib.hqt_set_row_samplers(eng.h, rows, t.ctypes.data_as(C.POINTER(_lib.hqt_row_sampler)))

    def set_pos(eng, pos, k=2):
        p = np.asarray(pos, dtype=np.int32)
        return eng.lib.hqt_set_row_positions(eng.h, len(p), p.ctypes.data_as(C.c_void_p), k)

    def set_pair(eng, pos_row, neg_row):
        return eng.lib.hqt_set_guidance(eng.h, 1, guide_pair_table(2, [(pos_row, neg_row, 1.5)]))

    def set_keep(eng, rows):
        m = np.ones((rows, n), dtype=np.uint8)
        kept = [torch.zeros((rows, n), dtype=torch.int64, device=dev), torch.zeros((rows, n, 4), dtype=torch.int64, device=dev)]
        return eng.lib.hqt_set_keep_mask(eng.h, rows, n, m.ctypes.data_as(C.c_void_p), (C.c_void_p * 3)(*[t.data_ptr() for t in kept]))

    def set_groups(eng, table_):
        g = np.asarray(table_, dtype=np.int32)
        return eng.lib.hqt_set_prompt_groups(eng.h, len(g), 2, g.ctypes.data_as(C.c_void_p))

    def set_logprob(eng):
        eng._refusal_buf = torch.zeros((B, n, 5), device=dev)
        return eng.lib.hqt_set_logprob_out(eng.h, ptr(eng._refusal_buf))

    refusals = [
        ('row_table_wrong_B', 'class', lambda e: set_rows(e, 3), lambda e: raw_sample(e, 'class')),
        ('keep_table_wrong_B', 'class', lambda e: set_keep(e, 3), lambda e: raw_sample(e, 'class')),
        ('group_table_wrong_B', 'text', lambda e: set_groups(e, [0, 1, 1]), lambda e: raw_sample(e, 'text')),
        ('segment_on_prefix_entry', 'class', lambda e: e.lib.hqt_set_segment(e.h, 0, 2), lambda e: raw_sample(e, 'class', prefix_len=P)),
        ('continuation_without_pass', 'class', lambda e: e.lib.hqt_set_segment(e.h, 2, 4), lambda e: raw_sample(e, 'class')),
        ('groups_with_prefix', 'text', lambda e: set_groups(e, [0, 1, 1, 0]), lambda e: raw_sample(e, 'text', prefix_len=P)),
        ('keep_on_prefix_entry', 'class', lambda e: set_keep(e, B), lambda e: raw_sample(e, 'class', prefix_len=P)),
        ('guidance_row_outside_B', 'class', lambda e: e.lib.hqt_set_guidance(e.h, 1, guide_pair_table(2, [(0, 5, 1.5)])), lambda e: raw_sample(e, 'class')),
        ('null_opts_behind_table', 'class', lambda e: set_rows(e, B), lambda e: raw_sample(e, 'class', opts=False)),
        ('score_behind_row_table', 'class', lambda e: set_rows(e, B), lambda e: raw_score(e, 'class')),
        ('score_behind_logprob_and_segment', 'class', lambda e: set_logprob(e) or e.lib.hqt_set_segment(e.h, 0, 2), lambda e: raw_score(e, 'class')),
        # not a refusal: a segment alone is cleared by hqt_score without one, and the plain call behind it runs all n positions
        ('score_behind_segment_alone', 'class', lambda e: e.lib.hqt_set_segment(e.h, 0, 2), lambda e: raw_score(e, 'class')),
        # two things staged together, or a wrong one: which of sample_call's tests speaks first.  (No case of a draw report whose top_n exceeds the
        # vocabulary: top_n is at most HQT_REPORT_MAX_TOP = 16 and the tiny spec has 512 codes.)
        ('segment_with_keep', 'class', lambda e: e.lib.hqt_set_segment(e.h, 0, 2) or set_keep(e, B), lambda e: raw_sample(e, 'class')),
        ('later_segment_with_groups', 'text', lambda e: e.lib.hqt_set_segment(e.h, 2, 4) or set_groups(e, [0, 1, 1, 0]), lambda e: raw_sample(e, 'text')),
        ('positions_with_segment', 'class', lambda e: set_pos(e, [0, 0, 0, 0]) or e.lib.hqt_set_segment(e.h, 0, 2), lambda e: raw_sample(e, 'class')),
        ('positions_with_keep', 'class', lambda e: set_pos(e, [0, 0, 0, 0]) or set_keep(e, B), lambda e: raw_sample(e, 'class')),
        ('positions_with_groups', 'text_joins', lambda e: set_pos(e, [0, 0, -1, -1]) or set_groups(e, [0, 1, 1, 0]), lambda e: raw_sample(e, 'text_joins')),
        ('positions_wrong_B', 'class', lambda e: set_pos(e, [0, 0, 0]), lambda e: raw_sample(e, 'class')),
        ('positions_k_beyond_n', 'class', lambda e: set_pos(e, [0, 0, 0, 0], k=n + 1), lambda e: raw_sample(e, 'class')),
        ('positions_pair_with_empty_slot', 'class', lambda e: set_pos(e, [0, -1, 0, 0]) or set_pair(e, 0, 1), lambda e: raw_sample(e, 'class')),
        # (the pair speaks before the slot bookkeeping: position 3 continues nothing on this handle)
        ('positions_pair_apart', 'class', lambda e: set_pos(e, [0, 3, 0, 0]) or set_pair(e, 0, 1), lambda e: raw_sample(e, 'class')),
        ('positions_continue_without_pass', 'class', lambda e: set_pos(e, [3, 0, 0, 0]), lambda e: raw_sample(e, 'class')),
        # refused where it is staged (staged_rc != 0): nothing is staged, and the call behind it is a plain one
        ('positions_on_text_without_max_joins', 'text', lambda e: set_pos(e, [0, 0, -1, -1]), lambda e: raw_sample(e, 'text')),
        ('positions_three_joiners', 'text_joins', lambda e: set_pos(e, [0, 0, 0, -1]), lambda e: raw_sample(e, 'text_joins')),
        ('positions_on_prefix_entry', 'class', lambda e: set_pos(e, [0, 0, 0, 0]), lambda e: raw_sample(e, 'class', prefix_len=P)),
        ('keep_with_force_top', 'class', lambda e: set_keep(e, B), lambda e: raw_sample(e, 'class', force_top=True)),
        ('row_table_temperature_0', 'class', lambda e: set_rows(e, B, [((0.0, 1.0), None, None)] + table[1:]), lambda e: raw_sample(e, 'class')),
    ]
    for name, model, stage, call in refusals:
        eng = engine(model)
        with torch.cuda.device(dev):
            staged_rc = stage(eng)
            rc = call(eng)
            text = eng.lib.hqt_last_error().decode() if rc != 0 else ''
        after = fn_of(model)(B, cond_of(model), n, precision=_lib.PRECISION_EXACT, use_graph=False, seed=93)
        torch.cuda.synchronize()
        rec[f'staged/refusals/{name}'] = {'staged_rc': int(staged_rc), 'rc': int(rc), 'error': text, 'after': [digest(t) for t in flat_all(after)]}
    for eng in engines.values():
        eng.close()


def record() -> dict:
    from hqtransformer_amd import _lib
    from hqtransformer_amd.spec import Stage2Spec
    tiny = dict(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=64,
                ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    rec = {}
    sample_cases(rec, 'class', Stage2Spec(**tiny), 11, 3, 6)
    sample_cases(rec, 'text', Stage2Spec(**dict(tiny, cond=2, n_classes=0)), 12, 3, 4)
    sample_cases(rec, 'l3_parallel_add', Stage2Spec(**tiny, levels=3, depth_decoding='parallel-add'), 13, 3, 3)
    sample_cases(rec, 'l3_top2mid2bot', Stage2Spec(**tiny, levels=3, depth_decoding='top2mid2bot'), 14, 3, 3)
    sample_cases(rec, 'bidirectional', Stage2Spec(**tiny, depth_decoding='bidirectional'), 15, 3, 4)
    wide = Stage2Spec(embed_dim=1536, n_layers=1, n_heads=24, n_layers_depth=1, vocab_top=8192, vocab_bot=8192, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=1000, cond=1, embedding=0)
    sample_cases(rec, 'merged640', wide, 31, 640, 2, policy=_lib.POLICY_THROUGHPUT, persist=(True,))
    staged_cases(rec, tiny)
    stage1_cases(rec)
    surface_cases(rec)
    return rec


# what the case list exists to reach: a record that misses one of these ran something else than it claims
COVERAGE = {
    'merged640/fast/persist=1': ('variant:tile_gemm', 'splitk', 'gemm_combine'),
    'merged640/split/persist=1': ('variant:split_gemm_kslices',),
    'stage1/decode/split': ('variant:conv3x3_planes_out', 'variant:conv_out_direct'),
    'stage1/decode/fast': ('gn_apply',),
    'staged/prefix/class/exact': ('embed_prefix', 'code_logprob'),
    'staged/prefix/text/fast': ('embed_prefix', 'code_logprob'),
    'staged/prefix/l3_parallel_add/exact': ('embed_prefix', 'code_logprob'),
    'staged/keep/class/exact': ('embed_prefix',),
    'staged/keep_guided/class/fast': ('embed_prefix', 'guide_logits'),
    'staged/row_samplers/class/fast/persist=1': ('persist_position',),
    'staged/row_samplers/bidirectional/exact': ('bidir_sampler_top', 'bidir_head_ln'),
    'staged/guidance/class/exact': ('guide_logits', 'code_logprob'),
    'staged/prompt_groups/text/exact': ('prompt_fanout',),
    'staged/segments/class/fast': ('kv_gather_rows', 'code_logprob'),
    'staged/segments/text/exact': ('kv_gather_rows', 'prompt_fanout'),
    'staged/score/class/exact': ('score_logprob', 'embed_prefix', 'score_depth_input'),
    'staged/score/text/fast': ('score_logprob', 'embed_prefix'),
    'staged/score/bidirectional/fast': ('score_logprob', 'bidir_head_ln'),
    'staged/score/l3_parallel_add/exact': ('score_logprob',),
    # rolling passes: the decode steps under per-row positions with their log-probabilities (a rolling call runs no prefill ...)
    'staged/rolling/class/exact': ('sampler', 'code_logprob', '!embed_prefix'),
    'staged/rolling/class/fast': ('sampler', 'code_logprob'),
    'staged/rolling/l3_parallel_add/exact': ('sampler', 'code_logprob'),
    'staged/rolling/bidirectional/fast': ('bidir_sampler_top', 'bidir_head_ln'),
    # ... but the join phase of a text pass: the joiners' prompts through the staging and the fan-out
    'staged/rolling_txt/text_joins/exact': ('prompt_fanout',),
    'staged/rolling_txt/text_joins/fast': ('prompt_fanout',),
    # a draw report takes code_logprob's place, also where log-probabilities are asked for
    'staged/report/class/exact': ('draw_report', '!code_logprob'),
    'staged/report/class/fast': ('draw_report', '!code_logprob'),
    'staged/report/bidirectional/exact': ('draw_report', '!code_logprob'),
    'staged/report_score/class/exact': ('draw_report', 'score_logprob'),
}


def check_coverage(rec: dict) -> list:
    """A needle names a slot the case must have launched; '!needle' one it must not have."""
    miss = []
    for case, needles in COVERAGE.items():
        slots = ' '.join(rec[case]['launches'])
        miss += [f'{case}: no slot matching {n!r}' for n in needles if not n.startswith('!') and n not in slots]
        miss += [f'{case}: a slot matching {n[1:]!r}' for n in needles if n.startswith('!') and n[1:] in slots]
    return miss


def compare(a: dict, b: dict) -> list:
    diff = [f'case only in one record: {k}' for k in sorted(set(a) ^ set(b))]
    for k in sorted(set(a) & set(b)):
        for field in sorted(set(a[k]) | set(b[k])):
            if a[k].get(field) != b[k].get(field):
                what = a[k].get(field), b[k].get(field)
                if field == 'launches' and all(isinstance(w, dict) for w in what):
                    slots = sorted(s for s in set(what[0]) | set(what[1]) if what[0].get(s) != what[1].get(s))
                    diff.append(f'{k}: launches differ in ' + ', '.join(f'{s} ({what[0].get(s, 0)} vs {what[1].get(s, 0)})' for s in slots))
                else:
                    diff.append(f'{k}: {field} differs')
    return diff


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', help='run the cases on cuda:0 and write the record here')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'), help='compare two records')
    args = ap.parse_args(argv)
    if bool(args.out) == bool(args.compare):
        ap.error('give --out FILE or --compare A B')
    if args.compare:
        recs = []
        for path in args.compare:
            with open(path) as fp:
                recs.append(json.load(fp))
        diff = compare(*recs)
        print('\n'.join(diff) if diff else f'equal: {len(recs[0])} cases, launch counts and hashes')
        return 1 if diff else 0
    rec = record()
    miss = check_coverage(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fp:
        json.dump(rec, fp, indent=1, sort_keys=True)
        fp.write('\n')
    print(f'{len(rec)} cases -> {args.out}')
    if miss:
        print('the case list no longer reaches what it is there for:\n' + '\n'.join(miss), file=sys.stderr)
    return 2 if miss else 0


if __name__ == '__main__':
    sys.exit(main())
