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
    stage1_cases(rec)
    surface_cases(rec)
    return rec


# what the case list exists to reach: a record that misses one of these ran something else than it claims
COVERAGE = {
    'merged640/fast/persist=1': ('variant:tile_gemm', 'splitk', 'gemm_combine'),
    'merged640/split/persist=1': ('variant:split_gemm_kslices',),
    'stage1/decode/split': ('variant:conv3x3_planes_out', 'variant:conv_out_direct'),
    'stage1/decode/fast': ('gn_apply',),
}


def check_coverage(rec: dict) -> list:
    miss = []
    for case, needles in COVERAGE.items():
        slots = ' '.join(rec[case]['launches'])
        miss += [f'{case}: no slot matching {n!r}' for n in needles if n not in slots]
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
