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
