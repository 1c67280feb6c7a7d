"""What pausing a pass costs, and what pruning buys (hqt_set_segment / hqt_select_rows): the benchmark model (configs/imagenet-12l.yaml, synthetic
weights) in FAST, graphed, one lane, B = 64, 64 positions, one process:
    pass                      the 64 positions as 1 plain call, as 1 segment (0, 64), as 8 segments of 8 and as 64 segments of 1
    select_rows               the cache gather at t = 32 for a permutation and for 64 -> 16 rows: time between device events, bytes moved (read + written), GB/s
    best_of                   sample_best_of with 8 candidates of 8 classes (64 rows), keep 1: unpruned against prune=[(16, 4), (32, 2)]; the same with 64
                              classes (512 rows: a pass whose time depends on its row count)
    plain_launches            launches per timing slot of ONE eager plain call under the engine's per-launch timers (hqt_timing_get)
Method: per mode `warmup` runs, then `reps` timed runs between device events on the current stream; median, minimum and maximum; the modes of `pass`
alternate run by run.  `--plain-only` measures the plain call and its launches alone and uses nothing this feature added, so the same file runs on the
parent commit; `--parent FILE` then merges that record into this one and compares the launch counts slot by slot (the plain call must launch the same kernels).

    python tools/bench_segments.py [--out profiles/segments.json] [--reps 7] [--warmup 2] [--plain-only] [--parent parent.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segments.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    p.add_argument('--reps', type=int, default=7)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--plain-only', action='store_true')
    p.add_argument('--parent', default=None)
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hqtransformer_amd._lib import PRECISION_FAST
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    B, n = 64, 64
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    spec = m.stage2.spec
    eng = m.stage2.engine(B, n)
    cond = (torch.arange(B) % spec.n_classes).cuda()
    kw = dict(precision=PRECISION_FAST, seed=100)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1), 3)

    def stats(ms):
        return {'ms': ms, 'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms)}

    outs = [torch.zeros((B, n), dtype=torch.int64, device='cuda'), torch.zeros((B, n, 4), dtype=torch.int64, device='cuda')]

    def segments(k):
        return lambda: [eng.sample(B, cond, n, out=outs, segment=(t, t + k), **kw) for t in range(0, n, k)]

    modes = {'plain_call': lambda: eng.sample(B, cond, n, out=outs, **kw)}
    if not a.plain_only:
        modes.update({'segments_1x64': segments(64), 'segments_8x8': segments(8), 'segments_64x1': segments(1)})
    res = {'what': f'tools/bench_segments.py --reps {a.reps} --warmup {a.warmup}{" --plain-only" if a.plain_only else ""}: the benchmark model (synthetic weights), FAST, '
                   'graphed, one lane, B = 64, 64 positions, one process; times in ms between device events (median, min, max; the modes of `pass` alternate run by '
                   'run, so a mode whose segment length differs from its predecessor\'s re-captures its graph inside its time: that is what a caller pays who mixes them).',
           'pass': {}}
    for fn in modes.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in modes}
    for _ in range(a.reps):
        for k, fn in modes.items():
            ms[k].append(timed(fn))
    if not a.plain_only:                                 # each mode on its own as well: back to back, its graph stays captured
        for k, fn in modes.items():
            fn()
            res['pass'][k + '_alone'] = stats([timed(fn) for _ in range(a.reps)])
    m.stage2.range_check()
    for k in modes:
        res['pass'][k] = stats(ms[k])
    # launches per timing slot of one eager plain call
    eng.timing_reset()
    eng.timing(True)
    eng.sample(B, cond, n, out=outs, **kw)
    torch.cuda.synchronize()
    report = eng.timing_report()
    eng.timing(False)
    eng.timing_reset()
    res['plain_launches'] = {s: int(v[0]) for s, v in sorted(report.items()) if v[0]}
    if not a.plain_only:
        from hqtransformer_amd.pipeline import sample_best_of
        D, layers = spec.embed_dim, spec.n_layers
        res['select_rows'] = {}
        g = torch.Generator().manual_seed(1)
        for name, table in (('permutation_64', torch.randperm(B, generator=g).tolist()), ('subset_64_to_16', list(range(0, B, 4)))):
            ms_sel = []
            for _ in range(a.warmup + a.reps):
                eng.sample(B, cond, n, out=outs, segment=(0, 32), **kw)
                ms_sel.append(timed(lambda: eng.select_rows(table, B)))
                eng.sample(len(table), cond[:len(table)], n, out=[o[:len(table)].contiguous() for o in outs], segment=(32, n), **kw)
            ms_sel = ms_sel[a.warmup:]
            moved = 2 * 2 * layers * len(table) * 32 * D * 2       # K and V, read + written, live rows 0 .. 31, bf16
            line = dict(stats(ms_sel), rows=len(table), t=32, bytes_moved=moved, gb_per_s=round(moved / (statistics.median(ms_sel) * 1e-3) / 1e9, 1))
            res['select_rows'][name] = line
        classes = torch.arange(8)
        bo = dict(use_fp16=True, max_seq_len=n, seed=7)
        many = torch.arange(64)                          # (beyond what the 64-row engine holds: the model rebuilds it for 512 rows, outside the timed runs)
        runs = {'unpruned': lambda: sample_best_of(m.stage2, classes, 8, 1, **bo),
                'pruned_16to4_32to2': lambda: sample_best_of(m.stage2, classes, 8, 1, prune=[(16, 4), (32, 2)], **bo),
                'unpruned_64_classes': lambda: sample_best_of(m.stage2, many, 8, 1, **bo),
                'pruned_16to4_32to2_64_classes': lambda: sample_best_of(m.stage2, many, 8, 1, prune=[(16, 4), (32, 2)], **bo)}
        res['best_of'] = {}
        for k, fn in runs.items():
            for _ in range(a.warmup):
                fn()
            res['best_of'][k] = stats([timed(fn) for _ in range(a.reps)])
        m.stage2.range_check()
    if a.parent:
        with open(a.parent) as fp:
            parent = json.load(fp)
        res['parent'] = {'plain_call': parent['pass']['plain_call'], 'plain_launches': parent['plain_launches']}
        res['plain_launches_equal_parent'] = parent['plain_launches'] == res['plain_launches']
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')


if __name__ == '__main__':
    main()
