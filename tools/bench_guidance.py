"""What guided sampling costs, and that it costs nothing when off: AR-loop time of the ImageNet-12L model in FAST, graphed, one lane, 64 positions, for
    rows64_off      one unguided batch-64 call (the persistent launch per position + the depth chain)
    rows640_off     one unguided merged pass of ten batch-64 steps (640 rows; every step keeps its seed and global offset)
    rows64_guided   32 pairs: the same 64 rows, rows 32 .. 63 the negative condition of rows 0 .. 31 (guidance_scale, one launch more per sub-step)
    rows640_guided  320 pairs in 640 rows
The `off` modes use nothing newer than row_seeds, so the worker also runs in the parent commit's checkout, where it reports only those lines.  The guided modes
also run once eagerly with the engine's timing on and report the launches and the time of the `guide_logits` slot.

Worker (one process, one tree):   python tools/bench_guidance.py --worker [--tree DIR] --modes rows64_off rows640_off [rows64_guided rows640_guided]
    prints one JSON line per mode: the time of every repeat in ms (device events), their median.
Driver (the A/B protocol):        python tools/bench_guidance.py --parent-tree DIR [--rounds 3] [--out profiles/guidance.json]
    DIR = a checkout of the parent commit with its library built.  Runs the parent's worker (`off` modes) and this tree's worker (all four modes) alternately,
    one fresh process each, `rounds` times, and writes the medians of every round, the spread between repeated parent runs and the differences."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ['rows64_off', 'rows640_off', 'rows64_guided', 'rows640_guided']
SCALE = 2.0


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree or ROOT))
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import sampling_ihqgpt
    B, n = 64, 64
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    eng = m.stage2.engine(10 * B, n)
    g = torch.Generator().manual_seed(0)
    cond = torch.randint(0, 1000, (10 * B,), generator=g)

    def run(mode, **more):
        k = 10 if mode.startswith('rows640') else 1
        rows = k * B
        seeds, offs = [100 + s for s in range(k) for _ in range(B)], [i for _ in range(k) for i in range(B)]
        if mode.endswith('_guided'):             # half the rows are images, the other half their negative condition (another class): the same row count
            h = rows // 2
            return sampling_ihqgpt(m.stage2, num_candidates=h, cond=cond[:h], use_fp16=True, is_tqdm=False, max_seq_len=n, seed=100, row_seeds=seeds[:h],
                                   row_offsets=offs[:h], guidance_scale=SCALE, neg_cond=(cond[:h] + 1) % 1000, **more)
        return sampling_ihqgpt(m.stage2, num_candidates=rows, cond=cond[:rows], use_fp16=True, is_tqdm=False, max_seq_len=n, seed=100, row_seeds=seeds,
                               row_offsets=offs, **more)

    for mode in a.modes:
        for _ in range(a.warmup):
            run(mode)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(mode)
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        m.stage2.range_check()
        line = {'mode': mode, 'rows': (10 if mode.startswith('rows640') else 1) * B, 'ar_ms': ms, 'ar_ms_median': statistics.median(ms)}
        if mode.endswith('_guided'):             # the slot's own figures, from one eager pass with device events around every launch
            eng.timing(True)
            eng.timing_reset()
            run(mode)
            torch.cuda.synchronize()
            launches, slot_ms = eng.timing_report().get('guide_logits', (0, 0.0))
            eng.timing(False)
            line.update(guide_logits_launches=int(launches), guide_logits_ms=round(float(slot_ms), 3))
        print(json.dumps(line), flush=True)


def driver(a):
    def one(tree, modes):
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree, '--config', a.config, '--reps', str(a.reps), '--warmup', str(a.warmup),
               '--modes'] + modes
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.worker_timeout)     # a worker that fails or hangs ends the run: nothing is started after it
        if r.returncode != 0:
            raise SystemExit(f'worker failed with status {r.returncode}: {" ".join(cmd)}')
        return {d['mode']: d for d in (json.loads(l) for l in r.stdout.splitlines() if l.startswith('{'))}

    parent, new = [], []
    for _ in range(a.rounds):
        parent.append(one(a.parent_tree, MODES[:2]))
        new.append(one(ROOT, MODES))
    med = lambda runs, mode: [r[mode]['ar_ms_median'] for r in runs]
    res = {'what': f'tools/bench_guidance.py --parent-tree <parent checkout> --rounds {a.rounds} --reps {a.reps} --warmup {a.warmup}: AR-loop time (ms, device events) of the '
                   f'ImageNet-12L model in FAST, graphed, 64 positions; rows64 = one batch-64 call, rows640 = one merged pass of ten batch-64 steps; guided = half the '
                   f'rows are the negative condition of the other half (scale {SCALE}).  The parent commit and this code alternately, one fresh process each; every '
                   'figure is the median of the timed passes of one process.'}
    for rows in ('rows64', 'rows640'):
        p, off, on = med(parent, rows + '_off'), med(new, rows + '_off'), med(new, rows + '_guided')
        spread = max(p) - min(p)
        within = max(max(r[rows + '_off']['ar_ms']) - min(r[rows + '_off']['ar_ms']) for r in parent)
        d_off, d_on = statistics.median(off) - statistics.median(p), statistics.median(on) - statistics.median(off)
        launches = new[-1][rows + '_guided']['guide_logits_launches']
        res[rows] = {'parent_off_ms': p, 'new_off_ms': off, 'new_guided_ms': on,
                     'parent_spread_ms': {'between_rounds': round(spread, 3), 'within_a_run_max': round(within, 3)},
                     'off_minus_parent_ms': round(d_off, 3), 'off_within_spread_of_parent': abs(d_off) <= max(spread, within),
                     'guided_minus_off_ms': round(d_on, 3), 'guided_minus_off_percent': round(100.0 * d_on / statistics.median(off), 2),
                     'guide_logits_launches': launches, 'guide_logits_slot_ms_eager': [r[rows + '_guided']['guide_logits_ms'] for r in new],
                     'us_per_extra_launch': round(1000.0 * d_on / launches, 2) if launches else None}
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--worker', action='store_true')
    p.add_argument('--tree', default=None, help='worker: the checkout whose package is measured (default: this one)')
    p.add_argument('--modes', nargs='+', default=MODES, choices=MODES)
    p.add_argument('--parent-tree', default=None)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--worker-timeout', type=float, default=420.0)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guidance.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    a = p.parse_args()
    if a.worker:
        worker(a)
    elif a.parent_tree:
        driver(a)
    else:
        p.error('give --worker (one tree) or --parent-tree DIR (the A/B run)')


if __name__ == '__main__':
    main()
