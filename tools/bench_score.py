"""What one teacher-forced pass buys over stepwise scoring: time of scoring B = 64 samples of n = 64 positions with the ImageNet-12L model (synthetic
weights) in FAST, one lane, for
    stepwise      score_codes(one_pass=False): one sampler call with every level forced -- n decode steps (the only way before hqt_score; runs in an older checkout)
    chunk64 / chunk1024 / chunk4096      score_codes(one_pass=True, score_chunk=...): hqt_score, the depth head over the 4096 pairs in chunks of that many

Worker (one process, one tree):   python tools/bench_score.py --worker [--tree DIR] --modes stepwise [chunk64 chunk1024 chunk4096]
    prints one JSON line per mode: the time of every repeat in ms (device events), their median, hqt_workspace_bytes of the engine; chunk4096 also its timing slots
    (one extra un-timed-by-events pass with per-launch timers on).
Driver (the A/B protocol):        python tools/bench_score.py --parent-tree DIR [--rounds 3] [--out profiles/score_one_pass.json]
    DIR = a checkout of the parent commit with its library built.  Runs the parent's worker (stepwise) and this tree's worker (all modes) alternately, one fresh
    process each, `rounds` times, and writes every round's medians and the speed-up of each chunk over the parent's stepwise time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ['stepwise', 'chunk64', 'chunk1024', 'chunk4096']


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree or ROOT))
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import score_codes
    B, n = 64, 64
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    g = torch.Generator().manual_seed(0)
    V = m.stage2.spec.vocab_top
    cond = torch.randint(0, 1000, (B,), generator=g)
    codes = [torch.randint(0, V, (B, n), generator=g).cuda(), torch.randint(0, V, (B, n, 4), generator=g).cuda()]

    def run(mode):
        if mode == 'stepwise':
            return score_codes(m.stage2, codes, cond, precision='fast')
        return score_codes(m.stage2, codes, cond, precision='fast', one_pass=True, score_chunk=int(mode[5:]))

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
        eng = m.stage2._engine
        rec = {'mode': mode, 'ms': ms, 'ms_median': statistics.median(ms), 'workspace_bytes': eng.workspace_bytes()}
        if mode == 'chunk4096':
            eng.timing_reset()
            eng.timing(True)
            run(mode)
            torch.cuda.synchronize()
            rec['slots'] = {k: [v[0], round(v[1], 3)] for k, v in sorted(eng.timing_report().items(), key=lambda kv: -kv[1][1]) if not k.startswith('variant:')}
            eng.timing(False)
        print(json.dumps(rec), flush=True)


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
        parent.append(one(a.parent_tree, MODES[:1]))
        new.append(one(ROOT, MODES))
    med = lambda runs, mode: [r[mode]['ms_median'] for r in runs]
    base = statistics.median(med(parent, 'stepwise'))
    res = {'what': f'tools/bench_score.py --parent-tree <parent checkout> --rounds {a.rounds} --reps {a.reps} --warmup {a.warmup}: time (ms, device events) of scoring B = 64 x n = 64 '
                   'given codes with the ImageNet-12L model (synthetic weights) in FAST.  The parent commit (stepwise, its only way) and this code alternately, one fresh '
                   'process each; every figure is the median of the timed passes of one process.',
           'parent_stepwise_ms': med(parent, 'stepwise'), 'parent_stepwise_workspace_bytes': parent[0]['stepwise']['workspace_bytes']}
    for mode in MODES:
        t = med(new, mode)
        res[mode] = {'ms': t, 'ms_median': statistics.median(t), 'speedup_over_parent_stepwise': round(base / statistics.median(t), 3),
                     'workspace_bytes': new[0][mode]['workspace_bytes']}
    res['chunk4096']['slots'] = new[-1]['chunk4096'].get('slots')
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
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_one_pass.json'))
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
