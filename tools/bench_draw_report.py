"""What a draw report costs (hqt_set_draw_report): the AR loop of the ImageNet-12L model with synthetic weights in FAST, graphed, one batch-64 call of 64
positions, host wall clock around calls that end in a device synchronise, for
    none        no outputs
    logprobs    the log-probability buffer only           (5 more launches per position: code_logprob)
    report0     a report with N = 0: entropy and rank     (5 more launches per position: draw_report)
    report16    a report with N = 16: the top-16 as well  (the same launches, 16 argmax rounds each)
    both        log-probabilities and the N = 16 report   (the same launches: one kernel writes both)
    fresh16     report16 through sampling_ihqgpt(return_report=16), which allocates the report's tensors per call: the pointers are part of the graph key, so a
                call whose allocator hands out other blocks than the last one captures its graph again
The first five write into buffers allocated once (Engine.sample(logprobs_out=, report_out=)): calls that differ in nothing replay one graph.
One process; the six configurations take turns, `rounds` times, `reps` timed calls a turn after `warmup` untimed ones, so that a drift of the machine
shows up as the spread between the rounds of one configuration and not as a difference between configurations.  There is no pass / fail number.

    python tools/bench_draw_report.py [--rounds 3] [--reps 5] [--warmup 2] [--out profiles/draw_report.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {'none': (False, None), 'logprobs': (True, None), 'report0': (False, 0), 'report16': (False, 16), 'both': (True, 16), 'fresh16': (False, 16)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'draw_report.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd._lib import PRECISION_FAST
    from hqtransformer_amd.engine import new_draw_report
    from hqtransformer_amd.sampling import sampling_ihqgpt
    if not torch.cuda.is_available():
        raise SystemExit('bench_draw_report: no GPU (a time measured elsewhere says nothing about the MI355X)')
    B, n = a.batch, 64
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    cond = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(0))

    eng = m.stage2.engine(B, n)
    logprobs = torch.empty((B, n, 5), dtype=torch.float32, device=eng.device)
    reports = {top_n: new_draw_report(B, n, 5, top_n, eng.device) for top_n in (0, 16)}

    def run(mode):
        lp, top_n = MODES[mode]
        if mode == 'fresh16':
            return sampling_ihqgpt(m.stage2, num_candidates=B, cond=cond, use_fp16=True, is_tqdm=False, max_seq_len=n, seed=100, return_report=top_n)
        return eng.sample(B, cond, n, precision=PRECISION_FAST, seed=100, logprobs_out=logprobs if lp else None, report_out=reports.get(top_n))

    want = run('none')
    for mode in MODES:                               # the codes do not depend on what is reported
        got = run(mode)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), mode
    ms = {mode: [] for mode in MODES}
    for _ in range(a.rounds):
        for mode in MODES:
            for _ in range(a.warmup):
                run(mode)
            torch.cuda.synchronize()
            turn = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                run(mode)
                torch.cuda.synchronize()
                turn.append(round(1000.0 * (time.perf_counter() - t0), 3))
            ms[mode].append(turn)
    m.stage2.range_check()
    med = {mode: statistics.median(t for turn in turns for t in turn) for mode, turns in ms.items()}
    res = {'what': f'tools/bench_draw_report.py --rounds {a.rounds} --reps {a.reps} --warmup {a.warmup} --batch {B}: AR-loop time (ms, host wall clock around a call that ends '
                   f'in a device synchronise) of the ImageNet-12L model with synthetic weights in FAST, graphed, one batch-{B} call of {n} positions on one MI355X; the '
                   'configurations take turns in one process, every list holds the timed calls of one turn.',
           'device': torch.cuda.get_device_name(0), 'launches_per_call_added': {mode: 0 if mode == 'none' else 5 * n for mode in MODES}}
    for mode, turns in ms.items():
        rounds = [statistics.median(t) for t in turns]
        res[mode] = {'ms': turns, 'median_ms': round(med[mode], 3), 'spread_between_rounds_ms': round(max(rounds) - min(rounds), 3),
                     'minus_none_ms': round(med[mode] - med['none'], 3), 'minus_none_percent': round(100.0 * (med[mode] - med['none']) / med['none'], 2),
                     'us_per_added_launch': round(1000.0 * (med[mode] - med['none']) / (5 * n), 2) if mode != 'none' else 0.0}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')
    print(json.dumps({k: (v['median_ms'], v['minus_none_ms']) for k, v in res.items() if isinstance(v, dict) and 'median_ms' in v}))


if __name__ == '__main__':
    main()
