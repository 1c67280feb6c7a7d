"""What the join run buys completion requests in a rolling pass (hqt_set_join_run / pipeline.RollingSampler(join_run=)): the benchmark model
(configs/imagenet-12l.yaml, synthetic weights) in FAST, graphed, AR loop only (no decode), n = 64 positions per image.  Every request keeps the top half of its
grid (a leading run of 32 positions, random codes) and draws the rest; requests arrive 16 at a time, one group every 16 positions of the pass:
    join_run_32  ONE rolling pass of 64 slots with join_run=32: a group prefills its run in the join phase of the call that admits it (32 + 1 + 16 positions in
                 that call) and finishes in the next.  The pass itself is the clock: a group "arrives" when the call that admits it begins.
    join_run_0   the same pass with join_run=0: the kept positions are forced steps, a request occupies its slot for all 64 positions.
    lanes        what the code could do before: each group of 16 a prefix call (prefix_codes of 32 positions) on the next lane of an InflightSampler (4 lanes),
                 submitted at the wall-clock offsets at which the join_run_32 run admitted its groups (the same arrival process, replayed).
Per mode `--repeat` runs; reported is the run with the median images/s (over the whole run, first arrival to last result) with the latency of its requests,
arrival to the host seeing its group finished (mean, median, max), and the images/s of every run.  Separately: the time of a 16-step call over 16 live rows in which 16 rows of run 32 join, against the same call without joiners (medians of `--repeat`
runs after warm-up): the cost of the join phase.  One process, host wall clock; `warmup` groups run through each mode first (graphs captured, lanes built).

    python tools/bench_rolling_keep.py [--out profiles/rolling_keep.json] [--groups 16] [--warmup 5] [--repeat 7]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, N, GROUP, RUN = 64, 64, 16, 32


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rolling_keep.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    p.add_argument('--groups', type=int, default=16)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeat', type=int, default=7)
    a = p.parse_args()
    if a.repeat < 7:
        p.error('--repeat: medians of at least 7 runs')
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import InflightSampler, RollingSampler
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    n_classes, V = m.stage2.spec.n_classes, m.stage2.spec.vocab_top
    m.stage2.engine(SLOTS, N, 0, max_prefix=RUN)         # one engine for both passes: the body workspace of a 32-position prefill
    mask = np.zeros(N, bool)
    mask[:RUN] = True

    def kept_of(g):
        """the kept codes of group g: one [GROUP, N] / [GROUP, N, 4] pair of random codes, read in the top half"""
        rng = np.random.default_rng(7000 + g)
        return [torch.from_numpy(rng.integers(0, V, (GROUP, N))), torch.from_numpy(rng.integers(0, V, (GROUP, N, 4)))]

    def rolling(groups, join_run):
        """-> (arrival offsets of the groups, finish offsets of the groups, per-call ms), all from the first arrival"""
        rs = RollingSampler(m.stage2, SLOTS, N, use_fp16=True, join_run=join_run)
        arrive, finish, calls = [], {}, []
        t0 = time.perf_counter()
        g = 0
        while g < groups or rs.live or rs.queue:
            t = time.perf_counter()
            if g < groups:
                arrive.append(t - t0)
                kept = kept_of(g)
                for i in range(GROUP):
                    rs.submit((g * GROUP + i) % n_classes, seed=1000 + g, sample_offset=i, keep_mask=mask, kept_codes=[kept[0][i], kept[1][i]])
                g += 1
            done = rs.step(GROUP)
            torch.cuda.synchronize()                     # the caller holds the finished codes
            calls.append(round((time.perf_counter() - t) * 1e3, 3))
            for ticket, _codes in done:
                finish[ticket // GROUP] = time.perf_counter() - t0
        m.stage2.range_check()
        return arrive, [finish[i] for i in range(groups)], calls

    def lanes(arrive):
        """every group its own 16-row prefix call on the next of 4 lanes, submitted at the given offsets -> finish offsets"""
        inf = lanes.sampler
        pending, finish = {}, {}
        t0 = time.perf_counter()

        def poll():
            for i, ev in list(pending.items()):
                if ev.query():
                    finish[i] = time.perf_counter() - t0
                    del pending[i]
        for i, at in enumerate(arrive):
            while time.perf_counter() - t0 < at:
                poll()
            cond = torch.tensor([(i * GROUP + j) % n_classes for j in range(GROUP)])
            kept = kept_of(i)
            pending[i] = inf.submit(GROUP, cond, seed=1000 + i, max_seq_len=N, use_fp16=True, decode=False,
                                    prefix_codes=[kept[0][:, :RUN].contiguous(), kept[1][:, :RUN].contiguous()])[3]
        while pending:
            poll()
        inf.drain()
        return [finish[i] for i in range(len(arrive))]
    lanes.sampler = InflightSampler(m, lanes=4)

    def join_cost(repeat):
        """a 16-step call over 16 live rows (positions 16 .. 31) with 16 joiners of run 32, and without -> ms per run"""
        out = {'with_16_joiners': [], 'without': []}
        for r in range(-2, repeat):                      # (two warm-up rounds)
            for mode in ('with_16_joiners', 'without'):
                rs = RollingSampler(m.stage2, SLOTS, N, use_fp16=True, join_run=RUN)
                for i in range(GROUP):
                    rs.submit(i % n_classes, seed=50 + r, sample_offset=i)
                rs.step(GROUP)
                if mode == 'with_16_joiners':
                    kept = kept_of(100 + r)
                    for i in range(GROUP):
                        rs.submit(i % n_classes, seed=60 + r, sample_offset=i, keep_mask=mask, kept_codes=[kept[0][i], kept[1][i]])
                torch.cuda.synchronize()
                t = time.perf_counter()
                rs.step(GROUP)
                torch.cuda.synchronize()
                if r >= 0:
                    out[mode].append(round((time.perf_counter() - t) * 1e3, 3))
                rs.drain(GROUP)
        m.stage2.range_check()
        return out

    def summary(arrive, finish):
        lat = [(f - s) * 1e3 for s, f in zip(arrive, finish)]
        total = max(finish) - arrive[0]
        return {'images': GROUP * len(arrive), 'total_ms': round(total * 1e3, 3), 'images_per_s': round(GROUP * len(arrive) / total, 1),
                'latency_ms_mean': round(statistics.mean(lat), 3), 'latency_ms_median': round(statistics.median(lat), 3), 'latency_ms_max': round(max(lat), 3),
                'latency_ms': [round(v, 3) for v in lat]}

    w_arrive, _, _ = rolling(a.warmup, RUN)
    rolling(a.warmup, 0)
    lanes(w_arrive)
    lanes.sampler.release(SLOTS, N)                      # lane 0 back to the latency-oriented kernels: the rolling pass runs alone
    m.stage2.engine(SLOTS, N, 0, max_prefix=RUN)
    res = {'what': f'tools/bench_rolling_keep.py --groups {a.groups} --warmup {a.warmup} --repeat {a.repeat}: the benchmark model (synthetic weights), FAST, graphed, '
                   f'AR loop only, n = {N}; every request keeps its first {RUN} positions; {a.groups} groups of {GROUP} requests, one group every {GROUP} positions '
                   f'of the rolling pass; one process, wall-clock times on the host'}
    def runs_of(one):
        """`repeat` runs of one mode -> the run with the median images/s, with the images/s of every run beside it"""
        runs = sorted((one() for _ in range(a.repeat)), key=lambda r: r['images_per_s'])
        return dict(runs[len(runs) // 2], images_per_s_runs=[r['images_per_s'] for r in runs])

    arrivals = []

    def roll32():
        arrive, finish, calls = rolling(a.groups, RUN)
        arrivals.append(arrive)
        return dict(summary(arrive, finish), slots=SLOTS, steps_per_call=GROUP, call_ms=calls, arrival_offsets_ms=[round(v * 1e3, 3) for v in arrive])

    def roll0():
        arrive, finish, calls = rolling(a.groups, 0)
        return dict(summary(arrive, finish), slots=SLOTS, steps_per_call=GROUP, call_ms=calls)
    res['join_run_32'] = runs_of(roll32)
    res['join_run_0'] = runs_of(roll0)
    cost = join_cost(a.repeat)
    res['join_phase'] = {'what': f'a {GROUP}-step call over {GROUP} live rows, {SLOTS} slots: with {GROUP} joiners of run {RUN} / without joiners; medians of {a.repeat} runs',
                         'call_ms_with_16_joiners_median': statistics.median(cost['with_16_joiners']), 'call_ms_without_median': statistics.median(cost['without']),
                         'call_ms_with_16_joiners': cost['with_16_joiners'], 'call_ms_without': cost['without']}
    replay = iter(arrivals)                              # run i of the lanes replays the arrivals of run i of the join_run_32 pass
    res['lanes'] = runs_of(lambda: (lambda arrive: dict(summary(arrive, lanes(arrive)), lanes=4, rows_per_pass=GROUP, prefix_len=RUN))(next(replay)))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')


if __name__ == '__main__':
    main()
