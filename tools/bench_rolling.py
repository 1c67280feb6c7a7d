"""What a rolling pass buys (hqt_set_row_positions / pipeline.RollingSampler): the benchmark model (configs/imagenet-12l.yaml, synthetic weights) in FAST,
graphed, AR loop only (no decode), n = 64 positions per image, requests arriving 16 at a time every 16 positions:
    rolling   ONE rolling pass of 64 slots: group g joins at position 0 of call g (16 steps per call) beside the groups that are 16, 32 and 48 positions in;
              in the steady state every call carries 64 rows.  The pass itself is the clock: a group "arrives" when the call that admits it begins.
    lanes     what the code could do before: each group of 16 its own plain pass on the next lane of an InflightSampler (4 lanes), submitted at the wall-clock
              offsets at which the rolling run admitted its groups (the same arrival process, replayed).
Per mode: images/s over the whole run (first arrival to last result) and the latency of a request, arrival to the host seeing its group finished (mean,
median, max); the rolling run also lists its per-call times.  One process; `warmup` groups run through each mode first (graphs captured, lanes built).

    python tools/bench_rolling.py [--out profiles/rolling.json] [--groups 16] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, N, GROUP = 64, 64, 16


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rolling.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    p.add_argument('--groups', type=int, default=16)
    p.add_argument('--warmup', type=int, default=5)
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import InflightSampler, RollingSampler
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    n_classes = m.stage2.spec.n_classes

    def rolling(groups):
        """-> (arrival offsets of the groups, finish offsets of the groups, per-call ms), all from the first arrival"""
        rs = RollingSampler(m.stage2, SLOTS, N, use_fp16=True)
        arrive, finish, calls = [], {}, []
        t0 = time.perf_counter()
        g = 0
        while g < groups or rs.live or rs.queue:
            t = time.perf_counter()
            if g < groups:
                arrive.append(t - t0)
                for i in range(GROUP):
                    rs.submit((g * GROUP + i) % n_classes, seed=1000 + g, sample_offset=i)
                g += 1
            done = rs.step(GROUP)
            torch.cuda.synchronize()                     # the caller holds the finished codes
            calls.append(round((time.perf_counter() - t) * 1e3, 3))
            for ticket, _codes in done:
                finish[ticket // GROUP] = time.perf_counter() - t0
        m.stage2.range_check()
        return arrive, [finish[i] for i in range(groups)], calls

    def lanes(arrive):
        """every group its own 16-row pass on the next of 4 lanes, submitted at the given offsets -> finish offsets"""
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
            pending[i] = inf.submit(GROUP, cond, seed=1000 + i, max_seq_len=N, use_fp16=True, decode=False)[3]
        while pending:
            poll()
        inf.drain()
        return [finish[i] for i in range(len(arrive))]
    lanes.sampler = InflightSampler(m, lanes=4)

    def summary(arrive, finish):
        lat = [(f - s) * 1e3 for s, f in zip(arrive, finish)]
        total = max(finish) - arrive[0]
        return {'images': GROUP * len(arrive), 'total_ms': round(total * 1e3, 3), 'images_per_s': round(GROUP * len(arrive) / total, 1),
                'latency_ms_mean': round(statistics.mean(lat), 3), 'latency_ms_median': round(statistics.median(lat), 3), 'latency_ms_max': round(max(lat), 3),
                'latency_ms': [round(v, 3) for v in lat]}

    w_arrive, _, _ = rolling(a.warmup)
    lanes(w_arrive)
    lanes.sampler.release(SLOTS, N)                      # lane 0 back to the latency-oriented kernels: the rolling pass runs alone
    arrive, finish, calls = rolling(a.groups)
    res = {'what': f'tools/bench_rolling.py --groups {a.groups} --warmup {a.warmup}: the benchmark model (synthetic weights), FAST, graphed, AR loop only, n = {N}; '
                   f'{a.groups} groups of {GROUP} requests, one group every {GROUP} positions of the rolling pass; one process, wall-clock times on the host',
           'rolling': dict(summary(arrive, finish), slots=SLOTS, steps_per_call=GROUP, call_ms=calls,
                           full_call_ms_median=statistics.median(calls[3:a.groups]) if a.groups > 4 else None),
           'arrival_offsets_ms': [round(v * 1e3, 3) for v in arrive]}
    res['lanes'] = dict(summary(arrive, lanes(arrive)), lanes=4, rows_per_pass=GROUP)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')


if __name__ == '__main__':
    main()
