"""What a rolling pass buys a text-to-image model (hqt_set_max_joins / pipeline.RollingSampler(max_joins=)): configs/cc15m-12l-txt.yaml with synthetic weights in
FAST, graphed, AR loop only (no decode), n = 64 positions per image, requests (one random prompt each) arriving 16 at a time every 16 steps:
    rolling   ONE rolling pass of 64 slots with max_joins = 16: group g joins in call g (its prompt prefill -- the join phase -- in front of the call's 16 steps)
              beside the groups that are 17, 33 and 49 positions in; a group draws 1 + 16 positions in its first call and finishes in its fourth.  The pass
              itself is the clock: a group "arrives" when the call that admits it begins.
    lanes     what the code could do before: each group of 16 its own plain pass on the next lane of an InflightSampler (4 lanes), submitted at the wall-clock
              offsets at which the rolling run admitted its groups (the same arrival process, replayed).
    join      separately, the cost of the join phase with its B-row depth pass for J rows: a call of 16 steps over 16 live rows and 48 empty slots, against the
              same call in which 16 of the empty slots join (the steps carry 64 GEMM rows either way: idle rows ride along), medians over `--reps` pairs.
Per mode: images/s over the whole run (first arrival to last result) and the latency of a request, arrival to the host seeing its group finished (mean,
median, max); the rolling run also lists its per-call times.  One process; `warmup` groups run through each mode first (graphs captured, lanes built).

    python tools/bench_rolling_txt.py [--out profiles/rolling_txt.json] [--groups 16] [--warmup 5] [--reps 7]"""
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
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rolling_txt.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'cc15m-12l-txt.yaml'))
    p.add_argument('--groups', type=int, default=16)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--reps', type=int, default=7)
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hqtransformer_amd import synth
    from hqtransformer_amd._lib import PRECISION_FAST
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.pipeline import InflightSampler, RollingSampler
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    spec = m.stage2.spec
    assert spec.cond == 2 and spec.levels == 2, 'a two-level text-conditional config is expected'
    T = spec.ctx_len_txt

    def prompts(g):
        return torch.from_numpy(synth.text_ids(7000 + g, GROUP, T, spec.vocab_txt))

    def rolling(groups):
        """-> (arrival offsets of the groups, finish offsets of the groups, per-call ms), all from the first arrival"""
        rs = RollingSampler(m.stage2, SLOTS, N, max_joins=GROUP, use_fp16=True)
        arrive, finish, calls = [], {}, []
        t0 = time.perf_counter()
        g = 0
        while g < groups or rs.live or rs.queue:
            t = time.perf_counter()
            if g < groups:
                arrive.append(t - t0)
                for i, prompt in enumerate(prompts(g)):
                    rs.submit(prompt, seed=1000 + g, sample_offset=i)
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
            pending[i] = inf.submit(GROUP, prompts(i), seed=1000 + i, max_seq_len=N, use_fp16=True, decode=False)[3]
        while pending:
            poll()
        inf.drain()
        return [finish[i] for i in range(len(arrive))]
    lanes.sampler = InflightSampler(m, lanes=4)

    def join_cost(reps):
        """ms of a 16-step call over 16 live rows without and with 16 joining rows, `reps` pairs (the first pair is the warm-up and is dropped)"""
        eng = m.stage2.engine(SLOTS, N, 0, max_joins=GROUP)
        dev = eng.device
        codes = [torch.zeros((SLOTS, N), dtype=torch.int64, device=dev), torch.zeros((SLOTS, N, 4), dtype=torch.int64, device=dev)]
        cond = torch.from_numpy(synth.text_ids(7999, SLOTS, T, spec.vocab_txt))
        kw = dict(precision=PRECISION_FAST, seed=3, out=codes)
        empty = [-1] * (SLOTS - GROUP)

        def timed(pos):
            eng.sample(SLOTS, cond, N, row_positions=([0] * GROUP + empty, 1), **kw)      # a new pass: 16 rows join and stand at position 2
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.sample(SLOTS, cond, N, row_positions=(pos, GROUP), **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        none, joined = [], []
        for _ in range(reps + 1):
            none.append(timed([2] * GROUP + empty))
            joined.append(timed([2] * GROUP + [0] * GROUP + [-1] * (SLOTS - 2 * GROUP)))
        eng.sample(SLOTS, cond, N, row_positions=([-1] * SLOTS, 1), **kw)                   # every slot vacated: the pass is over
        eng.range_check()
        none, joined = none[1:], joined[1:]
        return {'slots': SLOTS, 'live_rows': GROUP, 'joiners': GROUP, 'steps_per_call': GROUP, 'reps': reps,
                'call_ms_without_joiners': [round(v, 3) for v in none], 'call_ms_with_joiners': [round(v, 3) for v in joined],
                'call_ms_without_joiners_median': round(statistics.median(none), 3), 'call_ms_with_joiners_median': round(statistics.median(joined), 3),
                'join_phase_ms_median_difference': round(statistics.median(joined) - statistics.median(none), 3)}

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
    res = {'what': f'tools/bench_rolling_txt.py --groups {a.groups} --warmup {a.warmup} --reps {a.reps}: {os.path.basename(a.config)} (SYNTHETIC weights, random prompts), '
                   f'FAST, graphed, AR loop only, n = {N}; {a.groups} groups of {GROUP} requests, one group every call of {GROUP} steps of the rolling pass '
                   f'(max_joins = {GROUP}); one process, wall-clock times on the host',
           'rolling': dict(summary(arrive, finish), slots=SLOTS, steps_per_call=GROUP, max_joins=GROUP, call_ms=calls,
                           full_call_ms_median=statistics.median(calls[3:a.groups]) if a.groups > 4 else None),
           'arrival_offsets_ms': [round(v * 1e3, 3) for v in arrive],
           'join': join_cost(a.reps)}
    res['lanes'] = dict(summary(arrive, lanes(arrive)), lanes=4, rows_per_pass=GROUP)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')


if __name__ == '__main__':
    main()
