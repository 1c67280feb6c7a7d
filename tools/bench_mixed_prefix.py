"""AR-loop time of 20 batch-64 completion steps of the ImageNet-12L model in FAST whose prefix lengths are drawn from {0, 16, 32, 48} (seeded), in
windows of 10 steps as a merging service would see them, graphed:
    mixed     ONE pass of 10 x 64 rows per window with a keep table (keep_mask= / kept_codes=, what InflightSampler(mixed_prefixes=True) stages): every
              row keeps its own step's prefix, the shortest prefix of the window is the pass's prefill, the rest are decode steps
    grouped   the passes today's rule forces (check_mergeable: one prefix length per pass), at their best: per window ONE pass per distinct prefix length
              (prefix_codes=), one after the other.  Uses nothing newer, so this mode also runs in an older checkout.  Each length has a lane of its
              own: a handle keeps one captured graph, and the positions per graph depend on the positions left to draw
Every step keeps its own seed and global offset (row_seeds / row_offsets), as InflightSampler.flush passes them.  Each mode: HIP events around the 20
steps, median of --reps after --warmup, one JSON line.  A/B protocol: the modes in separate processes, alternately, on one machine;
``--merge GROUPED.json MIXED.json --out profiles/mixed_prefix.json`` joins two such lines into the record.  Recorded, not gated.
    python tools/bench_mixed_prefix.py --mode mixed [--steps 20] [--window 10] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENGTHS = (0, 16, 32, 48)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['mixed', 'grouped'])
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--window', type=int, default=10, help='steps a merged pass may hold')
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    p.add_argument('--merge', nargs=2, metavar=('GROUPED.json', 'MIXED.json'))
    p.add_argument('--out')
    a = p.parse_args()
    if a.merge:
        grouped, mixed = (json.loads(open(f).read().strip().splitlines()[-1]) for f in a.merge)
        assert grouped['mode'] == 'grouped' and mixed['mode'] == 'mixed' and grouped['prefix_lengths'] == mixed['prefix_lengths']
        rec = {'model': os.path.basename(a.config), 'precision': 'fast', 'steps': mixed['steps'], 'window': mixed['window'], 'prefix_lengths': mixed['prefix_lengths'],
               'mixed_ms': mixed['ar_ms_median'], 'grouped_ms': grouped['ar_ms_median'],
               'ratio_mixed_over_grouped': round(mixed['ar_ms_median'] / grouped['ar_ms_median'], 4), 'mixed': mixed, 'grouped': grouped}
        text = json.dumps(rec, indent=1)
        print(text)
        if a.out:
            with open(a.out, 'w') as fp:
                fp.write(text + '\n')
        return
    if not a.mode:
        p.error('--mode or --merge')
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import sampling_ihqgpt
    B, n, k, win = 64, 64, a.steps, a.window
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    V = m.stage2.spec.vocab_top
    g = torch.Generator().manual_seed(0)
    cond = torch.randint(0, 1000, (k * B,), generator=g)
    Ps = [LENGTHS[int(i)] for i in torch.randint(0, len(LENGTHS), (k,), generator=g)]
    top, bot = torch.randint(0, V, (k * B, n), generator=g).cuda(), torch.randint(0, V, (k * B, n, 4), generator=g).cuda()
    windows = [list(range(lo, min(lo + win, k))) for lo in range(0, k, win)]

    def rows_of(steps):
        return torch.cat([torch.arange(s * B, (s + 1) * B) for s in steps])

    def one_pass(steps, lane=0, **kw):
        rows = rows_of(steps)
        return sampling_ihqgpt(m.stage2, num_candidates=len(rows), cond=cond[rows], use_fp16=True, is_tqdm=False, max_seq_len=n, seed=100 + steps[0], lane=lane,
                               row_seeds=[100 + s for s in steps for _ in range(B)], row_offsets=[i for _ in steps for i in range(B)], **kw)

    passes = []
    if a.mode == 'mixed':
        for steps in windows:
            rows = rows_of(steps).cuda()
            mask = torch.zeros((len(rows), n), dtype=torch.bool)
            for i, s in enumerate(steps):
                mask[i * B:(i + 1) * B, :Ps[s]] = True
            passes.append((steps, 0, dict(keep_mask=mask, kept_codes=[top[rows], bot[rows]])))
    else:
        for steps in windows:
            for lane, P in enumerate(LENGTHS):
                group = [s for s in steps if Ps[s] == P]
                if group:
                    rows = rows_of(group).cuda()
                    passes.append((group, lane, dict(prefix_codes=[top[rows, :P].contiguous(), bot[rows, :P].contiguous()]) if P else {}))
        m.stage2.engine(max(len(s) for s, _, _ in passes) * B, n, 0, max_prefix=max(Ps))      # sized once: every lane inherits it

    def run():
        for steps, lane, kw in passes:
            one_pass(steps, lane=lane, **kw)

    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1), 2))
    m.stage2.range_check()
    med = statistics.median(ms)
    print(json.dumps({'mode': a.mode, 'steps': k, 'window': win, 'rows': k * B, 'prefix_lengths': Ps, 'passes': [len(s) * B for s, _, _ in passes], 'ar_ms': ms,
                      'ar_ms_median': med, 'ar_images_per_s': round(k * B / med * 1000.0, 1)}), flush=True)


if __name__ == '__main__':
    main()
