"""AR-loop time of k batch-64 steps of the ImageNet-12L model in FAST of which half draw without a cut-off (the harness settings) and half
with top_k = 2048 at T = 0.95 (the quality mode), one lane, graphed:
    grouped   one merged pass per settings group (k/2 x 64 rows each, one after the other): all that could be done before rows carried
              their own sampler settings -- this mode and `uniform` use nothing newer, so the file also runs in an older checkout.  Each
              group has a lane of its own: the scalar settings are part of a handle's graph key and a handle keeps ONE captured graph, so
              two groups on one lane would re-capture on every pass and the figure would be that of graph capture
    mixed     ONE pass of k x 64 rows with a row table (row_samplers=)
    uniform   ONE pass of k x 64 rows, every row without a cut-off (the scalar path: the kernels a merged pass has always launched)
Every step keeps its own seed and global offset (row_seeds / row_offsets), as InflightSampler.flush passes them.  Prints one JSON line per
mode: the time of every repeat, their median and the images per second of the AR loop at that median.  A/B protocol: run the modes in
separate processes, alternately, on one machine (profiles/mixed_sampler.json).
    python tools/bench_mixed_sampler.py --modes grouped uniform [--steps 20] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN = dict(top_k_top=None, top_k_bot=None, top_p_top=None, top_p_bot=None, softmax_temperature=[1.0, 1.0])
QUALITY = dict(top_k_top=2048, top_k_bot=2048, top_p_top=None, top_p_bot=None, softmax_temperature=[0.95, 0.95])


def main():
    import torch
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import sampling_ihqgpt
    p = argparse.ArgumentParser()
    p.add_argument('--modes', nargs='+', default=['grouped', 'mixed', 'uniform'], choices=['grouped', 'mixed', 'uniform'])
    p.add_argument('--steps', type=int, default=20, help='k: batch-64 steps, half of them per settings group')
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    a = p.parse_args()
    if a.steps < 2 or a.steps % 2:
        p.error('--steps must be even')
    B, n, k = 64, 64, a.steps
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    m.stage2.engine(k * B, n)
    g = torch.Generator().manual_seed(0)
    cond = torch.randint(0, 1000, (k * B,), generator=g)
    kinds = [PLAIN if s % 2 == 0 else QUALITY for s in range(k)]          # the two kinds of request arrive interleaved

    def one_pass(steps, lane=0, **kw):
        rows = torch.cat([torch.arange(s * B, (s + 1) * B) for s in steps])
        return sampling_ihqgpt(m.stage2, num_candidates=len(rows), cond=cond[rows], use_fp16=True, is_tqdm=False, max_seq_len=n, seed=100 + steps[0], lane=lane,
                               row_seeds=[100 + s for s in steps for _ in range(B)], row_offsets=[i for _ in steps for i in range(B)], **kw)

    def run(mode):
        if mode == 'grouped':
            one_pass([s for s in range(k) if kinds[s] is PLAIN], lane=0, **PLAIN)
            one_pass([s for s in range(k) if kinds[s] is QUALITY], lane=1, **QUALITY)
        elif mode == 'mixed':
            from hqtransformer_amd.pipeline import step_row_samplers
            one_pass(list(range(k)), row_samplers=step_row_samplers(2, [B] * k, kinds))
        else:
            one_pass(list(range(k)), **PLAIN)

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
            ms.append(round(e0.elapsed_time(e1), 2))
        m.stage2.range_check()
        med = statistics.median(ms)
        print(json.dumps({'mode': mode, 'steps': k, 'rows': k * B, 'ar_ms': ms, 'ar_ms_median': med, 'ar_images_per_s': round(k * B / med * 1000.0, 1)}), flush=True)


if __name__ == '__main__':
    main()
