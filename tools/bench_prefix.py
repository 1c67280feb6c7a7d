"""What it costs to push P known positions through the ImageNet-12L model in FAST at B = 64 (default P = 32):
    prefix    the prefill part of a prefix call: ``Engine.sample(prefix=...)`` with n_steps = P + 1, i.e. the copy of the prefix, the embedding
              of its P + 1 body rows, ONE causal pass of all body blocks over them, the depth head on the last row and the draws of position P
              -- no decode step follows
    forced    the only way without the feature: ``Engine.sample`` of n_steps = P with force_top / force_bot, i.e. P teacher-forced decode steps,
              each with its depth head, two heads and five draws (graphed).  Uses nothing newer, so the file also runs in an older checkout:
              the figure of record for this mode is taken on the parent commit
With a text-conditional ``--config`` (configs/cc15m-12l-txt.yaml) the same two modes around the prompt: ``prefix`` is the ONE pass of
ctx_len_txt + P rows per sample that draws position P, ``forced`` the prompt prefill followed by P teacher-forced decode steps (n_steps = P + 1:
the prefill draws position 0, the last step position P); the record is profiles/text_prefix_prefill.json.
Each mode: HIP events around the call, median of --reps after --warmup, one JSON line.  ``--merge FORCED.json PREFIX.json --out FILE`` joins two such
lines into the record (profiles/prefix_prefill.json) with their ratio.
    python tools/bench_prefix.py --mode prefix [--P 32] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['prefix', 'forced'])
    p.add_argument('--P', type=int, default=32)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'imagenet-12l.yaml'))
    p.add_argument('--merge', nargs=2, metavar=('FORCED.json', 'PREFIX.json'))
    p.add_argument('--out')
    a = p.parse_args()
    if a.merge:
        forced, prefix = (json.loads(open(f).read().strip().splitlines()[-1]) for f in a.merge)
        assert forced['mode'] == 'forced' and prefix['mode'] == 'prefix' and forced['P'] == prefix['P'] and forced['B'] == prefix['B']
        rec = {'model': os.path.basename(a.config), 'precision': 'fast', 'B': prefix['B'], 'P': prefix['P'],
               'prefix_prefill_ms': prefix['ms_median'], 'forced_steps_ms': forced['ms_median'],
               'ratio_prefix_over_forced': round(prefix['ms_median'] / forced['ms_median'], 4), 'prefix': prefix, 'forced': forced}
        text = json.dumps(rec, indent=1)
        print(text)
        if a.out:
            with open(a.out, 'w') as fp:
                fp.write(text + '\n')
        return
    if not a.mode:
        p.error('--mode or --merge')
    import torch
    from hqtransformer_amd._lib import PRECISION_FAST
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    B, P = a.batch, a.P
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    spec = m.stage2.spec
    V, text = spec.vocab_top, spec.cond == 2
    g = torch.Generator().manual_seed(0)
    cond = (torch.randint(0, spec.vocab_txt, (B, spec.ctx_len_txt), generator=g) if text else torch.randint(0, 1000, (B,), generator=g)).cuda()
    top, bot = torch.randint(0, V, (B, P), generator=g).cuda(), torch.randint(0, V, (B, P, 4), generator=g).cuda()
    if a.mode == 'prefix':
        eng = m.stage2.engine(B, P + 1, max_prefix=P)

        def run():
            eng.sample(B, cond, P + 1, precision=PRECISION_FAST, seed=1, prefix=[top, bot])
    else:
        n = P + 1 if text else P
        eng = m.stage2.engine(B, n)
        if text:                                     # position P is drawn, as in the prefix mode: its forced entry is never embedded
            top, bot = torch.cat([top, top[:, :1]], 1), torch.cat([bot, bot[:, :1]], 1)

        def run():
            eng.sample(B, cond, n, precision=PRECISION_FAST, seed=1, force_top=top, force_bot=bot)
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
        ms.append(round(e0.elapsed_time(e1), 3))
    eng.range_check()
    print(json.dumps({'mode': a.mode, 'B': B, 'P': P, 'rows_per_sample': (spec.ctx_len_txt if text else 0) + (P if text or a.mode == 'forced' else P + 1), 'ms': ms, 'ms_median': statistics.median(ms), 'workspace_bytes': eng.workspace_bytes()}), flush=True)


if __name__ == '__main__':
    main()
