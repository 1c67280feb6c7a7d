"""What sharing the prompt prefill buys (hqt_set_prompt_groups): AR-loop time of the CC-15M text model (configs/cc15m-12l-txt.yaml, synthetic weights) in FAST,
graphed, one lane, 64 positions, one pass of
    rows64 / rows640          B rows with G = B (no table: the launches of a build without the feature), G = B / 8 and G = 1 distinct prompts
    guided32                  32 captions under guidance: 64 rows, the 32 negative rows carrying one prompt -- unshared, and shared (33 groups)
Method: one process; per mode `warmup` passes, then `reps` timed passes between device events on the stream the pass runs on; median, minimum and maximum
are reported; the modes of one row count alternate pass by pass.  Every mode also runs ONE eager pass of a single position (n_steps = 1: the prefill, the fan-out and the depth head of position 0, no decode
step) with the engine's per-launch timers on, which gives the time of the `prompt_fanout` slot, of the prefill GEMMs and of the prefill attention.
The comparison is the unshared run of the same build in the same process: without a table the build issues the launches it issued before the feature.

    python tools/bench_shared_prompt.py [--out profiles/shared_prompt.json] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ('prompt_fanout', 'gemm_qkv', 'gemm_proj', 'gemm_fc1', 'gemm_fc2', 'gemm_combine', 'attention', 'layernorm')


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shared_prompt.json'))
    p.add_argument('--config', default=os.path.join(ROOT, 'configs', 'cc15m-12l-txt.yaml'))
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hqtransformer_amd._lib import PRECISION_FAST
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import guided_pairs, prompt_groups_of
    from hqtransformer_amd.text import pad_caption
    n = 64
    m = ImageGPT2(load_config(a.config), seed=0).to('cuda').eval()
    spec = m.stage2.spec
    eng = m.stage2.engine(640, n)
    g = torch.Generator().manual_seed(0)
    caps = torch.randint(0, spec.vocab_txt, (640, spec.ctx_len_txt), generator=g, dtype=torch.int64)

    def case(rows, G):
        """cond and table of `rows` rows over G distinct captions, interleaved (row b carries caption b % G); G == rows: no table."""
        if G == rows:
            return caps[:rows].cuda(), None
        return caps[:G].cuda(), [b % G for b in range(rows)]

    modes = []
    for rows in (64, 640):
        for G in (rows, rows // 8, 1):
            modes.append((f'rows{rows}_G{G}', rows, G) + case(rows, G) + (None,))
    guided = torch.cat([caps[:32], pad_caption(32, spec.ctx_len_txt)])
    pairs = guided_pairs(32, (2.0,) * spec.levels)
    uniq, table = prompt_groups_of(guided)
    modes.append(('guided32_unshared', 64, 64, guided.cuda(), None, pairs))
    modes.append(('guided32_shared', 64, int(uniq.shape[0]), uniq.cuda(), table.tolist(), pairs))

    def run(rows, cond, table, pairs, steps=n, **more):
        kw = dict(precision=PRECISION_FAST, seed=100, guidance=pairs, **more)
        if table is not None:
            kw['prompt_groups'] = table
        return eng.sample(rows, cond, steps, **kw)

    res = {'what': f'tools/bench_shared_prompt.py --reps {a.reps} --warmup {a.warmup}: AR-loop time (ms, device events) of one pass of the CC-15M text model '
                   '(synthetic weights) in FAST, graphed, 64 positions, one lane, one process.  rowsB_GG: B rows over G distinct prompts (G = B: no group table, '
                   'i.e. the launches of a build without the feature -- this is the comparison); guided32: 32 captions under guidance, 64 rows, the negative rows '
                   'one prompt.  prefill_pass_ms: one eager single-position pass (prefill, fan-out, depth head of position 0) under the per-launch timers, by slot.',
           'modes': {}}
    # modes of one row count share one captured graph (the table is not part of the graph key), so they alternate pass by pass inside the timed window: what
    # drifts on the box during it reaches all of them alike
    groups = [[md for md in modes if md[0].startswith(prefix)] for prefix in ('rows64_', 'rows640_', 'guided32_')]
    for group in groups:
        for _, rows, G, cond, table, pairs in group:
            for _ in range(a.warmup):
                run(rows, cond, table, pairs)
        torch.cuda.synchronize()
        ms = {md[0]: [] for md in group}
        for _ in range(a.reps):
            for name, rows, G, cond, table, pairs in group:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(rows, cond, table, pairs)
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(round(e0.elapsed_time(e1), 3))
        m.stage2.range_check()
        for name, rows, G, cond, table, pairs in group:
            eng.timing_reset()
            eng.timing(True)
            run(rows, cond, table, pairs, steps=1)
            torch.cuda.synchronize()
            report = eng.timing_report()
            eng.timing(False)
            eng.timing_reset()
            slots = {s: {'launches': int(report[s][0]), 'ms': round(float(report[s][1]), 3)} for s in SLOTS if s in report}
            line = {'rows': rows, 'groups': G, 'prefill_rows': G * spec.ctx_len_txt, 'ar_ms': ms[name], 'ar_ms_median': statistics.median(ms[name]),
                    'ar_ms_min': min(ms[name]), 'ar_ms_max': max(ms[name]), 'prefill_pass_ms': slots,
                    'prefill_pass_total_ms': round(sum(float(v[1]) for v in report.values()), 3)}
            res['modes'][name] = line
            print(json.dumps({name: line}), flush=True)
    md = res['modes']
    res['shared_minus_unshared_ms'] = {k: round(md[k]['ar_ms_median'] - md[base]['ar_ms_median'], 3)
                                       for base, ks in (('rows64_G64', ('rows64_G8', 'rows64_G1')), ('rows640_G640', ('rows640_G80', 'rows640_G1')),
                                                        ('guided32_unshared', ('guided32_shared',))) for k in ks}
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
        fp.write('\n')


if __name__ == '__main__':
    main()
