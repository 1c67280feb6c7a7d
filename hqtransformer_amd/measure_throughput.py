"""Counterpart of the reference's throughput harness (``measure_throughput/__main__.py:51-180``).

    python -m hqtransformer_amd.measure_throughput model_path=configs/imagenet-12l.yaml batch_size=64

Same dot-list keys and defaults (``Experiment`` dataclass, :34-48), same loop accounting: ``n_loop`` loops of
``ceil(1000 / batch_size)`` iterations, the first ``warmup`` loops discarded, every iteration = one
``sampling_ihqgpt`` call (random class, ``top_k = top_p = None``, temperatures 1.0, ``use_fp16=True``) timed as
"ar", then code rearrange + ``stage1.decode_code`` + ``clamp(0.5 x + 0.5, 0, 1)`` timed as "decode", GPU events for
both, and the same printed lines (``ms/sample (ar: .., decode: ..)``).  Random-init weights, like the reference.
Differences, stated: the whole batch is decoded in one call instead of ``batch_size`` calls of one image
(``decode_batch=1`` restores the reference's chunking).  The reference decodes in fp32 (outside autocast, :108-113); the
default ``decode_precision=split`` is fp32-accurate on the matrix cores (pixels within 1e-4 of the fp32 result), ``exact`` runs
fp32 FMA chains on the vector ALUs, ``fast`` bf16 MFMA (faster, 0.04 max pixel error).  ``inflight=N`` (default 1 = the reference's order) keeps N
iterations in flight on N lanes (``hqtransformer_amd.pipeline``): same iterations, same accounting of the loop's wall
time; the per-phase figures then are lane times, which overlap.  ``merge=k`` executes k consecutive iterations as one pass of
k x batch_size rows (every iteration keeps its own class id and seed; ``bench.py`` picks its schedule from its step count K: 2 lanes x passes of min(32, ceil(K / 2)) steps);
the per-phase figures are then measured per pass.
"""
from __future__ import annotations

import platform
import random
import sys
import time

import torch

from .config import load_config, parse_dotlist
from .models import ImageGPT2
from .pipeline import InflightSampler, decode_codes, sample_codes

EXPERIMENT_DEFAULTS = dict(f=32, model='huge', d=4, c=16384, batch_size=50, n_loop=6, warmup=1, model_path='',
                           top_resolution=8, code_levels=2, decode_batch=0, decode_precision='split', seed=0, inflight=1, merge=1)


def iterations_per_loop(batch_size: int) -> int:
    """``n_iter_per_loop = (1000 + batch_size - 1) // batch_size`` (measure_throughput/__main__.py:76, measure_throughput_txt/__main__.py:103)."""
    return (1000 + batch_size - 1) // batch_size


def load_model(result_path: str) -> ImageGPT2:
    return ImageGPT2(load_config(result_path))


def report_loop(tag: str, wall_s: float, phase_s, images: int) -> tuple:
    """The two lines of one loop; returns (whole iteration, AR loop, decode) in ms per sample."""
    print(f'{tag} | {wall_s:.1f} s/loop (ar: {phase_s[0]:.1f}, decode: {phase_s[1]:.1f})')
    per_image_ms = tuple(1000.0 * t / images for t in (wall_s, *phase_s))
    print(f'{tag} | {per_image_ms[0]:.1f} ms/sample (ar: {per_image_ms[1]:.1f}, decode: {per_image_ms[2]:.1f})')
    return per_image_ms


def summarize(title: str, per_loop: list, warmup: int) -> dict:
    """The summary line over the loops after the first ``warmup`` (run and dropped), and the harness's result."""
    kept = per_loop[warmup:]
    print('-' * 80)
    mean_ms, mean_ar_ms, mean_dec_ms = (sum(col) / len(kept) for col in zip(*kept))
    print(f'{title} | {mean_ms:.4f} ms/sample (ar: {mean_ar_ms:.4f}, decode: {mean_dec_ms:.4f})')
    print('=' * 80)
    return dict(ms_per_sample=mean_ms, ms_ar=mean_ar_ms, ms_decode=mean_dec_ms, images_per_s=1000.0 / mean_ms)


def run_loops(args, model_ar: ImageGPT2, next_cond, sampler: dict, num_candidates: int) -> dict:
    """The harness loop of both counterparts (measure_throughput/__main__.py:84-180, measure_throughput_txt/__main__.py:106-188).
    ``next_cond()`` draws the next iteration's class id / prompt batch, ``sampler`` holds the sampler's keywords, ``num_candidates`` is
    what a direct sampler call gets (a queued step always carries ``batch_size`` rows)."""
    device = torch.device('cuda')
    model_ar = model_ar.to(device)
    model_ar.eval()
    title = f'bs{args.batch_size}, sampling loops {args.warmup + 1}-{args.n_loop}'
    print(title)
    print('python: %s, torch: %s, hip: %s, gpu: %s' % (platform.python_version(), torch.__version__, torch.version.hip,
                                                      torch.cuda.get_device_name(device)))
    ar_size = sum(p.numel() for p in model_ar.stage2.parameters()) / (10 ** 6)
    print(f'transformer size: {ar_size:.1f}M')
    batch_size, n_loop = int(args.batch_size), int(args.n_loop)
    n_iter_per_loop = iterations_per_loop(batch_size)
    n_pos = int(args.top_resolution) * int(args.top_resolution)
    merge = max(1, int(args.merge))
    pipe = None
    if int(args.inflight) > 1 or merge > 1:
        pipe = InflightSampler(model_ar, lanes=int(args.inflight), device=device, merge=merge, record_phases=merge > 1)

    def iteration(marks):                              # marks: (AR start, AR end, decode end) events of this iteration
        cond = next_cond()
        if pipe is not None:
            pipe.submit(batch_size, cond, max_seq_len=n_pos, use_fp16=True, precision=args.decode_precision, clamp01=True,
                        phase_events=None if merge > 1 else marks, **sampler)
            return
        marks[0].record()
        codes = sample_codes(model_ar.stage2, num_candidates, cond, use_fp16=True, max_seq_len=n_pos, model_stage1=None, **sampler)
        marks[1].record()
        _ = decode_codes(model_ar.stage1, codes, args.decode_precision, int(args.decode_batch), int(args.top_resolution))
        marks[2].record()

    def loop(loop_idx: int):
        marks = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(3)) for _ in range(n_iter_per_loop)]
        torch.cuda.synchronize(device)
        t_begin = time.time()
        for m in marks:
            iteration(m)
        if pipe is not None:
            pipe.drain()
        torch.cuda.synchronize(device)
        wall_s = time.time() - t_begin
        model_ar.stage1.range_check()          # SPLIT decode: raises if an activation left the fp16 range
        model_ar.stage2.range_check()          # FAST AR sampling of up to 64 rows: raises if a persistent launch gave up (hqt_range_check)
        if pipe is not None and merge > 1:     # per pass: (AR start, AR end, decode end) on the pass's lane
            marks, pipe.phase_log = [ev for ev, _ in pipe.phase_log], []
        phase_s = [sum(m[a].elapsed_time(m[a + 1]) for m in marks) / 1000 for a in (0, 1)]
        return report_loop(f'{loop_idx + 1}/{n_loop}', wall_s, phase_s, n_iter_per_loop * batch_size)

    print('-' * 80)
    return summarize(title, [loop(k) for k in range(n_loop)], int(args.warmup))


def main(args) -> dict:
    torch.set_grad_enabled(False)
    if args.code_levels not in (2, 3):
        raise NotImplementedError('code_levels must be 2 or 3')
    random.seed(args.seed)
    model_ar = load_model(args.model_path)
    if model_ar.stage2.spec.levels != args.code_levels:
        raise ValueError(f'{args.model_path} has {model_ar.stage2.spec.levels} code levels, code_levels={args.code_levels}')
    # random class, top_k = top_p = None, temperatures 1.0 (measure_throughput/__main__.py:92-104, 116-126)
    return run_loops(args, model_ar, lambda: random.randint(0, 999), dict(softmax_temperature=[1.0] * args.code_levels), num_candidates=args.batch_size)


if __name__ == '__main__':
    main(parse_dotlist(sys.argv[1:], EXPERIMENT_DEFAULTS))
