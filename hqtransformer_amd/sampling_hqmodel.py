"""Counterpart of the reference's 50k-sample driver (``sampling_hqmodel.py:24-42,156-225``).

    python -m hqtransformer_amd.sampling_hqmodel -r out_dir -m <config.yaml | result_dir | ckpt path> [--top-k 2048 ...]

Same arguments and defaults, same outputs: ``samples_({cls+1}_{batch}).pkl`` = pickle (HIGHEST_PROTOCOL) of a float32
numpy array [B, 3, H, W] in [0, 1], and ``targets_({cls+1}_{batch}).npz`` with ``targets`` int64 [B]
(sampling_hqmodel.py:217-225), so ``eval_hqmodel.py`` / ``fid_utils.py:231-258`` of the reference read them unchanged.
``-m`` may point at a YAML (random-init weights, for smoke runs), a result directory holding ``config.yaml`` and
``ckpt/last.ckpt``, or the checkpoint file itself (sampling_hqmodel.py:64-82); the legacy ``stage1`` key remap of
:45-61 is applied when the checkpoint needs it.
"""
from __future__ import annotations

import argparse
import os
import pickle

import numpy as np
import torch

from .config import load_config
from .models import ImageGPT2
from .pipeline import canvas_windows, complete_images, decode_codes, sample_best_of, sample_canvas, sample_codes, sampler_cutoffs
from .utils import set_seed


def common_arguments(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """The arguments this driver shares with the text-to-image one (sampling_hqmodel.py:24-42, sampling_hqmodel_txt2img.py:27-42)."""
    p.add_argument('-r', '--result-path', type=str, required=True)
    p.add_argument('-m', '--model-path', type=str, default='', required=True)
    p.add_argument('--top-k', type=int, default=2048)
    p.add_argument('--top-p', type=float, default=1.0)
    p.add_argument('--temperature', type=float, default=1.0)
    p.add_argument('--temperature-decay', type=float, default=1.0)
    p.add_argument('--code-level', type=int, default=2)
    p.add_argument('--top-resolution', type=int, default=8)
    p.add_argument('--bot-resolution', type=int, default=16)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--decode-precision', choices=['split', 'exact', 'fast'], default='split',
                   help='the reference decodes in fp32: split = fp32-accurate on the matrix cores (default), exact = fp32 vector ALUs, fast = bf16')
    p.add_argument('--complete-from', type=str, default=None, metavar='FILE.npy',
                   help='complete images instead of sampling from scratch: float32 [N, 3, H, W] in [0, 1] (the layout of the samples this driver writes); '
                        'row i of a batch completes image (batch index * batch size + i) mod N.  Needs --keep-rows')
    p.add_argument('--guidance-scale', type=float, default=None, metavar='S',
                   help='guided sampling: every image runs under its condition and a negative one, codes are drawn from l_pos + (S - 1) (l_pos - l_neg); '
                        '1 draws what the unguided run draws (the reference trains without condition dropout: no effect on quality is claimed)')
    p.add_argument('--keep-rows', type=int, default=None, help='with --complete-from: rows of the top code grid kept from the image (1 .. top_resolution - 1)')
    return p


def build_parser() -> argparse.ArgumentParser:
    p = common_arguments(argparse.ArgumentParser())
    p.add_argument('--batch-size', type=int, default=50)
    p.add_argument('--num-classes', type=int, default=1000)
    p.add_argument('--samples-per-class', type=int, default=None, help='default 50000 // num_classes')
    p.add_argument('--canvas-grid', type=int, default=None, metavar='G',
                   help='sample a G x G top-code canvas (larger than the trained --top-resolution grid) with a sliding window; images come out at '
                        'resolution * G / top_resolution.  Needs --canvas-stride.  The mechanism is claimed, not the quality of the picture')
    p.add_argument('--canvas-stride', type=int, default=None, metavar='S', help='with --canvas-grid: cells the window moves by (1 <= S < top_resolution, (G - top_resolution) % S == 0)')
    p.add_argument('--negative-class', type=int, default=None, metavar='C', help='with --guidance-scale: the class id to push away from (required: there is no "null" class)')
    p.add_argument('--report-top', type=int, default=None, metavar='N',
                   help='also write report.npz: per draw the entropy of the distribution the code was drawn from, the rank of the code in it and the N most likely '
                        'codes with their log-probabilities (0 .. 16; 0: entropy and rank only).  Plain sampling only; the other outputs do not change')
    return p


def remap_legacy_keys(sd):
    """sampling_hqmodel.py:52-57: old checkpoints store stage-1 tensors under a 17-character prefix."""
    out = {}
    for k, v in sd.items():
        out['stage1.' + k[17:] if ('stage1' in k and not k.startswith('stage1.')) else k] = v
    return out


def read_checkpoint(path: str):
    """A checkpoint file as the reference writes them: Lightning's ``{'state_dict': ...}`` (``ckpt/last.ckpt``,
    sampling_hqmodel.py:77) or a bare state dict (``ckpt/state_dict.ckpt``, eval_stage1.py:164-166)."""
    obj = torch.load(path, map_location='cpu')
    return obj['state_dict'] if isinstance(obj, dict) and 'state_dict' in obj and not torch.is_tensor(obj['state_dict']) else obj


def load_model(model_path: str, device='cuda') -> ImageGPT2:
    """The ``-m`` forms of the reference's drivers: a result directory (``config.yaml`` + ``ckpt/state_dict.ckpt`` if present,
    else ``ckpt/last.ckpt``: eval_stage1.py:156-170, sampling_hqmodel.py:64-82), a checkpoint file inside ``<result>/ckpt/``
    (sampling_hqmodel.py:65-66), or -- no reference counterpart -- a bare YAML config (random-init weights, what
    measure_throughput builds).  Legacy ``stage1`` key prefixes are remapped (load_model_legacy, :45-61)."""
    if model_path.endswith(('.yaml', '.yml')):
        return ImageGPT2(load_config(model_path)).to(device)
    if 'ckpt' in model_path:
        config_path = os.path.join(os.path.dirname(model_path), '..', 'config.yaml')
        ckpt_path = model_path
    else:
        config_path = os.path.join(model_path, 'config.yaml')
        ckpt_path = os.path.join(model_path, 'ckpt/state_dict.ckpt')
        if not os.path.exists(ckpt_path):
            ckpt_path = os.path.join(model_path, 'ckpt/last.ckpt')
    print(ckpt_path)
    model = ImageGPT2(load_config(config_path))
    model.load_state_dict(remap_legacy_keys(read_checkpoint(ckpt_path)), strict=True)
    return model.to(device)


def load_model_legacy(result_path: str, device='cuda') -> ImageGPT2:
    """sampling_hqmodel.py:45-61: ``<result>/ckpt/last.ckpt`` whose stage-1 keys carry a 17-character legacy prefix."""
    model = ImageGPT2(load_config(os.path.join(result_path, 'config.yaml')))
    sd = torch.load(os.path.join(result_path, 'ckpt/last.ckpt'), map_location='cpu')['state_dict']
    model.load_state_dict(remap_legacy_keys(sd), strict=True)
    return model.to(device)


def save_pickle(fname, data):
    with open(fname, 'wb') as fp:
        pickle.dump(data, fp, pickle.HIGHEST_PROTOCOL)


def sample_pixels(model: ImageGPT2, args, num_candidates: int, cond) -> np.ndarray:
    """One batch of either driver (sampling_hqmodel.py:101-153,201-214): ``top_k`` / ``top_p`` shared by the levels, temperatures
    ``T * decay^level``, decode + ``clamp(0.5 x + 0.5, 0, 1)``; float32 [B, 3, H, W] in [0, 1] on the host."""
    temps = [args.temperature * (args.temperature_decay ** i) for i in range(args.code_level)]
    guided = {}
    if getattr(args, 'guidance_scale', None) is not None:      # --guidance-scale: twice the rows per pass, the negative condition from the driver
        guided = dict(guidance_scale=args.guidance_scale, neg_cond=getattr(args, 'neg_cond', None))
    images = getattr(args, 'complete_images', None)
    if images is not None:               # --complete-from: the same sampler settings, the first rows of every image kept
        first = getattr(args, 'complete_next', 0)
        count = int(cond.shape[0]) if model.stage2.use_txt_cond else num_candidates      # text: one image per prompt
        args.complete_next = first + count
        rows = torch.from_numpy(images[np.arange(first, first + count) % len(images)])
        pixels, _ = complete_images(model, 2.0 * rows - 1.0, args.keep_rows, cond=cond, decode_precision=args.decode_precision, softmax_temperature=temps,
                                    use_fp16=True, **guided, **sampler_cutoffs(args.code_level, args.top_k, args.top_p))
        model.stage1.range_check()
        model.stage2.range_check()
        return pixels.cpu().numpy()
    if getattr(args, 'canvas_grid', None) is not None:         # --canvas-grid: one sliding-window canvas per row, window k seeded seed + k of this batch
        first = getattr(args, 'canvas_next', 0)
        args.canvas_next = first + len(canvas_windows(args.canvas_grid, args.top_resolution, args.canvas_stride))
        _, pixels = sample_canvas(model, cond, grid=args.canvas_grid, stride=args.canvas_stride, seed=args.seed + first, num_candidates=num_candidates,
                                  decode_precision=args.decode_precision, softmax_temperature=temps, use_fp16=True, **guided,
                                  **sampler_cutoffs(args.code_level, args.top_k, args.top_p))
        model.stage1.at_resolution(int(pixels.shape[-1])).range_check()
        model.stage2.range_check()
        return pixels.cpu().numpy()
    sampler = dict(softmax_temperature=temps, use_fp16=True, max_seq_len=args.top_resolution * args.top_resolution, model_stage1=model.stage1,
                   **guided, **sampler_cutoffs(args.code_level, args.top_k, args.top_p))
    if getattr(args, 'share_prompts', False):      # --share-prompts (text driver): identical prompts of the pass are prefilled once
        sampler['share_prompts'] = True
    best_of = getattr(args, 'best_of', 1)
    report_top = getattr(args, 'report_top', None)
    if report_top is not None:           # --report-top N: the report of every draw travels behind the codes and is collected for report.npz
        codes = sample_codes(model.stage2, num_candidates, cond, return_report=report_top, **sampler)
        args.reports = getattr(args, 'reports', []) + [codes.pop()]
    elif best_of > 1:                      # --best-of N: N x num_candidates per condition in one pass, the num_candidates most likely kept
        codes, _ = sample_best_of(model.stage2, cond, best_of * num_candidates, num_candidates, **sampler)
    else:
        codes = sample_codes(model.stage2, num_candidates, cond, **sampler)
    pixels = decode_codes(model.stage1, codes, args.decode_precision)
    model.stage1.range_check()          # SPLIT decode: raises if an activation left the fp16 range
    model.stage2.range_check()          # FAST AR sampling of up to 64 rows: raises if a persistent launch gave up (hqt_range_check)
    return pixels.cpu().numpy()


def load_completion(args) -> None:
    """``--complete-from`` / ``--keep-rows`` of either driver, checked; the images go to ``args.complete_images``."""
    if (args.complete_from is None) != (args.keep_rows is None):
        raise SystemExit('--complete-from and --keep-rows come together')
    if args.complete_from is not None:
        args.complete_images = np.ascontiguousarray(np.load(args.complete_from), dtype=np.float32)
        if args.complete_images.ndim != 4 or args.complete_images.shape[1] != 3 or len(args.complete_images) < 1:
            raise SystemExit(f'--complete-from: expected float32 [N, 3, H, W], got {args.complete_images.shape}')
        if not 1 <= args.keep_rows < args.top_resolution:
            raise SystemExit(f'--keep-rows must lie in [1, top_resolution - 1 = {args.top_resolution - 1}]')


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.code_level not in (2, 3):
        raise NotImplementedError('--code-level must be 2 or 3')
    load_completion(args)
    if (args.guidance_scale is None) != (args.negative_class is None):
        raise SystemExit('--guidance-scale and --negative-class come together')
    args.neg_cond = args.negative_class
    if (args.canvas_grid is None) != (args.canvas_stride is None):
        raise SystemExit('--canvas-grid and --canvas-stride come together')
    if args.canvas_grid is not None:
        if args.complete_from is not None:
            raise SystemExit('--canvas-grid samples from scratch: not together with --complete-from')
        try:
            canvas_windows(args.canvas_grid, args.top_resolution, args.canvas_stride)
        except ValueError as e:
            raise SystemExit(f'--canvas-grid / --canvas-stride: {e}')
    if args.report_top is not None:
        if not 0 <= args.report_top <= 16:
            raise SystemExit('--report-top must lie in [0, 16]')
        if args.complete_from is not None or args.canvas_grid is not None:
            raise SystemExit('--report-top reports plain sampling: not together with --complete-from or --canvas-grid')
    set_seed(args.seed)
    os.makedirs(args.result_path, exist_ok=True)
    model = load_model(args.model_path).eval()
    per_class = args.samples_per_class if args.samples_per_class is not None else 50000 // args.num_classes
    n = args.batch_size
    for cls_idx in range(args.num_classes):
        for num_batches in range(per_class // n):
            targets = torch.ones(n, dtype=torch.long) * cls_idx
            pixels = sample_pixels(model, args, n, cls_idx)
            save_pickle(os.path.join(args.result_path, f'samples_({cls_idx + 1}_{num_batches}).pkl'), pixels)
            np.savez(os.path.join(args.result_path, f'targets_({cls_idx + 1}_{num_batches}).npz'), targets=targets.cpu().numpy())
    write_report(args)


def write_report(args) -> None:
    """``--report-top``: report.npz beside the samples -- the ``DrawReport`` fields of all batches in the order they were sampled, [images, positions, draws(, N)]."""
    reports = getattr(args, 'reports', None)
    if reports:
        fields = {f: torch.cat([getattr(r, f) for r in reports]).cpu().numpy() for f in reports[0]._fields if getattr(reports[0], f) is not None}
        np.savez(os.path.join(args.result_path, 'report.npz'), **fields)


if __name__ == '__main__':
    main()
