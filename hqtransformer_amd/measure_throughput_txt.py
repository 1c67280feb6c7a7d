"""Counterpart of the reference's text-to-image throughput harness (``measure_throughput_txt/__main__.py:83-188``).

    python -m hqtransformer_amd.measure_throughput_txt model_path=configs/cc15m-12l-txt.yaml batch_size=64

Same dot-list keys and defaults as its ``Experiment`` dataclass (:66-80: ``batch_size=50``, ``n_loop=6``, ``warmup=1``,
``top_resolution=8``, ``bot_resolution=16``, ``dataset='cc3m'``), same loop accounting (:106-165): ``n_loop`` loops of
``ceil(1000 / batch_size)`` iterations, the first ``warmup`` loops dropped, every iteration = one ``sampling_ihqgpt`` call on a
batch of prompts [B, ctx_len_txt] (``num_candidates=1`` as there -- with text conditioning the batch is the prompt count,
sampling.py:187-190) with the quality-mode sampler of that file (``top_k = 2048``, ``top_p = 1.0`` on both levels, temperature 1.0,
``use_fp16=True``) timed as "ar", then rearrange + ``stage1.decode_code`` + ``clamp(0.5 x + 0.5, 0, 1)`` timed as "decode", and the
same printed lines.

Differences, stated:
  * prompts.  The reference iterates ``CC3MTextOnly('val')`` (datasets/__init__.py:178-188), which is not available offline.
    ``prompts=synthetic`` (default) draws ids uniformly from the text vocabulary, one fresh batch per iteration, seeded;
    ``captions=<file>`` + ``tokenizer_vocab=`` / ``tokenizer_merges=`` runs real captions through the same BPE front-end
    (``hqtransformer_amd.text``), cycling over the file.
  * ``softmax_temperature``: the reference passes the float 1.0 (:135) where ``sampling_ihqgpt`` indexes a list -- its call raises
    TypeError as written; a float here means "this temperature on both levels".
  * decode: the whole batch in one call (``decode_batch=1`` restores the reference's one-image chunks, :146-150); the reference
    decodes in fp32 outside autocast, ``decode_precision=split`` (default) is fp32-accurate on the matrix cores.
  * ``inflight=N`` / ``merge=k``: several iterations in flight / merged into one pass, as in ``measure_throughput``.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .config import load_config, parse_dotlist
from .measure_throughput import iterations_per_loop, run_loops  # noqa: F401  (iterations_per_loop: measure_throughput_txt/__main__.py:103)
from .models import ImageGPT2
from .pipeline import sampler_cutoffs

EXPERIMENT_DEFAULTS = dict(f=32, model='huge', d=4, c=16384, batch_size=50, n_loop=6, warmup=1, model_path='',
                           top_resolution=8, bot_resolution=16, dataset='cc3m',
                           prompts='synthetic', captions='', tokenizer_vocab='', tokenizer_merges='',
                           top_k=2048, top_p=1.0, softmax_temperature=1.0,
                           decode_batch=0, decode_precision='split', seed=0, inflight=1, merge=1)


def prompt_batches(args, spec):
    """Generator of int64 [batch_size, ctx_len_txt] prompt batches: the text loader's role (:28-45, :118)."""
    B, ctx = int(args.batch_size), int(spec.ctx_len_txt)
    if args.captions:
        from . import text
        if not (args.tokenizer_vocab and args.tokenizer_merges):
            raise ValueError('captions= needs tokenizer_vocab= and tokenizer_merges= (the reference ships hqvae/tokenizers/pretrained/bpe-16k-*)')
        tok = text.build_tokenizer(args.tokenizer_vocab, args.tokenizer_merges, context_length=ctx)
        ids = text.encode(tok, text.read_captions(args.captions))
        if int(ids.max()) >= spec.vocab_txt:
            raise IndexError('a caption token id lies outside the model\'s text vocabulary')
        k = 0
        while True:
            idx = [(k + j) % ids.shape[0] for j in range(B)]
            k = (k + B) % ids.shape[0]
            yield ids[idx]
    else:
        rng = np.random.default_rng(int(args.seed) + 1)
        while True:
            yield torch.from_numpy(rng.integers(0, spec.vocab_txt, (B, ctx), dtype=np.int64))


def main(args) -> dict:
    torch.set_grad_enabled(False)
    model_ar = ImageGPT2(load_config(args.model_path))
    if not model_ar.stage2.use_txt_cond:
        raise ValueError(f'{args.model_path} is not a text-conditional model (use hqtransformer_amd.measure_throughput)')
    t = args.softmax_temperature
    temperature = [float(v) for v in t] if isinstance(t, (list, tuple)) else [float(t), float(t)]
    top_k = None if args.top_k in (None, 0, 'None') else int(args.top_k)
    top_p = None if args.top_p in (None, 0, 'None') else float(args.top_p)
    sampler = dict(sampler_cutoffs(2, top_k, top_p), softmax_temperature=temperature)
    prompts = prompt_batches(args, model_ar.stage2.spec)
    return run_loops(args, model_ar, lambda: next(prompts), sampler, num_candidates=1)


if __name__ == '__main__':
    main(parse_dotlist(sys.argv[1:], EXPERIMENT_DEFAULTS))
