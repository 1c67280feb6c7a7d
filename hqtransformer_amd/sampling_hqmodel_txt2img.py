"""Counterpart of the reference's text-to-image driver (``sampling_hqmodel_txt2img.py:27-42,157-217``).

    python -m hqtransformer_amd.sampling_hqmodel_txt2img -r out_dir -m <config.yaml | result_dir | ckpt path> \
        --captions val_list.txt --tokenizer-vocab bpe-16k-vocab.json --tokenizer-merges bpe-16k-merges.txt

Same arguments and defaults (``--batch_size`` keeps the reference's underscore), same loop: captions in file order,
``batch_size`` prompts per batch, one image per prompt (``num_candidates=1``: B = number of prompts, sampling.py:187-190),
``top_k`` / ``top_p`` shared by both levels, temperatures ``T * decay^level``, decode + ``clamp(0.5 x + 0.5, 0, 1)``, and
one ``samples_({batch+1}_{batch_size}).pkl`` per batch = pickle of a float32 numpy array [B, 3, H, W] in [0, 1]
(:213-216).  The caption source replaces the hard-wired CC3M directory of the reference's ``CC3MTextOnly``
(``--captions``: its ``val_list.txt`` format or one caption per line); ``--synthetic-prompts N`` draws random token ids
instead (no tokenizer files needed: smoke runs).  The last, shorter batch is kept (the reference's DataLoader does the same).
``--complete-from FILE.npy --keep-rows R`` (no reference counterpart): meaning and file formats of ``sampling_hqmodel --complete-from`` -- prompt i
completes image i mod N to its caption, the first R rows of its top code grid kept.
``--best-of N`` (no reference counterpart: the reference leaves the choice among its candidates to an external model): N candidates are sampled per
caption in one pass and the most likely one under the stage-2 model is kept (``pipeline.sample_best_of``); the output format is unchanged.
``--share-prompts`` (no reference counterpart): identical prompts among the rows of a pass -- the N candidates of a caption with ``--best-of``, the negative
rows with ``--guidance-scale`` -- are prefilled once and handed to their rows (``hqt_set_prompt_groups``); harmless where no prompt repeats.
"""
from __future__ import annotations

import argparse
import os

import torch

from . import text as T
from .sampling_hqmodel import common_arguments, load_completion, load_model, sample_pixels, save_pickle
from .utils import set_seed


def _at_least_one(text: str) -> int:
    n = int(text)
    if n < 1:
        raise argparse.ArgumentTypeError(f'expected an integer >= 1, got {n}')
    return n


def build_parser() -> argparse.ArgumentParser:
    p = common_arguments(argparse.ArgumentParser())
    p.add_argument('--batch_size', type=int, default=32)
    p.add_argument('--dataset', type=str, default='cc3m', choices=['cc3m'])
    # where the reference reads a fixed dataset directory and its bundled vocabulary
    p.add_argument('--captions', type=str, default=None, help='val_list.txt ("<image>\t<caption>" lines) or one caption per line')
    p.add_argument('--tokenizer-vocab', type=str, default=None)
    p.add_argument('--tokenizer-merges', type=str, default=None)
    p.add_argument('--reference-root', type=str, default=os.environ.get('HQT_REFERENCE_ROOT'),
                   help='checkout of kakaobrain/hqtransformer to take the bundled bpe-16k vocabulary from')
    p.add_argument('--synthetic-prompts', type=int, default=0, help='N random-id prompts instead of captions (smoke runs)')
    p.add_argument('--best-of', type=_at_least_one, default=1, metavar='N',
                   help='sample N x num_candidates images per caption and keep the num_candidates the stage-2 model finds most likely (1: keep all)')
    p.add_argument('--negative-prompt', type=str, default=None, metavar='TEXT',
                   help='with --guidance-scale: the caption to push away from (needs the tokenizer; default: the empty, all-[PAD] caption)')
    p.add_argument('--share-prompts', action='store_true',
                   help='prefill every distinct prompt of a pass once and hand it to the rows that carry it (pays with --best-of and --guidance-scale)')
    return p


def prompt_ids(args, ctx_len: int, vocab_txt: int) -> torch.Tensor:
    if args.synthetic_prompts:
        g = torch.Generator().manual_seed(args.seed)
        return torch.randint(0, vocab_txt, (args.synthetic_prompts, ctx_len), generator=g, dtype=torch.int64)
    if not args.captions:
        raise SystemExit('give --captions FILE (with a tokenizer) or --synthetic-prompts N')
    return encode_checked(tokenizer(args, ctx_len), T.read_captions(args.captions), vocab_txt)


def tokenizer(args, ctx_len: int):
    pair = (args.tokenizer_vocab, args.tokenizer_merges) if args.tokenizer_vocab and args.tokenizer_merges else \
        T.find_reference_vocab(args.reference_root)
    if pair is None:
        raise SystemExit('no tokenizer: pass --tokenizer-vocab/--tokenizer-merges or --reference-root')
    return T.build_tokenizer(pair[0], pair[1], context_length=ctx_len)


def encode_checked(tok, texts, vocab_txt: int) -> torch.Tensor:
    ids = T.encode(tok, texts)
    if int(ids.max()) >= vocab_txt:
        raise SystemExit(f'token id {int(ids.max())} outside the model vocabulary ({vocab_txt})')
    return ids


def negative_ids(args, ctx_len: int, vocab_txt: int):
    """``neg_cond`` of the samplers for --guidance-scale: the tokenized --negative-prompt [1, ctx_len], or None (the samplers' all-[PAD] caption)."""
    if args.negative_prompt is None:
        return None
    if args.guidance_scale is None:
        raise SystemExit('--negative-prompt comes with --guidance-scale')
    return encode_checked(tokenizer(args, ctx_len), [args.negative_prompt], vocab_txt)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.code_level != 2:
        raise NotImplementedError('--code-level 3 (HQTransformer 3-level path) is not built yet (SURVEY.md §8f rank 1)')
    load_completion(args)
    if args.best_of > 1 and args.complete_from is not None:
        raise SystemExit('--best-of and --complete-from do not combine')
    if args.share_prompts and args.complete_from is not None:
        raise SystemExit('--share-prompts and --complete-from do not combine: the prompt and the kept code prefix are one prefill')
    set_seed(args.seed)
    os.makedirs(args.result_path, exist_ok=True)
    model = load_model(args.model_path).eval()
    if not model.stage2.use_txt_cond:
        raise SystemExit('the model is not text-conditional (stage2.use_txt_cond)')
    spec = model.stage2.spec
    ids = prompt_ids(args, spec.ctx_len_txt, spec.vocab_txt)
    args.neg_cond = negative_ids(args, spec.ctx_len_txt, spec.vocab_txt)
    n = args.batch_size
    for batch_idx, txts in enumerate(ids.split(n)):     # one image per prompt (num_candidates=1: B = number of prompts, sampling.py:187-190)
        save_pickle(os.path.join(args.result_path, f'samples_({batch_idx + 1}_{n}).pkl'), sample_pixels(model, args, 1, txts.cuda()))


if __name__ == '__main__':
    main()
