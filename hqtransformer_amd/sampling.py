"""Counterpart of ``hqvae/utils/sampling.py`` for the HQ-Transformer path.

``sampling_ihqgpt`` keeps the reference's signature and return convention (sampling.py:164-237) and runs
the whole 64-position loop inside libhqt.so (KV cache, depth head, fused sampler, next-step embedding).
"""
from __future__ import annotations

from typing import List, Optional

import torch

from ._lib import PRECISION_EXACT, PRECISION_FAST, PRECISIONS
from .engine import DrawReport, check_keep, check_prefix, check_report_n, keep_leading_run, new_draw_report
from .text import pad_caption


def _seed_from_torch() -> int:
    """The reference consumes torch's global generator through ``torch.multinomial``; the Philox seed of the
    in-kernel Exp(1) noise is drawn from that same generator so ``set_seed`` keeps runs reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _precision(precision: Optional[str], use_fp16: bool) -> int:
    if precision is None:
        return PRECISION_FAST if use_fp16 else PRECISION_EXACT
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
    return PRECISIONS[precision]


def _batch_and_cond(model, num_candidates: int, cond):
    """``(num_candidates, cond)`` of the reference's samplers -> (B, cond tensor or None): text prompts [B, ctx_len_txt] set B themselves
    (sampling.py:187-190); a class id is an int, one id or B ids; anything else is unconditional."""
    if model.use_txt_cond:
        cond = torch.as_tensor(cond)
        if cond.dim() != 2:
            raise ValueError('text conditioning expects cond of shape [B, ctx_len_txt]')
        B = int(cond.shape[0])
    else:
        B = int(num_candidates)
        if model.use_cls_cond:
            if isinstance(cond, int):
                cond = torch.full((B,), int(cond), dtype=torch.int64)
            else:
                cond = torch.as_tensor(cond).reshape(-1)
                if cond.numel() == 1:
                    cond = cond.repeat(B)
            if int(cond.min()) < 0 or int(cond.max()) >= model.spec.n_classes:
                raise IndexError('index out of range in self')          # what nn.Embedding raises in the reference
        else:
            cond = None
    return B, cond


# ---------------------------------------------------------------------------------------------- guided sampling
# Every image runs as TWO rows of one pass, the same image under a positive and a negative condition; every code of both rows is drawn from
# l_pos + (scale - 1) (l_pos - l_neg) with one Philox key (hqt_set_guidance), so both rows return the same codes.  The reference trains without
# condition dropout and its class models have no "null" class: this is the mechanism and its arithmetic, not a claim about image quality.
def guidance_scales(levels: int, guidance_scale) -> Optional[tuple]:
    """``guidance_scale`` of the samplers -> one float per code level, coarse to fine (None stays None: no guidance): a float holds for every
    level, a list gives one per level."""
    if guidance_scale is None:
        return None
    L = int(levels)
    scales = (float(guidance_scale),) * L if isinstance(guidance_scale, (int, float)) else tuple(float(v) for v in guidance_scale)
    if len(scales) != L:
        raise ValueError(f'guidance_scale: expected a float or {L} floats (one per code level), got {len(scales)}')
    return scales


def guided_pairs(n: int, scales, lo: int = 0) -> list:
    """The pair table of ``n`` guided images whose 2 n rows start at row ``lo`` of a pass, positives first, then negatives: row ``lo + i`` is paired
    with row ``lo + n + i`` (entries ``(pos_row, neg_row, scales)``: ``guidance=`` of ``Engine.sample``)."""
    return [(int(lo) + i, int(lo) + int(n) + i, tuple(scales)) for i in range(int(n))]


def _twice(t, dim: int = 0):
    """A per-row input of n rows -> the 2 n rows of a guided call (the negative half repeats the positive one); None stays None."""
    return None if t is None else torch.cat([torch.as_tensor(t)] * 2, dim=dim)


def _twice_rows(rows):
    """``row_seeds`` / ``row_offsets`` / ``row_samplers`` of n rows -> 2 n rows; None stays None."""
    return None if rows is None else list(rows) * 2


def negative_cond(model, B: int, neg_cond) -> torch.Tensor:
    """The conditions of the B negative rows of a guided call -- text models: prompts [B, ctx_len_txt] or one prompt for all, default the
    all-``[PAD]`` caption (``text.pad_caption``); class models: one class id or B of them, required (the released class models have no "null" class
    to default to).  ValueError for an unconditional model."""
    if model.use_txt_cond:
        T = int(model.spec.ctx_len_txt)
        neg = pad_caption(B, T) if neg_cond is None else torch.as_tensor(neg_cond).reshape(-1, T).to(torch.int64)
    elif model.use_cls_cond:
        if neg_cond is None:
            raise ValueError('guidance_scale on a class-conditional model needs neg_cond: the class to push away from (there is no "null" class)')
        neg = torch.as_tensor(neg_cond).reshape(-1).to(torch.int64)
        if int(neg.min()) < 0 or int(neg.max()) >= model.spec.n_classes:
            raise IndexError('index out of range in self')
    else:
        raise ValueError('guidance_scale needs a conditional model: an unconditional model has no second condition to run its rows under')
    if int(neg.shape[0]) == 1:
        neg = neg.expand(B, *neg.shape[1:])
    if int(neg.shape[0]) != B:
        raise ValueError(f'neg_cond: expected one condition or {B} (one per image), got {int(neg.shape[0])}')
    return neg


def guided_cond(model, B: int, cond, neg_cond) -> torch.Tensor:
    """The conditions of a guided call's 2 B rows: ``cond`` (as ``_batch_and_cond`` returns it) for the positives, then ``negative_cond``."""
    neg = negative_cond(model, B, neg_cond)
    pos = torch.as_tensor(cond)
    return torch.cat([pos.to(torch.int64), neg.to(pos.device)])


def _guided(model, B: int, cond, guidance_scale, neg_cond, guidance):
    """What ``guidance_scale`` makes of a call: (rows of the pass, cond, pair table, rows to return).  Without a scale the call is what it was
    (``guidance``: a ready pair table over the rows as given, for callers that lay the rows out themselves)."""
    scales = guidance_scales(model.spec.levels, guidance_scale)
    if scales is None:
        if neg_cond is not None:
            raise ValueError('neg_cond comes with guidance_scale')
        return B, cond, guidance, B
    if guidance is not None:
        raise ValueError('guidance_scale builds the pair table itself: pass either guidance_scale (+ neg_cond) or guidance, not both')
    return 2 * B, guided_cond(model, B, cond, neg_cond), guided_pairs(B, scales), B


# ---------------------------------------------------------------------------------------------- shared prompts
# The prompt rows of a sample depend on nothing but its prompt: a pass whose rows repeat prompts (candidates of one caption, the negative rows of a guided
# batch) prefills every DISTINCT prompt once and copies the result to the rows that carry it (hqt_set_prompt_groups).
def prompt_groups_of(cond):
    """Text prompts [B, ctx_len_txt] -> (unique [G, ctx_len_txt], group_of_row int32 [B]): identical rows share a group, groups are numbered in the order in
    which their prompt first appears, and ``unique[group_of_row]`` reproduces ``cond``."""
    c = torch.as_tensor(cond)
    if c.dim() != 2 or int(c.shape[0]) < 1:
        raise ValueError(f'prompt_groups_of: expected prompts of shape [B, ctx_len_txt], got {tuple(c.shape)}')
    seen, first, group = {}, [], []
    for b, row in enumerate(c.cpu().tolist()):
        g = seen.setdefault(tuple(row), len(first))
        if g == len(first):
            first.append(b)
        group.append(g)
    return c[torch.as_tensor(first, device=c.device)], torch.tensor(group, dtype=torch.int32)


def _shared(model, share_prompts: bool, cond, prefix_codes=None, keep_mask=None, kept_codes=None):
    """What ``share_prompts`` makes of the rows of a pass as they will run (a guided call: positives, then negatives): (cond, prompt_groups) of ``Engine.sample``."""
    if not share_prompts:
        return cond, None
    if prefix_codes is not None or keep_mask is not None or kept_codes is not None:
        raise ValueError('share_prompts together with prefix_codes or keep_mask is not built: the prompt and a code prefix are one prefill whose prefix rows '
                         'differ per row')
    if not model.use_txt_cond:
        raise ValueError('share_prompts needs a text-conditional model: one embedding row per sample leaves no prefill to share')
    return prompt_groups_of(cond)


@torch.no_grad()
def sampling_ihqgpt(model,
                    num_candidates: int,
                    cond,
                    top_k_top: Optional[float] = None,
                    top_p_top: Optional[float] = None,
                    top_k_bot: Optional[float] = None,
                    top_p_bot: Optional[float] = None,
                    softmax_temperature: List[float] = [1.0, 1.0],
                    is_tqdm: bool = True,
                    use_fp16: bool = True,
                    max_seq_len: int = 256,
                    model_stage1=None,
                    given_top_code: Optional[torch.LongTensor] = None,
                    noise: Optional[torch.Tensor] = None,
                    sample_offset: int = 0,
                    seed: Optional[int] = None,
                    use_graph: bool = True,
                    lane: int = 0,
                    row_seeds=None,
                    row_offsets=None,
                    precision: Optional[str] = None,
                    row_samplers=None,
                    prefix_codes=None,
                    text_prefix: bool = False,
                    *,
                    return_logprobs: bool = False,
                    guidance_scale=None,
                    neg_cond=None,
                    guidance=None,
                    keep_mask=None,
                    kept_codes=None,
                    share_prompts: bool = False,
                    return_report: Optional[int] = None):
    """Returns ``(codes_top int64 [B, max_seq_len], codes_bot int64 [B, max_seq_len, 4])`` on the model's GPU; ``return_logprobs=True`` appends
    ``logprobs`` fp32 [B, max_seq_len, 5]: the log-probability of every code the call feeds forward (the drawn one; the given one where
    ``given_top_code`` forces the top level) under the raw logits of its draw -- temperature 1, no cut-off, so always finite; draw order top,
    bot0..bot3; positions below a prefix are NaN (``hqt_set_logprob_out``; ``pipeline.sequence_logprob`` sums them per sample).

    ``model`` is ``ImageGPT2.stage2``.  ``cond``: python int (class id, repeated for every candidate), an
    int64 tensor [B] of class ids, an int64 tensor [B, ctx_len_txt] (text; B replaces num_candidates,
    sampling.py:187-190) or anything (unconditional).  ``use_fp16=True`` -> FAST (bf16 MFMA) arithmetic,
    ``False`` -> EXACT fp32 (what the reference computes on its CPU path).  ``is_tqdm`` and ``model_stage1``
    are accepted and ignored (the latter only feeds a dead branch, hierarchical_ar.py:697-699).
    Extensions: ``noise`` fp32 [max_seq_len, 5, B, V] Exp(1) variates (draw = argmax(p/q), the multinomial
    identity) for bit-reproducible runs; ``sample_offset``/``seed`` for sharded batches; ``lane`` selects one of
    several workspaces over the same weights (one per batch in flight, see ``hqtransformer_amd.pipeline``);
    ``row_seeds`` / ``row_offsets`` (B entries each): merged steps -- row b draws what global row ``row_offsets[b]`` of a call
    seeded ``row_seeds[b]`` would draw, so several independent calls can share one pass over the weights;
    ``row_samplers`` (B entries ``(temperature per level, top_k per level, top_p per level)``, None = no cut-off): row b draws with its own
    settings in place of ``top_k_*`` / ``top_p_*`` / ``softmax_temperature``, bit for bit as in a call that has them for every row;
    ``precision`` ('exact' | 'fast' | 'split') overrides ``use_fp16``: 'split' = the fp32 launch sequence with every nn.Linear on the
    matrix cores (fp16 hi / lo operands, three MFMAs per term, fp32 accumulation): code sequences bit-identical to 'exact' wherever the
    draw is well-conditioned, at several times its speed;
    ``prefix_codes`` = ``[top [B, P], bot [B, P, 4]]``, 1 <= P <= max_seq_len - 1: completion -- the first P positions of the returned codes are
    these, the rest is drawn as a free run would draw it had its first P positions produced them (same Philox keys / ``noise`` slice per absolute
    position; ``given_top_code`` keeps its meaning for positions >= P).  The prefix goes through the body in one causal pass, not P decode steps.
    With text conditioning only on request, ``text_prefix=True``: the prompt and the prefix then share ONE prefill of ctx_len_txt + P rows per
    sample, and the engine's row workspace is sized for it (about twice the row buffers at the CC-15M shape: DESIGN §5.4); without the flag a
    text model refuses ``prefix_codes`` with ValueError before any engine is built.
    ``guidance_scale`` (a float, or one per code level) with ``neg_cond``: guided sampling -- every image runs as two rows of one pass, under ``cond``
    and under ``neg_cond`` (text: negative prompts [B, ctx_len_txt] or one for all, default the all-``[PAD]`` caption; class: the class id(s) to push
    away from, required), and every code is drawn from ``l_pos + (s - 1) (l_pos - l_neg)`` (``hqt_set_guidance``); s = 1 draws what the unguided
    call draws.  The pass has 2 B rows, positives first (the engine grows to that batch); ``noise``, ``given_top_code``, ``prefix_codes``,
    ``row_samplers`` and ``row_seeds`` / ``row_offsets`` are given for B rows and repeated for the negative half; the B positive rows are
    returned, so every result keeps its documented shape.  ValueError for an unconditional model.  The reference trains without condition dropout:
    what is claimed is the arithmetic, not an effect on image quality.  ``guidance`` instead of the two: a ready pair table
    ``[(pos_row, neg_row, scales), ...]`` over the B rows as given (``Engine.sample``; ``InflightSampler`` lays merged steps out this way).
    ``keep_mask`` bool [B, max_seq_len] with ``kept_codes`` = ``[top [B, max_seq_len], bot [B, max_seq_len, 4]]``: any positions of the grid held fixed
    (``hqt_set_keep_mask``) -- where the mask is set every level of the position is the given code, returned and fed forward; every other position is
    drawn as a free run would draw it had its earlier positions produced the same codes.  Rows may keep different positions: prefixes of different
    lengths, columns, everything outside a box.  The leading run all rows share goes through the one-pass prefill like ``prefix_codes`` (text
    conditioning: with ``text_prefix=True``; otherwise, and for every later kept position, a decode step each); log-probabilities of that run are
    NaN.  IndexError for a kept code outside the vocabulary.  Not together with ``given_top_code`` or ``prefix_codes``; with ``guidance_scale`` the
    two are given for B rows and repeated for the negative half.  Only the mechanism is claimed, not what it does to image quality.
    ``share_prompts=True`` (text models): identical prompts among the rows of the pass -- with ``guidance_scale`` the negative rows count, so one negative
    prompt for all is one group -- are prefilled once and handed to their rows (``prompt_groups_of``, ``hqt_set_prompt_groups``).  'exact' returns bit for bit
    what the call returns without it.  ValueError together with ``prefix_codes`` or ``keep_mask``.
    ``return_report=N`` (0..16; None: no report): appends one ``DrawReport(entropy, rank, top_codes, top_logprobs)`` behind the log-probabilities -- per draw, laid out
    [B, max_seq_len, 5] as they are, the entropy (nats) of the raw row the code was drawn from, the 0-based rank of the fed-forward code in it and, N >= 1, the N
    most likely codes with their log-probabilities [..., N] (``hqt_set_draw_report``; T = 1, no cut-off, whatever settings drew the code).  N = 0: entropy and
    rank only.  Positions below a prefix are NaN / -1.  The weights of the shipped configurations are synthetic: the mechanism and its arithmetic are claimed.

    The call is asynchronous and does not read the device's flags: 'split' passes above 256 rows SATURATE activations outside the fp16 range and
    only flag them, and a persistent FAST launch (up to 64 samples) that could not finish on a shared GPU only marks the handle -- call
    ``model.range_check()`` (``hqt_range_check``: raises ``HqtError``) once the codes are needed, as ``InflightSampler.drain`` and ``bench.py`` do.
    """
    spec = model.spec
    top_n = _report_n(spec, return_report)           # refused here, before an engine is built
    B, cond = _batch_and_cond(model, num_candidates, cond)
    rows, cond, guidance, keep = _guided(model, B, cond, guidance_scale, neg_cond, guidance)
    if rows != B:                                    # the negative half repeats every per-row input of the positive one
        noise, prefix_codes = _twice(noise, 2), None if prefix_codes is None else [_twice(p) for p in prefix_codes]
        row_seeds, row_offsets, row_samplers = _twice_rows(row_seeds), _twice_rows(row_offsets), _twice_rows(row_samplers)
        keep_mask, kept_codes = _twice(keep_mask), None if kept_codes is None else [_twice(c) for c in kept_codes]
        if given_top_code is not None:
            g = torch.as_tensor(given_top_code)
            given_top_code = g if g.dim() == 1 or g.shape[0] == 1 else _twice(g)
        B = rows
    cond, groups = _shared(model, share_prompts, cond, prefix_codes, keep_mask, kept_codes)
    prefix = check_prefix(spec, B, max_seq_len, prefix_codes, text_prefix=text_prefix)       # refused here, before an engine is built
    kept = _check_kept(spec, B, max_seq_len, keep_mask, kept_codes, prefix, given_top_code)
    force_top = None
    if given_top_code is not None and spec.depth_decoding == 'bidirectional':
        # the reference passes given_top_code to the 'parallel' head only and silently ignores it here (hierarchical_ar.py:451-479)
        raise ValueError("given_top_code is not supported by the 'bidirectional' depth head (the reference ignores it)")
    if given_top_code is not None:
        force_top = torch.as_tensor(given_top_code)
        if force_top.dim() == 1:
            force_top = force_top.unsqueeze(0)
        if force_top.shape[0] != B:
            force_top = force_top.repeat(B, 1)
        force_top = force_top[:, :max_seq_len]
    eng = model.engine(B, max_seq_len, lane, max_prefix=_prefix_room(spec, prefix) or _keep_room(spec, kept, text_prefix))
    if seed is None and noise is None:
        seed = _seed_from_torch()
    report = None if top_n is None else new_draw_report(B, max_seq_len, 5, top_n, eng.device)
    out = eng.sample(B, cond, max_seq_len, precision=_precision(precision, use_fp16),
                     top_k=(top_k_top, top_k_bot), top_p=(top_p_top, top_p_bot), temperature=softmax_temperature,
                     noise=noise, seed=seed or 0, sample_offset=sample_offset, force_top=force_top, use_graph=use_graph,
                     row_seeds=row_seeds, row_offsets=row_offsets, row_samplers=row_samplers, prefix=prefix, return_logprobs=return_logprobs,
                     guidance=guidance, keep=kept, report_out=report, **({} if groups is None else {'prompt_groups': groups}))
    out = out if report is None else out + (report,)
    return out if keep == B else tuple(_first_rows(t, keep) for t in out)          # (codes, log-probabilities and the report are [B, ...]: the positive half)


def _report_n(spec, return_report) -> Optional[int]:
    """``return_report`` of the samplers checked on the host: None, or N in [0, 16] and no more than the vocabulary holds."""
    top_n = check_report_n(return_report)
    if top_n is not None and top_n > spec.vocab_top:
        raise ValueError(f'return_report: N={top_n} alternatives, the vocabulary has {spec.vocab_top} codes')
    return top_n


def _first_rows(t, keep: int):
    """The first ``keep`` rows of a result [B, ...]; a ``DrawReport`` field by field."""
    if isinstance(t, DrawReport):
        return DrawReport(*(None if f is None else f[:keep] for f in t))
    return t[:keep]


def _prefix_room(spec, prefix) -> int:
    """``max_prefix`` of the engine a call with this prefix needs: none without one, else the length of this prefix.  The prefill's buffers
    grow with max_batch * (max_prefix + 1) rows (the split-K slab alone is 16 * rows * max(4 D, V) * 4 bytes: 1 GiB at 64 samples of the
    ImageNet-12L model with 32 positions, 2 GiB with 63), so room is taken for what is asked, not for every prefix the model could take.  Like the batch,
    the room only grows: a longer prefix later rebuilds the engine (weights are loaded and finalized again), and a caller who knows its
    longest prefix asks for it once with ``model.engine(batch, n_steps, max_prefix=...)``."""
    return 0 if prefix is None else int(prefix[0].shape[1])


def _check_kept(spec, B: int, n: int, keep_mask, kept_codes, prefix=None, given=None) -> Optional[tuple]:
    """``keep_mask`` / ``kept_codes`` of the samplers, checked on the host before an engine is built -> ``keep=`` of ``Engine.sample`` (None: neither given)."""
    if keep_mask is None and kept_codes is None:
        return None
    if keep_mask is None or kept_codes is None:
        raise ValueError('keep_mask and kept_codes come together')
    if prefix is not None:
        raise ValueError('keep_mask and prefix_codes: a prefix is a leading run of the keep mask -- put it there')
    if given is not None:
        raise ValueError('given_top_code together with keep_mask is not built: put the given codes into kept_codes')
    m, levels = check_keep(spec, B, n, (keep_mask, list(kept_codes)))
    return m, levels


def _keep_room(spec, kept, text_prefix: bool = True) -> int:
    """``max_prefix`` of the engine a call with this keep table asks for: the leading run all its rows share (``_prefix_room`` of that prefix); a text
    model shares the prompt's prefill with it on request only (``text_prefix``), as with ``prefix_codes`` -- without it every kept position is a decode step."""
    if kept is None or (spec.cond == 2 and (not text_prefix or spec.levels == 3 or spec.depth_decoding == 'bidirectional')):
        return 0
    return keep_leading_run(kept[0], kept[0].shape[1] - 1)


def sampling_hqtransformer(model,
                           num_candidates: int,
                           cond,
                           top_k: Optional[List[float]] = None,
                           top_p: Optional[List[float]] = None,
                           softmax_temperature: List[float] = [1.0, 1.0, 1.0],
                           is_tqdm: bool = True,
                           use_fp16: bool = True,
                           max_seq_len: int = 256,
                           model_stage1=None,
                           noise: Optional[torch.Tensor] = None,
                           sample_offset: int = 0,
                           seed: Optional[int] = None,
                           use_graph: bool = True,
                           lane: int = 0,
                           row_seeds=None,
                           row_offsets=None,
                           precision: Optional[str] = None,
                           row_samplers=None,
                           prefix_codes=None,
                           *,
                           return_logprobs: bool = False,
                           guidance_scale=None,
                           neg_cond=None,
                           guidance=None,
                           keep_mask=None,
                           kept_codes=None,
                           share_prompts: bool = False,
                           return_report: Optional[int] = None):
    """Counterpart of ``hqvae.utils.sampling.sampling_hqtransformer`` (sampling.py:240-307) for the three-level
    HQTransformer: returns ``[codes0 int64 [B, L], codes1 [B, L, 4], codes2 [B, L, 16]]`` on the model's GPU.
    ``top_k`` / ``top_p`` / ``softmax_temperature`` are per-level lists (None = no cut-off); ``cond`` as in
    ``sampling_ihqgpt``.  Extensions: ``noise`` fp32 [L, 21, B, V], ``seed`` / ``sample_offset``, ``lane``,
    ``row_samplers`` (per-row settings, as in ``sampling_ihqgpt``), ``prefix_codes`` = ``[t [B, P], m [B, P, 4], b [B, P, 16]]`` (completion,
    as in ``sampling_ihqgpt``), ``return_logprobs`` (appends fp32 [B, L, 21] to the list, as in ``sampling_ihqgpt``), ``guidance_scale`` (a float or
    three, one per level) / ``neg_cond`` / ``guidance`` (guided sampling over 2 B rows, the B positive ones returned, as in ``sampling_ihqgpt``),
    ``keep_mask`` [B, L] / ``kept_codes`` = ``[[B, L], [B, L, 4], [B, L, 16]]`` (kept positions, as in ``sampling_ihqgpt``),
    ``share_prompts`` (identical prompts of the pass prefilled once, as in ``sampling_ihqgpt``), ``return_report=N`` (appends a ``DrawReport`` of
    [B, L, 21(, N)] tensors behind the log-probabilities, as in ``sampling_ihqgpt``)."""
    spec = model.spec
    if spec.levels != 3:
        raise ValueError('sampling_hqtransformer needs the three-level HQTransformer (stage2.type multilevel-hq)')
    top_n = _report_n(spec, return_report)
    B, cond = _batch_and_cond(model, num_candidates, cond)
    rows, cond, guidance, keep = _guided(model, B, cond, guidance_scale, neg_cond, guidance)
    if rows != B:
        noise, prefix_codes = _twice(noise, 2), None if prefix_codes is None else [_twice(p) for p in prefix_codes]
        row_seeds, row_offsets, row_samplers = _twice_rows(row_seeds), _twice_rows(row_offsets), _twice_rows(row_samplers)
        keep_mask, kept_codes = _twice(keep_mask), None if kept_codes is None else [_twice(c) for c in kept_codes]
        B = rows
    cond, groups = _shared(model, share_prompts, cond, prefix_codes, keep_mask, kept_codes)
    prefix = check_prefix(spec, B, max_seq_len, prefix_codes)
    kept = _check_kept(spec, B, max_seq_len, keep_mask, kept_codes, prefix)
    top_k = list(top_k) if top_k is not None else [None, None, None]
    top_p = list(top_p) if top_p is not None else [None, None, None]
    eng = model.engine(B, max_seq_len, lane, max_prefix=_prefix_room(spec, prefix) or _keep_room(spec, kept))
    if seed is None and noise is None:
        seed = _seed_from_torch()
    report = None if top_n is None else new_draw_report(B, max_seq_len, 21, top_n, eng.device)
    out = eng.sample3(B, cond, max_seq_len, precision=_precision(precision, use_fp16), top_k=top_k, top_p=top_p,
                      temperature=softmax_temperature, noise=noise, seed=seed or 0, sample_offset=sample_offset, use_graph=use_graph,
                      row_seeds=row_seeds, row_offsets=row_offsets, row_samplers=row_samplers, prefix=prefix, return_logprobs=return_logprobs,
                      guidance=guidance, keep=kept, report_out=report, **({} if groups is None else {'prompt_groups': groups}))
    out = out if report is None else out + (report,)
    return list(out if keep == B else (_first_rows(t, keep) for t in out))


def rearrange_levels(codes: List[torch.Tensor], top_resolution: int) -> tuple:
    """'B (H W) -> B H W' and, level l, 'B (H W) (kerH kerW) -> B (H kerH) (W kerW)' with kerH = kerW = 2 ** l, as pure views."""
    B, K = codes[0].shape[0], top_resolution
    return tuple(c.reshape(B, K, K, 2 ** l, 2 ** l).permute(0, 1, 3, 2, 4).reshape(B, K << l, K << l) for l, c in enumerate(codes))


def rearrange_codes3(codes: List[torch.Tensor], top_resolution: int):
    """The three rearranges of ``sampling_hqmodel.py:150-153``, ``measure_throughput/__main__.py:128-130``."""
    return rearrange_levels(list(codes[:3]), top_resolution)


def rearrange_codes(codes_top: torch.Tensor, codes_bot: torch.Tensor, top_resolution: int):
    """The two rearranges of ``sampling_hqmodel.py:119-120``, ``measure_throughput/__main__.py:106-107``."""
    return rearrange_levels([codes_top, codes_bot], top_resolution)


# ---------------------------------------------------------------------------------------------- the reference's forward() layout
def global_to_sequence_index(n: int, level: int = 1) -> torch.Tensor:
    """int64 [n, 4 ** level]: entry (t, s) is the index, in the reference's global raster layout of code level ``level`` ('B (H H2 W W2)': the
    flattened (K << level) x (K << level) grid, n = K K), of slot s (row-major in the position's 2 ** level x 2 ** level block) of top position t --
    the sampler's layout [B, n, 4 ** level] is ``global[:, index]``."""
    K = int(round(n ** 0.5))
    if K * K != int(n):
        raise ValueError(f'n={n} top positions are not a square grid')
    k = 2 ** int(level)
    grid = torch.arange(n * k * k, dtype=torch.int64).reshape(1, K * k, K * k)
    return grid.reshape(1, K, k, K, k).permute(0, 1, 3, 2, 4).reshape(n, k * k)


def check_forward_codes(spec, codes):
    """Arguments of ``ImageGPT2.forward`` checked on the host, before any engine is built: two code levels, no text conditioning (its third output,
    ``logits_txt`` of the training-only ``head_txt``, is not built), ``codes = (top [B, n], bot [B, 4 n])`` with n a square."""
    if spec.cond == 2:
        raise NotImplementedError('forward of a text-conditional model also returns logits_txt = head_txt(ln_txt(h_txt)) (hierarchical_ar.py:386-390): head_txt '
                                  'is the training-only text head and is not built; score the image codes with pipeline.score_codes(one_pass=True)')
    if spec.levels != 2:
        raise ValueError('forward is built for two-level models (iHQGPT.forward); three-level codes are scored by pipeline.score_codes(one_pass=True)')
    if not isinstance(codes, (list, tuple)) or len(codes) != 2:
        raise ValueError('codes: expected (top [B, n], bot [B, 4 n])')
    top, bot = (torch.as_tensor(c) for c in codes)
    if top.dim() != 2:
        raise ValueError(f'codes[0]: expected shape (B, n), got {tuple(top.shape)}')
    B, n = (int(v) for v in top.shape)
    if int(round(n ** 0.5)) ** 2 != n:
        raise ValueError(f'codes[0]: n={n} top positions are not a square grid (the global raster layout of the bottom codes needs one)')
    if tuple(bot.shape) != (B, 4 * n):
        raise ValueError(f'codes[1]: expected shape {(B, 4 * n)} (global raster layout), got {tuple(bot.shape)}')
    return top, bot
