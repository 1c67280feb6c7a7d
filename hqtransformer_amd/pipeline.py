"""Several batches in flight on one GPU.

The reference's harness (``measure_throughput/__main__.py:84-116``) samples and decodes one batch at a time.  On an
MI355X the 64-row AR loop is a dependent chain of ~100 small kernels per position, each of which keeps well under half
of the 256 CUs busy and is bound by per-CU latency; independent chains interleave almost for free.  ``InflightSampler``
therefore round-robins consecutive batches over N *lanes*: every lane has its own stream, KV cache and activations
(``hqt_clone``) and shares the weights, every batch is still one complete ``sampling_ihqgpt`` + ``decode_code`` pass
of the configured batch size, and results do not depend on the lane (bit-identical, tests/test_gpu_surface.py).

``merge=k`` additionally executes k queued steps as ONE pass of k x B rows (class-conditional, unconditional, text-conditional; two or
three code levels): the steps stay independent -- every row keeps the class id / prompt, the Philox seed and the global row index of its own step (``hqt_sample_opts.row_seeds`` / ``row_offsets``), so in EXACT
arithmetic each step's codes are bit-identical to the unmerged call (tests/test_gpu_surface.py) -- but the weights are streamed
once for all of them instead of once per step.  ``mixed_samplers=True`` lets the steps of a pass differ in temperature, top-k and top-p as well:
every row then carries the sampler settings of its own step (``hqt_set_row_samplers``) and draws what it draws in that step's separate call.
"""
from __future__ import annotations

from typing import Any, Callable, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ._lib import POLICY_LATENCY, POLICY_THROUGHPUT
from .engine import DrawReport, check_select_rows, new_draw_report
from .sampling import (_batch_and_cond, _first_rows, _precision, _report_n, _seed_from_torch, guidance_scales, negative_cond, prompt_groups_of, rearrange_levels,
                       sampling_hqtransformer, sampling_ihqgpt)


# Code levels travel as one list, coarse to fine.  These are the only places that tell two levels from three: the sampler call, and the
# (codes_top, codes_bot) shape of a result, whose second entry is a tensor (two levels) or the list of the finer levels (three).
def sample_codes(stage2, num_candidates: int, cond, **kw) -> list:
    """One ``sampling_ihqgpt`` / ``sampling_hqtransformer`` call (keywords of that sampler) -> its codes as a list; ``return_logprobs=True``
    travels with the keywords, and the log-probabilities fp32 [B, n, draws] are then the list's last entry, behind the codes; so do
    ``guidance_scale`` / ``neg_cond`` (guided sampling: 2 B rows in the pass, the B positive ones returned)."""
    sampler = sampling_hqtransformer if stage2.spec.levels == 3 else sampling_ihqgpt
    return list(sampler(stage2, num_candidates=num_candidates, cond=cond, is_tqdm=False, **kw))


def sampler_cutoffs(levels: int, top_k, top_p) -> dict:
    """One top-k / top-p for every level (what the reference's drivers pass), in the keywords of that level count's sampler."""
    if levels == 3:
        return dict(top_k=[top_k] * 3, top_p=[top_p] * 3)
    return dict(top_k_top=top_k, top_p_top=top_p, top_k_bot=top_k, top_p_bot=top_p)


# the sampler keywords of sampling_ihqgpt (two levels) and sampling_hqtransformer (three): what the steps of a mixed pass may differ in
SAMPLER_KEYS = ('top_k_top', 'top_p_top', 'top_k_bot', 'top_p_bot', 'top_k', 'top_p', 'softmax_temperature')


def step_row_samplers(levels: int, sizes, sample_kws) -> list:
    """Steps of a mixed pass -> its row table: step i's sampler keywords (``sample_kws[i]``: those of ``sampling_ihqgpt`` for two levels, of
    ``sampling_hqtransformer`` for three; missing = the sampler's default) as one ``(temperature, top_k, top_p)`` entry, each per level, repeated
    for the step's ``sizes[i]`` rows.  The result is ``row_samplers=`` of the samplers (``Engine.sample``)."""
    L = int(levels)
    rows: list = []
    for n, kw in zip(sizes, sample_kws):
        if L == 3:
            top_k, top_p = (tuple(kw[k]) if kw.get(k) is not None else (None,) * 3 for k in ('top_k', 'top_p'))
        else:
            top_k, top_p = (kw.get('top_k_top'), kw.get('top_k_bot')), (kw.get('top_p_top'), kw.get('top_p_bot'))
        t = kw.get('softmax_temperature')
        temperature = tuple(float(v) for v in t) if t is not None else (1.0,) * L
        if not (len(temperature) == len(top_k) == len(top_p) == L):
            raise ValueError(f'sampler settings of a {L}-level step need {L} entries each, got {kw}')
        rows.extend([(temperature, top_k, top_p)] * int(n))
    return rows


# what a step of a merged pass may set for itself besides its rows: guided steps merge with each other and with unguided ones (the pair table is per row)
GUIDANCE_KEYS = ('guidance_scale', 'neg_cond')


def step_guidance(levels: int, sizes, sample_kws) -> Tuple[list, list]:
    """Steps of a merged pass -> its guidance: the pass lays the steps' own rows out first, step after step (``sizes[i]`` rows each, N in all: what an
    unguided pass holds), then one negative row for every row of every guided step, in the same order.  Returns ``(pairs, mirrors)``: ``pairs`` is
    ``guidance=`` of the samplers, step i's ``guidance_scale`` (``sample_kws[i]``; a float or one per level) on every pair of its rows
    ``(lo_i + j, N + k)``; ``mirrors[k]`` is the row that negative row ``N + k`` repeats in everything but its condition (key, sampler settings,
    prefix).  No guided step: ``([], [])``."""
    N = sum(int(n) for n in sizes)
    pairs, mirrors, lo = [], [], 0
    for n, kw in zip(sizes, sample_kws):
        scales = guidance_scales(levels, kw.get('guidance_scale'))
        if scales is None and kw.get('neg_cond') is not None:
            raise ValueError('neg_cond comes with guidance_scale')
        for j in range(int(n) if scales is not None else 0):
            pairs.append((lo + j, N + len(mirrors), scales))
            mirrors.append(lo + j)
        lo += int(n)
    return pairs, mirrors


def check_guided_step(stage2, num_candidates: int, sample_kw: dict) -> None:
    """What ``flush`` would refuse in a guided step, raised when the step is submitted: a scale count that does not match the levels, ``neg_cond``
    without a scale, a class model without ``neg_cond``, a ``neg_cond`` of the wrong length or outside the classes, an unconditional model."""
    scales = guidance_scales(stage2.spec.levels, sample_kw.get('guidance_scale'))
    if scales is None:
        if sample_kw.get('neg_cond') is not None:
            raise ValueError('neg_cond comes with guidance_scale')
        return
    negative_cond(stage2, int(num_candidates), sample_kw.get('neg_cond'))


def decode_codes(stage1, codes: list, precision: Optional[str] = None, decode_batch: int = 0, top_resolution: int = 0) -> torch.Tensor:
    """Sampled codes -> pixels in [0, 1]: rearrange + ``decode_code`` + ``clamp(0.5 x + 0.5, 0, 1)`` of the reference's drivers, folded into
    the decode kernels; ``decode_batch`` < B restores the reference's chunked decode of ``decode_batch`` images per call."""
    B = int(codes[0].shape[0])
    if decode_batch and decode_batch < B:
        grids = rearrange_levels(codes, top_resolution)
        pixels = torch.cat([stage1.decode_code([g[j:j + decode_batch] for g in grids], precision=precision) for j in range(0, B, decode_batch)], dim=0)
        return (0.5 * pixels + 0.5).clamp(0, 1)
    return stage1.decode_sequences(codes, precision=precision, clamp01=True)


def sequence_logprob(logprobs: torch.Tensor) -> torch.Tensor:
    """Log-probabilities of a sampler call fp32 [B, n, draws] -> the log-probability of every sample's whole code sequence, fp64 [B], summed over positions and
    draws in fp64 where the tensor lives.  NaN propagates: a sample with positions that were not scored (below a prefix) has no score -- slice them
    away first (``logprobs[:, P:]``) for the score of the completion alone."""
    if logprobs.dim() != 3:
        raise ValueError(f'logprobs: expected [B, n, draws], got {tuple(logprobs.shape)}')
    return logprobs.to(torch.float64).sum(dim=(1, 2))


def rank_candidates(scores: torch.Tensor, keep: int) -> torch.Tensor:
    """``scores`` [groups, candidates] -> int64 [groups, keep]: per group the indices of the ``keep`` highest scores, descending; equal scores keep their
    order (the lower candidate index first: a stable sort)."""
    if scores.dim() != 2 or not 1 <= int(keep) <= int(scores.shape[1]):
        raise ValueError(f'rank_candidates: keep={keep} of scores {tuple(scores.shape)}: expected [groups, candidates] and 1 <= keep <= candidates')
    return torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :int(keep)]


def uncertainty_map(entropy: torch.Tensor, levels: int) -> list:
    """The entropies of a ``DrawReport`` fp32 [B, n, draws] (n = K K top positions; draws = 5, or 21 with three levels, in the draw order top, bot0..bot3[,
    l2 0..15]) -> one grid per code level, so that a map lies over the decoded image: [B, K, K], [B, 2 K, 2 K][, [B, 4 K, 4 K]] -- cell (position t, slot s) of
    a level lands where ``decode_sequences`` / ``seq_layout`` place that code (``rearrange_levels``: 'B (H W) (kh kw) -> B (H kh) (W kw)').  Works on any per-draw
    quantity laid out like the log-probabilities (the rank, ``-logprobs``)."""
    L = int(levels)
    if L not in (2, 3) or entropy.dim() != 3 or int(entropy.shape[2]) != (4 ** L - 1) // 3:
        raise ValueError(f'uncertainty_map: expected [B, n, {(4 ** L - 1) // 3 if L in (2, 3) else "draws"}] for {levels} code levels, got {tuple(entropy.shape)}')
    n = int(entropy.shape[1])
    K = int(round(n ** 0.5))
    if K * K != n:
        raise ValueError(f'uncertainty_map: n={n} top positions are not a square grid')
    first = [(4 ** l - 1) // 3 for l in range(L + 1)]             # level l holds the draws [first[l], first[l + 1])
    per_level = [entropy[:, :, first[l]:first[l + 1]] for l in range(L)]
    per_level[0] = per_level[0][:, :, 0]
    return list(rearrange_levels(per_level, K))


def _score_report(eng, B: int, n: int, draws: int, report):
    """``report=N`` of the scoring calls -> the fresh ``DrawReport`` buffers the engine writes (None: none)."""
    from .engine import new_draw_report
    return None if report is None else new_draw_report(B, n, draws, report, eng.device)


def score_codes(stage2, codes, cond, precision: Optional[str] = None, one_pass: bool = False, score_chunk: Optional[int] = None, report: Optional[int] = None,
                **kw):
    """Log-probabilities of GIVEN codes under the model: ``codes`` = the code levels as one list, coarse to fine (int64 [B, n], [B, n, 4][, [B, n, 16]]),
    ``cond`` as in ``sampling_ihqgpt`` -> fp32 [B, n, draws], entry (b, t, d) the log-probability (T = 1, no cut-off) of the code of draw d at position t
    given the sample's codes before it: ``-sequence_logprob(...)`` is the stage-2 negative log-likelihood in nats.
    ``one_pass=False`` (the default): ONE sampler call with every level forced
    to ``codes`` (seed 0; its draws are discarded): teacher forcing through the sequential decode steps, so the cost is that of sampling n positions -- n
    decode steps --, not of one parallel pass.  ValueError for the 'bidirectional' depth head, where the sampling surface refuses forced codes too
    (``given_top_code``: the reference ignores them there).
    ``one_pass=True``: ``hqt_score`` -- the body once over all n rows per sample, the depth head over the B n (sample, position) pairs in chunks of
    ``score_chunk`` pairs (None: what the engine has, ``max_batch`` for a new one); the engine is asked for ``max_prefix = n - 1``.  Takes the 'bidirectional'
    head (nothing is forced in its depth pass); ValueError for 'top2mid2bot', which is scored stepwise only (``one_pass=False``).
    ``precision`` 'exact' | 'fast' | 'split' (default: ``use_fp16`` of ``kw``, i.e. FAST); further keywords: ``use_fp16``, ``lane``, ``use_graph`` (stepwise only).
    ``report=N`` (0..16; None: none), on either path: returns ``(logprobs, DrawReport)`` -- entropy and rank of every GIVEN code in the row it is scored under and,
    N >= 1, the N most likely codes there (``hqt_set_draw_report``; ``uncertainty_map`` folds the entropies into one grid per level)."""
    spec = stage2.spec
    report = _report_n(spec, report)                 # refused here, before an engine is built
    if one_pass:
        from .engine import check_score_codes
        check_score_codes(spec, codes, 'score_codes(one_pass=True)')
    elif spec.depth_decoding == 'bidirectional':
        raise ValueError("score_codes forces every code level, which the 'bidirectional' depth head does not support (as with given_top_code: the reference ignores it there); "
                         'one_pass=True scores it')
    codes = [torch.as_tensor(c) for c in codes]
    if len(codes) != spec.levels or codes[0].dim() != 2:
        raise ValueError(f'codes: expected the {spec.levels} code levels as one list, coarse to fine, the first of shape [B, n]')
    use_fp16, lane = kw.pop('use_fp16', True), kw.pop('lane', 0)
    unknown = set(kw) - {'use_graph'}
    if unknown:
        raise TypeError(f'score_codes: unexpected keywords {sorted(unknown)}')
    n = int(codes[0].shape[1])
    B, cond = _batch_and_cond(stage2, int(codes[0].shape[0]), cond)
    if B != int(codes[0].shape[0]):
        raise ValueError(f'codes hold {int(codes[0].shape[0])} samples, cond {B}')
    if one_pass:
        eng = stage2.engine(B, n, lane, max_prefix=n - 1, score_chunk=score_chunk)
        rep = _score_report(eng, B, n, (4 ** spec.levels - 1) // 3, report)
        logprobs = eng.score(B, cond, codes, precision=_precision(precision, use_fp16), report_out=rep)
        return logprobs if rep is None else (logprobs, rep)
    eng = stage2.engine(B, n, lane)
    rep = _score_report(eng, B, n, (4 ** spec.levels - 1) // 3, report)
    common = dict(precision=_precision(precision, use_fp16), seed=0, return_logprobs=True, report_out=rep, **kw)
    if spec.levels == 3:
        logprobs = eng.sample3(B, cond, n, force=codes, **common)[-1]
    else:
        logprobs = eng.sample(B, cond, n, force_top=codes[0], force_bot=codes[1], **common)[-1]
    return logprobs if rep is None else (logprobs, rep)


def score_images(model, images: torch.Tensor, cond=None, encode_precision: Optional[str] = None, report: Optional[int] = None, **score_kw):
    """Stage-2 log-likelihood of real images: ``images`` fp32 [B, 3, R, R] in [-1, 1] -> ``stage1.code_grids`` -> ``grids_to_sequences`` ->
    ``score_codes(one_pass=True)`` (``score_kw``: its further keywords, ``one_pass=False`` among them).  Returns ``(sequence_logprob fp64 [B], codes)``, the codes in
    the sampler's layout; ``report=N`` appends the ``DrawReport`` of the image's own codes -- ``uncertainty_map(report.entropy, levels)`` is an anomaly map over it."""
    codes = grids_to_sequences(list(model.stage1.code_grids(images, precision=encode_precision)))
    score_kw.setdefault('one_pass', True)
    if report is None:
        return sequence_logprob(score_codes(model.stage2, codes, cond, **score_kw)), codes
    logprobs, rep = score_codes(model.stage2, codes, cond, report=report, **score_kw)
    return sequence_logprob(logprobs), codes, rep


def session_cutoffs(levels: int, kw: dict) -> Tuple[tuple, tuple, tuple]:
    """Sampler keywords of ``sampling_ihqgpt`` (two levels) / ``sampling_hqtransformer`` (three; missing = the sampler's default) ->
    ``(top_k, top_p, temperature)`` per level, what ``Engine.sample`` / ``sample3`` take."""
    L = int(levels)
    if L == 3:
        top_k, top_p = (tuple(kw[k]) if kw.get(k) is not None else (None,) * 3 for k in ('top_k', 'top_p'))
    else:
        top_k, top_p = (kw.get('top_k_top'), kw.get('top_k_bot')), (kw.get('top_p_top'), kw.get('top_p_bot'))
    t = kw.get('softmax_temperature')
    temperature = tuple(float(v) for v in t) if t is not None else (1.0,) * L
    if not (len(temperature) == len(top_k) == len(top_p) == L):
        raise ValueError(f'sampler settings of a {L}-level model need {L} entries each, got {kw}')
    return top_k, top_p, temperature


class SamplingSession:
    """A sampling pass that can stop between two positions (``hqt_set_segment`` / ``hqt_select_rows``): ``advance`` draws the next positions, ``select``
    re-maps the rows -- reorder, drop, fork -- and ``finish`` draws what remains.  All segments together draw bit for bit what ONE sampler call with the same
    keys draws: ``SamplingSession(stage2, B, cond, n, seed=s).finish()`` equals ``sampling_ihqgpt(stage2, B, cond, max_seq_len=n, seed=s)``.
    The session owns the code tensors (``codes``: the levels as one list, full length; positions >= ``position`` are not drawn yet), the optional
    log-probabilities (``return_logprobs=True``: fp32 [B, n, draws], NaN where not drawn), the optional draw report (``return_report=N``: ``report``, a
    ``DrawReport`` of [B, n, draws(, N)] tensors, NaN / -1 where not drawn; ``select`` re-maps its rows with the log-probabilities) and one explicit Philox key per row -- ``row_seeds`` / ``row_offsets``,
    default ``(seed, sample_offset + b)``, the implicit keys of a plain call -- so that a row keeps its identity, and goes on drawing what it would have drawn,
    wherever ``select`` puts it.  ``cond`` as in ``sampling_ihqgpt``; ``sampler``: its sampler keywords (``top_k_top`` ... / ``top_k``, ``top_p``,
    ``softmax_temperature``), ``row_samplers`` and ``guidance`` (a ready pair table over the rows), the defaults of every ``advance``.
    ``share_prompts`` (text models): the first segment prefills every distinct prompt once.  One session at a time per engine lane: any other sampling or scoring
    call on the lane ends the paused pass, and the next ``advance`` raises ``HqtError``.  Not with ``prefix_codes``, ``keep_mask`` or ``guidance_scale``."""
    _DEFAULTS = SAMPLER_KEYS + ('row_samplers', 'guidance')

    def __init__(self, stage2, num_candidates: int, cond, n: int = 64, *, seed: Optional[int] = None, sample_offset: int = 0, row_seeds=None,
                 row_offsets=None, precision: Optional[str] = None, use_fp16: bool = True, use_graph: bool = True, lane: int = 0,
                 return_logprobs: bool = False, share_prompts: bool = False, return_report: Optional[int] = None, **sampler):
        top_n = _report_n(stage2.spec, return_report)
        unknown = set(sampler) - set(self._DEFAULTS)
        if unknown:
            raise TypeError(f'SamplingSession: unexpected keywords {sorted(unknown)} (sampler settings, row_samplers and guidance travel here)')
        self.stage2, self.L, self.n = stage2, int(stage2.spec.levels), int(n)
        if not 1 <= self.n <= stage2.spec.ctx_len_img:
            raise ValueError(f'n={self.n} outside [1, ctx_len_img={stage2.spec.ctx_len_img}]')
        self.B, self.cond = _batch_and_cond(stage2, int(num_candidates), cond)
        if share_prompts and not stage2.use_txt_cond:
            raise ValueError('share_prompts needs a text-conditional model: one embedding row per sample leaves no prefill to share')
        session_cutoffs(self.L, sampler)
        self.sampler, self.share_prompts = dict(sampler), bool(share_prompts)
        if (row_seeds is None) != (row_offsets is None):
            raise ValueError('row_seeds and row_offsets come together')
        if row_seeds is None:
            seed = _seed_from_torch() if seed is None else int(seed)
            row_seeds, row_offsets = [seed] * self.B, [int(sample_offset) + b for b in range(self.B)]
        if len(row_seeds) != self.B or len(row_offsets) != self.B:
            raise ValueError(f'row_seeds and row_offsets: {self.B} entries each')
        self.row_seeds, self.row_offsets = [int(v) for v in row_seeds], [int(v) for v in row_offsets]
        self.precision, self.use_graph = _precision(precision, use_fp16), bool(use_graph)
        self.engine = stage2.engine(self.B, self.n, lane)
        dev = self.engine.device
        self.position = 0
        self.codes = [torch.zeros((self.B, self.n) + ((4 ** l,) if l else ()), dtype=torch.int64, device=dev) for l in range(self.L)]
        self.logprobs = torch.full((self.B, self.n, (4 ** self.L - 1) // 3), float('nan'), dtype=torch.float32, device=dev) if return_logprobs else None
        self.report = None if top_n is None else new_draw_report(self.B, self.n, (4 ** self.L - 1) // 3, top_n, dev)

    @property
    def done(self) -> bool:
        return self.position >= self.n

    def advance(self, k: Optional[int] = None, force=None, **overrides) -> list:
        """Draws the next ``k`` positions (None: all that remain) and returns the codes so far, ``[c[:, :position] for c in codes]``.  ``overrides``: sampler
        keywords, ``row_samplers`` or ``guidance`` for THIS call in place of the session's; ``force``: one entry per level, None or a full-length code tensor
        fed forward in place of the draws (``force_top`` / ``force_bot`` of ``Engine.sample``).  Codes of position ``position - 1`` that the caller has edited in
        ``codes`` are what the pass goes on from -- for a level that is NOT forced: the engine reads the previous codes of a forced level from its ``force``
        tensor, which must therefore hold the code of position ``position - 1`` as well as those of the positions this call draws."""
        unknown = set(overrides) - set(self._DEFAULTS)
        if unknown:
            raise TypeError(f'advance: unexpected keywords {sorted(unknown)}')
        if self.done:
            raise ValueError(f'the session is finished: all {self.n} positions are drawn')
        k = self.n - self.position if k is None else int(k)
        if k < 1 or self.position + k > self.n:
            raise ValueError(f'advance(k={k}) at position {self.position}: expected 1 <= k <= {self.n - self.position} remaining positions')
        kw = {**self.sampler, **overrides}
        top_k, top_p, temperature = session_cutoffs(self.L, kw)
        start, stop = self.position, self.position + k
        cond, extra = self.cond, {}
        if self.share_prompts and start == 0:
            cond, extra['prompt_groups'] = prompt_groups_of(self.cond)
        force = [None] * self.L if force is None else list(force)
        if len(force) != self.L:
            raise ValueError(f'force: expected one entry per code level ({self.L}), None where a level is drawn')
        common = dict(precision=self.precision, top_k=top_k, top_p=top_p, temperature=temperature, seed=0, use_graph=self.use_graph,
                      row_seeds=self.row_seeds, row_offsets=self.row_offsets, row_samplers=kw.get('row_samplers'), guidance=kw.get('guidance'),
                      out=self.codes, segment=(start, stop), logprobs_out=self.logprobs, report_out=self.report, **extra)
        if self.L == 3:
            self.engine.sample3(self.B, cond, self.n, force=force, **common)
        else:
            self.engine.sample(self.B, cond, self.n, force_top=force[0], force_bot=force[1], **common)
        self.position = stop
        return [c[:, :stop] for c in self.codes]

    def select(self, rows_from, row_seeds=None, row_offsets=None, guidance=None) -> None:
        """Row j of the session becomes what row ``rows_from[j]`` was: the K/V cache (one gather on the device, ``hqt_select_rows``), the codes, the
        log-probabilities, the conditions, the Philox keys and the session's ``row_samplers`` table.  Any mapping: a permutation, a subset (prune), duplicates
        (fork).  Rows that share a key go on drawing the same codes; ``row_seeds`` / ``row_offsets`` (both, one entry per NEW row) give forked rows keys of
        their own.  A session built with a ``guidance`` pair table names rows by index, which no mapping carries over: ``guidance=`` gives the table over the
        NEW rows (``[]``: none from here on), and ValueError without it."""
        if self.done:
            raise ValueError('select on a finished session: nothing is left to draw')
        table = check_select_rows(rows_from, self.B, self.engine.max_batch)
        if self.sampler.get('guidance') and guidance is None:
            raise ValueError('select: the session\'s guidance pairs name rows by index -- pass guidance= with the pair table over the new rows ([]: none)')
        if (row_seeds is None) != (row_offsets is None):
            raise ValueError('row_seeds and row_offsets come together')
        if row_seeds is not None and (len(row_seeds) != len(table) or len(row_offsets) != len(table)):
            raise ValueError(f'row_seeds and row_offsets: {len(table)} entries each, one per new row')
        if self.position > 0:                        # (before the first position the cache holds nothing of this pass)
            self.engine.select_rows(table, self.B)
        rows = [int(r) for r in table]
        idx = torch.as_tensor(rows, dtype=torch.int64, device=self.codes[0].device)
        self.codes = [c.index_select(0, idx) for c in self.codes]
        if self.logprobs is not None:
            self.logprobs = self.logprobs.index_select(0, idx)
        if self.report is not None:
            self.report = DrawReport(*(None if f is None else f.index_select(0, idx) for f in self.report))
        if self.cond is not None:
            self.cond = torch.as_tensor(self.cond)
            self.cond = self.cond.index_select(0, idx.to(self.cond.device))
        self.row_seeds = [self.row_seeds[r] for r in rows] if row_seeds is None else [int(v) for v in row_seeds]
        self.row_offsets = [self.row_offsets[r] for r in rows] if row_offsets is None else [int(v) for v in row_offsets]
        if self.sampler.get('row_samplers') is not None:
            self.sampler['row_samplers'] = [self.sampler['row_samplers'][r] for r in rows]
        if guidance is not None:
            self.sampler['guidance'] = list(guidance) or None
        self.B = len(rows)

    def finish(self) -> list:
        """Draws what remains (nothing, when the session is done) and returns the full-length codes."""
        if not self.done:
            self.advance()
        return self.codes


class RollingSampler:
    """A rolling pass (``hqt_set_row_positions``): ``slots`` rows in which every request stands at its own position.  ``submit`` queues one request (one image:
    its class id -- None for an unconditional model --, its Philox seed and global row offset, its own sampler keywords), ``step`` admits queued requests into
    free slots at position 0 while their neighbours are mid-image, runs ONE engine call of ``k`` steps over all slots, and returns the requests that drew their
    last position in it; ``drain`` steps until nothing is queued or live.  A request draws bit for bit what the plain call of the same batch draws for it in its
    slot -- in EXACT arithmetic, where a row's draws do not depend on the pass it sits in, what ``sampling_ihqgpt(stage2, 1, cond, max_seq_len=n, seed=seed)`` draws.
    The sampler holds the slot bookkeeping on the host (free list, positions, keys, conditions, the row-sampler table) and the code tensors of the pass on the
    device; one rolling pass at a time per engine lane (any other sampling or scoring call on the lane ends it, and the next ``step`` raises ``HqtError``).
    Text models need ``max_joins`` (1 <= max_joins <= slots): a row that joins at position 0 needs a prompt prefill of its own, whose staging the engine sizes for
    that many joining rows per call (``hqt_set_max_joins``); without it they are refused.  ``submit(cond=...)`` then takes one prompt of ``ctx_len_txt`` token ids,
    ``step`` admits at most ``max_joins`` requests per call, and a request that joins in a call advances by 1 + k in it -- the join draws position 0 in front of
    the k steps --, every other by k.
    ``join_run=R`` (``hqt_set_join_run``; the stage-2 engine must be built with ``max_prefix`` >= R) lets a request bring cells that are GIVEN:
    ``submit(..., keep_mask=[n] bool, kept_codes=[[n], [n, 4][, [n, 16]]])``.  Kept cells are returned verbatim and everything else is drawn around them.  The
    requests that join in one call prefill the leading kept run they share, clipped to min(run, R, n - 1), in the call's join phase and advance by run + 1 + k in
    it; a kept cell behind the run is an ordinary step whose draw is discarded.  Admission stays in submission order: the head of the queue decides the run of
    the call, and admission stops at the first queued request whose clipped run differs -- it joins in the next call."""

    def __init__(self, stage2, slots: int, n: int, max_joins: Optional[int] = None, *, precision: Optional[str] = None, use_fp16: bool = True, use_graph: bool = True,
                 lane: int = 0, return_logprobs: bool = False, return_report: Optional[int] = None, join_run: Optional[int] = None):
        top_n = _report_n(stage2.spec, return_report)
        self.text_cond = bool(stage2.use_txt_cond)
        if self.text_cond and not max_joins:
            raise ValueError('RollingSampler: a rolling pass on a text-conditional model is not built (a row that joins at position 0 needs a prompt prefill of its own)'
                             ' unless max_joins= sizes one: RollingSampler(stage2, slots, n, max_joins=J) with 1 <= J <= slots')
        if max_joins is not None and not self.text_cond:
            raise ValueError('max_joins: only a text-conditional model prefills the rows that join (any other model joins without a prefill)')
        if self.text_cond and (isinstance(max_joins, bool) or not 1 <= int(max_joins) <= int(slots)):
            raise ValueError(f'max_joins={max_joins!r} outside [1, slots = {int(slots)}]')
        self.max_joins = int(max_joins) if self.text_cond else None
        self.stage2, self.L, self.slots, self.n = stage2, int(stage2.spec.levels), int(slots), int(n)
        if self.slots < 1:
            raise ValueError(f'slots={self.slots}: a rolling pass needs at least one slot')
        if not 1 <= self.n <= stage2.spec.ctx_len_img:
            raise ValueError(f'n={self.n} outside [1, ctx_len_img={stage2.spec.ctx_len_img}]')
        self.precision, self.use_graph = _precision(precision, use_fp16), bool(use_graph)
        if join_run is not None and (isinstance(join_run, bool) or not isinstance(join_run, (int, np.integer)) or not 0 <= int(join_run) <= self.n - 1):
            raise ValueError(f'join_run={join_run!r} outside [0, n - 1 = {self.n - 1}]')
        self.join_run = None if join_run is None else int(join_run)
        if self.join_run and self.text_cond and self.L == 3:
            raise ValueError(f'join_run={self.join_run}: a kept run is not prefilled on a text-conditional model with three code levels (join_run=0 is built)')
        extra = {} if not self.join_run else {'max_prefix': self.join_run}
        self.engine = stage2.engine(self.slots, self.n, lane, max_joins=self.max_joins, **extra) if self.text_cond else stage2.engine(self.slots, self.n, lane, **extra)
        dev = self.engine.device
        if self.join_run is not None:
            if int(getattr(self.engine, 'max_prefix', 0)) < self.join_run:
                raise ValueError(f'join_run={self.join_run} exceeds max_prefix={int(getattr(self.engine, "max_prefix", 0))} of the stage-2 engine')
            self.engine.set_join_run(self.max_joins if self.text_cond else self.slots, self.join_run)
        self.codes = [torch.full((self.slots, self.n) + ((4 ** l,) if l else ()), -1, dtype=torch.int64, device=dev) for l in range(self.L)]
        # the pass's keep table: the mask on the host, the kept codes in device tensors shaped like the codes (an empty or plain slot: nothing kept)
        self.keep_mask = np.zeros((self.slots, self.n), dtype=bool)
        self.kept = [torch.zeros_like(c) for c in self.codes] if self.join_run is not None else None
        self.logprobs = torch.full((self.slots, self.n, (4 ** self.L - 1) // 3), float('nan'), dtype=torch.float32, device=dev) if return_logprobs else None
        self.report = None if top_n is None else new_draw_report(self.slots, self.n, (4 ** self.L - 1) // 3, top_n, dev)
        self.class_cond = bool(stage2.spec.cond == 1)
        default = step_row_samplers(self.L, [1], [{}])[0]
        # per slot: the position it draws next (-1: empty), its request's ticket, condition, key and sampler settings
        self.pos, self.ticket = [-1] * self.slots, [None] * self.slots
        self.cond, self.row_seeds, self.row_offsets = [0] * self.slots, [0] * self.slots, [0] * self.slots
        if self.text_cond:                           # per slot one prompt; an empty slot's row is never read (token 0 is inside every vocabulary)
            self.cond = [[0] * int(stage2.spec.ctx_len_txt) for _ in range(self.slots)]
        self.row_samplers = [default] * self.slots
        self.free = list(range(self.slots))          # ascending: a request joins in the lowest free slot
        self.queue: list = []
        self.tickets = 0

    @property
    def live(self) -> int:
        return sum(p >= 0 for p in self.pos)

    def _check_kept(self, keep_mask, kept_codes):
        """``keep_mask`` / ``kept_codes`` of one request: (mask as a bool numpy array [n], the levels as int64 host tensors), or None without a mask."""
        if keep_mask is None and kept_codes is None:
            return None
        if self.join_run is None:
            raise ValueError('keep_mask / kept_codes: this rolling pass takes no given cells; build it with RollingSampler(..., join_run=R)')
        if keep_mask is None or kept_codes is None:
            raise ValueError('keep_mask and kept_codes come together')
        m = torch.as_tensor(keep_mask).cpu()
        if tuple(m.shape) != (self.n,) or m.dtype.is_floating_point:
            raise ValueError(f'keep_mask: expected bool of shape ({self.n},), got {m.dtype} of shape {tuple(m.shape)}')
        m = (m != 0).numpy().astype(bool)
        if not isinstance(kept_codes, (list, tuple)) or len(kept_codes) != self.L:
            raise ValueError(f'kept_codes: expected the {self.L} code levels as one list, coarse to fine')
        levels, V = [], int(self.stage2.spec.vocab_top)
        for l, c in enumerate(kept_codes):
            t = torch.as_tensor(c).cpu()
            want = (self.n,) + ((4 ** l,) if l else ())
            if tuple(t.shape) != want or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f'kept_codes[{l}]: expected integer codes of shape {want}, got {t.dtype} of shape {tuple(t.shape)}')
            t = t.to(torch.int64)
            if m.any():
                sel = t[torch.from_numpy(m)]
                lo, hi = int(sel.min()), int(sel.max())
                if lo < 0 or hi >= V:
                    raise IndexError(f'kept_codes[{l}]: index out of range (values span [{lo}, {hi}], table has {V} rows)')
            levels.append(t)
        return m, levels

    def _run_of(self, kept) -> int:
        """The leading kept run a request prefills when it joins: its count of leading ones clipped to min(join_run, n - 1); 0 without given cells."""
        if kept is None or not self.join_run:
            return 0
        m = kept[0]
        run = self.n if m.all() else int(np.argmin(m))
        return min(run, self.join_run, self.n - 1)

    def submit(self, cond, seed: int, sample_offset: int = 0, keep_mask=None, kept_codes=None, **sampler) -> int:
        """Queues one request and returns its ticket.  ``sampler``: the sampler keywords of ``sampling_ihqgpt`` / ``sampling_hqtransformer``; they travel as the
        ``row_samplers`` entry of the slot the request is admitted to.  ``keep_mask`` [n] bool and ``kept_codes`` (one tensor per level: [n], [n, 4][, [n, 16]]; read
        where the mask is set, IndexError outside the vocabulary there): the cells of the request that are given (a pass built with ``join_run=``)."""
        unknown = set(sampler) - set(SAMPLER_KEYS)
        if unknown:
            raise TypeError(f'submit: unexpected keywords {sorted(unknown)} (sampler settings travel here)')
        kept = self._check_kept(keep_mask, kept_codes)
        if self.class_cond:
            if cond is None or isinstance(cond, bool) or not 0 <= int(cond) < self.stage2.spec.n_classes:
                raise ValueError(f'cond={cond!r}: a class id in [0, {self.stage2.spec.n_classes}) is required')
            cond = int(cond)
        elif self.text_cond:
            T, V = int(self.stage2.spec.ctx_len_txt), int(self.stage2.spec.vocab_txt)
            ids = None if cond is None else torch.as_tensor(cond).cpu()
            if ids is None or ids.dtype.is_floating_point or ids.dtype == torch.bool or tuple(ids.shape) != (T,):
                raise ValueError(f'cond: one prompt of ctx_len_txt = {T} token ids is required' + ('' if ids is None else f', got {ids.dtype} of shape {tuple(ids.shape)}'))
            if int(ids.min()) < 0 or int(ids.max()) >= V:
                raise ValueError(f'cond: token ids span [{int(ids.min())}, {int(ids.max())}], outside the text vocabulary [0, vocab_txt = {V})')
            cond = [int(v) for v in ids.tolist()]
        elif cond is not None:
            raise ValueError('cond: an unconditional model takes None')
        entry = step_row_samplers(self.L, [1], [sampler])[0]
        ticket, self.tickets = self.tickets, self.tickets + 1
        self.queue.append((ticket, cond or 0, int(seed), int(sample_offset), entry, kept))
        return ticket

    def step(self, k: int = 1) -> list:
        """Admits queued requests into free slots (in submission order, lowest free slot first), runs one rolling call of ``k`` steps and returns the requests
        that finished in it as ``(ticket, codes[, logprobs][, report])``: ``codes`` the levels as one list, [n], [n, 4][, [n, 16]], gathered on the device;
        ``report`` (``return_report=N``): the request's ``DrawReport`` slice, [n, draws(, N)] per field.  A slot freed
        in this call takes a new request in the next one.  Nothing queued or live: no engine call, []."""
        k = int(k)
        if not 1 <= k <= self.n:
            raise ValueError(f'step(k={k}): expected 1 <= k <= n = {self.n}')
        admitted, run = 0, 0                         # the joiners of one call share one clipped leading run: the queue's head decides it
        while self.queue and self.free and (self.max_joins is None or admitted < self.max_joins):
            if admitted and self._run_of(self.queue[0][5]) != run:
                break                                # (it joins in the next call, as the head of the queue)
            run = self._run_of(self.queue[0][5])
            admitted += 1
            slot = self.free.pop(0)
            self.ticket[slot], self.cond[slot], self.row_seeds[slot], self.row_offsets[slot], self.row_samplers[slot], kept = self.queue.pop(0)
            self.pos[slot] = 0
            if self.kept is not None:
                self.keep_mask[slot] = kept[0] if kept is not None else False
                for dst, src in zip(self.kept, kept[1] if kept is not None else ()):
                    dst[slot] = src.to(dst.device)
        if not self.live:
            return []
        cond = torch.tensor(self.cond, dtype=torch.int64) if self.class_cond or self.text_cond else None
        common = dict(precision=self.precision, seed=0, use_graph=self.use_graph, row_seeds=list(self.row_seeds), row_offsets=list(self.row_offsets),
                      row_samplers=list(self.row_samplers), out=self.codes, logprobs_out=self.logprobs, report_out=self.report,
                      row_positions=(list(self.pos), k))
        if self.kept is not None:                    # every call of the pass stages the table: the captured steps stay the same whether a live request keeps cells or not
            common['keep'] = (torch.from_numpy(self.keep_mask.copy()), self.kept)
        if self.L == 3:
            self.engine.sample3(self.slots, cond, self.n, **common)
        else:
            self.engine.sample(self.slots, cond, self.n, **common)
        # the record the library keeps: a row that joined through a join phase (a text pass; a kept run to prefill) drew position `run` there, in front of the k steps
        joined = run + 1 if admitted and (self.text_cond or run > 0) else 0
        moved = [p if p < 0 else p + k + (joined if p == 0 else 0) for p in self.pos]
        done = [s for s in range(self.slots) if self.pos[s] >= 0 and moved[s] >= self.n]
        self.pos = [-1 if p < 0 or p >= self.n else p for p in moved]
        if not done:
            return []
        idx = torch.as_tensor(done, dtype=torch.int64, device=self.codes[0].device)
        codes = [c.index_select(0, idx) for c in self.codes]
        logprobs = self.logprobs.index_select(0, idx) if self.logprobs is not None else None
        report = None if self.report is None else [None if f is None else f.index_select(0, idx) for f in self.report]
        out = []
        for i, s in enumerate(done):
            out.append((self.ticket[s], [c[i] for c in codes]) + ((logprobs[i],) if logprobs is not None else ())
                       + ((DrawReport(*(None if f is None else f[i] for f in report)),) if report is not None else ()))
            self.ticket[s] = None
            self.keep_mask[s] = False
        self.free = sorted(self.free + done)
        return out

    def drain(self, k: int = 1) -> list:
        """Steps until nothing is queued or live; returns every request that finished on the way, in the order they finished."""
        out = []
        while self.queue or self.live:
            out.extend(self.step(k))
        return out


def check_prune(prune, num_candidates: int, keep: int, n: int) -> list:
    """``prune`` of ``sample_best_of`` checked on the host, before any engine is built: a list ``[(position, survivors_per_group), ...]`` with positions
    ascending inside [1, n - 1] and survivors descending, below ``num_candidates`` and never below ``keep``.  Returns it as a list of int pairs."""
    if not isinstance(prune, (list, tuple)) or not prune:
        raise ValueError('prune: expected a list [(position, survivors_per_group), ...]')
    plan, last_pos, last_s = [], 0, int(num_candidates)
    for entry in prune:
        if not isinstance(entry, (list, tuple)) or len(entry) != 2:
            raise ValueError(f'prune: expected (position, survivors_per_group) entries, got {entry!r}')
        pos, s = int(entry[0]), int(entry[1])
        if pos <= last_pos or pos >= int(n):
            raise ValueError(f'prune: positions must ascend inside [1, n - 1 = {int(n) - 1}], got {pos} after {last_pos}')
        if s >= last_s or s < int(keep):
            raise ValueError(f'prune: survivors must descend and stay at or above keep={int(keep)}, got {s} after {last_s}')
        plan.append((pos, s))
        last_pos, last_s = pos, s
    return plan


def prune_survivors(scores: torch.Tensor, survivors: int) -> torch.Tensor:
    """``scores`` [groups, candidates] -> int64 [groups, survivors]: per group the ``rank_candidates`` winners (ties to the lower index), listed in ASCENDING
    candidate index -- the order they keep among the rows of the pass, so that the final ranking breaks ties as the unpruned call does."""
    return torch.sort(rank_candidates(scores, survivors), dim=1).values


def _best_of_pruned(stage2, G: int, C: int, K: int, rows, plan, sampler: dict) -> Tuple[list, torch.Tensor]:
    for k in ('prefix_codes', 'keep_mask', 'kept_codes'):
        if sampler.get(k) is not None:
            raise ValueError(f'prune together with {k} is not built (segments of a pass with a code prefix or a keep table)')
    if sampler.get('guidance_scale') is not None or sampler.get('neg_cond') is not None:
        raise ValueError('prune together with guidance_scale is not built: lay the rows out yourself (SamplingSession, guidance=)')
    sampler = {k: v for k, v in sampler.items() if k not in ('is_tqdm', 'model_stage1')}
    n = int(sampler.pop('max_seq_len', 256))
    session = SamplingSession(stage2, G * C, rows, n, return_logprobs=True, **sampler)
    cur = C
    for pos, s in plan:
        session.advance(pos - session.position)
        scores = sequence_logprob(session.logprobs[:, :pos]).reshape(G, cur)
        idx = prune_survivors(scores, s)                                       # [G, s], candidate indices among the cur rows of the group
        session.select((idx + torch.arange(G, device=idx.device).unsqueeze(1) * cur).reshape(-1).cpu())
        cur = s
    codes = session.finish()
    scores = sequence_logprob(session.logprobs).reshape(G, cur)
    idx = rank_candidates(scores, K)
    flat = (idx + torch.arange(G, device=idx.device).unsqueeze(1) * cur).reshape(-1)
    return [c.index_select(0, flat) for c in codes], scores.gather(1, idx)


def sample_best_of(stage2, cond, num_candidates: int, keep: int, share_prompts: bool = False, prune=None, **sampler) -> Tuple[list, torch.Tensor]:
    """Sample ``num_candidates`` per condition and keep the ``keep`` most likely: ``cond`` = class ids (an int, or a tensor / list of G ids), text prompts
    [G, ctx_len_txt], or anything for an unconditional model (one group).  ONE sampler call over all G * num_candidates rows (group-major: row
    g * num_candidates + c), keywords of ``sampling_ihqgpt`` / ``sampling_hqtransformer`` in ``sampler``; every candidate is scored by
    ``sequence_logprob`` of its own draws (the model's log-probability at T = 1, whatever temperature and cut-offs drew it; with ``prefix_codes`` over
    the completed positions only; with ``guidance_scale`` -- ``neg_cond`` then per group, like ``cond`` -- under the guided logits) and ranked within its group, descending, ties to the lower candidate index; codes and scores are gathered on the
    device.  Returns ``(codes, scores)``: the code levels as one list, [G * keep, n], [G * keep, n, 4][, ...], group-major, best first, and fp64 [G, keep].
    ``share_prompts=True`` (text models): the ``num_candidates`` rows of a caption are one prompt -- it is prefilled once and handed to them
    (``sampling_ihqgpt``; with ``guidance_scale`` the negative rows are deduplicated too).
    ``prune`` = ``[(position, survivors_per_group), ...]`` (positions ascending, survivors descending, never below ``keep``): the pass stops behind each
    position, ranks every group by ``sequence_logprob`` of the positions drawn so far (ties to the lower candidate index) and goes on with the survivors only
    (``SamplingSession.select``), so a discarded candidate costs the positions up to its cut, not all of them.  Survivors draw what they draw unpruned (their
    Philox keys travel with them; bit for bit in 'exact').  None: the one call above, untouched.  Not together with ``prefix_codes``, ``keep_mask`` or
    ``guidance_scale``."""
    C, K = int(num_candidates), int(keep)
    if not 1 <= K <= C:
        raise ValueError(f'keep={K} outside [1, num_candidates={C}]')
    plan = None if prune is None else check_prune(prune, C, K, int(sampler.get('max_seq_len', 256)))
    if stage2.use_txt_cond:
        cond = torch.as_tensor(cond)
        if cond.dim() != 2:
            raise ValueError('text conditioning expects cond of shape [G, ctx_len_txt]')
        G = int(cond.shape[0])
        rows = cond.repeat_interleave(C, dim=0)
    elif stage2.use_cls_cond:
        ids = torch.as_tensor(cond).reshape(-1).to(torch.int64)
        G = int(ids.numel())
        rows = ids.repeat_interleave(C)
    else:
        G, rows = 1, cond
    if sampler.get('neg_cond') is not None and not isinstance(sampler['neg_cond'], int):      # per group, like cond: one row per candidate
        neg = torch.as_tensor(sampler['neg_cond'])
        neg = neg.reshape(-1, int(neg.shape[-1])) if stage2.use_txt_cond else neg.reshape(-1)
        sampler['neg_cond'] = neg.repeat_interleave(C, dim=0) if int(neg.shape[0]) == G and G > 1 else neg
    if share_prompts:
        sampler['share_prompts'] = True
    if plan is not None:
        return _best_of_pruned(stage2, G, C, K, rows, plan, sampler)
    *codes, logprobs = sample_codes(stage2, G * C, rows, return_logprobs=True, **sampler)
    prefix = sampler.get('prefix_codes')
    P = 0 if prefix is None else int(torch.as_tensor(prefix[0]).shape[-1])
    scores = sequence_logprob(logprobs[:, P:]).reshape(G, C)
    idx = rank_candidates(scores, K)                                           # [G, K], on the device
    flat = (idx + torch.arange(G, device=idx.device).unsqueeze(1) * C).reshape(-1)
    return [c.index_select(0, flat) for c in codes], scores.gather(1, idx)


def grids_to_sequences(grids: list) -> list:
    """Code grids [B, K << l, K << l], coarse to fine, -> the sampler's layout [B, K K], [B, K K, 4][, [B, K K, 16]]: the inverse of
    ``rearrange_levels`` ('B (H kerH) (W kerW) -> B (H W) (kerH kerW)')."""
    B, K = int(grids[0].shape[0]), int(grids[0].shape[-1])
    out = []
    for l, g in enumerate(grids):
        k = 2 ** l
        s = g.reshape(B, K, k, K, k).permute(0, 1, 3, 2, 4).reshape(B, K * K, k * k)
        out.append(s.reshape(B, K * K) if l == 0 else s.contiguous())
    return out


def _roll_images(rolling: 'RollingSampler', stage2, B: int, n: int, cond, mask: torch.Tensor, kept: list, sampler: dict) -> list:
    """``rolling=`` of ``complete_images`` / ``regenerate_region``: image b is ONE request of the rolling pass -- its condition, the key (seed, b) a plain call
    gives row b, its row of ``mask`` [B, n] and of ``kept`` -- and the pass is drained; -> the codes as the plain call returns them, [B, n], [B, n, 4][, ...].
    ``sampler`` may hold ``seed``, the sampler settings of ``RollingSampler.submit`` and ``steps_per_call`` (default 16); precision, graphs and the engine are the
    pass's own."""
    if not isinstance(rolling, RollingSampler) or rolling.stage2 is not stage2:
        raise ValueError('rolling: expected a RollingSampler over this model\'s stage 2')
    if rolling.n != int(n):
        raise ValueError(f'rolling: the pass has n={rolling.n} positions, the images have {int(n)}')
    if rolling.queue or rolling.live:
        raise ValueError('rolling: the pass holds requests of its own; drain it first (the images are submitted and drained together)')
    sampler = dict(sampler)
    sampler.pop('text_prefix', None)
    seed, k = sampler.pop('seed', None), int(sampler.pop('steps_per_call', 16))
    unknown = set(sampler) - set(SAMPLER_KEYS)
    if unknown:
        raise ValueError(f'rolling: {sorted(unknown)} belong to the RollingSampler the images join (its precision, graphs and lane), not to the call')
    seed = _seed_from_torch() if seed is None else int(seed)
    _, cond = _batch_and_cond(stage2, B, cond)
    kept = [c.cpu() for c in kept]
    tickets = [rolling.submit(None if cond is None else (cond[b] if cond.dim() == 2 else int(cond[b])), seed, sample_offset=b, keep_mask=mask[b],
                              kept_codes=[c[b] for c in kept], **sampler) for b in range(B)]
    done = {d[0]: d[1] for d in rolling.drain(max(1, min(k, rolling.n)))}
    return [torch.stack([done[t][l] for t in tickets]) for l in range(rolling.L)]


def complete_images(model, images: torch.Tensor, keep_rows: int, cond=None, encode_precision: Optional[str] = None,
                    decode_precision: Optional[str] = None, rolling: Optional['RollingSampler'] = None, **sampler) -> Tuple[torch.Tensor, list]:
    """Keep the first ``keep_rows`` rows of every image's top code grid and sample the rest: ``images`` fp32 [B, 3, R, R] in [-1, 1] (what
    ``stage1.get_codes`` takes) -> ``stage1`` codes -> the codes of the first ``P = keep_rows * top_resolution`` positions on every level (the
    bottom / middle grids cut at the matching rows) as ``prefix_codes`` of one sampler call over all ``top_resolution ** 2`` positions ->
    ``decode_codes``.  ``cond``: class ids as in ``sampling_ihqgpt``, or text prompts [B, ctx_len_txt] (two code levels: the prompt and the
    prefix then share one prefill, ``text_prefix=True`` of ``sampling_ihqgpt``); ``sampler``: further keywords of that sampler (cut-offs,
    temperatures, seed, precision ...).  Returns ``(pixels fp32 [B, 3, R, R] in [0, 1], codes)`` with ``codes`` the full-length code list, coarse to fine;
    its positions < P are the image's own codes.
    ``rolling=RollingSampler(stage2, slots, K K, join_run=R)``: every image joins that rolling pass as one request (key (seed, b), as row b of the plain call) and
    the pass is drained, instead of the one call: the images prefill min(P, R) of their kept positions in the join phase and may share the pass with other work
    between calls.  ``sampler`` then holds only ``seed``, sampler settings and ``steps_per_call``."""
    grids = list(model.stage1.code_grids(images, precision=encode_precision))
    K = int(grids[0].shape[-1])
    if not 1 <= int(keep_rows) < K:
        raise ValueError(f'keep_rows={keep_rows} outside [1, {K - 1}]: at least one row of the {K} x {K} top grid is kept and one is left to sample')
    P = int(keep_rows) * K
    prefix = [s[:, :P].contiguous() for s in grids_to_sequences(grids)]
    if rolling is not None:
        mask = torch.zeros((int(images.shape[0]), K * K), dtype=torch.bool)
        mask[:, :P] = True
        codes = _roll_images(rolling, model.stage2, int(images.shape[0]), K * K, cond, mask, grids_to_sequences(grids), sampler)
        return decode_codes(model.stage1, codes, decode_precision), codes
    if model.stage2.use_txt_cond and model.stage2.spec.levels == 2:
        sampler['text_prefix'] = True
    codes = sample_codes(model.stage2, int(images.shape[0]), cond, max_seq_len=K * K, prefix_codes=prefix, **sampler)
    return decode_codes(model.stage1, codes, decode_precision), codes


def box_keep_mask(K: int, box) -> torch.Tensor:
    """bool [K K]: the top positions OUTSIDE ``box = (r0, r1, c0, c1)`` (half-open, in cells of the K x K top grid), raster order -- the keep mask of one
    image whose box is drawn again.  ValueError unless 0 <= r0 < r1 <= K and 0 <= c0 < c1 <= K."""
    r0, r1, c0, c1 = (int(v) for v in box)
    if not (0 <= r0 < r1 <= K and 0 <= c0 < c1 <= K):
        raise ValueError(f'box={(r0, r1, c0, c1)}: expected (r0, r1, c0, c1) with 0 <= r0 < r1 <= {K} and 0 <= c0 < c1 <= {K} (half-open, top-grid cells)')
    keep = torch.ones((K, K), dtype=torch.bool)
    keep[r0:r1, c0:c1] = False
    return keep.reshape(-1)


def regenerate_region(model, images: torch.Tensor, box, cond=None, encode_precision: Optional[str] = None,
                      decode_precision: Optional[str] = None, rolling: Optional['RollingSampler'] = None, **sampler) -> Tuple[torch.Tensor, list]:
    """Draw a box of every image again and keep everything around it: ``images`` fp32 [B, 3, R, R] in [-1, 1] -> ``stage1`` codes -> one sampler call
    over all ``top_resolution ** 2`` positions that keeps every cell outside ``box = (r0, r1, c0, c1)`` (half-open, in top-grid cells) on every code
    level (``keep_mask`` / ``kept_codes`` of the samplers) and draws the inside, each position given everything before it in raster order -- the kept
    cells to the right of and below the box are not seen by the draws, as in any raster-order model -> ``decode_codes``.  ``cond`` and ``sampler`` as in
    ``complete_images``.  Returns ``(pixels fp32 [B, 3, R, R] in [0, 1], codes)``, the codes in the sampler's layout.  What is claimed is the mechanism,
    not the quality of the seam.  ``rolling=``: as in ``complete_images`` -- every image one request of that rolling pass, drained."""
    grids = list(model.stage1.code_grids(images, precision=encode_precision))
    B, K = int(images.shape[0]), int(grids[0].shape[-1])
    mask = box_keep_mask(K, box).unsqueeze(0).expand(B, K * K)
    if rolling is not None:
        codes = _roll_images(rolling, model.stage2, B, K * K, cond, mask, grids_to_sequences(grids), sampler)
        return decode_codes(model.stage1, codes, decode_precision), codes
    if model.stage2.use_txt_cond and model.stage2.spec.levels == 2:
        sampler['text_prefix'] = True
    codes = sample_codes(model.stage2, B, cond, max_seq_len=K * K, keep_mask=mask, kept_codes=grids_to_sequences(grids), **sampler)
    return decode_codes(model.stage1, codes, decode_precision), codes


def canvas_windows(G: int, w: int, s: int) -> list:
    """Offsets ``(oy, ox)`` of the w x w windows that tile a G x G canvas with stride s, over {0, s, ..., G - w} squared, in raster order.
    ValueError unless 1 <= s < w <= G and (G - w) % s == 0."""
    G, w, s = int(G), int(w), int(s)
    if not (1 <= s < w <= G) or (G - w) % s:
        raise ValueError(f'canvas_windows(G={G}, w={w}, s={s}): expected 1 <= s < w <= G and (G - w) % s == 0')
    steps = range(0, G - w + 1, s)
    return [(oy, ox) for oy in steps for ox in steps]


def canvas_keep_masks(G: int, w: int, s: int) -> list:
    """Per window of ``canvas_windows``, in its order: ``(oy, ox, keep bool [w, w])`` with ``keep`` the cells of the window that earlier windows filled."""
    filled = torch.zeros((G, G), dtype=torch.bool)
    out = []
    for oy, ox in canvas_windows(G, w, s):
        out.append((oy, ox, filled[oy:oy + w, ox:ox + w].clone()))
        filled[oy:oy + w, ox:ox + w] = True
    return out


def sample_canvas(model, cond, grid: int, stride: int, seed: int = 0, decode: bool = True, num_candidates: Optional[int] = None,
                  decode_precision: Optional[str] = None, **sampler) -> Tuple[list, Optional[torch.Tensor]]:
    """Sample a code canvas larger than the trained grid with a sliding window: the model's w x w top grid (w w = ctx_len_img) moves over a
    ``grid`` x ``grid`` canvas with ``stride`` (``canvas_windows``); window number k is ONE sampler call seeded ``seed + k`` whose keep mask is the
    cells of the window that earlier windows filled (``keep_mask`` / ``kept_codes`` of the samplers), and the cells it draws are written back to the canvas.
    ``cond``: as in ``sampling_ihqgpt``, the same for every window; ``num_candidates``: images B (default: one per entry of ``cond``); ``sampler``: further
    keywords of the sampler.  Returns ``(grids, pixels)``: the canvas code grids int64 [B, G, G], [B, 2 G, 2 G][, [B, 4 G, 4 G]] and, with ``decode``,
    pixels fp32 [B, 3, R G / w, R G / w] in [0, 1] from ``stage1.at_resolution`` (the same weights under a spec scaled by G / w: a second engine, built
    on first use), else None.  Square canvases only.  The model was trained on w x w grids with absolute positions: what is claimed is the mechanism --
    every window is an ordinary masked call that a plain forced call replays --, not the quality of the picture."""
    s2 = model.stage2.spec
    w = int(round(s2.ctx_len_img ** 0.5))
    if w * w != s2.ctx_len_img:
        raise ValueError(f'ctx_len_img={s2.ctx_len_img} is not a square grid')
    G, L = int(grid), s2.levels
    plan = canvas_keep_masks(G, w, int(stride))
    if num_candidates is None:
        num_candidates = 1 if isinstance(cond, int) or cond is None else int(torch.as_tensor(cond).shape[0])
    B = int(num_candidates)
    dev = model.stage2._device
    canvas = [torch.zeros((B, G << l, G << l), dtype=torch.int64, device=dev) for l in range(L)]
    for k, (oy, ox, keep) in enumerate(plan):
        window = [c[:, oy << l:(oy + w) << l, ox << l:(ox + w) << l] for l, c in enumerate(canvas)]
        codes = sample_codes(model.stage2, B, cond, seed=int(seed) + k, max_seq_len=w * w, keep_mask=keep.reshape(1, -1).expand(B, w * w),
                             kept_codes=grids_to_sequences(window), **sampler)
        for dst, g in zip(window, rearrange_levels(codes, w)):
            dst.copy_(g)                                 # the kept cells come back verbatim: only the cells this window owns change
    pixels = None
    if decode:
        R = model.stage1.spec.resolution
        if (R * G) % w:
            raise ValueError(f'a {G} x {G} canvas of a model with resolution {R} over a {w} x {w} grid has no integer resolution')
        pixels = (0.5 * model.stage1.at_resolution(R * G // w).decode_code(canvas, precision=decode_precision) + 0.5).clamp(0, 1)
    return canvas, pixels


def step_keep_table(levels: int, sizes, n: int, sample_kws) -> Tuple[torch.Tensor, list]:
    """Steps of a pass with mixed prefixes -> its keep table: step i's ``prefix_codes`` (``sample_kws[i]``; none: nothing kept) become its ``sizes[i]`` rows
    of ``(mask bool [N, n], codes [N, n], [N, n, 4][, [N, n, 16]])`` -- row r of a step with a prefix of P positions keeps its first P positions.  The result is
    ``keep_mask=`` / ``kept_codes=`` of the samplers; the leading run all rows share, i.e. the shortest prefix, is the pass's one prefill."""
    N = sum(int(b) for b in sizes)
    mask = torch.zeros((N, int(n)), dtype=torch.bool)
    where = next((torch.as_tensor(kw['prefix_codes'][0]).device for kw in sample_kws if kw.get('prefix_codes') is not None), torch.device('cpu'))
    codes = [torch.zeros((N, int(n)) + ((4 ** l,) if l else ()), dtype=torch.int64, device=where) for l in range(int(levels))]
    lo = 0
    for b, kw in zip(sizes, sample_kws):
        prefix = kw.get('prefix_codes')
        if prefix is not None:
            P = int(torch.as_tensor(prefix[0]).shape[-1])
            if len(prefix) != int(levels) or not 1 <= P < int(n):
                raise ValueError(f'prefix_codes: expected the {int(levels)} code levels with 1 <= P <= {int(n) - 1} positions')
            mask[lo:lo + int(b), :P] = True
            for c, p in zip(codes, prefix):
                c[lo:lo + int(b), :P] = torch.as_tensor(p).to(where, torch.int64)
        lo += int(b)
    return mask, codes


def _public(codes: list) -> tuple:
    return codes[0], (codes[1] if len(codes) == 2 else codes[1:])


def _levels_of(ct, cb) -> list:
    return [ct, *cb] if isinstance(cb, (list, tuple)) else [ct, cb]


def _rows(ct, cb, px, lo: int, n: int) -> tuple:
    """Rows [lo, lo + n) of a pass's (codes_top, codes_bot, pixels): one step of a merged pass."""
    return (*_public([c[lo:lo + n] for c in _levels_of(ct, cb)]), None if px is None else px[lo:lo + n])


def _same(a, b) -> bool:
    """Equality of sampler settings that may hold tensors (given codes): tensors compare by value, never through ``==``."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and bool(torch.equal(a.cpu(), b.cpu()))
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


class _Step(NamedTuple):
    """One queued step of a merging sampler: ``submit``'s arguments and the Pending handed out for it."""
    pending: 'Pending'
    num_candidates: int
    cond: Any
    seed: Optional[int]
    max_seq_len: int
    use_fp16: bool
    precision: Optional[str]
    clamp01: bool
    use_graph: bool
    after: Optional[Callable]
    order_after_current: bool
    sample_kw: dict

    def wants_logprobs(self) -> bool:
        return bool(self.sample_kw.get('return_logprobs'))

    def wants_report(self) -> bool:
        """``return_report=N`` is a step setting like the sampler's: it is NOT among the free ones of ``settings``, so steps merge only when their N is equal."""
        return self.sample_kw.get('return_report') is not None

    def prefix_len(self) -> int:
        """P of the step's ``prefix_codes`` (0: none)."""
        prefix = self.sample_kw.get('prefix_codes')
        return 0 if prefix is None else int(torch.as_tensor(prefix[0]).shape[-1])

    def settings(self, mixed_samplers: bool = False, mixed_prefixes: bool = False) -> tuple:
        """What the steps of one merged pass must share (``mixed_samplers``: all but the sampler settings, which then travel per row).
        Prefix codes belong to a step's rows like its class ids; their LENGTH is shared (a pass has one prefill) unless ``mixed_prefixes``:
        every step's prefix is then its rows of the pass's keep table."""
        free = ('sample_offset', 'prefix_codes', 'return_logprobs') + GUIDANCE_KEYS + (SAMPLER_KEYS if mixed_samplers else ())
        return (self.max_seq_len, self.use_fp16, self.precision, self.clamp01, self.use_graph, 0 if mixed_prefixes else self.prefix_len(),
                {k: v for k, v in self.sample_kw.items() if k not in free})


def check_mergeable(step: _Step, first: _Step, mixed_samplers: bool = False, mixed_prefixes: bool = False) -> None:
    """ValueError unless ``step`` can join the pass that ``first`` opened."""
    if not mixed_prefixes and step.prefix_len() != first.prefix_len():
        raise ValueError(f'steps merged into one pass must share the prefix length: this step has P={step.prefix_len()}, the pass P={first.prefix_len()} '
                         '(a merged pass has one prefill; flush() first to start a new pass)')
    if not _same(step.settings(mixed_samplers, mixed_prefixes), first.settings(mixed_samplers, mixed_prefixes)):
        if mixed_samplers:
            raise ValueError('steps of a mixed pass may differ in temperature, top-k and top-p only: max_seq_len, precision and every other '
                             'setting must match (flush() first to start a new pass)')
        raise ValueError('steps merged into one pass must share max_seq_len, precision and sampler settings (flush() first to start a new pass)')


class Pending:
    """Result of a step queued on a merging sampler: filled when its group is launched (``InflightSampler.flush`` / ``drain``)."""
    __slots__ = ('value',)

    def __init__(self):
        self.value = None

    def get(self):
        if self.value is None:
            raise RuntimeError('the step has not been launched yet: call flush() or drain() first')
        return self.value


class InflightSampler:
    def __init__(self, model, lanes: int = 3, device: Optional[torch.device] = None, merge: int = 1, record_phases: bool = False,
                 ar_high_priority: bool = False, mixed_samplers: bool = False, mixed_prefixes: bool = False, share_prompts: bool = False):
        if lanes < 1 or merge < 1:
            raise ValueError('lanes and merge must be >= 1')
        if share_prompts and mixed_prefixes:
            raise ValueError('share_prompts together with mixed_prefixes is not built: every pass of a mixed_prefixes sampler stages a keep table, and the prompt '
                             'and a code prefix are one prefill whose prefix rows differ per row')
        # text models: every pass prefills each DISTINCT prompt of its rows once -- over all its steps, negative rows included -- and hands it to the rows
        # that carry it (sampling_ihqgpt's share_prompts).  A pass-wide setting: it travels with every step's sampler keywords, which steps must share
        self.share_prompts = bool(share_prompts)
        self.model = model
        self.merge = int(merge)
        # merged steps may differ in top_k* / top_p* / softmax_temperature: every pass stages a row table on its lane (always, also when its steps
        # happen to agree: the launch sequence, hence the captured graph, then never depends on what was queued)
        self.mixed_samplers = bool(mixed_samplers)
        # merged steps may differ in the length of their prefix (none included): every pass stages a keep table on its lane (hqt_set_keep_mask; always,
        # as with the row table) whose rows keep their own step's prefix; the shortest prefix is the pass's one prefill, the rest are decode steps
        self.mixed_prefixes = bool(mixed_prefixes)
        self.record_phases = bool(record_phases)     # merged passes: (AR start, AR end, decode end) events per pass, appended to phase_log
        self.phase_log: list = []
        self._queue: list = []
        self.n = int(lanes)
        self.device = device if device is not None else model.stage2._device
        self.streams: List[torch.cuda.Stream] = [torch.cuda.Stream(device=self.device) for _ in range(self.n)]
        # ar_high_priority: a lane's AR loop runs on a stream of the highest priority, its decode on the lane's own stream behind an event.
        # The AR kernels of a pass are thousands of short dependent launches; on equal terms each of them queues behind the other lane's
        # convolution workgroups for compute units (tools/diag_overlap.py: 4 % overlap).  Priority decides who gets a freed slot first.
        self.ar_streams: List[torch.cuda.Stream] = []
        if ar_high_priority:
            hi = -1
            if hasattr(torch.cuda.Stream, 'priority_range'):
                hi = torch.cuda.Stream.priority_range()[1]
            self.ar_streams = [torch.cuda.Stream(device=self.device, priority=hi) for _ in range(self.n)]
        self.k = 0

    def submit(self, num_candidates: int, cond, *, seed: Optional[int] = None, max_seq_len: int = 64, use_fp16: bool = True,
               decode: bool = True, precision: Optional[str] = None, clamp01: bool = True, use_graph: bool = True,
               after=None, phase_events=None, order_after_current: bool = True, **sample_kw) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.cuda.Event]:
        """Queue one batch on the next lane; returns (codes_top, codes_bot, pixels or None, done_event) immediately.
        The tensors are valid once ``done_event`` has completed (or after ``drain()``).  ``phase_events``: three timing
        events recorded on the lane's stream at AR start / AR end / decode end (lane time: phases of different lanes overlap).
        ``return_logprobs=True`` (with the sampler keywords): the step's log-probabilities fp32 [num_candidates, max_seq_len, draws] as one more element,
        behind ``done_event``.  Steps of a merged pass need not agree on it: the pass computes the buffer if any of its steps asks, and only
        those steps get their rows.  ``guidance_scale`` / ``neg_cond`` (with the sampler keywords, as in ``sampling_ihqgpt``): a guided step; it
        merges with guided and unguided steps alike -- the pass carries one negative row per row of a guided step behind the rows of all steps
        (``step_guidance``), which are neither decoded nor returned.  ``return_report=N`` (with the sampler keywords, as in ``sampling_ihqgpt``): the step's
        ``DrawReport`` as the last element, behind the log-probabilities; steps merge into one pass only when their N is equal (None included)."""
        _report_n(self.model.stage2.spec, sample_kw.get('return_report'))      # refused here, before the step is queued or an engine is built
        if self.share_prompts:
            sample_kw.setdefault('share_prompts', True)
        if self.merge > 1:
            if decode is False or phase_events is not None or sample_kw.get('noise') is not None:
                raise ValueError('merged steps support the plain sample + decode step only (no explicit noise, no phase events)')
            p = Pending()
            step = _Step(p, num_candidates, cond, seed, max_seq_len, use_fp16, precision, clamp01, use_graph, after, order_after_current, sample_kw)
            # checked HERE, before the step is queued: a mismatch raises without touching the queue (every Pending already handed out stays valid)
            check_guided_step(self.model.stage2, num_candidates, sample_kw)
            if self._queue:
                check_mergeable(step, self._queue[0], self.mixed_samplers, self.mixed_prefixes)
            self._queue.append(step)
            if len(self._queue) >= self.merge:
                self.flush()
            return p
        return self._launch(num_candidates, cond, seed=seed, max_seq_len=max_seq_len, use_fp16=use_fp16, decode=decode, precision=precision,
                            clamp01=clamp01, use_graph=use_graph, after=after, phase_events=phase_events, order_after_current=order_after_current,
                            **sample_kw)

    def flush(self) -> None:
        """Launch the queued steps (merge > 1) as one pass; their Pending objects receive (codes_top, codes_bot, pixels, done_event)."""
        q, self._queue = self._queue, []
        if not q:
            return
        ref = q[0]
        sizes = [e.num_candidates for e in q]
        los = [sum(sizes[:i]) for i in range(len(q))]
        kw = {k: v for k, v in ref.sample_kw.items() if k not in ('sample_offset', 'prefix_codes', 'return_logprobs') + GUIDANCE_KEYS}
        pairs, mirrors = step_guidance(self.model.stage2.spec.levels, sizes, [e.sample_kw for e in q])
        want_lp = any(e.wants_logprobs() for e in q)
        if want_lp:
            kw['return_logprobs'] = True
        if self.mixed_prefixes:                      # every step's own prefix as its rows of the keep table (the negative rows repeat their positive ones)
            mask, kept = step_keep_table(self.model.stage2.spec.levels, sizes, ref.max_seq_len, [e.sample_kw for e in q])
            kw['keep_mask'] = torch.cat([mask, mask[mirrors]]) if mirrors else mask
            kw['kept_codes'] = [torch.cat([c, c[mirrors]]) for c in kept] if mirrors else kept
        elif ref.prefix_len():                       # every step's own prefix rows, in step order (one P: check_mergeable)
            where = torch.as_tensor(ref.sample_kw['prefix_codes'][0]).device       # device prefixes stay there: no copy back to the host
            kw['prefix_codes'] = [torch.cat([torch.as_tensor(e.sample_kw['prefix_codes'][l]).to(where, torch.int64) for e in q])
                                  for l in range(len(ref.sample_kw['prefix_codes']))]
            if mirrors:
                kw['prefix_codes'] = [torch.cat([p, p[mirrors]]) for p in kw['prefix_codes']]
        if self.mixed_samplers:                      # every row keeps the sampler settings of its own step
            kw = {k: v for k, v in kw.items() if k not in SAMPLER_KEYS}
            kw['row_samplers'] = step_row_samplers(self.model.stage2.spec.levels, sizes, [e.sample_kw for e in q])
            kw['row_samplers'] += [kw['row_samplers'][r] for r in mirrors]
        offs = [int(e.sample_kw.get('sample_offset', 0)) for e in q]
        cond = None
        if self.model.stage2.use_txt_cond:           # [n, ctx_len_txt] token ids per step
            cond = torch.cat([torch.as_tensor(e.cond).reshape(e.num_candidates, -1).to('cpu', torch.int64) for e in q])
        elif self.model.stage2.use_cls_cond:
            parts = []
            for e in q:
                c = torch.as_tensor(e.cond).reshape(-1).to('cpu', torch.int64)
                parts.append(c.expand(e.num_candidates) if c.numel() == 1 else c)
            cond = torch.cat(parts)
        if pairs:                                    # the negative rows, behind the rows of all steps: every guided step's negative condition for its rows
            kw['guidance'] = pairs
            negs = [negative_cond(self.model.stage2, n, e.sample_kw.get('neg_cond'))
                    for e, n in zip(q, sizes) if e.sample_kw.get('guidance_scale') is not None]
            cond = torch.cat([cond] + [n.to('cpu', torch.int64) for n in negs])
        seeds = [int(e.seed) if e.seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item()) for e in q]
        row_seeds = [s for s, n in zip(seeds, sizes) for _ in range(n)]
        row_offsets = [o + i for o, n in zip(offs, sizes) for i in range(n)]
        row_seeds += [row_seeds[r] for r in mirrors]     # a negative row draws with its positive row's key
        row_offsets += [row_offsets[r] for r in mirrors]

        def split_after(ct, cb, px):
            for e, lo in zip(q, los):
                if e.after is not None:
                    e.after(*_rows(ct, cb, px, lo, e.num_candidates))
        phases = None
        if self.record_phases:
            phases = tuple(torch.cuda.Event(enable_timing=True) for _ in range(3))
            self.phase_log.append((phases, sum(sizes)))
        ct, cb, px, ev, *more = self._launch(sum(sizes) + len(mirrors), cond, keep_rows=sum(sizes), seed=seeds[0], max_seq_len=ref.max_seq_len, use_fp16=ref.use_fp16, decode=True,
                                      precision=ref.precision, clamp01=ref.clamp01, use_graph=ref.use_graph,
                                      after=split_after if any(e.after is not None for e in q) else None, phase_events=phases,
                                      order_after_current=any(e.order_after_current for e in q), row_seeds=row_seeds, row_offsets=row_offsets, **kw)
        lp = more.pop(0) if want_lp else None
        report = more.pop(0) if ref.wants_report() else None
        for e, lo in zip(q, los):
            e.pending.value = ((*_rows(ct, cb, px, lo, e.num_candidates), ev) + ((lp[lo:lo + e.num_candidates],) if e.wants_logprobs() else ())
                               + ((DrawReport(*(None if f is None else f[lo:lo + e.num_candidates] for f in report)),) if report is not None else ()))

    def _launch(self, num_candidates: int, cond, *, seed: Optional[int] = None, max_seq_len: int = 64, use_fp16: bool = True,
                decode: bool = True, precision: Optional[str] = None, clamp01: bool = True, use_graph: bool = True,
                after=None, phase_events=None, order_after_current: bool = True, keep_rows: Optional[int] = None, **sample_kw):
        lane = self.k % self.n
        self.k += 1
        # `ar_precision` ('exact' | 'fast' | 'split', optional, travels with the sampler settings): arithmetic of the AR loop, overriding
        # use_fp16 (sampling_ihqgpt's `precision`; the `precision` of this method is the DECODE arithmetic)
        ar_precision = sample_kw.pop('ar_precision', None)
        want_lp = bool(sample_kw.pop('return_logprobs', False))
        want_report = sample_kw.get('return_report') is not None
        st = self.streams[lane]
        caller = torch.cuda.current_stream(self.device)
        # order the lane after whatever the caller's stream has queued (inputs; earlier direct use of lane 0's engine):
        # a lane's workspace must never be touched from two streams at once
        if order_after_current:                      # False: the caller has nothing queued that this batch depends on (keeps the null stream's queue idle)
            st.wait_stream(torch.cuda.current_stream(self.device))
        if self.n > 1:
            # several batches in flight: kernels that cost the fewest CU-microseconds (hqt_set_policy).  The policy lives on the
            # engine object, so a lane rebuilt for a larger batch (or after the model dropped its engines) gets it again.
            rows = num_candidates * (2 if sample_kw.get('guidance_scale') is not None else 1)      # a guided call doubles its rows itself
            eng = self.model.stage2.engine(rows, max_seq_len, lane)
            if eng.policy != POLICY_THROUGHPUT:
                eng.set_policy(POLICY_THROUGHPUT)
        ast = self.ar_streams[lane] if self.ar_streams else st
        if ast is not st:
            ast.wait_stream(st)                      # the lane stays one in-order sequence: AR of this pass behind the lane's previous decode
        with torch.cuda.stream(ast):
            if phase_events is not None:
                phase_events[0].record(ast)
            codes = sample_codes(self.model.stage2, num_candidates, cond, seed=seed, max_seq_len=max_seq_len, use_fp16=use_fp16,
                                 use_graph=use_graph, lane=lane, precision=ar_precision, return_logprobs=want_lp, **sample_kw)
            if keep_rows is not None and keep_rows < num_candidates:      # a merged pass's negative rows end here: not decoded, not returned
                codes = [_first_rows(c, keep_rows) for c in codes]
            report = codes.pop() if want_report else None      # (behind the log-probabilities)
            logprobs = codes.pop() if want_lp else None
            if phase_events is not None:
                phase_events[1].record(ast)
        if ast is not st:
            st.wait_stream(ast)
            for t in (*codes, logprobs, *(report or ())):
                if t is not None:
                    t.record_stream(st)
        ct, cb = _public(codes)                      # the 4-tuple shape of the result, whatever the level count
        with torch.cuda.stream(st):
            px = None
            if decode:
                px = self.model.stage1.decode_sequences(codes, precision=precision or ('fast' if use_fp16 else 'exact'), clamp01=clamp01, lane=lane)
            if phase_events is not None:
                phase_events[2].record(st)
            if after is not None:
                after(ct, cb, px)                    # e.g. a gather of the finished pixels, queued on the lane's stream
            ev = torch.cuda.Event()
            ev.record(st)
        # the results were allocated on the lane's stream and will be read (and eventually freed) on the caller's: tell the
        # caching allocator, or it may hand the memory to the lane again while the caller's stream still reads it
        for t in (*codes, px, logprobs, *(report or ())):
            if t is not None:
                t.record_stream(caller)
        return (ct, cb, px, ev) + ((logprobs,) if want_lp else ()) + ((report,) if want_report else ())

    def release(self, batch: int, max_seq_len: int) -> None:
        """Back to the latency-oriented kernels on lane 0 (the engine direct ``sampling_ihqgpt`` calls use)."""
        self.drain()
        if self.n > 1:
            self.model.stage2.engine(batch, max_seq_len, 0).set_policy(POLICY_LATENCY)

    def drain(self) -> None:
        """Launch what is still queued (merge > 1), wait for every lane; also orders the caller's stream after the lanes."""
        self.flush()
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            cur.wait_stream(st)
            st.synchronize()
        self.model.stage1.range_check()          # SPLIT decodes: an activation outside the fp16 range invalidates the pass (raises)
        self.model.stage2.range_check()          # ... and SPLIT AR passes (ar_precision='split')
