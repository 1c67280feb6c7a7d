"""Thin torch-tensor wrapper over one libhqt handle.

PyTorch is plumbing here (device memory, streams); all arithmetic happens inside libhqt.so.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import PRECISION_EXACT, PRECISION_FAST, hqt_config, hqt_draw_report, hqt_encode_out, hqt_guide_pair, hqt_row_sampler, hqt_sample_opts, hqt_sample_opts_l3
from .spec import DEPTH_DECODINGS, STAGE1_RESAMPLES, Stage1Spec, Stage2Spec


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def make_config(s2: Optional[Stage2Spec], s1: Optional[Stage1Spec], max_batch: int, max_steps: int, ar_layouts: int = 0) -> hqt_config:
    c = hqt_config()
    c.abi_version = _lib.ABI_VERSION
    c.max_batch = int(max_batch)
    c.max_steps = int(max_steps)
    c.ar_layouts = int(ar_layouts)
    if s2 is not None:
        c.has_stage2 = 1
        c.embed_dim, c.n_layers, c.n_heads, c.n_layers_depth = s2.embed_dim, s2.n_layers, s2.n_heads, s2.n_layers_depth
        c.vocab_top, c.vocab_bot, c.vocab_txt = s2.vocab_top, s2.vocab_bot, s2.vocab_txt
        c.ctx_len_img, c.ctx_len_txt, c.n_classes = s2.ctx_len_img, s2.ctx_len_txt, s2.n_classes
        c.cond_type, c.embedding_type, c.gelu_approx = s2.cond, s2.embedding, int(s2.gelu_approx)
        c.depth_decoding = DEPTH_DECODINGS.index(s2.depth_decoding)
    if (s2 is not None and s2.levels == 3) or (s1 is not None and s1.code_levels == 3):
        c.code_levels = 3
    if s1 is not None:
        c.has_stage1 = 1
        c.s1_ch, c.s1_n_mult = s1.ch, len(s1.ch_mult)
        for i, m in enumerate(s1.ch_mult):
            c.s1_ch_mult[i] = m
        c.s1_num_res_blocks = s1.num_res_blocks
        c.s1_n_attn_res = len(s1.attn_resolutions)
        for i, r in enumerate(s1.attn_resolutions):
            c.s1_attn_res[i] = r
        c.s1_resolution, c.s1_z_channels, c.s1_embed_dim = s1.resolution, s1.z_channels, s1.embed_dim
        c.s1_n_embed, c.s1_out_ch = s1.n_embed, s1.out_ch
        c.s1_use_init_downsample, c.s1_use_mid_block, c.s1_use_attn = (int(s1.use_init_downsample), int(s1.use_mid_block),
                                                                        int(s1.use_attn))
        c.s1_resample = STAGE1_RESAMPLES.index(s1.resample)
    return c


# (data_ptr, numel) -> tensor version of device tensors whose indices are known to be in range: produced by a sampler of this
# process (any engine: the stage-2 engine's codes go to the stage-1 engine's decode) or already validated once
_TRUSTED: Dict[tuple, tuple] = {}       # (data_ptr, shape, stride, dtype) -> (tensor version, weakref to its storage, largest valid id + 1)

def row_sampler_table(levels: int, row_samplers) -> np.ndarray:
    """Per-row sampler settings -> the ``hqt_row_sampler`` array ``hqt_set_row_samplers`` takes, as uint32 [B, 9] (three fp32 temperatures, three
    int32 top-k, three fp32 top-p; index = code level, levels the model lacks stay at temperature 1 / no cut-off).  Each entry is
    ``(temperature per level, top_k per level, top_p per level)``; ``None`` for a cut-off, or for all cut-offs of a kind, means none."""
    L = int(levels)
    rows = np.zeros((len(row_samplers), 9), dtype=np.uint32)
    done: Dict[tuple, np.ndarray] = {}           # by value: a merged step repeats one entry for all of its rows
    for b, entry in enumerate(row_samplers):
        if len(entry) != 3:
            raise ValueError(f'row_samplers[{b}]: expected (temperature, top_k, top_p), each per level')
        t, k, p = (tuple(v) if v is not None else (None,) * L for v in entry)
        if not (len(t) == len(k) == len(p) == L):
            raise ValueError(f'row_samplers[{b}]: expected {L} levels in each of temperature, top_k and top_p')
        row = done.get((t, k, p))
        if row is None:
            tf = np.ones(3, dtype=np.float32)
            tf[:L] = [1.0 if v is None else float(v) for v in t]
            ki = np.zeros(3, dtype=np.int32)
            ki[:L] = [int(v) if v else 0 for v in k]
            pf = np.zeros(3, dtype=np.float32)
            pf[:L] = [float(v) if v else 0.0 for v in p]
            row = done[(t, k, p)] = np.concatenate([tf.view(np.uint32), ki.view(np.uint32), pf.view(np.uint32)])
        rows[b] = row
    return rows


def guide_pair_table(levels: int, guidance):
    """Guidance pairs -> the ``hqt_guide_pair`` array ``hqt_set_guidance`` takes (20 bytes per pair).  Each entry is ``(pos_row, neg_row, scale)``:
    two different rows of the pass, and one scale for every code level or one per level, coarse to fine (levels the model lacks stay at 1.0 =
    no guidance).  Which rows exist, and that no row is named twice, is checked by the library against the call that takes the table."""
    L = int(levels)
    table = (hqt_guide_pair * len(guidance))()
    for i, entry in enumerate(guidance):
        if len(entry) != 3:
            raise ValueError(f'guidance[{i}]: expected (pos_row, neg_row, scale)')
        pos, neg, scale = entry
        scale = [float(scale)] * L if isinstance(scale, (int, float)) else [float(v) for v in scale]
        if len(scale) != L:
            raise ValueError(f'guidance[{i}]: expected one scale or {L} (one per code level), got {len(scale)}')
        table[i].pos_row, table[i].neg_row = int(pos), int(neg)
        for l in range(3):
            table[i].scale[l] = scale[l] if l < L else 1.0
    return table


def check_guided_rows(batch: int, n_pairs: int, max_batch: int) -> None:
    """ValueError, naming the doubling, when the rows of a guided call do not fit the engine: every image is two rows of the pass."""
    if int(batch) > int(max_batch):
        raise ValueError(f'guided sampling runs every image as two rows of one pass (positive and negative condition): batch={int(batch)} rows for '
                         f'{int(n_pairs)} pairs exceed max_batch={int(max_batch)} of this engine -- build it for twice the images')


def check_prompt_groups(s2: Stage2Spec, batch: int, cond, prompt_groups, max_batch: int, prefix=None, keep=None):
    """A prompt-group table (``hqt_set_prompt_groups``) checked on the host, before any engine is built or touched: ``prompt_groups`` holds one integer per row
    of the pass, row b carrying prompt ``cond[prompt_groups[b]]`` of ``cond`` [G, ctx_len_txt], 1 <= G <= batch.  Returns (table as a contiguous int32 numpy
    array, G); None stays None."""
    if prompt_groups is None:
        return None
    if s2.cond != 2:
        raise ValueError('prompt_groups: the model is not text-conditional (one embedding row per sample leaves no prefill to share)')
    if prefix is not None or keep is not None:
        raise ValueError('prompt_groups together with prefix or keep is not built: the prompt and a code prefix are one prefill whose prefix rows differ per row')
    B = int(batch)
    if B < 1 or B > int(max_batch):
        raise ValueError(f'prompt_groups: B={B} outside [1, max_batch={int(max_batch)}]')
    g = torch.as_tensor(prompt_groups).cpu()
    if g.dtype.is_floating_point or g.dtype == torch.bool:
        raise ValueError(f'prompt_groups: expected integers, got {g.dtype}')
    if tuple(g.shape) != (B,):
        raise ValueError(f'prompt_groups: expected shape ({B},) -- one entry per row of the pass --, got {tuple(g.shape)}')
    cshape = tuple(torch.as_tensor(cond).shape) if cond is not None else None
    if cshape is None or len(cshape) != 2 or cshape[1] != s2.ctx_len_txt or cshape[0] < 1:
        raise ValueError(f'cond (text token ids) with prompt_groups: expected shape (G, {s2.ctx_len_txt}), one row per distinct prompt, got {cshape}')
    G = int(cshape[0])
    if G > B:
        raise ValueError(f'prompt_groups: n_groups={G} exceeds B={B}')
    lo, hi = int(g.min()), int(g.max())
    if lo < 0 or hi >= G:
        raise ValueError(f'prompt_groups: index outside [0, n_groups={G}) (values span [{lo}, {hi}])')
    return np.ascontiguousarray(g.numpy().astype(np.int32)), G


# what the two- and the three-level surface call their levels in messages
_FORCE_NAMES = {2: ('force_top', 'force_bot'), 3: ('force[0]', 'force[1]', 'force[2]')}
_CODE_NAMES = {2: ('code_t', 'code_b'), 3: ('code grid',) * 3}


def check_prefix(s2: Stage2Spec, batch: int, n_steps: int, prefix, max_prefix: Optional[int] = None, text_prefix: bool = False) -> Optional[list]:
    """A code prefix checked on the host, before any engine is built or touched: ``prefix`` is the list of code levels, coarse to fine,
    int64 [B, P], [B, P, 4][, [B, P, 16]] with 1 <= P <= n_steps - 1 (and P <= ``max_prefix`` when given); every code inside the vocabulary
    (IndexError otherwise, as nn.Embedding raises in the reference).  Returns the levels as tensors; None stays None.
    ``text_prefix``: a text-conditional model takes the prefix (two code levels with the causal 'parallel' depth head: the prompt and the prefix
    share one prefill of ctx_len_txt + P rows per sample); a caller asks for it explicitly, because of the row workspace it costs."""
    if prefix is None:
        return None
    if s2.cond == 2:
        if not text_prefix:
            raise ValueError('a code prefix with text conditioning shares one prefill with the prompt (ctx_len_txt + P rows per sample) and is '
                             'run on request only: pass text_prefix=True')
        if s2.depth_decoding == 'bidirectional':
            raise ValueError("a code prefix with text conditioning is built for the two-level 'parallel' depth head; the 'bidirectional' head "
                             "with text conditioning is not built at all (the reference's own step does not pick the last text token)")
        if s2.levels == 3:
            raise ValueError("a code prefix with text conditioning is built for two code levels (the 'parallel' depth head); three code levels "
                             'with text conditioning are not')
    L = s2.levels
    if not isinstance(prefix, (list, tuple)) or len(prefix) != L:
        raise ValueError(f'prefix: expected the {L} code levels as one list, coarse to fine')
    levels = [torch.as_tensor(p) for p in prefix]
    if levels[0].dim() != 2 or int(levels[0].shape[0]) != int(batch):
        raise ValueError(f'prefix[0]: expected shape ({int(batch)}, P), got {tuple(levels[0].shape)}')
    P = int(levels[0].shape[1])
    if P < 1 or P >= int(n_steps):
        raise ValueError(f'prefix of P={P} positions: P must lie in [1, n_steps - 1 = {int(n_steps) - 1}] (at least one position is left to draw)')
    if max_prefix is not None and P > int(max_prefix):
        raise ValueError(f'prefix of P={P} positions exceeds max_prefix={int(max_prefix)} of this engine')
    for l, t in enumerate(levels):
        want = (int(batch), P) + ((4 ** l,) if l else ())
        if tuple(t.shape) != want:
            raise ValueError(f'prefix[{l}]: expected shape {want}, got {tuple(t.shape)}')
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f'prefix[{l}]: expected integer codes, got {t.dtype}')
        if not t.is_cuda:                            # device tensors are checked (once) by the engine: Engine._check_index
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= s2.vocab_top:
                raise IndexError(f'prefix[{l}]: index out of range (values span [{lo}, {hi}], table has {s2.vocab_top} rows)')
    return levels


def keep_leading_run(mask, max_prefix: int, text_l3: bool = False) -> int:
    """``L`` of a keep table (``hqt_set_keep_mask``): the smallest count of leading kept positions over the rows of ``mask`` [B, n], clipped to
    min(``max_prefix`` of the engine, n - 1), and 0 where the prefix prefill is not built (``text_l3``: text conditioning with three code levels).
    Positions < L go through the one-pass prefix prefill; the library applies the same rule to the table it is given."""
    m = np.asarray(torch.as_tensor(mask).cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f'keep mask: expected shape (B, n), got {m.shape}')
    if text_l3:
        return 0
    run = np.where(m.all(axis=1), m.shape[1], np.argmin(m, axis=1))      # per row: index of its first 0
    return int(max(0, min(int(run.min()), int(max_prefix), m.shape[1] - 1)))


def check_keep(s2: Stage2Spec, batch: int, n_steps: int, keep) -> Optional[tuple]:
    """A keep table checked on the host, before any engine is built or touched: ``keep = (mask, codes)``, mask bool [B, n] (1 = keep every level of that
    position), codes the code levels as one list, coarse to fine, int64 [B, n], [B, n, 4][, [B, n, 16]], read where the mask is set; host codes inside the
    vocabulary there (IndexError otherwise, as nn.Embedding raises in the reference; device tensors are checked once by the engine).  Returns
    (mask as a contiguous uint8 numpy array, the levels as tensors); None stays None."""
    if keep is None:
        return None
    if not isinstance(keep, (list, tuple)) or len(keep) != 2:
        raise ValueError('keep: expected (mask [B, n], codes: the code levels as one list)')
    mask, codes = keep
    m = torch.as_tensor(mask).cpu()
    if tuple(m.shape) != (int(batch), int(n_steps)):
        raise ValueError(f'keep mask: expected shape {(int(batch), int(n_steps))}, got {tuple(m.shape)}')
    if m.dtype.is_floating_point:
        raise ValueError(f'keep mask: expected bool (or 0 / 1 integers), got {m.dtype}')
    m = np.ascontiguousarray((m != 0).numpy().astype(np.uint8))
    L = s2.levels
    if not isinstance(codes, (list, tuple)) or len(codes) != L:
        raise ValueError(f'kept codes: expected the {L} code levels as one list, coarse to fine')
    levels = [torch.as_tensor(c) for c in codes]
    for l, t in enumerate(levels):
        want = (int(batch), int(n_steps)) + ((4 ** l,) if l else ())
        if tuple(t.shape) != want:
            raise ValueError(f'kept codes[{l}]: expected shape {want}, got {tuple(t.shape)}')
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f'kept codes[{l}]: expected integer codes, got {t.dtype}')
        if not t.is_cuda and m.any():
            sel = t[torch.from_numpy(m.astype(bool))]
            lo, hi = int(sel.min()), int(sel.max())
            if lo < 0 or hi >= s2.vocab_top:
                raise IndexError(f'kept codes[{l}]: index out of range (values span [{lo}, {hi}], table has {s2.vocab_top} rows)')
    return m, levels


def check_segment(n_steps: int, segment, prefix=None, keep=None, prompt_groups=None) -> Optional[Tuple[int, int]]:
    """A segment (``hqt_set_segment``) checked on the host, before any engine is built or touched: ``segment = (start, stop)`` with
    0 <= start < stop <= n_steps, integers; not together with ``prefix`` or ``keep``, and with ``prompt_groups`` only where start == 0 (the prompt prefill
    belongs to the first segment).  Returns (start, stop) as ints; None stays None."""
    if segment is None:
        return None
    if not isinstance(segment, (list, tuple)) or len(segment) != 2:
        raise ValueError('segment: expected (start, stop)')
    for v in segment:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'segment: expected two integers, got {segment!r}')
    start, stop = int(segment[0]), int(segment[1])
    if start < 0 or stop <= start or stop > int(n_steps):
        raise ValueError(f'segment=({start}, {stop}): a segment needs 0 <= start < stop <= n_steps = {int(n_steps)}')
    if prefix is not None:
        raise ValueError('segment together with prefix is not built (segments of a pass with a code prefix)')
    if keep is not None:
        raise ValueError('segment together with keep is not built')
    if prompt_groups is not None and start > 0:
        raise ValueError(f'segment=({start}, {stop}) together with prompt_groups: the prompt prefill belongs to the segment that starts at 0')
    return start, stop


def check_row_positions(cond_type: int, batch: int, n_steps: int, row_positions, prefix=None, keep=None, prompt_groups=None, segment=None, max_joins: int = 0,
                        rolling_keep: bool = False):
    """A rolling call (``hqt_set_row_positions``) checked on the host, before any engine is touched: ``row_positions = (pos, k)`` with ``pos`` one integer per row of
    the batch in [-1, n_steps - 1] (-1: an empty slot) and 1 <= k <= n_steps; on a text-conditional model only with ``max_joins`` > 0 (the engine has sized the
    prompt prefill of its joining rows, ``hqt_set_max_joins``) and then with at most that many rows at position 0; not together with ``prefix``,
    ``prompt_groups`` or ``segment``, and with ``keep`` only where ``rolling_keep`` says that the engine has opted in (``hqt_set_join_run``).  Returns (pos as a
    contiguous int32 numpy array, k); None stays None."""
    if row_positions is None:
        return None
    if not isinstance(row_positions, (list, tuple)) or len(row_positions) != 2:
        raise ValueError('row_positions: expected (pos, k)')
    text = int(cond_type) == 2
    if text and int(max_joins) < 1:
        raise ValueError('row_positions: a rolling pass on a text-conditional model is not built (a row that joins at position 0 needs a prompt prefill of its own)'
                         ' unless the engine has sized one: Engine(..., max_joins=J) / Engine.set_max_joins(J) with J > 0')
    for other, what in ((prefix, 'prefix'), (None if rolling_keep else keep, 'keep'), (prompt_groups, 'prompt_groups'), (segment, 'segment')):
        if other is not None:
            raise ValueError(f'row_positions together with {what} is not built')
    pos, k = row_positions
    p = torch.as_tensor(pos).cpu()
    if p.dtype.is_floating_point or p.dtype == torch.bool or p.dim() != 1 or p.numel() != int(batch):
        raise ValueError(f'row_positions: pos holds one integer per row of the batch ({int(batch)}), got {p.dtype} of shape {tuple(p.shape)}')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= int(n_steps):
        raise ValueError(f'row_positions: k={k!r} outside [1, n_steps = {int(n_steps)}]')
    p = np.ascontiguousarray(p.numpy().astype(np.int32))
    bad = np.nonzero((p < -1) | (p > int(n_steps) - 1))[0]
    if bad.size:
        raise ValueError(f'row_positions: pos[{int(bad[0])}]={int(p[bad[0]])} outside [-1, n_steps - 1 = {int(n_steps) - 1}] (-1: an empty slot)')
    joins = int((p == 0).sum())
    if text and joins > int(max_joins):
        raise ValueError(f'row_positions: {joins} rows join at position 0 in this call, the engine has sized the prompt prefill of max_joins={int(max_joins)}')
    return p, int(k)


class DrawReport(NamedTuple):
    """The report of a call's draws (``hqt_set_draw_report``), every tensor [B, n, draws] as the log-probabilities are, the two top arrays with a last axis of N:
    ``entropy`` fp32 (nats) and ``rank`` int32 (0-based) of the fed-forward code in the raw row of its draw, ``top_codes`` int32 / ``top_logprobs`` fp32 the N most
    likely codes by (logit descending, index ascending).  A field that was not asked for is None."""
    entropy: Optional[torch.Tensor]
    rank: Optional[torch.Tensor]
    top_codes: Optional[torch.Tensor]
    top_logprobs: Optional[torch.Tensor]


def check_report_n(return_report, what: str = 'return_report') -> Optional[int]:
    """``return_report=N`` checked on the host: None (no report) stays None; otherwise an integer in [0, 16] -- 0: entropy and rank only, 1..16: the top-N arrays too.
    A bool is refused: False would read as N = 0, which IS a report."""
    if return_report is None:
        return None
    if isinstance(return_report, bool) or not isinstance(return_report, (int, np.integer)):
        raise ValueError(f'{what}: expected None or an integer N in [0, {_lib.REPORT_MAX_TOP}] (0: entropy and rank only), got {return_report!r}')
    if not 0 <= int(return_report) <= _lib.REPORT_MAX_TOP:
        raise ValueError(f'{what}: N={int(return_report)} outside [0, {_lib.REPORT_MAX_TOP}]')
    return int(return_report)


def new_draw_report(batch: int, n_steps: int, draws: int, top_n: int, device) -> DrawReport:
    """Fresh buffers for a report with ``top_n`` alternatives, filled with what reads as "not written" (NaN; -1): the positions a prefix call does not compute, the
    entries of an idle slot of a rolling call."""
    shp = (int(batch), int(n_steps), int(draws))
    return DrawReport(torch.full(shp, float('nan'), dtype=torch.float32, device=device), torch.full(shp, -1, dtype=torch.int32, device=device),
                      torch.full(shp + (top_n,), -1, dtype=torch.int32, device=device) if top_n else None,
                      torch.full(shp + (top_n,), float('nan'), dtype=torch.float32, device=device) if top_n else None)


def check_report_out(report_out, batch: int, n_steps: int, draws: int, device=None, vocab: Optional[int] = None):
    """``report_out`` checked on the host, before any engine is touched: an object with the four fields of ``DrawReport``, each None or a contiguous tensor on
    ``device`` -- ``entropy`` fp32 and ``rank`` int32 of shape [batch, n_steps, draws], ``top_codes`` int32 and ``top_logprobs`` fp32 of shape [batch, n_steps, draws, N],
    both or neither, 1 <= N <= 16 (and N <= ``vocab`` where given).  Returns (the ``hqt_draw_report`` to stage, N), or None when there is nothing to write."""
    if report_out is None:
        return None
    fields = ('entropy', 'rank', 'top_codes', 'top_logprobs')
    if not all(hasattr(report_out, f) for f in fields):
        raise ValueError(f'report_out: expected an object with the fields {fields} (engine.DrawReport), got {type(report_out).__name__}')
    ent, rank, tc, tl = (getattr(report_out, f) for f in fields)
    if (tc is None) != (tl is None):
        raise ValueError('report_out: top_codes and top_logprobs come together')
    shp = (int(batch), int(n_steps), int(draws))
    top_n = 0
    if tc is not None:
        if not isinstance(tc, torch.Tensor) or tc.dim() != 4:
            raise ValueError(f'report_out.top_codes: expected a tensor of shape {shp + ("N",)}, got {tuple(getattr(tc, "shape", ()))}')
        top_n = int(tc.shape[3])
        if not 1 <= top_n <= _lib.REPORT_MAX_TOP:
            raise ValueError(f'report_out.top_codes: N={top_n} alternatives outside [1, {_lib.REPORT_MAX_TOP}]')
        if vocab is not None and top_n > int(vocab):
            raise ValueError(f'report_out.top_codes: N={top_n} alternatives, the vocabulary has {int(vocab)} codes')
    for t, what, want, dtype in ((ent, 'entropy', shp, torch.float32), (rank, 'rank', shp, torch.int32),
                                 (tc, 'top_codes', shp + (top_n,), torch.int32), (tl, 'top_logprobs', shp + (top_n,), torch.float32)):
        if t is None:
            continue
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != dtype or not t.is_contiguous()
                or (device is not None and t.device != torch.device(device))):
            raise ValueError(f'report_out.{what}: expected a contiguous {dtype} tensor of shape {want}' + (f' on {device}' if device is not None else '') +
                             f', got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "?")}')
    if ent is None and rank is None and not top_n:
        return None
    r = hqt_draw_report()
    r.entropy, r.rank, r.top_n, r.top_codes, r.top_logprobs = _ptr(ent), _ptr(rank), top_n, _ptr(tc), _ptr(tl)
    return r, top_n


def check_select_rows(rows_from, paused_batch: Optional[int], max_batch: int) -> np.ndarray:
    """A row mapping for ``Engine.select_rows`` (``hqt_select_rows``) checked on the host: integers, one dimension, 1 <= B_new <= ``max_batch`` entries, each in
    [0, ``paused_batch``) -- the rows of the paused pass; None: unknown to the caller, the library checks the entries.  Any mapping: the identity, a permutation, a
    subset, duplicates.  Returns it as a contiguous int32 numpy array."""
    r = torch.as_tensor(rows_from).cpu()
    if r.dim() != 1 or r.numel() < 1:
        raise ValueError(f'rows_from: expected a one-dimensional mapping of at least one row, got shape {tuple(r.shape)}')
    if r.dtype.is_floating_point or r.dtype == torch.bool:
        raise ValueError(f'rows_from: expected integers, got {r.dtype}')
    if r.numel() > int(max_batch):
        raise ValueError(f'rows_from: B_new={r.numel()} exceeds max_batch={int(max_batch)} of this engine')
    lo, hi = int(r.min()), int(r.max())
    if lo < 0 or (paused_batch is not None and hi >= int(paused_batch)):
        raise ValueError(f'rows_from: index outside [0, B={paused_batch}) of the paused pass (values span [{lo}, {hi}])')
    return np.ascontiguousarray(r.numpy().astype(np.int32))


def check_score_codes(s2: Stage2Spec, codes, what: str = 'one-pass scoring') -> int:
    """Codes for ``Engine.score`` checked on the host, before any engine is built or touched: the model's code levels as one list, coarse to fine, int64 [B, n],
    [B, n, 4][, [B, n, 16]]; host tensors inside the vocabulary (IndexError otherwise; device tensors are checked once by the engine).  ValueError for the heads
    the one pass is not built for.  Returns n."""
    if s2.depth_decoding == 'top2mid2bot':
        raise ValueError(f"{what}: the 'top2mid2bot' depth head runs 21 causal sub-steps per position and is scored stepwise only: use one_pass=False")
    if s2.cond == 2 and s2.levels == 3:
        raise ValueError(f'{what}: text conditioning with three code levels is not built (two code levels are): use one_pass=False')
    L = s2.levels
    if not isinstance(codes, (list, tuple)) or len(codes) != L:
        raise ValueError(f'codes: expected the {L} code levels as one list, coarse to fine')
    levels = [torch.as_tensor(c) for c in codes]
    if levels[0].dim() != 2 or int(levels[0].shape[1]) < 1:
        raise ValueError(f'codes[0]: expected shape (B, n), got {tuple(levels[0].shape)}')
    B, n = (int(v) for v in levels[0].shape)
    if n > s2.ctx_len_img:
        raise ValueError(f'codes of n={n} positions: the model has ctx_len_img={s2.ctx_len_img}')
    for l, t in enumerate(levels):
        want = (B, n) + ((4 ** l,) if l else ())
        if tuple(t.shape) != want:
            raise ValueError(f'codes[{l}]: expected shape {want}, got {tuple(t.shape)}')
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f'codes[{l}]: expected integer codes, got {t.dtype}')
        if not t.is_cuda:
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= s2.vocab_top:
                raise IndexError(f'codes[{l}]: index out of range (values span [{lo}, {hi}], table has {s2.vocab_top} rows)')
    return n


class Engine:
    """One libhqt handle on one GPU.  Not thread-safe; asynchronous on torch's current stream."""

    def __init__(self, s2: Optional[Stage2Spec], s1: Optional[Stage1Spec], device: torch.device, max_batch: int,
                 max_steps: Optional[int] = None, ar_layouts: int = 0, max_prefix: int = 0, score_chunk: int = 0, max_joins: int = 0,
                 join_run: Optional[Tuple[int, int]] = None):
        """``ar_layouts``: bit mask of ``_lib.LAYOUT_*`` -- which derived layouts of the AR loop's weights ``finalize`` builds
        (``hqt_config.ar_layouts``; 0 = all).  A FAST-only replica passes ``_lib.LAYOUT_FAST`` and holds 5.2 instead of 9.1 GB for the
        ImageNet-12L model; a call in a precision the engine was built without raises HqtError (HQT_ERR_STATE).
        ``max_prefix``: longest code prefix ``sample(..., prefix=...)`` may pass (``hqt_set_max_prefix``, called right after ``hqt_create``; 0 = none, and the workspace
        is exactly what it is without the feature).
        ``score_chunk``: (sample, position) pairs per depth chunk of ``score`` (``hqt_set_score_chunk``, called right after ``hqt_create``; 0 = ``max_batch`` pairs,
        and nothing is allocated for it).
        ``max_joins``: rows that may join a rolling pass of a text-conditional model in one call (``hqt_set_max_joins``, called right after ``hqt_create``; 0 = rolling
        passes on a text model stay refused, and nothing is allocated).
        ``join_run`` = (J, R): rolling calls may take ``keep`` (``hqt_set_join_run``, see ``set_join_run``); None = they stay refused."""
        self.lib = _lib.load()                      # raises HqtLibraryError when the HIP library is absent
        self.s2, self.s1 = s2, s1
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.HqtLibraryError(f'libhqt runs on an MI355X only; got device {self.device} (no CPU fallback)')
        self.max_batch = int(max_batch)
        self.max_steps = int(max_steps if max_steps is not None else (s2.ctx_len_img if s2 else 1))
        self.max_prefix = int(max_prefix)
        self.cfg = make_config(s2, s1, self.max_batch, self.max_steps, ar_layouts)
        h = C.c_void_p()
        _lib.check(self.lib.hqt_create(C.byref(self.cfg), self.device.index or 0, C.byref(h)))
        self.h = h
        self.finalized = False
        if self.max_prefix:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.hqt_set_max_prefix(self.h, self.max_prefix))
        self.score_chunk = int(score_chunk)
        if self.score_chunk:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.hqt_set_score_chunk(self.h, self.score_chunk))
        self.max_joins = 0
        if int(max_joins):
            self.set_max_joins(max_joins)
        self.join_run = None
        if join_run is not None:
            self.set_join_run(*join_run)
        self.policy = _lib.POLICY_LATENCY

    def set_max_joins(self, max_joins: int) -> None:
        """``hqt_set_max_joins``: sizes (grows, never shrinks) the staging of the prompt prefill that up to ``max_joins`` rows joining a rolling pass need in one call,
        on a text-conditional engine; 0 switches rolling passes off again and frees nothing.  Raises HqtError on any other engine, outside [0, max_batch], or while
        the engine holds a rolling pass."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.hqt_set_max_joins(self.h, int(max_joins)))
        self.max_joins = int(max_joins)

    def set_join_run(self, max_joins: int, max_run: int) -> None:
        """``hqt_set_join_run``: after it a rolling call (``row_positions=``) may take ``keep``; up to ``max_joins`` rows per call join through a join phase that
        prefills a shared leading kept run of up to ``max_run`` positions (``max_run`` <= ``max_prefix`` of the engine; 0 on a text model with three code levels).
        On a text-conditional engine it is also ``set_max_joins(max_joins)``.  Grows, never shrinks, the staging; ``max_joins`` = 0 switches the opt-in off again.
        Raises HqtError outside those ranges or while the engine holds a rolling pass."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.hqt_set_join_run(self.h, int(max_joins), int(max_run)))
        self.join_run = (int(max_joins), int(max_run)) if int(max_joins) > 0 else None
        if self.s2 is not None and self.s2.cond == 2:
            self.max_joins = int(max_joins)

    def clone(self) -> 'Engine':
        """A further lane over the same weights (``hqt_clone``): own KV cache / activations / graph cache, results
        bit-identical to this engine's.  Lanes on different streams keep several batches in flight on one GPU.  The lane takes this engine's root's
        ``set_persist`` / ``set_single_key`` / ``set_split_kslices`` values as they are now; a later ``set_*`` call changes only the engine it is called on."""
        if not self.finalized:
            raise _lib.HqtError(-1, 'clone() needs a finalized engine')
        e = Engine.__new__(Engine)
        e.lib, e.s2, e.s1, e.device = self.lib, self.s2, self.s1, self.device
        e.max_batch, e.max_steps, e.max_prefix, e.cfg = self.max_batch, self.max_steps, self.max_prefix, self.cfg
        e.score_chunk = self.score_chunk
        e.max_joins = getattr(self, '_parent', self).max_joins     # hqt_clone gives the lane a staging of its own for as many joins as the root has sized
        e.join_run = getattr(getattr(self, '_parent', self), 'join_run', None)      # ... and over as long a run
        h = C.c_void_p()
        _lib.check(self.lib.hqt_clone(self.h, C.byref(h)))
        e.h, e.finalized = h, True
        e.policy = _lib.POLICY_LATENCY               # hqt_clone resets a lane to the default policy
        e._parent = self                             # keeps the weights' owner alive
        self._clones = getattr(self, '_clones', [])
        self._clones.append(e)
        return e

    def set_policy(self, policy: int) -> None:
        """``hqt_set_policy``: 0 = latency-oriented kernel choice (one batch at a time), 1 = throughput-oriented (several
        lanes in flight).  Part of the graph key: the next sample() re-captures if it changed."""
        _lib.check(self.lib.hqt_set_policy(self.h, int(policy)))
        self.policy = int(policy)

    def set_persist(self, on: bool) -> None:
        """``hqt_set_switch(HQT_SWITCH_PERSIST)``: False = the launch chain instead of the persistent AR launch (FAST sampling of up to 64
        rows); True also re-arms a handle that fell back to the chain after a launch gave up.  Part of the graph key.  Per handle, as every
        ``hqt_set_switch`` value: this engine only, not the lanes cloned from it before (a lane copies its root's values in ``clone()``)."""
        _lib.check(self.lib.hqt_set_switch(self.h, _lib.SWITCH_PERSIST, int(bool(on))))

    def set_persist_fault(self, cu_plus_one: int) -> None:
        """Test hook ``hqt_set_switch(HQT_SWITCH_PERSIST_FAULT)``: compute unit ``cu_plus_one - 1`` withholds its first grid-barrier signal in
        every later persistent launch (0 = none), cached graphs included.  This engine only (per handle)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.hqt_set_switch(self.h, _lib.SWITCH_PERSIST_FAULT, int(cu_plus_one)))

    def set_split_kslices(self, on: bool) -> None:
        """``hqt_set_switch(HQT_SWITCH_SPLIT_KSLICES)``: False = the SPLIT AR GEMMs are never K-sliced (one fp32 summation order at every row count).
        Per handle: lanes that exist keep their value (the merged passes run on lanes: call it on each), a lane cloned afterwards copies its root's."""
        _lib.check(self.lib.hqt_set_switch(self.h, _lib.SWITCH_SPLIT_KSLICES, int(bool(on))))

    def set_single_key(self, on: bool) -> None:
        """``hqt_set_switch(HQT_SWITCH_SINGLE_KEY)``: False = depth sub-step 0 the long way round (A/B runs and tests; bit-identical results).  Per handle: this engine
        only, not the lanes cloned from it before."""
        _lib.check(self.lib.hqt_set_switch(self.h, _lib.SWITCH_SINGLE_KEY, int(bool(on))))

    def _note_split(self, precision: int, stream: int, ar_rows: int = 0) -> None:
        # calls whose validity the device reports after the fact: SPLIT (an activation outside the fp16 range) and FAST sampling of up to
        # 64 rows (the persistent AR chain: a launch that could not get the whole GPU gives up after 1 s instead of hanging)
        if int(precision) == _lib.PRECISION_SPLIT or (int(precision) == _lib.PRECISION_FAST and 0 < ar_rows <= 64):
            self._split_streams = getattr(self, '_split_streams', set()) | {int(stream or 0)}

    def range_check(self) -> None:
        """hqt_range_check for every stream SPLIT-precision calls (and FAST sampling calls of up to 64 rows) of this engine were enqueued on
        since the last check: waits for them and raises HqtError if an activation left the fp16 range (HQT_ERR_RANGE) or a persistent AR
        launch gave up on its grid barrier (HQT_ERR_STATE) -- the output of such a call is invalid.  No-op -- and no synchronisation --
        when no such call is pending."""
        streams, self._split_streams = getattr(self, '_split_streams', set()), set()
        err = None
        with torch.cuda.device(self.device):
            for st in sorted(streams):
                try:
                    _lib.check(self.lib.hqt_range_check(self.h, C.c_void_p(st)))
                except _lib.HqtError as e:       # keep draining the other streams: the flag is per handle and already cleared
                    err = e
        if err is not None:
            raise err

    def close(self) -> None:
        for c in getattr(self, '_clones', []):       # clones go first: the parent owns the weights
            c.close()
        self._clones = []
        if getattr(self, 'h', None) is not None and self.h.value:
            self.lib.hqt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def set_weight(self, name: str, t) -> None:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
        t = t.detach().to(dtype=torch.float32).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(self.lib.hqt_set_weight(self.h, name.encode(), C.c_void_p(t.data_ptr()), 0, shape, t.dim()))

    def load(self, stage2: Optional[Dict[str, object]] = None, stage1: Optional[Dict[str, object]] = None) -> None:
        for prefix, sd in (('stage2.', stage2), ('stage1.', stage1)):
            for k, v in (sd or {}).items():
                self.set_weight(prefix + k, v)

    def finalize(self) -> None:
        _lib.check(self.lib.hqt_finalize_weights(self.h))
        self.finalized = True

    # ------------------------------------------------------------------ input validation
    # The reference indexes nn.Embedding / F.embedding tables with these tensors and raises IndexError for an id outside the
    # table.  Host tensors are checked on the host (free).  Device tensors need one reduction + a host read, i.e. a stream
    # synchronisation: they are checked once per (storage, version) and remembered, and tensors this engine produced itself
    # (sampled codes fed to decode) are trusted -- so a pipelined run (bench.py: lanes, sampled codes straight into decode)
    # never synchronises.  The kernels clamp every such index into its table regardless (csrc/common.h: clamp_idx).
    @staticmethod
    def _ident(t: torch.Tensor) -> tuple:
        return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)

    def _trust(self, *tensors, bound: int) -> None:
        """Remember that every id in these device tensors lies in [0, bound): a later check against a table of n >= bound rows needs
        no reduction; against a SMALLER table the tensor is checked again."""
        for t in tensors:
            if t is not None:
                # (address, size) alone is not an identity: the caching allocator hands a freed block to the next tensor of that size.
                # The storage object is: torch keeps one Python wrapper per live storage, and a weak reference to it dies with the storage.
                _TRUSTED[self._ident(t)] = (t._version, weakref.ref(t.untyped_storage()), int(bound))
                if len(_TRUSTED) > 256:
                    _TRUSTED.pop(next(iter(_TRUSTED)))

    def _check_index(self, t: Optional[torch.Tensor], n: int, what: str) -> None:
        if t is None or t.numel() == 0:
            return
        seen = _TRUSTED.get(self._ident(t)) if t.is_cuda else None
        if seen is not None and seen[0] == t._version and seen[1]() is t.untyped_storage() and seen[2] <= n:
            return
        lo, hi = (int(v) for v in torch.stack([t.min(), t.max()]).tolist())
        if lo < 0 or hi >= n:
            raise IndexError(f'{what}: index out of range (values span [{lo}, {hi}], table has {n} rows)')
        if t.is_cuda:
            self._trust(t, bound=hi + 1)

    @staticmethod
    def _check_out(t: torch.Tensor, shape, dtype, dev, what: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise ValueError(f'{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, got '
                             f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "?")}')
        return t

    @staticmethod
    def _row_keys(o, B: int, row_seeds, row_offsets):
        """Fills ``o.row_seeds`` / ``o.row_offsets`` (host arrays of B entries) and returns them so that they outlive the call."""
        if row_seeds is None and row_offsets is None:
            return None
        if row_seeds is None or row_offsets is None or len(row_seeds) != B or len(row_offsets) != B:
            raise ValueError(f'row_seeds and row_offsets come together, {B} entries each')
        rs = (C.c_uint64 * B)(*[int(v) & (2 ** 64 - 1) for v in row_seeds])
        ro = (C.c_int64 * B)(*[int(v) for v in row_offsets])
        o.row_seeds, o.row_offsets = C.cast(rs, C.c_void_p), C.cast(ro, C.c_void_p)
        return rs, ro

    def _prep(self, t, shape, dtype, what: str, table: int = 0) -> Optional[torch.Tensor]:
        """A sampling input checked for its shape (and, ``table`` > 0, for ids inside a table of that many rows), on the device; None stays None."""
        if t is None:
            return None
        t = torch.as_tensor(t)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
        if table:
            self._check_index(t, table, what)
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _prep_cond(self, cond, B: int) -> Optional[torch.Tensor]:
        if self.s2.cond == 1:
            return self._prep(cond, (B,), torch.int64, 'cond (class ids)', self.s2.n_classes)
        if self.s2.cond == 2:
            return self._prep(cond, (B, self.s2.ctx_len_txt), torch.int64, 'cond (text token ids)', self.s2.vocab_txt)
        return None

    # ------------------------------------------------------------------ stage 2
    # Code levels are lists, coarse to fine; their number (2: hqt_sample, 3: hqt_sample_l3) is all that differs below.
    def _sample_levels(self, levels: int, batch: int, cond, n_steps: int, *, precision, top_k, top_p, temperature, noise, seed, sample_offset,
                       force: Sequence[Optional[torch.Tensor]], out: Optional[Sequence[torch.Tensor]], return_logits, use_graph,
                       row_seeds, row_offsets, row_samplers=None, prefix=None,
                       return_logprobs=False, guidance=None, keep=None,
                       prompt_groups=None, segment=None, logits_out=None,
                       logprobs_out=None, row_positions=None, report_out=None) -> Tuple[List[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
        """Returns (codes [B, n], [B, n, 4][, [B, n, 16]], logits [n, draws, B, V] or None, logprobs [B, n, draws] or None)."""
        dev = self.device
        B, V, L = int(batch), self.s2.vocab_top, int(levels)
        segment = check_segment(n_steps, segment, prefix, keep, prompt_groups)
        roll = check_row_positions(self.s2.cond, B, n_steps, row_positions, prefix, keep, prompt_groups, segment, max_joins=getattr(self, 'max_joins', 0),
                                   rolling_keep=getattr(self, 'join_run', None) is not None)
        if roll is not None and out is None:
            raise ValueError('row_positions: a rolling call writes the positions its rows draw into out (and reads the codes in front of them there) -- pass the tensors the pass lives in')
        if segment is not None and segment[0] > 0 and out is None:
            raise ValueError(f'segment={segment}: a continuation reads the codes of position {segment[0] - 1} from out -- pass the tensors the earlier segments wrote')
        groups = None if prompt_groups is None else check_prompt_groups(self.s2, B, cond, prompt_groups, self.max_batch, prefix, keep)
        # (a text engine was asked for the shared prompt + prefix prefill when it was built with max_prefix; without it P > max_prefix = 0 refuses)
        prefix = check_prefix(self.s2, B, n_steps, prefix, self.max_prefix, text_prefix=True)
        P = 0 if prefix is None else int(prefix[0].shape[1])
        keep = check_keep(self.s2, B, n_steps, keep)
        if keep is not None:
            if prefix is not None:
                raise ValueError('keep and prefix: a prefix is a leading run of the keep mask -- put it there')
            for f, what in zip(force, _FORCE_NAMES[L]):
                if f is not None:
                    raise ValueError(f'{what} together with keep is not built: put the forced codes into the kept codes')
            # the leading run every row shares runs as the prefix prefill; its rows of the logits / log-probabilities are not written, as with a prefix
            # (a rolling call prefills no run over all rows: which rows of the buffers it writes follows the positions, and the buffers are the caller's)
            P = 0 if roll is not None else keep_leading_run(keep[0], self.max_prefix, text_l3=self.s2.cond == 2 and L == 3)
        draws = (4 ** L - 1) // 3                   # one draw per code of a position: 1 + 4 (+ 16)
        report = check_report_out(report_out, B, n_steps, draws, dev, V)
        shapes = [(B, n_steps) + ((4 ** l,) if l else ()) for l in range(L)]
        o = hqt_sample_opts() if L == 2 else hqt_sample_opts_l3()
        o.precision, o.n_steps = int(precision), int(n_steps)
        for i in range(L):
            k, p, t = int(top_k[i]) if top_k[i] else 0, float(top_p[i]) if top_p[i] else 0.0, float(temperature[i])
            if L == 2:                              # hqt_sample_opts names its two levels: top_k_top, top_k_bot, ...
                for field, v in (('top_k', k), ('top_p', p), ('temperature', t)):
                    setattr(o, f'{field}_{("top", "bot")[i]}', v)
            else:
                o.top_k[i], o.top_p[i], o.temperature[i] = k, p, t
        o.seed, o.sample_offset, o.use_graph = int(seed) & (2 ** 64 - 1), int(sample_offset), int(bool(use_graph))
        rows = self._row_keys(o, B, row_seeds, row_offsets)
        table = None if row_samplers is None else row_sampler_table(L, row_samplers)     # its length is checked against B by the library
        pairs = guide_pair_table(L, guidance) if guidance is not None and len(guidance) else None      # its rows are checked against B by the library
        if pairs is not None:
            check_guided_rows(B, len(pairs), self.max_batch)
        cond = self._prep_cond(cond, B if groups is None else groups[1])     # (a group table: one row per distinct prompt)
        noise = self._prep(noise, (n_steps, draws, B, V), torch.float32, 'noise')
        force = [self._prep(f, shp, torch.int64, what, V) for f, shp, what in zip(force, shapes, _FORCE_NAMES[L])]
        if keep is not None:
            sel = torch.from_numpy(keep[0].astype(bool))

            def kept(t, shp, what):              # ids are checked where they are read: under the mask
                if t.is_cuda and sel.any():
                    try:                         # the whole tensor first: a tensor that passes is remembered, and a steady stream of calls never synchronises
                        self._check_index(t, V, what)
                    except IndexError:
                        self._check_index(t[sel.to(t.device)], V, what)
                return self._prep(t, shp, torch.int64, what)
            keep = (keep[0], [kept(t, shp, f'kept codes[{l}]') for l, (t, shp) in enumerate(zip(keep[1], shapes))])
        if prefix is not None:
            prefix = [self._prep(p, (B, P) + shp[2:], torch.int64, f'prefix[{l}]', V) for l, (p, shp) in enumerate(zip(prefix, shapes))]
        if out is None:
            outs = [torch.empty(shp, dtype=torch.int64, device=dev) for shp in shapes]
        else:
            outs = [self._check_out(t, shp, torch.int64, dev, f'out[{i}]') for i, (t, shp) in enumerate(zip(out, shapes))]
        # (with a prefix the rows of positions < P are not written: zeros)
        logits = (torch.zeros if P else torch.empty)((n_steps, draws, B, V), dtype=torch.float32, device=dev) if return_logits else None
        # (buffers a segmented pass fills piece by piece: every segment writes its own positions and no others)
        if logits_out is not None:
            logits, return_logits = self._check_out(logits_out, (n_steps, draws, B, V), torch.float32, dev, 'logits_out'), True
        if logprobs_out is not None:
            return_logprobs = True
        # (the positions a prefix call does not compute stay NaN: a zero would read as "certain", and a sum over a half-scored sequence must not look like a score)
        logprobs = None
        if logprobs_out is not None:
            logprobs = self._check_out(logprobs_out, (B, n_steps, draws), torch.float32, dev, 'logprobs_out')
        elif return_logprobs:
            logprobs = (torch.full((B, n_steps, draws), float('nan'), dtype=torch.float32, device=dev) if P
                        else torch.empty((B, n_steps, draws), dtype=torch.float32, device=dev))
        if prefix is not None:
            entry = self.lib.hqt_sample_prefix if L == 2 else self.lib.hqt_sample_prefix_l3

            def fn(h, b, cnd, opts, nz, *rest):
                return entry(h, b, cnd, opts, nz, P, *map(_ptr, prefix), *rest)
        else:
            fn = self.lib.hqt_sample if L == 2 else self.lib.hqt_sample_l3
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            if table is not None:                   # staged on the handle; the call below takes it (and clears it even when it fails)
                _lib.check(self.lib.hqt_set_row_samplers(self.h, len(table), table.ctypes.data_as(C.POINTER(hqt_row_sampler))))
            if logprobs is not None:                # staged like the table: taken and cleared by the call below
                _lib.check(self.lib.hqt_set_logprob_out(self.h, _ptr(logprobs)))
            if report is not None:                  # ... and so is the draw report (the caller's buffers, written where the log-probabilities are)
                _lib.check(self.lib.hqt_set_draw_report(self.h, C.byref(report[0])))
            if pairs is not None:                   # ... and so is the pair table (copied by the library)
                _lib.check(self.lib.hqt_set_guidance(self.h, len(pairs), pairs))
            if keep is not None:                    # ... and the keep table (the mask is copied; the codes are read by the call below)
                kp = (C.c_void_p * 3)(*[_ptr(t) for t in keep[1]])
                _lib.check(self.lib.hqt_set_keep_mask(self.h, B, int(n_steps), keep[0].ctypes.data_as(C.c_void_p), kp))
            if groups is not None:                  # ... and the group table (copied; this is also where the staging buffer of the shared prefill is sized)
                _lib.check(self.lib.hqt_set_prompt_groups(self.h, B, groups[1], groups[0].ctypes.data_as(C.c_void_p)))
            if segment is not None:                 # ... and the segment
                _lib.check(self.lib.hqt_set_segment(self.h, segment[0], segment[1]))
            if roll is not None:                    # ... and the positions of a rolling pass (copied)
                _lib.check(self.lib.hqt_set_row_positions(self.h, B, roll[0].ctypes.data_as(C.c_void_p), roll[1]))
            _lib.check(fn(self.h, B, _ptr(cond), C.byref(o), _ptr(noise), *map(_ptr, force), _ptr(logits), *map(_ptr, outs), C.c_void_p(stream)))
            self._note_split(precision, stream, ar_rows=B)        # every head runs persistently (run_position)
        # inputs must outlive the asynchronous launches
        self._keep = (cond, noise, force, rows, prefix, keep, report_out)     # (the row-sampler table was copied by hqt_set_row_samplers)
        self._trust(*outs, bound=max(self.s2.vocab_top, self.s2.vocab_bot))     # the sampler only writes ids inside the vocabulary
        return outs, logits, logprobs

    def sample(self, batch: int, cond: Optional[torch.Tensor], n_steps: int, *, precision: int = PRECISION_FAST,
               top_k: Sequence[Optional[int]] = (None, None), top_p: Sequence[Optional[float]] = (None, None),
               temperature: Sequence[float] = (1.0, 1.0), noise: Optional[torch.Tensor] = None, seed: int = 0,
               sample_offset: int = 0, force_top: Optional[torch.Tensor] = None, force_bot: Optional[torch.Tensor] = None,
               return_logits: bool = False, use_graph: bool = True,
               out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               row_seeds: Optional[Sequence[int]] = None, row_offsets: Optional[Sequence[int]] = None,
               row_samplers: Optional[Sequence[tuple]] = None, prefix: Optional[Sequence[torch.Tensor]] = None,
               return_logprobs: bool = False, guidance: Optional[Sequence[tuple]] = None, keep: Optional[tuple] = None,
               prompt_groups=None, segment: Optional[Tuple[int, int]] = None, logits_out: Optional[torch.Tensor] = None,
               logprobs_out: Optional[torch.Tensor] = None, row_positions: Optional[tuple] = None, report_out=None):
        """Two-level sampling: returns (codes_top [B, n], codes_bot [B, n, 4][, logits [n, 5, B, V]][, logprobs [B, n, 5]]).
        ``return_logprobs``: fp32 log-probability of every code the call feeds forward -- the drawn one, or the forced one where ``force_*`` is
        given -- under the raw logits of its draw (T = 1, no cut-off: ``hqt_set_logprob_out``), appended last; with a prefix the positions < P are NaN.
        ``prefix`` = [top [B, P], bot [B, P, 4]], 1 <= P <= min(n - 1, max_prefix of this engine): completion (``hqt_sample_prefix``) -- the
        returned codes hold the prefix at positions < P, and positions >= P are drawn as a free run would draw them had its first P positions
        produced these codes (same Philox keys, same slice of ``noise``, same sampler settings); the prefix runs through the body in ONE pass
        (text conditioning: together with the prompt, ctx_len_txt + P rows per sample).
        ``row_seeds`` / ``row_offsets`` (both or neither, ``batch`` entries): merged steps -- row b draws what the row with
        global index ``row_offsets[b]`` of a call seeded ``row_seeds[b]`` draws (``hqt_sample_opts.row_seeds``).
        ``row_samplers`` (``batch`` entries ``(temperature per level, top_k per level, top_p per level)``, see ``row_sampler_table``): row b
        draws with its own settings in place of ``top_k`` / ``top_p`` / ``temperature`` -- bit for bit what it draws in a call that has
        those settings for every row (``hqt_set_row_samplers``).
        ``guidance`` (entries ``(pos_row, neg_row, scale)``, scale a float or one per level: ``guide_pair_table``): guided sampling
        (``hqt_set_guidance``) -- the two rows of a pair are one image under two conditions (``cond[pos_row]`` / ``cond[neg_row]``); every code of both
        is drawn from ``l_pos + (scale - 1) (l_pos - l_neg)`` with the positive row's Philox key, so both rows return the same codes.  ``batch``
        counts all rows; ``noise``, ``force_*`` and ``prefix`` must agree in the two rows of a pair; returned logits hold the guided row in both,
        returned log-probabilities score the code under it.  Rows outside every pair draw what they draw without ``guidance``.
        ``keep`` = (mask bool [B, n], codes [top [B, n], bot [B, n, 4]]): any positions of the grid held fixed (``hqt_set_keep_mask``) -- where the mask is set
        every level of the position is the given code, returned and fed forward; every other position is drawn as a plain call draws it whose earlier
        positions had produced the same codes.  The leading run all rows share, up to ``max_prefix`` of this engine, runs as the prefix prefill (its logits
        rows are zeros, its log-probabilities NaN, as with ``prefix``); every other kept position costs a decode step.  Not together with ``force_*`` or
        ``prefix``; the two rows of a guided pair keep the same positions.
        ``prompt_groups`` (int tensor [B], text models): shared prompts (``hqt_set_prompt_groups``) -- ``cond`` is then [G, ctx_len_txt], one row per DISTINCT prompt,
        and row b of the pass carries ``cond[prompt_groups[b]]``; the prompt prefill runs over the G prompts once and its K/V are copied to the rows.  EXACT returns
        bit for bit what the call returns with ``cond`` expanded to [B, ctx_len_txt].  Not together with ``prefix`` or ``keep``.
        ``segment`` = (start, stop): the call runs positions [start, stop) of a pass of ``n_steps`` positions (``hqt_set_segment``) and leaves the pass paused behind
        stop - 1 (stop == n_steps finishes it).  Every tensor keeps its full-length shape; entries outside the segment are neither read nor written, except the
        codes of position start - 1.  start == 0 begins a pass; start > 0 continues the paused pass of this engine (same batch, n_steps and precision, paused at
        ``start``: HqtError otherwise) and needs ``out`` -- the tensors the earlier segments wrote, edited or gathered as the caller sees fit.  Samplers, row tables,
        guidance and keys may differ from segment to segment; all segments together return bit for bit what one call returns.  ``logits_out`` [n, 5, B, V] /
        ``logprobs_out`` [B, n, 5]: caller-owned buffers the call writes (and returns) in place of fresh ones, so that a segmented pass fills one tensor.  Not
        together with ``prefix`` or ``keep``; ``prompt_groups`` with start == 0 only.
        ``row_positions`` = (pos, k): a ROLLING call (``hqt_set_row_positions``) -- the ``batch`` rows are slots, ``pos[b]`` the position slot b draws next (-1: empty); the
        call runs k steps, in step j every row with pos[b] + j < n_steps draws position pos[b] + j as a plain call draws it given that row's earlier codes.  Needs ``out``
        (the tensors the pass lives in: the positions drawn are written there, the codes of pos[b] - 1 read from there); ``logits_out`` / ``logprobs_out`` are filled
        the same way, and nothing of an idle row is written.  A slot continues exactly where the engine's rolling pass left it, joins at 0 or is empty (HqtError
        otherwise); ``cond[b]`` is read where a row stands at 0, ``row_seeds`` / ``row_offsets`` / ``row_samplers`` give each slot its request's key and settings.
        Text models: only on an engine with ``max_joins`` > 0 (``set_max_joins``), with at most that many rows at position 0 per call; ``cond`` is [B, ctx_len_txt], a
        joining row's prompt prefill draws its position 0 in front of the k steps, so it advances by 1 + k in that call (every other row by k).
        Not together with ``prefix``, ``keep``, ``prompt_groups`` or ``segment``.
        ``report_out`` (a ``DrawReport`` of caller-owned tensors, see ``check_report_out`` / ``new_draw_report``): the call writes entropy, rank and the top-N codes of the
        row behind every draw into them (``hqt_set_draw_report``), exactly where ``logprobs_out`` entries are written; nothing is appended to the returned values."""
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError('out: expected a pair (codes_top [B, n_steps], codes_bot [B, n_steps, 4])')
        outs, logits, logprobs = self._sample_levels(2, batch, cond, n_steps, precision=precision, top_k=top_k, top_p=top_p, temperature=temperature,
                                           noise=noise, seed=seed, sample_offset=sample_offset, force=(force_top, force_bot), out=out,
                                           return_logits=return_logits, use_graph=use_graph, row_seeds=row_seeds, row_offsets=row_offsets,
                                           row_samplers=row_samplers, prefix=prefix, return_logprobs=return_logprobs, guidance=guidance, keep=keep,
                                           prompt_groups=prompt_groups, segment=segment, logits_out=logits_out, logprobs_out=logprobs_out,
                                           row_positions=row_positions, report_out=report_out)
        return ((outs[0], outs[1]) + ((logits,) if return_logits or logits_out is not None else ())
                + ((logprobs,) if return_logprobs or logprobs_out is not None else ()))

    def sample3(self, batch: int, cond: Optional[torch.Tensor], n_steps: int, *, precision: int = PRECISION_FAST,
                top_k: Sequence[Optional[int]] = (None, None, None), top_p: Sequence[Optional[float]] = (None, None, None),
                temperature: Sequence[float] = (1.0, 1.0, 1.0), noise: Optional[torch.Tensor] = None, seed: int = 0,
                sample_offset: int = 0, force: Optional[Sequence[torch.Tensor]] = None, return_logits: bool = False,
                use_graph: bool = True, row_seeds: Optional[Sequence[int]] = None, row_offsets: Optional[Sequence[int]] = None,
                row_samplers: Optional[Sequence[tuple]] = None, prefix: Optional[Sequence[torch.Tensor]] = None,
                return_logprobs: bool = False, guidance: Optional[Sequence[tuple]] = None, keep: Optional[tuple] = None,
                prompt_groups=None, segment: Optional[Tuple[int, int]] = None, out: Optional[Sequence[torch.Tensor]] = None,
                logits_out: Optional[torch.Tensor] = None, logprobs_out: Optional[torch.Tensor] = None, row_positions: Optional[tuple] = None,
                report_out=None):
        """Three-level sampling: returns (codes0 [B, n], codes1 [B, n, 4], codes2 [B, n, 16][, logits [n, 21, B, V]][, logprobs [B, n, 21]]); ``row_samplers``,
        ``return_logprobs`` and ``guidance`` (three scales per pair) as in ``sample``;
        ``prefix`` = [[B, P], [B, P, 4], [B, P, 16]]: completion, as in ``sample`` (``hqt_sample_prefix_l3``);
        ``keep`` = (mask [B, n], [[B, n], [B, n, 4], [B, n, 16]]): kept positions, as in ``sample``; ``prompt_groups``: shared prompts, as in ``sample``;
        ``segment`` / ``logits_out`` / ``logprobs_out``: a segment of a pass, as in ``sample``; ``out`` = the three code tensors to write into, as ``sample`` takes two;
        ``row_positions`` = (pos, k): a rolling call, as in ``sample``; ``report_out``: a ``DrawReport`` of [B, n, 21(, N)] tensors to write, as in ``sample``."""
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise ValueError('out: expected the three code tensors ([B, n_steps], [B, n_steps, 4], [B, n_steps, 16])')
        outs, logits, logprobs = self._sample_levels(3, batch, cond, n_steps, precision=precision, top_k=top_k, top_p=top_p, temperature=temperature,
                                           noise=noise, seed=seed, sample_offset=sample_offset, force=(None,) * 3 if force is None else force,
                                           out=out, return_logits=return_logits, use_graph=use_graph, row_seeds=row_seeds, row_offsets=row_offsets,
                                           row_samplers=row_samplers, prefix=prefix, return_logprobs=return_logprobs, guidance=guidance, keep=keep,
                                           prompt_groups=prompt_groups, segment=segment, logits_out=logits_out, logprobs_out=logprobs_out,
                                           row_positions=row_positions, report_out=report_out)
        return (tuple(outs) + ((logits,) if return_logits or logits_out is not None else ())
                + ((logprobs,) if return_logprobs or logprobs_out is not None else ()))

    def select_rows(self, rows_from, paused_batch: Optional[int] = None) -> int:
        """``hqt_select_rows``: re-maps the rows of the pass a ``segment`` call left paused -- afterwards row j of the K/V cache holds what row ``rows_from[j]``
        held (any mapping: a permutation, a subset, duplicates), and the pass goes on with ``len(rows_from)`` rows.  The codes, keys and conditions are the
        caller's: gather them with the same mapping.  ``paused_batch``: the rows of the paused pass where the caller knows them (the mapping is then checked on the
        host, before any engine call; the library checks it in any case).  Asynchronous on torch's current stream.  Returns the new row count."""
        table = check_select_rows(rows_from, paused_batch, self.max_batch)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            _lib.check(self.lib.hqt_select_rows(self.h, len(table), table.ctypes.data_as(C.c_void_p), C.c_void_p(stream)))
        return len(table)

    def score(self, batch: int, cond: Optional[torch.Tensor], codes: Sequence[torch.Tensor], *, precision: int = PRECISION_FAST,
              return_logits: bool = False, report_out=None):
        """``hqt_score``: log-probabilities fp32 [B, n, draws] of GIVEN codes (the code levels as one list, coarse to fine, int64 [B, n], [B, n, 4][, [B, n, 16]])
        in ONE teacher-forced pass over all positions -- entry (b, t, d) is what ``sample(..., force_*=codes, return_logprobs=True)`` reports, at the cost of one
        body pass over n rows per sample and the depth head over the B n pairs in chunks of ``score_chunk``.  The engine needs ``max_prefix >= n - 1``.
        ``return_logits``: also the raw logits per level, fp32 [B, n, V], [B, n, 4, V][, [B, n, 16, V]] (the head GEMMs then write them directly).
        ``report_out``: a ``DrawReport`` of [B, n, draws(, N)] tensors the pass writes for the GIVEN codes (``hqt_set_draw_report``), as in ``sample``.
        Asynchronous on torch's current stream, like ``sample``."""
        dev = self.device
        B, V, L = int(batch), self.s2.vocab_top, self.s2.levels
        check_score_codes(self.s2, codes)
        n = int(torch.as_tensor(codes[0]).shape[1])
        if int(torch.as_tensor(codes[0]).shape[0]) != B:
            raise ValueError(f'codes hold {int(torch.as_tensor(codes[0]).shape[0])} samples, batch={B}')
        shapes = [(B, n) + ((4 ** l,) if l else ()) for l in range(L)]
        draws = (4 ** L - 1) // 3
        report = check_report_out(report_out, B, n, draws, dev, V)
        cond = self._prep_cond(cond, B)
        cs = [self._prep(c, shp, torch.int64, f'codes[{l}]', V) for l, (c, shp) in enumerate(zip(codes, shapes))]
        logprobs = torch.empty((B, n, draws), dtype=torch.float32, device=dev)
        logits = [torch.empty(shp + (V,), dtype=torch.float32, device=dev) for shp in shapes] if return_logits else None
        cp = (C.c_void_p * 3)(*[_ptr(c) for c in cs])
        lp = (C.c_void_p * 3)(*[_ptr(t) for t in logits]) if logits is not None else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            if report is not None:                  # staged on the handle; hqt_score takes it (and clears it even when it fails)
                _lib.check(self.lib.hqt_set_draw_report(self.h, C.byref(report[0])))
            _lib.check(self.lib.hqt_score(self.h, B, _ptr(cond), cp, n, int(precision), _ptr(logprobs), lp, C.c_void_p(stream)))
            self._note_split(precision, stream)
        self._keep = (cond, cs, cp, lp, report_out)
        return (logprobs, logits) if return_logits else logprobs

    # ------------------------------------------------------------------ stage 1, encode side
    @property
    def has_encoder(self) -> bool:
        return self.lib.hqt_has_encoder(self.h) == 1

    def encode(self, pixels: torch.Tensor, *, precision: int = PRECISION_EXACT, want_quant: bool = False,
               want_resid: bool = False, want_recon: bool = False, want_diff: bool = False) -> Dict[str, object]:
        """``SimRQGAN2Generator.encode`` / ``HQVAEGenerator.encode`` (generator.py:298-310, 530-568) through ``hqt_encode``:
        fp32 [B, 3, R, R] -> ``codes`` (list, coarse -> fine, int64 [B, r_l, r_l]) and on request ``quant`` / ``resid``
        (lists of fp32 [B, dim_l, r_l, r_l]), ``recon`` (fp32 [B, E, r, r]) and ``diff`` (fp32 [levels])."""
        dev = self.device
        s1 = self.s1
        x = pixels.to(device=dev, dtype=torch.float32).contiguous()
        B = int(x.shape[0])
        if tuple(x.shape) != (B, 3, s1.resolution, s1.resolution):
            raise ValueError(f'pixels: expected {(B, 3, s1.resolution, s1.resolution)}, got {tuple(x.shape)}')
        L = 3 if s1.code_levels == 3 else 2
        r, E = s1.z_res, s1.embed_dim
        o = hqt_encode_out()
        res: Dict[str, object] = {'codes': [], 'quant': [], 'resid': []}
        wide = s1.resample == 'pixelshuffle'      # 'nearest' / 'conv2': every level is E wide
        for l in range(L):
            k = L - 1 - l
            rq, dim = r >> k, (E * 4 ** k if wide else E)
            c = torch.empty((B, rq, rq), dtype=torch.int64, device=dev)
            res['codes'].append(c)
            o.codes[l] = _ptr(c)
            if want_quant:
                q = torch.empty((B, dim, rq, rq), dtype=torch.float32, device=dev)
                res['quant'].append(q)
                o.quant[l] = _ptr(q)
            if want_resid:
                z = torch.empty((B, dim, rq, rq), dtype=torch.float32, device=dev)
                res['resid'].append(z)
                o.resid[l] = _ptr(z)
        if want_recon:
            res['recon'] = torch.empty((B, E, r, r), dtype=torch.float32, device=dev)
            o.recon = _ptr(res['recon'])
        if want_diff:
            res['diff'] = torch.empty((L,), dtype=torch.float32, device=dev)
            o.diff = _ptr(res['diff'])
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(self.lib.hqt_encode(self.h, B, _ptr(x), int(precision), C.byref(o), C.c_void_p(stream)))
            self._note_split(precision, stream)
        self._keep_enc = x
        return res

    # ------------------------------------------------------------------ stage 1
    def _decode_levels(self, codes: Sequence[Optional[torch.Tensor]], *, precision: int, clamp01: bool, seq_layout: bool,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Code tensors, coarse to fine (2: hqt_decode[_seq], 3: hqt_decode[_seq]_l3), at least one not None (a missing level = zero quant):
        grids [B, r_l, r_l] or, ``seq_layout``, the sampler's [B, n], [B, n, 4][, [B, n, 16]]."""
        dev = self.device
        L, r = len(codes), self.s1.z_res
        if L not in _CODE_NAMES:
            raise ValueError(f'two or three code levels are built, got {L}')
        B = int(next(c for c in codes if c is not None).shape[0])
        if seq_layout:
            want = [(B, (r >> (L - 1)) ** 2) + ((4 ** l,) if l else ()) for l in range(L)]
        else:
            want = [(B, r >> (L - 1 - l), r >> (L - 1 - l)) for l in range(L)]
        for c, w, what in zip(codes, want, _CODE_NAMES[L]):
            if c is not None and tuple(c.shape) != w:
                raise ValueError(f'{what}: expected {w}, got {tuple(c.shape)}')
        for c, what in zip(codes, _CODE_NAMES[L]):
            self._check_index(c, self.s1.n_embed, what)
        cs = [None if c is None else c.to(device=dev, dtype=torch.int64).contiguous() for c in codes]
        H = self.s1.resolution
        if out is None:
            out = torch.empty((B, self.s1.out_ch, H, H), dtype=torch.float32, device=dev)
        else:
            self._check_out(out, (B, self.s1.out_ch, H, H), torch.float32, dev, 'out')
        fn = getattr(self.lib, 'hqt_decode' + ('_seq' if seq_layout else '') + ('_l3' if L == 3 else ''))
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(fn(self.h, B, *map(_ptr, cs), _ptr(out), int(clamp01), int(precision), C.c_void_p(stream)))
            self._note_split(precision, stream)
        self._keep_dec = cs
        return out

    def decode(self, code_t: Optional[torch.Tensor], code_b: Optional[torch.Tensor], *, precision: int = PRECISION_EXACT,
               clamp01: bool = False, seq_layout: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if code_t is None and code_b is None:
            raise ValueError('code_t and code_b are both None')
        return self._decode_levels((code_t, code_b), precision=precision, clamp01=clamp01, seq_layout=seq_layout, out=out)

    def decode3(self, codes: Sequence[Optional[torch.Tensor]], *, precision: int = PRECISION_EXACT, clamp01: bool = False,
                seq_layout: bool = False) -> torch.Tensor:
        """``HQVAEGenerator.decode_code([t, m, b])``; ``seq_layout``: the sampler's [B, n], [B, n, 4], [B, n, 16]."""
        if len(codes) != 3 or all(c is None for c in codes):
            raise ValueError('decode3 takes three code tensors, at least one not None')
        return self._decode_levels(codes, precision=precision, clamp01=clamp01, seq_layout=seq_layout)

    # ------------------------------------------------------------------ timing (bench.py roofline numerator)
    def timing(self, on: bool) -> None:
        _lib.check(self.lib.hqt_timing_enable(self.h, int(on)))

    def timing_reset(self) -> None:
        _lib.check(self.lib.hqt_timing_reset(self.h))

    def timing_report(self) -> Dict[str, Tuple[int, float]]:
        out = {}
        for i in range(self.lib.hqt_timing_slots(self.h)):
            name = C.create_string_buffer(64)
            n, ms = C.c_int64(), C.c_double()
            _lib.check(self.lib.hqt_timing_get(self.h, i, name, 64, C.byref(n), C.byref(ms)))
            out[name.value.decode()] = (int(n.value), float(ms.value))
        return out

    def workspace_bytes(self) -> int:
        return int(self.lib.hqt_workspace_bytes(self.h))
