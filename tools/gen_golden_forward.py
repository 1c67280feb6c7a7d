#!/usr/bin/env python3
"""Generate tests/golden/g15_forward_{tiny_cls,tiny_txt,tiny_cls_bidirectional,l3_tiny_cls}.npz: the reference's eval-mode ``forward``
(iHQGPT.forward, hierarchical_ar.py:246-426; HQTransformer.forward, hqtransformer.py:226-407) on codes the reference's own sampler drew.

Container-only tool, like tools/gen_golden.py (whose import shims, builders and multinomial replacement it reuses, with the builders of
tools/gen_golden_bidir.py and tools/gen_golden_l3.py): the reference is imported, only its outputs are committed.  Weights, noise and text
prompts are not stored; both sides regenerate them from hqtransformer_amd.synth.

Each fixture uses the model, weight seed and conditioning of G4 / G3 / G13 / G7 with B = 2 and n = 64.  The codes are the reference's free run
under seeded Exp(1) noise at T = 1 without cut-offs; ``forward`` then sees them in its global raster layout.  Kept: ``logprob`` fp32 [B, n, draws]
(fp64 log-softmax of forward's logits at the codes), the whole ``logits_top``, the finer levels' logits at positions {0, 1, 31, 63} in the sampler's
layout, and the largest difference between forward's logits and the stepwise sampler's on the same codes.

    python tools/gen_golden_forward.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (binds the reference tree, stubs omegaconf)
import gen_golden_bidir as gb  # noqa: E402
import gen_golden_l3 as g3  # noqa: E402

import torch  # noqa: E402

from hqtransformer_amd import synth  # noqa: E402
from hqtransformer_amd.sampling import global_to_sequence_index  # noqa: E402
from hqtransformer_amd.spec import Stage2Spec  # noqa: E402

B, N, KEEP = 2, 64, [0, 1, 31, 63]


def to_global(seq: np.ndarray, level: int) -> torch.Tensor:
    """Sampler layout [B, n, 4 ** level] -> the reference's global raster layout [B, n 4 ** level]."""
    idx = global_to_sequence_index(seq.shape[1], level).reshape(-1)
    out = torch.empty((seq.shape[0], idx.numel()), dtype=torch.int64)
    out[:, idx] = torch.from_numpy(seq).reshape(seq.shape[0], -1)
    return out


def to_sequence(logits: torch.Tensor, n: int, level: int) -> np.ndarray:
    """forward's logits of a finer level [B, n 4 ** level, V] -> the sampler's layout [B, n, 4 ** level, V]."""
    idx = global_to_sequence_index(n, level)
    return logits[:, idx.reshape(-1)].reshape(logits.shape[0], n, idx.shape[1], -1).numpy()


def finish(name, model, codes, labels, stepwise, margin, meta):
    """codes: the sampler's layout, coarse to fine; stepwise: its raw logits [n, draws, B, V]."""
    glob = [torch.from_numpy(codes[0])] + [to_global(c, l) for l, c in enumerate(codes) if l]
    out = model(tuple(glob) if len(glob) == 2 else glob, labels)
    levels = [out[0].numpy()] + [to_sequence(out[l], N, l) for l in range(1, len(codes))]
    full = np.concatenate([lv.reshape(B, N, -1, lv.shape[-1]) for lv in levels], axis=2)          # [B, n, draws, V]
    diff = float(np.abs(full - stepwise.transpose(2, 0, 1, 3)).max())
    l64 = full.astype(np.float64)
    m = l64.max(-1)
    lse = m + np.log(np.exp(l64 - m[..., None]).sum(-1))
    picked = np.concatenate([c.reshape(B, N, -1) for c in codes], axis=2)
    logprob = (np.take_along_axis(l64, picked[..., None], -1)[..., 0] - lse).astype(np.float32)
    fx = dict(meta, B=B, n_steps=N, keep_steps=np.array(KEEP), margin=margin, forward_vs_stepwise=diff, logprob=logprob, logits_top=levels[0].astype(np.float32))
    for l, c in enumerate(codes):
        fx[f'codes{l}'] = c
        if l:
            fx[f'logits{l}'] = levels[l][:, KEEP].astype(np.float32)
    path = os.path.join(gg.OUT, f'g15_forward_{name}.npz')
    np.savez_compressed(path, **fx)
    print(f'{name}: margin {margin:.6f}, forward vs stepwise {diff:.3e}, logprob in [{logprob.min():.3f}, {logprob.max():.3f}], {os.path.getsize(path)} bytes')
    assert diff < 1e-4 and os.path.getsize(path) < 934 * 1024


def two_level(name, spec, weight_seed, noise_seed, cond, build, extra=None):
    m, _ = build(spec, weight_seed)
    noise = synth.exp_noise(noise_seed, N, B, spec.vocab_top)
    ct, cb, lg, margin = gg.run_sampling(m, spec, cond, B, N, noise, (None, None), (None, None), (1.0, 1.0))
    labels = cond if torch.is_tensor(cond) else (torch.full((B,), int(cond)) if cond is not None else None)
    meta = dict(spec=json.dumps(spec.__dict__), weight_seed=weight_seed, noise_seed=noise_seed, **(extra or {}))
    finish(name, m, [ct, cb], labels, lg, margin, meta)


def main():
    tiny_cls = Stage2Spec(embed_dim=128, n_layers=4, n_heads=4, n_layers_depth=4, vocab_top=512, vocab_bot=512, vocab_txt=64,
                          ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    two_level('tiny_cls', tiny_cls, 3, 151, 7, gg.build_stage2, dict(cond=7))
    tiny_txt = Stage2Spec(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=4, vocab_top=512, vocab_bot=512, vocab_txt=64,
                          ctx_len_img=64, ctx_len_txt=16, n_classes=0, cond=2, embedding=0)
    two_level('tiny_txt', tiny_txt, 5, 152, torch.from_numpy(synth.text_ids(8, B, 16, 64)), gg.build_stage2, dict(text_seed=8))
    bidir = Stage2Spec(embed_dim=128, n_layers=4, n_heads=4, n_layers_depth=4, vocab_top=512, vocab_bot=512, vocab_txt=64,
                       ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0, depth_decoding='bidirectional')
    two_level('tiny_cls_bidirectional', bidir, 31, 153, 6, gb.build_bidirectional, dict(cond=6))
    l3 = Stage2Spec(embed_dim=128, n_layers=3, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64,
                    ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0, levels=3)
    m, _ = g3.build_stage2_l3(l3, 61)
    noise = np.maximum(np.random.default_rng([154, 0x9e3779b9]).standard_exponential((N, 21, B, l3.vocab_top), dtype=np.float32), np.float32(1e-30))
    codes, lg, margin = g3.run_sampling_l3(m, B, 7, N, noise, (None,) * 3, (None,) * 3, (1.0,) * 3)
    finish('l3_tiny_cls', m, codes, torch.full((B,), 7), lg, margin, dict(spec=json.dumps(l3.__dict__), weight_seed=61, noise_seed=154, cond=7))


if __name__ == '__main__':
    main()
