#!/usr/bin/env python3
"""Generate tests/golden/g13_tiny_cls_bidirectional.npz: the reference's two-level iHQGPT with model_type 'bidirectional4'
(hierarchical_ar.py:791-878) sampled on the CPU in fp32.

Container-only tool, like tools/gen_golden.py (whose import shims and multinomial replacement it reuses): the reference is imported,
only its outputs are committed.  Weights and noise are not stored; both sides regenerate them from hqtransformer_amd.synth.

    python tools/gen_golden_bidir.py
"""
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (binds the reference tree, stubs omegaconf)

import torch  # noqa: E402
from hqvae.models.stage2.hierarchical_ar import iHQGPT  # noqa: E402

from hqtransformer_amd import synth  # noqa: E402
from hqtransformer_amd.spec import Stage2Spec, stage2_param_shapes  # noqa: E402

OUT = os.path.join(gg.ROOT, 'tests', 'golden', 'g13_tiny_cls_bidirectional.npz')


def build_bidirectional(spec: Stage2Spec, seed: int):
    hp = gg.AD(embed_dim=spec.embed_dim, n_layers=spec.n_layers, n_heads=spec.n_heads, n_dense_layers=spec.n_layers,
               ctx_len=None, ctx_len_img=spec.ctx_len_img, ctx_len_txt=spec.ctx_len_txt, embd_pdrop=0.0,
               resid_pdrop=0.1, attn_pdrop=0.0, mlp_bias=True, attn_bias=True, gelu_use_approx=spec.gelu_approx,
               use_head_txt=True, n_classes=spec.n_classes, causal_attn=None,
               embedding_type='reduce' if spec.embedding == 1 else 'transformer1', position_embedding='1d',
               bottom_head_type='linear', use_random_order=False, rate_random_order=1.0)
    hp_dec = None
    if spec.n_layers_depth != 4:
        hp_dec = copy.deepcopy(hp)
        hp_dec.n_layers = spec.n_layers_depth
    m = iHQGPT(spec.vocab_top, spec.vocab_bot, spec.vocab_txt, 4, spec.cond == 1, spec.cond == 2, 'bidirectional4', hp, hp_dec)
    assert m.model_type == 'bidirectional' and m.bot_win == 2
    sd = {k: torch.from_numpy(v) for k, v in synth.stage2_weights(spec, seed, 'fixture').items()}
    ref_shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert ref_shapes == {k: tuple(v) for k, v in stage2_param_shapes(spec).items()}, 'spec.stage2_param_shapes != reference state_dict'
    m.load_state_dict(sd, strict=True)
    return m.eval(), ref_shapes


def main():
    out = {}
    # class-conditional, transformer1 embedding: the G4 model with the bidirectional head
    spec = Stage2Spec(embed_dim=128, n_layers=4, n_heads=4, n_layers_depth=4, vocab_top=512, vocab_bot=512, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0, depth_decoding='bidirectional')
    m, shapes = build_bidirectional(spec, seed=31)
    B, n, keep = 3, 32, [0, 1, 31]
    noise = synth.exp_noise(32, n, B, 512)
    cond = 6                     # the reference's sampling_ihqgpt takes one class id for every candidate
    # top and bottom k / p / T differ in both settings: the reference draws all five codes with temperature[0], top_k_bot, top_p_bot
    settings = [((8, 64), (0.5, 0.9), (0.9, 1.3)), ((None, 24), (None, 0.8), (1.2, 0.7))]
    out.update(spec=json.dumps(spec.__dict__), weight_seed=31, noise_seed=32, B=B, n_steps=n, cond=cond, keep_steps=np.array(keep),
               settings=json.dumps(settings), param_shapes=json.dumps({k: list(v) for k, v in shapes.items()}))
    for si, (tk, tp, T) in enumerate(settings):
        ct, cb, lg, margin = gg.run_sampling(m, spec, cond, B, n, noise, tk, tp, T)
        out[f'codes_top_{si}'], out[f'codes_bot_{si}'], out[f'logits_{si}'], out[f'margin_{si}'] = ct, cb, lg[keep], margin
        print(f'bidirectional tiny_cls setting {si}: margin {margin:.6f}')
    # unconditional, 'reduce' embedding, two depth blocks
    spec_r = Stage2Spec(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64,
                        ctx_len_img=64, ctx_len_txt=16, n_classes=0, cond=0, embedding=1, depth_decoding='bidirectional')
    m, _ = build_bidirectional(spec_r, seed=33)
    nr = 16
    noise = synth.exp_noise(34, nr, B, 512)
    tk, tp, T = (100, 32), (0.95, 0.9), (1.0, 0.8)
    ct, cb, lg, margin = gg.run_sampling(m, spec_r, None, B, nr, noise, tk, tp, T)
    out.update(reduce_spec=json.dumps(spec_r.__dict__), reduce_weight_seed=33, reduce_noise_seed=34, reduce_n_steps=nr,
               reduce_setting=json.dumps((tk, tp, T)), reduce_codes_top=ct, reduce_codes_bot=cb, reduce_logits=lg[[0, nr - 1]],
               reduce_keep_steps=np.array([0, nr - 1]), reduce_margin=margin)
    print(f'bidirectional tiny_reduce_uncond: margin {margin:.6f}')
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
