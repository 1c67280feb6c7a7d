#!/usr/bin/env python3
"""Generate the fixtures of the 'conv2' and 'nearest' HQ-VAE variants (tests/golden/g14_resample_*.npz) by running the
REFERENCE's own ``SimRQGAN2Generator`` (CPU, fp32) with ``hparams_aux.upsample`` = ``conv2`` / ``nearest`` in the build container.

Container-only, like tools/gen_golden_enc.py: it imports the reference.  Only inputs and expected outputs are committed; weights
come from hqtransformer_amd.synth on both sides (keyed by state-dict name), images from ``gen_golden_enc.synth_images``.

Condition (as for G9): the smallest best / second-best squared-distance gap of every level must be >= MIN_MARGIN, so that
bit-identical codes are a well-conditioned demand; the weight seed is searched upwards from a start value until it holds, and
the seed used is stored in the fixture.

    python tools/gen_golden_resample.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the import shims)
import torch  # noqa: E402
from gen_golden_enc import code_margin, synth_images  # noqa: E402
from hqvae.models.stage1.generator import SimRQGAN2Generator  # noqa: E402

from hqtransformer_amd import synth  # noqa: E402
from hqtransformer_amd.spec import Stage1Spec, stage1_is_ignored  # noqa: E402

MIN_MARGIN = 4e-4


def build(spec: Stage1Spec, seed: int):
    hp = G.AD(double_z=False, z_channels=spec.z_channels, resolution=spec.resolution, in_channels=3, out_ch=spec.out_ch,
              ch=spec.ch, ch_mult=list(spec.ch_mult), num_res_blocks=spec.num_res_blocks,
              attn_resolutions=list(spec.attn_resolutions), pdrop=0.0, use_init_downsample=spec.use_init_downsample,
              use_mid_block=spec.use_mid_block, use_attn=spec.use_attn)
    aux = G.AD(upsample=spec.resample, shared_codebook=False, bottom_start=10 ** 11, decoding_type='concat',
               restart_unused_codes=None, code_levels=None)
    g = SimRQGAN2Generator(spec.n_embed, spec.embed_dim, True, hp, aux)
    sd = {k: torch.from_numpy(v) for k, v in synth.stage1_weights(spec, seed, 'fixture', encoder=True).items()}
    ref_shapes = {k: tuple(v.shape) for k, v in g.state_dict().items() if not stage1_is_ignored(k)}
    mine = {k: tuple(v.shape) for k, v in sd.items()}
    assert ref_shapes == mine, (sorted(set(ref_shapes) ^ set(mine)), [k for k in ref_shapes if k in mine and ref_shapes[k] != mine[k]])
    missing, unexpected = g.load_state_dict(sd, strict=False)
    assert not unexpected and all(stage1_is_ignored(k) for k in missing), (missing, unexpected)
    return g.eval(), ref_shapes


def main():
    os.makedirs(G.OUT, exist_ok=True)
    torch.set_grad_enabled(False)
    B = 3
    for resample, first_seed in (('conv2', 141), ('nearest', 151)):
        # G9's 64 x 64 shape (= G5's decode shape): 4x4 stride-2 conv_in, two levels, mid attention, 8x8 top / 16x16 bottom codes
        spec = Stage1Spec(ch=32, ch_mult=[1, 2], num_res_blocks=2, attn_resolutions=[16], resolution=64, z_channels=32,
                          embed_dim=16, n_embed=64, resample=resample)
        x = synth_images(first_seed + 1000, B, spec.resolution)
        xt = torch.from_numpy(x)
        for seed in range(first_seed, first_seed + 50):
            g, shapes = build(spec, seed)
            h_b = g.quant_conv_b(g.encoder(xt))
            h_t = g.down_t(h_b)
            quant_t, quant_b, diff_t, diff_b, (code_t, code_b, resid_b) = g.encode(xt)
            margins = [code_margin(h_t, g.quantize_t.embedding), code_margin(resid_b, g.quantize_b.embedding)]
            if min(margins) >= MIN_MARGIN:
                break
            print(f'{resample}: weight seed {seed} has margins {margins}, trying the next one')
        else:
            raise SystemExit(f'{resample}: no weight seed with margins >= {MIN_MARGIN}')
        assert min(margins) >= MIN_MARGIN
        ct, cb = g.get_codes(xt)
        assert (ct == code_t).all() and (cb == code_b).all()
        r = np.random.default_rng(seed + 1)
        rt, rb = spec.z_res // 2, spec.z_res
        dct = r.integers(0, spec.n_embed, (2, rt, rt))
        dcb = r.integers(0, spec.n_embed, (2, rb, rb))
        px = g.decode_code(torch.from_numpy(dct), torch.from_numpy(dcb))
        px_t = g.decode_code(torch.from_numpy(dct[:1]), None)
        px_b = g.decode_code(None, torch.from_numpy(dcb[:1]))
        # decode_code(codes) is decode(codebook rows): the lookup is the only thing between them
        qt = g.quantize_t.get_codebook_entry(torch.from_numpy(dct)).permute(0, 3, 1, 2)
        qb = g.quantize_b.get_codebook_entry(torch.from_numpy(dcb)).permute(0, 3, 1, 2)
        assert float((g.decode(qt, qb) - px).abs().max()) <= 5e-6
        z = g.post_quant_conv_b(torch.cat([g.upsample_t(qt), qb], dim=1))
        out = dict(spec=G.spec_json(spec), weight_seed=seed, image_seed=first_seed + 1000, B=B,
                   param_shapes=json.dumps({k: list(v) for k, v in shapes.items()}),
                   # decode side
                   code_t=dct, code_b=dcb, pixels=px.numpy(), pixels_top_only=px_t.numpy(), pixels_bot_only=px_b.numpy(), z=z.numpy()[:1],
                   # encode side: level 0 = top, 1 = bottom
                   images=x, h=h_b.numpy(), resid_0=h_t.numpy(), resid_1=resid_b.numpy(),
                   enc_code_0=code_t.numpy(), enc_code_1=code_b.numpy(), quant_0=quant_t.numpy(), quant_1=quant_b.numpy(),
                   recon=(quant_b + g.upsample_t(quant_t)).numpy(), diff_0=np.float32(diff_t), diff_1=np.float32(diff_b),
                   reconstruction=g.decode(quant_t, quant_b).numpy().astype(np.float32), margins=np.array(margins))
        path = os.path.join(G.OUT, f'g14_resample_{resample}.npz')
        np.savez_compressed(path, **out)
        print(f'g14_resample_{resample} ok: weight seed {seed}, margins', ['%.3g' % m for m in margins], 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
