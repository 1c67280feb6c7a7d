"""numpy restatement of the 'nearest' and 'conv2' HQ-VAE variants (``hparams_aux.upsample``; test infrastructure, never the product).

``ResampleOracle`` composes the unchanged ``OracleStage1.decoder(z)`` / ``.encoder(x)`` with the thin layer those variants change:
the codebook lookup, ``down_t``, ``upsample_t`` and the residual quantisation.  Each piece cites the reference lines it restates
(``hqvae/models/stage1/generator.py``).
"""
from typing import Dict, Optional

import numpy as np

from oracle.hqt_oracle import F32, OracleStage1, conv2d, nearest_code, pixel_unshuffle2, upsample_nearest2


class ResampleOracle(OracleStage1):
    def down_t(self, h: np.ndarray) -> np.ndarray:
        """generator.py:215 AvgPool2d(2) / generator.py:235 Conv2d(E, E, 2, stride 2)."""
        B, C, H, W = h.shape
        if self.s.resample == 'nearest':
            return (((h[:, :, 0::2, 0::2] + h[:, :, 0::2, 1::2]) + h[:, :, 1::2, 0::2]) + h[:, :, 1::2, 1::2]).astype(F32) * F32(0.25)
        w, b = self.w['down_t.weight'], self.w['down_t.bias']
        # stride == kernel: a Linear over the pixel-unshuffled map, whose channel ci * 4 + 2 a + b is the weight's own [ci][a][b] order
        return conv2d(pixel_unshuffle2(h), w.reshape(C, C * 4, 1, 1), b)

    def upsample_t(self, q: np.ndarray) -> np.ndarray:
        """generator.py:216-219 nearest x2 / generator.py:236-240 ConvTranspose2d(E, E, 2, stride 2): weight [in, out, kh, kw],
        up[co, 2y+a, 2x+b] = bias[co] + sum_ci q[ci, y, x] W[ci, co, a, b]."""
        if self.s.resample == 'nearest':
            return upsample_nearest2(q)
        w, b = self.w['upsample_t.weight'], self.w['upsample_t.bias']
        B, C, H, W = q.shape
        up = np.einsum('bcyx,coij->boyixj', q, w, optimize=True).reshape(B, w.shape[1], 2 * H, 2 * W)
        return (up + b[None, :, None, None]).astype(F32)

    def decode_code(self, code_t: Optional[np.ndarray], code_b: Optional[np.ndarray]) -> np.ndarray:
        """generator.py:323-367 + 312-321.  A missing level is a ZERO quant (339-342, 355-358) that still goes through
        ``decode``: a missing top level of 'conv2' therefore contributes upsample_t.bias."""
        assert code_t is not None or code_b is not None
        w, E = self.w, self.s.embed_dim
        ref = code_t if code_t is not None else code_b
        B = ref.shape[0]
        rb = self.s.z_res
        qt = w['quantize_t.embedding'][code_t].transpose(0, 3, 1, 2) if code_t is not None else np.zeros((B, E, rb // 2, rb // 2), F32)
        qb = w['quantize_b.embedding'][code_b].transpose(0, 3, 1, 2) if code_b is not None else np.zeros((B, E, rb, rb), F32)
        return self.decode(qt, qb)

    def decode(self, quant_t: np.ndarray, quant_b: np.ndarray) -> np.ndarray:
        """generator.py:312-321."""
        quant = np.concatenate([self.upsample_t(quant_t), quant_b], axis=1).astype(F32)
        return self.decoder(self._conv('post_quant_conv_b', quant))

    def encode(self, x: np.ndarray) -> Dict[str, object]:
        """generator.py:298-310; the same keys as ``OracleStage1.encode``."""
        w = self.w
        h = self._conv('quant_conv_b', self.encoder(x))
        h_t = self.down_t(h)
        q_t, diff_t, code_t = nearest_code(h_t, w['quantize_t.embedding'])
        up = self.upsample_t(q_t)
        h_b = (h - up).astype(F32)
        q_b, diff_b, code_b = nearest_code(h_b, w['quantize_b.embedding'])
        B = x.shape[0]
        return {'h': h, 'codes': [code_t.reshape(B, *h_t.shape[2:]), code_b.reshape(B, *h_b.shape[2:])], 'quant': [q_t, q_b],
                'resid': [h_t, h_b], 'diff': [diff_t, diff_b], 'recon': (q_b + up).astype(F32)}
