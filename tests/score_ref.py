"""Shared by the one-pass scoring tests (hqt_score): the G15 fixtures -- the reference's eval-mode forward on codes its own sampler drew,
tools/gen_golden_forward.py -- with the model, conditioning and noise each one names, and the oracle that replays them on the CPU."""
import json

import numpy as np

from hqtransformer_amd import synth
from hqtransformer_amd.spec import Stage2Spec
from oracle.hqt_oracle import F32, OracleStage2, OracleStage2L3, layer_norm, linear, sample_filtered
from tests.helpers import load

G15 = ['tiny_cls', 'tiny_txt', 'tiny_cls_bidirectional', 'l3_tiny_cls']
LOGPROB_TOL = 4e-4       # |d logprob| <= |d l_code| + |d lse| <= 2 max|d l|, with the project's EXACT logit gate of 2e-4 against reference fixtures
LOGIT_TOL = 2e-4


def g15(name):
    """(fixture, spec, weights, cond [B] / [B, ctx_len_txt], codes per level in the sampler's layout)."""
    fx = load(f'g15_forward_{name}.npz')
    spec = Stage2Spec(**json.loads(str(fx['spec'])))
    weights = synth.stage2_weights(spec, int(fx['weight_seed']), 'fixture')
    B = int(fx['B'])
    cond = synth.text_ids(int(fx['text_seed']), B, spec.ctx_len_txt, spec.vocab_txt) if spec.cond == 2 else np.full((B,), int(fx['cond']), np.int64)
    return fx, spec, weights, cond, [fx[f'codes{l}'] for l in range(spec.levels)]


def g15_noise(fx, spec):
    B, n = int(fx['B']), int(fx['n_steps'])
    if spec.levels == 3:
        return np.maximum(np.random.default_rng([int(fx['noise_seed']), 0x9e3779b9]).standard_exponential((n, 21, B, spec.vocab_top), dtype=np.float32), np.float32(1e-30))
    return synth.exp_noise(int(fx['noise_seed']), n, B, spec.vocab_top)


class OracleBidirectional(OracleStage2):
    """iHQGPT 'bidirectional4' sampling (hierarchical_ar.py:791-878) on the oracle's blocks: per position ONE pass of the depth blocks over five rows,
    [ln_f(h) + sos_depth, pos_emb_depth[0..3]], full attention and no cache; top logits from row 0, bottom from rows 1..4.  All five draws use
    temperature[0], top_k[1] and top_p[1] (:866-873, as run_position does); by default T = 1 without cut-offs.  The logits returned are the raw ones."""

    def sample(self, cond, batch, n_steps, noise, top_k=(None, None), top_p=(None, None), temperature=(1.0, 1.0), return_logits=True):
        w, s = self.w, self.s
        B = batch
        sos = w['sos.weight'][np.asarray(cond, np.int64).reshape(-1)][:, None, :] if s.cond == 1 else np.repeat(w['sos'], B, axis=0)
        cache = {}
        ct, cb = np.zeros((B, n_steps), np.int64), np.zeros((B, n_steps, 4), np.int64)
        logits = np.zeros((n_steps, 5, B, s.vocab_top), F32)
        for cnt in range(n_steps):
            xs = sos.astype(F32) if cnt == 0 else self._embed(ct[:, cnt - 1], cb[:, cnt - 1], cnt - 1)
            for i in range(s.n_layers):
                xs = self._block(f'blocks.{i}', xs, cache, causal_new=True)
            hs = layer_norm(xs, w['ln_f.weight'], w['ln_f.bias'])
            xd = np.concatenate([hs + w['sos_depth'], np.repeat(w['pos_emb_depth.weight'][None, :4], B, axis=0)], axis=1).astype(F32)
            dcache = {}
            for j in range(s.n_layers_depth):
                xd = self._block(f'depths.{j}', xd, dcache, causal_new=False)
            logits[cnt, 0] = linear(layer_norm(xd[:, :1], w['ln_top.weight'], w['ln_top.bias']), w['head_top.weight'])[:, 0]
            logits[cnt, 1:] = linear(layer_norm(xd[:, 1:], w['ln_bot.weight'], w['ln_bot.bias']), w['head_bot.weight']).transpose(1, 0, 2)
            ct[:, cnt], _ = sample_filtered(logits[cnt, 0], noise[cnt, 0], temperature[0], top_k[1], top_p[1])
            for k in range(4):
                cb[:, cnt, k], _ = sample_filtered(logits[cnt, 1 + k], noise[cnt, 1 + k], temperature[0], top_k[1], top_p[1])
        return ct, cb, logits


def oracle_free_run(spec, weights, cond, n, noise):
    """The oracle's free run at T = 1 without cut-offs -> (codes per level, raw logits [n, draws, B, V])."""
    B = noise.shape[2]
    if spec.levels == 3:
        *codes, lg = OracleStage2L3(spec, weights).sample(cond, B, n, noise, return_logits=True)
    elif spec.depth_decoding == 'bidirectional':
        *codes, lg = OracleBidirectional(spec, weights).sample(cond, B, n, noise)
    else:
        *codes, lg = OracleStage2(spec, weights).sample(cond, B, n, noise, return_logits=True)
    return codes, lg


def log_softmax_at(logits, codes):
    """fp64 log-softmax of rows [n, draws, B, V] at the codes (levels in the sampler's layout) -> [B, n, draws]."""
    l = np.asarray(logits, np.float64)
    m = l.max(-1)
    lse = m + np.log(np.exp(l - m[..., None]).sum(-1))
    B, n = codes[0].shape
    picked = np.concatenate([np.asarray(c).reshape(B, n, -1) for c in codes], axis=2)
    return (np.take_along_axis(l, picked.transpose(1, 2, 0)[..., None], -1)[..., 0] - lse).transpose(2, 0, 1)
