"""The off-grid depth-head table (tests/offgrid_depth_cases.py) on the CPU: every case runs through its oracle, its closest draw is well-conditioned
for the bit-exact comparison the GPU tests make (tests/test_gpu_offgrid_depth.py), its logits are finite, each case has on its shape the property it is
named for, the bidirectional oracle's sampler settings are pinned on the reference's fixture G13, and the attention kernel of every depth sub-step is
predicted from head size, Tq, t_base, B and precision -- the prediction the GPU test holds the engine's counters to."""
import json

import numpy as np
import pytest

from hqtransformer_amd import synth
from hqtransformer_amd.spec import Stage2Spec
from tests import offgrid_depth_cases as DC
from tests.helpers import load
from tests.score_ref import OracleBidirectional

LOGIT_TOL = 2e-4


@pytest.mark.parametrize('name', list(DC.CASES))
def test_oracle_runs_and_every_draw_is_well_conditioned(name):
    spec, weights, cond, noise, B, n, settings = DC.inputs(name)
    codes, lg, margin = DC.oracle(name)
    print(f'{name}: {spec.depth_decoding} B={B} n={n} D={spec.embed_dim} head size {spec.head_dim} V={spec.vocab_top}: margin {margin:.6f}, '
          f'logit std {lg.std():.3f}, max |logit| {np.abs(lg).max():.2f}')
    widths = (1, 4) if DC.is_bidir(name) else (1, 4, 16)
    assert [c.shape for c in codes] == [(B, n) if w == 1 else (B, n, w) for w in widths]
    assert lg.shape == (n, sum(widths), B, spec.vocab_top) and noise.shape == lg.shape
    assert margin >= DC.MIN_MARGIN, f'case {name}: the oracle\'s closest draw has margin {margin}: ill-conditioned for a bit-exact comparison, give the case another noise seed'
    assert np.isfinite(lg).all()
    assert all(0 <= c.min() and c.max() < spec.vocab_top for c in codes)


@pytest.mark.parametrize('si', [0, 1])
def test_the_bidirectional_oracle_draws_with_the_settings_as_the_reference_does(si):
    """Fixture G13 (tools/gen_golden_bidir.py, from the reference): two settings that give top and bottom different k, p and T.  All five draws take
    temperature[0], top_k[1] and top_p[1]; the reference logs post-temperature logits, the oracle returns the raw ones."""
    fx = load('g13_tiny_cls_bidirectional.npz')
    spec = Stage2Spec(**json.loads(str(fx['spec'])))
    weights = synth.stage2_weights(spec, int(fx['weight_seed']), 'fixture')
    tk, tp, T = json.loads(str(fx['settings']))[si]
    assert (tk[0], tp[0], T[0]) != (tk[1], tp[1], T[1])
    B, n = int(fx['B']), int(fx['n_steps'])
    noise = synth.exp_noise(int(fx['noise_seed']), n, B, spec.vocab_top)
    ct, cb, lg = OracleBidirectional(spec, weights).sample(np.full((B,), int(fx['cond'])), B, n, noise, tk, tp, T)
    err = np.abs(lg[fx['keep_steps']] / np.float32(T[0]) - fx[f'logits_{si}']).max()
    print(f'setting {si}: top_k {tk} top_p {tp} T {T}: logit error {err:.2e}')
    assert err <= LOGIT_TOL
    assert (ct == fx[f'codes_top_{si}']).all() and (cb == fx[f'codes_bot_{si}']).all()


def test_the_bidirectional_oracle_defaults_to_plain_draws():
    spec, weights, cond, noise, B, n, _ = DC.inputs('BA')
    a = OracleBidirectional(spec, weights).sample(cond, B, 2, noise[:2])
    b = OracleBidirectional(spec, weights).sample(cond, B, 2, noise[:2], (7, None), (0.3, None), (1.0, 0.5))      # the three values that must not matter
    assert all((x == y).all() for x, y in zip(a, b))


def test_the_table_is_off_the_grid_the_rest_of_the_suite_runs():
    """What each case is for, stated on its shape: hqt_create's conditions hold, and the property that sends the dispatchers elsewhere is there."""
    for name, (spec, B, n) in DC.CASES.items():
        D, hs, V = spec.embed_dim, spec.head_dim, spec.vocab_top
        assert D % 16 == 0 and D % spec.n_heads == 0 and hs in (8, 16, 32, 64, 128, 256) and V % 4 == 0 and V <= 16384 and n <= spec.ctx_len_img == 16, name
        assert spec.levels == (2 if name in DC.BIDIR else 3)
    s = {k: v[0] for k, v in DC.CASES.items()}
    Bs = {k: v[1] for k, v in DC.CASES.items()}
    heads = {k: v.depth_decoding for k, v in s.items()}
    assert heads == dict(LA='parallel-add', LB='parallel', LC='parallel-reduce', LD='parallel-add', LE='top2mid2bot', LF='top2mid2bot', LG='top2mid2bot',
                         BA='bidirectional', BB='bidirectional', BC='bidirectional', BD='bidirectional', BE='bidirectional')
    # LA / BA: K = 48 has neither the fp32 matrix path nor packed weights; sampler rows under 256 entries
    for k in ('LA', 'BA'):
        assert s[k].embed_dim % 32 and s[k].vocab_top % 16 and s[k].vocab_top < 256 and s[k].head_dim == 16
    assert [Bs['LA'] * t for t in (1, 4, 16)] == [5, 20, 80] and 5 * Bs['BA'] == 25
    # LB: 272 rows above the fp32 matrix path's 256; one lane per key row; a packed body (D % 32 == 0) in front of an unpacked head (V % 32 != 0)
    assert 16 * Bs['LB'] == 272 > 256 and s['LB'].head_dim == 8 and s['LB'].embed_dim % 32 == 0 and s['LB'].vocab_top % 32 and s['LB'].vocab_top % 16
    # LC: [V, 4 D] tables, head size 128, a vocabulary with a tail
    assert 'reduce' in heads['LC'] and s['LC'].head_dim == 128 and s['LC'].vocab_top % 32
    assert synth.stage2_weights(s['LC'], 900, 'fixture')['tok_emb_depth_levels.1.weight'].shape == (516, 4 * 256)
    # LD / LF / BC: head size 256 -- 16 keys per online-softmax group, so 21 keys cross into a second group; no few-query form beyond 8 keys
    for k in ('LD', 'LF', 'BC'):
        assert s[k].head_dim == 256 and 64 // (256 // 8) * 8 == 16 < 21 and s[k].embed_dim % 32 == 0 and s[k].vocab_top % 32 == 0
    # LE: unconditional, K = 80, a ragged batch
    assert s['LE'].cond == 0 and s['LE'].embed_dim % 32 and Bs['LE'] % 32 and Bs['LE'] > 64
    # LG: the production head size at the row count from which FAST takes the eight-heads kernel
    assert s['LG'].head_dim == 64 and Bs['LG'] >= 256
    # BB: 335 rows -- a ragged (M + 3) / 4 LayerNorm grid whose row map divides by 5, a 512-row packed block, compact operands of 67 and 268 rows
    M = 5 * Bs['BB']
    assert M == 335 and M % 4 and M % 5 == 0 and 256 < M <= 512 and 4 * Bs['BB'] == 268 and s['BB'].vocab_top % 32 and s['BB'].embed_dim % 32 == 0
    assert s['BD'].head_dim == 128 and s['BD'].vocab_top % 32
    assert s['BE'].cond == 0 and s['BE'].embedding == 1 and s['BE'].embed_dim % 32 and (4 * s['BE'].embed_dim) % 32 == 0
    # the sampler settings: three levels cut levels 1 and 2 differently; the bidirectional head reads temperature[0], top_k[1], top_p[1]
    assert DC.SETTINGS_L3 == dict(top_k=(None, 20, 37), top_p=(None, 0.9, None), temperature=(1.0, 0.9, 0.8))
    assert DC.SETTINGS_BIDIR == dict(top_k=(None, 20), top_p=(None, 0.9), temperature=(0.9, 1.0))


# What the issue's reading of launch_attention says each case reaches, per depth sub-step (None: the single-key shortcut, no launch)
_G, _1, _2, _H = 'generic', 'fewq1', 'fewq2', 'heads8'
WANT = {
    ('LA', False): [_G, _1, _1], ('LA', True): [_G, _1, _1],                 # hs 16: 32 keys per pass, 5 and 21 keys in one
    ('LB', False): [_G, _1, _1], ('LB', True): [_G, _1, _1],                 # hs 8: 64 keys per pass
    ('LC', False): [_G, _2, _G], ('LC', True): [_G, _2, _G],                 # hs 128: 4 keys per pass; 5 keys in two, 21 beyond the bound of 8
    ('LD', False): [_G, _G, _G], ('LD', True): [None, _G, _G],               # hs 256: 2 keys per pass; 5 keys beyond the bound of 4
    ('LE', False): [_G] * 21, ('LE', True): [_G] * 21,
    ('LF', False): [_G] * 21, ('LF', True): [None] + [_G] * 20,
    ('LG', False): [_G] * 21, ('LG', True): [None] + [_H] * 20,
    ('BA', False): [_1], ('BA', True): [_1], ('BB', False): [_1], ('BB', True): [_1],
    ('BC', False): [_G], ('BC', True): [_G], ('BD', False): [_2], ('BD', True): [_2], ('BE', False): [_1], ('BE', True): [_1],
}


@pytest.mark.parametrize('name', list(DC.CASES))
def test_the_attention_kernel_of_every_depth_sub_step_is_predicted(name):
    for fast in (False, True):
        assert DC.predicted_attention(name, fast) == WANT[(name, fast)], (name, fast)


def test_the_attention_choice_at_its_thresholds():
    """The bounds of the few-query kernel, as launch_attention states them: 1 < Tq <= 16, t_base + Tq <= 1024 / hs, one pass up to 512 / hs."""
    c = DC.attention_choice
    for hs in (8, 16, 32, 64, 128, 256):
        one, two = 512 // hs, 1024 // hs
        for Tq in (2, 4, 5, 16):
            for keys in {Tq, one, one + 1, two, two + 1}:
                if keys < Tq:
                    continue
                want = 'fewq1' if keys <= one else ('fewq2' if keys <= two else 'generic')
                assert c(hs, Tq, keys - Tq, 5, False) == want, (hs, Tq, keys)
        assert c(hs, 17, 0, 5, False) == 'generic' and c(hs, 1, 0, 5, False) == 'generic'
    assert c(32, 16, 5, 5, False) == 'fewq2' and c(64, 16, 5, 5, False) == 'generic'          # level 2 of a three-level head: 21 keys
    assert c(64, 4, 1, 64, False) == 'fewq8' and c(64, 4, 1, 63, False) == 'fewq1' and c(64, 5, 0, 64, False) == 'fewq1'
    assert c(64, 1, 7, 256, True) == 'heads8' and c(64, 1, 7, 255, True) == 'generic' and c(64, 1, 7, 256, False) == 'generic'
    # batch composition (EXACT): the kernel of a row does not depend on the rows beside it
    for name in ('LE', 'BB'):
        assert DC.predicted_attention(name, False, B=5) == DC.predicted_attention(name, False)
