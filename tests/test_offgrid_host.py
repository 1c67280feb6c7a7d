"""The off-grid case table (tests/offgrid_cases.py) on the CPU: every row runs through the oracle, its closest draw is well-conditioned for the
bit-exact comparison the GPU tests make (tests/test_gpu_offgrid_stage2.py), and its logits are finite -- so an ill-conditioned draw is found here and
never shows up as a GPU failure."""
import numpy as np
import pytest

from tests import offgrid_cases as OG


@pytest.mark.parametrize('name', list(OG.ROWS))
def test_oracle_runs_and_every_draw_is_well_conditioned(name):
    spec, weights, cond, noise, B, n, settings = OG.inputs(name)
    ct, cb, lg, margin = OG.oracle(name)
    print(f'{name}: B={B} n={n} D={spec.embed_dim} head size {spec.head_dim} V={spec.vocab_top}: margin {margin:.6f}, logit std {lg.std():.3f}, max |logit| {np.abs(lg).max():.2f}')
    assert ct.shape == (B, n) and cb.shape == (B, n, 4) and lg.shape == (n, 5, B, spec.vocab_top)
    assert margin >= OG.MIN_MARGIN, f'case {name}: the oracle\'s closest draw has margin {margin}: ill-conditioned for a bit-exact comparison, check another step'
    assert np.isfinite(lg).all()
    assert 0 <= ct.min() and ct.max() < spec.vocab_top and 0 <= cb.min() and cb.max() < spec.vocab_top


def test_the_table_is_off_the_grid_the_rest_of_the_suite_runs():
    """What each row is for, stated on its shape: hqt_create's conditions hold, and the property that sends the dispatcher elsewhere is there."""
    for name, (spec, B, n) in OG.CASES.items():
        D, hs, V = spec.embed_dim, spec.head_dim, spec.vocab_top
        assert D % 16 == 0 and D % spec.n_heads == 0 and hs in (8, 16, 32, 64, 128, 256) and V % 4 == 0 and V <= 16384 and n <= spec.ctx_len_img, name
    s = {k: v[0] for k, v in OG.CASES.items()}
    assert s['A'].embed_dim % 32 and s['A'].vocab_top % 16 and s['A'].vocab_top < 256
    assert s['B'].head_dim == 8 and s['B'].embed_dim % 32 == 0 and s['B'].vocab_top % 32 and s['B'].embed_dim % 64 and 4 * OG.CASES['B'][1] > 256
    assert s['C'].head_dim == 256 and OG.CASES['C'][2] > 2 * 16                      # three groups of 16 keys
    assert s['D'].head_dim == 128 and s['D'].ctx_len_txt + OG.CASES['D'][2] == 71 and s['D'].vocab_top % 32
    assert s['E'].embed_dim % 32 and (4 * s['E'].embed_dim) % 32 == 0 and 4 * OG.CASES['E'][1] > 256 and s['E'].cond == 0 and s['E'].embedding == 1
    assert s['F'].head_dim == 64 and s['F'].ctx_len_txt + OG.CASES['F'][2] == 128
    assert OG.CASES['G'][1] >= 256 and s['G'].ctx_len_txt + OG.CASES['G'][2] > 64
    assert [r for r in OG.ROWS if r.startswith('V')] == [f'V{V}-{k}' for V in OG.SWEEP_V for k in ('plain', 'cut')]
    assert OG.sweep_settings(16384, True)['top_p'] == (None, None) and OG.sweep_settings(5000, True)['top_k'] == (1666, 37)
