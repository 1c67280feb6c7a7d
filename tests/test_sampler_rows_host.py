"""The table of tests/sampler_rows.py, checked on the CPU: the injection is exact on the oracle at both heads, every case is well-conditioned with the
reference alone, and the table reaches every code path of the sampler kernels it was written for (restated as data -- the GPU tests run them)."""
import json
import math

import numpy as np
import pytest

from oracle.hqt_oracle import sample_filtered
from tests import sampler_rows as SR
from tests.helpers import load

ROWSET_IDS = [f'V{V}-{name}' for V, name in SR.ROWSETS]


@pytest.mark.parametrize('variant', ['f32', 'split', 'bf16'])
@pytest.mark.parametrize('V,name', list(SR.ROWSETS), ids=ROWSET_IDS)
def test_injection_is_exact_on_the_oracle(V, name, variant):
    r_top, r_bot = SR.rows(V, name, variant)
    lg = SR.oracle_rows(V, name, variant, batch=2, n=2)
    assert lg.shape == (2, 5, 2, V)
    assert (lg[:, 0].view(np.uint32) == r_top.view(np.uint32)).all(), 'top head'
    assert (lg[:, 1:].view(np.uint32) == r_bot.view(np.uint32)).all(), 'bottom head'


def test_rows_are_what_their_family_says():
    for (V, name), (top, bot, _) in SR.ROWSETS.items():
        for fam in (top, bot):
            for variant in ('f32', 'split', 'bf16'):
                row = SR.row_of(V, fam, variant)
                assert row.shape == (V,) and row.dtype == np.float32
                s = np.sort(row)[::-1]
                if fam[0] == 'block':
                    assert (row == 0).sum() == fam[1] and (row[row != 0] == SR.ROUND[variant](SR.NEVER)).all() and row[0] == 0 and row[-1] == 0
                elif fam[0] == 'ulp':
                    k, gap = fam[1], fam[2]
                    a, b = (int(v) for v in s[[k - 1, k]].view(np.uint32))
                    assert a - b == SR.ULP[variant](gap)
                elif fam[0] == 'tierun':
                    k, at = fam[1], SR.tierun_indices(V)
                    assert len(set(row[at])) == 1 and s[k - 1] == row[0] and (row > row[0]).sum() <= k - 2 and (row == row[0]).sum() > len(at)
                    assert {0, V - 1} <= set(at) and all({m - 1, m} <= set(at) for m in (4, 64, 256, 1024) if m < V)
                elif fam[0] == 'quant':
                    assert (row * 4 == np.round(row * 4)).all() and len(np.unique(row)) < V // 2 + 60
    fx = load('g1_sampler.npz')                                            # the reference's own rows travel by the same injection: finite values only
    assert np.isfinite(fx['logits']).all() and fx['logits'].shape[1] % 4 == 0


def test_the_shortcut_is_sample_filtered():
    """ref_draws evaluates the reference's probabilities once per row; its codes are sample_filtered's on the broadcast rows."""
    for V, name, sn in [(100, 'hf', 'kp'), (1000, 'sq', 'p'), (3000, 'tg', 'kp'), (2048, 'bu', 'p-last')]:
        setting = dict(SR.ROWSETS[(V, name)][2])[sn]
        q = SR.draw_noise(V)
        for level, row in enumerate(SR.rows(V, name, 'f32')):
            T, k, p = SR.level_values(setting, level)
            qq = q[0, level]
            want = sample_filtered(np.broadcast_to(row, qq.shape), qq, T, k, p)[0]
            assert (SR.ref_draws(row, qq, T, k, p)[0] == want).all()


def test_block_rows_keep_the_lowest_indices():
    """m equal probabilities and top_p = j / m keep exactly the j lowest indices: the j-th prefix IS p, `cum >= p` holds from there on, and the shift by one
    spares that token itself (the reference's rule; order: probability descending, index ascending).  m = 3 * 2^a and p = fl32(j fl(1 / m)): the same."""
    for V in SR.VOCABS:
        if V > SR.TOP_P_MAX_V:
            continue
        m = SR.pow2_below(V)
        row = SR.row_of(V, ('block', m))
        zeros = np.flatnonzero(row == 0)
        for j in (1, m // 4, m - 1):
            kept = np.flatnonzero(SR.ref_probs(row, 1.0, None, j / m))
            assert (kept == zeros[:j]).all()
        assert (np.flatnonzero(SR.ref_probs(row, 1.0, None, 1.0)) == zeros).all()
        top, bot, settings = SR.ROWSETS[(V, 'b3')]
        m3 = top[1]
        c = np.float32(1.0) / np.float32(m3)
        for _, s in settings:
            for level, fam in enumerate((top, bot)):
                row = SR.row_of(V, fam)
                zeros = np.flatnonzero(row == 0)
                p = s['top_p'][level]
                j = int(round(p / float(c)))
                assert float(np.float32(np.float64(c) * j)) == p and 1 <= j < m3
                assert (np.flatnonzero(SR.ref_probs(row, 1.0, None, p)) == zeros[:j]).all()


@pytest.mark.parametrize('V,name', list(SR.ROWSETS), ids=ROWSET_IDS)
def test_probes_read_out_what_they_should(V, name):
    """Every probe pass fits its bounds, reads each token on its list at least once, and excludes no top-k and no block-row probe."""
    top, bot, settings = SR.ROWSETS[(V, name)]
    for sn, setting in settings:
        n, noise, want_t, want_b, ok_t, ok_b = SR.probe_case(V, name, 'f32', setting, SR.EPS_EXACT)
        assert 1 <= n <= 4 and noise.shape == (n, 5, SR.B, V) and noise.min() == SR.PROBE_Q and noise.max() == 1.0
        assert ((noise != 1.0).sum(-1) == 1).all()
        for s, members in SR.groups_of(setting):
            for level, (fam, ok) in enumerate(((top, ok_t), (bot, ok_b))):
                T, k, p = SR.level_values(s, level)
                if not p or (fam[0] in SR.EXACT_BLOCKS and math.log2(T).is_integer()):
                    assert ok[members].all(), (sn, level)
                assert ok[members].any(), (sn, level)


@pytest.mark.parametrize('V', SR.VOCABS)
def test_draws_are_well_conditioned(V):
    """The reference alone excludes at most 1 % of a case's random draws, on EXACT's rows and on SPLIT's."""
    worst = 0.0
    for v, name, sn in SR.draw_cases():
        if v != V:
            continue
        setting = dict(SR.ROWSETS[(V, name)][2])[sn]
        for variant in ('f32', 'split'):
            _, _, _, ok_t, ok_b = SR.draw_case(V, name, variant, setting, SR.EPS_EXACT)
            excluded = 1.0 - (ok_t.sum() + ok_b.sum()) / (ok_t.size + ok_b.size)
            worst = max(worst, excluded)
            assert excluded <= SR.MAX_EXCLUDED, (V, name, sn, variant, excluded)
    print(f'V = {V}: largest excluded share {worst:.4f}')


def test_the_table_reaches_every_path():
    classes, passes, g4, forms, settings_seen = set(), set(), set(), set(), set()
    for V, name, sn, setting in SR.all_cases():
        forms.add(SR.dispatch_form(setting, V))
        for s, _ in SR.groups_of(setting):
            for level, row in enumerate(SR.rows(V, name, 'f32')):
                T, k, p = SR.level_values(s, level)
                classes.add(SR.sort_class(row, T, k, p))
                passes.add(SR.radix_pass(row, T, k))
                settings_seen.add(('T', T))
                settings_seen.add(('p', p))
                settings_seen.add(('k', 'V//3' if k == V // 3 else 'V-1' if k == V - 1 else 'V' if k == V else 'V+1' if k == V + 1 else k if k in (1, 2) else None))
                if SR.is_plain(s, level, V):
                    g4.add(SR.plain_g4(V))
    assert {(NT, path) for NT in (256, 1024) for path in ('regs1', 'regs2', 'lds')} <= classes
    assert {2, 4, 8} <= g4                           # sampler_plain_fast_kernel<2>, <4> and <8> (<4>: 2048 < V <= 4096, here 3000 and 4096)
    assert forms == {'one', 'two'}
    assert {1, 2, 3, 4} <= passes                    # the k-th value parts from the masked ones in every pass: keys that agree in 0, 8, 16 and 24 bits
    assert {('T', t) for t in (0.5, 0.7, 1.0, 1.3)} <= settings_seen
    assert {('p', p) for p in (1e-6, 0.5, 0.9, 0.999, 1.0, None)} <= settings_seen
    assert {('k', k) for k in (1, 2, 'V//3', 'V-1', 'V', 'V+1', None)} <= settings_seen
    # the tie pairs: two strides of one thread, a lower index in a higher wave, at the vocabularies of both thread counts and of each plain kernel
    for V in SR.VOCABS:
        pairs = SR.tie_pairs(V)
        assert (0, 1) in pairs and (3, 4) in pairs and (0, V - 1) in pairs
        if V > 1024:
            assert (256, 1024) in pairs and (0, 1024) in pairs
        if V > 4096:
            assert (256, 4096) in pairs and (2, 4098) in pairs


def test_known_answer_fixture_is_usable():
    fx = load('g1_sampler.npz')
    cases = json.loads(str(fx['cases']))
    assert fx['logits'].shape == fx['noise'].shape == (6, 512) and len(cases) == 6
