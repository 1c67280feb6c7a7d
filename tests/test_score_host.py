"""One-pass scoring (hqt_score): what can be checked without a GPU -- the binding table, argument validation before any engine is built, the
global <-> sampler layout maps, and the G15 fixtures pinned to the CPU oracle."""
import os
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.engine import check_score_codes
from hqtransformer_amd.models import ImageGPT2
from hqtransformer_amd.pipeline import grids_to_sequences, score_codes
from hqtransformer_amd.sampling import check_forward_codes, global_to_sequence_index, rearrange_levels
from hqtransformer_amd.spec import Stage2Spec
from tests.helpers import load
from tests.score_ref import G15, LOGPROB_TOL, g15, g15_noise, log_softmax_at, oracle_free_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spec_of(**kw):
    base = dict(embed_dim=128, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=64, ctx_len_txt=16,
                n_classes=10, cond=1, embedding=0)
    base.update(kw)
    return Stage2Spec(**base)


def stage2_stub(spec):
    """What score_codes touches before it builds an engine; engine() must not be reached."""
    def engine(*a, **k):
        raise AssertionError('an engine was built before the arguments were validated')
    return types.SimpleNamespace(spec=spec, use_cls_cond=spec.cond == 1, use_txt_cond=spec.cond == 2, engine=engine)


def test_binding_table_and_header_hold_both_symbols():
    assert 'hqt_score' in _lib.SYMBOLS and 'hqt_set_score_chunk' in _lib.SYMBOLS
    assert len(_lib.SYMBOLS['hqt_score'][1]) == 9 and len(_lib.SYMBOLS['hqt_set_score_chunk'][1]) == 2
    with open(os.path.join(ROOT, 'include', 'hqt.h')) as fp:
        header = fp.read()
    assert 'int hqt_score(hqt_handle* h, int B, const int64_t* cond, const int64_t* const* codes, int n, int precision, float* logprobs,' in header
    assert 'int hqt_set_score_chunk(hqt_handle* h, int pairs);' in header
    assert _lib.ABI_VERSION == 9 and '#define HQT_ABI_VERSION 9' in header


def test_one_pass_validation_raises_before_any_engine_is_built():
    spec = spec_of()
    top, bot = torch.zeros((2, 9), dtype=torch.int64), torch.zeros((2, 9, 4), dtype=torch.int64)
    st = stage2_stub(spec)
    with pytest.raises(ValueError, match=r'codes\[1\]: expected shape \(2, 9, 4\)'):
        score_codes(st, [top, bot[:, :8]], 3, one_pass=True)
    with pytest.raises(ValueError, match=r'codes\[1\]: expected shape'):
        score_codes(st, [top, bot.reshape(2, 36)], 3, one_pass=True)
    with pytest.raises(ValueError, match='code levels as one list'):
        score_codes(st, [top], 3, one_pass=True)
    with pytest.raises(ValueError, match='integer codes'):
        score_codes(st, [top, bot.float()], 3, one_pass=True)
    with pytest.raises(IndexError, match=r'codes\[1\]: index out of range'):
        score_codes(st, [top, bot + 512], 3, one_pass=True)
    with pytest.raises(ValueError, match='ctx_len_img'):
        check_score_codes(spec, [torch.zeros((1, 65), dtype=torch.int64), torch.zeros((1, 65, 4), dtype=torch.int64)])
    l3 = [top, bot, torch.zeros((2, 9, 16), dtype=torch.int64)]
    with pytest.raises(ValueError, match='one_pass=False'):
        score_codes(stage2_stub(spec_of(levels=3, depth_decoding='top2mid2bot')), l3, 3, one_pass=True)
    with pytest.raises(ValueError, match='three code levels'):
        score_codes(stage2_stub(spec_of(levels=3, cond=2)), l3, torch.zeros((2, 16), dtype=torch.int64), one_pass=True)
    # the stepwise default still refuses the bidirectional head, and now names the way out
    with pytest.raises(ValueError, match='one_pass=True'):
        score_codes(stage2_stub(spec_of(depth_decoding='bidirectional')), [top, bot], 3)
    assert check_score_codes(spec_of(depth_decoding='bidirectional'), [top, bot]) == 9


def test_forward_validation_raises_before_any_engine_is_built():
    spec = spec_of()
    model = ImageGPT2.__new__(ImageGPT2)
    model.stage2 = stage2_stub(spec)
    top = torch.zeros((2, 16), dtype=torch.int64)
    with pytest.raises(ValueError, match='not a square'):
        model.forward((torch.zeros((2, 12), dtype=torch.int64), torch.zeros((2, 48), dtype=torch.int64)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'codes\[1\]: expected shape \(2, 64\)'):
        model.forward((top, torch.zeros((2, 16, 4), dtype=torch.int64)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='two-level'):
        check_forward_codes(spec_of(levels=3), (top, torch.zeros((2, 64), dtype=torch.int64)))
    model.stage2 = stage2_stub(spec_of(cond=2))
    with pytest.raises(NotImplementedError, match='logits_txt.*head_txt'):
        model.forward((top, torch.zeros((2, 64), dtype=torch.int64)), torch.zeros((2, 16), dtype=torch.int64))


def test_layout_maps_agree_with_the_reference_index_maps():
    fx = load('g6_index_maps.npz')
    seq_bot, grid_bot = fx['codes_bot'], fx['grid_bot']                  # [2, 64, 4] and the reference's [2, 16, 16] grid of it
    idx = global_to_sequence_index(64).numpy()
    assert idx.shape == (64, 4) and sorted(idx.reshape(-1).tolist()) == list(range(256))
    glob = grid_bot.reshape(2, -1)                                       # 'B (H H2 W W2)'
    assert (glob[:, idx.reshape(-1)].reshape(2, 64, 4) == seq_bot).all()
    back = np.empty_like(glob)
    back[:, idx.reshape(-1)] = seq_bot.reshape(2, -1)
    assert (back == glob).all()
    seqs = grids_to_sequences([torch.from_numpy(fx['grid_top']), torch.from_numpy(grid_bot)])
    assert (seqs[0].numpy() == fx['codes_top']).all() and (seqs[1].numpy() == seq_bot).all()
    # level 2: a row-major 4 x 4 block per top position, the inverse of rearrange_levels
    i2 = global_to_sequence_index(4, 2)
    grid = torch.arange(64).reshape(1, 8, 8)
    assert torch.equal(rearrange_levels([torch.zeros((1, 4)), torch.zeros((1, 4, 4)), grid.reshape(1, -1)[:, i2.reshape(-1)].reshape(1, 4, 16)], 2)[2], grid)
    with pytest.raises(ValueError, match='square'):
        global_to_sequence_index(12)


@pytest.mark.parametrize('name', G15)
def test_fixture_is_pinned_to_the_oracle(name):
    """The oracle's free run under the recorded noise draws the fixture's codes bit for bit, and the log-softmax of its stepwise logits is the
    fixture's forward-pass ``logprob`` within 4e-4 (every position is recorded); the kept logits agree within 2e-4."""
    fx, spec, weights, cond, codes = g15(name)
    n = int(fx['n_steps'])
    assert float(fx['forward_vs_stepwise']) < 1e-4 and float(fx['margin']) > 1.0
    got, lg = oracle_free_run(spec, weights, cond, n, g15_noise(fx, spec))
    for l, (a, b) in enumerate(zip(got, codes)):
        assert (a == b).all(), f'{name}: level {l} codes differ from the reference run at {int((a != b).sum())} places'
    err = np.abs(log_softmax_at(lg, codes) - fx['logprob']).max()
    top = np.abs(lg[:, 0].transpose(1, 0, 2) - fx['logits_top']).max()
    print(f'{name}: oracle vs forward: logprob {err:.2e}, top logits {top:.2e}')
    assert err <= LOGPROB_TOL and top <= 2e-4
    keep, first = fx['keep_steps'], 1
    for l in range(1, spec.levels):
        rows = lg[keep][:, first:first + 4 ** l].transpose(2, 0, 1, 3)          # [B, keep, 4 ** l, V]
        assert np.abs(rows - fx[f'logits{l}']).max() <= 2e-4
        first += 4 ** l
