"""Log-probabilities of sampled codes (hqt_set_logprob_out), the parts that need no GPU: the symbol and its NULL-handle refusal, the fp64 sequence
score, the ranking helper of sample_best_of, score_codes' refusal of the bidirectional head and the --best-of flag of the text-to-image driver."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.config import load_config
from hqtransformer_amd.spec import stage2_spec_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    _lib.build()
    return _lib.load()


def test_symbol_is_exported_and_refuses_a_null_handle(lib):
    assert 'hqt_set_logprob_out' in _lib.exported_symbols()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert any(l.split()[-1] == 'hqt_set_logprob_out' for l in nm.splitlines() if l.strip())
    buf = (C.c_float * 8)()
    assert lib.hqt_set_logprob_out(None, C.cast(buf, C.c_void_p)) == -1          # HQT_ERR_INVALID
    assert b'null' in lib.hqt_last_error()
    assert lib.hqt_set_logprob_out(None, None) == -1                             # clearing needs a handle too
    # an entry point only: the option structs and the ABI version stay what they were
    assert lib.hqt_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert C.sizeof(_lib.hqt_sample_opts) == 72 and C.sizeof(_lib.hqt_sample_opts_l3) == 88


def test_sequence_logprob_sums_in_fp64_and_propagates_nan():
    from hqtransformer_amd.pipeline import sequence_logprob
    # 2^24 + 1 + 1 ...: an fp32 accumulator drops every 1 behind the large term, an fp64 one keeps them
    lp = torch.zeros((3, 4, 5), dtype=torch.float32)
    lp[0, 0, 0] = -float(2 ** 24)
    lp[0, 1:, :] = -1.0
    lp[1] = -0.5
    lp[2] = -0.25
    lp[2, 3, 4] = float('nan')
    got = sequence_logprob(lp)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,)
    assert got[0].item() == -(2.0 ** 24 + 15.0)
    assert got[1].item() == -10.0
    assert np.isnan(got[2].item())                           # a half-scored sequence has no score
    assert sequence_logprob(lp[2:, :3]).item() == -0.25 * 15  # ... until the unscored positions are sliced away
    with pytest.raises(ValueError):
        sequence_logprob(lp[0])


def test_ranking_breaks_ties_to_the_lower_index():
    from hqtransformer_amd.pipeline import rank_candidates
    scores = torch.tensor([[-3.0, -1.0, -1.0, -2.0, -1.0, -5.0],
                           [-7.0, -7.0, -7.0, -7.0, -7.0, -7.0]], dtype=torch.float64)
    idx = rank_candidates(scores, 4)
    assert idx.dtype == torch.int64 and idx.tolist() == [[1, 2, 4, 3], [0, 1, 2, 3]]
    assert rank_candidates(scores, 1).tolist() == [[1], [0]]
    # what a host-side stable argsort of the negated scores picks
    want = np.argsort(-scores.numpy(), axis=1, kind='stable')[:, :6]
    assert (rank_candidates(scores, 6).numpy() == want).all()
    for keep in (0, 7):
        with pytest.raises(ValueError):
            rank_candidates(scores, keep)


def test_score_codes_refuses_the_bidirectional_head_before_an_engine_is_built():
    from hqtransformer_amd.pipeline import score_codes
    spec = stage2_spec_from_config(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml'), ['stage2.type=hq-transformer/bidirectional4']))

    def no_engine(*a, **k):
        raise AssertionError('the refusal must come before any engine is built')
    stage2 = types.SimpleNamespace(spec=spec, use_txt_cond=False, use_cls_cond=True, engine=no_engine)
    codes = [torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 4, 4), dtype=torch.int64)]
    with pytest.raises(ValueError, match='bidirectional'):
        score_codes(stage2, codes, 3)


def test_best_of_flag_parses_and_rejects_less_than_one(capsys):
    from hqtransformer_amd.sampling_hqmodel_txt2img import build_parser
    base = ['-r', 'out', '-m', 'model.yaml']
    assert build_parser().parse_args(base).best_of == 1
    assert build_parser().parse_args(base + ['--best-of', '4']).best_of == 4
    for bad in ('0', '-2'):
        with pytest.raises(SystemExit) as e:
            build_parser().parse_args(base + ['--best-of', bad])
        assert e.value.code == 2
    assert '--best-of' in capsys.readouterr().err
