"""Stage 1 (HQ-VAE decode and encode) off the grid every other test sits on -- the case table of tests/offgrid_stage1_cases.py (checked on the CPU by
tests/test_offgrid_stage1_host.py) against the CPU oracle: EXACT and SPLIT pixels within 1e-4 on a NaN-poisoned workspace, FAST inside gates set at
about twice the measured error (profiles/offgrid_stage1_fast_gates.txt), the same bits run to run / alone or in a batch / wherever in the batch in all
three precisions, and the engine's own report of which kernel served each launch (profiles/offgrid_stage1_variants.txt) equal to what the restated
shape conditions predict.  M64 / M_A: the same at GroupNorm inputs whose group mean is 28 .. 58 standard deviations from zero."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.engine import Engine
from oracle import hqt_oracle as O
from tests import offgrid_stage1_cases as S1
from tests.helpers import _codebooks, _excess_distance, gate

pytestmark = pytest.mark.gpu
PIXEL_TOL = 1e-4
PRECISIONS = (('exact', PRECISION_EXACT), ('split', PRECISION_SPLIT), ('fast', PRECISION_FAST))
FAST_CAP = (0.1, 1e-2)             # the blanket bounds of the older decode tests: no gate below is wider
# FAST (bf16) max / mean absolute pixel error against the oracle: measured on the MI355X (comment), gate at about twice that
FAST_GATES = {
    'A': (0.058, 0.0094),          # 0.0289 / 0.00470
    'B': (0.061, 0.0100),          # 0.0304 / 0.00499
    'C': (0.056, 0.0098),          # 0.0282 / 0.00488
    'D': (0.076, 0.0100),          # 0.0382 / 0.00510
    'E': (0.062, 0.0100),          # 0.0312 / 0.00510
    'F': (0.055, 0.0095),          # 0.0275 / 0.00476
    'G': (0.100, 0.0100),          # 0.0511 / 0.00618
    'H': (0.054, 0.0083),          # 0.0272 / 0.00415
    'M64': (0.074, 0.0100),        # 0.0370 / 0.00628
    'M_A': (0.077, 0.0100),        # 0.0383 / 0.00782
}
# FAST encode: max |feature map - oracle| (about twice the measured 0.0365 / 0.0428 / 0.0323) and the share of top codes equal to the oracle's
# (measured 0.990 / 0.993 / 0.990; gated at the wide config's 0.95)
FAST_ENCODE_GATES = {'A': (0.073, 0.95), 'D': (0.086, 0.95), 'E': (0.065, 0.95)}
_ENGINES = {}


def np_(t):
    return t.detach().cpu().numpy()


def engine(name, encoder=False):
    """One engine per case (and one with the encoder), built on a NaN-poisoned workspace: whatever a kernel leaves unwritten shows up as NaN."""
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    key = (name, encoder)
    if key not in _ENGINES:
        spec, weights = S1.encode_inputs(name)[:2] if encoder else S1.inputs(name)[:2]
        os.environ['HQT_POISON_WORKSPACE'] = '1'
        try:
            e = Engine(None, spec, torch.device('cuda:0'), S1.N_IMAGES)
            e.load(stage1=weights)
            e.finalize()
        finally:
            del os.environ['HQT_POISON_WORKSPACE']
        _ENGINES[key] = e
    return _ENGINES[key]


def decode(eng, codes, **kw):
    t = [torch.from_numpy(np.ascontiguousarray(c)) for c in codes]
    return eng.decode3(t, **kw) if len(t) == 3 else eng.decode(t[0], t[1], **kw)


@pytest.mark.parametrize('name', list(S1.CASES))
def test_decode_vs_oracle(name):
    """EXACT and SPLIT within 1e-4 of the oracle (the large-mean cases included: SPLIT's one-pass statistics must not cancel), finite on the poisoned
    workspace, clamp01 = the oracle's postprocess; FAST inside its measured gate."""
    spec, weights, codes = S1.inputs(name)
    want = S1.want(name)
    eng = engine(name)
    got = {p: np_(decode(eng, codes, precision=prec)) for p, prec in PRECISIONS}
    err = {p: float(np.abs(g.astype(np.float64) - want).max()) if np.isfinite(g).all() else float('nan') for p, g in got.items()}
    d = np.abs(got['fast'] - want)
    print(f'DECODE {name}: exact {err["exact"]:.3e} split {err["split"]:.3e} fast max {d.max():.4f} mean {d.mean():.5f} (pixel std {want.std():.3f})')
    for p, g in got.items():
        assert g.shape == want.shape and np.isfinite(g).all(), p
    assert err['exact'] <= PIXEL_TOL, err
    assert err['split'] <= PIXEL_TOL, err
    cl = np_(decode(eng, codes, precision=PRECISION_SPLIT, clamp01=True))
    np.testing.assert_allclose(cl, O.postprocess(want), atol=PIXEL_TOL, rtol=0)
    gmax, gmean = FAST_GATES[name]
    assert gmax <= FAST_CAP[0] and gmean <= FAST_CAP[1]
    gate(f'offgrid_stage1.{name}.fast_pixels.max', d.max(), gmax)
    gate(f'offgrid_stage1.{name}.fast_pixels.mean', d.mean(), gmean)
    eng.range_check()


@pytest.mark.parametrize('name', list(S1.CASES))
def test_decode_bits_do_not_depend_on_run_batch_or_position(name):
    """Every reduction of the decoder is meant to run in a fixed order: three consecutive decodes are equal bit for bit, image 1 decoded alone equals
    image 1 of the batch, the flipped batch gives the flipped output -- in all three precisions, at widths whose GroupNorm passes are the generic ones."""
    codes = S1.inputs(name)[2]
    eng = engine(name)
    for p, prec in PRECISIONS:
        first = decode(eng, codes, precision=prec)
        for rep in range(2):
            again = decode(eng, codes, precision=prec)
            assert torch.equal(again, first), f'{name} {p}: decode {rep + 2} differs from the first in {int((again != first).sum())} values'
        one = decode(eng, [c[1:2] for c in codes], precision=prec)
        # FAST picks the halo-tile kernel by the rows of the whole chunk (big_tile_shape: a grid that fills the chip), so one image and three can
        # be served by different kernels -- case F's upsampling conv (2304 against 6912 rows) and conv_out are: its bf16 pixels then differ
        # (measured: 6911 of 6912 values, by up to 0.0067).  The identity is asserted wherever the predicted kernels are the same; DESIGN.md
        # lists the rest as an open property of FAST.
        if p != 'fast' or S1.variants(name, p, 1) == S1.variants(name, p):
            assert torch.equal(one[0], first[1]), f'{name} {p}: image 1 alone differs from image 1 of the batch in {int((one[0] != first[1]).sum())} values'
        else:
            print(f'BATCH {name} {p}: image 1 alone vs in the batch: max |diff| {float((one[0] - first[1]).abs().max()):.4f} (kernels differ: not asserted)')
        flipped = decode(eng, [c[::-1] for c in codes], precision=prec)
        assert torch.equal(flipped.flip(0), first), f'{name} {p}: the flipped batch differs in {int((flipped.flip(0) != first).sum())} values'


@pytest.mark.parametrize('name', list(S1.CASES))
def test_kernels_that_ran_are_the_predicted_ones(name):
    """One timed decode per precision: the `variant:*` slots of the timing report equal the prediction from the restated shape conditions
    (offgrid_stage1_cases.variants) -- so each case provably reaches the kernels it is in the table for."""
    codes = S1.inputs(name)[2]
    eng = engine(name)
    for p, prec in PRECISIONS:
        eng.timing(True)
        eng.timing_reset()
        decode(eng, codes, precision=prec)
        torch.cuda.synchronize()
        rep = {k: v[0] for k, v in eng.timing_report().items() if k.startswith('variant:') and v[0]}
        eng.timing(False)
        print(f'VARIANTS {name} {p} {json.dumps(rep, sort_keys=True)}')
        assert rep == S1.variants(name, p), (name, p)


@pytest.mark.parametrize('name', S1.ENCODE)
def test_encode_vs_oracle(name):
    """EXACT: quantiser input within 1e-4; codes equal the oracle's except at the oracle's own fp64 near-ties (gap <= 1e-4) and below a top code that
    differs, together at most 1 % of a level; decode(encode(x)) within 1e-4 of the oracle's decode of its codes for every image whose codes agree.
    FAST: every code is the nearest one for the device's own quantiser input; feature map and top-code agreement inside measured gates."""
    spec, weights, x, want = S1.encode_inputs(name)
    eng = engine(name, encoder=True)
    cbs = _codebooks(spec, weights)
    tx = torch.from_numpy(x)
    ex = eng.encode(tx, precision=PRECISION_EXACT, want_resid=True)
    herr = float(np.abs(np_(ex['resid'][0]) - want['resid'][0]).max())
    got = [np_(c) for c in ex['codes']]
    bad = [g != w for g, w in zip(got, want['codes'])]
    below = np.repeat(np.repeat(bad[0], 2, axis=1), 2, axis=2)                  # bottom codes under a top code that differs quantise another residual
    print(f'ENCODE {name}: exact feature map {herr:.3e}, codes differing {[int(b.sum()) for b in bad]} of {[b.size for b in bad]}')
    assert herr <= PIXEL_TOL, herr
    for l in range(2):
        tie = bad[l] & ~below if l else bad[l]
        if tie.any():
            assert _excess_distance(want['resid'][l], cbs[l], got[l])[tie.reshape(-1)].max() <= 1e-4, l
        assert bad[l].mean() <= 0.01, (l, bad[l].mean())
    same = [i for i in range(S1.N_IMAGES) if not any(b[i].any() for b in bad)]
    assert same, 'no image whose codes all agree with the oracle'
    rec = np_(eng.decode(ex['codes'][0], ex['codes'][1], precision=PRECISION_EXACT))
    ref = O.OracleStage1(spec, weights).decode_code(want['codes'][0][same], want['codes'][1][same])
    rerr = float(np.abs(rec[same] - ref).max())
    print(f'ENCODE {name}: decode(encode(x)) vs the oracle on images {same}: {rerr:.3e}')
    assert rerr <= PIXEL_TOL, rerr
    fa = eng.encode(tx, precision=PRECISION_FAST, want_resid=True)
    for l in range(2):
        assert _excess_distance(np_(fa['resid'][l]), cbs[l], np_(fa['codes'][l])).max() <= 1e-4, l
    ferr = float(np.abs(np_(fa['resid'][0]) - want['resid'][0]).max())
    agree = float(np.mean(np_(fa['codes'][0]) == want['codes'][0]))
    print(f'ENCODE {name}: fast feature map {ferr:.4f} (range {np.abs(want["resid"][0]).max():.2f}), top-code agreement {agree:.4f}')
    gate(f'offgrid_stage1.{name}.encode_fast_feature_map', ferr, FAST_ENCODE_GATES[name][0])
    gate(f'offgrid_stage1.{name}.encode_fast_code_agreement', agree, FAST_ENCODE_GATES[name][1], '>=')
    eng.range_check()
