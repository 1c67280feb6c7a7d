"""The draw report (hqt_set_draw_report, report_out= / return_report=, pipeline.uncertainty_map) without a GPU: the ABI surface, every refusal by name, the
map's layout against the reference's index tables, and the derived entropy gate held against a float32 emulation of the kernel's formula."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib
from hqtransformer_amd.engine import DrawReport, check_report_n, check_report_out, new_draw_report
from hqtransformer_amd.pipeline import InflightSampler, RollingSampler, SamplingSession, score_codes, uncertainty_map
from hqtransformer_amd.sampling import sampling_hqtransformer, sampling_ihqgpt
from hqtransformer_amd.spec import Stage2Spec
from tests import draw_report_ref as R
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    _lib.build()
    return _lib.load()


# ------------------------------------------------------------------------------- the ABI surface
def test_symbol_in_header_library_and_binding(lib):
    hdr = open(os.path.join(ROOT, 'include', 'hqt.h')).read()
    assert re.search(r'#define HQT_ABI_VERSION 9\b', hdr) and lib.hqt_abi_version() == 9 == _lib.ABI_VERSION
    assert re.search(r'#define HQT_REPORT_MAX_TOP 16\b', hdr) and _lib.REPORT_MAX_TOP == 16
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint hqt_set_draw_report\(hqt_handle\* h, const hqt_draw_report\* r\);', code)
    nm = subprocess.run(['nm', '-D', _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r'\bT hqt_set_draw_report\b', nm)
    assert _lib.SYMBOLS['hqt_set_draw_report'] == (C.c_int, [C.c_void_p, C.POINTER(_lib.hqt_draw_report)])
    assert C.sizeof(_lib.hqt_sample_opts) == 72


def test_struct_layout_matches_header():
    fields = ['entropy', 'rank', 'top_n', 'top_codes', 'top_logprobs']
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "hqt.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(hqt_draw_report));', '  printf("opts %zu\\n", sizeof(hqt_sample_opts));']
    lines += [f'  printf("{f} %zu\\n", offsetof(hqt_draw_report, {f}));' for f in fields] + ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'l.c'), os.path.join(d, 'l')
        open(src, 'w').write('\n'.join(lines))
        subprocess.run(['gcc', '-o', exe, src], check=True)
        want = dict(l.split() for l in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
    assert C.sizeof(_lib.hqt_draw_report) == int(want['size']) == 40 and int(want['opts']) == 72
    for f in fields:
        assert getattr(_lib.hqt_draw_report, f).offset == int(want[f]), f


def _struct(entropy=0, rank=0, top_n=0, top_codes=0, top_logprobs=0):
    r = _lib.hqt_draw_report()
    r.entropy, r.rank, r.top_n, r.top_codes, r.top_logprobs = entropy or None, rank or None, top_n, top_codes or None, top_logprobs or None
    return r


@pytest.mark.parametrize('kw,message', [
    (dict(entropy=64), 'null handle'),
    (dict(top_n=17, top_codes=64, top_logprobs=64), r'top_n=17 outside \[0, HQT_REPORT_MAX_TOP = 16\]'),
    (dict(top_n=-1), r'top_n=-1 outside'),
    (dict(top_n=4, top_logprobs=64), 'top_n=4 and top_codes is NULL'),
    (dict(top_n=4, top_codes=64), 'top_n=4 and top_logprobs is NULL'),
    (dict(entropy=64, top_codes=64), 'top_codes is set and top_n is 0'),
    (dict(entropy=64, top_logprobs=64), 'top_logprobs is set and top_n is 0')])
def test_the_library_refuses_by_name(lib, kw, message):
    """The struct is checked before the handle, so every refusal is reachable without a GPU (no handle exists here); the pointers are never read."""
    assert lib.hqt_set_draw_report(None, C.byref(_struct(**kw))) == -1          # HQT_ERR_INVALID
    assert re.search(message, lib.hqt_last_error().decode())
    assert lib.hqt_set_draw_report(None, None) == -1 and b'null handle' in lib.hqt_last_error()


# ------------------------------------------------------------------------------- the Python checks, before an engine exists
def test_check_report_n():
    assert check_report_n(None) is None and check_report_n(0) == 0 and check_report_n(16) == 16 and check_report_n(np.int64(3)) == 3
    for bad, message in ((17, r'N=17 outside \[0, 16\]'), (-1, 'outside'), (True, 'expected None or an integer'), (False, 'expected None or an integer'),
                         (2.0, 'expected None or an integer')):
        with pytest.raises(ValueError, match=message):
            check_report_n(bad)


def test_check_report_out():
    B, n, draws = 2, 3, 5
    good = new_draw_report(B, n, draws, 4, 'cpu')
    r, top_n = check_report_out(good, B, n, draws, 'cpu', 64)
    assert top_n == 4 and r.top_n == 4 and r.entropy == good.entropy.data_ptr() and r.top_logprobs == good.top_logprobs.data_ptr()
    assert good.top_codes.shape == (B, n, draws, 4) and good.rank.dtype == torch.int32 and bool(torch.isnan(good.entropy).all()) and int(good.rank.max()) == -1
    only = new_draw_report(B, n, draws, 0, 'cpu')
    assert only.top_codes is None and check_report_out(only, B, n, draws, 'cpu')[1] == 0
    assert check_report_out(None, B, n, draws) is None and check_report_out(DrawReport(None, None, None, None), B, n, draws) is None
    cases = [(good._replace(entropy=good.entropy.double()), r'report_out\.entropy: expected a contiguous torch\.float32 tensor of shape \(2, 3, 5\)'),
             (good._replace(rank=good.rank.long()), r'report_out\.rank: expected a contiguous torch\.int32'),
             (good._replace(entropy=good.entropy[:, :2]), r'report_out\.entropy: .*shape \(2, 3, 5\)'),
             (good._replace(rank=torch.zeros((B, n, 2 * draws), dtype=torch.int32)[:, :, ::2]), r'report_out\.rank: expected a contiguous'),
             (good._replace(top_logprobs=None), 'top_codes and top_logprobs come together'),
             (good._replace(top_logprobs=good.top_logprobs[..., :3].contiguous()), r'report_out\.top_logprobs: .*shape \(2, 3, 5, 4\)'),
             (new_draw_report(B, n, draws, 17, 'cpu'), r'N=17 alternatives outside \[1, 16\]'),
             (good._replace(top_codes=good.top_codes[0]), r'report_out\.top_codes: expected a tensor of shape'),
             ((1, 2, 3), 'expected an object with the fields')]
    for bad, message in cases:
        with pytest.raises(ValueError, match=message):
            check_report_out(bad, B, n, draws, 'cpu', 64)
    with pytest.raises(ValueError, match=r'N=4 alternatives, the vocabulary has 3 codes'):
        check_report_out(good, B, n, draws, 'cpu', 3)
    with pytest.raises(ValueError, match=r'report_out\.entropy: .* on cuda:0'):
        check_report_out(good, B, n, draws, 'cuda:0', 64)


def _model(levels=2, vocab=64, cond=1):
    """What the samplers read of a stage-2 model before they build an engine; ``engine`` raises: a test that gets there has not been refused in time."""
    spec = Stage2Spec(embed_dim=64, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=vocab, vocab_bot=vocab, vocab_txt=64, ctx_len_img=64, ctx_len_txt=16,
                      n_classes=10, cond=cond, embedding=0, **({'levels': 3} if levels == 3 else {}))

    def engine(*a, **k):
        raise AssertionError('an engine was asked for')
    return types.SimpleNamespace(spec=spec, use_txt_cond=cond == 2, use_cls_cond=cond == 1, engine=engine, _device=torch.device('cpu'))


def test_the_samplers_refuse_before_an_engine_is_built():
    m2, m3 = _model(), _model(levels=3)
    for call in (lambda **kw: sampling_ihqgpt(m2, 2, 1, max_seq_len=4, **kw), lambda **kw: sampling_hqtransformer(m3, 2, 1, max_seq_len=4, **kw),
                 lambda **kw: SamplingSession(m2, 2, 1, 4, **kw), lambda **kw: RollingSampler(m2, 2, 4, **kw)):
        with pytest.raises(ValueError, match=r'N=17 outside \[0, 16\]'):
            call(return_report=17)
        with pytest.raises(ValueError, match='expected None or an integer'):
            call(return_report=True)
    small = _model(vocab=8)
    with pytest.raises(ValueError, match=r'N=16 alternatives, the vocabulary has 8 codes'):
        sampling_ihqgpt(small, 2, 1, max_seq_len=4, return_report=16)
    codes = [torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 4, 4), dtype=torch.int64)]
    for one_pass in (False, True):
        with pytest.raises(ValueError, match=r'N=-2 outside'):
            score_codes(m2, codes, torch.tensor([1, 2]), one_pass=one_pass, report=-2)


def test_inflight_steps_merge_only_on_equal_n():
    model = types.SimpleNamespace(stage2=_model())
    s = InflightSampler.__new__(InflightSampler)
    s.model, s.merge, s.share_prompts, s.mixed_samplers, s.mixed_prefixes, s._queue = model, 4, False, False, False, []
    s.submit(2, 1, seed=1, return_report=3)
    s.submit(2, 2, seed=2, return_report=3)
    with pytest.raises(ValueError, match='steps merged into one pass must share'):
        s.submit(2, 3, seed=3, return_report=0)
    with pytest.raises(ValueError, match='steps merged into one pass must share'):
        s.submit(2, 3, seed=3)
    with pytest.raises(ValueError, match=r'N=40 outside'):
        s.submit(2, 3, seed=3, return_report=40)
    assert len(s._queue) == 2 and all(e.wants_report() for e in s._queue)


# ------------------------------------------------------------------------------- the map
def test_uncertainty_map_places_cells_where_the_decode_layout_places_codes():
    """The reference's index tables (G6): its sampler-layout codes [B, 64], [B, 64, 4] and the grids it decodes, [B, 8, 8] and [B, 16, 16].  A "report" whose
    entry (b, t, draw) IS the code of that draw must fold into exactly those grids."""
    fx = load('g6_index_maps.npz')
    top, bot = fx['codes_top'], fx['codes_bot']
    per_draw = torch.from_numpy(np.concatenate([top[:, :, None], bot], axis=2).astype(np.float32))
    maps = uncertainty_map(per_draw, 2)
    assert [tuple(m.shape) for m in maps] == [(2, 8, 8), (2, 16, 16)]
    assert (maps[0].numpy() == fx['grid_top']).all() and (maps[1].numpy() == fx['grid_bot']).all()
    # three levels: draws 5 .. 20 are the row-major 4 x 4 block of the position
    n, K = 4, 2
    e = torch.arange(2 * n * 21, dtype=torch.float32).reshape(2, n, 21)
    m0, m1, m2 = uncertainty_map(e, 3)
    assert m0.shape == (2, K, K) and m1.shape == (2, 2 * K, 2 * K) and m2.shape == (2, 4 * K, 4 * K)
    for t in range(n):
        Y, X = divmod(t, K)
        assert m0[1, Y, X] == e[1, t, 0]
        for s in range(4):
            assert m1[1, 2 * Y + s // 2, 2 * X + s % 2] == e[1, t, 1 + s]
        for s in range(16):
            assert m2[1, 4 * Y + s // 4, 4 * X + s % 4] == e[1, t, 5 + s]
    with pytest.raises(ValueError, match='expected'):
        uncertainty_map(torch.zeros((2, 4, 5)), 3)
    with pytest.raises(ValueError, match='square'):
        uncertainty_map(torch.zeros((2, 5, 5)), 2)


# ------------------------------------------------------------------------------- the reference itself, and the gate
def test_reference_order_and_rank():
    row = np.array([1.0, -0.0, 3.0, 0.0, 3.0, -5.0, 0.0, -0.0], np.float32)
    assert R.order(row).tolist() == [2, 4, 0, 1, 3, 6, 7, 5]
    assert [R.rank(row, c) for c in range(8)] == [2, 3, 0, 4, 1, 7, 5, 6]
    for V in (100, 4096):
        z = R.zeros_row(V)
        o = R.order(z)
        assert o[:10].tolist() == sorted(np.flatnonzero(z == 0).tolist())[:10] and np.signbit(z[o[0]]) and not np.signbit(z[o[1]])
        for name in R.FAMILIES:
            row = R.family_row(V, name)
            o = R.order(row)
            assert all(R.rank(row, int(o[j])) == j for j in (0, 1, 15, V - 1))
    const = R.family_row(1000, 'const')
    assert R.order(const)[:16].tolist() == list(range(16)) and R.rank(const, 777) == 777
    assert abs(R.entropy64(const) - np.log(1000)) < 1e-12 and abs(R.logprobs64(const)[5] + np.log(1000)) < 1e-12
    block = R.family_row(1000, 'block')
    assert abs(R.entropy64(block) - np.log(32)) < 1e-12


@pytest.mark.parametrize('V', R.VOCABS)
def test_entropy_gate_holds_a_quarter_for_the_float32_formula(V):
    """The derived 2e-4 gate: the kernel's formula, emulated in float32 in its reduction order, stays within a quarter of it on every injected family."""
    worst = {}
    for name in R.FAMILIES:
        row = R.family_row(V, name)
        worst[name] = abs(R.entropy32(row) - R.entropy64(row))
    print(f'V={V}: float32 entropy error per family: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert max(worst.values()) <= R.ENTROPY_GATE / 4, worst


def test_the_class_driver_refuses_a_bad_report_top(tmp_path):
    from hqtransformer_amd import sampling_hqmodel
    base = ['-r', str(tmp_path), '-m', 'nowhere.yaml']
    with pytest.raises(SystemExit, match=r'--report-top must lie in \[0, 16\]'):
        sampling_hqmodel.main(base + ['--report-top', '17'])
    with pytest.raises(SystemExit, match='not together with --complete-from or --canvas-grid'):
        sampling_hqmodel.main(base + ['--report-top', '4', '--canvas-grid', '12', '--canvas-stride', '2'])
    assert sampling_hqmodel.build_parser().parse_args(base).report_top is None
