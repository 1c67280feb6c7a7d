"""Per-row sampler settings (hqt_set_row_samplers), the parts that need no GPU: the ABI struct and symbol, the entry point's NULL-handle
refusal, and the pure functions that turn merged steps into the row table the library takes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hqtransformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    _lib.build()
    return _lib.load()


def test_row_sampler_struct_layout_matches_header():
    fields = ['temperature', 'top_k', 'top_p']
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "hqt.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(hqt_row_sampler));']
    lines += [f'  printf("{f} %zu\\n", offsetof(hqt_row_sampler, {f}));' for f in fields]
    lines += ['  printf("opts %zu\\n", sizeof(hqt_sample_opts));', '  printf("opts_l3 %zu\\n", sizeof(hqt_sample_opts_l3));',
              '  printf("abi %d\\n", HQT_ABI_VERSION);', '  return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'l.c'), os.path.join(d, 'l')
        with open(src, 'w') as fp:
            fp.write('\n'.join(lines))
        subprocess.run(['gcc', '-o', exe, src], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    want = {k: int(v) for k, v in (l.split() for l in out.strip().splitlines())}
    assert want['size'] == 36 and C.sizeof(_lib.hqt_row_sampler) == 36
    for f in fields:
        assert getattr(_lib.hqt_row_sampler, f).offset == want[f], f
    assert (want['temperature'], want['top_k'], want['top_p']) == (0, 12, 24)
    # the design adds an entry point: the option structs and the ABI version stay what they were
    assert want['opts'] == 72 and want['opts_l3'] == 88 and want['abi'] == 9
    assert _lib.ABI_VERSION == 9 and C.sizeof(_lib.hqt_sample_opts) == 72 and C.sizeof(_lib.hqt_sample_opts_l3) == 88


def test_symbol_is_exported_and_refuses_a_null_handle(lib):
    assert 'hqt_set_row_samplers' in _lib.exported_symbols()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert any(l.split()[-1] == 'hqt_set_row_samplers' for l in nm.splitlines() if l.strip())
    rows = (_lib.hqt_row_sampler * 2)()
    assert lib.hqt_set_row_samplers(None, 2, rows) == -1
    assert b'null' in lib.hqt_last_error()
    assert lib.hqt_set_row_samplers(None, 0, None) == -1       # clearing needs a handle too
    assert lib.hqt_abi_version() == 9


def _unpack(table):
    return table[:, 0:3].view(np.float32), table[:, 3:6].view(np.int32), table[:, 6:9].view(np.float32)


def test_steps_expand_to_rows_two_levels():
    from hqtransformer_amd.engine import row_sampler_table
    from hqtransformer_amd.pipeline import step_row_samplers
    sizes = [3, 1, 2]                                             # steps of unequal size
    kws = [dict(sample_offset=64),                                # sampler defaults: no cut-off, temperature 1
           dict(top_k_top=2048, top_k_bot=2048, top_p_top=None, top_p_bot=None, softmax_temperature=[0.95, 0.95]),
           dict(top_k_top=50, top_p_bot=0.9, softmax_temperature=[0.7, 1.3])]
    rows = step_row_samplers(2, sizes, kws)
    assert len(rows) == 6
    assert rows[0] == rows[1] == rows[2] == ((1.0, 1.0), (None, None), (None, None))
    assert rows[3] == ((0.95, 0.95), (2048, 2048), (None, None))
    assert rows[4] == rows[5] == ((0.7, 1.3), (50, None), (None, 0.9))
    table = row_sampler_table(2, rows)
    assert table.dtype == np.uint32 and table.shape == (6, 9) and table.flags['C_CONTIGUOUS'] and table.nbytes == 6 * 36
    t, k, p = _unpack(table)
    assert (t == np.float32([[1, 1, 1]] * 3 + [[0.95, 0.95, 1]] + [[0.7, 1.3, 1]] * 2)).all()
    assert (k == np.int32([[0, 0, 0]] * 3 + [[2048, 2048, 0]] + [[50, 0, 0]] * 2)).all()
    assert (p == np.float32([[0, 0, 0]] * 4 + [[0, 0.9, 0]] * 2)).all()
    # the ctypes view of the same memory
    arr = C.cast(table.ctypes.data_as(C.c_void_p), C.POINTER(_lib.hqt_row_sampler))
    assert arr[4].top_k[0] == 50 and abs(arr[4].top_p[1] - 0.9) < 1e-7 and abs(arr[3].temperature[1] - 0.95) < 1e-7 and arr[5].top_k[2] == 0


def test_steps_expand_to_rows_three_levels():
    from hqtransformer_amd.engine import row_sampler_table
    from hqtransformer_amd.pipeline import step_row_samplers
    rows = step_row_samplers(3, [2, 1], [dict(top_k=[100, None, 5], top_p=[0.9, None, None], softmax_temperature=[1.0, 0.9, 0.8]), dict()])
    assert rows == [((1.0, 0.9, 0.8), (100, None, 5), (0.9, None, None))] * 2 + [((1.0, 1.0, 1.0), (None,) * 3, (None,) * 3)]
    t, k, p = _unpack(row_sampler_table(3, rows))
    assert (t == np.float32([[1.0, 0.9, 0.8]] * 2 + [[1, 1, 1]])).all()
    assert (k == np.int32([[100, 0, 5]] * 2 + [[0, 0, 0]])).all()
    assert (p == np.float32([[0.9, 0, 0]] * 2 + [[0, 0, 0]])).all()
    # whole kinds of cut-off given as None, as the scalar arguments allow
    t, k, p = _unpack(row_sampler_table(3, [((0.5, 0.6, 0.7), None, None)]))
    assert (t == np.float32([[0.5, 0.6, 0.7]])).all() and not k.any() and not p.any()


def test_malformed_entries_are_refused():
    from hqtransformer_amd.engine import row_sampler_table
    from hqtransformer_amd.pipeline import step_row_samplers
    with pytest.raises(ValueError):
        row_sampler_table(2, [((1.0, 1.0, 1.0), (None, None), (None, None))])      # three temperatures for two levels
    with pytest.raises(ValueError):
        row_sampler_table(2, [((1.0, 1.0), (None, None))])
    with pytest.raises(ValueError):
        step_row_samplers(2, [1], [dict(softmax_temperature=[1.0, 1.0, 1.0])])


def test_mixed_queue_compares_everything_but_the_sampler_settings():
    """What `InflightSampler(mixed_samplers=True)` lets the steps of a pass differ in -- and nothing else."""
    from hqtransformer_amd.pipeline import SAMPLER_KEYS, Pending, _same, _Step

    def step(max_seq_len=64, **kw):
        return _Step(Pending(), 2, 3, 1, max_seq_len, True, None, True, True, None, True, kw)
    a, b = step(top_k_top=10, softmax_temperature=[1.0, 0.9]), step(top_p_bot=0.9, sample_offset=7)
    assert not _same(a.settings(), b.settings()) and _same(a.settings(True), b.settings(True))
    assert not _same(a.settings(True), step(max_seq_len=32).settings(True))
    assert not _same(a.settings(True), step(ar_precision='split').settings(True))
    assert set(SAMPLER_KEYS) == {'top_k_top', 'top_p_top', 'top_k_bot', 'top_p_bot', 'top_k', 'top_p', 'softmax_temperature'}
