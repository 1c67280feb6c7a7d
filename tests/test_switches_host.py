"""The library's environment switches (csrc/switches.h): one table, one reader, and documents and tools that name only what the table holds.  No GPU:
the parse rules and read times are checked on csrc/switches.hip compiled ALONE by the host C++ compiler into a stand-alone program."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hqtransformer_amd', 'csrc')
NAME = r'HQT_[A-Z0-9_]+'

# HQT_* names of tests/, tools/ and bench.py that are neither a switch of the library nor an identifier of include/hqt.h: variables the Python side reads ...
PYTHON_SIDE = ('HQT_RECORD_GATES', 'HQT_CPU_NO_AVX512')
PYTHON_SIDE_PREFIXES = ('HQT_BENCH_', 'HQT_REFERENCE', 'HQT_BPE16K_')
# ... and compile-time macros (`#ifdef` in csrc/, defined by the micro-benchmarks that include those sources): not read from the environment
COMPILE_TIME = ('HQT_TILE_STAMPS', 'HQT_SPLIT_GEMM_STAMPS')


def table():
    """The rows of SWITCH_TABLE: {variable: (parse kind, default, read time, effect, who flips it)}."""
    text = open(os.path.join(CSRC, 'switches.h')).read().replace('\\\n', ' ')
    rows = re.findall(rf'X\(\w+,\s*"({NAME})",\s*(SWP_\w+),\s*(-?\d+),\s*(SWR_\w+),\s*"([^"]+)",\s*"([^"]+)"\)', text)
    assert rows and len(rows) == len(re.findall(r'\bX\(\w+,\s*"', text)), 'a row of the table did not parse'
    out = {r[0]: (r[1], int(r[2]), r[3], r[4], r[5]) for r in rows}
    assert len(out) == len(rows), 'a variable stands in two rows'
    return out


def test_only_switches_hip_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and 'getenv' in open(os.path.join(CSRC, f), errors='replace').read()]
    assert readers == ['switches.hip'], readers
    from hqtransformer_amd import _lib
    assert 'switches.hip' in _lib.SOURCES


def test_design_lists_the_table():
    """DESIGN §7.1 has one table row per switch, with the read time the code has."""
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = re.search(r'^## 7\.1 .*?(?=^## )', design, re.S | re.M).group(0)
    listed = re.findall(rf'^\| `({NAME})` \| (once|live) \|', section, re.M)
    assert len(listed) == len(set(n for n, _ in listed)), 'a switch is listed twice'
    assert dict(listed) == {n: {'SWR_ONCE': 'once', 'SWR_LIVE': 'live'}[r[2]] for n, r in table().items()}
    assert set(re.findall(NAME, section)) >= set(table())


def test_tests_and_tools_name_known_switches_only():
    header = set(re.findall(NAME, open(os.path.join(ROOT, 'include', 'hqt.h')).read()))
    known = set(table()) | header | set(PYTHON_SIDE) | set(COMPILE_TIME)
    files = [os.path.join(ROOT, 'bench.py')]
    for top in ('tests', 'tools'):
        for d, dirs, names in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ('__pycache__', 'golden')]
            files += [os.path.join(d, n) for n in names]
    unknown = {}
    for f in files:
        try:
            text = open(f, encoding='utf-8').read()
        except UnicodeDecodeError:                      # a built micro-benchmark
            continue
        bad = {n for n in re.findall(NAME, text) if n not in known and not n.startswith(PYTHON_SIDE_PREFIXES)}
        if bad:
            unknown[os.path.relpath(f, ROOT)] = sorted(bad)
    assert not unknown, f'names that nothing reads: {unknown}'


MAIN = r'''
// argv: "NAME=value" sets a variable, "-NAME" unsets it, "NAME" prints switch_value of that switch
#include "switches.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
static const char* const VARS[SW_COUNT] = {
#define X(id, var, parse, dflt, read, effect, who) var,
    SWITCH_TABLE(X)
#undef X
};
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        char* a = argv[i];
        if (char* eq = strchr(a, '=')) { *eq = 0; setenv(a, eq + 1, 1); continue; }
        if (a[0] == '-') { unsetenv(a + 1); continue; }
        int s = 0;
        while (s < SW_COUNT && strcmp(VARS[s], a) != 0) ++s;
        if (s == SW_COUNT) { fprintf(stderr, "no switch %s\n", a); return 2; }
        printf("%d\n", switch_value(Switch(s)));
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def values(tmp_path_factory):
    """values(*argv) -> what the stand-alone program printed, started with no HQT_* variable set."""
    d = tmp_path_factory.mktemp('switches')
    src, exe = str(d / 'main.cpp'), str(d / 'switches')
    open(src, 'w').write(MAIN)
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, '-o', exe, '-x', 'c++', os.path.join(CSRC, 'switches.hip'), src], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith('HQT_')}

    def run(*argv):
        return [int(x) for x in subprocess.run([exe, *argv], env=env, check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    return run


def test_parse_kinds(values):
    rows = table()
    assert {r[0] for r in rows.values()} == {'SWP_PRESENT', 'SWP_ZERO_OFF', 'SWP_INT', 'SWP_INT_MIN1', 'SWP_INT_8_OR_16'}
    for name, (parse, dflt, *_rest) in rows.items():
        assert values(name) == [dflt], name                                 # unset: the row's default
        if parse == 'SWP_PRESENT':                                          # present = on, whatever the value
            assert dflt == 0 and values(f'{name}=0', name) == [1] and values(f'{name}=', name) == [1] and values(f'{name}=1', name) == [1], name
        elif parse == 'SWP_ZERO_OFF':                                       # off only when set and atoi gives 0
            assert dflt == 1 and values(f'{name}=0', name) == [0] and values(f'{name}=1', name) == [1] and values(f'{name}=off', name) == [0], name
    assert values('HQT_GRAPH_POSITIONS') == [16] and values('HQT_GRAPH_POSITIONS=0', 'HQT_GRAPH_POSITIONS') == [1]
    assert values('HQT_GRAPH_POSITIONS=5', 'HQT_GRAPH_POSITIONS') == [5] and values('HQT_GRAPH_POSITIONS=-3', 'HQT_GRAPH_POSITIONS') == [1]
    assert values('HQT_DEC_CHUNK') == [64] and values('HQT_DEC_CHUNK=0', 'HQT_DEC_CHUNK') == [0] and values('HQT_DEC_CHUNK=7', 'HQT_DEC_CHUNK') == [7]   # (the call site clamps)
    assert [values(f'HQT_HALO_TY={v}', 'HQT_HALO_TY') for v in ('8', '16', '12', '0', '', '32')] == [[8], [16], [0], [0], [0], [0]]
    assert values('HQT_HALO_TY') == [0]


def test_read_times(values):
    """A once switch keeps its first value after the variable changes, either way round; a live switch follows the variable."""
    other = {'SWP_PRESENT': '1', 'SWP_ZERO_OFF': '0', 'SWP_INT': '7', 'SWP_INT_MIN1': '5', 'SWP_INT_8_OR_16': '16'}
    for name, (parse, dflt, read, *_rest) in table().items():
        unset_first = values(name, f'{name}={other[parse]}', name, f'-{name}', name)
        set_first = values(f'{name}={other[parse]}', name, f'-{name}', name, f'{name}={other[parse]}', name)
        on = int(other[parse])
        if read == 'SWR_ONCE':
            assert unset_first == [dflt] * 3 and set_first == [on] * 3, name
        else:
            assert unset_first == [dflt, on, dflt] and set_first == [on, dflt, on], name
    assert table()['HQT_FORCE_TILE128'][2] == 'SWR_LIVE'            # tests flip it in-process (tests/test_gpu_parity.py)
