"""The plan and the tile order of the merged-pass GEMMs (csrc/tile_plan.h) on the CPU: the header compiled ALONE by the host C++ compiler into a
stand-alone program.  tile_of is swept for holes and duplicates over every grid the kernels can be launched on; the plan of every GEMM of every case of
tests/merged_rows_cases.py is printed by the real function and held against what the case was written for; and every case runs through the oracle, so an
ill-conditioned draw is found here and never shows up as a failure of tests/test_gpu_merged_rows.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import merged_rows_cases as MR
from tests import offgrid_cases as OG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hqtransformer_amd', 'csrc')

MAIN = r'''
// argv: "sweep"               every TM in 1..130, TN in 1..64, S in {1, 2, 3, 4, 6, 8}: the ids 0 .. TM TN S - 1 through tile_of, each (slice, row tile, column
//                             tile) exactly once; prints the number of grids checked, exits 1 at the first hole or duplicate
//       "order TM TN S"       one line per workgroup id: slice, row tile, column tile
//       "M N K store dln"...  (groups of five) one line per group: geom bm bn S branch
#include "tile_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
static int sweep() {
    static const int SS[6] = {1, 2, 3, 4, 6, 8};
    long grids = 0;
    std::vector<unsigned char> seen;
    for (int TM = 1; TM <= 130; ++TM)
        for (int TN = 1; TN <= 64; ++TN)
            for (int S : SS) {
                const int total = TM * TN, n = total * S;
                seen.assign(n, 0);
                for (int b = 0; b < n; ++b) {
                    int z = -1, tm = -1, tn = -1;
                    tile_of(b, total, S, TM, TN, z, tm, tn);
                    if (z < 0 || z >= S || tm < 0 || tm >= TM || tn < 0 || tn >= TN) { printf("TM %d TN %d S %d: id %d -> (%d, %d, %d) outside the grid\n", TM, TN, S, b, z, tm, tn); return 1; }
                    unsigned char& s = seen[(z * TM + tm) * TN + tn];
                    if (s) { printf("TM %d TN %d S %d: id %d -> (%d, %d, %d) a second time\n", TM, TN, S, b, z, tm, tn); return 1; }
                    s = 1;
                }
                ++grids;                    // n ids, all inside, none twice: every tile once
            }
    printf("%ld\n", grids);
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 5 && !strcmp(argv[1], "order")) {
        const int TM = atoi(argv[2]), TN = atoi(argv[3]), S = atoi(argv[4]);
        for (int b = 0; b < TM * TN * S; ++b) {
            int z, tm, tn;
            tile_of(b, TM * TN, S, TM, TN, z, tm, tn);
            printf("%d %d %d\n", z, tm, tn);
        }
        return 0;
    }
    if (argc < 6 || (argc - 1) % 5) return 2;
    for (int i = 1; i < argc; i += 5) {
        const TilePlan p = tile_plan(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]) != 0);
        printf("%d %d %d %d %d\n", p.geom, p.bm, p.bn, p.S, p.branch);
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    """program(*argv) -> the lines the stand-alone program printed, as lists of ints."""
    d = tmp_path_factory.mktemp('tile_plan')
    src, exe = str(d / 'main.cpp'), str(d / 'tile_plan')
    open(src, 'w').write(MAIN)
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, '-o', exe, src], check=True)

    def run(*argv):
        r = subprocess.run([exe, *map(str, argv)], stdout=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stdout
        return [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    return run


@pytest.fixture(scope='module')
def plans(program):
    """{(case, gemm, phase): Plan} of the whole table and of the timed-schedule shapes, from ONE run of the real plan function."""
    keys, argv = [], []
    for name, launches in list(MR.all_launches().items()) + list(MR.timed_schedule_launches().items()):
        for (gemm, phase), (M, N, K, store, dln) in launches.items():
            keys.append((name, gemm, phase))
            argv += [M, N, K, MR.STORES[store], int(dln)]
    lines = program(*argv)
    assert len(lines) == len(keys)
    return {k: MR.Plan(*line) for k, line in zip(keys, lines)}


# ------------------------------------------------------------------------------- tile order
def test_tile_of_visits_every_tile_exactly_once(program):
    """TM 1..130 x TN 1..64 x S in {1, 2, 3, 4, 6, 8}: grids that are no multiple of 8 workgroups, fewer tiles than XCD groups, short last bands."""
    assert program('sweep') == [[130 * 64 * 6]]


@pytest.mark.parametrize('TM,TN,S,bands', [(13, 12, 3, [7, 6]), (26, 12, 1, [7, 7, 7, 5]), (26, 12, 6, [7, 7, 7, 5]), (13, 2, 1, [7, 6]), (21, 12, 1, [7, 7, 7]), (16, 8, 4, [8, 8]),
                                           (12, 5, 8, [12]), (11, 24, 2, [11]), (1, 1, 8, [1]), (130, 3, 1, [8] * 16 + [2])])
def test_tile_of_bands(program, TM, TN, S, bands):
    """The grouped order itself: every slice walks bands of the stated heights, each column by column, and an XCD gets a contiguous run of that walk.
    The walk of a slice is read off the ids alone: ids b, b + 8, ... follow each other within an XCD; with S | 8 slice z belongs to the XCDs z, z + S, ...,
    otherwise to the ids z TM TN .. (z + 1) TM TN - 1."""
    assert MR.bands(TM) == bands              # (the restatement the coverage test below uses to find launches with a short last band)
    order = [tuple(o) for o in program('order', TM, TN, S)]
    total = TM * TN
    want, first = [], 0
    for rows in bands:
        want += [(first + r, c) for c in range(TN) for r in range(rows)]
        first += rows
    assert first == TM and len(want) == total
    for z in range(S):
        if S > 1 and 8 % S == 0:
            ids = [b for x in range(z, 8, S) for b in range(x, total * S, 8)]
        else:
            ids = [z * total + i for x in range(8) for i in range(x, total, 8)]
        assert [order[b][0] for b in ids] == [z] * total, z
        assert [order[b][1:] for b in ids] == want, z


# ------------------------------------------------------------------------------- the plan of every case
def test_every_case_reaches_what_it_was_written_for(plans):
    """Per case: the (geometry, S) the real plan gives each GEMM at both row counts equals the table's record (tests/merged_rows_cases.py: EXPECTED_PLANS, what
    the GPU test asserts from the counters), and the property the case stands for holds."""
    for name in MR.CASES:
        got = {(g, ph): (p.geom, p.S) for (c, g, ph), p in plans.items() if c == name}
        print(name, {f'{g}@{ph}': v for (g, ph), v in got.items()})
        assert got == MR.EXPECTED_PLANS[name], name
    P = lambda c, g, ph: plans[(c, g, ph)]
    L = lambda c, g, ph: MR.all_launches()[c][(g, ph)]
    ragged = lambda c, g, ph: L(c, g, ph)[0] % P(c, g, ph).bm          # rows of the last row tile (0: full)
    row_tiles = lambda c, g, ph: -(-L(c, g, ph)[0] // P(c, g, ph).bm)
    # R1: body qkv on loader waves with a 10-row last tile; the k/v GEMM (N = 2 D) on 8-wave tiles with 11 ragged row tiles; fc2 split-K 8; 21 row tiles in depth
    assert P('R1', 'qkv', 'body').geom == MR.TG_128_PC and ragged('R1', 'qkv', 'body') == 10
    assert L('R1', 'kv', 'depth0')[1] == 2 * 1536 and P('R1', 'kv', 'depth0').geom == MR.TG_64X128_W8 and row_tiles('R1', 'kv', 'depth0') == 11 and ragged('R1', 'kv', 'depth0')
    assert P('R1', 'fc2', 'body').S == 8 and P('R1', 'fc2', 'depth0').S == 8
    assert row_tiles('R1', 'fc1', 'depth1') == 21 and L('R1', 'head', 'depth1')[1] == 8192 and ragged('R1', 'head', 'depth1')
    # R2: fc2 split-K 6 (non-XCD order); 26 row tiles in depth, bands 7, 7, 7, 5
    assert P('R2', 'fc2', 'body').S == 6 and row_tiles('R2', 'fc1', 'depth1') == 26 and MR.bands(26) == [7, 7, 7, 5]
    # R3: 13 row tiles in depth, bands 7 + 6; fc2 split-K 3; a streaming body
    assert P('R3', 'fc2', 'depth1').S == 3 and row_tiles('R3', 'fc2', 'depth1') == 13 and MR.bands(13) == [7, 6]
    assert L('R3', 'qkv', 'body')[0] == 415 and all(P('R3', g, 'body').geom < 0 for g in ('qkv', 'proj', 'fc1', 'fc2'))
    # R4: fc2 on 8-wave tiles through the t64 window; proj on 8-wave tiles
    assert P('R4', 'fc2', 'body').branch == MR.TB_WIDE_W8 and P('R4', 'proj', 'body').branch == MR.TB_NARROW_W8
    # R5: geometry 0 with S = 4 (tiles % 64 == 0); 16 row tiles, the last with 80 rows
    assert P('R5', 'fc2', 'depth1').branch == MR.TB_WIDE_S4 and P('R5', 'fc2', 'depth1').geom == MR.TG_128 and row_tiles('R5', 'fc2', 'depth1') == 16 and ragged('R5', 'fc2', 'depth1') == 80
    # R6: fc2 split-K 8 at N = 768 (the 256-thread combine at N < 1024); proj on 64 x 64 tiles with 21 ragged row tiles
    assert P('R6', 'fc2', 'depth1').S == 8 and L('R6', 'fc2', 'depth1')[1] == 768
    assert P('R6', 'proj', 'depth1').geom == MR.TG_64X64 and row_tiles('R6', 'proj', 'depth1') == 21 and ragged('R6', 'proj', 'depth1')
    # R7: split-K 2
    assert any(P('R7', 'fc2', ph).S == 2 for ph in ('body', 'depth0', 'depth1'))
    # R8: the 4-wave 64 x 128 geometry; geometry 0 at K = 256 (8 stages of 32 k); 13 row tiles of 64, bands 7 + 6
    assert any(p.geom == MR.TG_64X128 and row_tiles(c, g, ph) == 13 for (c, g, ph), p in plans.items() if c == 'R8')
    assert any(p.geom == MR.TG_128 and L(c, g, ph)[2] == 256 for (c, g, ph), p in plans.items() if c == 'R8')


def test_the_table_covers_every_geometry_slice_count_and_branch(plans):
    table = {k: p for k, p in plans.items() if k[0] in MR.CASES}
    launches = MR.all_launches()
    rows = lambda k: launches[k[0]][k[1:]][0]
    # every geometry with a ragged last row tile
    assert {p.geom for k, p in table.items() if p.geom >= 0 and rows(k) % p.bm} == set(range(MR.TG_COUNT))
    # every split-K factor
    assert {p.S for p in table.values() if p.geom >= 0} == {1, 2, 3, 4, 6, 8}
    # every way out of the plan function, counting the shapes tests/test_gpu_timed_schedule.py runs
    taken = {p.branch for p in plans.values()}
    assert taken == set(range(MR.TB_COUNT)), sorted(set(range(MR.TB_COUNT)) - taken)
    # a geometry-0 launch and a launch on 64-row tiles whose last band is shorter than the others
    short = lambda k, p: len(set(MR.bands(-(-rows(k) // p.bm)))) > 1
    assert any(p.geom == MR.TG_128 and short(k, p) for k, p in table.items())
    assert any(p.bm == 64 and p.geom >= 0 and short(k, p) for k, p in table.items())


# ------------------------------------------------------------------------------- the oracle on every case
@pytest.mark.parametrize('name', list(MR.CASES))
def test_oracle_runs_and_every_draw_is_well_conditioned(name):
    spec, weights, cond, noise, B, n = MR.inputs(name)
    ct, cb, lg, margin = MR.oracle(name)
    print(f'{name}: B={B} n={n} D={spec.embed_dim} V={spec.vocab_top}: margin {margin:.6f}, logit std {lg.std():.3f}, max |logit| {np.abs(lg).max():.2f}')
    assert ct.shape == (B, n) and cb.shape == (B, n, 4) and lg.shape == (n, 5, B, spec.vocab_top)
    assert margin >= OG.MIN_MARGIN, f'case {name}: the oracle\'s closest draw has margin {margin}: ill-conditioned for a bit-exact comparison, change its noise seed'
    assert np.isfinite(lg).all()
    assert 0 <= ct.min() and ct.max() < spec.vocab_top and 0 <= cb.min() and cb.max() < spec.vocab_top
