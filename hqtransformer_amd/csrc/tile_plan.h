// The tiled MFMA GEMM of the merged AR passes (tile_gemm.hip): its tile geometries, the plan -- which geometry and split-K factor a shape gets --
// and the order in which the workgroups of a launch walk the tiles.
//
// Plain C++, no HIP header: tile_gemm.hip includes this file, and a host compiler builds it alone -- that is how tests/test_tile_plan_host.py
// sweeps tile_of for holes and duplicates and prints the plan of any shape.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TILE_PLAN_HD __host__ __device__
#else
#define TILE_PLAN_HD
#endif

// NLOAD_ > 0 (round 6): NLOAD_ further waves do nothing but the LDS-DMA of the ring (loader waves), the WGM x WGN waves only read fragments and
// multiply: a `buffer_load ... lds` piece costs its wave 60 .. 180 ISSUE cycles (the texture path takes 64 B/clk), and a wave issues in order -- in the
// all-consumer form every stage opens with CPW such pieces in front of the matrix instructions of the wave that issues them.
template <int WGM_, int WGN_, int MBW_, int NT_, int KU_, int NSTAGE_, int NLOAD_ = 0>
struct TileGeom {
    static constexpr int WGM = WGM_, WGN = WGN_, MBW = MBW_, NT = NT_, KU = KU_, NSTAGE = NSTAGE_, NLOAD = NLOAD_;
    static constexpr int NC = WGM * WGN;                       // consumer waves (wave tile (32 MBW) x (32 NT))
    static constexpr int NW = NC + NLOAD;                      // waves per workgroup
    static constexpr int NDMA = NLOAD ? NLOAD : NC;            // waves that issue the ring's DMA
    static constexpr int BM = 32 * MBW * WGM, BN = 32 * NT * WGN;
    static constexpr int ACH = BM / 32, WCH = BN / 32;         // 1-KiB fragments per k-step
    static constexpr int CPS = ACH + WCH;
    static constexpr int CH_STAGE = KU * CPS;
    static constexpr int CPW = CH_STAGE / NDMA;                // LDS-DMA instructions per issuing wave per stage
    static constexpr int STAGE_BYTES = CH_STAGE * 1024;
    static constexpr int RING_BYTES = NSTAGE * STAGE_BYTES;
    static constexpr int GR = NC * 64 / BM;                    // threads per row in the statistics prologue (consumer waves)
    // after the ring: (mean, rstd) per row, (bias, colsum) per column, prologue scratch
    static constexpr int AUX_BYTES = BM * 8 + BN * 8 + GR * BM * 8;
    static constexpr int LDS_BYTES = RING_BYTES + AUX_BYTES;
    static constexpr int WG_PER_CU = NW == 4 ? (160 * 1024 / LDS_BYTES < 4 ? 160 * 1024 / LDS_BYTES : 4) : (LDS_BYTES <= 80 * 1024 ? 2 : 1);   // by LDS; 4-wave workgroups up to 4 per CU
    static_assert(CH_STAGE % NDMA == 0, "every issuing wave issues the same number of DMA pieces per stage");
    static_assert(NC * 64 % BM == 0 && GR >= 1, "statistics prologue: whole thread groups per row");
    static_assert(WGN * BM * 8 <= RING_BYTES, "residual epilogue: per-wave partial statistics fit the dead ring");
};

// 128 x 128, 4 waves of 64 x 64, 3 stages of 32 k: 48 KiB ring, THREE workgroups per CU.  What the shapes of the AR loop want
// (tools/micro/bench_tile, in-kernel stamps): a workgroup spends about half of its life outside the main loop (ring fill,
// epilogue stores at ~10 B/clk/CU, slot turnover), so throughput comes from co-resident workgroups covering each other --
// with three per CU the matrix pipe is busy 93 % of a main loop.  256 x 256 (one per CU, 71 % busy loop, 20 us of exposed
// prologue + epilogue per 32 us loop) and 256 x 128 tiles measured 5-30 % slower in the dependent chain of the AR loop
// at 512 .. 5120 rows (profiles/r03_micro_tile_gemm.txt); they live on in tools/micro/bench_tile.hip.
typedef TileGeom<2, 2, 2, 2, 2, 3> Tile128;
// 64 x 128, 4 waves of 32 x 64, 36 KiB ring, FOUR workgroups per CU: the 512-row passes.  A 512 x 6144 output is only 192 tiles of
// 128 x 128 (qkv: 144) -- fewer workgroups than the chip has CUs, each walking K alone on its CU at the latency-bound pace of a single
// ring; halving the row tile doubles the workgroups for 1.5x the LDS-DMA bytes per FLOP, which these shapes have to spare.
typedef TileGeom<2, 2, 1, 2, 2, 3> Tile64;
// 64 x 128 with EIGHT waves (32 x 32 each), stages of 64 k (24 KiB), two workgroups per CU: launches of about one workgroup per CU
// (640-row passes: 360 tiles).  In-kernel stamps put a lone 4-wave workgroup's stage at ~650 cycles against 128-256 of MFMA work whatever
// the ring depth (6 stages in flight instead of 2 measured within 1 %: profiles/r04_tile_variants.txt) -- what paces it is the ISSUE of its
// LDS-DMA pieces, ~150 cycles per 1-KiB piece and wave; eight waves issue the same pieces twice as fast.
typedef TileGeom<2, 4, 1, 1, 4, 3> Tile64W8;
// 128 x 128 with FOUR loader waves beside the four multiplying waves (round 6): 4 stages of 32 k (64 KiB ring, two workgroups per CU)
typedef TileGeom<2, 2, 2, 2, 2, 4, 4> Tile128PC;
typedef TileGeom<2, 2, 1, 1, 4, 3> Tile64x64;     // 64 x 64, 4 waves of 32 x 32, stages of 64 k: 48 KiB ring, three workgroups per CU (proj at 640 rows: tile_plan)

// geom: TG_*, < 0: the shape is not the tile kernels'; S: split-K factor; branch: the TB_* decision of tile_plan that made the plan
struct TilePlan { int geom; int bm, bn; int S; int branch; };
enum { TG_128 = 0, TG_64X128 = 1, TG_64X128_W8 = 2, TG_64X64 = 3, TG_128_PC = 4, TG_COUNT = 5 };
// the store modes the plan tells apart (the STORE_* values of common.h: tile_gemm.hip asserts that they are)
enum { TPS_ROWS = 0, TPS_QKV = 2, TPS_PACKED = 3, TPS_RESID = 4 };
// one per way out of tile_plan, in source order
enum { TB_NOT_TAKEN = 0, TB_NARROW_64X64, TB_LOADERS, TB_W8, TB_W4, TB_NARROW_W8, TB_WIDE_LOADERS, TB_WIDE_W8, TB_WIDE_S4_LOADERS, TB_WIDE_S4, TB_WIDE_LARGEST_S,
       TB_PLAIN, TB_COUNT };
// the suffix of a launch's `variant:tile_gemm_<bm>x<bn>` counter: the geometries that share a tile size with another one
TILE_PLAN_HD inline const char* tile_geom_suffix(int geom) { return geom == TG_128_PC ? "pc" : (geom == TG_64X128_W8 ? "w8" : ""); }

// What of tile_gemm_ok depends on the shape alone: 512+ rows, whole 128-column tiles, k-steps divisible into stages; the narrow residual producer
// (proj, K = D: one short K loop over 48 column-tile rows.  Below 640 rows the streaming kernel's 64-row tiles win (23.5 vs 25.2 us at 512 rows); from 640
// rows the 8-wave 64 x 128 tiles do (27.8 -> 24.9 us at 640, 30.0 -> 26.8 at 768, 37.5 -> 29.3 at 1024)); a residual producer never normalises its operand.
TILE_PLAN_HD inline bool tile_shape_ok(int M, int N, int K, int store, bool dln) {
    if (M < 512 || N % 128 != 0 || K % 32 != 0 || K < 256) return false;
    if (store == TPS_RESID) return !dln && (K >= 3072 || M >= 640);
    return store == TPS_QKV || store == TPS_PACKED || store == TPS_ROWS;
}

// Split-K factor: only the residual producers with a long K (fc2: K = 4 D) whose tiles would leave most of the 768 resident
// slots empty; the slices leave fp32 slabs that resid_combine_kernel finishes (one extra launch: not worth it at K = D).
TILE_PLAN_HD inline TilePlan tile_plan(int M, int N, int K, int store, bool dln) {
    constexpr int max_s = 8;
    if (!tile_shape_ok(M, N, K, store, dln)) return TilePlan{-1, 0, 0, 1, TB_NOT_TAKEN};
    TilePlan p{TG_128, Tile128::BM, Tile128::BN, 1, TB_PLAIN};
    const int KS = K / 16, tiles = ((M + p.bm - 1) / p.bm) * (N / p.bn);
    // the narrow residual producer (proj: N = K = D) at the driver's 640 rows: 240 tiles of 64 x 64 (4 waves, three workgroups per CU) instead of 120 of 64 x 128 --
    // every CU gets one, half the matrix work per workgroup: 18.9 -> 16.5 ms per pass (1024 rows: 384 such tiles lose to 192 of 64 x 128, 21.4 vs 19.4)
    if (store == TPS_RESID && K < 3072 && ((M + 63) / 64) * (N / 64) <= 256 && KS % Tile64x64::KU == 0 && KS / Tile64x64::KU >= 2 * Tile64x64::NSTAGE)
        return TilePlan{TG_64X64, 64, 64, 1, TB_NARROW_64X64};
    // one round of 128 x 128 tiles that fills most of the chip (640 rows: qkv 180, fc1 240 tiles): the loader-wave geometry -- in-kernel stamps at 640 rows
    // (profiles/r06_micro_tile_gemm.txt): main loop 18.4 k cycles against 28.9 k for the all-consumer 128 x 128 tile, workgroup life 13.5-14 us against the
    // 8-wave 64 x 128 tiles' grid span of 16.5-17 us (360 / 480 workgroups: two rounds on part of the chip)
    if (store != TPS_RESID && tiles >= 160 && tiles <= 256 && KS % Tile128PC::KU == 0 && KS / Tile128PC::KU >= 2 * Tile128PC::NSTAGE)
        return TilePlan{TG_128_PC, Tile128PC::BM, Tile128PC::BN, 1, TB_LOADERS};
    if (store != TPS_RESID && tiles < 256 && KS / Tile64::KU >= Tile64::NSTAGE) {
        const int t64 = ((M + Tile64::BM - 1) / Tile64::BM) * (N / Tile64::BN);
        if (t64 <= 512 && KS % Tile64W8::KU == 0 && KS / Tile64W8::KU >= 2 * Tile64W8::NSTAGE) return TilePlan{TG_64X128_W8, Tile64::BM, Tile64::BN, 1, TB_W8};
        return TilePlan{TG_64X128, Tile64::BM, Tile64::BN, 1, TB_W4};
    }
    if (store == TPS_RESID && K < 3072 && tiles < 256 && KS % Tile64W8::KU == 0 && KS / Tile64W8::KU >= 2 * Tile64W8::NSTAGE)
        return TilePlan{TG_64X128_W8, Tile64::BM, Tile64::BN, 1, TB_NARROW_W8};
    // the wide-K residual producer when its 128 x 128 tiles are ONE round over most of the chip (fc2 at 2560 rows: 240 tiles): the loader-wave geometry without split-K --
    // grid span 46 us against 60-69 for 480 tiles of 64 x 128 (profiles/r06_micro_tile_gemm.txt: main loop 73 k cycles against 115 k for the all-consumer 128 x 128 tile)
    if (store == TPS_RESID && K >= 3072 && tiles >= 160 && tiles <= 256 && KS % Tile128PC::KU == 0 && KS / Tile128PC::KU >= 2 * Tile128PC::NSTAGE)
        return TilePlan{TG_128_PC, Tile128PC::BM, Tile128PC::BN, 1, TB_WIDE_LOADERS};
    if (store == TPS_RESID && K >= 3072 && tiles < 256) {
        // The wide-K residual producer (fc2).  Measured per (geometry, S) at the row counts the schedules produce (profiles/r04_fc2_plans.txt; GEMM + combine,
        // ms per pass): what counts is whole ROUNDS of workgroups (128 x 128: one per CU, 8-wave 64 x 128: two) and the slab traffic of the combine.
        //   * 8-wave 64 x 128 tiles without split-K when they fill the chip evenly (at most one or close to two per CU): 1024 rows 53.4 -> 47.5, 2560 rows 20.2 -> 18.4;
        //   * S = 4 when 4 x tiles is one round or a whole number of rounds: 512 rows 36.4 -> 34.7, 640 rows 38.0 -> 35.9, 2048 rows 80.9 -> 74.0 (was S = 8 / 8 / 3);
        //   * else the largest S that keeps the grid under 2.25 rounds.
        const int t64 = ((M + Tile64::BM - 1) / Tile64::BM) * (N / Tile64::BN);
        if (((t64 >= 176 && t64 <= 208) || (t64 >= 448 && t64 <= 512)) && KS % Tile64W8::KU == 0 && KS / Tile64W8::KU >= 2 * Tile64W8::NSTAGE)
            return TilePlan{TG_64X128_W8, Tile64::BM, Tile64::BN, 1, TB_WIDE_W8};
        if ((tiles * 4 <= 256 || tiles % 64 == 0) && KS % (Tile128::KU * 4) == 0 && KS / 4 / Tile128::KU >= 2 * Tile128::NSTAGE) {
            p.S = 4;
            p.branch = TB_WIDE_S4;
            // one round (640 rows: 60 tiles x 4 slices = 240 workgroups): the loader-wave geometry (fc2 at 640 rows, GEMM + combine: 29.2 -> 26.6 us).
            // Finishing the slices INSIDE the launch (TS_FUSED: write-through slabs, the tile's last arriver sums them) was built and measured in round 6 and LOSES:
            // 47.1 us (59.1 on this geometry) against 26.6 -- 256 KB of dependent sc1 reads by one workgroup per tile behind 64 KB of write-through stores per workgroup
            // (profiles/r06_micro_tile_fused.txt); the product never selects it, tools/micro/bench_tile still times and checks it.
            if (tiles * 4 <= 256 && KS / 4 / Tile128PC::KU >= 2 * Tile128PC::NSTAGE) { p.geom = TG_128_PC; p.branch = TB_WIDE_S4_LOADERS; }
            return p;
        }
        const int candidates[5] = {8, 6, 4, 3, 2};
        for (int S : candidates)
            if (S <= max_s && tiles * S <= 576 && KS % (Tile128::KU * S) == 0 && KS / S / Tile128::KU >= 2 * Tile128::NSTAGE) { p.S = S; p.branch = TB_WIDE_LARGEST_S; break; }
    }
    return p;
}

// Workgroup id -> (split-K slice, row tile, column tile).  Workgroups b and b + 8 share an XCD (MI355X_MICROARCH.md), and an XCD runs ~32 of
// them at a time; what its L2 has to pull over the fabric is one K-long fragment stream per DISTINCT row tile and column tile among its
// workgroups (tools/micro/bench_fill: a CU fills at ~135 GB/s from a hot L2 whatever the path, at ~27 GB/s when every CU pulls from beyond it).
// Each XCD therefore gets a contiguous run of a grouped order (bands of GM row tiles, walked column by column): a compact block of tiles, not a
// 32 x 1 column (which made every XCD pull the whole activation panel every k-step: fabric-bound at 4096+ rows).
//   * GM: up to 12 row tiles make ONE band (an XCD then owns whole columns: the weights cross the fabric once, the small activation panel
//     eight times; bands of 8 left 2 of 10 row tiles at 640 rows to the last XCDs, which pulled two thirds of the weight matrix each);
//     more row tiles are cut into equal bands of at most 8.
//   * split-K: with S | 8 slices, XCD x works on slice x % S only (S = 8: every XCD streams ITS eighth of K of both operands, once).
TILE_PLAN_HD inline void tile_of(int b, int total, int S, int TM, int TN, int& z, int& tm, int& tn) {
    int t;
    if (S > 1 && (8 % S) == 0) {
        const int xcd = b & 7, G = 8 / S, xg = xcd / S;
        z = xcd - xg * S;
        const int q = total / G, r = total - q * G;
        t = (xg < r ? xg * (q + 1) : r * (q + 1) + (xg - r) * q) + (b >> 3);
    } else {
        z = b / total;
        const int id = b - z * total;
        const int q = total >> 3, r = total & 7, xcd = id & 7;
        t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    }
    const int nb = TM <= 12 ? 1 : (TM + 7) >> 3;
    const int GM = (TM + nb - 1) / nb;
    const int per_group = GM * TN;
    const int group = t / per_group, in_group = t - group * per_group;
    const int first = group * GM, rows = TM - first < GM ? TM - first : GM;
    tn = in_group / rows;
    tm = first + in_group - tn * rows;
}
