// SPLIT precision: the 3x3 convolutions of the HQ-VAE decoder / encoder on the matrix cores (split_kernels.h).
//
// What this file ships:
//   conv3x3_split_ring16_kernel   3x3 stride-1 'same' conv, N % 128 == 0 (every released config): the default
//   conv2x2_split_up16_kernel     nearest-x2 upsampling conv as four 2x2 phase convolutions on the low-resolution image
//   conv3x3_split_out16_kernel    conv_out (<= 16 output channels, NCHW store + clamp)
// Shapes they do not take fall back to conv3x3_split_kernel (split_conv.hip), and from there to the fp32 vector-ALU kernel.
//
// Design, arrived at over five measured generations (the superseded kernels: git history up to round 3; DESIGN.md 5.2b
// what each one taught):
//   * 4 waves per workgroup, 8 x 16 pixel tile x 128 channels, two workgroups per CU; each wave owns 128 pixels x 32 channels
//     (8 pixel blocks x 2 channel blocks of v_mfma_f32_16x16x32_f16: 128 accumulator registers, main + cross);
//   * the FILTERS never touch LDS: packed at finalize in MFMA A-operand fragment order (1-KiB chunks, [32-channel group][chunk][tap]
//     [16-channel block][hi | lo]), every wave streams the fragments of its own channels straight into registers with coalesced
//     global_load_dwordx4, a ring of three taps ahead of the MFMAs, counted s_waitcnt vmcnt;
//   * the PATCH ((8 + 2) x (16 + 2) pixels x 32 channels, both planes) is double-buffered in LDS on an 80-byte pitch (no swizzle: a
//     fragment address is base + immediate), filled through registers by buffer loads whose range check supplies the zero padding:
//     ONE workgroup barrier per 32-channel chunk;
//   * the main loop is one basic block of straight-line code with asm loads in flight across its back edge; _lib.build() audits the
//     generated ISA (csrc/audit_ring.py) and refuses to link a library whose loops the compiler has touched.
// The three kernels differ in their hand-scheduled main loops only (which read, load or store goes at which tap, and every counted wait).
// What surrounds the loops -- geometry, tile decode, patch-piece addressing, the asm wrappers the loops call, the staged row epilogue and
// the GroupNorm partials -- is defined once, in split_ring.h.
#include "split_kernels.h"
#include "split_ring.h"
#include "gemm_generic.h"
#include "switches.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// Size of a fragment-packed 3x3 filter bank (hi + lo): ceil(N / 32) channel groups x Cin / 32 chunks x 9 taps x 4 KiB
// (+ three k-tiles of padding: the kernels prefetch the filters of up to five k-steps past the end of the last n-tile's stream, and drop them)
constexpr size_t R_FRAG_PAD = 3 * 4 * 512;
size_t split_frag_elems(int N, int Cin) { return (size_t)((N + 31) / 32) * (Cin / 32) * 9 * 4 * 512 + R_FRAG_PAD; }

// ---------------------------------------------------------------------------------------------
// conv3x3_split_ring16_kernel (fifth generation): the ring structure on v_mfma_f32_16x16x32_f16.  The ring kernel keeps the matrix pipe busy 85 % of the
// time (profiles/r02_pmc_mfma_util_*.txt) -- but under that load the chip holds its clock near 1.5 GHz instead of 2.4
// (GRBM_GUI_ACTIVE / 8 / duration), so what is left is the energy per MFMA, not the issue stream; MI355X_MICROARCH.md ('DVFS give-back',
// item 7) measures the 16x16x32 shape ~1.12-1.15x faster by wall than 32x32x16 at equal cycles per FLOP with operands read from LDS.
// Same tile, patch image, piece schedule and epilogue staging; per wave 8 pixel blocks (the 8 tile rows of 16 pixels) x 2 channel blocks
// of 16; one MFMA covers a whole 32-channel chunk of a tap, so a "step" is a tap: 48 MFMAs of 16 cycles against 16 fragment reads,
// 4 filter loads and <= 1 patch piece.  Filters are packed per 16-channel block ([32-channel group][chunk][tap][block][hi | lo],
// 1 KiB each: lane l holds W[16 block + (l & 15)][tap Cin + 32 c + 8 (l >> 4) + j]), ring of 3 taps (48 registers).
// ---------------------------------------------------------------------------------------------
__global__ void pack_split_frag16_kernel(const float* __restrict__ w, half_t* __restrict__ out, int N, int Cin, size_t total) {
    const int NC = Cin / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
        size_t ch = i >> 9;
        const int plane = (int)(ch & 1); ch >>= 1;
        const int blk = (int)(ch & 1); ch >>= 1;
        const int tap = (int)(ch % 9); ch /= 9;
        const int c = (int)(ch % NC);
        const int t = (int)(ch / NC);
        const int n = t * 32 + blk * 16 + (lane & 15), k = tap * Cin + c * 32 + 8 * (lane >> 4) + j;
        const float x = n < N ? w[(size_t)n * 9 * Cin + k] : 0.0f;
        const half_t hi = (half_t)x;
        out[i] = plane ? (half_t)((x - (float)hi) * 2048.0f) : hi;
    }
}
hipError_t launch_pack_split_frag16(const float* w_tapmajor, half_t* out, int N, int Cin, hipStream_t st) {
    const size_t total = split_frag_elems(N, Cin) - R_FRAG_PAD;
    pack_split_frag16_kernel<<<(int)std::min<size_t>((total + 255) / 256, 8192), 256, 0, st>>>(w_tapmajor, out, N, Cin, total);
    return hipGetLastError();
}

namespace {
// Epilogue staging of the kernels on 8 x 2 blocks of v_mfma_f32_16x16x32_f16 per wave (ring16, up16): main + cross / 2^11 of tile rows
// 4 half .. 4 half + 3 into the staging rows.  D map: col = lane & 15 -> pixel fx of tile row i; row = 4 (lane >> 4) + r -> channel
// 16 j + 4 fk + r of the wave's 32.
__device__ __forceinline__ void h_stage_half(char* stage, const f32x4 (&accm)[8][2], const f32x4 (&accx)[8][2], int half, int wave, int fx, int fk) {
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
        const int i = half * 4 + ii, r = ii * 16 + fx;          // pixel within the staged 64
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nl = wave * 32 + j * 16 + 4 * fk;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = accm[i][j][e] + accx[i][j][e] * R_INV;
            *reinterpret_cast<f32x4*>(stage + r * R_CPITCH + nl * 4) = v;
        }
    }
}
}  // namespace

template <int ABL = 0>
__global__ __launch_bounds__(256, 2) void conv3x3_split_ring16_kernel(GemmArgs g) {
    constexpr int NI = 8;                                           // pixel blocks = tile rows
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fx = lane & 15, fk = lane >> 4;
    int tile_m, tile_n;
    r_xcd_tile(tile_m, tile_n, g.tile_panel);
    const int n0 = tile_n * 128;
    int img, trem, ty0, tx0, tiles_x, tiles_y;
    ring_tile(tile_m, g.H, g.W, img, trem, ty0, tx0, tiles_x, tiles_y);
    const int Hin = g.H >> g.upsample, Win = g.W >> g.upsample;
    const int NC = g.Cin / 32;

    // ---- patch pieces: this wave's pieces wave + 4 u of either plane, fetched through registers (split_ring.h)
    const ring_rsrc_t img_rsrc = ring_image_rsrc(g.A, img, Hin, Win, g.Cin);
    unsigned poff[3];
    ring_piece_offsets(poff, wave, lane, ty0, tx0, g.H, g.W, Win, g.upsample, g.Cin);
    u32x4 pst[2];                                                   // pieces in flight: loaded at tap t, written to LDS at tap t + 2
    unsigned piece_base = ring_piece_base(lds_base, wave, lane);

    // this wave's filter stream: 4 KiB per tap ([block 0 hi][block 0 lo][block 1 hi][block 1 lo])
    const char* bfrag = reinterpret_cast<const char*>(reinterpret_cast<const half_t*>(g.Bw_frag16) + (size_t)(n0 / 32 + wave) * ((size_t)NC * 9 * 2048));
    unsigned lane16 = lane * 16;

    f32x4 accm[NI][2], accx[NI][2];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { accm[i][j][r] = 0.0f; accx[i][j][r] = 0.0f; }
    // fragment of pixel block i at tap (dy, dx): patch row (i + dy) * 18 + fx + dx, 16-B group fk -- one base + immediates
    const unsigned abase = ring_frag_base(lds_base, fx, fk);
    half8 ah[4], al[4];                                             // pixel blocks in flight: slot = block % 4
    half8 wh[H_RING][2], wl[H_RING][2];                             // filter fragments [tap % 3][channel block]

    // ---- prologue: first patch through the piece registers, filters of taps 0 and 1; everything lands first
#pragma unroll
    for (int rnd = 0; rnd < 3; ++rnd) {
        ring_load_piece(pst[0], poff, img_rsrc, 0, 2 * rnd, g.Cin); ring_load_piece(pst[1], poff, img_rsrc, 0, 2 * rnd + 1, g.Cin);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(pst[0]), "+v"(pst[1]));
        ring_store_piece(piece_base, pst[0], 0, 2 * rnd); ring_store_piece(piece_base, pst[1], 0, 2 * rnd + 1);
    }
#pragma unroll
    for (int s = 0; s < H_AHEAD; ++s) ring_load_b4(wh[s], wl[s], lane16, bfrag, s);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // ---- main loop: one iteration = two chunks = 18 taps of straight-line code
#pragma unroll 1
    for (int c0 = 0; c0 < NC; c0 += 2) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = c0 + cc, cn = min(c + 1, NC - 1);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (ABL != 4) { ring_read_a16(ah, al, abase, cc, 0, 0); ring_read_a16(ah, al, abase, cc, 0, 1); ring_read_a16(ah, al, abase, cc, 0, 2); ring_read_a16(ah, al, abase, cc, 0, 3); }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int s = cc * 9 + tap, slot = s % H_RING, nslot = (s + H_AHEAD) % H_RING;
                const long long S = (long long)c0 * 9 + s;
                const int tapoff = (tap / 3) * R_PITCH + tap % 3, ntapoff = ((tap + 1) / 3) * R_PITCH + (tap + 1) % 3;
                if (ABL != 4) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(wh[slot][0]), "+v"(wl[slot][0]), "+v"(wh[slot][1]), "+v"(wl[slot][1]) : "n"(h_younger(s)));
                // pixel blocks in pairs [m m m m x x x x x' x' x' x']: no MFMA directly follows the one it accumulates onto
#pragma unroll
                for (int pr = 0; pr < 4; ++pr) {
                    const int i0 = 2 * pr, i1 = 2 * pr + 1;
                    // reads in issue order: blocks (2 pr, 2 pr + 1) of this tap were issued two pairs ago; behind them: the next pair (4 reads)
                    if (ABL != 4) {
                        const bool more = !(tap == 8 && pr == 3);       // the last pair of a chunk has nothing behind it
                        if (more) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[i0 % 4]), "+v"(al[i0 % 4]), "+v"(ah[i1 % 4]), "+v"(al[i1 % 4]));
                        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[i0 % 4]), "+v"(al[i0 % 4]), "+v"(ah[i1 % 4]), "+v"(al[i1 % 4]));
                    }
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            accm[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot][j], ah[(i0 + ii) % 4], accm[i0 + ii][j], 0, 0, 0);
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            accx[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot][j], al[(i0 + ii) % 4], accx[i0 + ii][j], 0, 0, 0);
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            accx[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[slot][j], ah[(i0 + ii) % 4], accx[i0 + ii][j], 0, 0, 0);
                    if (ABL == 4) continue;
                    // refill the two slots: blocks (i0 + 4, i1 + 4) of this tap, or blocks (i0 - 4, i1 - 4) of the next tap
                    if (pr < 2) {
                        if (pr == 0) { ring_read_a16(ah, al, abase, cc, tapoff, 4); ring_read_a16(ah, al, abase, cc, tapoff, 5); }
                        else { ring_read_a16(ah, al, abase, cc, tapoff, 6); ring_read_a16(ah, al, abase, cc, tapoff, 7); }
                    } else if (tap < 8) {
                        if (pr == 2) { ring_read_a16(ah, al, abase, cc, ntapoff, 0); ring_read_a16(ah, al, abase, cc, ntapoff, 1); }
                        else { ring_read_a16(ah, al, abase, cc, ntapoff, 2); ring_read_a16(ah, al, abase, cc, ntapoff, 3); }
                    }
                    if (pr == 0 && ABL != 5) ring_load_b4(wh[nslot], wl[nslot], lane16, bfrag, S + H_AHEAD);            // the slot tap s - 1 released takes the filters of tap s + 2
                    if (pr == 1 && ABL != 2) {
                        // the piece of tap - 2: behind it were issued the filters of tap + 1 (4), the piece of tap - 1 and the filters of tap + 2 (4)
                        if (tap >= 2 && tap - 2 < R_PPW) {
                            if (tap - 1 < R_PPW) asm volatile("s_waitcnt vmcnt(9)" : "+v"(pst[tap % 2]));
                            else asm volatile("s_waitcnt vmcnt(8)" : "+v"(pst[tap % 2]));
                            ring_store_piece(piece_base, pst[tap % 2], cc ^ 1, tap - 2);
                        }
                        if (tap < R_PPW) ring_load_piece(pst[tap % 2], poff, img_rsrc, cn, tap, g.Cin);
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // the patch buffers become the epilogue's staging area
    __builtin_amdgcn_sched_barrier(0);
    if (ABL == 1) { ring_sink_acc(g, accm, accx); return; }
    // ---- epilogue.  D map: col = lane & 15 -> pixel fx of tile row i; row = 4 (lane >> 4) + r -> channel 16 j + 4 fk + r of the wave's 32.
    //      Staged store, 64 pixels (tile rows 4 half .. 4 half + 3) at a time, then whole NHWC rows (split_ring.h).
    const long long pix0 = ((long long)img * g.H + ty0) * g.W + tx0;
    char* stage = lds_raw;
    float bv[8], gs[8], gq[8];
    ring_bias8(g, n0 + (tid & 15) * 8, bv);
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gs[e] = 0.0f; gq[e] = 0.0f; }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half > 0) __syncthreads();                  // the previous half has been read back
        h_stage_half(stage, accm, accx, half, wave, fx, fk);
        __syncthreads();
        ring_store_rows<4, true>(g, stage, tid, n0, bv, true, [&](int r) { return pix0 + (long long)(half * 4 + (r >> 4)) * g.W + (r & 15); }, gs, gq, bad);
    }
    if (bad && g.range_flag) atomicOr(g.range_flag, 1);
    ring_reduce_gn(g, lds_raw, tid, gs, gq, n0, true, (long long)img * (tiles_x * tiles_y) + trem);
}


// ---------------------------------------------------------------------------------------------
// Upsampling convolution (stage1/modules/layers.py:42-53: nearest x2, then a 3x3 'same' conv) as FOUR 2x2 convolutions on the
// LOW-resolution image.  Output pixel (2 y + a, 2 x + b) sees, through its 3x3 window on the upsampled image, only the low-resolution
// pixels of rows {y - 1 + a, y + a} and columns {x - 1 + b, x + b}; taps that land on the same source pixel are added up once, at
// finalize (pack_split_up16_kernel):
//     rows:  a = 0: [w0 | w1 + w2]     a = 1: [w0 + w1 | w2]      (columns alike with b)
// The same sums as the reference, regrouped -- 4 multiply-adds per output and input channel instead of 9 (2.25x fewer MFMAs on 36 % of
// the decoder's convolution work), no approximation beyond the rounding of the summed filters, which are split into hi / lo like any
// other.  Zero padding carries over: row -1 / H of the low-resolution image is exactly what rows -1 / 2 H of the upsampled one are.
// Kernel = conv3x3_split_ring16_kernel with a workgroup = an 8 x 16 tile of LOW-resolution pixels x 128 channels of ONE phase (a, b)
// (grid.x = 4 phases x N / 128), the same (8 + 2) x (16 + 2) patch image, 4 taps per 32-channel chunk at patch offsets (a + ty, b + tx);
// with a chunk only 4 taps long the six patch pieces of the next chunk are fetched at taps 0, 1 (three each) and written at taps 2, 3,
// and the filters run ONE tap ahead (ring of 2: 32 registers) -- the second workgroup of the CU covers what that exposes.
// ---------------------------------------------------------------------------------------------
__global__ void pack_split_up16_kernel(const float* __restrict__ w, half_t* __restrict__ out, int N, int Cin, size_t total) {
    const int NC = Cin / 32, NG = (N + 31) / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
        size_t ch = i >> 9;
        const int plane = (int)(ch & 1); ch >>= 1;
        const int blk = (int)(ch & 1); ch >>= 1;
        const int tap = (int)(ch & 3); ch >>= 2;
        const int c = (int)(ch % NC); ch /= NC;
        const int t = (int)(ch % NG);
        const int phase = (int)(ch / NG);
        const int pa = phase >> 1, pb = phase & 1, ty = tap >> 1, tx = tap & 1;
        const int n = t * 32 + blk * 16 + (lane & 15), kin = c * 32 + 8 * (lane >> 4) + j;
        // 3x3 taps that fall on low-resolution offset ty (tx) for phase pa (pb)
        const int ky0 = pa == 0 ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), ky1 = pa == 0 ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
        const int kx0 = pb == 0 ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kx1 = pb == 0 ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
        double x = 0.0;
        if (n < N)
            for (int ky = ky0; ky <= ky1; ++ky)
                for (int kx = kx0; kx <= kx1; ++kx) x += (double)w[(size_t)n * 9 * Cin + (size_t)(ky * 3 + kx) * Cin + kin];
        const half_t hi = (half_t)(float)x;
        out[i] = plane ? (half_t)(float)((x - (double)(float)hi) * 2048.0) : hi;
    }
}
// 4 phases x ceil(N / 32) channel groups x NC chunks x 4 taps x 4 KiB (+ one tap of padding: the filters run one tap ahead)
size_t split_up_elems(int N, int Cin) { return (size_t)4 * ((N + 31) / 32) * (Cin / 32) * 4 * 2048 + 2048; }
hipError_t launch_pack_split_up16(const float* w_tapmajor, half_t* out, int N, int Cin, hipStream_t st) {
    const size_t total = split_up_elems(N, Cin) - 2048;
    pack_split_up16_kernel<<<(int)std::min<size_t>((total + 255) / 256, 8192), 256, 0, st>>>(w_tapmajor, out, N, Cin, total);
    return hipGetLastError();
}

template <int ABL = 0>
__global__ __launch_bounds__(256, 2) void conv2x2_split_up16_kernel(GemmArgs g) {
    constexpr int NI = 8, TAPS = 4;                                 // pixel blocks = tile rows; taps per chunk
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fx = lane & 15, fk = lane >> 4;
    int tile_m, tile_v;
    r_xcd_tile(tile_m, tile_v, g.tile_panel);
    const int NT = g.N / 128;                                       // real 128-channel tiles; the grid is 4 NT wide
    const int phase = tile_v / NT, pa = phase >> 1, pb = phase & 1;
    const int n0 = (tile_v - phase * NT) * 128;
    const int Hin = g.H >> 1, Win = g.W >> 1;                       // g.H / g.W: the OUTPUT
    int img, trem, ty0, tx0, tiles_x, tiles_y;                      // ty0 / tx0: low-resolution pixels
    ring_tile(tile_m, Hin, Win, img, trem, ty0, tx0, tiles_x, tiles_y);
    const int NC = g.Cin / 32;

    // ---- patch pieces: the (8 + 2) x (16 + 2) low-resolution neighbourhood (split_ring.h)
    const ring_rsrc_t img_rsrc = ring_image_rsrc(g.A, img, Hin, Win, g.Cin);
    unsigned poff[3];
    ring_piece_offsets(poff, wave, lane, ty0, tx0, Hin, Win, Win, 0, g.Cin);
    u32x4 pst[R_PPW];                                               // the six pieces of the next chunk: loaded at taps 0 / 1, written at taps 2 / 3
    unsigned piece_base = ring_piece_base(lds_base, wave, lane);

    // this wave's filter stream: 4 KiB per tap ([block 0 hi][block 0 lo][block 1 hi][block 1 lo]), 4 taps per chunk
    const char* bfrag = reinterpret_cast<const char*>(reinterpret_cast<const half_t*>(g.Bw_up16) +
                                                      ((size_t)phase * (g.N / 32) + n0 / 32 + wave) * ((size_t)NC * TAPS * 2048));
    unsigned lane16 = lane * 16;

    f32x4 accm[NI][2], accx[NI][2];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { accm[i][j][r] = 0.0f; accx[i][j][r] = 0.0f; }
    // fragment of pixel block i at tap (ty, tx) of phase (pa, pb): patch row (i + pa + ty) * 18 + fx + pb + tx -- the phase goes into the base
    const unsigned abase = ring_frag_base(lds_base, fx + pa * R_PITCH + pb, fk);
    half8 ah[4], al[4];                                             // pixel blocks in flight: slot = block % 4
    half8 wh[2][2], wl[2][2];                                       // filter fragments [tap % 2][channel block]

    // ---- prologue: the first patch through the piece registers, the filters of tap 0; everything lands first
#pragma unroll
    for (int u = 0; u < R_PPW; ++u) ring_load_piece(pst[u], poff, img_rsrc, 0, u, g.Cin);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(pst[0]), "+v"(pst[1]), "+v"(pst[2]), "+v"(pst[3]), "+v"(pst[4]), "+v"(pst[5]));
#pragma unroll
    for (int u = 0; u < R_PPW; ++u) ring_store_piece(piece_base, pst[u], 0, u);
    ring_load_b4(wh[0], wl[0], lane16, bfrag, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // ---- main loop: one iteration = two chunks = 8 taps of straight-line code.  Vector-memory operations in issue order per tap t:
    //      [filters of tap t + 1: 4] then, at taps 0 and 1, [three pieces].  They retire in that order, so the wait for the filters of
    //      tap t (issued at tap t - 1) leaves 3 younger loads in flight behind taps 0 / 1 and none behind taps 2 / 3 -- by then every
    //      piece has landed too, and the ds_writes at taps 2 / 3 need no wait of their own (the asm operands still carry the dependence).
#pragma unroll 1
    for (int c0 = 0; c0 < NC; c0 += 2) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = c0 + cc, cn = min(c + 1, NC - 1);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (ABL != 4) { ring_read_a16(ah, al, abase, cc, 0, 0); ring_read_a16(ah, al, abase, cc, 0, 1); ring_read_a16(ah, al, abase, cc, 0, 2); ring_read_a16(ah, al, abase, cc, 0, 3); }
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int s = cc * TAPS + tap, slot = s % 2, nslot = (s + 1) % 2;
                const long long S = (long long)c0 * TAPS + s;
                const int tapoff = (tap / 2) * R_PITCH + tap % 2, ntapoff = ((tap + 1) / 2) * R_PITCH + (tap + 1) % 2;
                if (ABL != 4) {
                    if (tap == 1 || tap == 2) asm volatile("s_waitcnt vmcnt(3)" : "+v"(wh[slot][0]), "+v"(wl[slot][0]), "+v"(wh[slot][1]), "+v"(wl[slot][1]));
                    else asm volatile("s_waitcnt vmcnt(0)" : "+v"(wh[slot][0]), "+v"(wl[slot][0]), "+v"(wh[slot][1]), "+v"(wl[slot][1]));
                    if (ABL != 5) ring_load_b4(wh[nslot], wl[nslot], lane16, bfrag, S + 1);                               // the slot tap s - 1 released takes the filters of tap s + 1: a whole tap of MFMAs ahead
                }
#pragma unroll
                for (int pr = 0; pr < 4; ++pr) {
                    const int i0 = 2 * pr, i1 = 2 * pr + 1;
                    if (ABL != 4) {
                        const bool more = !(tap == TAPS - 1 && pr == 3);       // the last pair of a chunk has nothing behind it
                        if (more) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[i0 % 4]), "+v"(al[i0 % 4]), "+v"(ah[i1 % 4]), "+v"(al[i1 % 4]));
                        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[i0 % 4]), "+v"(al[i0 % 4]), "+v"(ah[i1 % 4]), "+v"(al[i1 % 4]));
                    }
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            accm[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot][j], ah[(i0 + ii) % 4], accm[i0 + ii][j], 0, 0, 0);
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            accx[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot][j], al[(i0 + ii) % 4], accx[i0 + ii][j], 0, 0, 0);
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            accx[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[slot][j], ah[(i0 + ii) % 4], accx[i0 + ii][j], 0, 0, 0);
                    if (ABL == 4) continue;
                    // the piece written here goes in FRONT of the fragment reads: lgkmcnt(4) of the next pair then covers exactly those reads
                    if (pr >= 1 && tap >= 2 && ABL != 2) {
                        const int u = 3 * (tap - 2) + pr - 1;
                        // (already landed: see above; the count only has to be loose enough not to wait for anything younger -- the
                        //  filters of the next tap, and at tap 2 the three pieces tap 1 fetched)
                        if (tap == 2) asm volatile("s_waitcnt vmcnt(7)" : "+v"(pst[u])); else asm volatile("s_waitcnt vmcnt(4)" : "+v"(pst[u]));
                        ring_store_piece(piece_base, pst[u], cc ^ 1, u);
                    }
                    // refill the two slots: blocks (i0 + 4, i1 + 4) of this tap, or blocks (i0 - 4, i1 - 4) of the next tap
                    if (pr < 2) {
                        if (pr == 0) { ring_read_a16(ah, al, abase, cc, tapoff, 4); ring_read_a16(ah, al, abase, cc, tapoff, 5); }
                        else { ring_read_a16(ah, al, abase, cc, tapoff, 6); ring_read_a16(ah, al, abase, cc, tapoff, 7); }
                    } else if (tap < TAPS - 1) {
                        if (pr == 2) { ring_read_a16(ah, al, abase, cc, ntapoff, 0); ring_read_a16(ah, al, abase, cc, ntapoff, 1); }
                        else { ring_read_a16(ah, al, abase, cc, ntapoff, 2); ring_read_a16(ah, al, abase, cc, ntapoff, 3); }
                    }
                    if (pr >= 1 && tap < 2 && ABL != 2) ring_load_piece(pst[3 * tap + pr - 1], poff, img_rsrc, cn, 3 * tap + pr - 1, g.Cin);
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // the patch buffers become the epilogue's staging area
    __builtin_amdgcn_sched_barrier(0);
    if (ABL == 1) { ring_sink_acc(g, accm, accx); return; }
    // ---- epilogue: as the ring16 kernel, with low-resolution tile pixel (row, col) stored at output pixel (2 (ty0 + row) + pa, 2 (tx0 + col) + pb)
    char* stage = lds_raw;
    float bv[8], gs[8], gq[8];
    ring_bias8(g, n0 + (tid & 15) * 8, bv);
#pragma unroll
    for (int e = 0; e < 8; ++e) { gs[e] = 0.0f; gq[e] = 0.0f; }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half > 0) __syncthreads();                  // the previous half has been read back
        h_stage_half(stage, accm, accx, half, wave, fx, fk);
        __syncthreads();
        ring_store_rows<4>(g, stage, tid, n0, bv, true, [&](int r) {
            const long long oy = 2 * (ty0 + half * 4 + (r >> 4)) + pa, ox = 2 * (tx0 + (r & 15)) + pb;
            return ((long long)img * g.H + oy) * g.W + ox;
        }, gs, gq);
    }
    // one partial per (low-resolution tile, phase): 4 tiles_x tiles_y per image
    ring_reduce_gn(g, lds_raw, tid, gs, gq, n0, true, ((long long)img * (tiles_x * tiles_y) + trem) * 4 + phase);
}


// ---------------------------------------------------------------------------------------------
// conv_out (C_in -> 3 channels, NCHW fp32 + clamp) on the ring16 structure: the output channels are padded to ONE 16-channel MFMA block
// (32 in the stream kernel's variant: 10x the matrix work the 3 channels need, 36 % pipe utilisation), so the four waves of a tile split
// its PIXELS: wave w owns tile rows 2 w and 2 w + 1 (2 pixel blocks x 1 channel block: 6 MFMAs per tap) and all of them fetch the same
// filter fragments (L1 hits).  Patch image, piece schedule and waits as in conv3x3_split_ring16_kernel; the fragments of the next tap are
// read one tap ahead (4 register slots: tap parity x pixel block).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void conv3x3_split_out16_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fx = lane & 15, fk = lane >> 4;
    const int tile_m = blockIdx.y;
    int img, trem, ty0, tx0, tiles_x, tiles_y;
    ring_tile(tile_m, g.H, g.W, img, trem, ty0, tx0, tiles_x, tiles_y);
    const int Hin = g.H >> g.upsample, Win = g.W >> g.upsample;
    const int NC = g.Cin / 32;

    const ring_rsrc_t img_rsrc = ring_image_rsrc(g.A, img, Hin, Win, g.Cin);
    unsigned poff[3];
    ring_piece_offsets(poff, wave, lane, ty0, tx0, g.H, g.W, Win, g.upsample, g.Cin);
    u32x4 pst[2];
    unsigned piece_base = ring_piece_base(lds_base, wave, lane);

    // one filter stream for the whole tile: 4 KiB per tap in the 16-channel-block packing, block 0 only ([hi][lo])
    const char* bfrag = reinterpret_cast<const char*>(g.Bw_frag16);
    unsigned lane16 = lane * 16;

    f32x4 accm[2], accx[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) { accm[i][r] = 0.0f; accx[i][r] = 0.0f; }
    // this wave's pixel blocks = tile rows 2 wave, 2 wave + 1
    const unsigned abase = ring_frag_base(lds_base, 2 * wave * R_PITCH + fx, fk);
    half8 ah[4], al[4];                                             // [tap parity * 2 + block]
    half8 wh[H_RING], wl[H_RING];

#pragma unroll
    for (int rnd = 0; rnd < 3; ++rnd) {
        ring_load_piece(pst[0], poff, img_rsrc, 0, 2 * rnd, g.Cin); ring_load_piece(pst[1], poff, img_rsrc, 0, 2 * rnd + 1, g.Cin);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(pst[0]), "+v"(pst[1]));
        ring_store_piece(piece_base, pst[0], 0, 2 * rnd); ring_store_piece(piece_base, pst[1], 0, 2 * rnd + 1);
    }
#pragma unroll
    for (int s = 0; s < H_AHEAD; ++s) ring_load_b2(wh[s], wl[s], lane16, bfrag, s);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

#pragma unroll 1
    for (int c0 = 0; c0 < NC; c0 += 2) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = c0 + cc, cn = min(c + 1, NC - 1);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            ring_read_a16(ah, al, abase, cc, 0, 0, 0); ring_read_a16(ah, al, abase, cc, 0, 1, 1);       // tap 0 -> parity 0
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int s = cc * 9 + tap, slot = s % H_RING, nslot = (s + H_AHEAD) % H_RING;
                const long long S = (long long)c0 * 9 + s;
                const int par = tap & 1;
                const int ntapoff = ((tap + 1) / 3) * R_PITCH + (tap + 1) % 3;
                // the next tap's fragments first (read one tap ahead into the other parity's slots), then this tap's MFMAs
                if (tap < 8) {
                    if (par == 0) { ring_read_a16(ah, al, abase, cc, ntapoff, 0, 2); ring_read_a16(ah, al, abase, cc, ntapoff, 1, 3); }
                    else { ring_read_a16(ah, al, abase, cc, ntapoff, 0, 0); ring_read_a16(ah, al, abase, cc, ntapoff, 1, 1); }
                }
                asm volatile("s_waitcnt vmcnt(%2)" : "+v"(wh[slot]), "+v"(wl[slot]) : "n"(h_younger(s, 2)));
                if (tap < 8) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[2 * par]), "+v"(al[2 * par]), "+v"(ah[2 * par + 1]), "+v"(al[2 * par + 1]));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[2 * par]), "+v"(al[2 * par]), "+v"(ah[2 * par + 1]), "+v"(al[2 * par + 1]));
                accm[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot], ah[2 * par], accm[0], 0, 0, 0);
                accm[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot], ah[2 * par + 1], accm[1], 0, 0, 0);
                accx[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot], al[2 * par], accx[0], 0, 0, 0);
                accx[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[slot], al[2 * par + 1], accx[1], 0, 0, 0);
                accx[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[slot], ah[2 * par], accx[0], 0, 0, 0);
                accx[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[slot], ah[2 * par + 1], accx[1], 0, 0, 0);
                ring_load_b2(wh[nslot], wl[nslot], lane16, bfrag, S + H_AHEAD);
                if (tap >= 2 && tap - 2 < R_PPW) {
                    if (tap - 1 < R_PPW) asm volatile("s_waitcnt vmcnt(5)" : "+v"(pst[tap % 2]));     // behind the piece: filters of tap + 1 (2), piece of tap - 1, filters of tap + 2 (2)
                    else asm volatile("s_waitcnt vmcnt(4)" : "+v"(pst[tap % 2]));
                    ring_store_piece(piece_base, pst[tap % 2], cc ^ 1, tap - 2);
                }
                if (tap < R_PPW) ring_load_piece(pst[tap % 2], poff, img_rsrc, cn, tap, g.Cin);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    // ---- epilogue: D col = lane & 15 -> pixel fx of tile row 2 wave + i; row = 4 fk + r -> channel (< N <= 16)
    float* Cb = reinterpret_cast<float*>(g.C);
    const long long hw = (long long)g.H * g.W;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long pix = (long long)(ty0 + 2 * wave + i) * g.W + tx0 + fx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = 4 * fk + r;
            if (n >= g.N) continue;
            float v = (accm[i][r] + accx[i][r] * R_INV) * g.alpha + (g.bias ? g.bias[n] : 0.0f);
            if (g.clamp01) v = fminf(fmaxf(0.5f * v + 0.5f, 0.0f), 1.0f);
            Cb[((long long)img * g.N + n) * hw + pix] = v;
        }
    }
}

// can the conv's epilogue emit operand planes (GemmArgs::out_split)?  Only conv3x3_split_ring16_kernel does: g must take that kernel.
bool split_conv3_emits_planes(const GemmArgs& g) {
    const bool off = !switch_value(SW_SPLIT_PLANES_OUT);        // A/B switch: 0 = fp32 tensor + operand pass
    return !off && split_stream_ok(g) && g.store == STORE_ROWS && !g.upsample && g.ldc == g.N && g.N % 8 == 0;
}
bool split_stream_ok(const GemmArgs& g) {
    if (!g.Bw_frag16) return false;
    if (g.H % R_TY != 0 || g.W % R_TX != 0 || g.Cin % 64 != 0) return false;      // an even number of 32-channel chunks (static ring slots)
    // one image's operand planes are addressed with 32-bit byte offsets below 2^31 (buffer loads; 2^31 marks the padding ring)
    if ((long long)(g.H >> g.upsample) * (g.W >> g.upsample) * g.Cin * 4 >= (1ll << 31)) return false;
    if (g.store == STORE_NCHW) return g.N <= 16;          // conv_out: one 16-channel block
    return g.N % 128 == 0 && g.ldc % 8 == 0;              // whole 128-channel tiles (the packed fragments hold ceil(N / 32) n-tiles)
}
// upsampling conv as four 2x2 phase convolutions on the low-resolution image (conv2x2_split_up16_kernel)
static bool split_up_shape(const GemmArgs& g) {
    const bool off = !switch_value(SW_SPLIT_UP);              // A/B switch: 0 = nine taps on the upsampled image
    return !off && g.upsample == 1 && g.Bw_up16 && g.store == STORE_ROWS && (g.H / 2) % R_TY == 0 && (g.W / 2) % R_TX == 0 && g.N % 128 == 0;
}
int split_stream_tiles_per_image(const GemmArgs& g) { return split_up_shape(g) ? 4 * (g.H / 2 / R_TY) * (g.W / 2 / R_TX) : (g.H / R_TY) * (g.W / R_TX); }
hipError_t launch_split_conv3_stream(const GemmArgs& g, hipStream_t st) {
    if (g.store == STORE_NCHW) conv3x3_split_out16_kernel<<<dim3(1, g.M / (R_TY * R_TX), 1), 256, G_LDS, st>>>(g);
    else if (split_up_shape(g)) conv2x2_split_up16_kernel<0><<<dim3(4 * (g.N / 128), g.M / 4 / (R_TY * R_TX), 1), 256, G_LDS, st>>>(g);
    else conv3x3_split_ring16_kernel<0><<<dim3(g.N / 128, g.M / (R_TY * R_TX), 1), 256, G_LDS, st>>>(g);
    return hipGetLastError();
}
hipError_t split_stream_configure() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_split_ring16_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv2x2_split_up16_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_split_out16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
}

// ---------------------------------------------------------------------------------------------
// norm_out -> swish -> conv_out (stage1/modules/layers.py:404-410; <= 4 output channels, NCHW fp32 + clamp) in ONE kernel, fp32 FMAs.
// conv_out is 0.26 % of the decoder's multiply-adds on the decoder's LARGEST tensor: on the matrix cores it needs the tensor as fp16
// hi / lo planes (an operand pass over 2 x 2.1 GB at batch 64) and pads 3 output channels to a 16-channel MFMA block.  Here the fp32
// tensor is read ONCE: a workgroup takes a 16 x 16 pixel tile, per 32-channel chunk it applies GroupNorm + swish while it fills the
// (16 + 2) x (16 + 2) patch in LDS (zero padding = zeros AFTER the normalisation, as nn.Conv2d pads), then every thread accumulates the
// three outputs of its pixel with packed fp32 FMAs -- filters from scalar registers (uniform addresses), patch rows on a 144-byte pitch
// (8 consecutive pixels start in 8 different 16-byte bank groups).  The loads of chunk c + 1 are in flight under the FMAs of chunk c.
// Exact fp32 products: no split, no range to check.  Bounds: 2.1 GB of HBM reads (0.42 ms at batch 64) / ~2.7 G swish evaluations.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int O_T = 16, O_P = O_T + 2, O_CH = 32, O_PITCH = O_CH + 4;          // tile edge, patch edge, channels per chunk, floats per patch row
constexpr int O_LDS = O_P * O_P * O_PITCH * 4;                                  // 46656 B: three workgroups per CU
constexpr int O_V4 = O_P * O_P * (O_CH / 4);                                    // float4 slots of a chunk's patch (2592)
constexpr int O_PER = (O_V4 + 255) / 256;                                       // per thread (11; the last one partial)
typedef __attribute__((ext_vector_type(2))) float f32x2;
}  // namespace

template <int NO>
__global__ __launch_bounds__(256, 3) void conv_out_direct_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    float* patch = reinterpret_cast<float*>(lds_raw);
    const int tid = threadIdx.x;
    const int tiles_x = g.W / O_T, tiles = tiles_x * (g.H / O_T);
    const int img = blockIdx.x / tiles, trem = blockIdx.x - img * tiles;
    const int ty0 = (trem / tiles_x) * O_T, tx0 = (trem % tiles_x) * O_T;
    const int C = g.Cin, NC = C / O_CH;
    const float* __restrict__ X = reinterpret_cast<const float*>(g.A) + (long long)img * g.H * g.W * C;
    const float* __restrict__ Wt = reinterpret_cast<const float*>(g.Bw);        // [NO][9][C]
    // this thread's patch slots: slot = tid + 256 u -> pixel slot / 8, channel quad slot % 8 (the same quad for every u)
    const int v = tid & 7;
    int src[O_PER];                                     // element offset of the pixel inside the image (clamped: every load is unconditional)
    unsigned inside = 0;                                // bit u: slot u is a pixel of the image (else padding / past the patch: zeros)
#pragma unroll
    for (int u = 0; u < O_PER; ++u) {
        const int q = (tid + 256 * u) >> 3;
        const int qy = q / O_P, qx = q - qy * O_P;
        const int iy = ty0 + qy - 1, ix = tx0 + qx - 1;
        const bool in = (q < O_P * O_P) & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
        src[u] = in ? (iy * g.W + ix) * C + v * 4 : v * 4;
        inside |= in ? 1u << u : 0u;
    }
    const int cpg = C / g.gn_groups;
    const float* stats = g.gn_stats + (long long)img * g.gn_groups * 2;
    f32x4 r[O_PER];
    auto fetch = [&](int c) {
#pragma unroll
        for (int u = 0; u < O_PER; ++u) r[u] = *reinterpret_cast<const f32x4*>(X + src[u] + c * O_CH);
    };
    auto fill = [&](int c) {                            // GroupNorm + swish of the fetched quads into the patch
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = c * O_CH + v * 4 + j;
            const float mu = stats[(ch / cpg) * 2], rs = stats[(ch / cpg) * 2 + 1];
            a[j] = rs * g.gn_gamma[ch];
            b[j] = g.gn_beta[ch] - mu * a[j];
        }
#pragma unroll
        for (int u = 0; u < O_PER; ++u) {
            const int slot = tid + 256 * u;
            if (slot >= O_V4) continue;
            f32x4 y = {0.0f, 0.0f, 0.0f, 0.0f};
            if (inside >> u & 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = r[u][j] * a[j] + b[j];
                    if (g.gn_swish) t = t * __builtin_amdgcn_rcpf(1.0f + __expf(-t));
                    y[j] = t;
                }
            }
            *reinterpret_cast<f32x4*>(patch + (slot >> 3) * O_PITCH + v * 4) = y;
        }
    };
    const int py = tid >> 4, px = tid & 15;
    f32x2 acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = f32x2{0.0f, 0.0f};
    fetch(0);
    for (int c = 0; c < NC; ++c) {
        if (c > 0) __syncthreads();                     // the FMAs of chunk c - 1 have read the patch
        fill(c);
        __syncthreads();
        if (c + 1 < NC) fetch(c + 1);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float* row = patch + ((py + tap / 3) * O_P + px + tap % 3) * O_PITCH;
            f32x4 x[O_CH / 4];
#pragma unroll
            for (int q = 0; q < O_CH / 4; ++q) x[q] = *reinterpret_cast<const f32x4*>(row + q * 4);
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                const float* w = Wt + ((long long)o * 9 + tap) * C + c * O_CH;      // uniform: scalar loads
#pragma unroll
                for (int q = 0; q < O_CH / 4; ++q) {
                    acc[o] += f32x2{x[q][0], x[q][1]} * f32x2{w[q * 4], w[q * 4 + 1]};
                    acc[o] += f32x2{x[q][2], x[q][3]} * f32x2{w[q * 4 + 2], w[q * 4 + 3]};
                }
            }
        }
    }
    float* Cb = reinterpret_cast<float*>(g.C);
    const long long hw = (long long)g.H * g.W, pix = (long long)(ty0 + py) * g.W + tx0 + px;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        float val = (acc[o][0] + acc[o][1]) * g.alpha + (g.bias ? g.bias[o] : 0.0f);
        if (g.clamp01) val = fminf(fmaxf(0.5f * val + 0.5f, 0.0f), 1.0f);
        Cb[((long long)img * NO + o) * hw + pix] = val;
    }
}

bool conv_out_direct_ok(const GemmArgs& g) {
    const bool off = !switch_value(SW_CONV_OUT_DIRECT);        // A/B switch: 0 = operand pass + conv3x3_split_out16_kernel
    return !off && g.conv_taps == 9 && g.store == STORE_NCHW && g.N >= 1 && g.N <= 4 && g.Cin % O_CH == 0 && g.H % O_T == 0 && g.W % O_T == 0 &&
           !g.upsample && !g.conv_stride2 && !g.resid && g.gn_stats && g.gn_groups > 0 && g.Cin % g.gn_groups == 0 &&
           (long long)g.H * g.W * g.Cin < (1ll << 31);
}
hipError_t launch_conv_out_direct(const GemmArgs& g, hipStream_t st) {
    const int grid = (g.M / (g.H * g.W)) * (g.H / O_T) * (g.W / O_T);
    switch (g.N) {
        case 1: conv_out_direct_kernel<1><<<grid, 256, O_LDS, st>>>(g); break;
        case 2: conv_out_direct_kernel<2><<<grid, 256, O_LDS, st>>>(g); break;
        case 3: conv_out_direct_kernel<3><<<grid, 256, O_LDS, st>>>(g); break;
        default: conv_out_direct_kernel<4><<<grid, 256, O_LDS, st>>>(g); break;
    }
    return hipGetLastError();
}
