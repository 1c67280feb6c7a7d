// SPLIT precision: what the hand-scheduled 3x3 conv kernels share around their main loops -- conv3x3_split_ring16_kernel,
// conv2x2_split_up16_kernel, conv3x3_split_out16_kernel (split_stream_conv.hip) and the staged epilogue of conv3x3_split_kernel
// (split_conv.hip): tile geometry, the patch-piece addressing, one definition of every asm load / read / write the loops issue, and the
// second half of the epilogue (staged fp32 rows -> alpha / bias / residual -> store -> GroupNorm partials).
// Device-only and force-inlined: state travels by reference, nothing here is a struct the compiler could keep in memory.  The loops
// themselves -- which helper goes at which tap, and every counted s_waitcnt -- stay in the kernels (csrc/audit_ring.py audits them).
// An `int` parameter documented as IMMEDIATE ends up in an "n" asm operand: after inlining and unrolling it must be a constant.
#pragma once
#include "split_kernels.h"
#include "split_device.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

namespace {
constexpr float R_INV = 1.0f / 2048.0f;
constexpr int R_TY = 8, R_TX = 16, R_PITCH = R_TX + 2;
constexpr int R_ROWS = (R_TY + 2) * R_PITCH;                    // 180 patch rows (pixels) of 64 B per plane
constexpr int R_PIECES = (R_ROWS + 15) / 16;                    // 12 DMA pieces of 16 rows per plane
constexpr int R_PPW = 2 * R_PIECES / 4;                         // pieces per wave and chunk (both planes)
constexpr int R_CPITCH = 128 * 4 + 16;                          // fp32 staging row of the epilogue (bytes)
static_assert(R_PPW == 6, "one piece per wave at taps 0..5");
// Patch rows are 64 B of data on an 80-B pitch: 8 consecutive pixels then start in 8 different 16-B bank groups (5 q mod 8), so the
// fragment reads need no XOR swizzle -- and without one a fragment address is  base(fragment) + constant(buffer, tap, plane), i.e. an
// immediate offset: ZERO vector instructions per read (a swizzled layout cost ~7 each, and vector instructions are not hidden behind
// this wave's or its SIMD neighbour's MFMAs).
constexpr int G_PITCH = 80, G_PLANE = 16 * R_PIECES * G_PITCH, G_LDS = 4 * G_PLANE;       // 15 KiB per plane, 60 KiB per workgroup
static_assert(64 * R_CPITCH <= G_LDS, "epilogue staging (64 pixels at a time) must fit in the patch buffers");
static_assert(3 * G_PLANE + 38 * G_PITCH + 32 < 65536, "ds_read immediate offsets");

constexpr int H_RING = 3, H_AHEAD = H_RING - 1, H_STEPS = 18;         // ring slots (taps), prefetch distance, taps per loop body (two chunks)
static_assert(H_STEPS % H_RING == 0, "static ring slots");
constexpr bool h_piece_at(int u) { u = ((u % H_STEPS) + H_STEPS) % H_STEPS; return (u % 9) < 6; }
// loads issued after the filters of body step s (`per_step` loads, fetched during step s - 2, first hook) and before step s begins
constexpr int h_younger(int s, int per_step = 4) {
    int n = per_step * (H_AHEAD - 1);
    for (int u = s - H_AHEAD; u < s; ++u) n += h_piece_at(u) ? 1 : 0;
    return n;
}

__device__ __forceinline__ void r_xcd_tile(int& tile_m, int& tile_n, int panel) {
    const int nx = gridDim.x, total = gridDim.x * gridDim.y;
    int id = blockIdx.x + nx * blockIdx.y;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    if (panel > 0) {
        // panels of `panel` pixel tiles x all n-tiles; inside a panel the pixel tile runs fastest: the workgroups an XCD holds at one
        // time walk ONE filter stream together (L2 hits) and each its own patch
        const int per = panel * nx, p = id / per, r = id - p * per;
        const int rows = min(panel, (int)gridDim.y - p * panel);
        tile_n = r / rows;
        tile_m = p * panel + (r - tile_n * rows);
        return;
    }
    tile_m = id / nx;
    tile_n = id - tile_m * nx;
}

// pixel tile tile_m of a batch of H x W images cut into 8 x 16 tiles (up16: the LOW-resolution image; the others: the output)
__device__ __forceinline__ void ring_tile(int tile_m, int H, int W, int& img, int& trem, int& ty0, int& tx0, int& tiles_x, int& tiles_y) {
    tiles_x = W / R_TX; tiles_y = H / R_TY;
    img = tile_m / (tiles_x * tiles_y);
    trem = tile_m - img * (tiles_x * tiles_y);
    ty0 = (trem / tiles_x) * R_TY; tx0 = (trem % tiles_x) * R_TX;
}

// buffer resource of image `img` of the operand planes A = [pixel][hi Cin | lo Cin]: the range check of a buffer load supplies the zero padding
typedef int ring_rsrc_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ring_rsrc_t ring_image_rsrc(const void* A, int img, int Hin, int Win, int Cin) {
    const unsigned long long ib = (unsigned long long)(size_t)(reinterpret_cast<const half_t*>(A) + (long long)img * Hin * Win * (2 * Cin));
    ring_rsrc_t rsrc;
    rsrc[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)ib);
    rsrc[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(ib >> 32) & 0xffff);      // stride 0
    rsrc[2] = __builtin_amdgcn_readfirstlane(Hin * Win * 2 * Cin * 2);                 // bytes
    rsrc[3] = 0x00020000;                                                              // raw buffer, 32-bit data format (gfx9)
    return rsrc;
}
// hi-plane source offset of this lane's 16 B of pieces wave + 4 u, u = 0..2 (a piece = 16 patch rows; the lo plane is + Cin halves, a
// scalar offset).  The patch is the (8 + 2) x (16 + 2) neighbourhood of tile (ty0, tx0) in an H x W image whose pixel (y, x) is read from
// input pixel (y >> up, x >> up) of rows Win wide; outside the image: 2^31, which the range check turns into zeros.
__device__ __forceinline__ void ring_piece_offsets(unsigned (&poff)[3], int wave, int lane, int ty0, int tx0, int H, int W, int Win, int up, int Cin) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int piece = wave + 4 * u;
        const int q = piece * 16 + (lane >> 2);
        const int qy = (q * 3641) >> 16, qx = q - qy * R_PITCH;                 // q / 18 for q < 192
        const int iy = ty0 + qy - 1, ix = tx0 + qx - 1;
        const bool in = (q < R_ROWS) & ((unsigned)iy < (unsigned)H) & ((unsigned)ix < (unsigned)W);
        const unsigned off = (unsigned)((((iy >> up) * Win + (ix >> up)) * (2 * Cin) + (lane & 3) * 8) * 2);
        poff[u] = in ? off : 0x80000000u;
    }
}
// LDS address of this lane's 16 B inside piece `wave` of buffer 0, plane 0
__device__ __forceinline__ unsigned ring_piece_base(unsigned lds_base, int wave, int lane) {
    return lds_base + wave * (16 * G_PITCH) + (lane >> 2) * G_PITCH + (lane & 3) * 16;
}
// LDS address of a fragment's 16-B group fk in patch row `row` of buffer 0, plane 0: every read is this base + an immediate
__device__ __forceinline__ unsigned ring_frag_base(unsigned lds_base, int row, int fk) { return lds_base + row * G_PITCH + fk * 16; }

// piece u (0..5: plane u / 3, piece wave + 4 (u % 3)) of chunk c, global -> register
__device__ __forceinline__ void ring_load_piece(u32x4& dst, const unsigned (&poff)[3], const ring_rsrc_t& rsrc, int c, int u, int Cin) {
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(poff[u % 3]), "s"(rsrc), "s"(c * 64 + (u / 3) * Cin * 2));
}
// piece u, register -> patch buffer `buf` (both IMMEDIATE)
__device__ __forceinline__ void ring_store_piece(unsigned piece_base, const u32x4& src, int buf, int u) {
    asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(piece_base), "v"(src), "n"((buf * 2 + u / 3) * G_PLANE + 4 * (u % 3) * 16 * G_PITCH) : "memory");
}
// hi / lo fragments of pixel block i at patch offset tapoff, buffer ps (all three IMMEDIATE), into register slot `slot`
__device__ __forceinline__ void ring_read_a16(half8 (&ah)[4], half8 (&al)[4], unsigned abase, int ps, int tapoff, int i, int slot) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ah[slot]) : "v"(abase), "n"(ps * 2 * G_PLANE + (i * R_PITCH + tapoff) * G_PITCH));
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(al[slot]) : "v"(abase), "n"(ps * 2 * G_PLANE + (i * R_PITCH + tapoff) * G_PITCH + G_PLANE));
}
__device__ __forceinline__ void ring_read_a16(half8 (&ah)[4], half8 (&al)[4], unsigned abase, int ps, int tapoff, int i) {
    ring_read_a16(ah, al, abase, ps, tapoff, i, i % 4);
}
// filters of stream step S (4 KiB per step: [block 0 hi][block 0 lo][block 1 hi][block 1 lo]), global -> registers: both blocks | block 0
__device__ __forceinline__ void ring_load_b4(half8 (&wh)[2], half8 (&wl)[2], unsigned lane16, const char* bfrag, long long S) {
    const char* p = bfrag + S * 4096;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(wh[0]) : "v"(lane16), "s"(p));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(wl[0]) : "v"(lane16), "s"(p));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "=v"(wh[1]) : "v"(lane16), "s"(p));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:3072" : "=v"(wl[1]) : "v"(lane16), "s"(p));
}
__device__ __forceinline__ void ring_load_b2(half8& wh, half8& wl, unsigned lane16, const char* bfrag, long long S) {
    const char* p = bfrag + S * 4096;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(wh) : "v"(lane16), "s"(p));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(wl) : "v"(lane16), "s"(p));
}

// ablation 1 of tools/micro/bench_split (no epilogue): keep the accumulators alive, one store per wave at most
template <class V, int NI, int NJ>
__device__ __forceinline__ void ring_sink_acc(const GemmArgs& g, const V (&accm)[NI][NJ], const V (&accx)[NI][NJ]) {
    float sacc = 0.0f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < (int)(sizeof(V) / sizeof(float)); ++r) sacc += accm[i][j][r] + accx[i][j][r];
    if (sacc == 12345.678f) reinterpret_cast<float*>(g.C)[0] = sacc;
}

// ---- the epilogue behind the staging: the workgroup's 256 (active) threads read a staged [16 PASSES pixels][128 channels] fp32 tile back
//      as whole NHWC rows -- thread tid: channels n0 + 8 (tid & 15) .. + 7 of staged rows 16 pass + (tid >> 4)
__device__ __forceinline__ void ring_bias8(const GemmArgs& g, int nn, float (&bv)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = (g.bias && nn + e < g.N) ? g.bias[nn + e] : 0.0f;
}
// v * alpha + bias (+ residual) of this thread's 8 channels of its PASSES rows; staged row r goes to output pixel pixel_of(r).  Stored as
// fp32 or, OUT_SPLIT and g.out_split, as the hi / lo operand planes of the next conv; gs / gq accumulate the GroupNorm sums of what was stored.
template <int PASSES, bool OUT_SPLIT, class PixelOf>
__device__ __forceinline__ void ring_store_rows(const GemmArgs& g, const char* stage, int tid, int n0, const float (&bv)[8], bool active,
                                                PixelOf pixel_of, float (&gs)[8], float (&gq)[8], bool& bad) {
    float* Cb = reinterpret_cast<float*>(g.C);
    const float* Rb = reinterpret_cast<const float*>(g.resid);
    const int c8 = (tid & 15) * 8, nn = n0 + c8;
    if (active && nn < g.N) {                           // N % 8 == 0: a thread's 8 channels are all in or all out
        long long moff[PASSES];
        f32x4 r0[PASSES], r1[PASSES];
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {     // the residual rows of all passes are fetched together
            const int r = pass * 16 + (tid >> 4);
            moff[pass] = pixel_of(r) * g.ldc + nn;
            if (Rb) { r0[pass] = *reinterpret_cast<const f32x4*>(Rb + moff[pass]); r1[pass] = *reinterpret_cast<const f32x4*>(Rb + moff[pass] + 4); }
        }
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            const int r = pass * 16 + (tid >> 4);
            const f32x4 lo = *reinterpret_cast<const f32x4*>(stage + r * R_CPITCH + c8 * 4);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(stage + r * R_CPITCH + c8 * 4 + 16);
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] * g.alpha + bv[e];
            if (Rb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] += r0[pass][e]; v[4 + e] += r1[pass][e]; }
            }
            if (OUT_SPLIT && g.out_split) {             // uniform: the consumer is a SPLIT conv with no GroupNorm in front -- its operand planes leave from here
                unsigned hi[4], lo[4];
                split8_checked(v, hi, lo, bad);
                half_t* P = reinterpret_cast<half_t*>(g.C) + 2 * moff[pass] - nn;           // pixel * 2 N + channel (ldc == N)
                *reinterpret_cast<u32x4*>(P) = u32x4{hi[0], hi[1], hi[2], hi[3]};
                *reinterpret_cast<u32x4*>(P + g.N) = u32x4{lo[0], lo[1], lo[2], lo[3]};
            } else {
                const f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
                *reinterpret_cast<f32x4*>(Cb + moff[pass]) = o0;
                *reinterpret_cast<f32x4*>(Cb + moff[pass] + 4) = o1;
            }
            if (g.gn_part_out_d) {
                // the square is rounded, then added -- never fused: whether the compiler contracts this pair has depended on how the code
                // around it was inlined, and the GroupNorm statistics must not
#pragma clang fp contract(off)
#pragma unroll
                for (int e = 0; e < 8; ++e) { gs[e] += v[e]; const float sq = v[e] * v[e]; gq[e] += sq; }
            }
        }
    }
}
// no operand planes leave from here: nothing to range-check
template <int PASSES, class PixelOf>
__device__ __forceinline__ void ring_store_rows(const GemmArgs& g, const char* stage, int tid, int n0, const float (&bv)[8], bool active,
                                                PixelOf pixel_of, float (&gs)[8], float (&gq)[8]) {
    bool bad = false;
    ring_store_rows<PASSES, false>(g, stage, tid, n0, bv, active, pixel_of, gs, gq, bad);
}
// GroupNorm partial `part` of this workgroup (sum, sum of squares per group, double) from the per-thread sums: through LDS in a fixed
// order, then across the cpg consecutive channels = lanes of a group.  Called by the whole workgroup (g.gn_part_out_d is uniform).
__device__ __forceinline__ void ring_reduce_gn(const GemmArgs& g, char* lds_raw, int tid, const float (&gs)[8], const float (&gq)[8], int n0,
                                               bool active, long long part) {
    if (!g.gn_part_out_d) return;
    const int c8 = (tid & 15) * 8;
    __syncthreads();                                    // every staged value has been read
    float* redw = reinterpret_cast<float*>(lds_raw);    // [16 pixel rows][128 channels][2]; zeros from idle threads
    if (active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            redw[(((tid >> 4) * 128) + c8 + e) * 2] = gs[e];
            redw[(((tid >> 4) * 128) + c8 + e) * 2 + 1] = gq[e];
        }
    }
    __syncthreads();
    const float* red = reinterpret_cast<const float*>(lds_raw);
    if (active && tid < 128) {                          // one channel per thread, then its group
        double sa = 0.0, sq = 0.0;
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) { sa += (double)red[((rg * 128) + tid) * 2]; sq += (double)red[((rg * 128) + tid) * 2 + 1]; }
        const int cpg = g.N / g.gn_out_groups;
        for (int off = cpg >> 1; off > 0; off >>= 1) { sa += __shfl_xor(sa, off, 64); sq += __shfl_xor(sq, off, 64); }
        const int ch = n0 + tid;
        if (ch < g.N && (tid & (cpg - 1)) == 0) {
            double* pp = g.gn_part_out_d + (part * g.gn_out_groups + ch / cpg) * 2;
            pp[0] = sa; pp[1] = sq;
        }
    }
}
}  // namespace
