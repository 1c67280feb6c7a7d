// KV-cache attention of the HQ-Transformer sampling path (A4/K3: stage2/layers.py:93-102,183-187): six kernels behind launch_attention.
// The scale 1/sqrt(hs) is applied to K before the product, as the reference does (:102).  gfx950 only (wave = 64).
//
// The four vector kernels share one picture.  A key / value row of one head (hs elements) is read by hs/8 adjacent lanes ("chunks"),
// 8 elements (one 16-B vector in bf16) each, so every wave load covers 64 / (hs/8) whole rows: QK^T is 8 FMAs per lane plus a
// log2(hs/8)-step shuffle reduction, PV keeps 8 accumulators per lane and reduces over the row slots at the end.
//
// The helpers below are the pieces that could be shared with the generated code of every kernel unchanged.  Where a kernel still
// writes one of them out (marked "written out"), the call made hipcc schedule that kernel differently; so did every shared form of
// the lane geometry, of attention_kernel's softmax group (attention_fewq_kernel is one such group per query) and of the prefill
// kernels' V^T gather, score tile and output store.  The equalities the copies promise are held by tests/test_gpu_attention_paths.py.
#include "kernels.h"
#include "gemm_generic.h"
#include "switches.h"
#include <type_traits>

template <typename T> using raw_t = typename std::conditional<sizeof(T) == 2, uint4, float4>::type;      // 16-B vector of the cache dtype
template <typename T> constexpr int NRAW = sizeof(T) == 2 ? 1 : 2;                                        // vectors per 8 elements

// 8 elements of a q / cache row as fetched -> fp32
template <typename T> __device__ __forceinline__ void unpack_row(const raw_t<T>* r, float (&f)[8]) {
    if constexpr (sizeof(T) == 2) {
        bf16x8_to_f32(r[0], f);
    } else {
        const float4 a0 = r[0], a1 = r[1];
        f[0] = a0.x; f[1] = a0.y; f[2] = a0.z; f[3] = a0.w; f[4] = a1.x; f[5] = a1.y; f[6] = a1.z; f[7] = a1.w;
    }
}
// The lane's 8 elements of K and V row `row`, which the caller has clamped into the cache: the loads are unconditional, so all the
// fetches of a kernel are in flight at once
template <typename T> __device__ __forceinline__ void fetch_kv(const T* kc, const T* vc, long long row, int D, raw_t<T> (&k)[NRAW<T>], raw_t<T> (&v)[NRAW<T>]) {
    const raw_t<T>* ks = reinterpret_cast<const raw_t<T>*>(kc + row * D);
    const raw_t<T>* vs = reinterpret_cast<const raw_t<T>*>(vc + row * D);
#pragma unroll
    for (int e = 0; e < NRAW<T>; ++e) { k[e] = ks[e]; v[e] = vs[e]; }
}
// 8 consecutive outputs: one 16-B vector in bf16
template <typename T> __device__ __forceinline__ void store8(T* o, const float (&acc)[8]) {
    if constexpr (sizeof(T) == 2) {
        uint4 pk;
        pk.x = (unsigned)f32_to_bf16(acc[0]) | ((unsigned)f32_to_bf16(acc[1]) << 16);
        pk.y = (unsigned)f32_to_bf16(acc[2]) | ((unsigned)f32_to_bf16(acc[3]) << 16);
        pk.z = (unsigned)f32_to_bf16(acc[4]) | ((unsigned)f32_to_bf16(acc[5]) << 16);
        pk.w = (unsigned)f32_to_bf16(acc[6]) | ((unsigned)f32_to_bf16(acc[7]) << 16);
        *reinterpret_cast<uint4*>(o) = pk;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) st1<T>(o + i, acc[i]);
    }
}
// Element (row, col) of the output: the packed_off() layout, or [B * Tq, D] row-major (col a multiple of 4: the pieces stored there stay contiguous)
template <typename T> __device__ __forceinline__ T* out_at(const AttnArgs& a, int row, int col, int D) {
    return a.out_packed_mb ? reinterpret_cast<T*>(a.out) + packed_off(row, col, a.out_packed_mb)
                           : reinterpret_cast<T*>(a.out) + (long long)row * D + col;
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// The four k-step fragments (A or B operand alike) of row `row` of a K or Q tile: lane half hf holds elements 16 ks + 8 hf .. + 7
__device__ __forceinline__ void load_row_frags(const bf16_t* base, long long row, int D, int hf, bf16x8_t (&f)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = *reinterpret_cast<const bf16x8_t*>(base + row * D + 16 * ks + 8 * hf);
}
#endif

// One wave per (sample, head, query).  hs / 8 adjacent lanes ("chunks") cover one key / value row with 16-byte vectors,
// so a pass handles 64 / chunks rows and PB passes are fetched together (one memory round trip for K AND V of up to
// 64 keys at hs = 64).  Scores, probabilities and the output accumulator stay in registers: a group's score is
// xor-reduced over its chunk lanes (every lane of the group ends up with it), the running maximum / sum are reduced
// across the row slots, and further key groups are folded in with the online-softmax rescaling.  No LDS, no barriers.
template <typename T>
__global__ __launch_bounds__(256) void attention_kernel(AttnArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gid = blockIdx.x * 4 + wave;
    if (gid >= a.B * a.n_heads * a.Tq) return;
    long long stamp[5];
    if (a.dbg) stamp[0] = clock64();
    const int qi = gid % a.Tq;
    const int h = (gid / a.Tq) % a.n_heads;
    const int b = gid / (a.Tq * a.n_heads);
    const int hs = a.head_dim, D = a.n_heads * hs;
    const int chunks = hs >> 3;                  // lanes per row (power of two: hs in {8,16,32,64,128,256})
    const int rows_per_pass = 64 / chunks;
    const int c = lane % chunks, slot = lane / chunks;
    const T* q = reinterpret_cast<const T*>(a.q) + ((long long)(b * a.Tq + qi)) * D + h * hs + c * 8;
    const T* kc = reinterpret_cast<const T*>(a.kcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    const T* vc = reinterpret_cast<const T*>(a.vcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    float qv[8];
    unpack_row<T>(reinterpret_cast<const raw_t<T>*>(q), qv);                              // independent of the step state: in flight while t_base arrives
    // (a rolling pass: every sample at its own position -- the wave's key count is its own, and its arithmetic depends on nothing else)
    const int tb = a.t_base + (a.row_pos ? row_live(a.row_pos, b) : (a.t_base_dev ? *a.t_base_dev : 0));
    const int nkeys = a.causal ? tb + qi + 1 : tb + a.Tq;
    const float scale = 1.0f / sqrtf((float)hs);
    constexpr int PB = 8;                        // passes whose loads are issued together
    float run_max = -INFINITY, run_sum = 0.0f;   // identical in every lane after each group
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
    // A group is up to PB passes fetched in one round trip; the last (often the only) group runs exactly the passes it has keys for --
    // `np` is uniform over the launch, so the switch below picks a fully unrolled body.  Skipped passes contributed exp(-inf) = 0 and
    // max(-inf) before: the results are bit-identical, and a step with few cached keys no longer pays the arithmetic of 64.
    auto group = [&](int j0, auto np_tag) {
        constexpr int NP = decltype(np_tag)::value;
        raw_t<T> kbuf[NP][NRAW<T>], vbuf[NP][NRAW<T>];
#pragma unroll
        for (int p = 0; p < NP; ++p) fetch_kv<T>(kc, vc, min(j0 + p * rows_per_pass + slot, nkeys - 1), D, kbuf[p], vbuf[p]);
        __builtin_amdgcn_sched_barrier(0);
        if (a.dbg && j0 == 0) { stamp[1] = clock64(); __builtin_amdgcn_sched_barrier(0); }
        float sc[NP];
        float gmax = -INFINITY;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float kv[8];
            unpack_row<T>(kbuf[p], kv);
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(qv[i], kv[i] * scale, s);            // scale on K, as layers.py:102
            for (int off = chunks >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            sc[p] = (j0 + p * rows_per_pass + slot < nkeys) ? s : -INFINITY;
            gmax = fmaxf(gmax, sc[p]);
        }
        for (int off = chunks; off < 64; off <<= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, off, 64));     // across the row slots
        if (a.dbg && j0 == 0) stamp[2] = clock64();
        const float new_max = fmaxf(run_max, gmax);                     // finite: key j0 is always valid
        const float rescale = expf(run_max - new_max);                  // 0 for the first group (run_max = -inf)
        float gsum = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] *= rescale;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float e = expf(sc[p] - new_max);                      // 0 for masked rows
            gsum += e;
            float vv[8];
            unpack_row<T>(vbuf[p], vv);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(e, vv[i], acc[i]);
        }
        for (int off = chunks; off < 64; off <<= 1) gsum += __shfl_xor(gsum, off, 64);
        run_sum = run_sum * rescale + gsum;
        run_max = new_max;
        if (a.dbg && j0 == 0) stamp[3] = clock64();
    };
    const int npass = (nkeys + rows_per_pass - 1) / rows_per_pass;
    for (int p0 = 0; p0 < npass; p0 += PB) {
        const int j0 = p0 * rows_per_pass;
        switch (min(PB, npass - p0)) {
        case 1: group(j0, std::integral_constant<int, 1>{}); break;
        case 2: group(j0, std::integral_constant<int, 2>{}); break;
        case 3: group(j0, std::integral_constant<int, 3>{}); break;
        case 4: group(j0, std::integral_constant<int, 4>{}); break;
        case 5: group(j0, std::integral_constant<int, 5>{}); break;
        case 6: group(j0, std::integral_constant<int, 6>{}); break;
        case 7: group(j0, std::integral_constant<int, 7>{}); break;
        default: group(j0, std::integral_constant<int, 8>{}); break;
        }
    }
    for (int off = chunks; off < 64; off <<= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += __shfl_xor(acc[i], off, 64);
    const float inv = 1.0f / run_sum;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= inv;
    if (slot == 0) {
        const int row = b * a.Tq + qi, col = h * hs + c * 8;
        store8<T>(out_at<T>(a, row, col, D), acc);
    }
    if (a.dbg && lane == 0) {
        stamp[4] = clock64();
        long long* d = a.dbg + (long long)gid * 8;
        d[0] = wall_clock64(); d[1] = stamp[1] - stamp[0]; d[2] = stamp[2] - stamp[0]; d[3] = stamp[3] - stamp[0]; d[4] = stamp[4] - stamp[0];
    }
}
// Few queries over a short shared cache (depth sub-step 1: 4 queries x <= 5 keys; sub-steps of the three-level head): one wave per
// (sample, head) fetches the K / V rows ONCE and loops over the queries -- a quarter of the waves of the kernel above, whose cost at
// these sizes is the wave count (49 k waves at 512 samples: 50 us per launch for a few kilobytes of arithmetic).  Per query the same
// operations in the same order as attention_kernel with one group: bit-identical results (tests/test_gpu_attention_paths.py).
template <typename T, int NP>
__global__ __launch_bounds__(256) void attention_fewq_kernel(AttnArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gid = blockIdx.x * 4 + wave;
    if (gid >= a.B * a.n_heads) return;
    const int h = gid % a.n_heads, b = gid / a.n_heads;
    const int hs = a.head_dim, D = a.n_heads * hs;
    const int chunks = hs >> 3, rows_per_pass = 64 / chunks;
    const int c = lane % chunks, slot = lane / chunks;
    const T* kc = reinterpret_cast<const T*>(a.kcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    const T* vc = reinterpret_cast<const T*>(a.vcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    const int tb = a.t_base + (a.t_base_dev ? *a.t_base_dev : 0);
    const int nall = tb + a.Tq;                                       // keys any query of this call can see
    const float scale = 1.0f / sqrtf((float)hs);
    raw_t<T> kbuf[NP][NRAW<T>], vbuf[NP][NRAW<T>];
#pragma unroll
    for (int p = 0; p < NP; ++p) {                                    // fetch_kv, written out
        const long long j = min(p * rows_per_pass + slot, nall - 1);
        const raw_t<T>* ks = reinterpret_cast<const raw_t<T>*>(kc + j * D);
        const raw_t<T>* vs = reinterpret_cast<const raw_t<T>*>(vc + j * D);
#pragma unroll
        for (int e = 0; e < NRAW<T>; ++e) { kbuf[p][e] = ks[e]; vbuf[p][e] = vs[e]; }
    }
    for (int qi = 0; qi < a.Tq; ++qi) {
        const int nkeys = a.causal ? tb + qi + 1 : nall;
        float qv[8];
        unpack_row<T>(reinterpret_cast<const raw_t<T>*>(reinterpret_cast<const T*>(a.q) + ((long long)(b * a.Tq + qi)) * D + h * hs + c * 8), qv);
        float sc[NP], gmax = -INFINITY;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float kv[8];
            unpack_row<T>(kbuf[p], kv);
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(qv[i], kv[i] * scale, s);            // scale on K, as layers.py:102
            for (int off = chunks >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            sc[p] = (p * rows_per_pass + slot < nkeys) ? s : -INFINITY;
            gmax = fmaxf(gmax, sc[p]);
        }
        for (int off = chunks; off < 64; off <<= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, off, 64));
        const float new_max = fmaxf(-INFINITY, gmax);
        const float rescale = expf(-INFINITY - new_max);                // 0: one group, as the first group of attention_kernel
        float gsum = 0.0f, acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.0f * rescale;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float e = expf(sc[p] - new_max);
            gsum += e;
            float vv[8];
            unpack_row<T>(vbuf[p], vv);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(e, vv[i], acc[i]);
        }
        for (int off = chunks; off < 64; off <<= 1) gsum += __shfl_xor(gsum, off, 64);
        const float run_sum = 0.0f * rescale + gsum;
        for (int off = chunks; off < 64; off <<= 1)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += __shfl_xor(acc[i], off, 64);
        const float inv = 1.0f / run_sum;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] *= inv;
        if (slot == 0) {
            const int row = b * a.Tq + qi, col = h * hs + c * 8;
            store8<T>(out_at<T>(a, row, col, D), acc);
        }
    }
}

// Causal prefill of the text prompt (stage2/layers.py:107-111: every prompt token attends to itself and its predecessors), FAST
// precision, head size 64, up to 64 tokens: ONE wave per (sample, head) computes the whole T x T attention on the matrix cores
// instead of one wave per query re-reading the keys.
//   S^T = K Q^T   (v_mfma_f32_32x32x16_bf16; A = K rows, B = Q rows: both fragments are 16 contiguous bytes of a cache / q row, loaded
//                  straight from memory -- every K, Q, V element is fetched exactly once per (sample, head))
// leaves the scores of a query in ONE lane (column = query, the 16 registers of a tile = keys), so the causal mask, the maximum and
// the sum of the softmax are register loops plus one cross-half shuffle.  The probabilities then serve, converted to bf16 in place,
// as the B operand of
//   O^T = V^T P^T (A = V^T: element j of lane half h in k-step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3), the order in which the
//                  accumulator registers hold P -- cdna_hip_programming.md, 'An accumulator tile as the next MFMA's operand')
// Key tiles above the diagonal are skipped.  Outputs leave as 8-byte pieces of a row (4 consecutive head dimensions per register quad).
template <int NT>
__global__ __launch_bounds__(256) void attention_prefill_mfma_kernel(AttnArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gid = blockIdx.x * 4 + wave;
    if (gid >= a.B * a.n_heads) return;
    const int h = gid % a.n_heads, b = gid / a.n_heads;
    const int D = a.n_heads * 64, T = a.Tq;
    const int r = lane & 31, hf = lane >> 5;
    const bf16_t* qb = reinterpret_cast<const bf16_t*>(a.q) + (long long)b * T * D + h * 64;
    const bf16_t* kb = reinterpret_cast<const bf16_t*>(a.kcache) + (long long)b * a.Tmax * D + h * 64;
    const bf16_t* vb = reinterpret_cast<const bf16_t*>(a.vcache) + (long long)b * a.Tmax * D + h * 64;
    bf16x8_t kf[NT][4], qf[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const long long row = min(32 * t + r, T - 1);                 // clamped: rows beyond the prompt repeat its last token and are masked / not stored
        load_row_frags(kb, row, D, hf, kf[t]);
        load_row_frags(qb, row, D, hf, qf[t]);
    }
    // V^T fragments: element j <- V[key(kt, s, hf, j)][32 dt + r]; all loads in flight while the scores are computed
    unsigned short vraw[2][NT][2][8];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long long key = min(32 * kt + 16 * s2 + 8 * (j >> 2) + 4 * hf + (j & 3), T - 1);
                    vraw[dt][kt][s2][j] = vb[key * D + 32 * dt + r];
                }
    const float scale = 1.0f / sqrtf(64.0f);
    float inv_sum[NT];
    bf16x8_t pf[NT][NT][2];                                           // [key tile][query tile][k-step]: P^T as the B operand
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
        f32x16_t sc[NT];
        const int q = 32 * qt + r;
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt <= qt; ++kt) {
            f32x16_t acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kt][ks], qf[qt][ks], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = 32 * kt + (i & 3) + 8 * (i >> 2) + 4 * hf;
                const float v = key <= q ? acc[i] * scale : -INFINITY;
                acc[i] = v;
                m = fmaxf(m, v);
            }
            sc[kt] = acc;
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));                          // the other half of this query's keys; finite: key 0 is always visible
        float sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt <= qt; ++kt) {
            float e[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { e[i] = __expf(sc[kt][i] - m); sum += e[i]; }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8_t f;
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = (__bf16)e[8 * s2 + j];
                pf[kt][qt][s2] = f;
            }
        }
        sum += __shfl_xor(sum, 32, 64);
        inv_sum[qt] = 1.0f / sum;
    }
    const int row_base = b * T;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        bf16x8_t vf[NT][2];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                            u16x8_t raw;
#pragma unroll
                for (int j = 0; j < 8; ++j) raw[j] = vraw[dt][kt][s2][j];
                vf[kt][s2] = __builtin_bit_cast(bf16x8_t, raw);
            }
#pragma unroll
        for (int qt = 0; qt < NT; ++qt) {
            f32x16_t o;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] = 0.0f;
#pragma unroll
            for (int kt = 0; kt <= qt; ++kt)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kt][s2], pf[kt][qt][s2], o, 0, 0, 0);
            const int q = 32 * qt + r;
            if (q < T) {
                const int row = row_base + q;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int col = h * 64 + 32 * dt + 8 * g4 + 4 * hf;
                    bf16_t* dst = out_at<bf16_t>(a, row, col, D);
                    uint2 pk;
                    pk.x = (unsigned)f32_to_bf16(o[4 * g4] * inv_sum[qt]) | ((unsigned)f32_to_bf16(o[4 * g4 + 1] * inv_sum[qt]) << 16);
                    pk.y = (unsigned)f32_to_bf16(o[4 * g4 + 2] * inv_sum[qt]) | ((unsigned)f32_to_bf16(o[4 * g4 + 3] * inv_sum[qt]) << 16);
                    *reinterpret_cast<uint2*>(dst) = pk;
                }
            }
        }
    }
#endif
}

// Causal prefill of any row count (the text prompt followed by a code prefix: more than 64 rows per sample), FAST precision, head size 64,
// nothing cached before it: ONE wave per (sample, head, 32-query tile) walks the key tiles kt = 0 .. qt with the two products and operand
// orders of attention_prefill_mfma_kernel -- S^T = K Q^T leaves a query's scores in one lane, O^T = V^T P^T takes the probabilities,
// converted in place, as its B operand -- and an online softmax: running maximum and (per lane half) running sum of each query, the two O
// accumulator tiles rescaled per key tile.  A lane's column of S^T and of O^T is its query, so the rescale is lane-local.  What a wave holds
// does not depend on T: one Q tile, one K tile, one V tile pair (strided 2-byte loads, issued before the scores are computed), two
// accumulators.  Rows beyond T are clamped on load (they repeat the last row), masked in the scores of every valid query (key <= query < T)
// and never stored; key tiles above the diagonal are never visited; the diagonal tile is masked element-wise.
__global__ __launch_bounds__(256) void attention_prefill_tiled_kernel(AttnArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int T = a.Tq, nqt = (T + 31) / 32;
    const int gid = blockIdx.x * 4 + wave;
    if (gid >= a.B * a.n_heads * nqt) return;                         // idle waves of the last workgroup (no workgroup-wide step follows)
    const int qt = nqt - 1 - gid % nqt, bh = gid / nqt;               // the longest walks of a (sample, head) first
    const int h = bh % a.n_heads, b = bh / a.n_heads;
    const int D = a.n_heads * 64;
    const int r = lane & 31, hf = lane >> 5;
    const bf16_t* qb = reinterpret_cast<const bf16_t*>(a.q) + (long long)b * T * D + h * 64;
    const bf16_t* kb = reinterpret_cast<const bf16_t*>(a.kcache) + (long long)b * a.Tmax * D + h * 64;
    const bf16_t* vb = reinterpret_cast<const bf16_t*>(a.vcache) + (long long)b * a.Tmax * D + h * 64;
    const int q = 32 * qt + r;
    bf16x8_t qf[4];
    {                                                                 // load_row_frags, written out
        const long long row = min(q, T - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qb + row * D + 16 * ks + 8 * hf);
    }
    const float scale = 1.0f / sqrtf(64.0f);
    f32x16_t o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.0f;
    float m = -INFINITY, sum = 0.0f;                                  // m: over all keys of the query (both lane halves agree); sum: this half's keys
    for (int kt = 0; kt <= qt; ++kt) {
        bf16x8_t kf[4];
        load_row_frags(kb, min(32 * kt + r, T - 1), D, hf, kf);
        // V^T fragments: element j <- V[key(kt, s2, hf, j)][32 dt + r], the order in which the accumulator registers hold P
        u16x8_t vraw[2][2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long long key = min(32 * kt + 16 * s2 + 8 * (j >> 2) + 4 * hf + (j & 3), T - 1);
                    vraw[dt][s2][j] = vb[key * D + 32 * dt + r];
                }
        f32x16_t sc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], sc, 0, 0, 0);
        float tmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = 32 * kt + (i & 3) + 8 * (i >> 2) + 4 * hf;
            const float v = key <= q ? sc[i] * scale : -INFINITY;     // masks only in the diagonal tile
            sc[i] = v;
            tmax = fmaxf(tmax, v);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));                 // the other half of this tile's keys; finite: key 32 kt <= q is visible
        const float m_new = fmaxf(m, tmax);
        const float alpha = __expf(m - m_new);                        // 0 in the first tile (m = -inf)
        m = m_new;
        sum *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
        bf16x8_t pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float e = __expf(sc[8 * s2 + j] - m);           // 0 for masked keys
                sum += e;
                pf[s2][j] = (__bf16)e;
            }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, vraw[dt][s2]), pf[s2], o[dt], 0, 0, 0);
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv_sum = 1.0f / sum;
    if (q < T) {
        const int row = b * T + q;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int col = h * 64 + 32 * dt + 8 * g4 + 4 * hf;
                bf16_t* dst = out_at<bf16_t>(a, row, col, D);
                uint2 pk;
                pk.x = (unsigned)f32_to_bf16(o[dt][4 * g4] * inv_sum) | ((unsigned)f32_to_bf16(o[dt][4 * g4 + 1] * inv_sum) << 16);
                pk.y = (unsigned)f32_to_bf16(o[dt][4 * g4 + 2] * inv_sum) | ((unsigned)f32_to_bf16(o[dt][4 * g4 + 3] * inv_sum) << 16);
                *reinterpret_cast<uint2*>(dst) = pk;
            }
    }
#endif
}

// The same few-query case with head size 64 and at most 8 keys (depth sub-step 1: 4 queries x 5 keys), from 64 samples: EIGHT heads per
// wave.  A head is the 8 lanes that cover one 128-byte key / value row, and all its keys sit in that group's registers, so a wave holds
// 8 x (NK keys + NK values + Tq queries) x 16 bytes in flight instead of one head's, an eighth of the waves are dispatched (at 2048
// samples 6 144 instead of 49 152: the launch was paced by occupancy rounds of one-round-trip waves; 73.6 -> 21.2 us, 8.0 -> 5.3 us at 64
// samples: tools/micro/bench_attn), and every lane stores.  Scores, maxima and exponentials are the very operations of attention_fewq_kernel; the sums over the keys are taken in the
// order of its cross-lane tree (slot ^ 1, ^ 2, ^ 4), so the results are bit-identical (tests/test_gpu_attention_paths.py).
template <typename T, int NK, int TQ>
__global__ __launch_bounds__(256) void attention_fewq8_kernel(AttnArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gid = (blockIdx.x * 4 + wave) * 8 + (lane >> 3);          // (sample, head) of this 8-lane group
    const bool live = gid < a.B * a.n_heads;
    const int g = live ? gid : a.B * a.n_heads - 1;
    const int h = g % a.n_heads, b = g / a.n_heads, c = lane & 7;
    constexpr int hs = 64;
    const int D = a.n_heads * hs;
    const T* kc = reinterpret_cast<const T*>(a.kcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    const T* vc = reinterpret_cast<const T*>(a.vcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    const T* qp = reinterpret_cast<const T*>(a.q) + (long long)b * a.Tq * D + h * hs + c * 8;
    raw_t<T> kbuf[NK][NRAW<T>], vbuf[NK][NRAW<T>], qbuf[TQ][NRAW<T>];
#pragma unroll
    for (int j = 0; j < NK; ++j) fetch_kv<T>(kc, vc, j, D, kbuf[j], vbuf[j]);
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) {
        const raw_t<T>* qs = reinterpret_cast<const raw_t<T>*>(qp + (long long)min(qi, a.Tq - 1) * D);
#pragma unroll
        for (int e = 0; e < NRAW<T>; ++e) qbuf[qi][e] = qs[e];
    }
    const float scale = 0.125f;                                        // 1 / sqrt(64), exact
    float kf[NK][8];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        unpack_row<T>(kbuf[j], kf[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[j][i] *= scale;                 // scale on K, as layers.py:102
    }
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) {
        if (qi >= a.Tq) break;
        const int nkeys = a.causal ? a.t_base + qi + 1 : a.t_base + a.Tq;
        float qv[8];
        unpack_row<T>(qbuf[qi], qv);
        float sc[8], gmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sc[j] = -INFINITY;
            if (j < NK) {
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < 8; ++i) s = fmaf(qv[i], kf[j][i], s);
                s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
                if (j < nkeys) sc[j] = s;
            }
            gmax = fmaxf(gmax, sc[j]);
        }
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = j < NK ? expf(sc[j] - gmax) : 0.0f;      // 0 for masked keys
        const float run_sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
        const float inv = 1.0f / run_sum;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = 0.0f;
#pragma unroll
            for (int j = 0; j < NK; ++j) {
                float vv[8];
                unpack_row<T>(vbuf[j], vv);
                p[j] = fmaf(e[j], vv[i], 0.0f);
            }
            acc[i] = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) * inv;
        }
        if (live) {
            const int row = b * a.Tq + qi, col = h * hs + c * 8;
            store8<T>(out_at<T>(a, row, col, D), acc);
        }
    }
}
// One query per sample over the body's KV cache (a decode step of the AR loop), head size 64, bf16: EIGHT heads per wave, like
// attention_fewq8_kernel.  The 8 lanes of a head walk its keys in chunks of CH rows (K and V of a chunk in flight together; chunk
// i + 1 is fetched before the work on chunk i), scores by 8 FMAs and a 3-step shuffle inside the lane group, online softmax
// across chunks in registers, every lane stores its 8 outputs.  Against attention_kernel (one head per wave, 8 keys per pass across the
// lane groups) a launch dispatches an eighth of the waves -- with one key cached that kernel took 14 us at 512 samples and 57 us at
// 2048 for 3 / 12 MB: occupancy rounds of one-round-trip waves, under every launch of the pass -- and a key row of 8 neighbouring heads
// is one contiguous kilobyte.  The sums run over the keys in index order (attention_kernel: a tree across lane groups), so results
// differ from that kernel's in the last bits (FAST passes only: see launch_attention).
__global__ __launch_bounds__(256) void attention_heads8_kernel(AttnArgs a) {
    typedef bf16_t T;
    constexpr int hs = 64, CH = 8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gid = (blockIdx.x * 4 + wave) * 8 + (lane >> 3);
    const bool live = gid < a.B * a.n_heads;
    const int g = live ? gid : a.B * a.n_heads - 1;
    const int h = g % a.n_heads, b = g / a.n_heads, c = lane & 7;
    const int D = a.n_heads * hs;
    const T* kc = reinterpret_cast<const T*>(a.kcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    const T* vc = reinterpret_cast<const T*>(a.vcache) + (long long)b * a.Tmax * D + h * hs + c * 8;
    raw_t<T> qraw[NRAW<T>];
    {
        const raw_t<T>* qs = reinterpret_cast<const raw_t<T>*>(reinterpret_cast<const T*>(a.q) + (long long)b * D + h * hs + c * 8);
#pragma unroll
        for (int e = 0; e < NRAW<T>; ++e) qraw[e] = qs[e];                 // independent of the step state: in flight while t_base arrives
    }
    // Tq == 1: causal or not, the query sees every cached key and itself.  A rolling pass: the key count is per sample, i.e. per 8-lane group -- the groups
    // of a wave leave the chunk loop at different trips, and every shuffle below stays inside one group
    const int nkeys = a.t_base + (a.row_pos ? row_live(a.row_pos, b) : (a.t_base_dev ? *a.t_base_dev : 0)) + 1;
    raw_t<T> kb[2][CH][NRAW<T>], vb[2][CH][NRAW<T>];
    auto fetch = [&](int j0, int slot) {
#pragma unroll
        for (int p = 0; p < CH; ++p) fetch_kv<T>(kc, vc, min(j0 + p, nkeys - 1), D, kb[slot][p], vb[slot][p]);
    };
    float qv[8];
    float run_max = -INFINITY, run_sum = 0.0f, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
    auto work = [&](int j0, int slot) {
        float sc[CH], cmax = -INFINITY;
#pragma unroll
        for (int p = 0; p < CH; ++p) {
            float kv[8];
            unpack_row<T>(kb[slot][p], kv);
            float sdot = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) sdot = fmaf(qv[i], kv[i] * 0.125f, sdot);     // scale 1 / sqrt(64) on K, as layers.py:102
            sdot += __shfl_xor(sdot, 4, 64); sdot += __shfl_xor(sdot, 2, 64); sdot += __shfl_xor(sdot, 1, 64);
            sc[p] = (j0 + p < nkeys) ? sdot : -INFINITY;
            cmax = fmaxf(cmax, sc[p]);
        }
        const float new_max = fmaxf(run_max, cmax);                     // finite: key j0 is valid
        const float rescale = expf(run_max - new_max);                  // 0 for the first chunk
        run_sum *= rescale;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] *= rescale;
#pragma unroll
        for (int p = 0; p < CH; ++p) {
            const float e = expf(sc[p] - new_max);                      // 0 for masked rows
            run_sum += e;
            float vv[8];
            unpack_row<T>(vb[slot][p], vv);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(e, vv[i], acc[i]);
        }
        run_max = new_max;
    };
    fetch(0, 0);
    unpack_row<T>(qraw, qv);
    for (int j0 = 0; j0 < nkeys; j0 += 2 * CH) {                        // two chunks per trip: static register slots
        if (j0 + CH < nkeys) fetch(j0 + CH, 1);
        work(j0, 0);
        if (j0 + CH >= nkeys) break;
        if (j0 + 2 * CH < nkeys) fetch(j0 + 2 * CH, 0);
        work(j0 + CH, 1);
    }
    const float inv = 1.0f / run_sum;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= inv;
    if (live) {
        const int col = h * hs + c * 8;
        store8<T>(out_at<T>(a, b, col, D), acc);
    }
}
template <typename T>
static hipError_t launch_fewq8(const AttnArgs& a, hipStream_t st) {
    const int groups = a.B * a.n_heads, grid = (groups + 31) / 32;
    switch (a.t_base + a.Tq) {
    case 2: attention_fewq8_kernel<T, 2, 4><<<grid, 256, 0, st>>>(a); break;
    case 3: attention_fewq8_kernel<T, 3, 4><<<grid, 256, 0, st>>>(a); break;
    case 4: attention_fewq8_kernel<T, 4, 4><<<grid, 256, 0, st>>>(a); break;
    case 5: attention_fewq8_kernel<T, 5, 4><<<grid, 256, 0, st>>>(a); break;
    case 6: attention_fewq8_kernel<T, 6, 4><<<grid, 256, 0, st>>>(a); break;
    case 7: attention_fewq8_kernel<T, 7, 4><<<grid, 256, 0, st>>>(a); break;
    default: attention_fewq8_kernel<T, 8, 4><<<grid, 256, 0, st>>>(a); break;
    }
    return hipGetLastError();
}

// The one choice of kernel for a call (kernels.h): launch_attention switches on it, run_block reports it.
AttnKernel attention_choice(const AttnArgs& a) {
    const int chunks = a.head_dim / 8;
    if (a.head_dim % 8 != 0 || chunks > 64 || (chunks & (chunks - 1)) != 0) return ATTN_INVALID;
    // few queries over a cache known on the host to fit one pass (depth sub-steps): one wave per (sample, head), see attention_fewq_kernel
    if (a.Tq > 1 && a.Tq <= 16 && !a.t_base_dev && !a.dbg && a.t_base + a.Tq <= 2 * (64 / chunks)) {
        if (!switch_value(SW_NO_FEWQ_ATTN)) {                                   // A/B switch
            // head size 64, <= 4 queries over <= 8 keys, 64+ samples: eight heads per wave (attention_fewq8_kernel; HQT_NO_FEWQ8=1: A/B switch)
            const bool off8 = switch_value(SW_NO_FEWQ8);
            if (!off8 && a.head_dim == 64 && a.Tq <= 4 && a.t_base + a.Tq <= 8 && a.B >= 64) return ATTN_FEWQ8;
            return a.t_base + a.Tq <= 64 / chunks ? ATTN_FEWQ1 : ATTN_FEWQ2;
        }
    }
    // causal prefill of a whole prompt (bf16, head size 64, nothing cached before it) on the matrix cores: up to 64 rows per sample one wave
    // per (sample, head) with the whole problem in registers, above that one wave per 32-query tile (attention_prefill_tiled_kernel).
    // HQT_PREFILL_TILED=1 (test hook, read per launch so that one process can compare the two): the tiled kernel from 5 rows on
    const bool prefill = a.causal && a.dtype == DT_BF16 && a.head_dim == 64 && a.Tq > 4 && a.t_base == 0 && !a.t_base_dev && !a.dbg && (a.n_heads * 64) % 8 == 0;
    if (prefill) return a.Tq > 64 || switch_value(SW_PREFILL_TILED) ? ATTN_PREFILL_TILED : ATTN_PREFILL_MFMA;      // (MFMA: 4 < Tq <= 64)
    // one query per sample, head size 64 (the decode steps of a merged FAST pass): eight heads per wave (HQT_NO_HEADS8=1: A/B switch)
    const bool no_h8 = switch_value(SW_NO_HEADS8);
    // FAST only, from 256 samples: below that the launch is a handful of waves and the chunk-by-chunk walk loses to attention_kernel's
    // single round trip from 32 keys on (64 samples x 64 keys: 19.1 vs 9.3 us); EXACT keeps ONE kernel for every row count, so that a
    // row's draws do not depend on the pass it sits in (hqt.h: merged steps).
    if (!no_h8 && a.Tq == 1 && a.head_dim == 64 && !a.dbg && a.dtype == DT_BF16 && a.B >= 256) return ATTN_HEADS8;
    return ATTN_GENERIC;
}
const char* attention_kernel_name(AttnKernel k) {
    static const char* const names[] = {"invalid", "fewq1", "fewq2", "fewq8", "prefill_mfma", "prefill_tiled", "heads8", "generic"};
    return names[k];
}

hipError_t launch_attention(const AttnArgs& a, hipStream_t st) {
    const int g2 = (a.B * a.n_heads + 3) / 4;                         // one wave per (sample, head)
    switch (attention_choice(a)) {
    case ATTN_INVALID: return hipErrorInvalidValue;
    case ATTN_FEWQ8: return a.dtype == DT_BF16 ? launch_fewq8<bf16_t>(a, st) : launch_fewq8<float>(a, st);
    case ATTN_FEWQ1:
        if (a.dtype == DT_BF16) attention_fewq_kernel<bf16_t, 1><<<g2, 256, 0, st>>>(a);
        else attention_fewq_kernel<float, 1><<<g2, 256, 0, st>>>(a);
        break;
    case ATTN_FEWQ2:
        if (a.dtype == DT_BF16) attention_fewq_kernel<bf16_t, 2><<<g2, 256, 0, st>>>(a);
        else attention_fewq_kernel<float, 2><<<g2, 256, 0, st>>>(a);
        break;
    case ATTN_PREFILL_TILED: {
        if (a.Tq > a.Tmax) return hipErrorInvalidValue;
        const long long waves = (long long)a.B * a.n_heads * ((a.Tq + 31) / 32);
        attention_prefill_tiled_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(a);
        break;
    }
    case ATTN_PREFILL_MFMA:
        if (a.Tq <= 32) attention_prefill_mfma_kernel<1><<<g2, 256, 0, st>>>(a);
        else attention_prefill_mfma_kernel<2><<<g2, 256, 0, st>>>(a);
        break;
    case ATTN_HEADS8:
        attention_heads8_kernel<<<(a.B * a.n_heads + 31) / 32, 256, 0, st>>>(a);
        break;
    case ATTN_GENERIC: {
        const int grid = (a.B * a.n_heads * a.Tq + 3) / 4;
        if (a.dtype == DT_BF16) attention_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
        else attention_kernel<float><<<grid, 256, 0, st>>>(a);
        break;
    }
    }
    return hipGetLastError();
}
