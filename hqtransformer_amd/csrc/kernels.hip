// Small kernels of the HQ-Transformer sampling path: embeddings, LayerNorm, the fused sampler, codebook
// gather, GroupNorm statistics (KV-cache attention: attention.hip).  gfx950 only (wave = 64).
#include "kernels.h"
#include "switches.h"
#include <mutex>
#include "gemm_generic.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// reductions (256-thread workgroups = 4 waves), deterministic for a fixed launch shape
// ---------------------------------------------------------------------------------------------
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* scratch /* >= blockDim.x / 64 */) {
    v = wave_reduce(v, op);
    const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[wid] = v;
    __syncthreads();
    T r = scratch[0];
    for (int i = 1; i < nw; ++i) r = op(r, scratch[i]);
    return r;
}
struct OpAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpMin { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };

// Writes the bf16 copy of one fp32 row into the packed_off() layout and its (sum, sumsq) -- computed on the rounded
// values, which is what the MFMA will multiply -- for the deferred-LayerNorm GEMMs.  Called by all 256 threads.
__device__ __forceinline__ void emit_packed_row(const float* x, int m, int D, bf16_t* xpk, int pk_mb, float* parts, float* red) {
    float s = 0.0f, q = 0.0f;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const bf16_t hb = f32_to_bf16(x[d]);
        xpk[packed_off(m, d, pk_mb)] = hb;
        const float r = bf16_to_f32(hb);
        s += r; q += r * r;
    }
    s = block_reduce(s, OpAdd(), red);
    q = block_reduce(q, OpAdd(), red);
    if (threadIdx.x == 0) { parts[2 * m] = s; parts[2 * m + 1] = q; }
}

// ---------------------------------------------------------------------------------------------
// step state
// ---------------------------------------------------------------------------------------------
__global__ void advance_step_kernel(StepState* s, int d_tbase) { s->step += 1; s->t_base += d_tbase; }
__global__ void set_step_kernel(StepState* s, int step, int t_base) { s->step = step; s->t_base = t_base; }
__global__ void set_rows_kernel(RowKey* rows, int B, unsigned long long seed, long long sample_offset) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { rows[b].seed = seed; rows[b].global_row = sample_offset + b; }
}
hipError_t launch_set_rows(RowKey* rows, int B, uint64_t seed, int64_t sample_offset, hipStream_t st) {
    set_rows_kernel<<<(B + 255) / 256, 256, 0, st>>>(rows, B, (unsigned long long)seed, (long long)sample_offset);
    return hipGetLastError();
}
hipError_t launch_advance_step(StepState* s, int d_tbase, hipStream_t st) {
    advance_step_kernel<<<1, 1, 0, st>>>(s, d_tbase);
    return hipGetLastError();
}
// Rolling pass, between two steps of a call: every live row moves on by one position; a row that has just drawn its last one (n_steps - 1) turns idle
__global__ void advance_rows_kernel(int* row_pos, int B, int n_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int p = row_pos[b];
    if (p >= 0) row_pos[b] = p + 1 < n_steps ? p + 1 : -1;
}
hipError_t launch_advance_rows(int* row_pos, int B, int n_steps, hipStream_t st) {
    advance_rows_kernel<<<(B + 255) / 256, 256, 0, st>>>(row_pos, B, n_steps);
    return hipGetLastError();
}
hipError_t launch_set_step(StepState* s, int step, int t_base, hipStream_t st) {
    set_step_kernel<<<1, 1, 0, st>>>(s, step, t_base);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// A3/K1: input embedding of one top position (hierarchical_ar.py:493-544)
// ---------------------------------------------------------------------------------------------
// Body input row `step` of sample b: the sos row (step 0), else the embedding of position step - 1's codes with pos_emb_top[step - 1].
// The ONE place that does this arithmetic: the decode step and the prefix prefill both call it, so a row is bit-identical whichever wrote it.
__device__ __forceinline__ void embed_row(const EmbedArgs& a, int b, int step, float* x) {
    const int D = a.D;
    if (step == 0) {
        const float* src = a.cond_type == 1 ? a.sos + clamp_idx(a.cond[b], a.n_classes) * (long long)D : a.sos;
        for (int d = threadIdx.x; d < D; d += blockDim.x) x[d] = src[d];
        return;
    }
    const int p = step - 1;
    const long long ct = clamp_idx(a.codes_top[(long long)b * a.n_steps + p], a.V);
    long long cb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) cb[s] = clamp_idx(a.codes_bot[((long long)b * a.n_steps + p) * 4 + s], a.V);
    if (a.embedding == 1) {                      // 'reduce': channel k*4+slot of the bottom part (:522-526)
        const int Dq = D / 4;
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            const float top = a.tok_top[ct * D + d] + a.pos_top[(long long)p * D + d];
            x[d] = top + a.tok_bot[cb[d & 3] * Dq + (d >> 2)];
        }
    } else if (a.levels == 3) {                  // three levels: mean over the 21 tokens (hqtransformer.py:466-488)
        long long c2[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) c2[k] = clamp_idx(a.codes_l2[((long long)b * a.n_steps + p) * 16 + k], a.V);
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            float s = (a.tok_top[ct * D + d] + a.pos_top[(long long)p * D + d]) + a.pos_emb[d];
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a.tok_bot[cb[k] * D + d] + a.pos_emb[(1 + k) * D + d];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += a.tok_l2[c2[k] * D + d] + a.pos_emb[(5 + k) * D + d];
            x[d] = s / 21.0f;
        }
    } else {                                     // 'transformer1': mean over the 5 tokens (:535-544)
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            float s = (a.tok_top[ct * D + d] + a.pos_top[(long long)p * D + d]) + a.pos_emb[d];
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a.tok_bot[cb[k] * D + d] + a.pos_emb[(1 + k) * D + d];
            x[d] = s / 5.0f;
        }
    }
}

__global__ __launch_bounds__(256) void embed_step_kernel(EmbedArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    float* x = a.x + (long long)b * a.D;
    // an idle row of a rolling pass (workgroup-uniform) has no input: zeros, without a read of sos (NULL on a text handle), cond or the codes
    if (row_idle(a.row_pos, b)) { for (int d = threadIdx.x; d < a.D; d += blockDim.x) x[d] = 0.0f; }
    else embed_row(a, b, step_of(a.state, a.row_pos, b), x);
    if (a.xpk) { __syncthreads(); emit_packed_row(x, b, a.D, a.xpk, a.pk_mb, a.parts, red); }
}
hipError_t launch_embed_step(const EmbedArgs& a, hipStream_t st) {
    embed_step_kernel<<<a.B, 256, 0, st>>>(a);
    return hipGetLastError();
}

// Prefix prefill: `rows` body input rows of every sample in one launch, x[b * stride + row_off + j] = embed_row(b, step_off + j), j < rows.
// Class-conditional / unconditional (stride = rows = P + 1, no offsets): row 0 the sos row, row j the input the decode step at position j
// would have computed from the codes of position j - 1 (a.codes_*: the handle's code buffers, which hold the prefix).  Text (stride = T + P,
// row_off = T, step_off = 1, rows = P): the rows behind the prompt rows embed_text_kernel wrote.  One workgroup per row; no packed copy
// (the prefill pass takes the classic LayerNorm path).
__global__ __launch_bounds__(256) void embed_prefix_kernel(EmbedArgs a, int rows, int stride, int row_off, int step_off) {
    const int b = blockIdx.x / rows, j = blockIdx.x - b * rows;
    embed_row(a, b, step_off + j, a.x + ((long long)b * stride + row_off + j) * a.D);
}
hipError_t launch_embed_prefix(const EmbedArgs& a, int rows, int stride, int row_off, int step_off, hipStream_t st) {
    // (embed_row reads the codes of position step - 1 < n_steps)
    if (rows < 1 || row_off < 0 || step_off < 0 || row_off + rows > stride || step_off + rows > a.n_steps || a.xpk) return hipErrorInvalidValue;
    embed_prefix_kernel<<<a.B * rows, 256, 0, st>>>(a, rows, stride, row_off, step_off);
    return hipGetLastError();
}

// The gathered sibling (the join phase of a rolling pass: hqt_set_join_run): only the rows that join take part, and their body rows are packed by group.  Row b with
// g = group_of_row[b] in [0, G) writes x[g * stride + row_off + j] = embed_row(b, step_off + j), reading cond[b] and the codes of ITS row of a.codes_*; every other row
// (group -1: mid-image, or an empty slot) reads and writes nothing.
__global__ __launch_bounds__(256) void embed_prefix_rows_kernel(EmbedArgs a, const int* group_of_row, int G, int rows, int stride, int row_off, int step_off) {
    const int b = blockIdx.x / rows, j = blockIdx.x - b * rows;
    if (b >= a.B) return;
    const int g = group_of_row[b];
    if (g < 0 || g >= G) return;
    embed_row(a, b, step_off + j, a.x + ((long long)g * stride + row_off + j) * a.D);
}
hipError_t launch_embed_prefix_rows(const EmbedArgs& a, const int* group_of_row, int G, int rows, int stride, int row_off, int step_off, hipStream_t st) {
    if (a.B < 1 || G < 1 || G > a.B || !group_of_row || !a.x) return hipErrorInvalidValue;
    if (rows < 1 || row_off < 0 || step_off < 0 || row_off + rows > stride || step_off + rows > a.n_steps || a.xpk) return hipErrorInvalidValue;
    embed_prefix_rows_kernel<<<a.B * rows, 256, 0, st>>>(a, group_of_row, G, rows, stride, row_off, step_off);
    return hipGetLastError();
}

// The prefix codes of one level, [B, P, width], into the first P positions of the handle's [B, n_steps, width] code buffer (clamped into
// the vocabulary like every index that arrives from the caller)
__global__ __launch_bounds__(256) void copy_prefix_kernel(const int64_t* src, int64_t* dst, long long n, int per_sample, int dst_per_sample, int V) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per_sample, r = i - b * per_sample;
    dst[b * dst_per_sample + r] = clamp_idx(src[i], V);
}
hipError_t launch_copy_prefix(const int64_t* src, int64_t* dst, int B, int P, int n_steps, int width, int V, hipStream_t st) {
    if (P < 1 || P > n_steps) return hipErrorInvalidValue;
    const long long n = (long long)B * P * width;
    copy_prefix_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, dst, n, P * width, n_steps * width, V);
    return hipGetLastError();
}

// The kept codes of one level (hqt_set_keep_mask): both buffers are [B, n_steps, width]; entry i belongs to (sample, position) i / width
__global__ __launch_bounds__(256) void copy_kept_kernel(const int64_t* src, int64_t* dst, const unsigned char* keep, long long n, int width, int V) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (keep[i / width]) dst[i] = clamp_idx(src[i], V);
}
hipError_t launch_copy_kept(const int64_t* src, int64_t* dst, const unsigned char* keep, int B, int n_steps, int width, int V, hipStream_t st) {
    if (B < 1 || n_steps < 1 || width < 1 || !keep) return hipErrorInvalidValue;
    const long long n = (long long)B * n_steps * width;
    copy_kept_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, dst, keep, n, width, V);
    return hipGetLastError();
}

// The per-row-span sibling (a rolling pass that takes a keep table: hqt_set_join_run): row b scatters only the kept positions of the span it advances over in this
// call, [pos[b], pos[b] + (pos[b] == 0 ? k0 : k)) clipped to n_steps -- k0 >= k: a row that joins through a join phase passes its prefilled run too.  `pos` is the table
// as the call received it (device, [B]); a row with pos[b] < 0 (an empty slot) and every position outside the span are neither read nor written, in mask, src or dst.
// One thread per unit of UNIT codes of a (row, span position): two (one 16-byte vector) where the width is even and both pointers are 16-byte aligned, else one.
template <int UNIT>
__global__ __launch_bounds__(256) void copy_kept_rows_kernel(const int64_t* src, int64_t* dst, const unsigned char* keep, const int* pos, long long n, int k, int k0,
                                                             int width, int n_steps, int V) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int units = width / UNIT;
    const long long per_row = (long long)k0 * units;
    const long long b = i / per_row, r = i - b * per_row;
    const int j = (int)(r / units), u = (int)(r - (long long)j * units);
    const int p0 = pos[b];
    if (p0 < 0 || j >= (p0 == 0 ? k0 : k)) return;
    const int p = p0 + j;
    if (p >= n_steps || !keep[b * n_steps + p]) return;
    const long long at = (b * n_steps + p) * width + (long long)u * UNIT;
    if (UNIT == 2) {
        const longlong2 v = *reinterpret_cast<const longlong2*>(src + at);
        *reinterpret_cast<longlong2*>(dst + at) = make_longlong2(clamp_idx(v.x, V), clamp_idx(v.y, V));
    } else {
        dst[at] = clamp_idx(src[at], V);
    }
}
hipError_t launch_copy_kept_rows(const int64_t* src, int64_t* dst, const unsigned char* keep, const int* pos, int B, int n_steps, int width, int k, int k0, int V,
                                 hipStream_t st) {
    if (B < 1 || n_steps < 1 || width < 1 || k < 1 || k0 < k || !src || !dst || !keep || !pos) return hipErrorInvalidValue;
    const bool vec = width % 2 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    const long long n = (long long)B * k0 * (width / (vec ? 2 : 1));
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (vec) copy_kept_rows_kernel<2><<<grid, 256, 0, st>>>(src, dst, keep, pos, n, k, k0, width, n_steps, V);
    else copy_kept_rows_kernel<1><<<grid, 256, 0, st>>>(src, dst, keep, pos, n, k, k0, width, n_steps, V);
    return hipGetLastError();
}

// The T prompt rows of every sample, x[b * rows_per_sample + t] (rows_per_sample > T: a code prefix's rows follow, embed_prefix_kernel)
__global__ __launch_bounds__(256) void embed_text_kernel(const int64_t* cond, const float* tok, const float* pos,
                                                         float* x, int T, int D, int vocab, int rows_per_sample) {
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    const long long id = clamp_idx(cond[blockIdx.x], vocab), row = (long long)b * rows_per_sample + t;
    for (int d = threadIdx.x; d < D; d += blockDim.x) x[row * D + d] = tok[id * D + d] + pos[(long long)t * D + d];
}
hipError_t launch_embed_text(const int64_t* cond, const float* tok, const float* pos, float* x, int B, int T, int D,
                             hipStream_t st, int vocab, int rows_per_sample) {
    if (rows_per_sample == 0) rows_per_sample = T;
    if (rows_per_sample < T) return hipErrorInvalidValue;
    embed_text_kernel<<<B * T, 256, 0, st>>>(cond, tok, pos, x, T, D, vocab, rows_per_sample);
    return hipGetLastError();
}

// The sibling for the rows that join a rolling pass (hqt_set_max_joins): their prompts are not contiguous in cond [B, T].  `group_of_row` (device, [B]) is the
// row list: row b with group g in [0, G) writes its T prompt rows to x[g * rows_per_sample + t] (rows_per_sample > T: the rows of a kept run follow,
// embed_prefix_rows_kernel); every other row (group -1: mid-image, or an empty slot) reads and writes nothing.
__global__ __launch_bounds__(256) void embed_text_rows_kernel(const int64_t* cond, const int* group_of_row, const float* tok, const float* pos,
                                                              float* x, int G, int T, int D, int vocab, int rows_per_sample) {
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    const int g = group_of_row[b];
    if (g < 0 || g >= G) return;
    const long long id = clamp_idx(cond[blockIdx.x], vocab), row = (long long)g * rows_per_sample + t;
    for (int d = threadIdx.x; d < D; d += blockDim.x) x[row * D + d] = tok[id * D + d] + pos[(long long)t * D + d];
}
hipError_t launch_embed_text_rows(const int64_t* cond, const int* group_of_row, const float* tok, const float* pos, float* x, int B, int G, int T, int D,
                                  hipStream_t st, int vocab, int rows_per_sample) {
    if (rows_per_sample == 0) rows_per_sample = T;
    if (B < 1 || G < 1 || G > B || T < 1 || D < 1 || rows_per_sample < T || !cond || !group_of_row || !x) return hipErrorInvalidValue;
    embed_text_rows_kernel<<<B * T, 256, 0, st>>>(cond, group_of_row, tok, pos, x, G, T, D, vocab, rows_per_sample);
    return hipGetLastError();
}

// Shared prompts: the hand-out of a prefill that ran over the G distinct prompts of a pass (FanoutArgs, kernels.h).  The T rows of a (layer, prompt)
// are contiguous in the staging buffer and the T prompt tokens of a (layer, cache slot) are contiguous in the cache, so the work is
// 2 n_layers B "chunks" of T * row_bytes bytes (blockIdx.x = ((layer * B + b) * 2 + (0: K, 1: V))) and B chunks of one fp32 x row behind them;
// blockIdx.y cuts a chunk into pieces of FANOUT_PIECE bytes, eight 16-byte vectors per thread with all loads issued before the stores.  A chunk
// whose pointers or length are not multiples of 16 (D * sizeof(activation) % 16 != 0) goes in 2-byte units instead: every length here is even.
// Nothing is computed and no type is interpreted.  Every index is checked: a group outside [0, G) copies nothing.
constexpr int FANOUT_VECS = 8, FANOUT_PIECE = 256 * FANOUT_VECS * 16;
__global__ __launch_bounds__(256) void prompt_fanout_kernel(FanoutArgs a) {
    const long long kv_chunks = 2LL * a.n_layers * a.B, chunk = blockIdx.x;
    const char* src;
    char* dst;
    long long bytes;
    if (chunk < kv_chunks) {
        const int kv = (int)(chunk & 1);
        const long long lb = chunk >> 1;
        const int b = (int)(lb % a.B), l = (int)(lb / a.B);
        const int g = a.group_of_row[b];
        if (g < 0 || g >= a.G) return;
        bytes = (long long)a.T * a.row_bytes;
        src = reinterpret_cast<const char*>(kv ? a.v_src : a.k_src) + ((long long)l * a.G + g) * bytes;
        dst = reinterpret_cast<char*>(kv ? a.v_dst : a.k_dst) + ((long long)l * a.cache_slots + b) * a.Tcache * a.row_bytes;
    } else {
        const long long b = chunk - kv_chunks;
        if (b >= a.B) return;
        const int g = a.group_of_row[b];
        if (g < 0 || g >= a.G) return;
        bytes = (long long)a.D * 4;
        src = reinterpret_cast<const char*>(a.x_src + ((long long)g * a.T + a.T - 1) * a.D);
        dst = reinterpret_cast<char*>(a.x_out + b * a.D);
    }
    const long long p0 = (long long)blockIdx.y * FANOUT_PIECE, p1 = min(p0 + FANOUT_PIECE, bytes);
    if (p0 >= bytes) return;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)bytes) & 15) == 0) {
        const uint4* s = reinterpret_cast<const uint4*>(src + p0);
        uint4* d = reinterpret_cast<uint4*>(dst + p0);
        const int nvec = (int)((p1 - p0) >> 4);
        uint4 v[FANOUT_VECS];
#pragma unroll
        for (int i = 0; i < FANOUT_VECS; ++i) {
            const int idx = i * 256 + threadIdx.x;
            if (idx < nvec) v[i] = s[idx];
        }
#pragma unroll
        for (int i = 0; i < FANOUT_VECS; ++i) {
            const int idx = i * 256 + threadIdx.x;
            if (idx < nvec) d[idx] = v[i];
        }
    } else {
        const unsigned short* s = reinterpret_cast<const unsigned short*>(src + p0);
        unsigned short* d = reinterpret_cast<unsigned short*>(dst + p0);
        const int n = (int)((p1 - p0) >> 1);
        for (int i = threadIdx.x; i < n; i += 256) d[i] = s[i];
    }
}
hipError_t launch_prompt_fanout(const FanoutArgs& a, hipStream_t st) {
    if (a.n_layers < 1 || a.B < 1 || a.G < 1 || a.G > a.B || a.T < 1 || a.D < 1 || a.B > a.cache_slots || a.T > a.Tcache) return hipErrorInvalidValue;
    if ((a.row_bytes != 2 * a.D && a.row_bytes != 4 * a.D) || !a.group_of_row || !a.k_src || !a.v_src || !a.k_dst || !a.v_dst || !a.x_src || !a.x_out) return hipErrorInvalidValue;
    const long long chunks = 2LL * a.n_layers * a.B + a.B;
    const long long longest = std::max((long long)a.T * a.row_bytes, (long long)a.D * 4);
    const long long pieces = (longest + FANOUT_PIECE - 1) / FANOUT_PIECE;
    if (chunks > 0x7fffffffLL || pieces > 65535) return hipErrorInvalidValue;
    prompt_fanout_kernel<<<dim3((unsigned)chunks, (unsigned)pieces), 256, 0, st>>>(a);
    return hipGetLastError();
}

// hqt_select_rows: the gather of cache rows along the batch axis, in place (KvGatherArgs, kernels.h).  The live tokens of a (K | V, layer, cache slot) are
// one contiguous run of `live_bytes` bytes, and slot j of every run becomes what slot rows_from[j] held: a piece (one byte range of the run, the same in
// every slot) depends on no other piece.  A workgroup owns one piece of one (K | V, layer) (blockIdx.y = layer * 2 + (0: K, 1: V), blockIdx.x = piece):
// it reads the B_new source pieces into LDS, passes the barrier, then writes slots 0 .. B_new - 1.  Workgroups touch disjoint pieces, so duplicates, cycles
// and sources at or above B_new need no ordering between them.  Unit = uint4 (16 bytes per lane) where run length and pointers allow, else 2 bytes: every
// length here is even.  Nothing is computed and no type is interpreted.  Every index is checked: an entry outside [0, cache_slots) moves nothing.
template <class Unit>
__global__ __launch_bounds__(256) void kv_gather_rows_kernel(KvGatherArgs a, int piece_units) {
    extern __shared__ uint4 gather_lds[];
    Unit* lds = reinterpret_cast<Unit*>(gather_lds);
    const int kv = (int)(blockIdx.y & 1), l = (int)(blockIdx.y >> 1);
    const long long run_units = a.live_bytes / (long long)sizeof(Unit);
    const long long u0 = (long long)blockIdx.x * piece_units;
    if (l >= a.n_layers || u0 >= run_units) return;
    const int nu = (int)min((long long)piece_units, run_units - u0);
    char* const base = reinterpret_cast<char*>(kv ? a.v : a.k) + (long long)l * a.cache_slots * a.slot_bytes;
    const int total = a.B_new * nu;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int j = e / nu, u = e - j * nu;
        const int src = a.rows_from[j];
        if (src < 0 || src >= a.cache_slots) continue;
        lds[e] = reinterpret_cast<const Unit*>(base + (long long)src * a.slot_bytes)[u0 + u];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += 256) {
        const int j = e / nu, u = e - j * nu;
        const int src = a.rows_from[j];
        if (src < 0 || src >= a.cache_slots) continue;
        reinterpret_cast<Unit*>(base + (long long)j * a.slot_bytes)[u0 + u] = lds[e];
    }
}
size_t kv_gather_lds_limit() { return 160u * 1024u; }
hipError_t launch_kv_gather_rows(const KvGatherArgs& a, hipStream_t st) {
    if (a.n_layers < 1 || a.B_new < 1 || a.B_new > a.cache_slots || a.live_bytes < 2 || a.live_bytes > a.slot_bytes || !a.k || !a.v || !a.rows_from) return hipErrorInvalidValue;
    if ((a.live_bytes | a.slot_bytes) & 1) return hipErrorInvalidValue;
    const bool vec = (((uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.live_bytes | (uintptr_t)a.slot_bytes) & 15) == 0;
    const long long unit = vec ? 16 : 2, run_units = a.live_bytes / unit;
    // piece width: as many units as B_new pieces fit into KV_GATHER_LDS (two workgroups per CU); more rows than that: up to the CU's whole LDS
    constexpr long long KV_GATHER_LDS = 64 * 1024;
    long long lds = KV_GATHER_LDS;
    if ((long long)a.B_new * unit > lds) lds = (long long)kv_gather_lds_limit();
    long long piece = lds / ((long long)a.B_new * unit);
    if (piece < 1) return hipErrorInvalidValue;                  // (hqt_select_rows refuses such a B_new by name first)
    piece = std::min(piece, run_units);
    const long long pieces = (run_units + piece - 1) / piece;
    if (pieces > 0x7fffffffLL || 2LL * a.n_layers > 65535 || (long long)a.B_new * piece > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t shmem = (size_t)((long long)a.B_new * piece * unit);
    const dim3 grid((unsigned)pieces, (unsigned)(2 * a.n_layers));
    if (vec) {
        if (shmem > 64 * 1024) { hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kv_gather_rows_kernel<uint4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem); if (e != hipSuccess) return e; }
        kv_gather_rows_kernel<uint4><<<grid, 256, shmem, st>>>(a, (int)piece);
    } else {
        if (shmem > 64 * 1024) { hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kv_gather_rows_kernel<unsigned short>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem); if (e != hipSuccess) return e; }
        kv_gather_rows_kernel<unsigned short><<<grid, 256, shmem, st>>>(a, (int)piece);
    }
    return hipGetLastError();
}

// Positions [p0, p1) of one code level between two [B, n_steps, width] buffers (a segment of a pass: hqt_set_segment); other entries are neither read nor written
__global__ __launch_bounds__(256) void copy_positions_kernel(const int64_t* src, int64_t* dst, long long n, int per_sample, int stride, int off) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per_sample, r = i - b * per_sample;
    dst[b * stride + off + r] = src[b * stride + off + r];
}
hipError_t launch_copy_positions(const int64_t* src, int64_t* dst, int B, int n_steps, int width, int p0, int p1, hipStream_t st) {
    if (B < 1 || width < 1 || p0 < 0 || p1 <= p0 || p1 > n_steps || !src || !dst) return hipErrorInvalidValue;
    const long long n = (long long)B * (p1 - p0) * width;
    copy_positions_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, dst, n, (p1 - p0) * width, n_steps * width, p0 * width);
    return hipGetLastError();
}

// The per-row sibling (a rolling pass: hqt_set_row_positions): row b copies positions [pos[b] + lo, pos[b] + hi) clipped to [0, n_steps); a row with pos[b] < 0
// (an empty slot) copies nothing.  `pos` is the table as the call received it (device, [B]).
__global__ __launch_bounds__(256) void copy_row_positions_kernel(const int64_t* src, int64_t* dst, const int* pos, long long n, int span, int width, int n_steps, int lo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = i / (span * width), r = i - b * (span * width);
    const int p0 = pos[b];
    const int p = p0 + lo + (int)(r / width);
    if (p0 < 0 || p < 0 || p >= n_steps) return;
    const long long at = (b * n_steps + p) * width + r % width;
    dst[at] = src[at];
}
hipError_t launch_copy_row_positions(const int64_t* src, int64_t* dst, const int* pos, int B, int n_steps, int width, int lo, int hi, hipStream_t st) {
    if (B < 1 || width < 1 || hi <= lo || !src || !dst || !pos) return hipErrorInvalidValue;
    const long long n = (long long)B * (hi - lo) * width;
    copy_row_positions_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, dst, pos, n, hi - lo, width, n_steps, lo);
    return hipGetLastError();
}

// `tok_ld` = row length of the table: D, or 4 D for the 'reduce' head, where slot s of a code takes the D-slice s of its row
// (hqtransformer.py:108-116,532-533)
// depth_embed_row: output row `row` (slot row & 3 of its group), from the top code at index `at` of codes_top.  Shared by the decode step's kernel
// (at = b * n_steps + step) and hqt_score's (at = the pair's index)
__device__ __forceinline__ void depth_embed_row(const int64_t* codes_top, long long at, int row, const float* tok, const float* pos, float* x, int D,
                                                bf16_t* xpk, int pk_mb, float* parts, int V, int tok_ld, float* red) {
    const int s = row & 3;
    const long long code = clamp_idx(codes_top[at], V);
    const float* e = tok + code * tok_ld + (tok_ld > D ? s * D : 0);
    for (int d = threadIdx.x; d < D; d += blockDim.x) x[(long long)row * D + d] = e[d] + pos[(long long)s * D + d];
    if (xpk) { __syncthreads(); emit_packed_row(x + (long long)row * D, row, D, xpk, pk_mb, parts, red); }
}
__global__ __launch_bounds__(256) void depth_embed_kernel(const int64_t* codes_top, int n_steps, const StepState* state,
                                                          const float* tok, const float* pos, float* x, int D, bf16_t* xpk,
                                                          int pk_mb, float* parts, int V, int tok_ld, const int* row_pos) {
    __shared__ float red[4];
    const int row = blockIdx.x, b = row >> 2;
    depth_embed_row(codes_top, (long long)b * n_steps + step_of(state, row_pos, b), row, tok, pos, x, D, xpk, pk_mb, parts, V, tok_ld, red);
}
// hqt_score: the rows of a chunk of pairs, pair pair0 + (row >> 2) -- codes_top is [B n] there, indexed by the pair
__global__ __launch_bounds__(256) void score_depth_embed_kernel(const int64_t* codes_top, int pair0, const float* tok, const float* pos, float* x, int D,
                                                                bf16_t* xpk, int pk_mb, float* parts, int V, int tok_ld) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    depth_embed_row(codes_top, (long long)pair0 + (row >> 2), row, tok, pos, x, D, xpk, pk_mb, parts, V, tok_ld, red);
}
hipError_t launch_score_depth_embed(const int64_t* codes_top, int pair0, int pairs, const float* tok, const float* pos, float* x, int D, bf16_t* xpk,
                                    int pk_mb, float* parts, hipStream_t st, int V, int tok_ld) {
    if (pair0 < 0 || pairs < 1) return hipErrorInvalidValue;
    score_depth_embed_kernel<<<pairs * 4, 256, 0, st>>>(codes_top, pair0, tok, pos, x, D, xpk, pk_mb, parts, V, tok_ld > 0 ? tok_ld : D);
    return hipGetLastError();
}
hipError_t launch_depth_embed(const int64_t* codes_top, int n_steps, const StepState* state, const float* tok,
                              const float* pos, float* x, int B, int D, bf16_t* xpk, int pk_mb, float* parts, hipStream_t st, int V, int tok_ld, const int* row_pos) {
    depth_embed_kernel<<<B * 4, 256, 0, st>>>(codes_top, n_steps, state, tok, pos, x, D, xpk, pk_mb, parts, V, tok_ld > 0 ? tok_ld : D, row_pos);
    return hipGetLastError();
}

// Level-2 tokens of the three-level head, (H1 H2 W1 W2) raster: token i carries its parent's level-1 embedding (the D-slice of child
// (H2 W2) when the table is [V, 4 D]: 'reduce'), position i and -- `tok0` non-NULL: 'add' -- the top code's embedding (hqtransformer.py:537-551)
// depth_embed_l2_row: output row `row` (token row & 15 of its group), from the codes at index `at` of codes0 / group `at` of codes1 (see depth_embed_row)
__device__ __forceinline__ void depth_embed_l2_row(const int64_t* codes0, const int64_t* codes1, long long at, int row, const float* tok0, const float* tok1,
                                                   const float* pos, float* x, int D, bf16_t* xpk, int pk_mb, float* parts, int V, int tok1_ld, float* red) {
    const int i = row & 15;
    const int parent = (i >> 3) * 2 + ((i & 3) >> 1);                  // (H1 H2 W1 W2) raster -> (H1 W1)
    const int child = ((i >> 2) & 1) * 2 + (i & 1);                    //                      -> (H2 W2)
    const long long c0 = clamp_idx(codes0[at], V);
    const long long c1 = clamp_idx(codes1[at * 4 + parent], V);
    const float* e1 = tok1 + c1 * tok1_ld + (tok1_ld > D ? child * D : 0);
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float v = e1[d] + pos[(long long)i * D + d];
        if (tok0) v += tok0[c0 * D + d];
        x[(long long)row * D + d] = v;
    }
    if (xpk) { __syncthreads(); emit_packed_row(x + (long long)row * D, row, D, xpk, pk_mb, parts, red); }
}
__global__ __launch_bounds__(256) void depth_embed_l2_kernel(const int64_t* codes0, const int64_t* codes1, int n_steps, const StepState* state,
                                                             const float* tok0, const float* tok1, const float* pos, float* x, int D,
                                                             bf16_t* xpk, int pk_mb, float* parts, int V, int tok1_ld, const int* row_pos) {
    __shared__ float red[4];
    const int row = blockIdx.x, b = row >> 4;
    depth_embed_l2_row(codes0, codes1, (long long)b * n_steps + step_of(state, row_pos, b), row, tok0, tok1, pos, x, D, xpk, pk_mb, parts, V, tok1_ld, red);
}
__global__ __launch_bounds__(256) void score_depth_embed_l2_kernel(const int64_t* codes0, const int64_t* codes1, int pair0, const float* tok0, const float* tok1,
                                                                   const float* pos, float* x, int D, bf16_t* xpk, int pk_mb, float* parts, int V, int tok1_ld) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    depth_embed_l2_row(codes0, codes1, (long long)pair0 + (row >> 4), row, tok0, tok1, pos, x, D, xpk, pk_mb, parts, V, tok1_ld, red);
}
hipError_t launch_score_depth_embed_l2(const int64_t* codes0, const int64_t* codes1, int pair0, int pairs, const float* tok0, const float* tok1, const float* pos,
                                       float* x, int D, bf16_t* xpk, int pk_mb, float* parts, hipStream_t st, int V, int tok1_ld) {
    if (pair0 < 0 || pairs < 1) return hipErrorInvalidValue;
    score_depth_embed_l2_kernel<<<pairs * 16, 256, 0, st>>>(codes0, codes1, pair0, tok0, tok1, pos, x, D, xpk, pk_mb, parts, V, tok1_ld > 0 ? tok1_ld : D);
    return hipGetLastError();
}
hipError_t launch_depth_embed_l2(const int64_t* codes0, const int64_t* codes1, int n_steps, const StepState* state, const float* tok0,
                                 const float* tok1, const float* pos, float* x, int B, int D, bf16_t* xpk, int pk_mb, float* parts,
                                 hipStream_t st, int V, int tok1_ld, const int* row_pos) {
    depth_embed_l2_kernel<<<B * 16, 256, 0, st>>>(codes0, codes1, n_steps, state, tok0, tok1, pos, x, D, xpk, pk_mb, parts, V, tok1_ld > 0 ? tok1_ld : D, row_pos);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void depth_embed_causal_kernel(const int64_t* codes, int stride, int slot, int n_steps, const StepState* state,
                                                                 const float* tok, const float* pos_row, float* x, int D, bf16_t* xpk,
                                                                 int pk_mb, float* parts, int V, const int* row_pos) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const long long code = clamp_idx(codes[((long long)b * n_steps + step_of(state, row_pos, b)) * stride + slot], V);
    for (int d = threadIdx.x; d < D; d += blockDim.x) x[(long long)b * D + d] = tok[code * D + d] + pos_row[d];
    if (xpk) { __syncthreads(); emit_packed_row(x + (long long)b * D, b, D, xpk, pk_mb, parts, red); }
}
hipError_t launch_depth_embed_causal(const int64_t* codes, int stride, int slot, int n_steps, const StepState* state, const float* tok,
                                     const float* pos_row, float* x, int B, int D, bf16_t* xpk, int pk_mb, float* parts, hipStream_t st, int V, const int* row_pos) {
    depth_embed_causal_kernel<<<B, 256, 0, st>>>(codes, stride, slot, n_steps, state, tok, pos_row, x, D, xpk, pk_mb, parts, V, row_pos);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// LayerNorm (eps 1e-5), two-pass, one workgroup per row
// ---------------------------------------------------------------------------------------------
// One wave per row (4 rows per workgroup): the row lives in registers as float4 vectors (coalesced 1-KiB
// wave loads), mean and variance are two shuffle reductions, no LDS and no barrier.
// MODE selects where a row goes (the bidirectional depth head, [B, 5, D] depth rows):
//   LN_PLAIN:       output row m.
//   LN_BIDIR_INPUT: output row 5 m (ln_f + sos_depth of sample m), and rows 5 m + 1 .. 5 m + 4 = a.fill rows 0..3 (pos_emb_depth).
//   LN_BIDIR_HEADS: input row m = 5 b + s; s == 0 -> ln_top (gamma / beta) into row b of y, s > 0 -> ln_bot (gamma2 / beta2) into
//                   row 4 b + s - 1 of y2 (each with its own packed layout).
enum { LN_PLAIN = 0, LN_BIDIR_INPUT = 1, LN_BIDIR_HEADS = 2 };
// ln_row: one row by one wave -- row m of the launch, read from input row in_row.  The ONE place that does this arithmetic: layernorm_kernel and
// score_depth_input_kernel (whose rows come through a row map) both call it, so a row is bit-identical whichever kernel wrote it.
template <typename TO, int MODE>
__device__ __forceinline__ void ln_row(const LNArgs& a, int m, long long in_row, int lane) {
    const int D = a.D;
    int om = m, opk = a.out_packed_mb;
    const float* gamma = a.gamma;
    const float* beta = a.beta;
    void* y = a.y;
    if (MODE == LN_BIDIR_INPUT) om = 5 * m;
    if (MODE == LN_BIDIR_HEADS) {
        const int b = m / 5, s = m - 5 * b;
        om = s ? 4 * b + s - 1 : b;
        if (s) { gamma = a.gamma2; beta = a.beta2; y = a.y2; opk = a.out2_packed_mb; }
    }
    float* x = a.x + in_row * D;
    constexpr int MAXV = 8;                       // D <= 2048 in registers; wider rows fall back to re-reading
    float4 v[MAXV], gmv[MAXV], btv[MAXV];      // affine parameters are fetched with the row, ahead of the reductions
    float s = 0.0f;
    const int nvec = D >> 2;                      // D % 4 == 0
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = lane + i * 64;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        gmv[i] = v[i]; btv[i] = v[i];
        if (vi < nvec) {
            gmv[i] = *reinterpret_cast<const float4*>(gamma + vi * 4);
            btv[i] = *reinterpret_cast<const float4*>(beta + vi * 4);
            if (a.add) { const float4 ad = *reinterpret_cast<const float4*>(a.add + vi * 4); btv[i].x += ad.x; btv[i].y += ad.y; btv[i].z += ad.z; btv[i].w += ad.w; }
            float4 t = *reinterpret_cast<const float4*>(x + vi * 4);
            if (a.n_slabs > 0) {                  // fold in the split-K partial sums (+bias) of the previous GEMM
                if (a.slab_bias) { const float4 bb = *reinterpret_cast<const float4*>(a.slab_bias + vi * 4); t.x += bb.x; t.y += bb.y; t.z += bb.z; t.w += bb.w; }
                for (int sl = 0; sl < a.n_slabs; ++sl) {
                    const float4 p = *reinterpret_cast<const float4*>(a.slabs + ((long long)sl * a.slab_rows + in_row) * D + vi * 4);   // slabs are indexed like x
                    t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w;
                }
                *reinterpret_cast<float4*>(x + vi * 4) = t;
            }
            v[i] = t;
            s += (t.x + t.y) + (t.z + t.w);
        }
    }
    for (int vi = lane + MAXV * 64; vi < nvec; vi += 64) { const float4 t = *reinterpret_cast<const float4*>(x + vi * 4); s += (t.x + t.y) + (t.z + t.w); }
    const float mean = wave_reduce(s, OpAdd()) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        if (lane + i * 64 < nvec) {
            const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
    for (int vi = lane + MAXV * 64; vi < nvec; vi += 64) {
        const float4 t = *reinterpret_cast<const float4*>(x + vi * 4);
        const float dx = t.x - mean, dy = t.y - mean, dz = t.z - mean, dw = t.w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = 1.0f / sqrtf(wave_reduce(q, OpAdd()) / (float)D + a.eps);
    float ys = 0.0f, yq = 0.0f;
    auto emit = [&](int vi, float4 t, float4 gm, float4 bt) {
        const int d = vi * 4;
        float o[4] = {(t.x - mean) * rstd * gm.x + bt.x, (t.y - mean) * rstd * gm.y + bt.y, (t.z - mean) * rstd * gm.z + bt.z,
                      (t.w - mean) * rstd * gm.w + bt.w};
        TO* dst = opk ? reinterpret_cast<TO*>(y) + packed_off(om, d, opk)      // 4 consecutive k stay contiguous
                              : reinterpret_cast<TO*>(y) + (long long)om * D + d;
        if (sizeof(TO) == 2) {
            uint2 pk;
            pk.x = (unsigned)f32_to_bf16(o[0]) | ((unsigned)f32_to_bf16(o[1]) << 16);
            pk.y = (unsigned)f32_to_bf16(o[2]) | ((unsigned)f32_to_bf16(o[3]) << 16);
            *reinterpret_cast<uint2*>(dst) = pk;
        } else {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        }
        if (a.ypk) {                              // deferred-LN consumers read this row as bf16 + its statistics
            uint2 pk;
            pk.x = (unsigned)f32_to_bf16(o[0]) | ((unsigned)f32_to_bf16(o[1]) << 16);
            pk.y = (unsigned)f32_to_bf16(o[2]) | ((unsigned)f32_to_bf16(o[3]) << 16);
            *reinterpret_cast<uint2*>(a.ypk + packed_off(om, d, a.ypk_mb)) = pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float r = bf16_to_f32(f32_to_bf16(o[e])); ys += r; yq += r * r; }
        }
    };
#pragma unroll
    for (int i = 0; i < MAXV; ++i) if (lane + i * 64 < nvec) emit(lane + i * 64, v[i], gmv[i], btv[i]);
    for (int vi = lane + MAXV * 64; vi < nvec; vi += 64) {
        float4 bt = *reinterpret_cast<const float4*>(beta + vi * 4);
        if (a.add) { const float4 ad = *reinterpret_cast<const float4*>(a.add + vi * 4); bt.x += ad.x; bt.y += ad.y; bt.z += ad.z; bt.w += ad.w; }
        emit(vi, *reinterpret_cast<const float4*>(x + vi * 4), *reinterpret_cast<const float4*>(gamma + vi * 4), bt);
    }
    if (a.ypk) {
        ys = wave_reduce(ys, OpAdd());
        yq = wave_reduce(yq, OpAdd());
        if (lane == 0) { a.yparts[2 * om] = ys; a.yparts[2 * om + 1] = yq; }
    }
    if (MODE == LN_BIDIR_INPUT) {                 // the four bottom query rows: pos_emb_depth[0..3], no code embedding (hierarchical_ar.py:815-818)
        for (int j = 1; j <= 4; ++j) {
            const int r = om + j;
            float ps = 0.0f, pq = 0.0f;
            for (int vi = lane; vi < nvec; vi += 64) {
                const float4 t = *reinterpret_cast<const float4*>(a.fill + (long long)(j - 1) * D + vi * 4);
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(y) + (long long)r * D + vi * 4) = t;
                if (a.ypk) {
                    const float o[4] = {t.x, t.y, t.z, t.w};
                    uint2 pk;
                    pk.x = (unsigned)f32_to_bf16(o[0]) | ((unsigned)f32_to_bf16(o[1]) << 16);
                    pk.y = (unsigned)f32_to_bf16(o[2]) | ((unsigned)f32_to_bf16(o[3]) << 16);
                    *reinterpret_cast<uint2*>(a.ypk + packed_off(r, vi * 4, a.ypk_mb)) = pk;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float r4 = bf16_to_f32(f32_to_bf16(o[e])); ps += r4; pq += r4 * r4; }
                }
            }
            if (a.ypk) {
                ps = wave_reduce(ps, OpAdd());
                pq = wave_reduce(pq, OpAdd());
                if (lane == 0) { a.yparts[2 * r] = ps; a.yparts[2 * r + 1] = pq; }
            }
        }
    }
}
template <typename TO, int MODE = LN_PLAIN>
__global__ __launch_bounds__(256) void layernorm_kernel(LNArgs a) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    ln_row<TO, MODE>(a, m, (long long)m * a.in_rows_per_group + a.in_row_offset, threadIdx.x & 63);      // ln_f of the prefill reads the last token of each sample
}
// hqt_score: depth input of level 0 for a chunk of (sample, position) pairs -- ln_f + sos_depth of body row b * stride + off + t of pair
// p = pair0 + m = b n + t (stride = n, off = 0; text: stride = T + n - 1, off = T - 1), into row m of xd (BIDIR: row 5 m, then the four pos_emb_depth rows)
template <int MODE>
__global__ __launch_bounds__(256) void score_depth_input_kernel(LNArgs a, int pair0, int n, int stride, int off) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    const int p = pair0 + m, b = p / n, t = p - b * n;
    ln_row<float, MODE>(a, m, (long long)b * stride + off + t, threadIdx.x & 63);
}
hipError_t launch_score_depth_input(const LNArgs& a, int pair0, int n, int stride, int off, hipStream_t st) {
    if (a.D % 4 != 0 || a.out_dtype != DT_F32 || a.out_packed_mb || a.n_slabs || pair0 < 0 || n < 1 || off < 0 || off + n > stride) return hipErrorInvalidValue;
    if (a.fill) score_depth_input_kernel<LN_BIDIR_INPUT><<<(a.M + 3) / 4, 256, 0, st>>>(a, pair0, n, stride, off);
    else score_depth_input_kernel<LN_PLAIN><<<(a.M + 3) / 4, 256, 0, st>>>(a, pair0, n, stride, off);
    return hipGetLastError();
}
hipError_t launch_layernorm(const LNArgs& a, hipStream_t st) {
    if (a.D % 4 != 0) return hipErrorInvalidValue;
    if (a.out_dtype == DT_BF16) layernorm_kernel<bf16_t><<<(a.M + 3) / 4, 256, 0, st>>>(a);
    else layernorm_kernel<float><<<(a.M + 3) / 4, 256, 0, st>>>(a);
    return hipGetLastError();
}
hipError_t launch_bidir_depth_input(const LNArgs& a, hipStream_t st) {
    if (a.D % 4 != 0 || a.out_dtype != DT_F32 || a.out_packed_mb || !a.fill) return hipErrorInvalidValue;
    layernorm_kernel<float, LN_BIDIR_INPUT><<<(a.M + 3) / 4, 256, 0, st>>>(a);
    return hipGetLastError();
}
hipError_t launch_bidir_head_ln(const LNArgs& a, hipStream_t st) {
    if (a.D % 4 != 0 || a.M % 5 != 0 || a.add || a.ypk || !a.y2 || !a.gamma2 || !a.beta2) return hipErrorInvalidValue;
    if (a.out_dtype == DT_BF16) layernorm_kernel<bf16_t, LN_BIDIR_HEADS><<<(a.M + 3) / 4, 256, 0, st>>>(a);
    else layernorm_kernel<float, LN_BIDIR_HEADS><<<(a.M + 3) / 4, 256, 0, st>>>(a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// A7/K6: fused sampler -- temperature, top-k, softmax, top-p, argmax(p / q), code write-back.
// One 256-thread workgroup per logits row.  Restates hqvae/utils/sampling.py:12-37 and
// hierarchical_ar.py:762-785; torch.multinomial(p, 1) == argmax(p / q), q ~ Exp(1).
// ---------------------------------------------------------------------------------------------
// The radix key of the top-k select: unsigned order == float order.  Both zeros get the key of +0.0: the reference masks `logits < kth`
// (sampling.py:18), where -0.0 is not below +0.0, and a tiny negative logit divided by the temperature underflows to -0.0 -- with the sign
// bit in the key such a token was masked whenever the k-th largest value was +0.0 (tests/test_gpu_sampler_rows.py).
__device__ __forceinline__ uint32_t f2ord(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return __umulhi(a, b); }
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Which kernel draws a row of a FAST pass whose vocabulary sampler_plain_fast_kernel takes: the rows without a cut-off go there, the others to sampler_kernel --
// the choice launch_sampler makes for a uniform call, made per row when the settings come from a row table (the two kernels differ in the last bit of a ratio,
// so a row must stay with the kernel it would get alone)
__host__ __device__ __forceinline__ bool sampler_row_plain(int top_k, float top_p, int V) { return !(top_k > 0 && top_k < V) && !(top_p > 0.0f); }

// NT threads per logits row: 1024 (16 waves, 4 per SIMD) hides the latency of the exp / log / divide / Philox chains that a
// lone 4-wave workgroup per CU exposes (25 -> ~10 us per launch at V = 8192); 256 for small vocabularies.
// FM: fast-math forms for FAST-precision calls.  The plain path (no top-k / top-p) is bound by the IEEE expf / logf / divisions of its
// 8192 entries per row, not by memory (21.5 us per 512 rows); EXACT calls keep them: their draws are the parity gate, compared bit for bit with the CPU restatement of the reference.
template <int NT, bool FM>
__global__ __launch_bounds__(NT, 8) void sampler_kernel(SamplerArgs a, int n2) {   // 8 waves per SIMD = two 1024-thread rows per CU: the plain path is 30 % slower at 7 (tools/micro/bench_sampler)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    // layout: double dsum[NT]; float redf[16]; int redi[16]; unsigned hist[256]; int sel[4]; float lp[V];
    //         (top-p only) float skey[n2]; unsigned short sidx[n2]; unsigned char keep[V]
    double* dsum = reinterpret_cast<double*>(smem_raw);
    float* redf = reinterpret_cast<float*>(dsum + NT);
    int* redi = reinterpret_cast<int*>(redf + 16);
    unsigned* hist = reinterpret_cast<unsigned*>(redi + 16);
    int* sel = reinterpret_cast<int*>(hist + 256);
    float* lp = reinterpret_cast<float*>(sel + 4);
    const int V = a.V, tid = threadIdx.x;
    float* skey = lp + V;
    unsigned short* sidx = reinterpret_cast<unsigned short*>(skey + n2);
    unsigned char* keep = reinterpret_cast<unsigned char*>(sidx + n2);

    const int r = blockIdx.x, b = r / a.slots, slot = r % a.slots;
    // the row's own settings when the call carries a row table (workgroup-uniform: scalar loads); under dispatch a row without a cut-off belongs to
    // sampler_plain_fast_kernel, and this workgroup leaves before it touches anything
    float temperature = a.temperature, top_p = a.top_p;
    int top_k = a.top_k;
    if (a.row_set) {
        const RowSampler& rs = a.row_set[b];
        temperature = rs.temperature[a.row_lv_t]; top_k = rs.top_k[a.row_lv_k]; top_p = rs.top_p[a.row_lv_k];
        if (a.row_dispatch && sampler_row_plain(top_k, top_p, V)) return;
    }
    const int step = step_of(a.state, a.row_pos, b);
    const bool idle = row_idle(a.row_pos, b);        // rolling pass: the row computes (as at position 0) and writes nothing the caller can see
    const int draw = a.draw0 + slot;
    const float* lg = a.logits + (long long)r * V;
    const int draws = a.draws > 0 ? a.draws : 5;
    const long long nidx = (((long long)step * draws + draw) * a.B + b) * V;

    // ---- temperature (logits /= T, hierarchical_ar.py:763,779) and raw-logit dump
    const float inv_t = FM ? __builtin_amdgcn_rcpf(temperature) : 0.0f;
    for (int i = tid; i < V; i += NT) {
        const float v = lg[i];
        if (a.logits_out && !idle) a.logits_out[nidx + i] = v;
        lp[i] = FM ? v * inv_t : v / temperature;
    }
    __syncthreads();

    // ---- top-k: exact k-th largest by 4-pass radix select, keep >= threshold (sampling.py:12-19)
    if (top_k > 0 && top_k < V) {
        uint32_t prefix = 0;
        int remaining = top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const uint32_t himask = shift == 24 ? 0u : ~((1u << (shift + 8)) - 1u);
            for (int i = tid; i < V; i += NT) {
                const uint32_t o = f2ord(lp[i]);
                if ((o & himask) == prefix) atomicAdd(&hist[(o >> shift) & 255u], 1u);
            }
            __syncthreads();
            // the bin that holds the k-th largest = the highest bin b >= 1 with (elements in bins above b) + hist[b] >= remaining, else
            // bin 0 (what a scan from bin 255 downwards finds): suffix sums over the 256 bins by 4 waves instead of 256 dependent LDS
            // reads on one thread
            if (tid == 0) sel[0] = 0;
            unsigned h = 0, incl = 0, above = 0;
            const int lane_k = tid & 63, wave_k = tid >> 6;
            if (tid < 256) {
                h = hist[tid];
                incl = h;
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned v = (unsigned)__shfl_down((int)incl, off, 64);
                    if (lane_k + off < 64) incl += v;
                }
                if (lane_k == 0) redi[wave_k] = (int)incl;
            }
            __syncthreads();
            if (tid < 256) {
                above = incl - h;
                for (int w = wave_k + 1; w < 4; ++w) above += (unsigned)redi[w];
                if (tid >= 1 && above + h >= (unsigned)remaining) atomicMax(&sel[0], tid);
            }
            __syncthreads();
            const int bin_sel = sel[0];
            if (tid == bin_sel) sel[1] = remaining - (int)above;
            __syncthreads();
            prefix |= ((uint32_t)bin_sel) << shift;
            remaining = sel[1];
            __syncthreads();
        }
        for (int i = tid; i < V; i += NT)
            if (f2ord(lp[i]) < prefix) lp[i] = -INFINITY;
        __syncthreads();
    }

    // ---- softmax (fp32): p = exp(l - max) / sum
    float m = -INFINITY;
    for (int i = tid; i < V; i += NT) m = fmaxf(m, lp[i]);
    m = block_reduce(m, OpMax(), redf);
    float s = 0.0f;
    for (int i = tid; i < V; i += NT) { const float e = FM ? __expf(lp[i] - m) : expf(lp[i] - m); lp[i] = e; s += e; }
    s = block_reduce(s, OpAdd(), redf);
    const float inv_s = FM ? __builtin_amdgcn_rcpf(s) : 0.0f;
    for (int i = tid; i < V; i += NT) lp[i] = FM ? lp[i] * inv_s : lp[i] / s;
    __syncthreads();

    // ---- top-p (sampling.py:22-37): descending sort, prefix sums accumulated in double and rounded
    //      to fp32 per element (what torch.cumsum does on the CPU), cut after the first prefix >= p
    float renorm = 1.0f;
    const bool use_p = top_p > 0.0f;
    if (use_p) {
        // Only entries with p > 0 can matter (zeros -- everything top-k masked -- sort last, add nothing to the prefix sums and stay zero
        // whether kept or not), so they alone are compacted, sorted and scanned: with top_k = 2048 of V = 8192 the bitonic network
        // shrinks from 91 passes x 8 elements per thread to 66 x 2 (1.1 ms -> see profiles/ per launch at 2048 rows).  Same results bit
        // for bit: the network orders (probability desc, index asc) pairs, a total order that does not depend on where they start.
        const int per = (V + NT - 1) / NT, lane_ = tid & 63, wave_ = tid >> 6;
        int c_local = 0;
        for (int c = 0; c < per; ++c) { const int j = tid * per + c; if (j < V && lp[j] > 0.0f) ++c_local; }
        int incl = c_local;
        for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (lane_ >= off) incl += v; }
        if (lane_ == 63) redi[wave_] = incl;
        __syncthreads();
        int pos = incl - c_local, cnt = 0;
        for (int w = 0; w < NT / 64; ++w) { const int t = redi[w]; if (w < wave_) pos += t; cnt += t; }
        for (int c = 0; c < per; ++c) {
            const int j = tid * per + c;
            if (j < V && lp[j] > 0.0f) { skey[pos] = lp[j]; sidx[pos] = (unsigned short)j; ++pos; }
        }
        int n2e = 256;
        while (n2e < cnt) n2e <<= 1;                                 // <= n2 (cnt <= V)
        for (int i = cnt + tid; i < n2e; i += NT) { skey[i] = -1.0f; sidx[i] = (unsigned short)i; }
        __syncthreads();
        // The bitonic network with the elements in registers: element e of thread t is position e NT + t, so a partner at distance
        // j >= NT is another register of the same thread, at j < 64 a lane of the same wave (one shuffle each for key and index), and
        // only 64 <= j < NT goes through LDS with barriers: 14 of the 66 steps at 2048 entries on 1024 threads.
        constexpr int EMAX = 2;
        const int E = n2e > NT ? n2e / NT : 1;
        const bool in_regs = E <= EMAX;
        if (in_regs) {
            float kv[EMAX];
            int iv[EMAX];
#pragma unroll
            for (int e = 0; e < EMAX; ++e) {
                const int i = e * NT + tid;
                kv[e] = (e < E && i < n2e) ? skey[i] : -2.0f;
                iv[e] = (e < E && i < n2e) ? (int)sidx[i] : 0xFFFF;
            }
            auto first = [](float ka, int ia, float kb, int ib) { return ka > kb || (ka == kb && ia < ib); };      // a before b: prob desc, index asc
            for (int k2 = 2; k2 <= n2e; k2 <<= 1) {
                for (int j = k2 >> 1; j > 0; j >>= 1) {
                    if (j >= NT) {                                    // (E == 2, j == NT) partner = the thread's other register
                        const bool up = (tid & k2) == 0;              // position of register 0; bit j is clear in it
                        const bool a_first = first(kv[0], iv[0], kv[1], iv[1]);
                        if (up ? !a_first : a_first) { const float tk = kv[0]; kv[0] = kv[1]; kv[1] = tk; const int ti = iv[0]; iv[0] = iv[1]; iv[1] = ti; }
                    } else if (j >= 64) {                             // partner in another wave: through LDS
                        __syncthreads();
#pragma unroll
                        for (int e = 0; e < EMAX; ++e) { const int i = e * NT + tid; if (e < E && i < n2e) { skey[i] = kv[e]; sidx[i] = (unsigned short)iv[e]; } }
                        __syncthreads();
#pragma unroll
                        for (int e = 0; e < EMAX; ++e) {
                            const int i = e * NT + tid;
                            if (e < E && i < n2e) {
                                const float kb = skey[i ^ j]; const int ib = sidx[i ^ j];
                                const bool lower = (i & j) == 0, up = (i & k2) == 0;
                                const bool me_first = first(kv[e], iv[e], kb, ib);
                                if ((lower == up) ? !me_first : me_first) { kv[e] = kb; iv[e] = ib; }      // lower & up (or upper & down) keeps the first
                            }
                        }
                    } else {                                          // partner = lane ^ j of this wave
#pragma unroll
                        for (int e = 0; e < EMAX; ++e) {
                            const int i = e * NT + tid;
                            const float kb = __shfl_xor(kv[e], j, 64); const int ib = __shfl_xor(iv[e], j, 64);
                            const bool lower = (i & j) == 0, up = (i & k2) == 0;
                            const bool me_first = first(kv[e], iv[e], kb, ib);
                            if ((lower == up) ? !me_first : me_first) { kv[e] = kb; iv[e] = ib; }
                        }
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < EMAX; ++e) { const int i = e * NT + tid; if (e < E && i < n2e) { skey[i] = kv[e]; sidx[i] = (unsigned short)iv[e]; } }
            __syncthreads();
        }
        for (int k2 = 2; !in_regs && k2 <= n2e; k2 <<= 1) {
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n2e; i += NT) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const float ka = skey[i], kb = skey[ixj];
                        const unsigned short ia = sidx[i], ib = sidx[ixj];
                        const bool a_first = ka > kb || (ka == kb && ia < ib);   // order: prob desc, index asc
                        const bool up = (i & k2) == 0;
                        if (up ? !a_first : a_first) { skey[i] = kb; skey[ixj] = ka; sidx[i] = ib; sidx[ixj] = ia; }
                    }
                }
                __syncthreads();
            }
        }
        const int chunk = (n2e + NT - 1) / NT;
        double local = 0.0;
        for (int c = 0; c < chunk; ++c) { const int j = tid * chunk + c; if (j < cnt) local += (double)skey[j]; }
        // exclusive prefix of the per-thread sums: shuffle scan inside each wave, then the totals of the waves in front (a 1024-step
        // serial loop on one thread before: ~9 us per row).  Everything is accumulated in double, as torch.cumsum does for an fp32 row;
        // the association differs from a strictly sequential sum only below 2^-53 relative.
        double scan = local;
        for (int off = 1; off < 64; off <<= 1) { const double v = __shfl_up(scan, off, 64); if (lane_ >= off) scan += v; }
        if (lane_ == 63) dsum[wave_] = scan;
        __syncthreads();
        double run = scan - local;
        for (int w = 0; w < wave_; ++w) run += dsum[w];
        int first = V;                                   // first sorted position whose prefix >= p
        for (int c = 0; c < chunk; ++c) {
            const int j = tid * chunk + c;
            if (j < cnt) {
                run += (double)skey[j];
                if ((float)run >= top_p && j < first) first = j;
            }
        }
        first = block_reduce(first, OpMin(), redi);
        for (int i = tid; i < V; i += NT) keep[i] = 0;
        __syncthreads();
        for (int j = tid; j < cnt; j += NT)
            if (j <= first) keep[sidx[j]] = 1;           // position `first` itself is kept (shifted mask)
        __syncthreads();
        float ks = 0.0f;
        for (int i = tid; i < V; i += NT) { if (!keep[i]) lp[i] = 0.0f; ks += lp[i]; }
        renorm = block_reduce(ks, OpAdd(), redf);
        __syncthreads();
    }

    // ---- draw: argmax_i p_i / q_i, lowest index on ties
    float best = -1.0f;
    int besti = 0;
    const uint64_t seed = a.rows[b].seed;                // per-call / per-row values live in device memory: the captured graph is call-independent
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint64_t grow = (uint64_t)a.rows[b].global_row;
    for (int i4 = tid; i4 * 4 < V; i4 += NT) {
        float q[4];
        if (a.noise) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = (i4 * 4 + e < V) ? a.noise[nidx + i4 * 4 + e] : 1.0f;
        } else {
            uint32_t rnd[4];
            philox4x32_10((uint32_t)i4, (uint32_t)(step * draws + draw), (uint32_t)grow, (uint32_t)(grow >> 32), k0, k1, rnd);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float u = ((float)(rnd[e] >> 9) + 0.5f) * (1.0f / 8388608.0f);     // 23 bits + 0.5: exact in fp32, u in [2^-24, 1 - 2^-24] -- never 1.0 (q = 0)
                q[e] = FM ? -__logf(u) : -logf(u);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i4 * 4 + e;
            if (i < V) {
                float p = lp[i];
                if (use_p) p = p / renorm;
                const float ratio = FM ? p * __builtin_amdgcn_rcpf(q[e]) : p / q[e];
                if (ratio > best) { best = ratio; besti = i; }      // ascending i per lane: first max wins
            }
        }
    }
    // reduce (value desc, index asc)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(besti, off, 64);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { redf[tid >> 6] = best; redi[tid >> 6] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NT / 64; ++w)
            if (redf[w] > best || (redf[w] == best && redi[w] < besti)) { best = redf[w]; besti = redi[w]; }
        int64_t* const dst = a.out + (a.out_stride > 0 ? ((long long)b * a.n_steps + step) * a.out_stride + a.out_slot : ((long long)b * a.n_steps + step) * a.slots + slot);
        if (idle) {}                                     // an idle row: the draw is discarded and `out` is left alone (the fused embedding below takes the discarded code: any code in range)
        else if (a.keep && a.keep[(long long)b * a.n_steps + step]) besti = (int)*dst;      // a kept position: the draw is discarded, the code (clamped when it was stored) stays
        else *dst = (int64_t)besti;
        if (a.emb_tok) sel[0] = a.emb_feed ? (int)clamp_idx(a.emb_feed[((long long)b * a.n_steps + step) * a.slots + slot], a.V) : besti;
    }
    if (!a.emb_tok) return;                              // workgroup-uniform
    // ---- fused embedding lookup: this workgroup drew the top code of sample b, so it also writes the four depth-token rows
    __syncthreads();
    const long long code = sel[0];
    const int D = a.emb_D;
#pragma unroll 1
    for (int s4 = 0; s4 < 4; ++s4) {
        const int row = b * 4 + s4;
        float rs = 0.0f, rq = 0.0f;
        for (int d = tid; d < D; d += NT) {
            const float v = a.emb_tok[code * D + d] + a.emb_pos[(long long)s4 * D + d];
            a.emb_x[(long long)row * D + d] = v;
            if (a.emb_xpk) {
                const bf16_t hb = f32_to_bf16(v);
                a.emb_xpk[packed_off(row, d, a.emb_pk_mb)] = hb;
                const float r = bf16_to_f32(hb);
                rs += r; rq += r * r;
            }
        }
        if (a.emb_xpk) {                                 // fixed-order reduction: waves, then wave 0 .. NT/64-1
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { rs += __shfl_xor(rs, off, 64); rq += __shfl_xor(rq, off, 64); }
            __syncthreads();
            if ((tid & 63) == 0) { redf[tid >> 6] = rs; dsum[tid >> 6] = (double)rq; }
            __syncthreads();
            if (tid == 0) {
                float ts = 0.0f, tq = 0.0f;
                for (int w = 0; w < NT / 64; ++w) { ts += redf[w]; tq += (float)dsum[w]; }
                a.emb_parts[2 * row] = ts; a.emb_parts[2 * row + 1] = tq;
            }
        }
    }
}

// FAST draws without a cut-off (top_k = top_p = None: the H1 harness settings): at 2048 samples per pass the bottom codes are 8192 rows
// x 8192 logits per position.  argmax_i p_i / q_i does not need p normalised, so the row never
// leaves the registers: 4 waves per row, thread t owns the float4 groups t, t + 256, ... (the Philox counter of a group is its index,
// as in sampler_kernel), one pass for the maximum, one for exp(l - max) / q and the running best, two 4-wave barriers in all -- against
// five block-wide reductions over 16 waves and four trips through a 32-KB LDS row in the general kernel (8192 rows: 239 -> 93 us, 2048
// rows: 65 -> 31 us, tools/micro/bench_sampler).  Same v_exp / v_log / v_rcp forms as sampler_kernel<.., true>; the ratio lacks the factor 1 / sum, which cannot
// change the winner except between ratios that differ in the last bit.
template <int G4>
__global__ __launch_bounds__(256) void sampler_plain_fast_kernel(SamplerArgs a) {
    __shared__ float redf[4];
    __shared__ int redi[4];
    const int V = a.V, tid = threadIdx.x;
    const int r = blockIdx.x, b = r / a.slots, slot = r % a.slots;
    float temperature = a.temperature;
    if (a.row_set) {             // row table: this kernel takes the rows without a cut-off, sampler_kernel (launched over the same rows) the others
        const RowSampler& rs = a.row_set[b];
        temperature = rs.temperature[a.row_lv_t];
        if (!sampler_row_plain(rs.top_k[a.row_lv_k], rs.top_p[a.row_lv_k], V)) return;      // workgroup-uniform
    }
    const int step = step_of(a.state, a.row_pos, b);
    const bool idle = row_idle(a.row_pos, b);        // rolling pass: the row computes (as at position 0) and writes nothing the caller can see
    const int draw = a.draw0 + slot;
    const float* lg = a.logits + (long long)r * V;
    const int draws = a.draws > 0 ? a.draws : 5;
    const long long nidx = (((long long)step * draws + draw) * a.B + b) * V;
    const float inv_t = __builtin_amdgcn_rcpf(temperature);
    float4 v[G4];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < G4; ++k) {
        const int i4 = tid + 256 * k;
        if (i4 * 4 < V) {                                 // V % 4 == 0
            v[k] = *reinterpret_cast<const float4*>(lg + i4 * 4);
            if (a.logits_out && !idle) *reinterpret_cast<float4*>(a.logits_out + nidx + i4 * 4) = v[k];
            v[k].x *= inv_t; v[k].y *= inv_t; v[k].z *= inv_t; v[k].w *= inv_t;
            m = fmaxf(fmaxf(m, fmaxf(v[k].x, v[k].y)), fmaxf(v[k].z, v[k].w));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) redf[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    float best = -1.0f;
    int besti = 0;
    const uint64_t seed = a.rows[b].seed;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint64_t grow = (uint64_t)a.rows[b].global_row;
#pragma unroll
    for (int k = 0; k < G4; ++k) {
        const int i4 = tid + 256 * k;
        if (i4 * 4 < V) {
            float q[4];
            if (a.noise) {
                const float4 n4 = *reinterpret_cast<const float4*>(a.noise + nidx + i4 * 4);
                q[0] = n4.x; q[1] = n4.y; q[2] = n4.z; q[3] = n4.w;
            } else {
                uint32_t rnd[4];
                philox4x32_10((uint32_t)i4, (uint32_t)(step * draws + draw), (uint32_t)grow, (uint32_t)(grow >> 32), k0, k1, rnd);
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] = -__logf(((float)(rnd[e] >> 9) + 0.5f) * (1.0f / 8388608.0f));
            }
            const float l[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ratio = __expf(l[e] - m) * __builtin_amdgcn_rcpf(q[e]);
                if (ratio > best) { best = ratio; besti = i4 * 4 + e; }         // ascending index per thread: the first maximum wins
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(besti, off, 64);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    __syncthreads();                                      // redf has been read by everyone
    if ((tid & 63) == 0) { redf[tid >> 6] = best; redi[tid >> 6] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (redf[w] > best || (redf[w] == best && redi[w] < besti)) { best = redf[w]; besti = redi[w]; }
        int64_t* const dst = a.out + (a.out_stride > 0 ? ((long long)b * a.n_steps + step) * a.out_stride + a.out_slot : ((long long)b * a.n_steps + step) * a.slots + slot);
        if (idle) {}                                     // an idle row: the draw is discarded and `out` is left alone (the fused embedding below takes the discarded code: any code in range)
        else if (a.keep && a.keep[(long long)b * a.n_steps + step]) besti = (int)*dst;      // a kept position: the draw is discarded, the code (clamped when it was stored) stays
        else *dst = (int64_t)besti;
        if (a.emb_tok) redi[0] = a.emb_feed ? (int)clamp_idx(a.emb_feed[((long long)b * a.n_steps + step) * a.slots + slot], a.V) : besti;
    }
    if (!a.emb_tok) return;                              // workgroup-uniform
    // ---- fused embedding lookup, as in sampler_kernel: the four input rows of depth sub-step 1 for the top code just drawn.  The four rows share the token
    // embedding: one pass with every load in flight and ONE reduction for the eight row statistics (row after row -- four dependent round trips and eight
    // barriers -- this tail was ~7 of the kernel's 17 us at 64 rows); per row the same sums in the same order as before.
    __shared__ float reds[4][4], redq[4][4];
    __syncthreads();
    const long long code = redi[0];
    const int D = a.emb_D;
    float rs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int d = tid; d < D; d += 256) {
        const float t = a.emb_tok[code * D + d];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int row = b * 4 + s4;
            const float x = t + a.emb_pos[(long long)s4 * D + d];
            a.emb_x[(long long)row * D + d] = x;
            if (a.emb_xpk) {
                const bf16_t hb = f32_to_bf16(x);
                a.emb_xpk[packed_off(row, d, a.emb_pk_mb)] = hb;
                const float rr = bf16_to_f32(hb);
                rs[s4] += rr; rq[s4] += rr * rr;
            }
        }
    }
    if (a.emb_xpk) {                                     // fixed-order reduction: lanes, then waves 0 .. 3
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { rs[s4] += __shfl_xor(rs[s4], off, 64); rq[s4] += __shfl_xor(rq[s4], off, 64); }
            if ((tid & 63) == 0) { reds[s4][tid >> 6] = rs[s4]; redq[s4][tid >> 6] = rq[s4]; }
        }
        __syncthreads();
        if (tid < 4) {
            const int row = b * 4 + tid;
            a.emb_parts[2 * row] = ((reds[tid][0] + reds[tid][1]) + reds[tid][2]) + reds[tid][3];
            a.emb_parts[2 * row + 1] = ((redq[tid][0] + redq[tid][1]) + redq[tid][2]) + redq[tid][3];
        }
    }
}

static size_t sampler_smem(int V, bool use_p, int& n2) {
    n2 = 256;
    while (n2 < V) n2 <<= 1;
    size_t sz = 1024 * sizeof(double) + 16 * sizeof(float) + 16 * sizeof(int) + 256 * sizeof(unsigned) + 4 * sizeof(int) +
                (size_t)V * sizeof(float);
    if (use_p) sz += (size_t)n2 * sizeof(float) + (size_t)n2 * sizeof(unsigned short) + (size_t)V;
    return (sz + 15) & ~(size_t)15;
}
// hipFuncSetAttribute applies to the CURRENT device and is only ever RAISED here: the limit is a per-device maximum over every
// (V, top_p) any handle of this process has asked for, so a handle that needs 42 KB can never lower the limit under another
// handle's (or another thread's) 99 KB launch or captured graph.
hipError_t sampler_configure(int V, bool use_top_p) {
    int n2;
    const size_t smem = sampler_smem(V, use_top_p, n2);
    if (smem > 160 * 1024 || (use_top_p && V > 65536)) return hipErrorInvalidValue;
    static std::mutex mu;
    static size_t limit[64] = {};                                   // per device ordinal
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 0 && dev < 64 && smem <= limit[dev]) return hipSuccess;
    for (const void* k : {reinterpret_cast<const void*>(sampler_kernel<256, false>), reinterpret_cast<const void*>(sampler_kernel<256, true>),
                          reinterpret_cast<const void*>(sampler_kernel<1024, false>), reinterpret_cast<const void*>(sampler_kernel<1024, true>)}) {
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    if (e == hipSuccess && dev >= 0 && dev < 64) limit[dev] = smem;
    return e;
}
hipError_t launch_sampler(const SamplerArgs& args, hipStream_t st) {
    SamplerArgs a = args;
    const bool table = a.row_set != nullptr;
    int n2;
    const size_t smem = sampler_smem(a.V, table ? a.row_top_p != 0 : a.top_p > 0.0f, n2);
    if (smem > 160 * 1024) return hipErrorInvalidValue;               // sampler_configure(V, top_p) ran in sample_run for this call's options
    // FAST, no cut-offs, V <= 8192: the register-resident kernel (HQT_NO_PLAIN_SAMPLER=1: A/B switch).  With a row table it runs over every row in front of the
    // general kernel and each of the two leaves the other one's rows alone (row_dispatch): two launches whatever the table holds.
    const bool no_plain = switch_value(SW_NO_PLAIN_SAMPLER);
    const bool plain_v = !no_plain && a.fast_math && a.V % 4 == 0 && a.V <= 8192 && a.V >= 1024;
    a.row_dispatch = table && plain_v ? 1 : 0;
    if (plain_v && (table || sampler_row_plain(a.top_k, a.top_p, a.V))) {
        if (a.V <= 2048) sampler_plain_fast_kernel<2><<<a.R, 256, 0, st>>>(a);
        else if (a.V <= 4096) sampler_plain_fast_kernel<4><<<a.R, 256, 0, st>>>(a);
        else sampler_plain_fast_kernel<8><<<a.R, 256, 0, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (!table || e != hipSuccess) return e;
    }
    if (a.V >= 4096) { if (a.fast_math) sampler_kernel<1024, true><<<a.R, 1024, smem, st>>>(a, n2); else sampler_kernel<1024, false><<<a.R, 1024, smem, st>>>(a, n2); }
    else { if (a.fast_math) sampler_kernel<256, true><<<a.R, 256, smem, st>>>(a, n2); else sampler_kernel<256, false><<<a.R, 256, smem, st>>>(a, n2); }
    return hipGetLastError();
}

// Log-probability of the code a draw feeds forward, under the model's own distribution (T = 1, no cut-off): l[code] - max(l) - log sum exp(l - max(l)) over the RAW
// logits row the sampler has just read (launched behind it; the row is in L2).  One launch per draw (slot): workgroup b takes row b * slots + slot, 256 threads per
// row as in sampler_plain_fast_kernel -- thread t owns the float4 groups t, t + 256, ... (16-byte loads, the row stays in registers between the two passes; groups past
// V are skipped, so any V % 4 == 0 up to 1024 G4 entries works).  Two passes, IEEE expf / logf in every precision: a reported number, not a draw.  Deterministic and row-local:
// per thread a pairwise tree over its groups (padded with zeros to G4), then the xor butterfly of the wave, then the four wave sums as (w0 + w1) + (w2 + w3) -- the
// value depends on the row's bits and on V alone, never on B, the batch row or the other rows.  `feed` is indexed like `out`: the forced code where a level is forced
// (clamped into the vocabulary, as the embedding kernels clamp it), else the code the sampler wrote.
// row_max_sel / row_sums / logprob_row: the arithmetic of one row, by the 256 threads of a workgroup.  The ONE place that does it: code_logprob_kernel and
// score_logprob_kernel call logprob_row, the draw-report kernels call the same two halves and go on with the row they left in registers.
// row_max_sel: loads the row into v (groups past V are left unset and never read), returns m = max l to every thread and leaves l[code] in *sel (LDS; valid
// for every thread once the function returns).
template <int G4>
__device__ __forceinline__ float row_max_sel(const float* lg, int code, int V, float4 (&v)[G4], float* sel) {
    __shared__ float redf[4];
    const int tid = threadIdx.x;
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < G4; ++k) {
        const int i4 = tid + 256 * k;
        if (i4 * 4 < V) {                                 // V % 4 == 0
            v[k] = *reinterpret_cast<const float4*>(lg + i4 * 4);
            m = fmaxf(fmaxf(m, fmaxf(v[k].x, v[k].y)), fmaxf(v[k].z, v[k].w));
            if (i4 == (code >> 2)) { const int e = code & 3; *sel = e == 0 ? v[k].x : (e == 1 ? v[k].y : (e == 2 ? v[k].z : v[k].w)); }      // one thread of the workgroup
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) redf[tid >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
}
// one product of the entropy's T = sum expf(l - m) (l - m), rounded on its own (never contracted with the sum around it: numpy in float32 follows it step by step)
__device__ __forceinline__ float exp_times(float e, float d) {
#pragma clang fp contract(off)
    const float p = e * d;
    return p;
}
// row_sums: S = sum expf(l_i - m) and, WITH_T, T = sum expf(l_i - m) (l_i - m), to every thread; both in the one fixed order (see above): per float4 group
// (x + y) + (z + w), per thread a pairwise tree over its groups, the xor butterfly of the wave, the four wave sums as (w0 + w1) + (w2 + w3).
template <int G4, bool WITH_T>
__device__ __forceinline__ void row_sums(const float4 (&v)[G4], float m, int V, float& S, float& T) {
    __shared__ float reds[4], redt[4];
    const int tid = threadIdx.x;
    float s[G4], t[WITH_T ? G4 : 1];
#pragma unroll
    for (int k = 0; k < G4; ++k) {
        s[k] = 0.0f;
        if (WITH_T) t[k] = 0.0f;
        if ((tid + 256 * k) * 4 < V) {
            const float dx = v[k].x - m, dy = v[k].y - m, dz = v[k].z - m, dw = v[k].w - m;
            const float ex = expf(dx), ey = expf(dy), ez = expf(dz), ew = expf(dw);
            s[k] = (ex + ey) + (ez + ew);
            if (WITH_T) t[k] = (exp_times(ex, dx) + exp_times(ey, dy)) + (exp_times(ez, dz) + exp_times(ew, dw));
        }
    }
#pragma unroll
    for (int w = 1; w < G4; w <<= 1)
#pragma unroll
        for (int k = 0; k < G4; k += 2 * w) { s[k] += s[k + w]; if (WITH_T) t[k] += t[k + w]; }
    float sum = s[0], tsum = WITH_T ? t[0] : 0.0f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off, 64); if (WITH_T) tsum += __shfl_xor(tsum, off, 64); }
    if ((tid & 63) == 0) { reds[tid >> 6] = sum; if (WITH_T) redt[tid >> 6] = tsum; }
    __syncthreads();
    S = (reds[0] + reds[1]) + (reds[2] + reds[3]);
    T = WITH_T ? (redt[0] + redt[1]) + (redt[2] + redt[3]) : 0.0f;
}
// logprob_row: thread 0 stores the value of the row at `code` in *dst
template <int G4>
__device__ __forceinline__ void logprob_row(const float* lg, int code, int V, float* dst) {
    __shared__ float sel;
    float4 v[G4];
    const float m = row_max_sel<G4>(lg, code, V, v, &sel);
    float S, T;
    row_sums<G4, false>(v, m, V, S, T);
    if (threadIdx.x == 0) *dst = (sel - m) - logf(S);
}
template <int G4>
__global__ __launch_bounds__(256) void code_logprob_kernel(SamplerArgs a, const int64_t* feed, float* logprob, int slot) {
    const int V = a.V;
    const int b = blockIdx.x, r = b * a.slots + slot;
    if (row_idle(a.row_pos, b)) return;                  // workgroup-uniform: an idle row of a rolling pass has no entry
    const int step = step_of(a.state, a.row_pos, b);
    const int draw = a.draw0 + slot;
    const int draws = a.draws > 0 ? a.draws : 5;
    const long long pos = (long long)b * a.n_steps + step;
    const int code = (int)clamp_idx(feed[a.out_stride > 0 ? pos * a.out_stride + a.out_slot : pos * a.slots + slot], V);
    logprob_row<G4>(a.logits + (long long)r * V, code, V, logprob + pos * draws + draw);
}
// hqt_score: ALL rows of a sub-step in one launch, one workgroup per (pair, slot): row r = pair * slots + slot of logits [pairs * slots, V], the code
// codes[r] (the level's codes of these pairs, [pairs, slots]) -> logprob[pair * draws + draw0 + slot]; both pointers are already at the chunk's first pair
template <int G4>
__global__ __launch_bounds__(256) void score_logprob_kernel(const float* logits, const int64_t* codes, float* logprob, int V, int slots, int draw0, int draws) {
    const int r = blockIdx.x, pair = r / slots, slot = r - pair * slots;
    logprob_row<G4>(logits + (long long)r * V, (int)clamp_idx(codes[r], V), V, logprob + (long long)pair * draws + draw0 + slot);
}
hipError_t launch_score_logprob(const float* logits, const int64_t* codes, float* logprob, int pairs, int V, int slots, int draw0, int draws, hipStream_t st) {
    if (V % 4 || V > HQT_MAX_V || pairs < 1 || slots < 1 || draw0 < 0 || draw0 + slots > draws) return hipErrorInvalidValue;
    const unsigned rows = (unsigned)pairs * slots;
    if (V <= 4096) score_logprob_kernel<4><<<rows, 256, 0, st>>>(logits, codes, logprob, V, slots, draw0, draws);
    else if (V <= 8192) score_logprob_kernel<8><<<rows, 256, 0, st>>>(logits, codes, logprob, V, slots, draw0, draws);
    else score_logprob_kernel<16><<<rows, 256, 0, st>>>(logits, codes, logprob, V, slots, draw0, draws);
    return hipGetLastError();
}
hipError_t launch_code_logprob(const SamplerArgs& a, const int64_t* feed, float* logprob, int slot, hipStream_t st) {
    if (a.V % 4 || a.V > HQT_MAX_V || slot < 0 || slot >= a.slots) return hipErrorInvalidValue;
    if (a.V <= 4096) code_logprob_kernel<4><<<a.B, 256, 0, st>>>(a, feed, logprob, slot);
    else if (a.V <= 8192) code_logprob_kernel<8><<<a.B, 256, 0, st>>>(a, feed, logprob, slot);
    else code_logprob_kernel<16><<<a.B, 256, 0, st>>>(a, feed, logprob, slot);
    return hipGetLastError();
}

// Draw report (kernels.h: ReportOut): entropy, rank and the top-N of the row behind a draw, by the 256 threads that hold the row in registers as logprob_row
// holds it -- m and S come from the same two functions, so a log-probability written here has the bits code_logprob_kernel gives it.  Every index into v[] is a
// compile-time one (fully unrolled loops; what is taken is a 4 G4-bit mask per thread, tested at constant shifts): no scratch.  No atomics: every tie is decided
// by index.  The order is (value descending, index ascending) under float compares, so -0.0 and +0.0 tie and the lower index comes first; NaN logits are not
// ordered at all (finite logits are assumed, as everywhere behind the head GEMM).
__device__ __forceinline__ bool report_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// the thread's best element not yet taken; none left: (-inf, INT_MAX), which loses against every element of the row
template <int G4>
__device__ __forceinline__ void report_local_best(const float4 (&v)[G4], unsigned long long taken, float& bv, int& bi) {
    bv = -INFINITY;
    bi = INT_MAX;
#pragma unroll
    for (int k = 0; k < G4; ++k) {
        const int base = ((int)threadIdx.x + 256 * k) * 4;
        if (!((taken >> (4 * k + 0)) & 1) && report_before(v[k].x, base + 0, bv, bi)) { bv = v[k].x; bi = base + 0; }
        if (!((taken >> (4 * k + 1)) & 1) && report_before(v[k].y, base + 1, bv, bi)) { bv = v[k].y; bi = base + 1; }
        if (!((taken >> (4 * k + 2)) & 1) && report_before(v[k].z, base + 2, bv, bi)) { bv = v[k].z; bi = base + 2; }
        if (!((taken >> (4 * k + 3)) & 1) && report_before(v[k].w, base + 3, bv, bi)) { bv = v[k].w; bi = base + 3; }
    }
}
// one row: entry e of the report and, logprob_dst non-NULL, the log-probability.  r is workgroup-uniform, so every barrier below is reached by all or by none.
template <int G4>
__device__ __forceinline__ void report_row(const float* lg, int code, int V, float* logprob_dst, const ReportOut& r, long long e) {
    __shared__ float sel, wv[2][4];
    __shared__ int wi[2][4], wcnt[4];
    const int tid = threadIdx.x;
    float4 v[G4];
    const float m = row_max_sel<G4>(lg, code, V, v, &sel);
    float S, T;
    row_sums<G4, true>(v, m, V, S, T);
    const float lc = sel, logS = logf(S);
    if (tid == 0) {
        if (logprob_dst) *logprob_dst = (lc - m) - logS;
        if (r.entropy) r.entropy[e] = logS - T / S;
    }
    if (r.rank) {                                         // an integer count: elements in front of (l_c, c) in the order
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < G4; ++k) {
            const int base = (tid + 256 * k) * 4;
            if (base < V)
                cnt += (int)report_before(v[k].x, base + 0, lc, code) + (int)report_before(v[k].y, base + 1, lc, code) +
                       (int)report_before(v[k].z, base + 2, lc, code) + (int)report_before(v[k].w, base + 3, lc, code);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
        __syncthreads();
        if (tid == 0) r.rank[e] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    }
    if (r.top_n > 0) {
        // top_n rounds of a workgroup argmax: every thread offers its best element not yet taken, the wave's butterfly and then the four wave winners (through
        // LDS, two buffers in turn: one barrier per round) name the round's element, and only the thread that owns it looks for its next best
        unsigned long long taken = 0;
#pragma unroll
        for (int k = 0; k < G4; ++k) if ((tid + 256 * k) * 4 >= V) taken |= 0xFull << (4 * k);        // groups past V: never loaded, never offered
        float bv;
        int bi;
        report_local_best<G4>(v, taken, bv, bi);
        for (int j = 0; j < r.top_n; ++j) {
            float cv = bv;
            int ci = bi;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(cv, off, 64);
                const int oi = __shfl_xor(ci, off, 64);
                if (report_before(ov, oi, cv, ci)) { cv = ov; ci = oi; }
            }
            const int buf = j & 1;
            if ((tid & 63) == 0) { wv[buf][tid >> 6] = cv; wi[buf][tid >> 6] = ci; }
            __syncthreads();
            cv = wv[buf][0];
            ci = wi[buf][0];
#pragma unroll
            for (int w = 1; w < 4; ++w) if (report_before(wv[buf][w], wi[buf][w], cv, ci)) { cv = wv[buf][w]; ci = wi[buf][w]; }
            if (tid == 0) {
                r.top_codes[e * r.top_n + j] = ci;
                r.top_logprobs[e * r.top_n + j] = (cv - m) - logS;
            }
            if (ci < V && ((ci >> 2) & 255) == tid) {     // element ci = 4 (tid + 256 k) + lane: bit 4 k + lane of the owner's mask
                taken |= 1ull << (4 * (ci >> 10) + (ci & 3));
                report_local_best<G4>(v, taken, bv, bi);
            }
        }
    }
}
template <int G4>
__global__ __launch_bounds__(256) void draw_report_kernel(SamplerArgs a, const int64_t* feed, float* logprob, ReportOut rep, int slot) {
    const int V = a.V;
    const int b = blockIdx.x, r = b * a.slots + slot;
    if (row_idle(a.row_pos, b)) return;                  // workgroup-uniform: an idle row of a rolling pass has no entry
    const int step = step_of(a.state, a.row_pos, b);
    const int draw = a.draw0 + slot;
    const int draws = a.draws > 0 ? a.draws : 5;
    const long long pos = (long long)b * a.n_steps + step;
    const int code = (int)clamp_idx(feed[a.out_stride > 0 ? pos * a.out_stride + a.out_slot : pos * a.slots + slot], V);
    const long long e = pos * draws + draw;
    report_row<G4>(a.logits + (long long)r * V, code, V, logprob ? logprob + e : nullptr, rep, e);
}
template <int G4>
__global__ __launch_bounds__(256) void score_report_kernel(const float* logits, const int64_t* codes, ReportOut rep, int pair0, int V, int slots, int draw0, int draws) {
    const int r = blockIdx.x, pair = r / slots, slot = r - pair * slots;
    report_row<G4>(logits + (long long)r * V, (int)clamp_idx(codes[r], V), V, nullptr, rep, (long long)(pair0 + pair) * draws + draw0 + slot);
}
static bool report_ok(const ReportOut& rep, int V) {
    return rep.any() && rep.top_n >= 0 && rep.top_n <= 16 && rep.top_n <= V && (rep.top_n == 0 || (rep.top_codes && rep.top_logprobs));
}
hipError_t launch_draw_report(const SamplerArgs& a, const int64_t* feed, float* logprob, const ReportOut& rep, int slot, hipStream_t st) {
    if (a.V % 4 || a.V > HQT_MAX_V || slot < 0 || slot >= a.slots || !report_ok(rep, a.V)) return hipErrorInvalidValue;
    if (a.V <= 4096) draw_report_kernel<4><<<a.B, 256, 0, st>>>(a, feed, logprob, rep, slot);
    else if (a.V <= 8192) draw_report_kernel<8><<<a.B, 256, 0, st>>>(a, feed, logprob, rep, slot);
    else draw_report_kernel<16><<<a.B, 256, 0, st>>>(a, feed, logprob, rep, slot);
    return hipGetLastError();
}
hipError_t launch_score_report(const float* logits, const int64_t* codes, const ReportOut& rep, int pair0, int pairs, int V, int slots, int draw0, int draws, hipStream_t st) {
    if (V % 4 || V > HQT_MAX_V || pair0 < 0 || pairs < 1 || slots < 1 || draw0 < 0 || draw0 + slots > draws || !report_ok(rep, V)) return hipErrorInvalidValue;
    const unsigned rows = (unsigned)pairs * slots;
    if (V <= 4096) score_report_kernel<4><<<rows, 256, 0, st>>>(logits, codes, rep, pair0, V, slots, draw0, draws);
    else if (V <= 8192) score_report_kernel<8><<<rows, 256, 0, st>>>(logits, codes, rep, pair0, V, slots, draw0, draws);
    else score_report_kernel<16><<<rows, 256, 0, st>>>(logits, codes, rep, pair0, V, slots, draw0, draws);
    return hipGetLastError();
}

// Guidance: the logits rows of a pair (the same image under two conditions, two rows of one pass) become ONE row, g = l_pos + (s - 1) (l_pos - l_neg), written
// over both, in place, between the head GEMM and the sampler.  Both rows carry the same Philox key and sampler settings (engine.hip), so both draw the same code from
// the same bits and feed it forward: the two KV caches stay in step without any kernel knowing of pairs.  Workgroup (pair, slot) of a sub-step's logits
// [B * slots, V]; the pair is read from the device table at a workgroup-uniform address (every lane loads the same 20 bytes: vector loads, one cache line), so a changed table replays the same graph.  256 threads per
// row pair as in code_logprob_kernel: thread t owns the float4 groups t, t + 256, ... and skips groups past V.  V % 4 == 0 always -- hqt_create refuses any other
// vocabulary, so rows are 16-byte aligned and there is no scalar path.  Every group is read from both rows before either is written, and no other workgroup touches
// these two rows (a row is in at most one pair: checked on the host), so the update in place is safe.  s - 1, the difference, the product and the sum are four
// separately rounded fp32 operations in every precision: numpy in float32 gives the same bits, and s = 1 gives m = +-0 and hence l_pos itself (finite logits; a
// logit of -0 may come back as +0).  No LDS, no atomics, no dependence between rows of different pairs.
// guide_mix: the product must not be contracted with the sum into a v_fma.  __fsub_rn / __fmul_rn / __fadd_rn do not see to that: in this toolchain's headers they
// are the plain operators (no OCML_BASIC_ROUNDED_OPERATIONS) and, once inlined, contract like them.  What holds is the pragma on the operators themselves, as in
// split_ring.h (hipcc's default, fast-honor-pragmas, honours it); the ISA of this kernel holds v_pk_add_f32 / v_pk_mul_f32 and no v_fma / v_fmac.
__device__ __forceinline__ float guide_mix(float a, float b, float sm1) {
#pragma clang fp contract(off)
    const float d = a - b;
    const float m = sm1 * d;
    return a + m;
}
__global__ __launch_bounds__(256) void guide_logits_kernel(float* logits, const GuidePair* pairs, int V, int slots, int level) {
    const GuidePair p = pairs[blockIdx.x];
    const int slot = blockIdx.y;
    const float sm1 = p.scale[level] - 1.0f;
    float4* lp = reinterpret_cast<float4*>(logits + ((long long)p.pos_row * slots + slot) * V);
    float4* ln = reinterpret_cast<float4*>(logits + ((long long)p.neg_row * slots + slot) * V);
    for (int i4 = threadIdx.x; i4 * 4 < V; i4 += 256) {
        const float4 a = lp[i4], b = ln[i4];
        float4 g;
        g.x = guide_mix(a.x, b.x, sm1);
        g.y = guide_mix(a.y, b.y, sm1);
        g.z = guide_mix(a.z, b.z, sm1);
        g.w = guide_mix(a.w, b.w, sm1);
        lp[i4] = g;
        ln[i4] = g;
    }
}
hipError_t launch_guide_logits(float* logits, const GuidePair* pairs, int n_pairs, int V, int slots, int level, hipStream_t st) {
    if (V % 4 || V > HQT_MAX_V || n_pairs < 1 || slots < 1 || level < 0 || level > 2) return hipErrorInvalidValue;
    guide_logits_kernel<<<dim3(n_pairs, slots), 256, 0, st>>>(logits, pairs, V, slots, level);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// A9/A10/A13: codebook gather + PixelShuffle(2) + concat, NHWC output
// (quantizer.py:179-186, generator.py:316-318,361-364; sampling_hqmodel.py:119-120)
// ---------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void quant_gather_kernel(QuantArgs a) {
    const int pix = blockIdx.x;                      // b * r * r + Y * r + X
    const int r = a.r, rt = r / 2, E = a.E;
    const int b = pix / (r * r), Y = (pix / r) % r, X = pix % r;
    long long ct = -1, cb = -1;
    if (a.code_t) ct = clamp_idx(a.code_t[((long long)b * rt + (Y >> 1)) * rt + (X >> 1)], a.n_embed);
    if (a.code_b) {
        if (a.seq_layout) cb = a.code_b[(((long long)b * rt + (Y >> 1)) * rt + (X >> 1)) * 4 + (Y & 1) * 2 + (X & 1)];
        else cb = a.code_b[((long long)b * r + Y) * r + X];
        cb = clamp_idx(cb, a.n_embed);
    }
    TO* out = reinterpret_cast<TO*>(a.quant) + (long long)pix * 2 * E;
    const int sub = (Y & 1) * 2 + (X & 1);
    for (int c = threadIdx.x; c < 2 * E; c += blockDim.x) {
        float v = 0.0f;
        if (c < E) { if (ct >= 0) v = a.emb_t[ct * 4 * E + 4 * c + sub]; }        // out[c, 2h+i, 2w+j] = in[4c+2i+j, h, w]
        else if (cb >= 0) v = a.emb_b[cb * E + (c - E)];
        st1<TO>(out + c, v);
    }
}
hipError_t launch_quant_gather(const QuantArgs& a, hipStream_t st) {
    const int grid = a.B * a.r * a.r;
    if (a.out_dtype == DT_BF16) quant_gather_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
    else quant_gather_kernel<float><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

template <typename TO>
__global__ __launch_bounds__(256) void quant_gather3_kernel(QuantArgs3 a) {
    const int pix = blockIdx.x;                      // b * r * r + Y * r + X
    const int r = a.r, rm = r / 2, rt = r / 4, E = a.E;
    const int b = pix / (r * r), Y = (pix / r) % r, X = pix % r;
    long long c0 = -1, c1 = -1, c2 = -1;
    if (a.code_t) c0 = a.code_t[((long long)b * rt + (Y >> 2)) * rt + (X >> 2)];      // same index in both layouts
    if (a.code_m) {
        if (a.seq_layout) c1 = a.code_m[(((long long)b * rt + (Y >> 2)) * rt + (X >> 2)) * 4 + ((Y >> 1) & 1) * 2 + ((X >> 1) & 1)];
        else c1 = a.code_m[((long long)b * rm + (Y >> 1)) * rm + (X >> 1)];
    }
    if (a.code_b) {
        if (a.seq_layout) c2 = a.code_b[(((long long)b * rt + (Y >> 2)) * rt + (X >> 2)) * 16 + (Y & 3) * 4 + (X & 3)];
        else c2 = a.code_b[((long long)b * r + Y) * r + X];
    }
    if (c0 >= 0) c0 = clamp_idx(c0, a.n_embed);
    if (c1 >= 0) c1 = clamp_idx(c1, a.n_embed);
    if (c2 >= 0) c2 = clamp_idx(c2, a.n_embed);
    TO* out = reinterpret_cast<TO*>(a.quant) + (long long)pix * E;
    const int sub = (Y & 1) * 2 + (X & 1), subm = ((Y >> 1) & 1) * 2 + ((X >> 1) & 1);
    for (int c = threadIdx.x; c < E; c += blockDim.x) {
        float v = 0.0f;                                  // reference order: (PS(PS(q0) + q1)) + q2
        if (c0 >= 0) v = a.emb0[c0 * 16 * E + 4 * (4 * c + sub) + subm];
        if (c1 >= 0) v += a.emb1[c1 * 4 * E + 4 * c + sub];
        if (c2 >= 0) v += a.emb2[c2 * E + c];
        st1<TO>(out + c, v);
    }
}
hipError_t launch_quant_gather3(const QuantArgs3& a, hipStream_t st) {
    const int grid = a.B * a.r * a.r;
    if (a.out_dtype == DT_BF16) quant_gather3_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
    else quant_gather3_kernel<float><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

// 'nearest' / 'conv2' top level: both halves of a pixel are contiguous E-float rows, so one lane moves one 16-byte segment
// (4 channels) of one pixel; consecutive lanes cover consecutive segments of the 2E-channel output row.
template <typename TO>
__global__ __launch_bounds__(256) void quant_gather_rows_kernel(QuantRowsArgs a) {
    const int r = a.r, rt = r / 2, E = a.E, segs = 2 * E / 4;
    const long long n = (long long)a.B * r * r * segs;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / segs;
        const int c = (int)(i - pix * segs) * 4;         // first channel of this segment in [0, 2E)
        const int b = (int)(pix / (r * r)), Y = (int)((pix / r) % r), X = (int)(pix % r);
        const float* src = nullptr;
        if (c < E) {
            if (a.code_t) {
                const long long ct = clamp_idx(a.code_t[((long long)b * rt + (Y >> 1)) * rt + (X >> 1)], a.n_embed);
                const int sub = a.top_sub == 4 ? (Y & 1) * 2 + (X & 1) : 0;
                src = a.top + (ct * a.top_sub + sub) * E + c;
            } else if (a.top_null) src = a.top_null + c;
        } else if (a.code_b) {
            long long cb;
            if (a.seq_layout) cb = a.code_b[(((long long)b * rt + (Y >> 1)) * rt + (X >> 1)) * 4 + (Y & 1) * 2 + (X & 1)];
            else cb = a.code_b[((long long)b * r + Y) * r + X];
            src = a.emb_b + clamp_idx(cb, a.n_embed) * E + (c - E);
        }
        const float4 v = src ? *reinterpret_cast<const float4*>(src) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        TO* out = reinterpret_cast<TO*>(a.quant) + pix * 2 * E + c;
        if constexpr (sizeof(TO) == 4) *reinterpret_cast<float4*>(out) = v;
        else {
            uint2 pk;
            pk.x = (unsigned)f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
            pk.y = (unsigned)f32_to_bf16(v.z) | ((unsigned)f32_to_bf16(v.w) << 16);
            *reinterpret_cast<uint2*>(out) = pk;
        }
    }
}
hipError_t launch_quant_gather_rows(const QuantRowsArgs& a, hipStream_t st) {
    if (a.E % 4 || (a.top_sub != 1 && a.top_sub != 4)) return hipErrorInvalidValue;
    const long long n = (long long)a.B * a.r * a.r * (2 * a.E / 4);
    const int grid = (int)std::min<long long>((n + 255) / 256, 8192);
    if (a.out_dtype == DT_BF16) quant_gather_rows_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
    else quant_gather_rows_kernel<float><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

// ConvTranspose2d(E, E, 2, stride 2) of a codebook row (stride == kernel: every output pixel has exactly one input pixel).
// Summation order of an entry: acc = bias[co]; for ci = 0 .. E-1: acc = fma(emb[n][ci], w[ci][co][a][b], acc)  (fp32, ci ascending).
__global__ __launch_bounds__(256) void fold_upsample_t_kernel(const float* __restrict__ emb, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ table, int n_embed, int E) {
    const long long n = (long long)n_embed * 4 * E;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(i % E), ab = (int)((i / E) & 3);
        const long long row = i / (4 * E);
        const float* e = emb + row * E;
        float acc = bias[co];
        for (int ci = 0; ci < E; ++ci) acc = fmaf(e[ci], w[((long long)ci * E + co) * 4 + ab], acc);
        table[i] = acc;
    }
}
hipError_t launch_fold_upsample_t(const float* emb, const float* w, const float* bias, float* table, int n_embed, int E, hipStream_t st) {
    const long long n = (long long)n_embed * 4 * E;
    fold_upsample_t_kernel<<<(int)std::min<long long>((n + 255) / 256, 8192), 256, 0, st>>>(emb, w, bias, table, n_embed, E);
    return hipGetLastError();
}

__global__ void repack_upsample_t_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wt, float* __restrict__ bias4, int E) {
    const int n = 4 * E * E;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int ci = i % E, row = i / E, co = row % E, ab = row / E;       // wt[(ab * E + co)][ci]
        wt[i] = w[((long long)ci * E + co) * 4 + ab];
        if (ci == 0) bias4[row] = bias[co];
    }
}
hipError_t launch_repack_upsample_t(const float* w, const float* bias, float* wt, float* bias4, int E, hipStream_t st) {
    repack_upsample_t_kernel<<<std::min((4 * E * E + 255) / 256, 4096), 256, 0, st>>>(w, bias, wt, bias4, E);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// GroupNorm statistics (32 groups, eps 1e-6; stage1/modules/layers.py:17-21), NHWC input.
// One workgroup per (sample, group); sums in double.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* x, float* stats, int HW, int C, int groups, float eps) {
    __shared__ double red[4];
    const int b = blockIdx.x / groups, g = blockIdx.x % groups;
    const int cpg = C / groups;
    const T* base = x + (long long)b * HW * C + g * cpg;
    const long long n = (long long)HW * cpg;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) s += (double)ld1<T>(base + (i / cpg) * C + (i % cpg));
    const double mean = block_reduce(s, OpAdd(), red) / (double)n;
    double v = 0.0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const double t = (double)ld1<T>(base + (i / cpg) * C + (i % cpg)) - mean;
        v += t * t;
    }
    const double var = block_reduce(v, OpAdd(), red) / (double)n;
    if (threadIdx.x == 0) {
        stats[(long long)blockIdx.x * 2] = (float)mean;
        stats[(long long)blockIdx.x * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}
hipError_t launch_gn_stats(const void* x, int dtype, float* stats, int B, int HW, int C, int groups, float eps,
                           hipStream_t st) {
    if (dtype == DT_BF16) gn_stats_kernel<bf16_t><<<B * groups, 256, 0, st>>>((const bf16_t*)x, stats, HW, C, groups, eps);
    else gn_stats_kernel<float><<<B * groups, 256, 0, st>>>((const float*)x, stats, HW, C, groups, eps);
    return hipGetLastError();
}

// FAST variants: one pass over contiguous pixel chunks (every load a full 16-B vector), per-channel fp32
// partials in registers, per-group double partials to memory, tiny finalize.  Fixed-order reductions throughout
// (no atomics): the decode is bit-reproducible from run to run and from lane to lane.
// pixels per workgroup: HW/32 clamped to [64, 1024] -> 4..64 chunks per image
static inline int gn_chunk_pix(int HW) { int c = HW / 32; return c < 64 ? 64 : (c > 1024 ? 1024 : c); }
static inline bool gn_fixed_ok(int C) { return C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0; }
// 8 consecutive channels of a pixel -> fp32
template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float (&v)[8]) { bf16x8_to_f32(*reinterpret_cast<const uint4*>(p), v); }
// thread t owns channels 8 (t % vpp) .. + 7 of pixels (t / vpp) + k rpi (vpp = C / 8 vectors per pixel, rpi = 256 / vpp)
template <typename T>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* x, double* partial, int HW, int C, int groups, int nchunk, int chunk_pix) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* part = reinterpret_cast<float*>(smem_raw);      // [rpi][C] sums, then [rpi][C] sums of squares; later [C] + [C] totals
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int p0 = ch * chunk_pix, p1 = min(HW, p0 + chunk_pix);
    const int vpp = C / 8, rpi = 256 / vpp;
    const int cv = threadIdx.x % vpp, pl = threadIdx.x / vpp;
    float s[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s[i] = 0.0f; q[i] = 0.0f; }
    const T* base = x + ((long long)b * HW) * C + cv * 8;
    int p = p0 + pl;
    for (; p + 3 * rpi < p1; p += 4 * rpi) {                // four independent pixel loads in flight
        float f[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) ld8<T>(base + (long long)(p + u * rpi) * C, f[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { s[i] += f[u][i]; q[i] += f[u][i] * f[u][i]; }
        }
    }
    for (; p < p1; p += rpi) {
        float f[8];
        ld8<T>(base + (long long)p * C, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) { s[i] += f[i]; q[i] += f[i] * f[i]; }
    }
    float* ps = part + (size_t)pl * C + cv * 8;
    float* pq = part + (size_t)rpi * C + (size_t)pl * C + cv * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) { ps[i] = s[i]; pq[i] = q[i]; }
    __syncthreads();
    float ts = 0.0f, tq = 0.0f;                             // C <= 2048 channels over 256 threads: loop, fixed order over the pixel lanes
    for (int c = threadIdx.x; c < C; c += 256) {
        ts = 0.0f; tq = 0.0f;
        for (int r = 0; r < rpi; ++r) { ts += part[(size_t)r * C + c]; tq += part[(size_t)(rpi + r) * C + c]; }
        part[(size_t)2 * rpi * C + c] = ts;
        part[(size_t)2 * rpi * C + C + c] = tq;
    }
    __syncthreads();
    const float* tot = part + (size_t)2 * rpi * C;
    const int cpg = C / groups;
    for (int g = threadIdx.x; g < groups; g += 256) {
        double a = 0.0, c2 = 0.0;
        for (int i = 0; i < cpg; ++i) { a += (double)tot[g * cpg + i]; c2 += (double)tot[C + g * cpg + i]; }
        partial[((long long)blockIdx.x * groups + g) * 2] = a;
        partial[((long long)blockIdx.x * groups + g) * 2 + 1] = c2;
    }
}
// channel counts the fixed mapping does not cover (C / 8 does not divide 256, e.g. C = 96, 160, 192): the same thread <-> channel mapping with
// rpi = floor(256 / vpp) pixel lanes -- the threads beyond rpi * vpp sit the pixel loop out -- and the same fixed-order LDS pass: no atomics, so
// the statistics (and every SPLIT / FAST pixel behind them) do not depend on the order in which waves arrive.  More than 256 vectors per pixel:
// one pixel lane, a thread walks vectors t, t + 256, ...
static inline int gn_generic_rpi(int C) { const int vpp = C / 8; return vpp <= 256 ? 256 / vpp : 1; }
template <typename T>
__global__ __launch_bounds__(256) void gn_partial_generic_kernel(const T* x, double* partial, int HW, int C, int groups, int nchunk, int chunk_pix) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* part = reinterpret_cast<float*>(smem_raw);      // [rpi][C] sums, then [rpi][C] sums of squares; later [C] + [C] totals
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int p0 = ch * chunk_pix, p1 = min(HW, p0 + chunk_pix);
    const int vpp = C / 8, rpi = vpp <= 256 ? 256 / vpp : 1;
    const int pl = threadIdx.x / vpp;
    const T* img = x + ((long long)b * HW) * C;
    if (pl < rpi) {
        for (int cv = threadIdx.x - pl * vpp; cv < vpp; cv += 256) {
            float s[8], q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { s[i] = 0.0f; q[i] = 0.0f; }
            for (int p = p0 + pl; p < p1; p += rpi) {
                float f[8];
                ld8<T>(img + (long long)p * C + cv * 8, f);
#pragma unroll
                for (int i = 0; i < 8; ++i) { s[i] += f[i]; q[i] += f[i] * f[i]; }
            }
            float* ps = part + (size_t)pl * C + cv * 8;
            float* pq = part + (size_t)(rpi + pl) * C + cv * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) { ps[i] = s[i]; pq[i] = q[i]; }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {           // fixed order over the pixel lanes
        float ts = 0.0f, tq = 0.0f;
        for (int r = 0; r < rpi; ++r) { ts += part[(size_t)r * C + c]; tq += part[(size_t)(rpi + r) * C + c]; }
        part[(size_t)2 * rpi * C + c] = ts;
        part[(size_t)2 * rpi * C + C + c] = tq;
    }
    __syncthreads();
    const float* tot = part + (size_t)2 * rpi * C;
    const int cpg = C / groups;
    for (int g = threadIdx.x; g < groups; g += 256) {
        double a = 0.0, c2 = 0.0;
        for (int i = 0; i < cpg; ++i) { a += (double)tot[g * cpg + i]; c2 += (double)tot[C + g * cpg + i]; }
        partial[((long long)blockIdx.x * groups + g) * 2] = a;
        partial[((long long)blockIdx.x * groups + g) * 2 + 1] = c2;
    }
}
__global__ void gn_finalize_kernel(const double* partial, float* stats, int nchunk, int groups, double count, float eps, int n) {
    const int bg = blockIdx.x * blockDim.x + threadIdx.x;     // b * groups + g
    if (bg >= n) return;
    const int b = bg / groups, g = bg % groups;
    double a = 0.0, q = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) {
        a += partial[(((long long)b * nchunk + ch) * groups + g) * 2];
        q += partial[(((long long)b * nchunk + ch) * groups + g) * 2 + 1];
    }
    const double mean = a / count;
    const double var = fmax(q / count - mean * mean, 0.0);
    stats[(long long)bg * 2] = (float)mean;
    stats[(long long)bg * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}
// (mean, rstd) from the per-tile partials a halo conv left behind: one wave per (image, group); lane l sums tiles
// l, l + 64, ... in order and the lanes are combined by the fixed xor tree -> bit-reproducible, double accumulation
template <typename TP>
__global__ __launch_bounds__(64) void gn_finalize_tiles_kernel(const TP* partial, float* stats, int tiles, int groups, double count, float eps) {
    const int bg = blockIdx.x;                                  // b * groups + g
    const int b = bg / groups, g = bg % groups;
    double a = 0.0, q = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 64) {
        const TP* p = partial + (((long long)b * tiles + t) * groups + g) * 2;
        a += (double)p[0];
        q += (double)p[1];
    }
    a = wave_reduce(a, OpAdd());
    q = wave_reduce(q, OpAdd());
    if (threadIdx.x == 0) {
        const double mean = a / count;
        const double var = fmax(q / count - mean * mean, 0.0);
        stats[(long long)bg * 2] = (float)mean;
        stats[(long long)bg * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}
hipError_t launch_gn_finalize_tiles(const float* partial, float* stats, int B, int tiles, int HW, int C, int groups, float eps, hipStream_t st) {
    gn_finalize_tiles_kernel<float><<<B * groups, 64, 0, st>>>(partial, stats, tiles, groups, (double)HW * (C / groups), eps);
    return hipGetLastError();
}
hipError_t launch_gn_finalize_tiles_d(const double* partial, float* stats, int B, int tiles, int HW, int C, int groups, float eps, hipStream_t st) {
    gn_finalize_tiles_kernel<double><<<B * groups, 64, 0, st>>>(partial, stats, tiles, groups, (double)HW * (C / groups), eps);
    return hipGetLastError();
}
size_t gn_stats_fast_partial_elems(int B, int HW, int C, int groups) {
    (void)C;
    const int cp = gn_chunk_pix(HW);
    return (size_t)B * ((HW + cp - 1) / cp) * groups * 2;
}
hipError_t launch_gn_stats_fast(const void* x, float* stats, double* partial, int B, int HW, int C, int groups, float eps,
                                hipStream_t st, int dtype) {
    const int cp = gn_chunk_pix(HW);
    const int nchunk = (HW + cp - 1) / cp;
    if (gn_fixed_ok(C)) {
        const int rpi = 256 / (C / 8);
        const size_t smem = (size_t)(2 * rpi + 2) * C * sizeof(float);
        if (dtype == DT_F32) gn_partial_kernel<float><<<B * nchunk, 256, smem, st>>>((const float*)x, partial, HW, C, groups, nchunk, cp);
        else gn_partial_kernel<bf16_t><<<B * nchunk, 256, smem, st>>>((const bf16_t*)x, partial, HW, C, groups, nchunk, cp);
    } else {
        const size_t smem = (size_t)(2 * gn_generic_rpi(C) + 2) * C * sizeof(float);
        if (C % 8 != 0 || smem > 64 * 1024) return hipErrorInvalidValue;
        if (dtype == DT_F32) gn_partial_generic_kernel<float><<<B * nchunk, 256, smem, st>>>((const float*)x, partial, HW, C, groups, nchunk, cp);
        else gn_partial_generic_kernel<bf16_t><<<B * nchunk, 256, smem, st>>>((const bf16_t*)x, partial, HW, C, groups, nchunk, cp);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n = B * groups;
    gn_finalize_kernel<<<(n + 63) / 64, 64, 0, st>>>(partial, stats, nchunk, groups, (double)HW * (C / groups), eps, n);
    return hipGetLastError();
}

// y = swish?(gamma (x - mean) rstd + beta): a thread keeps scale/shift of its 8 channels in registers and streams
// pixels with four 16-B loads in flight (same thread <-> channel mapping as gn_partial_kernel)
__global__ __launch_bounds__(256) void gn_apply_kernel(const bf16_t* x, bf16_t* y, const float* stats, const float* gamma,
                                                       const float* beta, int HW, int C, int groups, int swish, int nchunk, int chunk_pix) {
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int p0 = ch * chunk_pix, p1 = min(HW, p0 + chunk_pix);
    const int vpp = C / 8, rpi = 256 / vpp, cpg = C / groups;
    const int cv = threadIdx.x % vpp, pl = threadIdx.x / vpp;
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = cv * 8 + i;
        const float* st = stats + ((long long)b * groups + c / cpg) * 2;
        sc[i] = st[1] * gamma[c];
        sh[i] = beta[c] - st[0] * sc[i];
    }
    const long long off = ((long long)b * HW) * C + cv * 8;
    auto norm_store = [&](const uint4& raw, long long pix) {
        float f[8];
        bf16x8_to_f32(raw, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float t = fmaf(f[i], sc[i], sh[i]);
            if (swish) t = t * __builtin_amdgcn_rcpf(1.0f + __expf(-t));
            f[i] = t;
        }
        uint4 o;
        o.x = (unsigned)f32_to_bf16(f[0]) | ((unsigned)f32_to_bf16(f[1]) << 16);
        o.y = (unsigned)f32_to_bf16(f[2]) | ((unsigned)f32_to_bf16(f[3]) << 16);
        o.z = (unsigned)f32_to_bf16(f[4]) | ((unsigned)f32_to_bf16(f[5]) << 16);
        o.w = (unsigned)f32_to_bf16(f[6]) | ((unsigned)f32_to_bf16(f[7]) << 16);
        *reinterpret_cast<uint4*>(y + off + pix * C) = o;
    };
    int p = p0 + pl;
    for (; p + 3 * rpi < p1; p += 4 * rpi) {
        uint4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = *reinterpret_cast<const uint4*>(x + off + (long long)(p + u * rpi) * C);
#pragma unroll
        for (int u = 0; u < 4; ++u) norm_store(r[u], p + u * rpi);
    }
    for (; p < p1; p += rpi) norm_store(*reinterpret_cast<const uint4*>(x + off + (long long)p * C), p);
}
__global__ __launch_bounds__(256) void gn_apply_generic_kernel(const bf16_t* x, bf16_t* y, const float* stats, const float* gamma,
                                                               const float* beta, long long total_vec, int HW, int C, int groups, int swish) {
    const int cpg = C / groups, vec_per_pix = C / 8;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < total_vec; v += (long long)gridDim.x * blockDim.x) {
        const long long pix = v / vec_per_pix;
        const int c8 = (int)(v - pix * vec_per_pix) * 8;
        const int b = (int)(pix / HW);
        float f[8];
        bf16x8_to_f32(*reinterpret_cast<const uint4*>(x + v * 8), f);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* st = stats + ((long long)b * groups + (c8 + i) / cpg) * 2;
            const float scl = st[1] * gamma[c8 + i];
            float t = fmaf(f[i], scl, beta[c8 + i] - st[0] * scl);
            if (swish) t = t * __builtin_amdgcn_rcpf(1.0f + __expf(-t));
            f[i] = t;
        }
        uint4 o;
        o.x = (unsigned)f32_to_bf16(f[0]) | ((unsigned)f32_to_bf16(f[1]) << 16);
        o.y = (unsigned)f32_to_bf16(f[2]) | ((unsigned)f32_to_bf16(f[3]) << 16);
        o.z = (unsigned)f32_to_bf16(f[4]) | ((unsigned)f32_to_bf16(f[5]) << 16);
        o.w = (unsigned)f32_to_bf16(f[6]) | ((unsigned)f32_to_bf16(f[7]) << 16);
        *reinterpret_cast<uint4*>(y + v * 8) = o;
    }
}
hipError_t launch_gn_apply(const void* x, void* y, const float* stats, const float* gamma, const float* beta, int B, int HW,
                           int C, int groups, int swish, hipStream_t st) {
    if (gn_fixed_ok(C)) {
        const int cp = gn_chunk_pix(HW);
        const int nchunk = (HW + cp - 1) / cp;
        gn_apply_kernel<<<B * nchunk, 256, 0, st>>>((const bf16_t*)x, (bf16_t*)y, stats, gamma, beta, HW, C, groups, swish, nchunk, cp);
        return hipGetLastError();
    }
    const long long total_vec = (long long)B * HW * C / 8;
    const int grid = (int)std::min<long long>((total_vec + 255) / 256, 256 * 16);
    gn_apply_generic_kernel<<<grid, 256, 0, st>>>((const bf16_t*)x, (bf16_t*)y, stats, gamma, beta, total_vec, HW, C, groups, swish);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// row softmax (decoder AttnBlock, stage1/modules/layers.py:177), in place
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(T* x, int n) {
    __shared__ float red[4];
    T* row = x + (long long)blockIdx.x * n;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, ld1<T>(row + i));
    m = block_reduce(m, OpMax(), red);
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += expf(ld1<T>(row + i) - m);
    s = block_reduce(s, OpAdd(), red);
    for (int i = threadIdx.x; i < n; i += blockDim.x) st1<T>(row + i, expf(ld1<T>(row + i) - m) / s);
}
hipError_t launch_softmax_rows(void* x, int dtype, int rows, int n, hipStream_t st) {
    if (dtype == DT_BF16) softmax_rows_kernel<bf16_t><<<rows, 256, 0, st>>>((bf16_t*)x, n);
    else softmax_rows_kernel<float><<<rows, 256, 0, st>>>((float*)x, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// HQ-VAE encode side: image layout, nearest-code search bookkeeping (the distance GEMM itself is STORE_ARGMIN)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void image_to_nhwc_kernel(const float* __restrict__ img, T* __restrict__ out, int B, int R, int cpad) {
    const long long npix = (long long)B * R * R;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const long long b = p / ((long long)R * R), pix = p - b * R * R;
        for (int c = 0; c < cpad; ++c) {
            const float v = c < 3 ? img[(b * 3 + c) * R * R + pix] : 0.0f;
            st1<T>(out + p * cpad + c, v);
        }
    }
}
hipError_t launch_image_to_nhwc(const float* img, void* out, int out_dtype, int B, int R, int cpad, hipStream_t st) {
    const long long npix = (long long)B * R * R;
    const int blocks = (int)std::min<long long>((npix + 255) / 256, 4096);
    if (out_dtype == DT_BF16) image_to_nhwc_kernel<bf16_t><<<blocks, 256, 0, st>>>(img, (bf16_t*)out, B, R, cpad);
    else image_to_nhwc_kernel<float><<<blocks, 256, 0, st>>>(img, (float*)out, B, R, cpad);
    return hipGetLastError();
}

// fixed-order sum over the 256 threads of a workgroup (same result on every run)
__device__ inline float block_sum_256(float v, float* sh) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[wave] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <typename T>
__global__ __launch_bounds__(256) void row_sumsq_kernel(const T* __restrict__ rows, float* __restrict__ out, int M, int K) {
    __shared__ float sh[4];
    const int m = blockIdx.x;
    float acc = 0.0f;
    for (int k = threadIdx.x; k < K; k += 256) { const float v = ld1<T>(rows + (long long)m * K + k); acc += v * v; }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) out[m] = acc;
}
hipError_t launch_row_sumsq(const void* rows, int dtype, float* out, int M, int K, hipStream_t st) {
    if (dtype == DT_BF16) row_sumsq_kernel<bf16_t><<<M, 256, 0, st>>>((const bf16_t*)rows, out, M, K);
    else row_sumsq_kernel<float><<<M, 256, 0, st>>>((const float*)rows, out, M, K);
    return hipGetLastError();
}

// (level row m = (b, y, x), level column cq)  ->  offset into the bottom-layout NHWC [B, r, r, E] tensors
__device__ __forceinline__ long long vq_bottom_off(int b, int y, int x, int cq, int k, int r, int E) {
    int c = cq;
    for (int t = 0; t < k; ++t) {           // PixelUnshuffle(2): channel c * 4 + 2 i + j of the coarse map = channel c at (2 y + i, 2 x + j)
        const int j = c & 1, i = (c >> 1) & 1;
        c >>= 2;
        y = 2 * y + i; x = 2 * x + j;
    }
    return (((long long)b * r + y) * r + x) * E + c;
}

template <typename T>
__global__ __launch_bounds__(256) void vq_rows_kernel(VqArgs a) {
    __shared__ float sh[4];
    const int rq = a.r >> a.k, dim = a.E << (2 * a.k);
    const int m = blockIdx.x;
    const int b = m / (rq * rq), pix = m - b * rq * rq, y = pix / rq, x = pix - y * rq;
    T* zrow = reinterpret_cast<T*>(a.z) + (long long)m * dim;
    float acc = 0.0f;
    for (int cq = threadIdx.x; cq < dim; cq += 256) {
        const long long o = vq_bottom_off(b, y, x, cq, a.k, a.r, a.E);
        float v = a.h[o];
        if (a.recon) v = v - a.recon[o];                    // generator.py:303 / 544: h - upsampled coarser quant
        if (a.resid_nchw) a.resid_nchw[((long long)b * dim + cq) * rq * rq + pix] = v;
        st1<T>(zrow + cq, v);
        const float vr = ld1<T>(zrow + cq);                  // the value the distance GEMM will read
        acc += vr * vr;
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) a.zz[m] = acc;
}
hipError_t launch_vq_rows(const VqArgs& a, hipStream_t st) {
    const int rq = a.r >> a.k, M = a.B * rq * rq;
    if (a.z_dtype == DT_BF16) vq_rows_kernel<bf16_t><<<M, 256, 0, st>>>(a);
    else vq_rows_kernel<float><<<M, 256, 0, st>>>(a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void vq_finish_kernel(VqArgs a) {
    __shared__ float sh[4];
    const int rq = a.r >> a.k, dim = a.E << (2 * a.k);
    const int m = blockIdx.x;
    const int b = m / (rq * rq), pix = m - b * rq * rq, y = pix / rq, x = pix - y * rq;
    const long long code = (long long)(a.best[m] & 0xffffffffull);
    if (threadIdx.x == 0) a.codes[m] = code;
    const float* e = a.emb + code * dim;
    float acc = 0.0f;
    for (int cq = threadIdx.x; cq < dim; cq += 256) {
        const long long o = vq_bottom_off(b, y, x, cq, a.k, a.r, a.E);
        const float rec = a.recon ? a.recon[o] : 0.0f;
        const float z = a.recon ? a.h[o] - rec : a.h[o];
        const float d = e[cq] - z;
        acc += d * d;                                        // quantizer.py:130 (before the straight-through form)
        const float q = z + d;                               // quantizer.py:131: z + (z_q - z).detach()
        if (a.quant_nchw) a.quant_nchw[((long long)b * dim + cq) * rq * rq + pix] = q;
        if (a.recon) a.recon[o] = q + rec;                   // generator.py:552: _quant + recons[-1], then pixel-shuffled (= this layout)
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) a.err_rows[m] = acc;
}
hipError_t launch_vq_finish(const VqArgs& a, hipStream_t st) {
    const int rq = a.r >> a.k, M = a.B * rq * rq;
    vq_finish_kernel<<<M, 256, 0, st>>>(a);
    return hipGetLastError();
}

// AvgPool2d(2) over the bottom-layout feature map, one 16-byte channel segment of one top row per lane.  Order of the four terms:
// ((h[2y][2x] + h[2y][2x+1]) + h[2y+1][2x]) + h[2y+1][2x+1], then * 0.25 (exact): the window order of torch's avg_pool2d.
__global__ __launch_bounds__(256) void vq_avgpool_rows_kernel(const float* __restrict__ h, float* __restrict__ rows, int B, int r, int E) {
    const int rq = r / 2, segs = E / 4;
    const long long n = (long long)B * rq * rq * segs;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / segs;
        const int c = (int)(i - m * segs) * 4;
        const int b = (int)(m / (rq * rq)), y = (int)((m / rq) % rq), x = (int)(m % rq);
        const float* p = h + (((long long)b * r + 2 * y) * r + 2 * x) * E + c;
        const float4 v00 = *reinterpret_cast<const float4*>(p), v01 = *reinterpret_cast<const float4*>(p + E);
        const float4 v10 = *reinterpret_cast<const float4*>(p + (long long)r * E), v11 = *reinterpret_cast<const float4*>(p + (long long)r * E + E);
        float4 o;
        o.x = (((v00.x + v01.x) + v10.x) + v11.x) * 0.25f;
        o.y = (((v00.y + v01.y) + v10.y) + v11.y) * 0.25f;
        o.z = (((v00.z + v01.z) + v10.z) + v11.z) * 0.25f;
        o.w = (((v00.w + v01.w) + v10.w) + v11.w) * 0.25f;
        *reinterpret_cast<float4*>(rows + m * E + c) = o;
    }
}
hipError_t launch_vq_avgpool_rows(const float* h, float* rows, int B, int r, int E, hipStream_t st) {
    if (E % 4 || r % 2) return hipErrorInvalidValue;
    const long long n = (long long)B * (r / 2) * (r / 2) * (E / 4);
    vq_avgpool_rows_kernel<<<(int)std::min<long long>((n + 255) / 256, 8192), 256, 0, st>>>(h, rows, B, r, E);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void vq_finish_top_kernel(VqTopArgs a) {
    __shared__ float sh[4];
    const int rq = a.r / 2, E = a.E;
    const int m = blockIdx.x;
    const int b = m / (rq * rq), pix = m - b * rq * rq, y = pix / rq, x = pix - y * rq;
    const long long code = (long long)(a.best[m] & 0xffffffffull);
    if (threadIdx.x == 0) a.codes[m] = code;
    const float* e = a.emb + code * E;
    const float* zrow = a.z + (long long)m * E;
    float acc = 0.0f;
    for (int c = threadIdx.x; c < E; c += 256) {
        const float z = zrow[c];
        const float d = e[c] - z;
        acc += d * d;                                        // quantizer.py:130
        const float q = z + d;                               // quantizer.py:131: z + (z_q - z).detach()
        if (a.quant_nchw) a.quant_nchw[((long long)b * E + c) * rq * rq + pix] = q;
        if (a.q_rows) a.q_rows[(long long)m * E + c] = q;
        if (a.recon) {                                       // nearest x2: bottom pixel (Y, X) reads top entry (Y / 2, X / 2)
            float* o = a.recon + (((long long)b * a.r + 2 * y) * a.r + 2 * x) * E + c;
            o[0] = q; o[E] = q; o[(long long)a.r * E] = q; o[(long long)a.r * E + E] = q;
        }
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) a.err_rows[m] = acc;
}
hipError_t launch_vq_finish_top(const VqTopArgs& a, hipStream_t st) {
    const int rq = a.r / 2;
    vq_finish_top_kernel<<<a.B * rq * rq, 256, 0, st>>>(a);
    return hipGetLastError();
}

// one 16-byte segment per lane on both sides: up row m = (b, y, x) holds the four output pixels (a, b') of its block as E-float runs
__global__ __launch_bounds__(256) void vq_scatter_up_kernel(const float* __restrict__ up, float* __restrict__ recon, int B, int r, int E) {
    const int rq = r / 2, segs = 4 * E / 4;
    const long long n = (long long)B * rq * rq * segs;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / segs;
        const int col = (int)(i - m * segs) * 4;             // (a * 2 + b') * E + co
        const int ab = col / E, co = col - ab * E;
        const int b = (int)(m / (rq * rq)), y = (int)((m / rq) % rq), x = (int)(m % rq);
        const float4 v = *reinterpret_cast<const float4*>(up + m * 4 * E + col);
        *reinterpret_cast<float4*>(recon + (((long long)b * r + 2 * y + (ab >> 1)) * r + 2 * x + (ab & 1)) * E + co) = v;
    }
}
hipError_t launch_vq_scatter_up(const float* up, float* recon, int B, int r, int E, hipStream_t st) {
    if (E % 4 || r % 2) return hipErrorInvalidValue;
    const long long n = (long long)B * (r / 2) * (r / 2) * E;
    vq_scatter_up_kernel<<<(int)std::min<long long>((n + 255) / 256, 8192), 256, 0, st>>>(up, recon, B, r, E);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void vq_diff_kernel(const float* __restrict__ err_rows, int M, float scale, float* __restrict__ diff) {
    __shared__ float sh[4];
    float acc = 0.0f;
    for (int m = threadIdx.x; m < M; m += 256) acc += err_rows[m];
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) diff[0] = acc * scale;
}
hipError_t launch_vq_diff(const float* err_rows, int M, float scale, float* diff, hipStream_t st) {
    vq_diff_kernel<<<1, 256, 0, st>>>(err_rows, M, scale, diff);
    return hipGetLastError();
}

__global__ void nhwc_to_nchw_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int hw, int C) {
    const long long n = (long long)B * hw * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / ((long long)hw * C), rem = i - b * hw * C;
        const int c = (int)(rem / hw), p = (int)(rem - (long long)c * hw);          // i indexes the NCHW output
        out[i] = in[(b * hw + p) * C + c];
    }
}
hipError_t launch_nhwc_to_nchw_f32(const float* in, float* out, int B, int hw, int C, hipStream_t st) {
    const long long n = (long long)B * hw * C;
    nhwc_to_nchw_f32_kernel<<<(int)std::min<long long>((n + 255) / 256, 4096), 256, 0, st>>>(in, out, B, hw, C);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// generic GEMM dispatch
// ---------------------------------------------------------------------------------------------
hipError_t launch_gemm_generic(const GemmArgs& g, int ta, int tb, int tc, hipStream_t st) {
    if (g.K % 16 != 0 || (g.conv_taps && g.Cin % 4 != 0)) return hipErrorInvalidValue;
    const dim3 grid((g.N + 63) / 64, (g.M + 63) / 64, g.batch > 0 ? g.batch : 1);
    const int key = ta * 4 + tb * 2 + tc;
    switch (key) {
        case 0:
            // plain fp32 nn.Linear (the AR loop): the four-quarter summation order exact_mfma_gemm_kernel shares (exact_gemm.hip)
            if (g.k_quarters && !g.conv_taps && !g.a_packed_mb && !g.a_rows_per_group && g.batch <= 1 && !g.gn_stats && g.K % 32 == 0 && (g.store == STORE_ROWS || g.store == STORE_QKV))
                gemm_tile_kernel<float, float, float, true><<<grid, 256, 0, st>>>(g);
            else gemm_tile_kernel<float, float, float><<<grid, 256, 0, st>>>(g);
            break;
        case 7: gemm_tile_kernel<bf16_t, bf16_t, bf16_t><<<grid, 256, 0, st>>>(g); break;
        case 6: gemm_tile_kernel<bf16_t, bf16_t, float><<<grid, 256, 0, st>>>(g); break;
        case 2: gemm_tile_kernel<float, bf16_t, float><<<grid, 256, 0, st>>>(g); break;
        case 3: gemm_tile_kernel<float, bf16_t, bf16_t><<<grid, 256, 0, st>>>(g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
