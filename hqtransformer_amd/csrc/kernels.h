// Host-side launch wrappers of every kernel in libhqt.so.  All asynchronous on `st`.
#pragma once
#include "common.h"

enum { DT_F32 = 0, DT_BF16 = 1 };

// generic GEMM (vector ALUs).  ta/tb/tc are DT_*.
hipError_t launch_gemm_generic(const GemmArgs& g, int ta, int tb, int tc, hipStream_t st);
// EXACT nn.Linear of the AR loop on the fp32 matrix instructions, one T x T tile per wave (exact_gemm.hip)
bool exact_mfma_ok(const GemmArgs& g);
hipError_t launch_exact_mfma_gemm(const GemmArgs& g, hipStream_t st);
hipError_t launch_pack_exact_tiles(const float* w, float* out, int N, int K, hipStream_t st);   // fp32 [N][K] -> MFMA fragment order [N / 16][K / 32][chunk][lane][4]

struct EmbedArgs {
    int B, D, n_steps;
    int embedding;               // HQT_EMB_*
    int cond_type;               // HQT_COND_*
    const StepState* state;      // position = state->step
    const int64_t* cond;         // [B] class ids (class-cond)
    const float* sos;            // class: [n_classes, D]; uncond: [D]
    const float* tok_top;        // [V, D]
    const float* tok_bot;        // [V, D] or [V, D/4]
    const float* pos_top;        // [ctx_img, D]
    const float* pos_emb;        // [5, D] (transformer1)
    const int64_t* codes_top;    // [B, n_steps]    (drawn or teacher-forced)
    const int64_t* codes_bot;    // [B, n_steps, 4]
    float* x;                    // [B, D]
    bf16_t* xpk;                 // optional: bf16 copy in the packed_off() layout (pk_mb) + row statistics (FAST deferred LN)
    int pk_mb;
    float* parts;                // [1][32 pk_mb][2] (sum, sumsq) of the bf16 copy
    // three code levels (HQTransformer, hqtransformer.py:466-488): mean over 1 + 4 + 16 tokens; tok_top / tok_bot are then
    // tok_emb_levels.0 / .1, pos_emb has 21 rows
    int levels;                  // 0 or 2: two levels; 3: three
    const float* tok_l2;         // [V, D] tok_emb_levels.2
    const int64_t* codes_l2;     // [B, n_steps, 16]
    int V, n_classes;            // table sizes for the index clamp (0: unchecked)
    const int* row_pos;          // rolling pass (embed_step only): sample b stands at row_live(row_pos, b) in place of state->step; NULL: the step state.
                                 // An idle row (row_pos[b] < 0) gets a row of zeros: sos (NULL on a text handle), cond and the codes are not read for it
};
hipError_t launch_embed_step(const EmbedArgs& a, hipStream_t st);
// prefix prefill: x[b * stride + row_off + j] = body input row step_off + j of sample b, j < rows (row 0: sos; row s: position s - 1's codes),
// the arithmetic of launch_embed_step; `state` is not read and no packed copy is written
hipError_t launch_embed_prefix(const EmbedArgs& a, int rows, int stride, int row_off, int step_off, hipStream_t st);
// dst[b, p < P, :] = src[b, p, :] for one code level (dst [B, n_steps, width], src [B, P, width]), clamped into [0, V)
hipError_t launch_copy_prefix(const int64_t* src, int64_t* dst, int B, int P, int n_steps, int width, int V, hipStream_t st);
// The masked sibling (hqt_set_keep_mask): dst[b, t, :] = clamp(src[b, t, :]) where keep[b * n_steps + t] != 0, both [B, n_steps, width]; other entries of dst are left alone
hipError_t launch_copy_kept(const int64_t* src, int64_t* dst, const unsigned char* keep, int B, int n_steps, int width, int V, hipStream_t st);
// The per-row-span sibling (a rolling pass with a keep table): row b takes only the kept positions of [pos[b], pos[b] + (pos[b] == 0 ? k0 : k)) clipped to n_steps
// (pos: device, [B], the table as received; k0 >= k); rows with pos[b] < 0 and positions outside the span are neither read nor written
hipError_t launch_copy_kept_rows(const int64_t* src, int64_t* dst, const unsigned char* keep, const int* pos, int B, int n_steps, int width, int k, int k0, int V,
                                 hipStream_t st);
// The gathered sibling of launch_embed_prefix (the join phase of a rolling pass): row b of the pass whose g = group_of_row[b] (device, [a.B]) lies in [0, G) writes
// x[g * stride + row_off + j] = its body input row step_off + j, j < rows; other rows are neither read nor written
hipError_t launch_embed_prefix_rows(const EmbedArgs& a, const int* group_of_row, int G, int rows, int stride, int row_off, int step_off, hipStream_t st);

// text prompt: x[b * rows_per_sample + t, :] = tok_emb_txt[cond[b, t]] + pos_emb_txt[t]
hipError_t launch_embed_text(const int64_t* cond, const float* tok, const float* pos, float* x, int B, int T, int D,
                             hipStream_t st, int vocab = 0, int rows_per_sample = 0);      // rows_per_sample 0: T

// the prompts of the rows that join a rolling pass: x[g * rows_per_sample + t, :] = tok_emb_txt[cond[b, t]] + pos_emb_txt[t] for every row b of cond [B, T] whose
// g = group_of_row[b] (device, [B]) lies in [0, G); other rows are neither read nor written
hipError_t launch_embed_text_rows(const int64_t* cond, const int* group_of_row, const float* tok, const float* pos, float* x, int B, int G, int T, int D,
                                  hipStream_t st, int vocab, int rows_per_sample = 0);      // rows_per_sample 0: T

// Shared prompts (hqt_set_prompt_groups) and the join phase of a rolling pass (T = the rows per joiner: prompt or sos row, then its kept run): the prefill ran
// over G distinct prompts into a staging K/V of [n_layers][G][T][row_bytes]; one launch hands
// every row b of the pass the prompt of its group g = group_of_row[b] (device, B entries):
//   cache slot b, tokens 0 .. T - 1 of every layer <- staging rows of g (K and V; the cache is [n_layers][cache_slots][Tcache][row_bytes]),
//   x_out[b, :] <- x_src[g * T + T - 1, :] (fp32 [., D]: the last prompt row of the residual stream; x_out must not overlap x_src)
// A pure byte copy (row_bytes = D * sizeof(activation)); rows whose group is outside [0, G) are left alone.
struct FanoutArgs {
    const void *k_src, *v_src;   // staging
    void *k_dst, *v_dst;         // the handle's cache
    const float* x_src;          // [G * T, D]
    float* x_out;                // [B, D]
    const int* group_of_row;     // device, [B]
    int n_layers, B, G, T, D;
    int row_bytes;               // D * sizeof(activation)
    int cache_slots, Tcache;     // max_batch and Tmax of the cache
};
hipError_t launch_prompt_fanout(const FanoutArgs& a, hipStream_t st);

// Paused passes (hqt_select_rows): cache slot j of every layer <- what slot rows_from[j] held, j < B_new, for the first live_bytes bytes of a slot (the live
// tokens 0 .. t_base - 1, contiguous), K and V, in place: any mapping (identity, permutation, subset, duplicates, B_new above the paused row count).  A pure byte
// copy through LDS; entries of rows_from outside [0, cache_slots) move nothing.  B_new * 16 bytes must fit kv_gather_lds_limit() (the CU's LDS).
struct KvGatherArgs {
    void *k, *v;                 // the handle's cache, [n_layers][cache_slots][slot_bytes]
    const int* rows_from;        // device, [B_new]
    int n_layers, B_new, cache_slots;
    long long slot_bytes;        // Tmax * D * sizeof(activation)
    long long live_bytes;        // t_base * D * sizeof(activation)
};
size_t kv_gather_lds_limit();
hipError_t launch_kv_gather_rows(const KvGatherArgs& a, hipStream_t st);
// dst[b, p, :] = src[b, p, :] for p in [p0, p1), both [B, n_steps, width] (one code level of a segment, hqt_set_segment)
hipError_t launch_copy_positions(const int64_t* src, int64_t* dst, int B, int n_steps, int width, int p0, int p1, hipStream_t st);

// dst[b, p, :] = src[b, p, :] for p in [pos[b] + lo, pos[b] + hi) clipped to [0, n_steps), rows with pos[b] < 0 skipped (pos: device, [B]; a rolling pass)
hipError_t launch_copy_row_positions(const int64_t* src, int64_t* dst, const int* pos, int B, int n_steps, int width, int lo, int hi, hipStream_t st);

// depth sub-step 1 input: x[b*4+s, :] = tok_top_depth[top[b, step]] + pos_depth[s]
hipError_t launch_depth_embed(const int64_t* codes_top, int n_steps, const StepState* state, const float* tok,
                              const float* pos, float* x, int B, int D, bf16_t* xpk, int pk_mb, float* parts, hipStream_t st, int V = 0, int tok_ld = 0,
                              const int* row_pos = nullptr);      // row_pos (here and in the two launchers below): a rolling pass, step = row_live(row_pos, b)

// hqt_score: launch_depth_embed over a chunk of pairs addressed by pair index -- rows [4 i, 4 i + 4) from codes_top[pair0 + i], i < pairs (codes_top [B n])
hipError_t launch_score_depth_embed(const int64_t* codes_top, int pair0, int pairs, const float* tok, const float* pos, float* x, int D, bf16_t* xpk,
                                    int pk_mb, float* parts, hipStream_t st, int V = 0, int tok_ld = 0);

struct LNArgs {
    float* x;                    // [rows_in, D]; rewritten in place when split-K slabs are folded in
    const float* gamma;
    const float* beta;
    const float* add;            // optional [D] vector added after the affine (sos_depth)
    void* y;                     // [M, D] fp32 or bf16
    int M, D;
    int in_rows_per_group;       // input row = m * in_rows_per_group + in_row_offset  (pick one token per sample)
    int in_row_offset;
    float eps;
    int out_dtype;               // DT_*
    int out_packed_mb;           // > 0: write y in the packed_off() layout (bf16 only)
    // pending split-K residual of the previous GEMM: x[m] += slab_bias + sum_s slabs[s][m][:] before normalising
    const float* slabs;          // [n_slabs][slab_rows][D] fp32 or NULL
    int n_slabs;
    int slab_rows;
    const float* slab_bias;      // [D] or NULL
    // optional second output for the FAST deferred-LN path: bf16 packed copy of y (fp32 out) + its row statistics
    bf16_t* ypk;
    int ypk_mb;
    float* yparts;
    // bidirectional depth head only (launch_bidir_*)
    const float* fill;           // [4, D] rows 1..4 of every sample's depth input (pos_emb_depth)
    const float* gamma2;         // ln_bot affine of rows 1..4
    const float* beta2;
    void* y2;                    // [4 B, D] bottom-head operand
    int out2_packed_mb;
};
hipError_t launch_layernorm(const LNArgs& a, hipStream_t st);
// hqt_score, depth input of level 0 for a chunk of a.M (sample, position) pairs: row m (bidirectional, a.fill non-NULL: row 5 m, then the four fill rows, as
// launch_bidir_depth_input) = ln_f + add of body row b * stride + off + t of pair p = pair0 + m = b n + t; a.in_rows_per_group / in_row_offset are not read.
// fp32 y, optional packed copy + row statistics (ypk); the row arithmetic is launch_layernorm's own (ln_row)
hipError_t launch_score_depth_input(const LNArgs& a, int pair0, int n, int stride, int off, hipStream_t st);
// bidirectional depth head (hierarchical_ar.py:803-826): x[b] = last body row of sample b (in_rows_per_group / in_row_offset) ->
// y rows [5 b] = ln_f(x[b]) + add, [5 b + 1 .. 5 b + 4] = fill[0..3]; fp32 y, optional packed copy + row statistics (ypk)
hipError_t launch_bidir_depth_input(const LNArgs& a, hipStream_t st);
// M = 5 B depth rows: row 5 b -> ln_top into row b of y, row 5 b + 1 + s -> ln_bot into row 4 b + s of y2
hipError_t launch_bidir_head_ln(const LNArgs& a, hipStream_t st);

struct AttnArgs {
    const void* q;               // [B*Tq, D]
    const void* kcache;          // [B, Tmax, D]
    const void* vcache;
    void* out;                   // [B*Tq, D]
    int B, Tq, n_heads, head_dim, Tmax;
    int t_base;                  // keys already cached before this call's Tq tokens
    const int* t_base_dev;       // optional device int added to t_base
    int causal;                  // 1: query i sees keys [0, t_base + i]; 0: all t_base + Tq keys
    int dtype;                   // DT_* of q / cache / out
    int out_packed_mb;           // > 0: write out in the packed_off() layout
    long long* dbg;              // tools/micro only: per-wave clock stamps (NULL in the product)
    const int* row_pos;          // rolling pass, Tq == 1 (attention_kernel / attention_heads8_kernel): sample b has row_live(row_pos, b) keys cached in place of *t_base_dev
};
// Which kernel of attention.hip serves a call: the one choice, read by launch_attention (which switches on it) and by the timing report
// ("variant:attn_<name>:<body|depth>", counted in run_block).  ATTN_INVALID: a head size no kernel takes.
enum AttnKernel { ATTN_INVALID = 0, ATTN_FEWQ1, ATTN_FEWQ2, ATTN_FEWQ8, ATTN_PREFILL_MFMA, ATTN_PREFILL_TILED, ATTN_HEADS8, ATTN_GENERIC };
AttnKernel attention_choice(const AttnArgs& a);
const char* attention_kernel_name(AttnKernel k);      // "fewq1", "fewq2", "fewq8", "prefill_mfma", "prefill_tiled", "heads8", "generic"
hipError_t launch_attention(const AttnArgs& a, hipStream_t st);

struct SamplerArgs {
    const float* logits;         // [R, V], row r = b * slots + slot
    int R, V, slots, B;
    float temperature;
    int top_k;                   // <= 0: none
    float top_p;                 // <= 0: none
    const float* noise;          // [n_steps, 5, B, V] or NULL
    int draw0;                   // first draw index of slot 0 (0 for top, 1 for bottom; 5 for the third level)
    const StepState* state;      // step of the current call
    const RowKey* rows;          // [B] Philox seed and global row index of every batch row (merged steps: they differ per row)
    int n_steps;
    int64_t* out;                // top: [B, n_steps]; bottom: [B, n_steps, 4]
    float* logits_out;           // optional [n_steps, draws, B, V]
    int draws;                   // draws per top position: 5 (two levels; 0 means 5) or 21 (three levels) -- noise / logits_out stride
    // ---- fused embedding lookup of the code just drawn (top draw, slots == 1): the four input rows of depth sub-step 1,
    //      x[(b * 4 + s)] = emb_tok[code] + emb_pos[s] (hierarchical_ar.py:705-712), plus the packed bf16 copy and row statistics
    //      the deferred-LayerNorm GEMMs read.  emb_tok == NULL: no fusion (depth_embed_kernel does it).
    const float* emb_tok;        // [V, D]
    const float* emb_pos;        // [>= 4, D]
    const int64_t* emb_feed;     // code to embed instead of the drawn one (teacher forcing), same indexing as `out`; NULL: the drawn code
    float* emb_x;                // [4 B, D]
    int emb_D;
    bf16_t* emb_xpk;             // optional packed copy (packed_off layout with emb_pk_mb row blocks)
    int emb_pk_mb;
    float* emb_parts;            // [4 B][2]
    int out_stride, out_slot;    // out_stride > 0: the drawn code goes to out[(b * n_steps + step) * out_stride + out_slot] (slots == 1: one sub-step of the
                                 // 21-step causal head writes ONE slot of a 4- or 16-wide code group)
    int fast_math;               // FAST-precision calls: v_exp / v_log / v_rcp forms of exp, log and the divisions (1-2 ulp each; EXACT keeps the IEEE forms: its draws are the parity gate, compared bit for bit)
    // ---- per-row settings (hqt_set_row_samplers): row b draws with temperature[row_lv_t], top_k[row_lv_k], top_p[row_lv_k] of row_set[b] in place of the three
    //      scalars above (the two indices differ under the bidirectional head only).  NULL: the scalars, for every row.
    const RowSampler* row_set;   // [B], device
    int row_lv_t, row_lv_k;
    int row_top_p;               // some row of the table uses top-p: the general kernel's LDS is sized for it (a launch-time choice, so a host-side one)
    int row_dispatch;            // set by launch_sampler: both kernels run over the pass and a workgroup leaves at once when its row belongs to the other one
    // ---- kept positions (hqt_set_keep_mask): where keep[b * n_steps + step] != 0 the draw is spent and discarded -- `out` already holds the kept code, which is
    //      left in place and is what the fused embedding looks up.  NULL: every position is drawn.
    const unsigned char* keep;   // [B, n_steps], device
    // ---- rolling pass (hqt_set_row_positions): row b draws position row_live(row_pos, b) in place of state->step -- the Philox position, the slice of `noise`, the
    //      indices into out / logits_out / the log-probabilities --, and an idle row (row_pos[b] < 0) spends its draw without writing any of them.  NULL: the step state.
    const int* row_pos;          // [B], device
};
// Uniform call: one launch.  With a row table in a FAST pass whose vocabulary the register-resident kernel takes: that kernel, then the general one, each over
// every row -- which rows are in which class is read on the device, so the launch sequence does not depend on the table's values.
hipError_t launch_sampler(const SamplerArgs& a, hipStream_t st);
// code_logprob_kernel, behind launch_sampler on the same stream with the same arguments: logprob[(b * n_steps + step) * draws + draw0 + slot] = log-softmax of the RAW row
// b * slots + slot of a.logits (before temperature, no cut-off; IEEE expf / logf in every precision) at feed[index of that draw in `out`] -- `feed` is the forced
// codes of the level, or a.out itself (the code just drawn).  One launch per slot, B workgroups; a row's value depends on its own bits and V only.
hipError_t launch_code_logprob(const SamplerArgs& a, const int64_t* feed, float* logprob, int slot, hipStream_t st);
// score_logprob_kernel (hqt_score): the value code_logprob_kernel defines, for ALL rows of a sub-step in one launch, one workgroup per (pair, slot): row
// r = i * slots + slot of logits [pairs * slots, V] at codes[r] -> logprob[i * draws + draw0 + slot]; every pointer is at the chunk's first pair
hipError_t launch_score_logprob(const float* logits, const int64_t* codes, float* logprob, int pairs, int V, int slots, int draw0, int draws, hipStream_t st);
// Draw report (hqt_set_draw_report): what the distribution behind a draw looked like, one entry per (b, step, draw) laid out as the log-probabilities are --
// e = (b * n_steps + step) * draws + draw0 + slot.  Over the same RAW row l, with the same m = max l and S = sum expf(l - m) as the log-probability (shared code):
//   entropy[e]              = logf(S) - T / S, T = sum expf(l_i - m) (l_i - m), reduced in the order of S            (nats; NULL: not written)
//   rank[e]                 = #{i : l_i > l_c} + #{i < c : l_i == l_c}, c the fed-forward code                        (0-based; NULL: not written)
//   top_codes[e * top_n + j]    = the j-th index by (l descending, index ascending), float compares: -0.0 ties with +0.0 and the lower index wins
//   top_logprobs[e * top_n + j] = (l[top_codes[j]] - m) - logf(S): the bits the log-probability has when that code is fed forward
struct ReportOut {
    float* entropy;
    int* rank;
    int top_n;                   // 0 .. 16 <= V
    int* top_codes;
    float* top_logprobs;
    bool any() const { return entropy || rank || top_n > 0; }
};
// draw_report_kernel, in code_logprob_kernel's place (same stream, same arguments, one launch per slot, B workgroups): writes the report entry of the draw and,
// logprob non-NULL, the log-probability too -- bit for bit what launch_code_logprob writes, so a call with both staged launches this one alone.
hipError_t launch_draw_report(const SamplerArgs& a, const int64_t* feed, float* logprob, const ReportOut& rep, int slot, hipStream_t st);
// score_report_kernel (hqt_score): the report of ALL rows of a sub-step's chunk in one launch, one workgroup per (pair, slot) as in launch_score_logprob; `rep`
// holds the call's base pointers and pair0 is the chunk's first pair: entry e = (pair0 + i) * draws + draw0 + slot.  logits / codes are at the chunk's first pair.
hipError_t launch_score_report(const float* logits, const int64_t* codes, const ReportOut& rep, int pair0, int pairs, int V, int slots, int draw0, int draws, hipStream_t st);
// guide_logits_kernel, IN FRONT of launch_sampler on the same stream: for every pair of `pairs` [n_pairs] (device) and every slot < slots, the rows
// pos_row * slots + slot and neg_row * slots + slot of logits [B * slots, V] are both overwritten with g = l_pos + (scale[level] - 1) (l_pos - l_neg), each
// operation rounded to fp32 on its own (no FMA) in every precision.  One launch per sub-step, n_pairs x slots workgroups; rows outside every pair are not touched.
hipError_t launch_guide_logits(float* logits, const GuidePair* pairs, int n_pairs, int V, int slots, int level, hipStream_t st);
// depth sub-step 2 of the three-level model (hqtransformer.py:537-551): token i (raster (H1 H2 W1 W2)) =
// tok1[codes1[b, step, parent(i)]] + pos[i] (+ tok0[codes0[b, step]]: 'add', tok0 non-NULL), 16 rows per sample; tok1_ld = 4 D:
// the 'reduce' table, child (H2 W2) takes its D-slice of the parent's row
hipError_t launch_depth_embed_l2(const int64_t* codes0, const int64_t* codes1, int n_steps, const StepState* state, const float* tok0,
                                 const float* tok1, const float* pos, float* x, int B, int D, bf16_t* xpk, int pk_mb, float* parts,
                                 hipStream_t st, int V = 0, int tok1_ld = 0, const int* row_pos = nullptr);
// hqt_score: launch_depth_embed_l2 over a chunk of pairs -- rows [16 i, 16 i + 16) from codes0[pair0 + i] and codes1[(pair0 + i) * 4 ..]
hipError_t launch_score_depth_embed_l2(const int64_t* codes0, const int64_t* codes1, int pair0, int pairs, const float* tok0, const float* tok1, const float* pos,
                                       float* x, int D, bf16_t* xpk, int pk_mb, float* parts, hipStream_t st, int V = 0, int tok1_ld = 0);
// 'top2mid2bot' head (hqtransformer.py:700-735): input of causal sub-step cnt >= 1 = tok[codes[(b * n_steps + step) * stride + slot]] + pos_row
hipError_t launch_depth_embed_causal(const int64_t* codes, int stride, int slot, int n_steps, const StepState* state, const float* tok,
                                     const float* pos_row, float* x, int B, int D, bf16_t* xpk, int pk_mb, float* parts, hipStream_t st, int V, const int* row_pos = nullptr);
// raises the dynamic-LDS limit of the sampler for (V, top-p) outside any stream capture
hipError_t sampler_configure(int V, bool use_top_p);

hipError_t launch_advance_step(StepState* state, int d_tbase, hipStream_t st);
// rolling pass: row_pos[b] += 1 for every live row (>= 0) of the B; a row that reaches n_steps turns idle (-1)
hipError_t launch_advance_rows(int* row_pos, int B, int n_steps, hipStream_t st);
hipError_t launch_set_step(StepState* state, int step, int t_base, hipStream_t st);
// rows[b] = (seed, sample_offset + b) for b < B
hipError_t launch_set_rows(RowKey* rows, int B, uint64_t seed, int64_t sample_offset, hipStream_t st);

// int64 codes [B, n_steps(,4)] written by the sampler are final; this copies forced codes into the
// feed-back arrays when teacher forcing is on.
// ---- decoder
struct QuantArgs {
    const int64_t* code_t;       // grid [B, r/2, r/2] or seq [B, (r/2)^2]; NULL = zeros
    const int64_t* code_b;       // grid [B, r, r] or seq [B, (r/2)^2, 4]; NULL = zeros
    int seq_layout;              // 1: sampler layout (rearranges folded into the addressing)
    const float* emb_t;          // [n_embed, 4*E]
    const float* emb_b;          // [n_embed, E]
    void* quant;                 // NHWC [B, r, r, 2E]
    int B, r, E;
    int out_dtype;
    int n_embed;                 // codebook rows for the index clamp (0: unchecked)
};
hipError_t launch_quant_gather(const QuantArgs& a, hipStream_t st);
// Three-level additive pyramid (HQVAEGenerator.decode_code, generator.py:577-599): quant[b, Y, X, c] =
//   emb0[code_t[Y/4, X/4]][4 (4c + 2 (Y%2) + X%2) + 2 ((Y/2)%2) + (X/2)%2] + emb1[code_m[Y/2, X/2]][4c + 2 (Y%2) + X%2] + emb2[code_b[Y, X]][c]
// (two PixelShuffle(2) steps written out); NULL level = zeros; seq_layout = the sampler's [B, n], [B, n, 4], [B, n, 16].
struct QuantArgs3 {
    const int64_t *code_t, *code_m, *code_b;
    int seq_layout;
    const float *emb0, *emb1, *emb2;   // [n_embed, 16E], [n_embed, 4E], [n_embed, E]
    void* quant;                       // NHWC [B, r, r, E]
    int B, r, E;
    int out_dtype;
    int n_embed;
};
hipError_t launch_quant_gather3(const QuantArgs3& a, hipStream_t st);
// Two-level models whose top level is E wide (hqt_config.s1_resample: 'nearest', 'conv2'; generator.py:214-219,233-242,316-318).  Both
// halves of an output pixel are whole rows of a table:  quant[b, Y, X, 0:E] = top[(code_t[Y/2, X/2] * top_sub + sub) * E ...],
// quant[b, Y, X, E:2E] = emb_b[code_b[Y, X] * E ...].  'nearest': top = the codebook, top_sub = 1 (every pixel of the 2x2 block reads
// the same row).  'conv2': top = the folded table of launch_fold_upsample_t, top_sub = 4, sub = 2 (Y % 2) + X % 2.
// A NULL code_t reads top_null (upsample_t.bias: the reference runs upsample_t over a zero quant_t) or, top_null == NULL, zeros.
struct QuantRowsArgs {
    const int64_t* code_t;       // grid [B, r/2, r/2] or seq [B, (r/2)^2]; NULL = top_null
    const int64_t* code_b;       // grid [B, r, r] or seq [B, (r/2)^2, 4]; NULL = zeros
    int seq_layout;
    const float* top;            // [n_embed, top_sub, E]
    int top_sub;                 // 1 or 4
    const float* top_null;       // [E] or NULL
    const float* emb_b;          // [n_embed, E]
    void* quant;                 // NHWC [B, r, r, 2E]
    int B, r, E;                 // E % 4 == 0
    int out_dtype;
    int n_embed;
};
hipError_t launch_quant_gather_rows(const QuantRowsArgs& a, hipStream_t st);
// table[n][a][b][co] = bias[co] + sum_ci emb[n][ci] * w[ci][co][a][b]: ConvTranspose2d(E, E, 2, stride 2) (weight [in, out, kh, kw]) applied
// to codebook row n, i.e. the four output pixels a top code expands to.  One fp32 FMA chain per entry, ci ascending, starting from the bias.
hipError_t launch_fold_upsample_t(const float* emb, const float* w, const float* bias, float* table, int n_embed, int E, hipStream_t st);
// wt[(a * 2 + b) * E + co][ci] = w[ci][co][a][b], bias4[(a * 2 + b) * E + co] = bias[co]: the transposed conv as a Linear with N = 4 E, K = E
hipError_t launch_repack_upsample_t(const float* w, const float* bias, float* wt, float* bias4, int E, hipStream_t st);

// GroupNorm statistics over NHWC x: stats[b][g] = (mean, rstd)
hipError_t launch_gn_stats(const void* x, int dtype, float* stats, int B, int HW, int C, int groups, float eps,
                           hipStream_t st);

// in-place softmax over the last axis of fp32 [rows, n]
hipError_t launch_softmax_rows(void* x, int dtype, int rows, int n, hipStream_t st);

// FAST decoder: y = swish?(GroupNorm(x)) as its own bandwidth-bound pass (bf16 NHWC -> bf16 NHWC), so the
// convolution's operand loader stays a plain im2col gather.  stats: [B][groups][2] (mean, rstd).
hipError_t launch_gn_apply(const void* x, void* y, const float* stats, const float* gamma, const float* beta, int B, int HW,
                           int C, int groups, int swish, hipStream_t st);
// FAST decoder GroupNorm statistics: coalesced partial sums per (image, pixel chunk), then a finalize pass
hipError_t launch_gn_stats_fast(const void* x, float* stats, double* partial, int B, int HW, int C, int groups, float eps,
                                hipStream_t st, int dtype = DT_BF16);
size_t gn_stats_fast_partial_elems(int B, int HW, int C, int groups);
// statistics from the per-tile partials of a halo conv (fast_kernels.h: conv_halo_stats_ok)
hipError_t launch_gn_finalize_tiles(const float* partial, float* stats, int B, int tiles, int HW, int C, int groups, float eps, hipStream_t st);
// the same from the double partials a SPLIT conv leaves (split_kernels.h)
hipError_t launch_gn_finalize_tiles_d(const double* partial, float* stats, int B, int tiles, int HW, int C, int groups, float eps, hipStream_t st);

// ---- HQ-VAE encode side (generator.py:298-310, 530-568; quantizer.py:91-133)
// fp32 NCHW image [B, 3, R, R] -> NHWC [B, R, R, cpad] (channels >= 3 are zero) in the activation dtype
hipError_t launch_image_to_nhwc(const float* img, void* out, int out_dtype, int B, int R, int cpad, hipStream_t st);
// out[m] = sum_k rows[m][k]^2 (fp32, fixed order)
hipError_t launch_row_sumsq(const void* rows, int dtype, float* out, int M, int K, hipStream_t st);

// One residual-quantisation level.  Everything is kept in the bottom layout (NHWC fp32 [B, r, r, E]): h = quant_conv_b(encoder(x)),
// recon = the pixel-shuffled sum of the coarser levels' quants (NULL at level 0).  Level rows: m = (b, y, x) at resolution
// r >> k, column cq in [0, E * 4^k) <-> k nested pixel-unshuffles (cq = (...(c * 4 + 2 i1 + j1) * 4 + 2 i2 + j2)...).
struct VqArgs {
    const float* h;
    float* recon;
    int B, r, E, k;
    // rows pass
    void* z;                 // [M, dim] residual rows in `z_dtype` (the distance GEMM's A operand)
    int z_dtype;
    float* zz;               // [M] |z|^2 of the stored (rounded) rows
    float* resid_nchw;       // optional [B, dim, rq, rq] fp32: the quantiser's input (reference `resids` / code[2])
    // finish pass
    const unsigned long long* best;
    const float* emb;        // [n_embed, dim] fp32
    int64_t* codes;          // [B, rq, rq]
    float* quant_nchw;       // optional [B, dim, rq, rq]: z + (e - z)  (the straight-through value, quantizer.py:131)
    float* err_rows;         // [M] sum_c (e - z)^2
};
hipError_t launch_vq_rows(const VqArgs& a, hipStream_t st);
hipError_t launch_vq_finish(const VqArgs& a, hipStream_t st);
// ---- top level of the 'nearest' / 'conv2' variants (E wide; hqt_config.s1_resample).  Top rows m = (b, y, x) at resolution r / 2.
// AvgPool2d(2) while gathering: rows[m][c] = ((h[2y, 2x] + h[2y, 2x+1]) + h[2y+1, 2x]) + h[2y+1, 2x+1]) * 0.25 (generator.py:215, 300)
hipError_t launch_vq_avgpool_rows(const float* h, float* rows, int B, int r, int E, hipStream_t st);
// finish pass over E-wide top rows z: codes, err_rows, quant_nchw as launch_vq_finish; the straight-through rows q = z + (e - z) go to
// q_rows [M, E] (may be NULL) and, recon != NULL, to the four bottom pixels of the block (nearest x2: generator.py:216-219, 302)
struct VqTopArgs {
    const float* z;          // [M, E] the quantiser's input rows (h_t)
    const unsigned long long* best;
    const float* emb;        // [n_embed, E]
    int B, r, E;             // r = bottom grid
    int64_t* codes;          // [B, r/2, r/2]
    float* quant_nchw;       // optional [B, E, r/2, r/2]
    float* q_rows;           // optional [M, E]
    float* recon;            // optional NHWC [B, r, r, E]: q replicated over the 2x2 block
    float* err_rows;         // [M]
};
hipError_t launch_vq_finish_top(const VqTopArgs& a, hipStream_t st);
// recon[b, 2y+a, 2x+b', co] = up[m][(a * 2 + b') * E + co]: the 2x2 scatter of the transposed conv's GEMM output ([M, 4E], launch_repack_upsample_t order)
hipError_t launch_vq_scatter_up(const float* up, float* recon, int B, int r, int E, hipStream_t st);
// diff[0] = scale * sum(err_rows[0..M)) in a fixed order (one workgroup)
hipError_t launch_vq_diff(const float* err_rows, int M, float scale, float* diff, hipStream_t st);
// fp32 NHWC [B, r, r, E] -> fp32 NCHW
hipError_t launch_nhwc_to_nchw_f32(const float* in, float* out, int B, int hw, int C, hipStream_t st);

