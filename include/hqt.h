/*
 * hqt.h -- C ABI of libhqt.so, the MI355X (gfx950) HQ-Transformer sampling engine.
 *
 * The reference (kakaobrain/hqtransformer) has no FFI/plugin layer: its sampling path is ordinary
 * nn.Module methods.  The boundary is therefore the Python call surface its drivers use (SURVEY.md
 * §8b); hqtransformer_amd/ re-exposes that surface and binds the entry points below with ctypes.
 * Each entry point names the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every tensor pointer is a DEVICE
 * pointer owned by the caller unless stated otherwise.  Calls enqueue work on `stream` (a
 * hipStream_t passed as void*; NULL = the null stream) and return without synchronising.  Every
 * function returns 0 on success or a negative hqt_status; the message is available from
 * hqt_last_error() (thread-local).  Nothing throws across the ABI.  A handle is bound to one device
 * and must be driven by one host thread at a time.
 */
#ifndef HQT_H
#define HQT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HQT_ABI_VERSION 9

typedef enum {
    HQT_OK = 0,
    HQT_ERR_INVALID = -1,      /* bad argument / unsupported configuration   */
    HQT_ERR_HIP = -2,          /* a HIP runtime call failed                  */
    HQT_ERR_STATE = -3,        /* call order (e.g. sample before finalize)   */
    HQT_ERR_UNKNOWN_WEIGHT = -4,
    HQT_ERR_SHAPE = -5,
    HQT_ERR_MISSING_WEIGHT = -6,
    HQT_ERR_RANGE = -7         /* SPLIT precision: an activation left the fp16 range (hqt_range_check) */
} hqt_status;

/* conditioning of the top GPT -- hqvae/models/stage2/hierarchical_ar.py:64-78 */
enum { HQT_COND_NONE = 0, HQT_COND_CLASS = 1, HQT_COND_TEXT = 2 };
/* input embedding -- hierarchical_ar.py:83-113 ('transformer1' has zero embedding blocks) */
enum { HQT_EMB_TRANSFORMER1 = 0, HQT_EMB_REDUCE = 1 };
/* arithmetic of a call.  EXACT = fp32 weights/activations/accumulation (what the reference computes
 * on its CPU path, where autocast is off); FAST = bf16 weights and MFMA, fp32 accumulation, fp32
 * softmax/normalisation/sampler (the counterpart of the reference's use_fp16=True autocast path).
 * SPLIT (stage-1 entry points: decode / encode) = fp32 tensors, fp32 GroupNorm / softmax / activations, and the
 * convolutions on the matrix cores with every fp32 operand carried as two fp16 values (hi, lo * 2^11): three
 * v_mfma_f32_16x16x32_f16 per product term, fp32 accumulation -- fp32-accurate (2^-22 per operand), what the reference's
 * fp32 decode (measure_throughput/__main__.py:108-113, outside autocast) computes up to summation order, at matrix-core
 * speed; layers whose shapes the split kernels do not take run the EXACT kernels.
 * SPLIT on the stage-2 entry points (hqt_sample / hqt_sample_l3, round 4): the EXACT launch sequence -- fp32 activations, LayerNorm,
 * attention, softmax and sampler exactly as EXACT -- with every nn.Linear (stage2/layers.py:73-85,190,313-315; the heads) on the matrix
 * cores: the fp32 activation rows are split into fp16 hi / lo while their tile is staged, the weights travel as fp16 hi / lo planes,
 * three v_mfma_f32_32x32x16_f16 per product term.  Code sequences are bit-identical to EXACT (and to the reference's CPU path) wherever
 * the draw is well-conditioned, logits within 2e-4; hqt_range_check applies as for stage 1. */
enum { HQT_PRECISION_EXACT = 0, HQT_PRECISION_FAST = 1, HQT_PRECISION_SPLIT = 2 };
enum { HQT_DTYPE_F32 = 0 };

typedef struct hqt_handle hqt_handle;

/* Model description.  Stage-2 fields restate the arguments of iHQGPT.__init__
 * (hierarchical_ar.py:24-33) as ImageGPT2 passes them (hqvae/models/__init__.py:123-137); stage-1
 * fields restate SimRQGAN2Generator / Decoder (hqvae/models/stage1/generator.py:179-259,
 * hqvae/models/stage1/modules/layers.py:300-383).  Set has_stage2 / has_stage1 to 0 to build half. */
typedef struct {
    int32_t abi_version;            /* HQT_ABI_VERSION */
    /* stage 2: 'hq-transformer/parallel', ratio_bot2top = 4 */
    int32_t has_stage2;
    int32_t embed_dim, n_layers, n_heads, n_layers_depth;
    int32_t vocab_top, vocab_bot, vocab_txt;
    int32_t ctx_len_img, ctx_len_txt, n_classes;
    int32_t cond_type;              /* HQT_COND_*  */
    int32_t embedding_type;         /* HQT_EMB_*   */
    int32_t gelu_approx;            /* hparams.gelu_use_approx */
    /* stage 1: 'simrqgan2', decoding_type = concat, upsample = pixelshuffle(2) unless s1_resample (last field) says otherwise */
    int32_t has_stage1;
    int32_t s1_ch, s1_n_mult, s1_ch_mult[8];
    int32_t s1_num_res_blocks;
    int32_t s1_n_attn_res, s1_attn_res[4];
    int32_t s1_resolution, s1_z_channels, s1_embed_dim, s1_n_embed, s1_out_ch;
    int32_t s1_use_init_downsample, s1_use_mid_block, s1_use_attn;
    /* sizing */
    int32_t max_batch;              /* largest B of any later call; workspaces are sized once */
    int32_t max_steps;              /* largest number of top positions per call (<= ctx_len_img) */
    /* three code levels: stage 2 = HQTransformer 'multilevel-hq' / 'parallel-add'
     * (hqvae/models/stage2/hqtransformer.py:24-205, one vocabulary size for all levels = vocab_top), stage 1 =
     * HQVAEGenerator with code_levels = 3 (generator.py:451-515).  0 or 2: the two-level models above. */
    int32_t code_levels;
    /* three levels only: HQTransformer.decoding_type (hqtransformer.py:105-157: tables of the depth head; :526-551: what the
     * depth sub-steps are fed).  0 'parallel-add' (the released level-3 config), 1 'parallel' (level-2 tokens without the top
     * code's embedding), 2 'parallel-reduce' (tok_emb_depth_levels.{0,1} are [V, 4 D]: child position c of a code takes slice c).
     * 3 'top2mid2bot': a causal head of 21 sequential one-token sub-steps (hqtransformer.py:700-800; pos_emb_depths.0 is [21, D],
     * the sub-step inputs come from tok_emb_levels).  The other values of the reference ('tree', 'old-parallel',
     * 'parallel-add-reduce') cannot sample three levels there either.
     * Two levels: 0 = iHQGPT 'parallel' (the released checkpoints), or 4 'bidirectional' (stage2.type hq-transformer/bidirectional4,
     * hierarchical_ar.py:791-878, since ABI version 8): one unmasked pass of the depth blocks over [ln_f(h) + sos_depth,
     * pos_emb_depth[0..3]] per position, all five codes drawn from it.  As in the reference, all five draws use
     * temperature_top, top_k_bot and top_p_bot.  Not with text conditioning. */
    int32_t depth_decoding;
    /* Which derived layouts of the AR loop's nn.Linear weights hqt_finalize_weights builds (bit mask of HQT_LAYOUT_*; 0 = all of them,
     * what ABI <= 6 always did: 9.6 GiB measured for the 2.1 GB ImageNet-12L model and its batch-64 workspace).  The fp32 tensors as received are always kept: they are
     * what EXACT computes from.  A replica that only ever samples in FAST precision passes HQT_LAYOUT_FAST (5.95 GiB measured); a hqt_sample /
     * hqt_sample_l3 call in a precision whose layout the handle was built without fails with HQT_ERR_STATE (EXACT without
     * HQT_LAYOUT_EXACT still runs, on the row-major fp32 weights: same results, slower below 257 rows).  Stage 1 is not affected. */
    int32_t ar_layouts;
    /* Two-level stage 1 only (since ABI version 9): the down_t / upsample_t pair between the top and the bottom grid
     * (hparams_aux.upsample, kernel size 2; generator.py:193-242).  0 is what every earlier version built.
     *   HQT_RESAMPLE_PIXELSHUFFLE 0  PixelUnshuffle(2) / PixelShuffle(2); stage1.quantize_t.embedding is [n_embed, 4 E].
     *   HQT_RESAMPLE_NEAREST      1  AvgPool2d(2) / nearest x2 ('nearest', 'nearest2'); stage1.quantize_t.embedding is [n_embed, E];
     *                                a NULL code_t contributes zero.
     *   HQT_RESAMPLE_CONV2        2  Conv2d(E, E, 2, stride 2) / ConvTranspose2d(E, E, 2, stride 2), both with bias ('conv2');
     *                                stage1.quantize_t.embedding is [n_embed, E].  Further tensors: stage1.upsample_t.weight
     *                                [E in, E out, 2, 2] and stage1.upsample_t.bias [E], needed by decode and encode (without them
     *                                hqt_finalize_weights fails with HQT_ERR_MISSING_WEIGHT); stage1.down_t.weight [E, E, 2, 2] and
     *                                stage1.down_t.bias [E], encode side only and optional like the encoder tensors (without them
     *                                hqt_encode fails with HQT_ERR_STATE).  A NULL code_t is a ZERO quant_t that still passes
     *                                through upsample_t (generator.py:339-342, 316): it contributes upsample_t.bias, not zero.
     * With 1 and 2 both levels of hqt_encode are E wide: quant[0] / resid[0] are [B, E, r/2, r/2], resid[0] = h_t = down_t(h_b),
     * and recon = quant_b + upsample_t(quant_t).  Three code levels take 0 only. */
    int32_t s1_resample;
} hqt_config;
#define HQT_RESAMPLE_PIXELSHUFFLE 0
#define HQT_RESAMPLE_NEAREST 1
#define HQT_RESAMPLE_CONV2 2
#define HQT_LAYOUT_FAST 1   /* bf16 MFMA-fragment packing (+ the LayerNorm-folded copies, the persistent chain's per-CU stream) */
#define HQT_LAYOUT_EXACT 2  /* fragment-ordered fp32 copy (v_mfma_f32_16x16x4_f32 kernel of passes up to 256 rows) */
#define HQT_LAYOUT_SPLIT 4  /* fp16 hi / lo planes (SPLIT precision on the stage-2 entry points) */
#define HQT_LAYOUT_ALL 7
#define HQT_DEPTH_PARALLEL_ADD 0
#define HQT_DEPTH_PARALLEL 1
#define HQT_DEPTH_PARALLEL_REDUCE 2
#define HQT_DEPTH_TOP2MID2BOT 3
#define HQT_DEPTH_BIDIRECTIONAL 4

/* Sampling options = the keyword arguments of sampling_ihqgpt (hqvae/utils/sampling.py:164-177).
 * top_k <= 0 means None (no cut-off), top_p <= 0 means None. */
typedef struct {
    int32_t precision;              /* HQT_PRECISION_*  (use_fp16=True -> FAST) */
    int32_t n_steps;                /* max_seq_len: top positions to generate */
    int32_t top_k_top, top_k_bot;
    float top_p_top, top_p_bot;
    float temperature_top, temperature_bot;       /* softmax_temperature[0], [1] */
    uint64_t seed;                  /* Philox seed, used when noise == NULL */
    int64_t sample_offset;          /* global index of row 0 (sharded batches draw the noise of the
                                       global batch: Philox counters are keyed by global row) */
    int32_t use_graph;              /* 1: replay the per-position launch sequence from a hipGraph */
    /* Merged steps: several independent sampling_ihqgpt calls (each with its own seed and global offset) executed as ONE
     * batch, so that the weights are streamed once for all of them.  Optional HOST arrays of B entries: row b then draws
     * exactly what row (b - first row of its call) of a separate hqt_sample call with (row_seeds[b], sample_offset =
     * row_offsets[b] - that row index) would draw -- Philox counters are keyed by (seed, global row), nothing else.
     * NULL: every row uses `seed` and `sample_offset + b`. */
    const uint64_t* row_seeds;
    const int64_t* row_offsets;
} hqt_sample_opts;

/* hqt_create -- replaces ImageGPT2(config) construction (hqvae/models/__init__.py:92-174) for the
 * tensors of the sampling path; allocates all device workspaces (KV cache, activations). */
int hqt_create(const hqt_config* cfg, int device, hqt_handle** out);

/* hqt_set_weight -- replaces load_state_dict (sampling_hqmodel.py:77-79): `name` is the reference
 * state-dict key without the 'stage1.' / 'stage2.' prefix namespace collision ('stage2.' keys are
 * passed as e.g. "stage2.blocks.0.attn.key.weight", stage-1 keys as "stage1.decoder.conv_in.weight").
 * `data` may be a host or a device pointer to contiguous fp32 in the reference's own layout
 * ([out,in] Linear, [O,I,kh,kw] Conv2d, [n_embed,dim] codebooks); it is copied before return. */
int hqt_set_weight(hqt_handle* h, const char* name, const void* data, int dtype, const int64_t* shape, int ndim);

/* hqt_finalize_weights -- checks every tensor arrived, builds the device layouts the kernels read
 * (fused QKV, tap-major conv filters, bf16 MFMA-fragment packing for FAST). */
int hqt_finalize_weights(hqt_handle* h);

/* hqt_clone -- a further LANE over the weights of a finalized handle.  The reference's throughput harness
 * (measure_throughput/__main__.py:84-116) runs one batch at a time; its 64-row AR loop is a chain of small
 * latency-bound kernels that leaves most of an MI355X idle, so the harness here keeps several batches in flight,
 * one lane and one HIP stream each (independent chains interleave on the GPU).  The clone shares every weight
 * buffer of `src` and owns only its workspace (KV cache, activations, step state, graph cache); results of a lane
 * are bit-identical to the parent's.  The lane starts with the root's hqt_set_switch values as they are at this call (and with the LATENCY
 * policy); later changes on either side stay there.  Destroy clones before their parent (hqt_destroy(parent) fails otherwise). */
int hqt_clone(hqt_handle* src, hqt_handle** out);

/* hqt_set_policy -- kernel selection for the AR loop.  LATENCY (default): tile shapes that finish one batch soonest
 * (every GEMM spread over as many CUs as possible).  THROUGHPUT: shapes that cost the fewest CU-microseconds (64-row
 * weight tiles: half the activation re-reads per weight byte), for several lanes in flight (hqt_clone), where kernels
 * of different batches share the chip: ~7 % more images/s with 3 lanes, ~15 % slower alone.  Results are unchanged up
 * to fp32 summation order in FAST arithmetic (EXACT arithmetic does not use these kernels). */
enum { HQT_POLICY_LATENCY = 0, HQT_POLICY_THROUGHPUT = 1 };
int hqt_set_policy(hqt_handle* h, int policy);

/* hqt_set_switch -- two choices of launch sequence that do not change what is computed beyond fp32 summation order (no reference
 * counterpart; A/B runs and tests).  Both are part of the graph key: the next hqt_sample re-captures if one changed.
 * SCOPE: the handle it is called on, and no other.  A lane copies its root's values when hqt_clone makes it; a later hqt_set_switch on the root
 * does not reach the lanes that exist, nor one on a lane its root or its siblings: call it on every handle that is to change.  (The environment
 * variables named below only set the values a ROOT handle starts with.)
 *   HQT_SWITCH_PERSIST     1 (default): FAST hqt_sample of up to 64 rows on a root handle runs a top position as ONE persistent launch
 *                          (csrc/persist.h); 0: the launch chain.  The default is 0 when HQT_PERSIST=0 was in the environment at hqt_create
 *                          -- the environment is read there, once, never per call.  A handle whose persistent launch gave up
 *                          (hqt_range_check) switches itself to 0; setting 1 re-arms it.
 *   HQT_SWITCH_SINGLE_KEY  1 (default): depth sub-step 0 (one query over one key) skips the query third of the fused GEMM and the
 *                          attention launch, bit-identically; 0: the long way round (default 0 when HQT_NO_SINGLE_KEY was set at hqt_create). */
/*   HQT_SWITCH_SPLIT_KSLICES  1 (default): SPLIT-precision hqt_sample cuts K of the narrow GEMMs (proj / fc2) of passes up to 1024 rows into slices summed in index order
 *                          (deterministic; the fp32 summation order, hence the last bits of a logit, then depends on the row count of the pass); 0: one order at every
 *                          row count (default 0 when HQT_SPLIT_KSLICES_OFF was set at hqt_create).
 *   HQT_SWITCH_PERSIST_FAULT  test hook (0 = none, the default): on = c + 1 makes compute unit c withhold its first grid-barrier signal in every
 *                          later persistent launch, so the launch gives up after its time limit (tests/test_gpu_persist.py).  A device word, not
 *                          part of the graph key: a cached graph replays it.  Synchronises the device. */
enum { HQT_SWITCH_PERSIST = 0, HQT_SWITCH_SINGLE_KEY = 1, HQT_SWITCH_PERSIST_FAULT = 2, HQT_SWITCH_SPLIT_KSLICES = 3 };
int hqt_set_switch(hqt_handle* h, int which, int on);

/* hqt_set_row_samplers -- no reference counterpart as a call: the reference filters and draws every row on its own (hqvae/utils/sampling.py:12-37 cut each
 * row of the logits separately; hierarchical_ar.py:762-785, 866-873 apply one temperature / top-k / top-p triple per code level to the whole batch), so rows of
 * ONE pass may carry the settings of different calls without changing what any of them draws.  Merged steps (row_seeds / row_offsets above) need exactly that
 * when their calls differ in sampler settings.  `rows` is a HOST array of n entries, index = code level (a two-level model ignores index 2), copied before
 * return; n = 0 or rows = NULL clears.  The table is STAGED on the handle (a lane from hqt_clone has its own): the next hqt_sample / hqt_sample_l3 on that
 * handle takes it and clears it, whether that call succeeds or not.  That call then fails with HQT_ERR_INVALID unless n equals its B, every temperature it
 * uses is > 0 and no row asks for top-p on a vocabulary above 8192; row b draws with rows[b] in place of the scalars of `opts` (which are ignored), through
 * the same arithmetic as in a call whose scalars are rows[b]: bit-identical codes.  top_k <= 0 / top_p <= 0 mean None, as in hqt_sample_opts.  The
 * bidirectional head keeps the reference's mapping per row: all five draws use temperature[0], top_k[1], top_p[1].  The values live in device memory, not in
 * the captured graph: calls that differ only in the table replay one graph. */
typedef struct { float temperature[3]; int32_t top_k[3]; float top_p[3]; } hqt_row_sampler;   /* 36 bytes */
int hqt_set_row_samplers(hqt_handle* h, int n, const hqt_row_sampler* rows);

/* hqt_set_logprob_out -- no reference counterpart: the reference draws from its logits and keeps no probability (hierarchical_ar.py:762-785).  `logprobs` is a
 * DEVICE pointer, fp32 [B, n_steps, draws] (draws = 5, or 21 with three code levels; draw order as in `noise`), STAGED on the handle (a lane from hqt_clone has its
 * own): the next hqt_sample / hqt_sample_l3 / hqt_sample_prefix / hqt_sample_prefix_l3 on that handle takes it and clears it, whether that call succeeds or
 * not; NULL clears; a NULL handle is HQT_ERR_INVALID.  The taking call writes, behind every draw,
 *   logprobs[(b * n_steps + step) * draws + draw] = l[code] - max(l) - log sum_i exp(l_i - max(l))
 * over the RAW logits row l of that draw: before temperature, without top-k / top-p -- the model's own log-probability at T = 1, finite whatever cut-off the
 * draw used; two passes in fp32 with IEEE expf / logf in every precision, a fixed reduction order per row (the same bits for the same logits at any B, eager
 * or replayed).  `code` is the code the call FEEDS FORWARD: where a level is forced (force_*, given_top_code) the forced code -- not the drawn one, which is
 * still written to out_* --, otherwise the code just drawn.  With a prefix the entries of positions < prefix_len are not written (as with logits_out).  The
 * pointer is part of the graph key; a call without it launches exactly what it launched before, a call with it one more kernel per draw (timing slot
 * "code_logprob").  Forcing every level to given codes makes the call a scorer of those codes, at the cost of its n_steps decode steps. */
int hqt_set_logprob_out(hqt_handle* h, float* logprobs);

/* hqt_set_draw_report -- no reference counterpart (LLM sampling APIs call the last two fields top_logprobs).  What the distribution behind every draw looked
 * like, in a few numbers per draw where `logits_out` writes the whole row: how flat it was, where the fed-forward code stood in it, which codes were the
 * alternatives.  All pointers are DEVICE pointers, each [B, n_steps, draws] as the hqt_set_logprob_out buffer (draws = 5, or 21 with three code levels; draw
 * order as in `noise`), the two top arrays with top_n entries per draw; a NULL entropy / rank is not written, top_n = 0 writes no top arrays.  STAGED on the
 * handle exactly like hqt_set_logprob_out (a lane from hqt_clone has its own): the next hqt_sample / hqt_sample_l3 / hqt_sample_prefix / hqt_sample_prefix_l3
 * or hqt_score on that handle takes it and clears it, whether that call succeeds or not; r = NULL, or a struct with nothing to write (all pointers NULL,
 * top_n = 0), clears.  HQT_ERR_INVALID, naming the field: a NULL handle, top_n outside [0, HQT_REPORT_MAX_TOP], top_n > 0 with top_codes or top_logprobs
 * NULL, top_n = 0 with either of them set; the taking call fails with HQT_ERR_INVALID when its vocabulary is smaller than top_n.
 * Over the RAW fp32 logits row l of the draw (with a guidance pair the guided row, equal in both rows), at T = 1 without cut-off whatever settings drew the
 * code, with m = max l and S = sum_i expf(l_i - m) -- the m and S of the log-probability, from the same code in the same reduction order -- and c the code the
 * call feeds forward (forced where a level is forced, clamped into the vocabulary):
 *   top_codes[j]    the j-th index when indices are sorted by (l descending, index ascending); float compares, so -0.0 ties with +0.0 and the lower index wins
 *   top_logprobs[j] (l[top_codes[j]] - m) - logf(S): bit for bit the hqt_set_logprob_out entry of a call that feeds top_codes[j] forward
 *   rank            #{i : l_i > l_c} + #{i < c : l_i == l_c}, 0-based; rank < top_n implies top_codes[rank] == c
 *   entropy         logf(S) - T / S in nats, T = sum_i expf(l_i - m) (l_i - m) reduced in the order of S (per thread a pairwise tree, the wave's xor
 *                   butterfly, four wave sums as (w0 + w1) + (w2 + w3)); IEEE expf / logf and an IEEE division in every precision
 * Every value depends on the row's bits and on V alone, never on B, the batch row, or eager versus replayed.  Entries are written exactly where a staged
 * log-probability buffer is written and nowhere else: behind every draw, at kept positions and forced levels as there, not for positions < prefix_len, not for
 * an idle row of a rolling pass.  One launch per draw in code_logprob's place (timing slot "draw_report"); with a log-probability buffer staged as well that
 * one kernel writes both (no "code_logprob" launch; the log-probabilities keep their bits).  The pointers and top_n are part of the graph key; a call with
 * nothing staged launches exactly what it launched before.  hqt_score writes the report of the GIVEN codes for all (pair, slot) rows of a depth chunk in one
 * launch next to its log-probabilities.  Finite logits are assumed. */
#define HQT_REPORT_MAX_TOP 16
typedef struct {
    float*   entropy;       /* device, fp32  [B, n_steps, draws]         or NULL */
    int32_t* rank;          /* device, int32 [B, n_steps, draws]         or NULL */
    int32_t  top_n;         /* 0 .. HQT_REPORT_MAX_TOP                            */
    int32_t* top_codes;     /* device, int32 [B, n_steps, draws, top_n]  (top_n > 0) */
    float*   top_logprobs;  /* device, fp32  [B, n_steps, draws, top_n]  (top_n > 0) */
} hqt_draw_report;          /* 40 bytes */
int hqt_set_draw_report(hqt_handle* h, const hqt_draw_report* r);

/* hqt_set_guidance -- no reference counterpart: the reference trains without condition dropout and draws every image under one condition.  Guided sampling
 * runs an image under TWO conditions, as two rows of one pass (both count against max_batch), and draws every code of both rows from
 *   g = l_pos + (scale - 1) * (l_pos - l_neg)
 * -- scale 1: the positive row's own logits; scale > 1: away from the negative condition (for text models typically the all-[PAD] caption, for class models a
 * class the caller names).  `pairs` is a HOST array of n_pairs entries, copied; 0 / NULL clears; a NULL handle or n_pairs outside [0, max_batch / 2] is
 * HQT_ERR_INVALID.  The table is STAGED on the handle (a lane from hqt_clone has its own): the next hqt_sample / hqt_sample_l3 / hqt_sample_prefix /
 * hqt_sample_prefix_l3 on that handle takes it and clears it, whether that call succeeds or not.  That call, between the head GEMM and the sampler of every
 * sub-step, overwrites the logits rows of pos_row AND neg_row with g, scale[level] being the scale of the code level drawn (one kernel per sub-step, timing
 * slot "guide_logits"): three fp32 operations, each rounded on its own in every precision -- d = l_pos - l_neg, m = (scale - 1) * d, g = l_pos + m (scale - 1
 * itself rounded to fp32) --, so fp32 arithmetic on the host reproduces the row bit for bit.  The negative row's Philox key is made the positive row's
 * (whether keys come from seed / sample_offset or from row_seeds / row_offsets), so both rows draw the same code and feed the same code forward; rows outside
 * every pair are untouched and draw what they draw without a table.  What the order implies: `logits_out` holds the GUIDED row, in both rows of a pair; a staged
 * hqt_set_logprob_out buffer scores the fed-forward code under the guided row, equally in both rows.  Per-row inputs that the engine cannot compare -- `noise`,
 * `force_*`, prefix codes: device pointers -- must hold the same values for both rows of a pair; the caller sees to that.  Only that a table is staged and its pair
 * count enter the graph key: a changed table of the same size replays the same graph.  The taking call fails with HQT_ERR_INVALID (and a message naming the
 * pair) when a row is outside [0, B), pos_row == neg_row, a row appears in more than one pair, a scale of a level the model has is not finite, the handle's
 * cond_type is HQT_COND_NONE, a staged hqt_set_row_samplers table gives the two rows different settings, or row_seeds / row_offsets give them different keys
 * (implicit keys are overridden; explicit ones are never silently changed).  Without a staged table a call launches exactly what it launched before. */
typedef struct { int32_t pos_row, neg_row; float scale[3]; } hqt_guide_pair;   /* 20 bytes */
int hqt_set_guidance(hqt_handle* h, int n_pairs, const hqt_guide_pair* pairs);

/* hqt_set_keep_mask -- no reference counterpart: the reference can hold codes fixed only by teacher-forcing a level at every position (given_top_code).  A keep
 * table fixes any set of (row, position) cells of the code grid and lets the call draw the rest around them: rows of one pass with prefixes of different lengths
 * (or none), the left columns of an image, everything outside a box, the cells of a sliding window that earlier windows filled.  `keep` is a HOST array
 * [B, n_steps] of 0 / 1, copied before return; `codes` holds one DEVICE pointer per code level, coarse to fine, in the sampler's layout (int64 [B, n_steps],
 * [B, n_steps, 4][, [B, n_steps, 16]]), read by the taking call and only where keep is 1; values outside the vocabulary are clamped into it on the device, as every
 * id that arrives from the caller.  The table is STAGED on the handle (a lane from hqt_clone has its own): the next hqt_sample / hqt_sample_l3 on that handle takes it
 * and clears it, whether that call succeeds or not; B == 0 or a NULL keep clears; a NULL handle is HQT_ERR_INVALID.
 * The taking call first scatters the kept codes into the handle's code buffers (one launch per level, outside any captured graph), where every level's embeddings read
 * them; the sampler kernels then leave those entries alone.  At a kept (b, t) EVERY level of the position is the kept code: it is what out_* holds and what is fed
 * forward.  Every other position draws exactly what it draws in a plain call whose earlier positions had produced the same codes: Philox keys by (seed, global row,
 * ABSOLUTE position, draw, chunk), the same slice of `noise`, the same sampler settings and row tables.  A kept position still spends its draw; the result is
 * discarded.  `logits_out` and a staged hqt_set_logprob_out buffer are written at kept positions as at any other, the log-probability being that of the code fed
 * forward, i.e. the kept one: a fully kept row scores itself.
 * Leading run: with L = the smallest count of leading ones over the rows, clipped to min(max_prefix of the handle, n_steps - 1) -- and 0 where the prefix prefill is
 * not built (text conditioning with three code levels) --, positions < L go through the one-pass prefix prefill exactly as hqt_sample_prefix with prefix_len = L runs
 * them, and like there their rows of logits_out / the log-probabilities are not written.  All later kept positions are ordinary decode steps.  Only "a table is
 * staged" and L enter the graph key; the mask lives in device memory: a changed table with the same L replays the same graph.  Every depth head and every precision.
 * The taking call fails with HQT_ERR_INVALID (and a message naming the cause) when B or n_steps differ from the table's, a level pointer is NULL, force_* is given
 * (refused by name: the caller puts forced codes into the kept codes), the call is a prefix entry point (the leading run IS the prefix), or the two rows of a
 * hqt_set_guidance pair keep different positions.  Not built: keeping some levels of a position and not others.  A rolling call (hqt_set_row_positions) takes the
 * table only on a handle that has opted in with hqt_set_join_run, and reads it per row, by the rules given there; without the opt-in it is refused.  Without a
 * staged table a call launches exactly what it launched before. */
int hqt_set_keep_mask(hqt_handle* h, int B, int n_steps, const uint8_t* keep, const int64_t* const* codes);

/* hqt_set_prompt_groups -- no reference counterpart: the reference prefills the text prompt of every row (sampling.py:187-190), also where the rows are candidates of
 * one caption or the negative rows of a guided batch.  The prompt rows of a sample depend on nothing but the prompt, so the taking call prefills every DISTINCT prompt
 * once and hands the result to the rows that carry it.  `group_of_row` is a HOST array of B entries in [0, n_groups), copied before return; the mapping is arbitrary
 * (unsorted, groups of any size).  The table is STAGED on the handle (a lane from hqt_clone has its own, and its own staging buffer): the next hqt_sample /
 * hqt_sample_l3 on that handle takes it and clears it, whether that call succeeds or not.  In that call `cond` is [n_groups, ctx_len_txt] (prompt g in row g) and
 * row b of the pass carries prompt group_of_row[b]: the prompt embedding and the body blocks run causally over n_groups * ctx_len_txt rows, their K/V going to a
 * staging buffer of [n_layers][n_groups][ctx_len_txt][D]; one launch (timing slot "prompt_fanout") copies the K/V of every row's prompt into its cache slot and
 * gathers the last prompt row of the residual stream per row; the depth head then runs on the B rows and draws position 0.  The decode steps, the captured graph and
 * its key are those of a call without a table: they see the cache an unshared prefill leaves.  In HQT_PRECISION_EXACT the call returns bit for bit what the same call
 * returns with the prompts expanded to [B, ctx_len_txt]; in the other precisions the prefill of fewer rows may be served by other GEMM kernels.
 * Memory: the staging buffer (2 * n_layers * n_groups * ctx_len_txt * D * 4 bytes, counted by hqt_workspace_bytes) and the gathered rows (max_batch * D * 4 bytes)
 * are allocated HERE -- grown when n_groups exceeds what an earlier table needed, never shrunk -- and nowhere else: a sampling call allocates nothing.
 * HQT_ERR_INVALID, with a message naming the cause: a NULL handle or table, a handle that is not text-conditional, B or n_groups outside [1, max_batch],
 * n_groups > B, an entry outside [0, n_groups); in the taking call: a B that differs from the table's, a prefix entry point, or a staged hqt_set_keep_mask table
 * whose rows share a leading run (prefix_len > 0: the prompt and the prefix are then one prefill whose prefix rows differ per row).  hqt_score clears a staged table
 * and fails with HQT_ERR_STATE.  Without a staged table a call launches exactly what it launched before. */
int hqt_set_prompt_groups(hqt_handle* h, int B, int n_groups, const int32_t* group_of_row);

/* hqt_set_segment -- the engine side of the reference's per-position loop (sampling_ihqgpt calls stage2.sampling_step once per position, hqvae/utils/sampling.py:
 * 194-235, and its caller may look at, or change, the codes between two of them): a pass that stops behind any position and goes on later, bit for bit.  The
 * segment is STAGED on the handle (a lane from hqt_clone has its own): the next hqt_sample / hqt_sample_l3 on that handle takes it and clears it, whether that
 * call succeeds or not; a NULL handle is HQT_ERR_INVALID.  The taking call runs positions [start, stop) of a pass that is opts->n_steps positions long.  Every
 * buffer keeps its full-length layout and absolute indexing -- out_*, force_*, noise, logits_out, a staged hqt_set_logprob_out buffer --; entries outside
 * [start, stop) are neither read nor written, except that the codes of position start - 1 are read.
 *   start == 0  the call launches what a plain call launches for those positions (text models: the prompt prefill too, and a staged hqt_set_prompt_groups table
 *               is allowed), stops behind position stop - 1 and leaves the step state there.  The handle records the PAUSED pass: B, n_steps, code levels,
 *               precision and position = stop.
 *   start > 0   needs a paused pass on this handle with the same B, n_steps, code levels and precision and with position == start; anything else is
 *               HQT_ERR_STATE, with a message naming what differs (the paused pass is kept).  The call sets the Philox keys and any staged table as every call
 *               does, does NOT reset the step state, runs no prefill, and runs stop - start decode steps, eager or from the graph (the graph key is what it was;
 *               the positions per graph launch are chosen from stop - start).  The codes of position start - 1 are read from this call's own out_* buffers (a
 *               forced level: from force_*): the caller passes buffers that hold them, and if it has edited them since they were drawn the pass goes on as if the
 *               edited codes had been drawn.
 *   stop == n_steps: the pass is finished and the record is cleared.
 * Row-sampler tables, guidance tables, the log-probability buffer, row_seeds / row_offsets and logits_out work in every segment as in a whole call, so settings
 * may change from one segment to the next: Philox keys are (seed, global row, ABSOLUTE position, draw, chunk), and between two positions a row's whole state is its
 * body K/V rows, the step state and the codes in the caller's buffers (the depth cache is rebuilt every position).
 * HQT_ERR_INVALID in the taking call, with a message naming the cause: stop <= start, start < 0 or stop > n_steps; a prefix entry point; a staged keep table;
 * a staged prompt-group table with start > 0.  The record of a paused pass is cleared by every other call that writes the body cache or the step state: a plain or
 * prefix sampling call, a segment with start == 0, hqt_score.  Without a staged segment a call launches exactly what it launched before.
 * Not built: segments together with keep tables or code prefixes.  Rows of one pass at different positions: hqt_set_row_positions, below.
 *
 * hqt_select_rows -- re-maps the rows of the paused pass: afterwards cache row j of every body layer holds what row rows_from[j] held, for the live rows
 * 0 .. t_base - 1 (text models: the prompt rows and the drawn positions), K and V, in the cache's type for the paused precision; the paused B becomes B_new.
 * `rows_from` is a HOST array of B_new entries in [0, paused B), 1 <= B_new <= max_batch, copied before return; any mapping: the identity, a permutation, a subset
 * (drop rows), duplicates (fork rows), B_new above the paused B.  The codes are the caller's tensors: the caller gathers them itself, and gives forked rows new
 * Philox keys (row_seeds / row_offsets) where they are to differ.  The step state does not change.  One launch (timing slot "kv_gather_rows"), in place through
 * LDS, on `stream`; allocates no device memory (the table travels through the pinned staging ring of the row tables).  HQT_ERR_STATE: no paused pass.  HQT_ERR_INVALID: a NULL argument, B_new outside [1, max_batch], an entry out of range,
 * B_new * 16 bytes beyond the 160 KiB of LDS of a compute unit (10240 rows). */
int hqt_set_segment(hqt_handle* h, int start, int stop);
int hqt_select_rows(hqt_handle* h, int B_new, const int32_t* rows_from, void* stream);

/* hqt_set_row_positions -- no reference counterpart: the reference starts all rows of a batch together.  A ROLLING pass is a fixed number of slots (the B rows of
 * a call) in which every row stands at its own position: a row that finishes frees its slot, a new request joins in a free slot at position 0 while its neighbours
 * are mid-image, so the weights streamed for a position serve a full pass.  `pos` is a HOST array of B entries, copied before return (it travels through the pinned
 * staging ring of the row tables): pos[b] is the position row b draws next, -1 an empty slot.  The table is STAGED on the handle (a lane from hqt_clone has its own):
 * the next hqt_sample / hqt_sample_l3 on that handle takes it and clears it, whether that call succeeds or not; B == 0 or a NULL pos clears.
 * The taking call, with n = opts->n_steps, runs k steps (1 <= k <= n).  In step j every row with pos[b] >= 0 and pos[b] + j < n draws position pos[b] + j exactly as
 * a plain call draws it given that row's earlier codes: Philox keys by (seed, global row, ABSOLUTE position, draw, chunk), the same slice of `noise`, the same sampler
 * settings and row tables; force_*, logits_out and a staged hqt_set_logprob_out buffer behave as in a plain call, all indexed by absolute position.  cond[b] is read
 * where a row stands at position 0; row_seeds / row_offsets give each slot its request's key.  The codes of position pos[b] - 1 are read from the caller's out_* (a
 * forced level: force_*), as a segment reads them.  Every depth head and every precision; a row's bits do not depend on where its neighbours stand.
 * Idle rows -- empty slots, and rows that have drawn position n - 1 in an earlier step of the call -- still occupy rows of the GEMMs: they compute on an input row of
 * zeros at position 0, inside their own (dead) cache slot, and nothing the caller can see of them is written (out_*, logits_out, the log-probabilities).
 * The handle records the ROLLING PASS: B, n, code levels, precision and per slot the next position; a slot whose row reached n becomes empty.  The taking call
 * checks every slot against the record and fails with HQT_ERR_STATE naming the row (the record is kept) unless pos[b] is -1 (vacate, or stay empty), 0 (join: always
 * allowed, the slot's old contents are dead) or exactly the recorded next position (continue); without a record every entry must be 0 or -1.  A B, n, level count or
 * precision that differs from the record's is HQT_ERR_STATE.  The record is cleared by every other call that writes the body cache (a plain, prefix or segment
 * sampling call, hqt_score), as the paused pass is; a rolling call clears a paused pass.  A pass whose slots are all empty is over (its record is dropped: the
 * next rolling call begins a pass, with any B, n and precision).  A first call of empty slots only is legal and draws nothing.
 * Rolling calls always take the launch chain (the persistent launch keeps one t_base for all its rows).  The positions live in device memory: only "rolling" and
 * the steps per graph launch enter the graph key, calls that differ only in positions replay one graph.  Without a staged table a call launches exactly what it
 * launched before.
 * HQT_ERR_INVALID, with a message naming the cause: a NULL handle; B outside [1, max_batch] or different from the taking call's; k outside [1, n]; an entry outside
 * [-1, n - 1]; a text-conditional handle that has not sized the prefill of its joining rows (hqt_set_max_joins, below), or more joining rows in one call than it
 * sized; a prefix entry point; a staged segment, keep table or prompt-group table; a hqt_set_guidance pair whose two rows stand at different positions or of which
 * exactly one is empty.
 * TEXT-CONDITIONAL handles (after hqt_set_max_joins(h, J > 0)) differ in these points, and in nothing else.  cond is [B, ctx_len_txt]; row b of it is read only
 * where pos[b] == 0.  Position 0 of a text row is not a decode step: the row's prompt prefill draws it.  A call whose table holds joining rows (pos[b] == 0) first
 * runs the JOIN PHASE -- the prompts of the joining rows through the body into a staging buffer, from there into their cache slots, and the depth head, which draws
 * position 0 under each joiner's own key, sampler row and noise slice (out_*[b, 0], logits_out, the log-probabilities and the draw report at position 0) -- and then
 * the k steps, in all of which a joining row takes part at positions 1 .. k: it advances by 1 + k (clipped at n), every other row by k.  The handle's record, what
 * the next call must present for the slot and the entries of every output that are written follow that rule.  With n == 1 a joining row is finished behind the
 * join phase and idles in the steps.  The two rows of a guidance pair stand at one position, so they join together.  The join phase runs in front of the
 * captured steps, as the prompt prefill of a plain call does, and allocates nothing.  In EXACT a request draws bit for bit what the plain call draws for it in its
 * slot; in FAST and SPLIT the prefill of J prompts may be served by other GEMM kernels than the prefill of B, so the plain call that equals a join is the one
 * that prefills the same J prompts (hqt_set_prompt_groups).
 * KEEP TABLES (after hqt_set_join_run(h, J > 0, R), below; without it a staged keep table is refused as it always was).  The table is [B, n] with one device pointer
 * per level, exactly as hqt_set_keep_mask stages it; row b of it is read only inside the positions row b passes in this call.  Before the steps, outside the
 * captured graph, the kept codes of row b go into out_* only at kept positions inside the span row b advances over in this call; empty slots and positions outside
 * the span are neither read nor written.  Every kept position that is not prefilled is an ordinary step of the row, as in a plain keep call: the draw is spent and
 * discarded, the kept code is what out_* holds and what is fed forward, and logits_out, the log-probabilities and the draw report are written for it.  JOIN RUN:
 * among the rows with pos[b] == 0 in the call, L = min(smallest leading run of ones of their mask rows, R, n - 1); L is 0 without a table and when no row joins.  The
 * join phase runs iff the handle is text-conditional or L > 0: the joiners' body input rows -- the prompt rows (text) or the sos / class row, then the L input rows of
 * positions 1 .. L, read from their kept codes -- go through the body over the joiners alone into the staging buffer, ONE launch hands every joiner its (ctx_len_txt
 * | 1) + L rows of K/V and its last row of x, and the depth head draws position L (which may itself be kept) under the join table.  The steps then find the joiners
 * at L + 1: a row that joins through a join phase advances by L + 1 + k (clipped at n), every other row by k (L = 0 on a text handle: the 1 + k above).  Rows of
 * positions < L of logits_out, the log-probabilities and the report are not written, as in hqt_sample_prefix.  Without a join phase (no text, L == 0) the call
 * launches what it launched before plus the scatter and the samplers' guard.  Only "rolling" and "a keep table is staged" enter the graph key -- never positions,
 * mask or L.  HQT_ERR_INVALID in the taking call: no opt-in; the table's B or n differ from the call's; a NULL level pointer; force_* with a table; more rows
 * joining through a join phase than max_joins; the two rows of a guidance pair keep different positions.
 * Not built: rolling together with segments, prefixes or prompt groups (a join prefills every joining row's prompt, equal or not); per-row join runs in one prefill
 * (the joiners of a call share L); a kept run prefilled on text handles with three code levels; a depth pass
 * over the joining rows alone (the join phase's depth head runs over all B rows); hqt_select_rows on a rolling pass (HQT_ERR_STATE: slots are reused in place);
 * a rolling form of the persistent launch. */
int hqt_set_row_positions(hqt_handle* h, int B, const int32_t* pos, int k);

/* hqt_set_max_joins -- opt-in sizing of rolling passes on a text-conditional handle: allocates (grows, never shrinks) what the prompt prefill of up to max_joins
 * joining rows per call needs -- the staging K/V of [n_layers][max_joins][ctx_len_txt][D] at 4 bytes per element and the gathered rows [max_batch][D] fp32.  These
 * are the buffers of hqt_set_prompt_groups, sized to the larger of the two needs and counted by hqt_workspace_bytes; a sampling call allocates nothing.  A lane from
 * hqt_clone of a handle with max_joins > 0 gets a staging of its own for as many.  max_joins == 0 switches rolling passes off again and frees nothing.  A text
 * handle that never called it refuses hqt_set_row_positions as it always has.
 * HQT_ERR_INVALID: a NULL handle, a handle that is not text-conditional, max_joins outside [0, max_batch].  HQT_ERR_STATE: the handle holds a rolling pass. */
int hqt_set_max_joins(hqt_handle* h, int max_joins);

/* hqt_set_join_run -- opt-in sizing of rolling calls that take a keep table (hqt_set_row_positions, KEEP TABLES): after hqt_set_join_run(h, J >= 1, R >= 0) such a
 * call is taken, up to J rows per call join through a join phase, and R is the longest leading kept run they prefill there in one pass.  R <= max_prefix of the
 * handle (hqt_set_max_prefix has sized the body workspace for such a pass); R == 0 with text conditioning and three code levels, where the prefix prefill is not
 * built.  On a text-conditional handle the call also counts as hqt_set_max_joins(h, J).  Grows, never shrinks, the staging K/V to [n_layers][J][rows][D] at 4 bytes
 * per element, rows = ctx_len_txt + R on a text handle and 1 + R otherwise, and the gathered rows [max_batch][D] fp32: the buffers of hqt_set_prompt_groups /
 * hqt_set_max_joins, sized to the largest need and counted by hqt_workspace_bytes.  A handle without text conditioning and with R == 0 needs none (no join phase
 * ever runs there).  A sampling call allocates nothing.  A lane from hqt_clone inherits the setting and gets a staging of its own.  max_joins == 0 switches the
 * opt-in off again and frees nothing.
 * HQT_ERR_INVALID: a NULL handle, a handle without stage 2, max_joins outside [0, max_batch], max_run outside [0, max_prefix], max_run > 0 on a text handle with
 * three code levels.  HQT_ERR_STATE: the handle holds a rolling pass. */
int hqt_set_join_run(hqt_handle* h, int max_joins, int max_run);

/* hqt_sample -- replaces sampling_ihqgpt + iHQGPT.sampling_step (hqvae/utils/sampling.py:164-237,
 * hierarchical_ar.py:428-480, 482-563, 667-789) for a batch of B independent images.
 *   cond        int64 [B] class ids (HQT_COND_CLASS), int64 [B, ctx_len_txt] token ids
 *               (HQT_COND_TEXT), ignored/NULL (HQT_COND_NONE)
 *   noise       fp32 [n_steps, 5, B, V] Exp(1) variates q, draw order top, bot0..bot3; the draw is
 *               argmax(p / q) (== torch.multinomial(p, 1) for the q it draws).  NULL: Philox(seed).
 *   force_top   optional int64 [B, n_steps]: the top code fed back instead of the drawn one
 *               (given_top_code, hierarchical_ar.py:768-774); the draw is still written to out_top
 *   force_bot   optional int64 [B, n_steps, 4]: same for the four bottom codes (teacher forcing)
 *   logits_out  optional fp32 [n_steps, 5, B, V]: raw (pre-temperature) logits of every draw
 *   out_top     int64 [B, n_steps]      codes_top
 *   out_bot     int64 [B, n_steps, 4]   codes_bot, slot = 2*kh + kw */
int hqt_sample(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts* opts, const float* noise,
               const int64_t* force_top, const int64_t* force_bot, float* logits_out,
               int64_t* out_top, int64_t* out_bot, void* stream);

/* Three-level counterparts.  hqt_sample_l3 replaces sampling_hqtransformer + HQTransformer.sampling_step
 * (hqvae/utils/sampling.py:240-307, hqtransformer.py:409-635): per top position 1 + 4 + 16 codes.
 *   noise / logits_out  fp32 [n_steps, 21, B, V], draw order level 0, level-1 slots 0..3, level-2 tokens 0..15 in
 *                       (H1 H2 W1 W2) raster order (= kh * 4 + kw of the 4x4 block)
 *   force0/1/2          optional teacher forcing, int64 [B, n_steps] / [B, n_steps, 4] / [B, n_steps, 16]
 *   out0/1/2            int64 [B, n_steps], [B, n_steps, 4], [B, n_steps, 16]
 * hqt_decode_l3 replaces HQVAEGenerator.decode_code([t, m, b]) (generator.py:577-599): code grids [B, r/4, r/4],
 * [B, r/2, r/2], [B, r, r] (any may be NULL = zero quant); hqt_decode_seq_l3 takes the sampler's own outputs and folds
 * the rearranges of sampling_hqmodel.py:150-153 into the lookup. */
typedef struct {
    int32_t precision, n_steps;
    int32_t top_k[3];
    float top_p[3];
    float temperature[3];
    uint64_t seed;
    int64_t sample_offset;
    int32_t use_graph;
    const uint64_t* row_seeds;      /* as in hqt_sample_opts */
    const int64_t* row_offsets;
} hqt_sample_opts_l3;
int hqt_sample_l3(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts_l3* opts, const float* noise,
                  const int64_t* force0, const int64_t* force1, const int64_t* force2, float* logits_out,
                  int64_t* out0, int64_t* out1, int64_t* out2, void* stream);
/* hqt_set_max_prefix -- no reference counterpart.  Largest code prefix a later hqt_sample_prefix / hqt_sample_prefix_l3 call on this handle
 * may pass.  A handle starts with max_prefix = 0: such calls are refused and the workspace is what hqt_create has always allocated.  The
 * prefix prefill runs all body blocks over max_batch * (max_prefix + 1) rows at once (text conditioning: the prompt and the prefix share
 * one pass of max_batch * (ctx_len_txt + max_prefix) rows); this call re-sizes the body workspace (activations,
 * split-K slabs, packed copies -- not the KV cache, which max_steps already covers) for that pass.  An entry point and not a field of
 * hqt_config, so that the struct, and with it ABI version 9, stay what they are (as with hqt_set_row_samplers).  Call it between hqt_create
 * and hqt_finalize_weights (HQT_ERR_STATE afterwards: lanes, captured graphs and the persistent chain's phase tables hold workspace pointers);
 * lanes made by hqt_clone inherit the value.  HQT_ERR_INVALID: max_prefix outside [0, max_steps - 1], a handle without stage 2, text
 * conditioning with three code levels, text conditioning with max_batch * (ctx_len_txt + max_prefix) beyond the 16384 rows of one pass. */
int hqt_set_max_prefix(hqt_handle* h, int max_prefix);

/* hqt_sample_prefix / hqt_sample_prefix_l3 -- completion (no reference counterpart as a call: the reference can only
 * teacher-force a whole run position by position): the codes of positions 0 .. prefix_len - 1 are given, positions prefix_len .. n_steps - 1
 * are drawn exactly as hqt_sample / hqt_sample_l3 would draw them had its first prefix_len positions produced these codes -- same Philox keys
 * (seed, global row, ABSOLUTE position, draw, chunk), same slice of `noise` (indexed by absolute position), same sampler settings and row
 * tables.  The prefix is not fed through the model one position at a time: its prefix_len + 1 body input rows per sample (the sos / class row,
 * then the input embedding of every prefix position) are written by one kernel and all body blocks run causally over them in ONE pass that
 * fills the KV cache; the depth head runs on the last row only and draws position prefix_len.  The remaining positions are ordinary decode steps.
 * Text conditioning (two code levels): the ctx_len_txt prompt rows and the prefix_len input rows of positions 1 .. prefix_len are that ONE
 * pass (ctx_len_txt + prefix_len rows per sample; FAST: the tiled matrix-core prefill attention from 65 rows on).
 *   prefix_len   1 .. min(n_steps - 1, max_prefix of the handle: hqt_set_max_prefix)
 *   prefix_top   int64 [B, prefix_len]; prefix_bot int64 [B, prefix_len, 4]   (l3: prefix0 [B, P], prefix1 [B, P, 4], prefix2 [B, P, 16]);
 *                values outside the vocabulary are clamped into it on the device, as every id that arrives from the caller (cond,
 *                force_*): device pointers cannot be checked on the host, so such input is NOT an error here and hqt_range_check
 *                does not report it -- a caller that cannot vouch for its codes checks them first (the Python surface raises IndexError)
 *   out_*        full length, as in hqt_sample: positions < prefix_len hold the prefix verbatim -- for a prefix inside the
 *                vocabulary; a clamped value comes back clamped
 *   force_*      [B, n_steps] ... as in hqt_sample; entries of positions < prefix_len are not read
 *   logits_out   as in hqt_sample; the rows of positions < prefix_len are not written
 * Every other argument as in hqt_sample / hqt_sample_l3.  HQT_ERR_INVALID: prefix_len < 1, prefix_len >= n_steps, prefix_len >
 * the handle's max_prefix (the message names hqt_set_max_prefix), a NULL prefix pointer, a text-conditional model with three code levels. */
int hqt_sample_prefix(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts* opts, const float* noise,
                      int prefix_len, const int64_t* prefix_top, const int64_t* prefix_bot,
                      const int64_t* force_top, const int64_t* force_bot, float* logits_out,
                      int64_t* out_top, int64_t* out_bot, void* stream);
int hqt_sample_prefix_l3(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts_l3* opts, const float* noise,
                         int prefix_len, const int64_t* prefix0, const int64_t* prefix1, const int64_t* prefix2,
                         const int64_t* force0, const int64_t* force1, const int64_t* force2, float* logits_out,
                         int64_t* out0, int64_t* out1, int64_t* out2, void* stream);
/* hqt_score -- the eval-mode `forward` of the reference (iHQGPT.forward, hierarchical_ar.py:246-426; HQTransformer.forward,
 * hqtransformer.py:226-407) as a scoring call: the log-probability of GIVEN codes in one teacher-forced pass over all positions.  Every body
 * input row follows from the codes, so the body runs once, causally, over n rows per sample (the prefix prefill with prefix_len = n - 1; text:
 * ctx_len_txt + n - 1 rows); the depth head then runs over all B n (sample, position) pairs, numbered p = b n + t, in chunks of at most
 * `chunk` pairs (hqt_set_score_chunk; never called: max_batch pairs and no allocation beyond hqt_create's).  A chunk may straddle samples.
 *   codes        one device pointer per level, coarse to fine, in the sampler's layout: int64 [B, n], [B, n, 4][, [B, n, 16]]; values outside
 *                the vocabulary are clamped into it, as in hqt_sample_prefix
 *   logprobs     fp32 [B, n, draws], draws = 5 or 21: entry (b, t, d) = l[code] - max(l) - logf(sum expf(l - max(l))) over the raw logits row
 *                of draw d at position t given the sample's codes before t (T = 1, no cut-off: what hqt_set_logprob_out reports for a forced run)
 *   logits_out   NULL, or one pointer per level, each NULL or fp32 raw logits [B, n, V], [B, n, 4, V][, [B, n, 16, V]]
 * Runs eagerly on `stream`; touches neither the graph cache nor its key, leaves the step state at (0, 0) and the K/V cache and the code
 * buffers overwritten: a sampling call afterwards draws what it drew before.  The handle needs hqt_set_max_prefix(h, >= n - 1) (n = 1: none).
 * HQT_ERR_STATE: not finalized, max_prefix too small, a precision whose layout the handle was built without, a staged row-sampler table,
 * pair table or log-probability buffer (they belong to a sampling call; hqt_score clears them).  A staged hqt_set_draw_report IS taken: entry
 * (b, t, d) of the report describes the row of logprobs entry (b, t, d), c being the given code (timing slot "draw_report", one launch per
 * level and chunk).  HQT_ERR_INVALID: NULL logprobs / codes, a staged report whose top_n exceeds the vocabulary,
 * B or n out of range, the 'top2mid2bot' head (21 causal sub-steps: score it stepwise, hqt_sample_l3 with forced codes), three code levels
 * with text conditioning.
 * hqt_set_score_chunk -- pairs per depth chunk, between hqt_create and hqt_finalize_weights (lanes inherit it): sizes the depth workspace
 * (depth rows, logits, depth K/V) for `pairs` pairs and the row buffers for pairs x Tdepth rows (Tdepth = 4, 5 'bidirectional', 16 three
 * levels) where they are smaller.  HQT_ERR_INVALID: pairs < 0 or pairs x Tdepth beyond the 16384 rows of one pass; 0 restores the default. */
int hqt_set_score_chunk(hqt_handle* h, int pairs);
int hqt_score(hqt_handle* h, int B, const int64_t* cond, const int64_t* const* codes, int n, int precision, float* logprobs,
              float* const* logits_out, void* stream);
int hqt_decode_l3(hqt_handle* h, int B, const int64_t* code_t, const int64_t* code_m, const int64_t* code_b, float* out_pixels,
                  int clamp01, int precision, void* stream);
int hqt_decode_seq_l3(hqt_handle* h, int B, const int64_t* codes0, const int64_t* codes1, const int64_t* codes2, float* out_pixels,
                      int clamp01, int precision, void* stream);

/* hqt_encode -- replaces SimRQGAN2Generator.encode / get_codes (generator.py:298-310, 369-370) and, on a three-level
 * handle, HQVAEGenerator.encode (generator.py:530-568): Encoder.forward (stage1/modules/layers.py:270-297), quant_conv_b,
 * then per level coarse -> fine: PixelUnshuffle of (h - reconstruction so far), nearest code
 * argmin(|z|^2 + |e|^2 - 2 z.e) (quantizer.py:91-103), reconstruction += PixelShuffle(z + (e - z)).
 * Needs the encoder tensors (stage1.encoder.*, stage1.quant_conv_b.*) to have been set before hqt_finalize_weights;
 * without them the call fails with HQT_ERR_STATE.
 *   pixels   fp32 [B, 3, R, R] NCHW (device)
 * Level index l runs coarse -> fine (two levels: 0 = top, 1 = bottom); r_l = r >> (levels - 1 - l),
 * dim_l = embed_dim * 4^(levels - 1 - l) (s1_resample != 0: dim_l = embed_dim on both levels, the top quantiser's input is
 * down_t(h) and the reconstruction of the top level is upsample_t(quant_t): see hqt_config.s1_resample).  Every pointer of
 * hqt_encode_out except codes[] may be NULL.
 *   codes[l]  int64 [B, r_l, r_l]                 (the reference returns them flattened)
 *   quant[l]  fp32 [B, dim_l, r_l, r_l]           the straight-through quantised tensor of level l (quant_t / quant_b)
 *   resid[l]  fp32 [B, dim_l, r_l, r_l]           the quantiser's input of level l (resid[1] of a two-level model is
 *                                                 the reference's code[2] = h_b)
 *   recon     fp32 [B, embed_dim, r, r]           sum of all levels in the bottom layout (HQVAEGenerator: recons[-1])
 *   diff      fp32 [levels]                       0.25 * mean((e - z)^2) per level (quantizer.py:130)
 * EXACT computes every convolution in fp32; FAST runs the convolutions in bf16 MFMA with fp32 accumulation.  The distance
 * GEMM and the argmin are fp32 in both, so the codes are always the exact nearest ones of the feature map the handle
 * computed (under FAST that map, and hence some codes, differ slightly from the fp32 one). */
typedef struct {
    int64_t* codes[3];
    float* quant[3];
    float* resid[3];
    float* recon;
    float* diff;
} hqt_encode_out;
int hqt_encode(hqt_handle* h, int B, const float* pixels, int precision, const hqt_encode_out* out, void* stream);
/* 1 when the handle holds the encoder tensors (hqt_encode is usable), else 0; -1 on a NULL handle */
int hqt_has_encoder(const hqt_handle* h);

/* hqt_decode -- replaces SimRQGAN2Generator.decode_code (generator.py:323-367: codebook lookup
 * quantizer.py:179-186, PixelShuffle, concat, post_quant_conv_b, Decoder.forward layers.py:385-410).
 *   code_t      int64 [B, r/2, r/2] or NULL (that level contributes a zero quant, generator.py:328-358; with
 *               s1_resample = HQT_RESAMPLE_CONV2 the zero quant still collects upsample_t.bias)
 *   code_b      int64 [B, r, r] or NULL          (r = bottom grid = resolution / 2^n_levels)
 *   out_pixels  fp32 [B, out_ch, H, W] NCHW; clamp01 != 0 fuses clamp(0.5 x + 0.5, 0, 1)
 *               (measure_throughput/__main__.py:113) into the last kernel, else raw decoder output
 * hqt_decode_seq takes the sampler's own outputs (codes_top [B, (r/2)^2], codes_bot [B, (r/2)^2, 4])
 * and folds the two rearranges of sampling_hqmodel.py:119-120 into the lookup addressing. */
int hqt_decode(hqt_handle* h, int B, const int64_t* code_t, const int64_t* code_b, float* out_pixels,
               int clamp01, int precision, void* stream);
int hqt_decode_seq(hqt_handle* h, int B, const int64_t* codes_top, const int64_t* codes_bot, float* out_pixels,
                   int clamp01, int precision, void* stream);

/* hqt_range_check -- no reference counterpart (the reference decodes in fp32, generator.py:323-367, where nothing can leave the
 * range).  SPLIT-precision calls carry every fp32 activation as two fp16 values; an activation that is NaN or >= 65504 in magnitude
 * cannot travel that way.  The operand pass saturates it and sets a flag on the handle instead of failing the (asynchronous) call.
 * hqt_range_check synchronises `stream` (the one the calls were enqueued on), returns HQT_ERR_RANGE if any SPLIT call since the last
 * check met such a value (and clears the flag), HQT_OK otherwise.  The Python surface calls it wherever it hands pixels or codes of a
 * SPLIT call to the host side (decode_code / encode of lane 0, InflightSampler.drain).
 * Since round 5 it also reports the one asynchronous failure of a FAST call: hqt_sample of up to 64 samples on a root handle runs a top
 * position as ONE persistent launch that needs every compute unit of the device resident at once (hqtransformer_amd/csrc/persist.h); every
 * spin in it is bounded (1 s), and a launch that could not finish -- the GPU is shared with something that keeps compute units busy --
 * marks the handle instead of hanging: HQT_ERR_STATE here ("... gave up at the grid barrier in front of phase p"), the codes of that call
 * are invalid, later launches return at once until this call has cleared the mark -- and the handle then takes the launch chain
 * (hqt_set_switch(h, HQT_SWITCH_PERSIST, 1) re-arms the persistent launch).  Persistent launches of ALL handles of a process on one
 * device are ordered behind each other (an event chain inside the library), so two root handles sampling on two streams both finish.
 * hqt_set_switch(h, HQT_SWITCH_PERSIST, 0), or HQT_PERSIST=0 in the environment at hqt_create, selects the launch chain from the start. */
int hqt_range_check(hqt_handle* h, void* stream);

/* introspection */
int hqt_abi_version(void);
int64_t hqt_param_count(const hqt_handle* h, int stage);       /* stage 1 | 2: elements received */
int64_t hqt_workspace_bytes(const hqt_handle* h);
/* name of the kernel that dominates phase (0 = AR loop, 1 = decode) and its launch count / total
 * device time in ms since hqt_timing_reset, measured with HIP events on the caller's stream when
 * timing is enabled (bench.py's roofline numerator) */
int hqt_timing_enable(hqt_handle* h, int on);
int hqt_timing_reset(hqt_handle* h);
int hqt_timing_get(hqt_handle* h, int slot, char* name, int name_len, int64_t* launches, double* total_ms);
int hqt_timing_slots(const hqt_handle* h);

int hqt_destroy(hqt_handle* h);
const char* hqt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HQT_H */
