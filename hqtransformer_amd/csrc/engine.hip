// libhqt.so host side: handle, weight registry, workspaces and the launch sequences behind the C ABI
// of include/hqt.h.  No CPU compute path exists here: every tensor operation is a HIP kernel.
#include "../../include/hqt.h"
#include "kernels.h"
#include "fast_kernels.h"
#include "split_kernels.h"
#include "persist.h"
#include "switches.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(expr)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return fail(HQT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                              \
    } while (0)
#define CHK(expr)                  \
    do {                           \
        int r_ = (expr);           \
        if (r_ != HQT_OK) return r_; \
    } while (0)

// Entry points run on the handle's device and put the caller's current device back on return (C-ABI callers that drive several
// devices from one thread would otherwise find it silently changed).
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = prev == dev || hipSetDevice(dev) == hipSuccess;
        if (prev == dev) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};
#define ON_DEVICE(h_)                                                                          \
    DeviceGuard dg_((h_)->device);                                                             \
    if (!dg_.ok) return fail(HQT_ERR_HIP, "hipSetDevice(%d) failed", (h_)->device)

struct Tensor {
    float* d = nullptr;
    std::vector<int64_t> shape;
    size_t n = 0;
};

struct Lin {            // one nn.Linear / conv filter bank in every layout the kernels read
    const float* w32 = nullptr;   // [N, K] fp32 (conv: tap-major [O][tap][I])
    const float* b32 = nullptr;   // [N] or null
    bf16_t* w16 = nullptr;        // [N, K] bf16 row-major (FAST generic + conv MFMA)
    half_t* w16h = nullptr;       // [N, K] fp16 hi / lo planes of w32 (SPLIT convolutions: split_kernels.h)
    half_t* w16l = nullptr;
    float* w32t = nullptr;        // fp32 copy in MFMA fragment order [N / 16][K / 32][chunk][lane][4] (EXACT AR loop at small row counts: exact_gemm.hip)
    half_t* wfrag16 = nullptr;    // 3x3 filters, hi + lo, packed in MFMA fragment order (16-channel blocks of v_mfma_f32_16x16x32_f16; split_stream_conv.hip)
    half_t* wup16 = nullptr;      // upsampling convs: the four 2x2 phase filters (pre-summed taps), same packing
    bf16_t* wpk = nullptr;        // MFMA-fragment-packed bf16 for the weight-streaming GEMM (FAST AR)
    bf16_t* wpk_ln = nullptr;     // same packing of gamma o W (deferred LayerNorm), with its column sums and folded bias
    float* colsum = nullptr;
    float* bias_ln = nullptr;
    int N = 0, K = 0;
};

struct BlockW {
    bool body = false;       // a block of the top GPT (its weights are read once per position), not of the depth head
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    Lin qkv, proj, fc1, fc2;
};

struct DecLayer {
    int kind;            // 0 conv3, 1 res, 2 attn, 3 upconv, 4 out; encoder: 5 Downsample, 6 conv_in, 7 out
    std::string name;
    int cin, cout, res;
    Lin conv1, conv2, nin, q, k, v, proj;      // conv3/upconv/out use conv1
    const float *n1_g = nullptr, *n1_b = nullptr, *n2_g = nullptr, *n2_b = nullptr;
};

// One program of the persistent AR chain (persist.h): the weight streams belong to the root handle, the phase table holds
// workspace pointers and is bound per handle (a clone binds its own).
struct PersistProg {
    std::vector<PersistPhase> phases;         // host copy; pointers filled by persist_bind
    char* stream = nullptr;
    unsigned long long* d_cu_off = nullptr;
    PersistPhase* d_phases = nullptr;
    bool ok = false;
};

struct TimingSlot {
    std::string name;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    int64_t launches = 0;
    double total_ms = 0.0;
};

struct hqt_handle {
    hqt_config cfg;
    int device = 0;
    bool finalized = false;
    std::map<std::string, Tensor> w;
    std::vector<void*> owned;                 // every device allocation, freed in destroy
    size_t workspace_bytes = 0;
    int64_t params[3] = {0, 0, 0};
    // ---- stage 2
    std::vector<BlockW> body, depth;
    Lin head_top, head_bot;
    int Tmax = 0;
    int max_prefix = 0;                       // hqt_set_max_prefix: longest code prefix a call may pass (0: none); lanes inherit it
    static constexpr int BODY_BUFS = 10;
    size_t body_bytes[BODY_BUFS] = {};        // what alloc_body_rows allocated, in its order
    int depth_rows = 0;                       // keys of the depth cache: 5 (two code levels) or 21 (three)
    int score_chunk = 0;                      // hqt_set_score_chunk: (sample, position) pairs per depth chunk of hqt_score (0: max_batch); lanes inherit it
    int depth_cap() const { return std::max(cfg.max_batch, score_chunk); }      // "samples" the depth workspace (xd, logits, dk, dv) holds
    static constexpr int DEPTH_BUFS = 4;
    size_t depth_bytes[DEPTH_BUFS] = {};      // what alloc_depth_ws allocated, in its order
    float *x = nullptr, *xd = nullptr, *logits = nullptr;
    void *hbuf = nullptr, *qbuf = nullptr, *abuf = nullptr, *mbuf = nullptr;    // fp32-sized, reused as bf16 in FAST
    void *kcache = nullptr, *vcache = nullptr, *dk = nullptr, *dv = nullptr;
    bf16_t *xpk = nullptr, *xdpk = nullptr;   // bf16 packed copies of the residual streams (FAST deferred LayerNorm)
    float *parts = nullptr, *partsd = nullptr; // their partial row statistics [D/32][Mpad][2]
    int nparts = 0, npartsd = 0;
    float* fold_tmp = nullptr;
    bool tile_gemm = true;                    // merged passes through the LDS-tiled MFMA kernels (HQT_NO_TILE_GEMM=1: streaming kernels at every row count)
    float* splitk = nullptr;                  // split-K partial slabs of the streaming GEMM
    size_t splitk_elems = 0;
    struct { const float* slabs; int S; int rows; const float* bias; } pend = {nullptr, 0, 0, nullptr};   // folded in by the next LayerNorm
    StepState* state = nullptr;
    RowKey* rows = nullptr;                   // [max_batch] Philox seed + global row of every batch row of the current call
    // per-row keys of merged steps travel through a ring of PINNED staging buffers (an asynchronous copy from pinned memory reads its
    // source when the stream gets there: a buffer is rewritten only after the copy that last read it has completed, hipEventSynchronize)
    static constexpr int ROWS_RING = 4;
    RowKey* rows_pinned[ROWS_RING] = {nullptr, nullptr, nullptr, nullptr};       // each: the five tables of a RingSlot (ring_slot)
    hipEvent_t rows_ev[ROWS_RING] = {nullptr, nullptr, nullptr, nullptr};
    bool rows_busy[ROWS_RING] = {false, false, false, false};
    int rows_next = 0;
    RowSampler* row_set = nullptr;            // [max_batch] per-row sampler settings of the current call (hqt_set_row_samplers)
    GuidePair* guide = nullptr;               // [guide_room()] pair table of the current call (hqt_set_guidance)
    size_t guide_room() const { return (size_t)std::max(1, cfg.max_batch / 2); }      // a row is in at most one pair
    unsigned char* keep_mask = nullptr;       // [max_batch * max_steps] mask of the current call
    int* group_of_row = nullptr;              // [max_batch] group table of the current call
    int* row_pos = nullptr;                   // [3 * max_batch] rolling pass (hqt_set_row_positions): [0, max_batch) the position every row stands at, moved on by
                                              // advance_rows between the steps of a call; [max_batch, 2 max_batch) the table as the call received it (what it copies out);
                                              // [2 max_batch, 3 max_batch) the join table of a text pass: 0 for a row that joins in this call, -1 for every other
    int* row_pos_received() const { return row_pos + cfg.max_batch; }
    int* row_pos_join() const { return row_pos + 2 * (size_t)cfg.max_batch; }
    // What the hqt_set_* calls leave for the next hqt_sample / hqt_sample_l3 (or prefix entry point) of this handle, which takes all of it
    struct Staged {
        std::vector<hqt_row_sampler> row_set;     // hqt_set_row_samplers: host table
        float* logprob = nullptr;                 // hqt_set_logprob_out: device fp32 [B, n_steps, draws]
        ReportOut report = {nullptr, nullptr, 0, nullptr, nullptr};   // hqt_set_draw_report: device buffers [B, n_steps, draws(, top_n)]; hqt_score takes it too
        std::vector<hqt_guide_pair> guide;        // hqt_set_guidance: host table
        std::vector<uint8_t> keep;                // hqt_set_keep_mask: host mask [keep_B, keep_n] and one device pointer per level
        int keep_B = 0, keep_n = 0;
        const int64_t* keep_codes[3] = {nullptr, nullptr, nullptr};
        std::vector<int32_t> groups;              // hqt_set_prompt_groups: host table [B] of prompt indices in [0, groups_G)
        int groups_G = 0;
        bool seg = false;                         // hqt_set_segment: positions [seg_start, seg_stop)
        int seg_start = 0, seg_stop = 0;
        std::vector<int32_t> roll;                // hqt_set_row_positions: host table [B] of next positions (-1: empty slot) and the steps of the call
        int roll_k = 0;
        // what hqt_score refuses; deliberately not the segment: one staged alone is cleared there without a refusal
        bool holds_table() const { return !row_set.empty() || logprob || !guide.empty() || !keep.empty() || !groups.empty(); }
    } staged;
    Staged take_staged() { Staged s = std::move(staged); staged = Staged(); return s; }
    void clear_staged() { staged = Staged(); }
    // staging of staged_prompt_prefill (shared prompts; the joiners of a rolling pass), sized (grown) by hqt_set_prompt_groups, hqt_set_max_joins and hqt_set_join_run
    // (reserve_prompt_staging) and by nothing else: K and V of [n_layers][prompts][rows][D] at 4 bytes per element (any mode's activation type fits) for the largest
    // prompts * rows asked for (rows: ctx_len_txt, with hqt_set_join_run + max_run, 1 + max_run without text), and the [max_batch, D] fp32 rows the fan-out gathers
    // for the depth head of the position behind the prefill
    void *pg_k = nullptr, *pg_v = nullptr;
    float* pg_x = nullptr;
    int pg_cap = 0;                           // prompts (of ctx_len_txt rows or more) the staging holds
    size_t pg_bytes = 0;                      // bytes of pg_k (= pg_v)
    int max_joins = 0;                        // hqt_set_max_joins: rows that may join a rolling pass of a text handle in one call (0: such a pass is refused)
    int join_run = -1;                        // hqt_set_join_run: a rolling call may take a keep table, and joining rows prefill a shared leading kept run of up to this
                                              // many positions in the join phase, max_joins of them per call (-1: not opted in, such a call is refused)
    int staging_rows(int run) const { return (cfg.cond_type == HQT_COND_TEXT ? cfg.ctx_len_txt : 1) + run; }      // body rows of one joiner in the join phase
    // the pass a segment stopped in: what a continuation must match, and `pos`, the position it goes on from (the step state says pos over t_live keys)
    struct Paused { bool live = false; int B = 0, n_steps = 0, levels = 0, precision = 0, pos = 0; } paused;
    // the rolling pass the last hqt_set_row_positions call left: what the next one must match, and per slot the position it draws next (-1: empty)
    struct Rolling { bool live = false; int B = 0, n_steps = 0, levels = 0, precision = 0; std::vector<int32_t> next; } rolling;
    int64_t *cond_buf = nullptr, *codes_top = nullptr, *codes_bot = nullptr;   // call-independent homes of cond / the drawn codes
    int64_t* codes_l2 = nullptr;              // third level: [B, max_steps, 16]
    Lin head_l2;                              // head_levels.2 (three-level models; head_top / head_bot hold levels 0 / 1)
    // ---- stage 1
    std::vector<DecLayer> dec;
    std::vector<DecLayer> enc;               // Encoder.forward in execution order (kinds 6 conv_in, 1, 2, 5 Downsample, 7 norm_out + conv_out)
    bool has_encoder = false;                 // the encoder tensors were set before finalize: hqt_encode is usable
    Lin post_quant, quant_conv;
    float* cb_norm[3] = {nullptr, nullptr, nullptr};   // |e_n|^2 of each codebook (distance GEMM epilogue)
    float *vq_h = nullptr, *vq_recon = nullptr, *vq_zz = nullptr, *vq_err = nullptr;
    void* vq_z = nullptr;
    unsigned long long* vq_best = nullptr;
    // ---- E-wide top level (hqt_config.s1_resample != 0: 'nearest', 'conv2')
    float* up_table = nullptr;                // conv2: upsample_t folded over the top codebook, [n_embed][2][2][E] (launch_fold_upsample_t)
    Lin up_lin, down_lin;                     // conv2, encode side: upsample_t as a Linear [4E, E] (launch_repack_upsample_t), down_t as a Linear [E, 4E]
    float *vq_t = nullptr, *vq_q = nullptr;   // encode workspace: the top quantiser's input rows h_t and its straight-through rows, [B (r/2)^2, E] each
    void* act[4] = {nullptr, nullptr, nullptr, nullptr};   // 3 rotating activation buffers + the normalised/activated copy (FAST)
    double* gn_partial = nullptr;
    float* gn_tiles = nullptr;                // per-tile output statistics of the last halo conv ([image][tile][32][2]); S1Ctx::gn_ready says of which tensor
    void* zero_page = nullptr;
    int* range_flag = nullptr;                // set by the SPLIT operand pass when an activation leaves the fp16 range (hqt_range_check)
    size_t act_elems = 0;
    int dec_chunk = 0;
    void *aq = nullptr, *ak = nullptr, *av = nullptr, *ao = nullptr, *as = nullptr, *quant = nullptr;
    float* gn = nullptr;                      // [chunk][32][2] x 2
    // ---- graph cache
    hipGraphExec_t graph_exec = nullptr;
    std::vector<uint64_t> graph_key;
    // ---- lanes: a clone shares every weight buffer of its parent (non-owning) and owns only its workspace
    hqt_handle* parent = nullptr;
    int n_clones = 0;
    int policy = 0;                           // HQT_POLICY_*: tile choice of the streaming GEMMs (part of the graph key)
    // ---- persistent AR chain (FAST precision, up to 64 rows, latency policy, root handle): body blocks / depth sub-step 0 + head_top
    PersistProg pbody, pfull;                 // body only (three code levels) / the whole position up to the top logits (persist_build)
    float* lnf_shift = nullptr;               // ln_f.bias + sos_depth (PP_LNF)
    int ncu = 0;
    unsigned* persist_counters = nullptr;     // workspace: barrier + quad counters (zeroed by every launch)
    unsigned* persist_err = nullptr;          // workspace: set by a launch that gave up on a barrier
    float* persist_slabs = nullptr;           // workspace: K-split partials
    bool persist_used = false;                // a persistent launch was queued since the last check of persist_err
    bool persist_enabled = true;              // HQT_SWITCH_PERSIST (default: on unless HQT_PERSIST=0 was in the environment at hqt_create)
    bool persist_tripped = false;             // a persistent launch of this handle gave up (hqt_range_check): the launch chain until HQT_SWITCH_PERSIST re-arms it
    bool single_key = true;                   // HQT_SWITCH_SINGLE_KEY (default: on unless HQT_NO_SINGLE_KEY was in the environment at hqt_create)
    bool split_kslices = true;                // HQT_SWITCH_SPLIT_KSLICES (default: on unless HQT_SPLIT_KSLICES_OFF was in the environment at hqt_create)
    bool capture_persist = false;             // run_persist ran since sample_run cleared it (is a persistent launch inside the graph being captured?)
    bool graph_has_persist = false;           // the cached graph holds persistent launches: every replay marks persist_used
    int layouts = 0;                          // HQT_LAYOUT_* bits hqt_finalize_weights builds for the AR loop's nn.Linear weights
    // ---- timing
    bool timing = false;
    std::vector<TimingSlot> slots;
    hipEvent_t chain_ev = nullptr;
    bool chain_valid = false;
    std::vector<hipEvent_t> all_events;
};

static int dev_alloc(hqt_handle* h, void** p, size_t bytes, bool workspace) {
    HIPCHK(hipMalloc(p, bytes ? bytes : 16));
    // test hook: HQT_POISON_WORKSPACE=1 fills every workspace buffer with 0xFF (NaN as fp32 / bf16, -1 as int64) so that
    // a read of something no kernel wrote shows up instead of passing on freshly zeroed memory
    const bool poison = switch_value(SW_POISON_WORKSPACE);                // read per allocation: tests switch it on around one engine
    if (poison && workspace && bytes) HIPCHK(hipMemset(*p, 0xFF, bytes));
    h->owned.push_back(*p);
    if (workspace) h->workspace_bytes += bytes;
    return HQT_OK;
}

// The one place that allocates the staging of staged_prompt_prefill, the prompt prefill over fewer rows than the pass has (hqt_handle::pg_*): room for `n_groups`
// prompts, grown and never shrunk (a larger need frees the old pair once the device has drained, a smaller one reuses it), and with the first need the gathered
// x rows.  Those start as zeros: with joiners as the prompts the prefill writes only their rows and runs the depth head over all.  The caller has set the device.
static int reserve_prompt_staging(hqt_handle* h, int n_groups, int rows = 0) {      // rows per prompt; 0: ctx_len_txt
    const hqt_config& c = h->cfg;
    if (rows == 0) rows = c.ctx_len_txt;
    if (!h->pg_x) {
        CHK(dev_alloc(h, (void**)&h->pg_x, (size_t)c.max_batch * c.embed_dim * 4, true));
        HIPCHK(hipMemset(h->pg_x, 0, (size_t)c.max_batch * c.embed_dim * 4));
        HIPCHK(hipDeviceSynchronize());          // (the calls that read it run on the caller's streams)
    }
    const size_t bytes = (size_t)c.n_layers * n_groups * rows * c.embed_dim * 4;
    if (bytes <= h->pg_bytes) { h->pg_cap = std::max(h->pg_cap, n_groups); return HQT_OK; }      // (rows >= ctx_len_txt: as many prompts fit)
    const int held = h->pg_cap;                  // (the larger pair holds them too)
    if (h->pg_k) {
        HIPCHK(hipDeviceSynchronize());          // an earlier call may still be reading the old pair
        for (void** p : {&h->pg_k, &h->pg_v}) {
            HIPCHK(hipFree(*p));
            h->owned.erase(std::remove(h->owned.begin(), h->owned.end(), *p), h->owned.end());
            h->workspace_bytes -= h->pg_bytes;
            *p = nullptr;
        }
        h->pg_cap = 0; h->pg_bytes = 0;
    }
    CHK(dev_alloc(h, &h->pg_k, bytes, true));
    CHK(dev_alloc(h, &h->pg_v, bytes, true));
    h->pg_bytes = bytes;
    h->pg_cap = std::max(held, n_groups);
    return HQT_OK;
}

// ------------------------------------------------------------------------------------------ timing
static int slot_id(hqt_handle* h, const char* name) {
    for (size_t i = 0; i < h->slots.size(); ++i)
        if (h->slots[i].name == name) return (int)i;
    h->slots.push_back(TimingSlot());
    h->slots.back().name = name;
    return (int)h->slots.size() - 1;
}
// Per-launch timers (bench.py's roofline numerator): consecutive launches share one event -- the end event of a
// launch is the start event of the next -- so a timed pass adds one hipEventRecord per kernel.
struct Timed {
    hqt_handle* h; int slot; hipStream_t st; bool on;
    Timed(hqt_handle* h_, const char* name, hipStream_t st_) : h(h_), slot(-1), st(st_), on(h_->timing) {
        if (!on) return;
        slot = slot_id(h, name);
        if (!h->chain_valid) {
            hipEventCreate(&h->chain_ev);
            hipEventRecord(h->chain_ev, st);
            h->chain_valid = true;
        }
    }
    // the launches so far belong to this timer's slot; what follows goes to `name` (a GEMM and its split-K combine)
    void next(const char* name) {
        if (!on) return;
        hipEvent_t e;
        hipEventCreate(&e);
        hipEventRecord(e, st);
        h->slots[slot].ev.push_back({h->chain_ev, e});
        h->slots[slot].used++;
        h->all_events.push_back(h->chain_ev);
        h->chain_ev = e;
        slot = slot_id(h, name);
    }
    ~Timed() {
        if (!on) return;
        hipEvent_t e;
        hipEventCreate(&e);
        hipEventRecord(e, st);
        h->slots[slot].ev.push_back({h->chain_ev, e});
        h->slots[slot].used++;
        h->all_events.push_back(h->chain_ev);
        h->chain_ev = e;
    }
};
// Which kernel variant served a launch, as zero-time slots of the timing report ("variant:<kernel>:<shape class>"): counted only
// while timing is on (un-graphed passes), so tests and bench.py can state what the timed schedule ran.
static void count_variant(hqt_handle* h, const char* fmt, ...) {
    if (!h->timing) return;
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    h->slots[slot_id(h, buf)].launches++;
}
static void timing_collect(hqt_handle* h) {
    if (h->chain_valid) hipEventSynchronize(h->chain_ev);
    for (auto& s : h->slots) {
        for (auto& pr : s.ev) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { s.total_ms += ms; s.launches++; }
        }
        s.ev.clear();
        s.used = 0;
    }
    for (hipEvent_t e : h->all_events) hipEventDestroy(e);
    h->all_events.clear();
    if (h->chain_valid) { hipEventDestroy(h->chain_ev); h->chain_valid = false; }
}

// ------------------------------------------------------------------------------------------ plan
static void build_decoder_plan(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    const int n = c.s1_n_mult;
    int block_in = c.s1_ch * c.s1_ch_mult[n - 1];
    int res = c.s1_resolution >> (c.s1_use_init_downsample ? n : n - 1);
    auto is_attn_res = [&](int r) {
        for (int i = 0; i < c.s1_n_attn_res; ++i) if (c.s1_attn_res[i] == r) return true;
        return false;
    };
    auto add = [&](int kind, const std::string& name, int cin, int cout, int r) {
        DecLayer l; l.kind = kind; l.name = name; l.cin = cin; l.cout = cout; l.res = r;
        h->dec.push_back(l);
    };
    add(0, "decoder.conv_in", c.s1_z_channels, block_in, res);
    if (c.s1_use_mid_block) {
        add(1, "decoder.mid.block_1", block_in, block_in, res);
        if (c.s1_use_attn) add(2, "decoder.mid.attn_1", block_in, block_in, res);
        add(1, "decoder.mid.block_2", block_in, block_in, res);
    }
    for (int lvl = n - 1; lvl >= 0; --lvl) {
        const int block_out = c.s1_ch * c.s1_ch_mult[lvl];
        for (int b = 0; b <= c.s1_num_res_blocks; ++b) {
            add(1, "decoder.up." + std::to_string(lvl) + ".block." + std::to_string(b), block_in, block_out, res);
            block_in = block_out;
            if (is_attn_res(res) && c.s1_use_attn)
                add(2, "decoder.up." + std::to_string(lvl) + ".attn." + std::to_string(b), block_in, block_in, res);
        }
        if (lvl != 0 || c.s1_use_init_downsample) {
            add(3, "decoder.up." + std::to_string(lvl) + ".upsample.conv", block_in, block_in, res);
            res *= 2;
        }
    }
    add(4, "decoder", block_in, c.s1_out_ch, res);
}

// Encoder.forward (stage1/modules/layers.py:270-297).  The reference tracks `curr_res` from `resolution` even when conv_in
// already halves the image (layers.py:221), so with use_init_downsample the attention test runs on twice the real size.
static void build_encoder_plan(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    const int n = c.s1_n_mult;
    auto is_attn_res = [&](int r) {
        for (int i = 0; i < c.s1_n_attn_res; ++i) if (c.s1_attn_res[i] == r) return true;
        return false;
    };
    auto add = [&](int kind, const std::string& name, int cin, int cout, int r) {
        DecLayer l; l.kind = kind; l.name = name; l.cin = cin; l.cout = cout; l.res = r;
        h->enc.push_back(l);
    };
    add(6, "encoder.conv_in", 3, c.s1_ch, c.s1_resolution);
    int label = c.s1_resolution;
    int res = c.s1_use_init_downsample ? c.s1_resolution / 2 : c.s1_resolution;
    int block_in = c.s1_ch;
    for (int lvl = 0; lvl < n; ++lvl) {
        const int block_out = c.s1_ch * c.s1_ch_mult[lvl];
        for (int b = 0; b < c.s1_num_res_blocks; ++b) {
            add(1, "encoder.down." + std::to_string(lvl) + ".block." + std::to_string(b), block_in, block_out, res);
            block_in = block_out;
            if (is_attn_res(label) && c.s1_use_attn)
                add(2, "encoder.down." + std::to_string(lvl) + ".attn." + std::to_string(b), block_in, block_in, res);
        }
        if (lvl != n - 1) {
            add(5, "encoder.down." + std::to_string(lvl) + ".downsample.conv", block_in, block_in, res);
            res /= 2; label /= 2;
        }
    }
    if (c.s1_use_mid_block) {
        add(1, "encoder.mid.block_1", block_in, block_in, res);
        if (c.s1_use_attn) add(2, "encoder.mid.attn_1", block_in, block_in, res);
        add(1, "encoder.mid.block_2", block_in, block_in, res);
    }
    add(7, "encoder", block_in, c.s1_z_channels, res);
}

// ------------------------------------------------------------------------------------------ create
extern "C" int hqt_abi_version(void) { return HQT_ABI_VERSION; }
extern "C" const char* hqt_last_error(void) { return g_err.c_str(); }

static int alloc_workspace(hqt_handle* hp);

extern "C" int hqt_create(const hqt_config* cfg, int device, hqt_handle** out) {
    if (!cfg || !out) return fail(HQT_ERR_INVALID, "null argument");
    if (cfg->abi_version != HQT_ABI_VERSION) return fail(HQT_ERR_INVALID, "abi_version %d != %d", cfg->abi_version, HQT_ABI_VERSION);
    if (cfg->max_batch < 1) return fail(HQT_ERR_INVALID, "max_batch must be >= 1");
    DeviceGuard dg(device);
    if (!dg.ok) return fail(HQT_ERR_HIP, "hipSetDevice(%d) failed", device);
    std::unique_ptr<hqt_handle> h(new hqt_handle());
    // the per-handle switches take their defaults from the environment HERE, once per handle (hqt_set_switch changes them afterwards); the other
    // switches of the call path are read where they act, once per process or per launch as their row of switches.h says
    h->tile_gemm = !switch_value(SW_NO_TILE_GEMM);
    h->persist_enabled = switch_value(SW_PERSIST);
    h->single_key = !switch_value(SW_NO_SINGLE_KEY);
    h->split_kslices = !switch_value(SW_SPLIT_KSLICES_OFF);
    h->cfg = *cfg;
    h->layouts = (cfg->ar_layouts & HQT_LAYOUT_ALL) ? (cfg->ar_layouts & HQT_LAYOUT_ALL) : HQT_LAYOUT_ALL;
    h->device = device;
    const hqt_config& c = h->cfg;
    if (c.has_stage2) {
        if (c.embed_dim % c.n_heads || c.embed_dim % 16) return fail(HQT_ERR_INVALID, "embed_dim must be a multiple of n_heads and 16");
        const int hs = c.embed_dim / c.n_heads;
        if (hs % 8 || hs > 256 || (hs & (hs - 1))) return fail(HQT_ERR_INVALID, "head_dim %d unsupported (power of two in [8, 256])", hs);
        if (c.vocab_top != c.vocab_bot) return fail(HQT_ERR_INVALID, "vocab_top != vocab_bot");
        const bool bidir = c.depth_decoding == HQT_DEPTH_BIDIRECTIONAL;
        if (c.depth_decoding < 0 || c.depth_decoding > HQT_DEPTH_BIDIRECTIONAL || (c.depth_decoding && !bidir && c.code_levels != 3) || (bidir && c.code_levels == 3))
            return fail(HQT_ERR_INVALID, "depth_decoding %d: 0 'parallel-add', 1 'parallel', 2 'parallel-reduce', 3 'top2mid2bot' (three code levels only), "
                        "4 'bidirectional' (two code levels only)", c.depth_decoding);
        if (bidir && c.cond_type == HQT_COND_TEXT)       // the reference's bidirectional step does not pick the last text token (hierarchical_ar.py:808)
            return fail(HQT_ERR_INVALID, "depth_decoding 4 'bidirectional' with text conditioning is not built");
        if (c.vocab_top > HQT_MAX_V || c.vocab_top % 4) return fail(HQT_ERR_INVALID, "vocab size %d unsupported", c.vocab_top);
        if (c.cond_type == HQT_COND_CLASS && c.n_classes < 1) return fail(HQT_ERR_INVALID, "n_classes");
        if (c.max_steps < 1 || c.max_steps > c.ctx_len_img) return fail(HQT_ERR_INVALID, "max_steps must be in [1, ctx_len_img]");
    }
    if (c.has_stage1) {
        if (c.s1_n_mult < 1 || c.s1_n_mult > 8) return fail(HQT_ERR_INVALID, "s1_n_mult");
        if (c.s1_ch % 32) return fail(HQT_ERR_INVALID, "GroupNorm(32) needs ch %% 32 == 0");
        if (c.s1_z_channels % 16 || (2 * c.s1_embed_dim) % 16) return fail(HQT_ERR_INVALID, "z_channels and 2*embed_dim must be multiples of 16");
        if (c.s1_resample < 0 || c.s1_resample > HQT_RESAMPLE_CONV2) return fail(HQT_ERR_INVALID, "s1_resample %d: 0 pixelshuffle, 1 nearest, 2 conv2", c.s1_resample);
        if (c.s1_resample && c.code_levels == 3) return fail(HQT_ERR_INVALID, "s1_resample %d with three code levels: the three-level HQ-VAE is built with pixelshuffle only", c.s1_resample);
        if (c.s1_resample == HQT_RESAMPLE_CONV2 && c.s1_embed_dim % 16) return fail(HQT_ERR_INVALID, "s1_resample 2 (conv2) needs embed_dim %% 16 == 0");
        build_decoder_plan(h.get());
        build_encoder_plan(h.get());
    }
    CHK(alloc_workspace(h.get()));
    *out = h.release();
    return HQT_OK;
}

// Everything a lane owns: activations, KV caches, step state, decoder buffers (the weights live in `w` / the Lin structs).
// nearest-code search state of hqt_encode: allocated once the encoder tensors are known to be present (finalize), and for clones
static int alloc_encode_workspace(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    const int r = h->dec.front().res;
    const size_t rows = (size_t)c.max_batch * r * r, elems = rows * c.s1_embed_dim;
    CHK(dev_alloc(h, (void**)&h->vq_h, elems * 4, true));
    CHK(dev_alloc(h, (void**)&h->vq_recon, elems * 4, true));
    CHK(dev_alloc(h, &h->vq_z, elems * 4, true));
    CHK(dev_alloc(h, (void**)&h->vq_zz, rows * 4, true));
    CHK(dev_alloc(h, (void**)&h->vq_best, rows * 8, true));
    CHK(dev_alloc(h, (void**)&h->vq_err, rows * 4 * 3, true));
    if (c.s1_resample) {
        CHK(dev_alloc(h, (void**)&h->vq_t, elems / 4 * 4, true));
        CHK(dev_alloc(h, (void**)&h->vq_q, elems / 4 * 4, true));
    }
    return HQT_OK;
}

// The stage-2 buffers sized by the rows of the widest pass: the body's text prompt (followed by max_prefix rows of a code prefix) or prefix
// prefill (max_prefix + 1 rows per sample; 0: one row) and the widest depth sub-step.  release_old (hqt_set_max_prefix): the handle's own
// earlier set goes first.
static int alloc_body_rows(hqt_handle* h, bool release_old) {
    const hqt_config& c = h->cfg;
    const size_t B = (size_t)c.max_batch, D = c.embed_dim;
    const int Tp = c.cond_type == HQT_COND_TEXT ? c.ctx_len_txt + h->max_prefix : (h->max_prefix > 0 ? h->max_prefix + 1 : 1);    // rows per sample of the widest body pass
    const int Tdepth = c.code_levels == 3 ? 16 : (c.depth_decoding == HQT_DEPTH_BIDIRECTIONAL ? 5 : 4);
    // (hqt_set_score_chunk: a depth chunk of hqt_score runs depth_cap() pairs x Tdepth rows through the same buffers; never called, depth_cap() is B)
    const size_t rows = (std::max(B * (size_t)std::max(Tp, Tdepth), (size_t)h->depth_cap() * Tdepth) + 31) / 32 * 32;
    // packed_off() buffers are addressed with a row stride of 32 * packed_mb(M) (32 / 64 / ... / 4096 rows), which can
    // exceed round32(M): size them for the widest padded block any M <= PACKED_MAX_ROWS pass can use
    size_t rows_pk = 256;
    while (rows_pk < rows && rows_pk < (size_t)PACKED_MAX_ROWS) rows_pk *= 2;
    rows_pk = std::max(rows_pk, rows);
    h->splitk_elems = (size_t)16 * rows * (size_t)std::max<size_t>(4 * D, (size_t)c.vocab_top);
    void** const bufs[hqt_handle::BODY_BUFS] = {(void**)&h->x, &h->hbuf, &h->qbuf, &h->abuf, &h->mbuf, (void**)&h->splitk,
                                                (void**)&h->xpk, (void**)&h->xdpk, (void**)&h->parts, (void**)&h->partsd};
    const size_t bytes[hqt_handle::BODY_BUFS] = {rows * D * 4, rows * D * 4, rows * D * 4, rows * D * 4, rows * 4 * D * 4, h->splitk_elems * 4,
                                                 rows_pk * D * 2, rows_pk * D * 2, (D / 32 + 1) * rows_pk * 2 * 4, (D / 32 + 1) * rows_pk * 2 * 4};
    for (int i = 0; i < hqt_handle::BODY_BUFS; ++i) {
        if (release_old && *bufs[i]) {
            HIPCHK(hipFree(*bufs[i]));
            h->owned.erase(std::remove(h->owned.begin(), h->owned.end(), *bufs[i]), h->owned.end());
            h->workspace_bytes -= h->body_bytes[i];
            *bufs[i] = nullptr;
        }
        CHK(dev_alloc(h, bufs[i], bytes[i], true));
        h->body_bytes[i] = bytes[i];
    }
    return HQT_OK;
}

// The depth workspace: input rows, logits and the depth K/V cache of depth_cap() "samples" (max_batch; hqt_set_score_chunk: the pairs of a chunk)
static int alloc_depth_ws(hqt_handle* h, bool release_old) {
    const hqt_config& c = h->cfg;
    const size_t cap = (size_t)h->depth_cap(), D = c.embed_dim;
    const int Tdepth = c.code_levels == 3 ? 16 : (c.depth_decoding == HQT_DEPTH_BIDIRECTIONAL ? 5 : 4);      // rows per sample of the widest depth sub-step
    const size_t dkv = (size_t)c.n_layers_depth * cap * h->depth_rows * D * 4;
    void** const bufs[hqt_handle::DEPTH_BUFS] = {(void**)&h->xd, (void**)&h->logits, &h->dk, &h->dv};
    const size_t bytes[hqt_handle::DEPTH_BUFS] = {cap * Tdepth * D * 4, cap * Tdepth * (size_t)c.vocab_top * 4, dkv, dkv};
    for (int i = 0; i < hqt_handle::DEPTH_BUFS; ++i) {
        if (release_old && *bufs[i]) {
            HIPCHK(hipFree(*bufs[i]));
            h->owned.erase(std::remove(h->owned.begin(), h->owned.end(), *bufs[i]), h->owned.end());
            h->workspace_bytes -= h->depth_bytes[i];
            *bufs[i] = nullptr;
        }
        CHK(dev_alloc(h, bufs[i], bytes[i], true));
        h->depth_bytes[i] = bytes[i];
    }
    return HQT_OK;
}

extern "C" int hqt_set_score_chunk(hqt_handle* h, int pairs) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    const hqt_config& c = h->cfg;
    if (!c.has_stage2) return fail(HQT_ERR_INVALID, "hqt_set_score_chunk: the handle was created without stage 2");
    if (h->finalized || h->parent) return fail(HQT_ERR_STATE, "hqt_set_score_chunk comes between hqt_create and hqt_finalize_weights (lanes inherit the value)");
    const int Tdepth = c.code_levels == 3 ? 16 : (c.depth_decoding == HQT_DEPTH_BIDIRECTIONAL ? 5 : 4);
    if (pairs < 0) return fail(HQT_ERR_INVALID, "hqt_set_score_chunk: pairs=%d is negative (0 restores the default, max_batch pairs)", pairs);
    if ((long long)pairs * Tdepth > PACKED_MAX_ROWS)
        return fail(HQT_ERR_INVALID, "hqt_set_score_chunk: pairs * Tdepth = %d * %d exceeds the %d rows of one pass (at most %d pairs for this depth head)", pairs, Tdepth, PACKED_MAX_ROWS, PACKED_MAX_ROWS / Tdepth);
    if (pairs == h->score_chunk) return HQT_OK;
    ON_DEVICE(h);
    const int cap_before = h->depth_cap();
    h->score_chunk = pairs;
    if (h->depth_cap() == cap_before) return HQT_OK;         // a chunk of at most max_batch pairs fits what hqt_create allocated
    CHK(alloc_depth_ws(h, true));
    return alloc_body_rows(h, true);
}

extern "C" int hqt_set_max_prefix(hqt_handle* h, int max_prefix) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    const hqt_config& c = h->cfg;
    if (!c.has_stage2) return fail(HQT_ERR_INVALID, "hqt_set_max_prefix: the handle was created without stage 2");
    if (h->finalized || h->parent) return fail(HQT_ERR_STATE, "hqt_set_max_prefix comes between hqt_create and hqt_finalize_weights (lanes inherit the value)");
    if (max_prefix < 0 || max_prefix > c.max_steps - 1) return fail(HQT_ERR_INVALID, "max_prefix=%d outside [0, max_steps - 1 = %d]", max_prefix, c.max_steps - 1);
    if (max_prefix && c.cond_type == HQT_COND_TEXT) {     // the prompt and the prefix share one prefill of ctx_len_txt + prefix_len rows per sample
        // (the two-level 'bidirectional' head with text conditioning is refused by hqt_create)
        if (c.code_levels == 3) return fail(HQT_ERR_INVALID, "max_prefix with text conditioning and three code levels is not built (two code levels are)");
        if ((long long)c.max_batch * (c.ctx_len_txt + max_prefix) > PACKED_MAX_ROWS)
            return fail(HQT_ERR_INVALID, "max_batch * (ctx_len_txt + max_prefix) = %d * (%d + %d) exceeds the %d rows of one pass", c.max_batch, c.ctx_len_txt, max_prefix, PACKED_MAX_ROWS);
    }
    if (max_prefix == h->max_prefix) return HQT_OK;
    ON_DEVICE(h);
    h->max_prefix = max_prefix;
    return alloc_body_rows(h, true);
}

static int alloc_workspace(hqt_handle* hp) {
    struct { hqt_handle* p; hqt_handle* get() const { return p; } hqt_handle* operator->() const { return p; } } h{hp};
    const hqt_config& c = h->cfg;
    const size_t B = (size_t)c.max_batch;
    // source of padded rows / taps for the LDS-DMA kernels (stage-2 GEMMs with more than 256 rows use them too: the text
    // prefill and the third code level)
    CHK(dev_alloc(h.get(), &h->zero_page, 256, true));
    HIPCHK(hipMemset(h->zero_page, 0, 256));
    CHK(dev_alloc(h.get(), (void**)&h->range_flag, 256, true));
    HIPCHK(hipMemset(h->range_flag, 0, 256));
    if (c.has_stage2) {
        const size_t D = c.embed_dim;
        h->Tmax = (c.cond_type == HQT_COND_TEXT ? c.ctx_len_txt : 0) + c.max_steps;
        h->depth_rows = c.code_levels == 3 ? 21 : 5;
        CHK(alloc_body_rows(h.get(), false));
        h->xd = h->logits = nullptr; h->dk = h->dv = nullptr;     // (a clone starts from its root's pointers)
        CHK(alloc_depth_ws(h.get(), false));
        const size_t kv = (size_t)c.n_layers * B * h->Tmax * D * 4;
        CHK(dev_alloc(h.get(), &h->kcache, kv, true));
        CHK(dev_alloc(h.get(), &h->vcache, kv, true));
        CHK(dev_alloc(h.get(), (void**)&h->state, sizeof(StepState), true));
        CHK(dev_alloc(h.get(), (void**)&h->rows, B * sizeof(RowKey), true));
        CHK(dev_alloc(h.get(), (void**)&h->row_set, B * sizeof(RowSampler), true));
        CHK(dev_alloc(h.get(), (void**)&h->guide, h->guide_room() * sizeof(GuidePair), true));
        CHK(dev_alloc(h.get(), (void**)&h->keep_mask, B * (size_t)c.max_steps, true));
        CHK(dev_alloc(h.get(), (void**)&h->group_of_row, B * sizeof(int), true));
        CHK(dev_alloc(h.get(), (void**)&h->row_pos, 3 * B * sizeof(int), true));
        CHK(dev_alloc(h.get(), (void**)&h->cond_buf, B * (size_t)std::max(1, c.cond_type == HQT_COND_TEXT ? c.ctx_len_txt : 1) * 8, true));
        CHK(dev_alloc(h.get(), (void**)&h->codes_top, B * (size_t)c.max_steps * 8, true));
        CHK(dev_alloc(h.get(), (void**)&h->codes_bot, B * (size_t)c.max_steps * 4 * 8, true));
        if (c.code_levels == 3) CHK(dev_alloc(h.get(), (void**)&h->codes_l2, B * (size_t)c.max_steps * 16 * 8, true));
        if (!h->parent) {                        // the persistent chain runs on root handles only (persist_on)
            CHK(dev_alloc(h.get(), (void**)&h->persist_counters, PERSIST_COUNTER_BYTES, true));
            CHK(dev_alloc(h.get(), (void**)&h->persist_err, 256, true));
            HIPCHK(hipMemset(h->persist_err, 0, 256));
            CHK(dev_alloc(h.get(), (void**)&h->persist_slabs, persist_slab_floats(256) * 4, true));
        } else {
            h->persist_counters = nullptr; h->persist_err = nullptr; h->persist_slabs = nullptr;
        }
    }
    if (c.has_stage1) {
        std::vector<DecLayer> both(h->dec);                 // decoder and encoder share the activation / attention / statistics buffers
        both.insert(both.end(), h->enc.begin(), h->enc.end());
        size_t per_img = 0;
        for (auto& l : both) {
            const size_t in_e = (size_t)l.res * l.res * (l.kind == 6 ? 16 : l.cin);       // conv_in reads the image padded to <= 16 channels
            const size_t out_r = l.kind == 3 ? 2 * l.res : l.res;
            const size_t out_e = out_r * out_r * (size_t)(l.kind == 4 ? 0 : l.cout);
            per_img = std::max(per_img, std::max(in_e, out_e));
        }
        h->dec_chunk = std::max(1, std::min<int>(c.max_batch, switch_value(SW_DEC_CHUNK)));     // images per decode pass.  Decoder alone 64 -> 128 -> 256: 2047 -> 2090 -> 2102 images/s (SPLIT), but in the pipeline 128 measured 0.4 % slower (1275 vs 1280 images/s, same box)
        h->act_elems = per_img * h->dec_chunk;
        for (int i = 0; i < 3; ++i) CHK(dev_alloc(h.get(), &h->act[i], h->act_elems * 4, true));
        CHK(dev_alloc(h.get(), &h->act[3], h->act_elems * 4, true));     // bf16 copy (FAST) or fp16 hi / lo planes (SPLIT)
        {
            size_t pe = 0;
            for (auto& l : both) if (l.kind != 6) pe = std::max(pe, gn_stats_fast_partial_elems(h->dec_chunk, l.res * l.res, l.cin, 32));
            for (auto& l : both) if (l.kind == 1) pe = std::max(pe, gn_stats_fast_partial_elems(h->dec_chunk, l.res * l.res, l.cout, 32));
            CHK(dev_alloc(h.get(), (void**)&h->gn_partial, pe * sizeof(double), true));
            size_t te = 0;
            for (auto& l : both) { const int ro = l.kind == 3 ? 2 * l.res : l.res; te = std::max(te, (size_t)h->dec_chunk * (ro / 8 + 1) * (ro / 16 + 1) * 64); }
            CHK(dev_alloc(h.get(), (void**)&h->gn_tiles, te * sizeof(double), true));     // floats (FAST) or doubles (SPLIT)
        }
        const int r = h->dec.front().res;
        size_t attn_c = 0;
        for (auto& l : both) if (l.kind == 2) attn_c = std::max(attn_c, (size_t)l.cin * l.res * l.res);
        const size_t hw = (size_t)r * r;
        if (attn_c) {
            CHK(dev_alloc(h.get(), &h->aq, attn_c * h->dec_chunk * 4, true));
            CHK(dev_alloc(h.get(), &h->ak, attn_c * h->dec_chunk * 4, true));
            CHK(dev_alloc(h.get(), &h->av, attn_c * h->dec_chunk * 4, true));
            CHK(dev_alloc(h.get(), &h->ao, attn_c * h->dec_chunk * 4, true));
            size_t smax = 0;
            for (auto& l : both) if (l.kind == 2) smax = std::max(smax, (size_t)l.res * l.res * l.res * l.res);
            CHK(dev_alloc(h.get(), &h->as, smax * h->dec_chunk * 4, true));
        }
        CHK(dev_alloc(h.get(), &h->quant, hw * 2 * c.s1_embed_dim * h->dec_chunk * 4, true));
        CHK(dev_alloc(h.get(), (void**)&h->gn, (size_t)h->dec_chunk * 32 * 2 * 2 * 4, true));
        if (h->has_encoder) CHK(alloc_encode_workspace(h.get()));            // clones of a handle with an encoder
    }
    return HQT_OK;
}

// A second lane over the same weights: several batches in flight on one GPU, one lane + stream each (the AR loop is a
// chain of small latency-bound kernels that leaves most CUs idle; independent chains interleave).  The clone shares
// every weight buffer and derived layout of `src` (which must be finalized and outlive it) and owns a fresh workspace.
extern "C" int hqt_clone(hqt_handle* src, hqt_handle** out) {
    if (!src || !out) return fail(HQT_ERR_INVALID, "null argument");
    if (!src->finalized) return fail(HQT_ERR_STATE, "hqt_clone needs a finalized handle");
    ON_DEVICE(src);
    hqt_handle* root = src->parent ? src->parent : src;
    std::unique_ptr<hqt_handle> h(new hqt_handle(*root));       // weights map, Lin structs and decoder plan by value: same device pointers
    h->owned.clear();
    h->workspace_bytes = 0;
    h->parent = root;
    h->n_clones = 0;
    h->graph_exec = nullptr;
    h->graph_key.clear();
    h->timing = false;
    h->slots.clear();
    h->chain_ev = nullptr;
    h->chain_valid = false;
    h->all_events.clear();
    h->pend = {nullptr, 0, 0, nullptr};
    for (int i = 0; i < hqt_handle::ROWS_RING; ++i) { h->rows_pinned[i] = nullptr; h->rows_ev[i] = nullptr; h->rows_busy[i] = false; }
    h->rows_next = 0;
    h->clear_staged();                           // a lane has its own staged tables, buffer and segment
    h->pg_k = h->pg_v = nullptr; h->pg_x = nullptr; h->pg_cap = 0; h->pg_bytes = 0;      // ... its own prefill staging (hqt_set_prompt_groups on the lane sizes it)
    h->paused = hqt_handle::Paused();            // ... and its own paused pass
    h->rolling = hqt_handle::Rolling();          // ... and its own rolling pass
    h->nparts = h->npartsd = 0;
    h->pbody.d_phases = nullptr; h->pfull.d_phases = nullptr;      // phase tables hold workspace pointers: bound per handle (persist_bind)
    h->persist_used = false; h->persist_tripped = false; h->capture_persist = false; h->graph_has_persist = false;
    h->policy = HQT_POLICY_LATENCY;              // a lane's tile choice never depends on what the root ran when it was cloned
    int rc = alloc_workspace(h.get());
    // (hqt_set_max_joins / hqt_set_join_run on the root: the lane joins as many rows over as long a run, in a staging of its own; without text and a run there is none)
    if (rc == HQT_OK && h->max_joins > 0 && (h->cfg.cond_type == HQT_COND_TEXT || h->join_run > 0))
        rc = reserve_prompt_staging(h.get(), h->max_joins, h->staging_rows(std::max(h->join_run, 0)));
    if (rc != HQT_OK) { for (void* p : h->owned) hipFree(p); return rc; }
    root->n_clones++;
    *out = h.release();
    return HQT_OK;
}

extern "C" int hqt_destroy(hqt_handle* h) {
    if (!h) return HQT_OK;
    if (h->n_clones > 0) return fail(HQT_ERR_STATE, "%d clone(s) of this handle are still alive", h->n_clones);
    DeviceGuard dg(h->device);
    hipDeviceSynchronize();
    if (h->graph_exec) hipGraphExecDestroy(h->graph_exec);
    timing_collect(h);
    for (void* p : h->owned) hipFree(p);             // a clone owns only its workspace
    for (int i = 0; i < hqt_handle::ROWS_RING; ++i) {
        if (h->rows_pinned[i]) hipHostFree(h->rows_pinned[i]);
        if (h->rows_ev[i]) hipEventDestroy(h->rows_ev[i]);
    }
    if (h->parent) h->parent->n_clones--;
    delete h;
    return HQT_OK;
}

// ------------------------------------------------------------------------------------------ weights
extern "C" int hqt_set_weight(hqt_handle* h, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape || ndim < 1 || ndim > 4) return fail(HQT_ERR_INVALID, "bad argument");
    if (dtype != HQT_DTYPE_F32) return fail(HQT_ERR_INVALID, "only fp32 weights are accepted");
    if (h->finalized) return fail(HQT_ERR_STATE, "weights already finalized");
    ON_DEVICE(h);
    Tensor t;
    t.n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.n *= (size_t)shape[i]; }
    auto it = h->w.find(name);
    if (it != h->w.end()) {
        if (it->second.n != t.n) return fail(HQT_ERR_SHAPE, "%s: re-set with a different size", name);
        t.d = it->second.d;
    } else {
        CHK(dev_alloc(h, (void**)&t.d, t.n * 4, false));
        const int stage = strncmp(name, "stage1.", 7) == 0 ? 1 : 2;
        h->params[stage] += (int64_t)t.n;
    }
    HIPCHK(hipMemcpy(t.d, data, t.n * 4, hipMemcpyDefault));
    h->w[name] = t;
    return HQT_OK;
}

static int get_w(hqt_handle* h, const std::string& name, std::vector<int64_t> shape, const float** out) {
    auto it = h->w.find(name);
    if (it == h->w.end()) return fail(HQT_ERR_MISSING_WEIGHT, "missing weight '%s'", name.c_str());
    if (it->second.shape != shape) {
        std::string got, want;
        for (auto v : it->second.shape) got += std::to_string(v) + ",";
        for (auto v : shape) want += std::to_string(v) + ",";
        return fail(HQT_ERR_SHAPE, "weight '%s' has shape [%s] expected [%s]", name.c_str(), got.c_str(), want.c_str());
    }
    *out = it->second.d;
    return HQT_OK;
}

static int make_lin(hqt_handle* h, Lin& l, const float* w32, const float* b32, int N, int K, bool stream_pack, bool split_planes = false) {
    l.w32 = w32; l.b32 = b32; l.N = N; l.K = K;
    if (!stream_pack || (h->layouts & HQT_LAYOUT_FAST)) {
        CHK(dev_alloc(h, (void**)&l.w16, (size_t)N * K * 2, false));
        HIPCHK(launch_f32_to_bf16(w32, l.w16, (size_t)N * K, 0));
    }
    // the AR loop's nn.Linear weights (stream_pack) build only the layouts the handle was created for (hqt_config.ar_layouts)
    const bool ar = stream_pack;
    if (split_planes && (!ar || (h->layouts & HQT_LAYOUT_SPLIT))) {
        CHK(dev_alloc(h, (void**)&l.w16h, (size_t)N * K * 2, false));
        CHK(dev_alloc(h, (void**)&l.w16l, (size_t)N * K * 2, false));
        HIPCHK(launch_split_f32(w32, l.w16h, l.w16l, (size_t)N * K, 0));
    }
    if (stream_pack && (h->layouts & HQT_LAYOUT_EXACT) && N % 16 == 0 && K % 32 == 0) {          // the AR loop's linears: tile-contiguous fp32 for the EXACT small-row GEMM
        CHK(dev_alloc(h, (void**)&l.w32t, (size_t)N * K * 4, false));
        HIPCHK(launch_pack_exact_tiles(w32, l.w32t, N, K, 0));
    }
    if (stream_pack && (h->layouts & HQT_LAYOUT_FAST) && stream_gemm_supported(N, K)) {
        CHK(dev_alloc(h, (void**)&l.wpk, (size_t)N * K * 2, false));
        HIPCHK(launch_pack_stream_weights(w32, l.wpk, N, K, 0));
    }
    return HQT_OK;
}

// deferred LayerNorm: fold (gamma, beta) of the LayerNorm in front of `l` into a second packed copy of its weights
static int fold_ln(hqt_handle* h, Lin& l, const float* gamma, const float* beta) {
    if (!l.wpk) return HQT_OK;
    CHK(dev_alloc(h, (void**)&l.wpk_ln, (size_t)l.N * l.K * 2, false));
    CHK(dev_alloc(h, (void**)&l.colsum, (size_t)l.N * 4, false));
    CHK(dev_alloc(h, (void**)&l.bias_ln, (size_t)l.N * 4, false));
    HIPCHK(launch_fold_layernorm(l.w32, gamma, beta, l.b32, h->fold_tmp, l.wpk_ln, l.colsum, l.bias_ln, l.N, l.K, 0));
    return HQT_OK;
}

static int load_block(hqt_handle* h, const std::string& p, BlockW& b) {
    const int64_t D = h->cfg.embed_dim;
    CHK(get_w(h, p + ".ln1.weight", {D}, &b.ln1_g));
    CHK(get_w(h, p + ".ln1.bias", {D}, &b.ln1_b));
    CHK(get_w(h, p + ".ln2.weight", {D}, &b.ln2_g));
    CHK(get_w(h, p + ".ln2.bias", {D}, &b.ln2_b));
    const float *wq, *wk, *wv, *bq, *bk, *bv, *w, *bias;
    CHK(get_w(h, p + ".attn.query.weight", {D, D}, &wq));
    CHK(get_w(h, p + ".attn.key.weight", {D, D}, &wk));
    CHK(get_w(h, p + ".attn.value.weight", {D, D}, &wv));
    CHK(get_w(h, p + ".attn.query.bias", {D}, &bq));
    CHK(get_w(h, p + ".attn.key.bias", {D}, &bk));
    CHK(get_w(h, p + ".attn.value.bias", {D}, &bv));
    float *wqkv, *bqkv;                       // fused [query; key; value] rows
    CHK(dev_alloc(h, (void**)&wqkv, (size_t)3 * D * D * 4, false));
    CHK(dev_alloc(h, (void**)&bqkv, (size_t)3 * D * 4, false));
    HIPCHK(hipMemcpy(wqkv, wq, D * D * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(wqkv + D * D, wk, D * D * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(wqkv + 2 * D * D, wv, D * D * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(bqkv, bq, D * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(bqkv + D, bk, D * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(bqkv + 2 * D, bv, D * 4, hipMemcpyDeviceToDevice));
    CHK(make_lin(h, b.qkv, wqkv, bqkv, 3 * D, D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
    CHK(get_w(h, p + ".attn.proj.weight", {D, D}, &w));
    CHK(get_w(h, p + ".attn.proj.bias", {D}, &bias));
    CHK(make_lin(h, b.proj, w, bias, D, D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
    CHK(get_w(h, p + ".mlp.0.weight", {4 * D, D}, &w));
    CHK(get_w(h, p + ".mlp.0.bias", {4 * D}, &bias));
    CHK(make_lin(h, b.fc1, w, bias, 4 * D, D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
    CHK(get_w(h, p + ".mlp.2.weight", {D, 4 * D}, &w));
    CHK(get_w(h, p + ".mlp.2.bias", {D}, &bias));
    CHK(make_lin(h, b.fc2, w, bias, D, 4 * D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
    CHK(fold_ln(h, b.qkv, b.ln1_g, b.ln1_b));
    CHK(fold_ln(h, b.fc1, b.ln2_g, b.ln2_b));
    return HQT_OK;
}

static int load_conv(hqt_handle* h, const std::string& name, int O, int I, int ksz, Lin& l, bool upsampling = false) {
    const float *w, *b;
    CHK(get_w(h, "stage1." + name + ".weight", {O, I, ksz, ksz}, &w));
    CHK(get_w(h, "stage1." + name + ".bias", {O}, &b));
    const int taps = ksz * ksz;
    float* wt = const_cast<float*>(w);
    if (taps > 1) {                          // [O][I][kh][kw] -> tap-major [O][kh*kw][I] (k = tap * I + i)
        CHK(dev_alloc(h, (void**)&wt, (size_t)O * I * taps * 4, false));
        HIPCHK(launch_repack_conv(w, wt, O, I, taps, 0));
    }
    CHK(make_lin(h, l, wt, b, O, I * taps, false, true));
    if (taps == 9 && I % 32 == 0) {              // fragment-packed copies for the ring kernels (whole 128-channel tiles; conv_out: one 16-channel block)
        if (O % 128 == 0 || O <= 16) {
            CHK(dev_alloc(h, (void**)&l.wfrag16, split_frag_elems(O, I) * sizeof(half_t), false));
            HIPCHK(launch_pack_split_frag16(wt, l.wfrag16, O, I, 0));
        }
        if (upsampling && O % 128 == 0 && I % 64 == 0) {      // nearest x2 + 3x3 = four 2x2 phase convs on the low-resolution image
            CHK(dev_alloc(h, (void**)&l.wup16, split_up_elems(O, I) * sizeof(half_t), false));
            HIPCHK(hipMemset(l.wup16, 0, split_up_elems(O, I) * sizeof(half_t)));
            HIPCHK(launch_pack_split_up16(wt, l.wup16, O, I, 0));
        }
    }
    return HQT_OK;
}

// the image enters conv_in as NHWC with its 3 channels zero-padded: 4 for the 4x4 stride-2 filter (K = 64), 16 for the 3x3 one (K = 144)
static int conv_in_cpad(const hqt_config& c) { return c.s1_use_init_downsample ? 4 : 16; }

// Encoder + quant_conv_b + the codebooks as distance-GEMM operands (hqt_encode).  All-or-nothing: called when
// stage1.encoder.conv_in.weight was set; any other missing encoder tensor is an error.
static int load_encoder(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    for (auto& l : h->enc) {
        if (l.kind == 6) {
            const int ks = c.s1_use_init_downsample ? 4 : 3, taps = ks * ks, cp = conv_in_cpad(c);
            const float *w, *b;
            CHK(get_w(h, "stage1.encoder.conv_in.weight", {l.cout, 3, ks, ks}, &w));
            CHK(get_w(h, "stage1.encoder.conv_in.bias", {l.cout}, &b));
            float* wt;
            CHK(dev_alloc(h, (void**)&wt, (size_t)l.cout * cp * taps * 4, false));
            HIPCHK(launch_repack_conv(w, wt, l.cout, 3, taps, 0, cp));
            CHK(make_lin(h, l.conv1, wt, b, l.cout, cp * taps, false));
        } else if (l.kind == 5) {
            CHK(load_conv(h, l.name, l.cout, l.cin, 3, l.conv1));
        } else if (l.kind == 1) {
            CHK(get_w(h, "stage1." + l.name + ".norm1.weight", {l.cin}, &l.n1_g));
            CHK(get_w(h, "stage1." + l.name + ".norm1.bias", {l.cin}, &l.n1_b));
            CHK(get_w(h, "stage1." + l.name + ".norm2.weight", {l.cout}, &l.n2_g));
            CHK(get_w(h, "stage1." + l.name + ".norm2.bias", {l.cout}, &l.n2_b));
            CHK(load_conv(h, l.name + ".conv1", l.cout, l.cin, 3, l.conv1));
            CHK(load_conv(h, l.name + ".conv2", l.cout, l.cout, 3, l.conv2));
            if (l.cin != l.cout) CHK(load_conv(h, l.name + ".nin_shortcut", l.cout, l.cin, 1, l.nin));
        } else if (l.kind == 2) {
            CHK(get_w(h, "stage1." + l.name + ".norm.weight", {l.cin}, &l.n1_g));
            CHK(get_w(h, "stage1." + l.name + ".norm.bias", {l.cin}, &l.n1_b));
            CHK(load_conv(h, l.name + ".q", l.cin, l.cin, 1, l.q));
            CHK(load_conv(h, l.name + ".k", l.cin, l.cin, 1, l.k));
            CHK(load_conv(h, l.name + ".v", l.cin, l.cin, 1, l.v));
            CHK(load_conv(h, l.name + ".proj_out", l.cin, l.cin, 1, l.proj));
        } else {
            CHK(get_w(h, "stage1.encoder.norm_out.weight", {l.cin}, &l.n1_g));
            CHK(get_w(h, "stage1.encoder.norm_out.bias", {l.cin}, &l.n1_b));
            CHK(load_conv(h, "encoder.conv_out", l.cout, l.cin, 3, l.conv1));
        }
    }
    const int E = c.s1_embed_dim, L = c.code_levels == 3 ? 3 : 2;
    CHK(load_conv(h, "quant_conv_b", E, c.s1_z_channels, 1, h->quant_conv));
    if (c.s1_resample == HQT_RESAMPLE_CONV2) {     // Conv2d(E, E, 2, stride 2): [co][ci][a][b] is already the Linear [E, 4E] over pixel-unshuffled rows (k = ci * 4 + 2 a + b)
        const float *w, *b;
        CHK(get_w(h, "stage1.down_t.weight", {E, E, 2, 2}, &w));
        CHK(get_w(h, "stage1.down_t.bias", {E}, &b));
        h->down_lin = Lin();
        h->down_lin.w32 = w; h->down_lin.b32 = b; h->down_lin.N = E; h->down_lin.K = 4 * E;
    }
    for (int l = 0; l < L; ++l) {
        const int dim = c.s1_resample ? E : E << (2 * (L - 1 - l));
        const std::string name = L == 3 ? "stage1.quantizers." + std::to_string(l) + ".embedding"
                                        : (l == 0 ? "stage1.quantize_t.embedding" : "stage1.quantize_b.embedding");
        const float* e = h->w[name].d;
        CHK(dev_alloc(h, (void**)&h->cb_norm[l], (size_t)c.s1_n_embed * 4, false));
        HIPCHK(launch_row_sumsq(e, DT_F32, h->cb_norm[l], c.s1_n_embed, dim, 0));
    }
    h->has_encoder = true;
    return alloc_encode_workspace(h);
}

static std::string key2(const hqt_handle* h, const char* name);

static int finalize_impl(hqt_handle* h);
static int persist_build(hqt_handle* h);
extern "C" int hqt_finalize_weights(hqt_handle* h) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    if (h->finalized) return HQT_OK;
    DeviceGuard dg(h->device);
    if (!dg.ok) return fail(HQT_ERR_HIP, "hipSetDevice(%d) failed", h->device);
    // all or nothing: on failure every derived buffer allocated by this attempt is released and the derived state cleared, so a
    // retry (after the missing tensor was set) starts clean instead of re-allocating on top of half-built layouts
    const size_t owned_before = h->owned.size();
    const int rc = finalize_impl(h);
    if (h->fold_tmp) { hipFree(h->fold_tmp); h->fold_tmp = nullptr; }
    if (rc != HQT_OK) {
        hipDeviceSynchronize();
        for (size_t i = owned_before; i < h->owned.size(); ++i) hipFree(h->owned[i]);
        h->owned.resize(owned_before);
        h->body.clear(); h->depth.clear();
        h->pbody = PersistProg(); h->pfull = PersistProg();
        h->head_top = h->head_bot = h->head_l2 = h->post_quant = h->quant_conv = Lin();
        for (auto& l : h->dec) { l.conv1 = l.conv2 = l.nin = l.q = l.k = l.v = l.proj = Lin(); }
        for (auto& l : h->enc) { l.conv1 = l.conv2 = l.nin = l.q = l.k = l.v = l.proj = Lin(); }
        for (auto& p : h->cb_norm) p = nullptr;
        h->vq_h = h->vq_recon = h->vq_zz = h->vq_err = nullptr; h->vq_z = nullptr; h->vq_best = nullptr;
        h->vq_t = h->vq_q = nullptr; h->up_table = nullptr; h->up_lin = h->down_lin = Lin();
        h->has_encoder = false;
    }
    return rc;
}
static int finalize_impl(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    if (c.has_stage2) {
        HIPCHK(hipMalloc((void**)&h->fold_tmp, (size_t)std::max(4 * c.embed_dim, c.vocab_top) * c.embed_dim * 4));
        h->body.resize(c.n_layers);
        h->depth.resize(c.n_layers_depth);
        for (int i = 0; i < c.n_layers; ++i) { CHK(load_block(h, "stage2.blocks." + std::to_string(i), h->body[i])); h->body[i].body = true; }
        for (int i = 0; i < c.n_layers_depth; ++i) CHK(load_block(h, "stage2.depths." + std::to_string(i), h->depth[i]));
        const float* w;
        const int64_t D = c.embed_dim;
        const bool l3 = c.code_levels == 3;
        CHK(get_w(h, key2(h, "head_top.weight"), {c.vocab_top, D}, &w));
        CHK(make_lin(h, h->head_top, w, nullptr, c.vocab_top, D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
        CHK(get_w(h, key2(h, "head_bot.weight"), {c.vocab_bot, D}, &w));
        CHK(make_lin(h, h->head_bot, w, nullptr, c.vocab_bot, D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
        if (l3) {
            CHK(get_w(h, "stage2.head_levels.2.weight", {c.vocab_top, D}, &w));
            CHK(make_lin(h, h->head_l2, w, nullptr, c.vocab_top, D, true, true));      // + fp16 hi / lo planes: the SPLIT AR loop
        }
        // presence/shape checks of the remaining tensors happen here so that sample() cannot fail late
        const float* t;
        CHK(get_w(h, "stage2.ln_f.weight", {D}, &t)); CHK(get_w(h, "stage2.ln_f.bias", {D}, &t));
        CHK(get_w(h, key2(h, "ln_top.weight"), {D}, &t)); CHK(get_w(h, key2(h, "ln_top.bias"), {D}, &t));
        CHK(get_w(h, key2(h, "ln_bot.weight"), {D}, &t)); CHK(get_w(h, key2(h, "ln_bot.bias"), {D}, &t));
        CHK(get_w(h, "stage2.sos_depth", {1, 1, D}, &t));
        CHK(get_w(h, key2(h, "tok_emb_top.weight"), {c.vocab_top, D}, &t));
        CHK(get_w(h, key2(h, "tok_emb_bot.weight"), {c.vocab_bot, c.embedding_type == HQT_EMB_REDUCE ? D / 4 : D}, &t));
        if (c.embedding_type == HQT_EMB_TRANSFORMER1) CHK(get_w(h, "stage2.pos_emb_emb.weight", {l3 ? 21 : 5, D}, &t));
        CHK(get_w(h, "stage2.pos_emb_top.weight", {c.ctx_len_img, D}, &t));
        const int dmul = (l3 && c.depth_decoding == HQT_DEPTH_PARALLEL_REDUCE) ? 4 : 1;      // 'reduce': [V, 4 D] depth tables (hqtransformer.py:108-116)
        const bool causal_head = l3 && c.depth_decoding == HQT_DEPTH_TOP2MID2BOT;            // its sub-step inputs come from tok_emb_levels (hqtransformer.py:718-725)
        if (!causal_head) CHK(get_w(h, key2(h, "tok_emb_top_depth.weight"), {c.vocab_top, dmul * D}, &t));
        CHK(get_w(h, key2(h, "pos_emb_depth.weight"), {causal_head ? 21 : (l3 ? 4 : 5), D}, &t));
        if (l3) {
            CHK(get_w(h, "stage2.tok_emb_levels.2.weight", {c.vocab_top, D}, &t));
            if (!causal_head) {
                CHK(get_w(h, "stage2.tok_emb_depth_levels.1.weight", {c.vocab_top, dmul * D}, &t));
                CHK(get_w(h, "stage2.pos_emb_depths.1.weight", {16, D}, &t));
            }
            CHK(get_w(h, "stage2.ln_levels.2.weight", {D}, &t)); CHK(get_w(h, "stage2.ln_levels.2.bias", {D}, &t));
        }
        {
            const float *g1, *b1;
            CHK(get_w(h, key2(h, "ln_top.weight"), {D}, &g1)); CHK(get_w(h, key2(h, "ln_top.bias"), {D}, &b1));
            CHK(fold_ln(h, h->head_top, g1, b1));
            CHK(get_w(h, key2(h, "ln_bot.weight"), {D}, &g1)); CHK(get_w(h, key2(h, "ln_bot.bias"), {D}, &b1));
            CHK(fold_ln(h, h->head_bot, g1, b1));
            if (l3) {
                CHK(get_w(h, "stage2.ln_levels.2.weight", {D}, &g1)); CHK(get_w(h, "stage2.ln_levels.2.bias", {D}, &b1));
                CHK(fold_ln(h, h->head_l2, g1, b1));
            }
            HIPCHK(hipDeviceSynchronize());          // fold_tmp is released by hqt_finalize_weights on every exit
        }
        CHK(persist_build(h));                       // weight streams of the persistent AR chain (FAST, up to 64 rows)
        if (c.cond_type == HQT_COND_CLASS) CHK(get_w(h, "stage2.sos.weight", {c.n_classes, D}, &t));
        else if (c.cond_type == HQT_COND_TEXT) {
            CHK(get_w(h, "stage2.tok_emb_txt.weight", {c.vocab_txt, D}, &t));
            CHK(get_w(h, "stage2.pos_emb_txt.weight", {c.ctx_len_txt, D}, &t));
        } else CHK(get_w(h, "stage2.sos", {1, 1, D}, &t));
    }
    if (c.has_stage1) {
        const int E = c.s1_embed_dim;
        const float* t;
        if (c.code_levels == 3) {                // HQVAEGenerator: additive pyramid, E channels into the 1x1 conv
            CHK(get_w(h, "stage1.quantizers.0.embedding", {c.s1_n_embed, 16 * E}, &t));
            CHK(get_w(h, "stage1.quantizers.1.embedding", {c.s1_n_embed, 4 * E}, &t));
            CHK(get_w(h, "stage1.quantizers.2.embedding", {c.s1_n_embed, E}, &t));
            CHK(load_conv(h, "post_quant_conv_b", c.s1_z_channels, E, 1, h->post_quant));
        } else {
            CHK(get_w(h, "stage1.quantize_t.embedding", {c.s1_n_embed, c.s1_resample ? E : 4 * E}, &t));      // generator.py:214,231,242
            if (c.s1_resample == HQT_RESAMPLE_CONV2) {
                const float *uw, *ub;
                CHK(get_w(h, "stage1.upsample_t.weight", {E, E, 2, 2}, &uw));
                CHK(get_w(h, "stage1.upsample_t.bias", {E}, &ub));
                // decode: q_t is always a codebook row, so the transposed conv folds into a table the size of the pixelshuffle top codebook
                CHK(dev_alloc(h, (void**)&h->up_table, (size_t)c.s1_n_embed * 4 * E * 4, false));
                HIPCHK(launch_fold_upsample_t(t, uw, ub, h->up_table, c.s1_n_embed, E, 0));
                // encode: the straight-through rows are not codebook rows; there the transposed conv is a Linear [4E, E] + bias
                float *wt, *b4;
                CHK(dev_alloc(h, (void**)&wt, (size_t)4 * E * E * 4, false));
                CHK(dev_alloc(h, (void**)&b4, (size_t)4 * E * 4, false));
                HIPCHK(launch_repack_upsample_t(uw, ub, wt, b4, E, 0));
                h->up_lin = Lin();
                h->up_lin.w32 = wt; h->up_lin.b32 = b4; h->up_lin.N = 4 * E; h->up_lin.K = E;
            }
            CHK(get_w(h, "stage1.quantize_b.embedding", {c.s1_n_embed, E}, &t));
            CHK(load_conv(h, "post_quant_conv_b", c.s1_z_channels, 2 * E, 1, h->post_quant));
        }
        for (auto& l : h->dec) {
            if (l.kind == 0 || l.kind == 3) CHK(load_conv(h, l.name, l.cout, l.cin, 3, l.conv1, l.kind == 3));
            else if (l.kind == 1) {
                CHK(get_w(h, "stage1." + l.name + ".norm1.weight", {l.cin}, &l.n1_g));
                CHK(get_w(h, "stage1." + l.name + ".norm1.bias", {l.cin}, &l.n1_b));
                CHK(get_w(h, "stage1." + l.name + ".norm2.weight", {l.cout}, &l.n2_g));
                CHK(get_w(h, "stage1." + l.name + ".norm2.bias", {l.cout}, &l.n2_b));
                CHK(load_conv(h, l.name + ".conv1", l.cout, l.cin, 3, l.conv1));
                CHK(load_conv(h, l.name + ".conv2", l.cout, l.cout, 3, l.conv2));
                if (l.cin != l.cout) CHK(load_conv(h, l.name + ".nin_shortcut", l.cout, l.cin, 1, l.nin));
            } else if (l.kind == 2) {
                CHK(get_w(h, "stage1." + l.name + ".norm.weight", {l.cin}, &l.n1_g));
                CHK(get_w(h, "stage1." + l.name + ".norm.bias", {l.cin}, &l.n1_b));
                CHK(load_conv(h, l.name + ".q", l.cin, l.cin, 1, l.q));
                CHK(load_conv(h, l.name + ".k", l.cin, l.cin, 1, l.k));
                CHK(load_conv(h, l.name + ".v", l.cin, l.cin, 1, l.v));
                CHK(load_conv(h, l.name + ".proj_out", l.cin, l.cin, 1, l.proj));
            } else {
                CHK(get_w(h, "stage1.decoder.norm_out.weight", {l.cin}, &l.n1_g));
                CHK(get_w(h, "stage1.decoder.norm_out.bias", {l.cin}, &l.n1_b));
                CHK(load_conv(h, "decoder.conv_out", l.cout, l.cin, 3, l.conv1));
            }
        }
    }
    // the encode side is optional as a whole: the encoder tensors and, for conv2, down_t (decode needs neither)
    if (c.has_stage1 && h->w.count("stage1.encoder.conv_in.weight") && (c.s1_resample != HQT_RESAMPLE_CONV2 || h->w.count("stage1.down_t.weight")))
        CHK(load_encoder(h));
    HIPCHK(stream_gemm_configure());
    HIPCHK(tile_gemm_configure());
    HIPCHK(mfma_gemm_configure());
    HIPCHK(split_kernels_configure());
    HIPCHK(hipDeviceSynchronize());
    h->finalized = true;
    return HQT_OK;
}

// ------------------------------------------------------------------------------------------ GEMM dispatch
struct Mode {
    bool fast = false;
    bool split = false;     // stage 1: fp32 tensors, convolutions on the matrix cores with fp16 hi / lo operands (split_kernels.h)
    bool split_ar = false;  // stage 2 (hqt_sample / hqt_sample_l3): the EXACT launch sequence -- fp32 activations, LayerNorm, attention, sampler -- with
                            // every nn.Linear on the matrix cores: fp32 activation rows split into fp16 hi / lo while their tile is staged, the weights as
                            // fp16 hi / lo planes, three MFMAs per product term, fp32 accumulation (split_gemm_kernel<fp32 A>)
    int act_dt() const { return fast ? DT_BF16 : DT_F32; }
    size_t act_sz() const { return fast ? 2 : 4; }
};
static int mode_of(int precision, bool stage1, Mode* md) {
    if (precision == HQT_PRECISION_FAST) md->fast = true;
    else if (precision == HQT_PRECISION_SPLIT && stage1) md->split = true;
    else if (precision == HQT_PRECISION_SPLIT) md->split_ar = true;
    else if (precision != HQT_PRECISION_EXACT) return fail(HQT_ERR_INVALID, "unknown precision %d", precision);
    return HQT_OK;
}

// What every launch of filter bank `l` takes from it and from the handle (both dispatchers, and the shape probes of stage 1);
// split_planes: the filters are the fp16 hi / lo planes (and their fragment-packed copies) of the SPLIT kernels
static void lin_args(const hqt_handle* h, GemmArgs& g, const Lin& l, bool split_planes) {
    g.N = l.N; g.K = l.K; g.ldb = l.K;
    g.bias = l.b32;
    g.zero_page = h->zero_page;
    g.tune = h->policy;
    if (g.alpha == 0.0f) g.alpha = 1.0f;
    if (g.lda == 0) g.lda = l.K;
    if (split_planes) { g.Bw = l.w16h; g.Bw_lo = l.w16l; g.Bw_frag16 = l.wfrag16; g.Bw_up16 = l.wup16; }
}

// Timing slot of a dispatched launch: `tag`, or `tag@rows` under HQT_TIMING_BY_ROWS (tools/ar_pass_time.py --by-rows: one slot per
// (GEMM, row count) instead of per GEMM)
struct SlotName {
    char s[64];
    SlotName(const char* tag, int rows) {
        const bool by_rows = switch_value(SW_TIMING_BY_ROWS);
        snprintf(s, sizeof s, by_rows ? "%s@%d" : "%s", tag, rows);
    }
};

// Stage 2, y = x W^T (+b)(act)(+resid) of one nn.Linear of the AR loop.  FAST: the LDS-tiled, the weight-streaming or the plain MFMA kernel;
// SPLIT: fp16 hi / lo planes above 256 rows; otherwise fp32.  defer_residual: a split-K launch may leave its slabs in h->pend for the next
// LayerNorm.  resid_nparts (STORE_RESID launches): the partial row statistics the producer leaves per row.
static int ar_linear(hqt_handle* h, const Mode& md, GemmArgs g, const Lin& l, int a_dt, int c_dt, hipStream_t st,
                     const char* tag, bool defer_residual = false, int* resid_nparts = nullptr) {
    lin_args(h, g, l, false);
    g.k_quarters = 1;                           // every caller is the AR loop: see GemmArgs.k_quarters
    const SlotName slot(tag, g.M);
    Timed t(h, slot.s, st);
    if (md.fast) {
        if (resid_nparts) *resid_nparts = g.N / 32;          // streaming GEMM: one per 32 columns
        // merged passes (512+ rows): the LDS-tiled MFMA kernels (tile_gemm.hip); same operands, same store modes
        if ((g.ln_parts ? l.wpk_ln : l.wpk) && h->tile_gemm && tile_gemm_ok(g, a_dt, c_dt)) {
            const TilePlan tp = tile_gemm_plan(g);
            if (tp.geom >= 0 && (size_t)tp.S * 32 * g.a_packed_mb * g.N <= h->splitk_elems) {
                if (g.ln_parts) g.bias = l.bias_ln;
                HIPCHK(launch_tile_gemm(g, g.ln_parts ? l.wpk_ln : l.wpk, a_dt, c_dt, tp, h->splitk, st));
                if (tp.S > 1) {
                    count_variant(h, "variant:tile_gemm_%dx%d%s_splitk%d:%s", tp.bm, tp.bn, tile_geom_suffix(tp.geom), tp.S, slot.s);
                    t.next(SlotName("gemm_combine", g.M).s);
                    HIPCHK(launch_resid_combine(g, h->splitk, tp.S, st));
                } else count_variant(h, "variant:tile_gemm_%dx%d%s%s:%s", tp.bm, tp.bn, tile_geom_suffix(tp.geom), g.ln_parts ? "_dln" : "", slot.s);
                if (resid_nparts) *resid_nparts = tp.S > 1 ? 1 : g.N / tp.bn;
                return HQT_OK;
            }
        }
        if (g.ln_parts) {                       // deferred LayerNorm: gamma-folded weights, folded bias; stream kernel only
            if (!l.wpk_ln || !stream_gemm_ok(g, a_dt, c_dt)) return fail(HQT_ERR_STATE, "deferred-LayerNorm GEMM without folded weights (%s)", tag);
            g.bias = l.bias_ln;
            HIPCHK(launch_stream_gemm(g, l.wpk_ln, a_dt, c_dt, 1, nullptr, st));
            count_variant(h, "variant:stream_gemm_dln:%s", tag);
            return HQT_OK;
        }
        if (l.wpk && stream_gemm_ok(g, a_dt, c_dt)) {
            int S = (defer_residual && g.store != STORE_RESID) ? stream_gemm_splitk(g) : 1;
            if ((size_t)S * 32 * g.a_packed_mb * g.N > h->splitk_elems) S = 1;
            HIPCHK(launch_stream_gemm(g, l.wpk, a_dt, c_dt, S, h->splitk, st));
            count_variant(h, "variant:stream_gemm:%s", tag);
            if (S > 1) h->pend = {h->splitk, S, 32 * g.a_packed_mb, l.b32};
            return HQT_OK;
        }
        g.Bw = l.w16;
        // no packed layout for this shape (stream_gemm_supported: N, K multiples of 32): the plain MFMA kernel, or the generic one where K % 32 != 0
        if (mfma_gemm_ok(g, a_dt, DT_BF16, c_dt)) {
            HIPCHK(launch_mfma_gemm(g, a_dt, DT_BF16, c_dt, st));
            count_variant(h, "variant:mfma_gemm:%s", tag);
        } else {
            HIPCHK(launch_gemm_generic(g, a_dt, DT_BF16, c_dt, st));
            count_variant(h, "variant:gemm_generic_bf16:%s", tag);
        }
        return HQT_OK;
    }
    // (up to 256 rows the fp32 matrix instructions of exact_gemm.hip are faster than three fp16 MFMAs on 128 x 128 tiles that are mostly padding:
    //  249 vs 483 ms of AR loop per batch-64 step -- SPLIT takes them there, and is bit-identical to EXACT on those launches)
    if (md.split_ar && l.w16h && l.w16l && !g.a_packed_mb && g.M > 256) {
        GemmArgs sg = g;
        lin_args(h, sg, l, true);
        sg.a_f32 = 1; sg.range_flag = h->range_flag;
        if (split_gemm_ok(sg)) {
            // few tiles (fc2 / proj at 640 rows: 60): K slices into the split-K workspace, summed in index order by the combine launch
            const int S = h->split_kslices ? split_gemm_slices(sg) : 1;
            if (S > 1 && (size_t)S * sg.M * sg.N <= h->splitk_elems) { sg.k_slices = S; sg.k_slabs = h->splitk; }
            HIPCHK(launch_split_gemm(sg, st));
            if (sg.k_slices > 1) count_variant(h, "variant:split_gemm_kslices%d:%s", sg.k_slices, tag);
            else count_variant(h, "variant:split_gemm:%s", tag);
            return HQT_OK;
        }
    }
    g.Bw = l.w32;
    if (exact_mfma_ok(g)) {                      // the fp32 matrix instructions, one tile per wave
        if (l.w32t && g.N % 16 == 0) { g.Bw = l.w32t; g.b_tile16 = 1; }
        HIPCHK(launch_exact_mfma_gemm(g, st));
        count_variant(h, "variant:exact_mfma:%s", tag);
        return HQT_OK;
    }
    HIPCHK(launch_gemm_generic(g, DT_F32, DT_F32, DT_F32, st));
    count_variant(h, "variant:gemm_generic_f32:%s", tag);
    return HQT_OK;
}

// ------------------------------------------------------------------------------------------ stage 2
static const int LEVEL_WIDTH[3] = {1, 4, 16};    // codes per position of each code level
struct SamplerSet { float temperature = 1.f; int top_k = 0; float top_p = 0.f; };   // one code level's sampler settings
struct SampleCtx {
    int B;
    const int64_t* cond;
    int levels;                                  // code levels: 2 (hqt_sample) or 3 (hqt_sample_l3)
    int precision, n_steps, use_graph;
    uint64_t seed;
    int64_t sample_offset;
    const uint64_t* row_seeds;
    const int64_t* row_offsets;
    SamplerSet lv[3];
    const hqt_row_sampler* row_set = nullptr;    // host table of B rows staged by hqt_set_row_samplers: in place of lv[] (which then holds defaults)
    bool top_p = false, row_top_p = false;       // some level (or row of the table) uses top-p; row_top_p: and it is a row of the table
    const float* noise;
    const int64_t* feed[3] = {nullptr, nullptr, nullptr};   // codes each level's embeddings read: the drawn ones (out) or the forced ones
    int64_t* out[3] = {nullptr, nullptr, nullptr};
    int prefix_len = 0;                          // hqt_sample_prefix: positions [0, prefix_len) are given ...
    const int64_t* prefix[3] = {nullptr, nullptr, nullptr};   // ... as [B, prefix_len], [B, prefix_len, 4][, [B, prefix_len, 16]]
    bool with_prefix = false;                    // the call came through a prefix entry point (prefix_len is then validated)
    float* logits_out;
    float* logprob_out = nullptr;                // hqt_set_logprob_out: [B, n_steps, draws], NULL: no code_logprob launches at all
    ReportOut report = {nullptr, nullptr, 0, nullptr, nullptr};   // hqt_set_draw_report: nothing to write: no draw_report launches at all; with something, they take code_logprob's place
    const hqt_guide_pair* guide = nullptr;       // host table of n_guide pairs staged by hqt_set_guidance, NULL: no guide_logits launches at all
    int n_guide = 0;
    const uint8_t* keep = nullptr;               // host mask [B, n_steps] staged by hqt_set_keep_mask, NULL: every position is drawn (and nothing below is read)
    const int64_t* keep_codes[3] = {nullptr, nullptr, nullptr};   // its codes per level, device, [B, n_steps(, 4 | 16)]
    const int32_t* groups = nullptr;             // host table [B] staged by hqt_set_prompt_groups, NULL: every row prefills its own prompt (and cond is [B, T])
    int n_groups = 0;                            // with a table: cond is [n_groups, T]
    bool seg = false;                            // hqt_set_segment staged a segment: the call runs positions [start, stop) of its n_steps ...
    int start = 0, stop = 0;                     // ... (without one: 0 and n_steps); start > 0 continues the handle's paused pass
    const int32_t* roll = nullptr;               // host table [B] staged by hqt_set_row_positions, NULL: every row stands at the step state's position
    int roll_k = 0;                              // ... and the steps the call runs (it then is positions [0, roll_k) of the launch loop: start = 0, stop = roll_k)
    const int* row_pos = nullptr;                // ... and its device copy (h->row_pos) that the launches of a rolling call read, NULL otherwise
    const int64_t* roll_prev[3] = {nullptr, nullptr, nullptr};   // ... and the caller's out_*: where the codes of position pos[b] - 1 of every continued row are read
    int n_join = 0;                              // ... where a join phase runs (a text handle; a kept run to prefill): the rows with roll[b] == 0, which it draws position join_len for in front of the steps
    int join_len = 0;                            // ... and the leading kept run those rows share and prefill there (0 without a keep table)
    hipStream_t st;
    Mode md;
};

// a text handle that has not opted in (hqt_set_max_joins): the sentence the rolling entry points have always refused it with, and where to go
static const char ROLLING_TEXT_REFUSAL[] =
    "hqt_set_row_positions: a rolling pass on a text-conditional handle is not built (a row that joins at position 0 needs a prompt prefill of its own)"
    " unless the handle has sized one: hqt_set_max_joins(h, J > 0) allocates the staging for J joining rows per call";

// What a rolling call leaves of the position a row presented (-1: an empty slot): where the slot stands behind it, -1 once its last position is drawn.  A row
// that joins (position 0) through a join phase (`join_phase`: a text handle, or a kept run of join_len > 0 to prefill) is moved on by the phase, which covers
// positions [0, join_len], AND by the k steps: join_len + 1 + k.  The handle's record, what the next call must present and the copy-out all follow this rule.
static int rolled_to(int pos, int k, int n, bool join_phase, int join_len) {
    if (pos < 0) return -1;
    const int next = pos + k + (join_phase && pos == 0 ? join_len + 1 : 0);
    return next < n ? next : -1;
}

// State-dict key of a stage-2 tensor: the code below names tensors as iHQGPT does; the three-level HQTransformer keeps
// the same roles under indexed names (hqtransformer.py:24-205).
static std::string key2(const hqt_handle* h, const char* name) {
    std::string n(name);
    if (h->cfg.code_levels == 3) {
        static const char* const tr[][2] = {
            {"tok_emb_top.weight", "tok_emb_levels.0.weight"}, {"tok_emb_bot.weight", "tok_emb_levels.1.weight"},
            {"tok_emb_top_depth.weight", "tok_emb_depth_levels.0.weight"}, {"pos_emb_depth.weight", "pos_emb_depths.0.weight"},
            {"ln_top.weight", "ln_levels.0.weight"}, {"ln_top.bias", "ln_levels.0.bias"},
            {"ln_bot.weight", "ln_levels.1.weight"}, {"ln_bot.bias", "ln_levels.1.bias"},
            {"head_top.weight", "head_levels.0.weight"}, {"head_bot.weight", "head_levels.1.weight"}};
        for (auto& t : tr) if (n == t[0]) { n = t[1]; break; }
    }
    return "stage2." + n;
}
static const float* W(hqt_handle* h, const char* name) { return h->w[key2(h, name)].d; }


// ------------------------------------------------------------------------------------------ persistent AR chain (persist.h)
// FAST precision, up to 64 rows, decode steps (one token per sample), root handle under the latency policy: the twelve body blocks of a top
// position, ln_f + sos_depth, depth sub-step 0 (single-key blocks) and head_top run as ONE launch (three code levels: the body).  Everything else -- merged passes, lanes,
// EXACT / SPLIT, the text prefill, depth sub-step 1 (256 rows: MI355X_MICROARCH.md's verdict for 256-row blocks is "cut at every seam") --
// keeps the launch chain.  HQT_PERSIST=0 switches it off (A/B).
struct PackSrc { const float* w; const float* gamma; };

static void persist_block_shapes(hqt_handle* h, const BlockW& bw, bool single_key, int cache_T, int* k4, std::vector<PersistPhase>& out, std::vector<PackSrc>& src) {
    const int D = h->cfg.embed_dim;
    PersistPhase ph{};
    if (single_key) {        // depth sub-step 0: one query over one key -- the attention output IS the value row (run_block); only [key; value] is computed
        ph.type = PP_KV1; ph.N = 2 * D; ph.K = D; ph.dln = 1; ph.cache_T = cache_T; ph.kv_row = 0;
        out.push_back(ph); src.push_back({bw.qkv.w32 + (size_t)D * D, bw.ln1_g});
    } else {
        ph.type = PP_QKV; ph.N = 3 * D; ph.K = D; ph.dln = 1; ph.cache_T = cache_T;
        out.push_back(ph); src.push_back({bw.qkv.w32, bw.ln1_g});
        ph = PersistPhase{}; ph.type = PP_ATTN; ph.cache_T = cache_T;
        out.push_back(ph); src.push_back({nullptr, nullptr});
    }
    ph = PersistPhase{}; ph.type = PP_RESID; ph.map = PP_MAP_QUAD; ph.N = D; ph.K = D;
    out.push_back(ph); src.push_back({bw.proj.w32, nullptr});
    ph = PersistPhase{}; ph.type = PP_GELU; ph.N = 4 * D; ph.K = D; ph.dln = 1; ph.act = h->cfg.gelu_approx ? ACT_GELU_SIGMOID : ACT_GELU_ERF;
    out.push_back(ph); src.push_back({bw.fc1.w32, bw.ln2_g});
    ph = PersistPhase{}; ph.type = PP_RESID_K4; ph.map = PP_MAP_K4; ph.N = D; ph.K = 4 * D; ph.k4_epoch = ++*k4;
    out.push_back(ph); src.push_back({bw.fc2.w32, nullptr});
}

static int persist_build_one(hqt_handle* h, PersistProg& pr, const std::vector<PackSrc>& src) {
    const hqt_config& c = h->cfg;
    pr.ok = false;
    if (!persist_program_ok(pr.phases, c.embed_dim, 64, c.n_heads, h->ncu)) return HQT_OK;
    std::vector<unsigned long long> cu_off, tile_off;
    const size_t bytes = persist_layout(pr.phases, h->ncu, cu_off, tile_off);
    CHK(dev_alloc(h, (void**)&pr.stream, bytes + 1024, false));
    CHK(dev_alloc(h, (void**)&pr.d_cu_off, cu_off.size() * 8, false));
    HIPCHK(hipMemcpy(pr.d_cu_off, cu_off.data(), cu_off.size() * 8, hipMemcpyHostToDevice));
    unsigned long long* d_tile = nullptr;
    HIPCHK(hipMalloc((void**)&d_tile, tile_off.size() * 8));
    hipError_t e = hipMemcpy(d_tile, tile_off.data(), tile_off.size() * 8, hipMemcpyHostToDevice);
    for (size_t p = 0; p < pr.phases.size() && e == hipSuccess; ++p)
        if (src[p].w) e = launch_persist_pack(src[p].w, src[p].gamma, pr.phases[p], h->ncu, pr.stream, d_tile + p * h->ncu, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    hipFree(d_tile);
    HIPCHK(e);
    pr.ok = true;
    return HQT_OK;
}

// finalize (root): the weight streams of both programs
static int persist_build(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    h->pbody = PersistProg(); h->pfull = PersistProg();
    if (!c.has_stage2 || !(h->layouts & HQT_LAYOUT_FAST) || switch_value(SW_PERSIST_BUILD_OFF)) return HQT_OK;
    HIPCHK(hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, h->device));
    // one 576-thread workgroup with its whole LDS ring must fit a compute unit, or the grid barrier can never complete: no program then (launch chain)
    HIPCHK(persist_configure());
    if (persist_blocks_per_cu() < 1) return HQT_OK;
    for (auto& b : h->body) if (!b.qkv.bias_ln || !b.fc1.bias_ln) return HQT_OK;        // no deferred-LayerNorm layouts for these shapes: launch chain
    for (auto& b : h->depth) if (!b.qkv.bias_ln || !b.fc1.bias_ln) return HQT_OK;
    std::vector<PackSrc> src;
    int k4 = 0;
    if (c.code_levels != 3 && c.depth_decoding != HQT_DEPTH_BIDIRECTIONAL && h->head_top.bias_ln) {
        // two levels, 'parallel': body -> ln_f + sos_depth (a phase on the residual stream itself) -> the four single-key blocks of depth sub-step 0 -> head_top
        PersistProg& pr = h->pfull;
        for (auto& b : h->body) persist_block_shapes(h, b, false, h->Tmax, &k4, pr.phases, src);
        PersistPhase ph{};
        ph.type = PP_LNF; ph.N = c.embed_dim; ph.K = c.embed_dim; ph.map = PP_MAP_QUAD; ph.dln = 1;
        pr.phases.push_back(ph); src.push_back({nullptr, nullptr});
        for (auto& b : h->depth) persist_block_shapes(h, b, true, h->depth_rows, &k4, pr.phases, src);
        ph = PersistPhase{};
        ph.type = PP_ROWS; ph.N = c.vocab_top; ph.K = c.embed_dim; ph.dln = 1;
        pr.phases.push_back(ph); src.push_back({h->head_top.w32, h->w[key2(h, "ln_top.weight")].d});
        CHK(persist_build_one(h, pr, src));
        if (pr.ok) {
            const int D = c.embed_dim;
            std::vector<float> beta(D), sos(D);
            HIPCHK(hipMemcpy(beta.data(), h->w[key2(h, "ln_f.bias")].d, (size_t)D * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(sos.data(), h->w[key2(h, "sos_depth")].d, (size_t)D * 4, hipMemcpyDeviceToHost));
            for (int i = 0; i < D; ++i) beta[i] += sos[i];
            CHK(dev_alloc(h, (void**)&h->lnf_shift, (size_t)D * 4, false));
            HIPCHK(hipMemcpy(h->lnf_shift, beta.data(), (size_t)D * 4, hipMemcpyHostToDevice));
        }
    }
    if (!h->pfull.ok) {                          // three code levels, 'bidirectional' (or no folded head): the body alone
        src.clear(); k4 = 0;
        for (auto& b : h->body) persist_block_shapes(h, b, false, h->Tmax, &k4, h->pbody.phases, src);
        CHK(persist_build_one(h, h->pbody, src));
    }
    HIPCHK(persist_configure());
    return HQT_OK;
}

// per handle (a clone binds its own workspace): the phase tables with this handle's buffers.  Outside stream capture.
static int persist_bind(hqt_handle* h) {
    const hqt_config& c = h->cfg;
    if (h->parent) return HQT_OK;                // lanes never launch it (persist_on): no phase tables, no uploads
    const size_t D = c.embed_dim;
    auto upload = [&](PersistProg& pr) -> int {
        CHK(dev_alloc(h, (void**)&pr.d_phases, pr.phases.size() * sizeof(PersistPhase), true));
        HIPCHK(hipMemcpy(pr.d_phases, pr.phases.data(), pr.phases.size() * sizeof(PersistPhase), hipMemcpyHostToDevice));
        return HQT_OK;
    };
    auto bind_body = [&](PersistProg& pr) -> size_t {
        const size_t kv_layer = (size_t)c.max_batch * h->Tmax * D;              // bf16 elements
        size_t p = 0;
        for (int l = 0; l < c.n_layers; ++l) {
            const BlockW& bw = h->body[l];
            bf16_t* kc = reinterpret_cast<bf16_t*>(h->kcache) + l * kv_layer;
            bf16_t* vc = reinterpret_cast<bf16_t*>(h->vcache) + l * kv_layer;
            PersistPhase* ph = &pr.phases[p];
            ph[0].A = h->xpk; ph[0].bias = bw.qkv.bias_ln; ph[0].colsum = bw.qkv.colsum; ph[0].out = h->qbuf; ph[0].kc = kc; ph[0].vc = vc;
            ph[1].A = reinterpret_cast<bf16_t*>(h->qbuf); ph[1].out = h->abuf; ph[1].kc = kc; ph[1].vc = vc;
            ph[2].A = reinterpret_cast<bf16_t*>(h->abuf); ph[2].bias = bw.proj.b32; ph[2].out = h->xpk;
            ph[3].A = h->xpk; ph[3].bias = bw.fc1.bias_ln; ph[3].colsum = bw.fc1.colsum; ph[3].out = h->mbuf;
            ph[4].A = reinterpret_cast<bf16_t*>(h->mbuf); ph[4].bias = bw.fc2.b32; ph[4].out = h->xpk;
            p += 5;
        }
        return p;
    };
    if (h->pbody.ok && !h->pbody.d_phases) {
        bind_body(h->pbody);
        CHK(upload(h->pbody));
    }
    if (h->pfull.ok && !h->pfull.d_phases) {
        size_t p = bind_body(h->pfull);
        PersistPhase& lf = h->pfull.phases[p++];
        lf.A = h->xpk; lf.bias = h->lnf_shift; lf.colsum = W(h, "ln_f.weight"); lf.out = h->xdpk;
        const size_t dkv_layer = (size_t)h->depth_cap() * h->depth_rows * D;      // run_depth's stride: the chain's sub-step 1 reads what this launch appends
        for (int l = 0; l < c.n_layers_depth; ++l) {
            const BlockW& bw = h->depth[l];
            PersistPhase* ph = &h->pfull.phases[p];
            ph[0].A = h->xdpk; ph[0].bias = bw.qkv.bias_ln + D; ph[0].colsum = bw.qkv.colsum + D;
            ph[0].kc = reinterpret_cast<bf16_t*>(h->dk) + l * dkv_layer; ph[0].vc = reinterpret_cast<bf16_t*>(h->dv) + l * dkv_layer;
            ph[0].vpk = reinterpret_cast<bf16_t*>(h->abuf);
            ph[1].A = reinterpret_cast<bf16_t*>(h->abuf); ph[1].bias = bw.proj.b32; ph[1].out = h->xdpk;
            ph[2].A = h->xdpk; ph[2].bias = bw.fc1.bias_ln; ph[2].colsum = bw.fc1.colsum; ph[2].out = h->mbuf;
            ph[3].A = reinterpret_cast<bf16_t*>(h->mbuf); ph[3].bias = bw.fc2.b32; ph[3].out = h->xdpk;
            p += 4;
        }
        PersistPhase& hd = h->pfull.phases[p];
        hd.A = h->xdpk; hd.bias = h->head_top.bias_ln; hd.colsum = h->head_top.colsum; hd.out = h->logits;
        CHK(upload(h->pfull));
    }
    return HQT_OK;
}

static bool persist_on(hqt_handle* h, const SampleCtx& c, const PersistProg& pr) {
    return h->persist_enabled && !h->persist_tripped && pr.ok && pr.d_phases && c.md.fast && c.B <= 64 && h->policy == HQT_POLICY_LATENCY && !h->parent &&
           !c.row_pos;       // a rolling pass takes the launch chain: the persistent launch keeps ONE t_base for all its rows (persist.h)
}

static int run_persist(hqt_handle* h, const SampleCtx& c, const PersistProg& pr, float* x32, int write_back, const int* t_dev, const char* slot) {
    Timed t(h, slot, c.st);
    PersistArgs a{};
    a.phases = pr.d_phases; a.n_phases = (int)pr.phases.size(); a.wstream = pr.stream; a.cu_off = pr.d_cu_off;
    a.counters = h->persist_counters; a.err = h->persist_err; a.x32 = x32; a.slabs = h->persist_slabs;
    a.D = h->cfg.embed_dim; a.M = c.B; a.MB = packed_mb(c.B); a.n_heads = h->cfg.n_heads; a.head_dim = h->cfg.embed_dim / h->cfg.n_heads;
    a.t_base = 0; a.t_base_dev = t_dev; a.write_back = write_back;
    a.nt_weights = switch_value(SW_PERSIST_NT);
    persist_default_fill(a);
    HIPCHK(launch_persist(a, h->ncu, c.st));
    h->persist_used = true;
    h->capture_persist = true;
    count_variant(h, "variant:%s", slot);
    return HQT_OK;
}

// The split-K slabs the last GEMM left pending go to this LayerNorm, which folds them into x before normalising
static void take_pend(hqt_handle* h, LNArgs& ln) {
    ln.slabs = h->pend.slabs; ln.n_slabs = h->pend.S; ln.slab_rows = h->pend.rows; ln.slab_bias = h->pend.bias;
    h->pend = {nullptr, 0, 0, nullptr};
}

static int run_ln(hqt_handle* h, hipStream_t st, float* x, const float* g, const float* b, const float* add, void* y, int M,
                  int D, int in_rpg, int in_off, int out_dt, int out_pk) {
    Timed t(h, "layernorm", st);
    LNArgs ln{x, g, b, add, y, M, D, in_rpg, in_off, 1e-5f, out_dt, out_pk};
    take_pend(h, ln);
    HIPCHK(launch_layernorm(ln, st));
    return HQT_OK;
}

// One residual stream of the AR loop: fp32 master rows.  xpk non-null: FAST deferred LayerNorm -- the stream also keeps a bf16 packed
// copy with *nparts partial row statistics per row in `parts`; null: classic LayerNorm launches.
struct Resid { float* x; bf16_t* xpk; float* parts; int* nparts; };

static bool dln_ok(hqt_handle* h, const SampleCtx& c, const BlockW& bw, int M) {
    if (switch_value(SW_NO_DLN)) return false;                    // debugging / A-B switch: classic LayerNorm kernels
    return c.md.fast && M <= PACKED_MAX_ROWS && bw.qkv.wpk_ln && bw.fc1.wpk_ln && bw.proj.wpk && bw.fc2.wpk && h->cfg.embed_dim % 32 == 0;
}

// One transformer block over M = B*Tq rows (stage2/layers.py:324-328,371-375): qkv, attention, proj, fc1, fc2.
// Classic: a LayerNorm launch in front of qkv and of fc1 (7 launches).  Deferred LayerNorm (5 launches): qkv / fc1 consume the packed copy of
// the stream with gamma-folded weights and normalise in their epilogue, proj / fc2 update master rows, copy and statistics in theirs.
// (Round 4's ninth "prefetch" wave, which touched the NEXT launch's weights from inside this one, bought nothing --
// profiles/r04_micro_weight_prefetch.txt -- and left with its switch in round 5.)
static int run_block(hqt_handle* h, const SampleCtx& c, const BlockW& bw, const Resid& r, int Tq, void* kc, void* vc, int Tcache,
                     int t_base, const int* t_base_dev, int causal) {
    const int D = h->cfg.embed_dim, M = c.B * Tq, adt = c.md.act_dt();
    const bool dln = r.xpk != nullptr;
    // FAST: GEMM A operands travel in the MFMA-fragment-packed layout when the streaming GEMM serves them
    const int pk = (dln || (c.md.fast && M <= PACKED_MAX_ROWS && bw.qkv.wpk && bw.proj.wpk && bw.fc1.wpk && bw.fc2.wpk)) ? packed_mb(M) : 0;
    // the A operand of qkv / fc1: the normalised stream
    auto normed = [&](GemmArgs& g, const float* gamma, const float* beta, const Lin& l) -> int {
        g.M = M; g.batch = 1; g.a_packed_mb = pk;
        if (dln) { g.A = r.xpk; g.ln_parts = r.parts; g.ln_nparts = *r.nparts; g.ln_colsum = l.colsum; g.ln_eps = 1e-5f; return HQT_OK; }
        g.A = h->hbuf;
        return run_ln(h, c.st, r.x, gamma, beta, nullptr, h->hbuf, M, D, 1, 0, adt, pk);
    };
    // proj / fc2: x += A W^T + b
    auto residual = [&](const void* A, const Lin& l, const char* tag) -> int {
        GemmArgs g{};
        g.A = A; g.M = M; g.batch = 1; g.a_packed_mb = pk; g.C = r.x; g.ldc = D;
        if (dln) { g.store = STORE_RESID; g.resid_pk = r.xpk; g.resid_parts = r.parts; g.c_packed_mb = pk; }
        else { g.store = STORE_ROWS; g.resid = r.x; }
        return ar_linear(h, c.md, g, l, adt, DT_F32, c.st, tag, true, dln ? r.nparts : nullptr);
    };
    GemmArgs g{};
    CHK(normed(g, bw.ln1_g, bw.ln1_b, bw.qkv));
    g.C = h->qbuf; g.C2 = kc; g.C3 = vc; g.ldc = D; g.qkv_D = D; g.store = STORE_QKV;
    g.rows_per_group = Tq; g.group_stride = Tcache; g.row_offset = t_base; g.row_offset_dev = t_base_dev;
    // a rolling pass: where a decode step of the body reads the step state's t_base, every sample reads its own position (the depth blocks never do)
    const int* const row_pos = t_base_dev ? c.row_pos : nullptr;
    g.row_pos = row_pos;
    // One query over one key (depth sub-step 0: hierarchical_ar.py:690-702 with an empty cache): softmax of a single
    // score is exactly 1, so the attention output is the value row itself.  The GEMM then skips the query third of
    // the fused weight (rows [D, 3D) only), appends K/V to the cache for sub-step 1 and writes V straight into the
    // projection's operand; no attention launch.
    if (dln && Tq == 1 && t_base == 0 && !t_base_dev && h->single_key) {
        g.qkv_first = 1; g.qkv_v_pk = reinterpret_cast<bf16_t*>(h->abuf); g.c_packed_mb = pk;
        Lin kv = bw.qkv;
        kv.N = 2 * D;
        kv.wpk_ln = bw.qkv.wpk_ln + (size_t)D * bw.qkv.K;          // packed n-tiles are contiguous: skip D rows
        kv.bias_ln = bw.qkv.bias_ln + D;
        kv.colsum = bw.qkv.colsum + D;
        g.ln_colsum = kv.colsum;
        CHK(ar_linear(h, c.md, g, kv, adt, adt, c.st, "gemm_qkv"));
    } else {
        CHK(ar_linear(h, c.md, g, bw.qkv, adt, adt, c.st, "gemm_qkv"));
        Timed t(h, "attention", c.st);
        AttnArgs a{h->qbuf, kc, vc, h->abuf, c.B, Tq, h->cfg.n_heads, D / h->cfg.n_heads, Tcache, t_base, t_base_dev, causal, adt, pk, nullptr, row_pos};
        if (h->timing) count_variant(h, "variant:attn_%s:%s", attention_kernel_name(attention_choice(a)), r.x == h->xd ? "depth" : "body");
        HIPCHK(launch_attention(a, c.st));
    }
    CHK(residual(h->abuf, bw.proj, "gemm_proj"));
    g = GemmArgs{};
    CHK(normed(g, bw.ln2_g, bw.ln2_b, bw.fc1));
    g.C = h->mbuf; g.ldc = 4 * D;
    g.store = pk ? STORE_PACKED : STORE_ROWS; g.c_packed_mb = pk;
    g.act = h->cfg.gelu_approx ? ACT_GELU_SIGMOID : ACT_GELU_ERF;
    CHK(ar_linear(h, c.md, g, bw.fc1, adt, adt, c.st, "gemm_fc1"));
    return residual(h->mbuf, bw.fc2, "gemm_fc2");
}

// The body blocks of one position over Tq_body rows: as ONE persistent launch up to the top logits (pfull: two code levels, 'parallel' -- persist_build
// makes that program for no other head; dln0: sub-step 0 of the depth head takes the deferred-LayerNorm path), as one persistent launch of the body
// alone (pbody), or as the launch chain.  *pfull: the whole-position launch ran.
// `stage` (staged_prompt_prefill: shared prompts, the joiners of a rolling text pass): K/V go to the staging buffer of [n_layers][c.B][Tq_body][D] instead of the cache.
struct KvStage { void *k, *v; };
static int run_body(hqt_handle* h, const SampleCtx& c, int Tq_body, int body_t_base, bool body_tbase_from_state, bool dln0, bool* pfull,
                    const KvStage* stage = nullptr) {
    const hqt_config& cf = h->cfg;
    const int Tcache = stage ? Tq_body : h->Tmax;
    const size_t kv_layer = (size_t)(stage ? c.B : cf.max_batch) * Tcache * cf.embed_dim * c.md.act_sz();
    char* const kc = (char*)(stage ? stage->k : h->kcache);
    char* const vc = (char*)(stage ? stage->v : h->vcache);
    const int* tb_dev = body_tbase_from_state ? &h->state->t_base : nullptr;
    // deferred LayerNorm needs the packed copy + row statistics of x from the caller's embedding kernel: embed_step emits
    // them (decode steps, Tq = 1); the text prefill's embed_text does not, so the prefill pass takes the classic path
    const bool dln_body = Tq_body == 1 && dln_ok(h, c, h->body[0], c.B * Tq_body);
    // the twelve body blocks as ONE persistent launch (persist.h): decode steps of up to 64 samples
    const bool body_persistable = dln_body && body_tbase_from_state && body_t_base == 0;
    *pfull = body_persistable && dln0 && h->single_key && persist_on(h, c, h->pfull);
    const bool pbody = !*pfull && body_persistable && persist_on(h, c, h->pbody);
    if (*pfull) CHK(run_persist(h, c, h->pfull, h->x, 0, tb_dev, "persist_position"));
    if (pbody) CHK(run_persist(h, c, h->pbody, h->x, 1, tb_dev, "persist_body"));
    const Resid r{h->x, dln_body ? h->xpk : nullptr, h->parts, &h->nparts};
    for (int l = 0; l < (pbody || *pfull ? 0 : cf.n_layers); ++l)
        CHK(run_block(h, c, h->body[l], r, Tq_body, kc + l * kv_layer, vc + l * kv_layer, Tcache, body_t_base, tb_dev, 1));
    return HQT_OK;
}

// The depth blocks over the Tq tokens per sample in xd, at offset tbase of the depth cache
static int run_depth(hqt_handle* h, const SampleCtx& c, bool dln, int Tq, int tbase) {
    const hqt_config& cf = h->cfg;
    const size_t dkv_layer = (size_t)h->depth_cap() * h->depth_rows * cf.embed_dim * c.md.act_sz();      // (max_batch, unless hqt_set_score_chunk made room for more)
    const Resid r{h->xd, dln ? h->xdpk : nullptr, h->partsd, &h->npartsd};
    for (int l = 0; l < cf.n_layers_depth; ++l)
        CHK(run_block(h, c, h->depth[l], r, Tq, (char*)h->dk + l * dkv_layer, (char*)h->dv + l * dkv_layer, h->depth_rows, tbase, nullptr, 0));
    return HQT_OK;
}

static int head_pk(const SampleCtx& c, const Lin& head, int M) {      // FAST: the head GEMM's operand travels packed when the streaming GEMM serves it
    return (c.md.fast && M <= PACKED_MAX_ROWS && head.wpk) ? packed_mb(M) : 0;
}

// Logits of the M depth rows of code level lv into h->logits: ln_levels[lv] folded into the head GEMM (dln: the deferred-LayerNorm operand), or
// the LayerNorm of xd into hbuf and then the GEMM.  `normed` non-null: the operand is already normalised there (the bidirectional head).
// `out` non-null (hqt_score): the rows go there instead (contiguous, ldc = V).
static int run_head(hqt_handle* h, const SampleCtx& c, const Lin& head, int lv, int M, bool dln, void* normed, float* out = nullptr) {
    static const char* const ln_names[3][2] = {{"ln_top.weight", "ln_top.bias"}, {"ln_bot.weight", "ln_bot.bias"}, {"ln_levels.2.weight", "ln_levels.2.bias"}};
    const int adt = c.md.act_dt(), pk = head_pk(c, head, M);
    GemmArgs g{};
    if (dln) {
        g.A = h->xdpk; g.ln_parts = h->partsd; g.ln_nparts = h->npartsd; g.ln_colsum = head.colsum; g.ln_eps = 1e-5f;
    } else {
        if (!normed) {
            normed = h->hbuf;
            CHK(run_ln(h, c.st, h->xd, W(h, ln_names[lv][0]), W(h, ln_names[lv][1]), nullptr, normed, M, h->cfg.embed_dim, 1, 0, adt, pk));
        }
        g.A = normed;
    }
    g.a_packed_mb = pk; g.M = M; g.batch = 1; g.C = out ? out : h->logits; g.ldc = h->cfg.vocab_top; g.store = STORE_ROWS;
    return ar_linear(h, c.md, g, head, adt, DT_F32, c.st, "gemm_head");
}

// One depth sub-step: code level lv, Tq tokens per sample at offset tbase of the depth sequence (which is also the first draw index of the
// sampler); out_stride > 0: each token writes slot out_slot of an out_stride-wide code group (the 21-step causal head)
struct SubStep { int lv, Tq, tbase, out_stride, out_slot; };
static SubStep sub_step(const hqt_config& cf, int sub) {
    static const int first[3] = {0, 1, 5};
    if (cf.depth_decoding != HQT_DEPTH_TOP2MID2BOT) return {sub, LEVEL_WIDTH[sub], first[sub], 0, 0};
    const int lv = sub == 0 ? 0 : (sub < 5 ? 1 : 2);
    return {lv, 1, sub, lv ? LEVEL_WIDTH[lv] : 0, sub - first[lv]};
}

// The input rows of depth sub-step `sub` in xd (dln: with their packed copy and row statistics); sub-step 0 reads the last of the Tq_body rows per sample in x
static int run_depth_input(hqt_handle* h, const SampleCtx& c, float* x, int sub, bool dln, int Tq_body, bool fuse) {
    const hqt_config& cf = h->cfg;
    const int D = cf.embed_dim, B = c.B, V = cf.vocab_top;
    const SubStep s = sub_step(cf, sub);
    const int M = B * s.Tq, pk = dln ? packed_mb(M) : 0, dmul = cf.depth_decoding == HQT_DEPTH_PARALLEL_REDUCE ? 4 : 1;
    bf16_t* xpk = dln ? h->xdpk : nullptr;
    if (sub == 0) {           // ln_f on the last token of each sample, + sos_depth (hierarchical_ar.py:561,684-686) -> depth input of level 0
        Timed t(h, "layernorm", c.st);
        LNArgs ln{x, W(h, "ln_f.weight"), W(h, "ln_f.bias"), W(h, "sos_depth"), h->xd, B, D, Tq_body, Tq_body - 1, 1e-5f, DT_F32, 0,
                  nullptr, 0, 0, nullptr, xpk, pk, h->partsd};
        take_pend(h, ln);
        HIPCHK(launch_layernorm(ln, c.st));
    } else if (cf.depth_decoding == HQT_DEPTH_TOP2MID2BOT) {   // the previous sub-step's code, embedded by the spatial tables, + its position in the 21-token sequence
        Timed t(h, "embed", c.st);
        const SubStep p = sub_step(cf, sub - 1);
        const int tbl = sub == 1 ? 0 : (sub < 5 ? 1 : 2);
        const float* tok = tbl == 0 ? W(h, "tok_emb_top.weight") : (tbl == 1 ? W(h, "tok_emb_bot.weight") : W(h, "tok_emb_levels.2.weight"));
        HIPCHK(launch_depth_embed_causal(c.feed[p.lv], p.lv ? p.out_stride : 1, p.out_slot, c.n_steps, h->state, tok,
                                         W(h, "pos_emb_depth.weight") + (size_t)p.tbase * D, h->xd, B, D, xpk, pk, h->partsd, c.st, V, c.row_pos));
    } else if (s.lv == 1) {   // emb(top code) + positions 0..3 (fuse: the top sampler wrote them)
        if (fuse) return HQT_OK;
        Timed t(h, "embed", c.st);
        HIPCHK(launch_depth_embed(c.feed[0], c.n_steps, h->state, W(h, "tok_emb_top_depth.weight"), W(h, "pos_emb_depth.weight"),
                                  h->xd, B, D, xpk, pk, h->partsd, c.st, V, dmul * D, c.row_pos));
    } else {                  // parent's level-1 embedding + position i (+ emb(top code): 'add'), 16 tokens
        Timed t(h, "embed", c.st);
        HIPCHK(launch_depth_embed_l2(c.feed[0], c.feed[1], c.n_steps, h->state,
                                     cf.depth_decoding == HQT_DEPTH_PARALLEL_ADD ? W(h, "tok_emb_top_depth.weight") : nullptr,
                                     W(h, "tok_emb_depth_levels.1.weight"), W(h, "pos_emb_depths.1.weight"),
                                     h->xd, B, D, xpk, pk, h->partsd, c.st, V, dmul * D, c.row_pos));
    }
    return HQT_OK;
}

static const Lin& head_of(const hqt_handle* h, int lv) { return lv == 0 ? h->head_top : (lv == 1 ? h->head_bot : h->head_l2); }      // the head of code level lv
// Sub-step `s` of the depth head takes the deferred-LayerNorm path (never the bidirectional head's single pass, which decides for itself)
static bool depth_dln(hqt_handle* h, const SampleCtx& c, const SubStep& s) {
    return h->cfg.depth_decoding != HQT_DEPTH_BIDIRECTIONAL && dln_ok(h, c, h->depth[0], c.B * s.Tq) && head_of(h, s.lv).wpk_ln;
}

// The bidirectional head behind its input launch: one pass of the depth blocks over the depth_rows rows per sample in xd, then ln_top / ln_bot of the
// interleaved rows into two compact head operands, normed[0] = [B, D] (hbuf) and normed[1] = [4 B, D] (abuf)
static int run_bidir_tail(hqt_handle* h, const SampleCtx& c, bool dln, void** normed) {
    const int B = c.B, M = B * h->depth_rows;
    CHK(run_depth(h, c, dln, h->depth_rows, 0));      // Tq = 5 > 1: never the single-key shortcut of run_block
    Timed t(h, "bidir_head_ln", c.st);
    LNArgs ln{h->xd, W(h, "ln_top.weight"), W(h, "ln_top.bias"), nullptr, h->hbuf, M, h->cfg.embed_dim, 1, 0, 1e-5f, c.md.act_dt(), head_pk(c, h->head_top, B)};
    ln.gamma2 = W(h, "ln_bot.weight"); ln.beta2 = W(h, "ln_bot.bias"); ln.y2 = h->abuf; ln.out2_packed_mb = head_pk(c, h->head_bot, 4 * B);
    take_pend(h, ln);
    HIPCHK(launch_bidir_head_ln(ln, c.st));
    normed[0] = h->hbuf; normed[1] = h->abuf;
    return HQT_OK;
}

// Split-K slabs the last body GEMM left for "the next LayerNorm" belong to all M rows of x: folded into them here through ln_f (the normalised rows in hbuf
// are not read), before anything gathers x and before the depth GEMMs reuse the slab workspace
static int fold_pending(hqt_handle* h, const SampleCtx& c, int M) {
    if (!h->pend.slabs) return HQT_OK;
    return run_ln(h, c.st, h->x, W(h, "ln_f.weight"), W(h, "ln_f.bias"), nullptr, h->hbuf, M, h->cfg.embed_dim, 1, 0, DT_F32, 0);
}

// Everything of one top position after the body input x is ready (hierarchical_ar.py:482-563,667-789; three code levels:
// hqtransformer.py:409-635): the body blocks, ln_f, then the depth sub-steps, each an input step, the depth blocks, a head and its draws.
//  - 'parallel' (two levels; three: 'parallel-add', 'parallel-reduce'): one sub-step per level over 1, 4 (and 16) tokens.  Every sub-step's
//    tokens see all earlier and current depth tokens (the 'parallel' mask of layers.py:154-178 restricted to the rows being evaluated is
//    all-ones), so the attention runs non-causally over tbase + Tq keys of the depth cache.
//  - 'top2mid2bot' (hqtransformer.py:700-800): 21 causal sub-steps of ONE token -- sub-step cnt >= 1 is fed the code drawn by cnt - 1
//    through tok_emb_levels[cnt == 1 ? 0 : (cnt < 5 ? 1 : 2)] (:718-723: the table follows the sub-step being computed, so the last middle
//    code is embedded with the level-2 table, as there) + pos_emb_depths.0[cnt - 1]; head of level (cnt == 0 ? 0 : cnt < 5 ? 1 : 2)
//  - 'bidirectional' (hierarchical_ar.py:791-878; its Blocks have causal_attn = False: layers.py:290-330, no mask at all): ONE pass of the
//    depth blocks over five rows per sample, [ln_f(h) + sos_depth, pos_emb_depth[0..3]], with full 5 x 5 attention and no cache carried to
//    the next position; then the two 'parallel' sub-steps' heads and draws, top logits from row 0 (ln_top, head_top), bottom from rows 1..4
//    (ln_bot, head_bot).  All five draws use temperature_top, top_k_bot and top_p_bot, as the reference does (:866-873).
// The depth-head half of a position: ln_f on the last of the Tq_body rows per sample in x (h->x, or the rows a staged prompt prefill gathered; a pending split-K
// fold rewrites them), the sub-steps and their draws.  pfull: the whole-position persistent launch already computed sub-step 0 up to its logits (run_body).
static int run_depth_head(hqt_handle* h, const SampleCtx& c, float* x, int Tq_body, bool pfull) {
    const hqt_config& cf = h->cfg;
    const int D = cf.embed_dim, B = c.B, V = cf.vocab_top;
    const bool bidir = cf.depth_decoding == HQT_DEPTH_BIDIRECTIONAL, causal_head = cf.depth_decoding == HQT_DEPTH_TOP2MID2BOT;
    const int nsub = causal_head ? h->depth_rows : c.levels;       // 'top2mid2bot': one sub-step per depth token
    // the draw and the embedding lookup of the drawn code in one kernel: the two-level top sampler's workgroup of sample b also writes the
    // four input rows of depth sub-step 1 (HQT_NO_FUSED_EMBED=1: separate depth_embed_kernel, for A/B runs)
    const bool fuse = !switch_value(SW_NO_FUSED_EMBED) && c.levels == 2 && !bidir;
    void* normed[3] = {nullptr, nullptr, nullptr};
    SamplerSet bidir_set;
    if (bidir) {                  // one pass over all depth rows
        const int M = B * h->depth_rows;
        const bool dln = dln_ok(h, c, h->depth[0], M);
        {
            Timed t(h, "bidir_depth_input", c.st);
            LNArgs ln{x, W(h, "ln_f.weight"), W(h, "ln_f.bias"), W(h, "sos_depth"), h->xd, B, D, Tq_body, Tq_body - 1, 1e-5f, DT_F32, 0,
                      nullptr, 0, 0, nullptr, dln ? h->xdpk : nullptr, dln ? packed_mb(M) : 0, h->partsd};
            ln.fill = W(h, "pos_emb_depth.weight");
            take_pend(h, ln);
            HIPCHK(launch_bidir_depth_input(ln, c.st));
            h->npartsd = 1;
        }
        CHK(run_bidir_tail(h, c, dln, normed));
        bidir_set = {c.lv[0].temperature, c.lv[1].top_k, c.lv[1].top_p};
    }
    for (int sub = 0; sub < nsub; ++sub) {
        const SubStep s = sub_step(cf, sub);
        const int M = B * s.Tq;
        const bool dln = depth_dln(h, c, s), in_pfull = pfull && sub == 0;      // the whole-position launch computed sub-step 0 up to its logits
        if (!bidir && !in_pfull) {    // the bidirectional pass ran its depth blocks above
            CHK(run_depth_input(h, c, x, sub, dln, Tq_body, fuse));
            h->npartsd = 1;
            CHK(run_depth(h, c, dln, s.Tq, s.tbase));
        }
        if (!in_pfull) CHK(run_head(h, c, head_of(h, s.lv), s.lv, M, dln, normed[s.lv]));
        if (c.guide) {            // both rows of every pair become the guided row before anything reads the logits (the sampler, its logits_out copy, code_logprob)
            Timed t(h, "guide_logits", c.st);
            HIPCHK(launch_guide_logits(h->logits, h->guide, c.n_guide, V, s.Tq, s.lv, c.st));
        }
        {
            Timed t(h, bidir ? (s.lv ? "bidir_sampler_bot" : "bidir_sampler_top") : "sampler", c.st);
            const SamplerSet& set = bidir ? bidir_set : c.lv[s.lv];
            SamplerArgs sa{h->logits, M, V, s.Tq, B, set.temperature, set.top_k, set.top_p, c.noise, s.tbase,
                           h->state, h->rows, c.n_steps, c.out[s.lv], c.logits_out, h->depth_rows};
            sa.out_stride = s.out_stride; sa.out_slot = s.out_slot;
            sa.fast_math = c.md.fast ? 1 : 0;
            if (c.row_set) {      // the bidirectional head keeps its mapping per row: every draw with temperature[0], top_k[1], top_p[1]
                sa.row_set = h->row_set; sa.row_top_p = c.row_top_p ? 1 : 0;
                sa.row_lv_t = bidir ? 0 : s.lv; sa.row_lv_k = bidir ? 1 : s.lv;
            }
            if (c.keep) sa.keep = h->keep_mask;
            sa.row_pos = c.row_pos;
            if (fuse && sub == 0) {
                const bool dln_next = depth_dln(h, c, sub_step(cf, 1));
                sa.emb_tok = W(h, "tok_emb_top_depth.weight"); sa.emb_pos = W(h, "pos_emb_depth.weight");
                sa.emb_feed = c.feed[0] != c.out[0] ? c.feed[0] : nullptr;
                sa.emb_x = h->xd; sa.emb_D = D;
                sa.emb_xpk = dln_next ? h->xdpk : nullptr; sa.emb_pk_mb = dln_next ? packed_mb(4 * B) : 0; sa.emb_parts = h->partsd;
            }
            HIPCHK(launch_sampler(sa, c.st));
            // one launch per draw, each under a timing slot of its own (the sampler's ends here): the log-probability, or the report, which also writes that where a buffer is staged
            const bool report = c.report.any();
            for (int slot = 0; slot < (report || c.logprob_out ? s.Tq : 0); ++slot) {
                t.next(report ? "draw_report" : "code_logprob");
                if (report) HIPCHK(launch_draw_report(sa, c.feed[s.lv], c.logprob_out, c.report, slot, c.st));
                else HIPCHK(launch_code_logprob(sa, c.feed[s.lv], c.logprob_out, slot, c.st));
            }
        }
    }
    return HQT_OK;
}

// One position: the body blocks, then the depth head
static int run_position(hqt_handle* h, const SampleCtx& c, int Tq_body, int body_t_base, bool body_tbase_from_state) {
    bool pfull = false;
    CHK(run_body(h, c, Tq_body, body_t_base, body_tbase_from_state, depth_dln(h, c, sub_step(h->cfg, 0)), &pfull));
    return run_depth_head(h, c, h->x, Tq_body, pfull);
}

// hqt_config.ar_layouts: a precision whose weight layout the handle was created without fails here, loudly (never a silent slower path)
static int layout_check(const hqt_handle* h, const Mode& md) {
    if (md.fast && !(h->layouts & HQT_LAYOUT_FAST)) return fail(HQT_ERR_STATE, "HQT_PRECISION_FAST on a handle created without HQT_LAYOUT_FAST (hqt_config.ar_layouts = %d)", h->cfg.ar_layouts);
    if (md.split_ar && !(h->layouts & HQT_LAYOUT_SPLIT)) return fail(HQT_ERR_STATE, "HQT_PRECISION_SPLIT on a handle created without HQT_LAYOUT_SPLIT (hqt_config.ar_layouts = %d)", h->cfg.ar_layouts);
    return HQT_OK;
}

// What the body-input embedding reads: the tables, cond and the codes of every level in `codes` ([B, n_steps(, 4 | 16)])
static EmbedArgs embed_args(hqt_handle* h, const SampleCtx& c, const int64_t* const* codes) {
    const hqt_config& cf = h->cfg;
    EmbedArgs e{c.B, cf.embed_dim, c.n_steps, cf.embedding_type, cf.cond_type, h->state, c.cond,
                cf.cond_type == HQT_COND_CLASS ? W(h, "sos.weight") : (cf.cond_type == HQT_COND_NONE ? W(h, "sos") : nullptr),
                W(h, "tok_emb_top.weight"), W(h, "tok_emb_bot.weight"), W(h, "pos_emb_top.weight"),
                cf.embedding_type == HQT_EMB_TRANSFORMER1 ? W(h, "pos_emb_emb.weight") : nullptr,
                codes[0], codes[1], h->x, nullptr, 0, h->parts};
    if (c.levels == 3) { e.levels = 3; e.tok_l2 = W(h, "tok_emb_levels.2.weight"); e.codes_l2 = codes[2]; }
    e.V = cf.vocab_top; e.n_classes = cf.n_classes;
    e.row_pos = c.row_pos;                       // (read by the decode step's kernel only: a rolling call runs no prefill)
    return e;
}

// The body input rows of a prefill over P given positions, whose codes the embedding reads from `codes`; *rows: the body rows per sample.
//  - text: the T prompt rows, then row T + j = the input the decode step at position j + 1 computes from the codes of position j
//  - otherwise: the sos row, then the same P rows
static int embed_prefill(hqt_handle* h, const SampleCtx& c, const int64_t* const* codes, int P, int* rows) {
    const hqt_config& cf = h->cfg;
    const bool text = cf.cond_type == HQT_COND_TEXT;
    const int T = text ? cf.ctx_len_txt : 0;
    *rows = text ? T + P : P + 1;
    if (text) HIPCHK(launch_embed_text(c.cond, W(h, "tok_emb_txt.weight"), W(h, "pos_emb_txt.weight"), h->x, c.B, T, cf.embed_dim, c.st, cf.vocab_txt, T + P));
    if (text && P == 0) return HQT_OK;
    Timed t(h, "embed_prefix", c.st);
    HIPCHK(launch_embed_prefix(embed_args(h, c, codes), *rows - T, *rows, T, text ? 1 : 0, c.st));      // text: P rows behind the prompt, at step offset 1; otherwise P + 1 from the sos row
    return HQT_OK;
}

static int embed_step(hqt_handle* h, const SampleCtx& c) {      // the body input row of a decode step, one per sample (with the packed copy where run_body wants it)
    Timed t(h, "embed", c.st);
    EmbedArgs e = embed_args(h, c, c.feed);
    if (dln_ok(h, c, h->body[0], c.B)) { e.xpk = h->xpk; e.pk_mb = packed_mb(c.B); h->nparts = 1; }
    HIPCHK(launch_embed_step(e, c.st));
    return HQT_OK;
}
static int run_decode_step(hqt_handle* h, const SampleCtx& c) {      // one KV-cached position, Tq = 1
    CHK(embed_step(h, c));
    // a rolling pass of a text handle: row b stands behind its prompt, at cache row ctx_len_txt - 1 + pos[b] -- where the plain text call's step state puts
    // position pos[b]; the offset is a constant of the handle (an idle row stores at row ctx_len_txt - 1 of its own, dead slot and is read by nothing)
    const int behind_prompt = c.row_pos && h->cfg.cond_type == HQT_COND_TEXT ? h->cfg.ctx_len_txt - 1 : 0;
    CHK(run_position(h, c, 1, behind_prompt, true));
    if (c.row_pos) HIPCHK(launch_advance_rows(h->row_pos, c.B, c.n_steps, c.st));      // a rolling pass: every live row moves on; the step state is not read
    else HIPCHK(launch_advance_step(h->state, 1, c.st));
    return HQT_OK;
}

static int sample_run(hqt_handle* h, const SampleCtx& c);

// One buffer of the pinned ring (hqt_handle::rows_pinned) as the six host tables it holds.  ring_slot is the only place that knows their order and
// sizes: the keys come first, and every later section starts at a multiple of 4 bytes, which aligns each for its type.
struct RingSlot { RowKey* keys; RowSampler* samplers; GuidePair* pairs; int32_t* groups; int32_t* pos; unsigned char* keep; size_t bytes; };
static_assert(alignof(RowKey) == 8 && alignof(RowSampler) == 4 && alignof(GuidePair) == 4 && alignof(int32_t) == 4 &&
              sizeof(RowKey) % 4 == 0 && sizeof(RowSampler) % 4 == 0 && sizeof(GuidePair) % 4 == 0, "the order of a ring slot's sections no longer aligns each for its type");
static RingSlot ring_slot(const hqt_handle* h, RowKey* base) {      // (base null: only `bytes`, what a slot needs)
    const size_t B = h->cfg.max_batch;
    const size_t samplers = B * sizeof(RowKey), pairs = samplers + B * sizeof(RowSampler), groups = pairs + h->guide_room() * sizeof(GuidePair),
                 pos = groups + B * sizeof(int32_t), keep = pos + 3 * B * sizeof(int32_t);      // pos: the three tables of hqt_handle::row_pos, in its order
    RingSlot r{};
    r.bytes = keep + B * h->cfg.max_steps;
    if (!base) return r;
    unsigned char* const p = reinterpret_cast<unsigned char*>(base);
    r.keys = base;
    r.samplers = reinterpret_cast<RowSampler*>(p + samplers);
    r.pairs = reinterpret_cast<GuidePair*>(p + pairs);
    r.groups = reinterpret_cast<int32_t*>(p + groups);
    r.pos = reinterpret_cast<int32_t*>(p + pos);
    r.keep = p + keep;
    return r;
}

// The next buffer of the pinned ring, free to be rewritten: the copy that last read it (4 takes ago) is done.  The caller ends with ring_sent behind its copies.
static int rows_ring_take(hqt_handle* h, int* slot_out, RingSlot* view) {
    const int slot = h->rows_next;
    h->rows_next = (slot + 1) % hqt_handle::ROWS_RING;
    if (!h->rows_pinned[slot]) {
        HIPCHK(hipHostMalloc((void**)&h->rows_pinned[slot], ring_slot(h, nullptr).bytes, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&h->rows_ev[slot], hipEventDisableTiming));
    }
    if (h->rows_busy[slot]) HIPCHK(hipEventSynchronize(h->rows_ev[slot]));
    *slot_out = slot;
    *view = ring_slot(h, h->rows_pinned[slot]);
    return HQT_OK;
}
// n elements of a host table into a section of the slot (table null: they were built there) and, behind the stream's work, on to the device buffer
template <class T, class S> static int ring_send(T* section, const S* table, size_t n, T* dev, hipStream_t st) {
    static_assert(sizeof(T) == sizeof(S), "a staged table travels to the device as it is");
    if (table) memcpy(section, table, n * sizeof(T));
    HIPCHK(hipMemcpyAsync(dev, section, n * sizeof(T), hipMemcpyHostToDevice, st));
    return HQT_OK;
}
static int ring_sent(hqt_handle* h, int slot, hipStream_t st) {
    HIPCHK(hipEventRecord(h->rows_ev[slot], st));
    h->rows_busy[slot] = true;
    return HQT_OK;
}

// ---- what sample_call refuses, one function per staged feature (segment, row positions, prefix, keep table, prompt groups, row samplers, guidance), called in
// this order: any two refusals speak in the order of the lines below.  `s` is what the call took off the handle (the sizes the tables were staged with), cf and
// B the handle's config and the call's rows; what a check computes travels in `c`: start / stop and n_join, prefix_len of a keep table, top_p / row_top_p.
static int check_segment(const hqt_handle* h, const SampleCtx& c, int B) {
    if (c.start < 0 || c.stop <= c.start || c.stop > c.n_steps)
        return fail(HQT_ERR_INVALID, "hqt_set_segment staged [%d, %d): a segment needs 0 <= start < stop <= n_steps = %d", c.start, c.stop, c.n_steps);
    if (c.with_prefix) return fail(HQT_ERR_INVALID, "hqt_set_segment: the staged segment was taken by a prefix entry point; segments of a pass with a code prefix are not built (hqt_sample / hqt_sample_l3 take the segment)");
    if (c.keep) return fail(HQT_ERR_INVALID, "hqt_set_segment together with a staged keep table (hqt_set_keep_mask) is not built");
    if (c.groups && c.start > 0)
        return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups together with a segment that starts at position %d: the prompt prefill belongs to the segment that starts at 0", c.start);
    if (c.start > 0) {                       // a continuation: the cache and the step state must be those of THIS pass, stopped in front of `start`
        const hqt_handle::Paused& p = h->paused;
        if (!p.live) return fail(HQT_ERR_STATE, "hqt_set_segment: a segment that starts at position %d continues a paused pass, and this handle holds none "
                                                "(none was begun, the pass was finished, or another call has overwritten its cache since)", c.start);
        if (p.B != B) return fail(HQT_ERR_STATE, "hqt_set_segment: the paused pass has B=%d, this call has B=%d (hqt_select_rows changes the rows of a paused pass)", p.B, B);
        if (p.n_steps != c.n_steps) return fail(HQT_ERR_STATE, "hqt_set_segment: the paused pass has n_steps=%d, this call has n_steps=%d", p.n_steps, c.n_steps);
        if (p.levels != c.levels) return fail(HQT_ERR_STATE, "hqt_set_segment: the paused pass has %d code levels, this call has %d", p.levels, c.levels);
        if (p.precision != c.precision) return fail(HQT_ERR_STATE, "hqt_set_segment: the paused pass runs in precision %d, this call asks for precision %d (the cache holds that precision's type)", p.precision, c.precision);
        if (p.pos != c.start) return fail(HQT_ERR_STATE, "hqt_set_segment: the paused pass stands at position %d, this segment has start=%d", p.pos, c.start);
    }
    return HQT_OK;
}
// The join phase of a rolling call (sample_run): which rows it takes and the kept run it prefills.  The rows that join (position 0) share
// L = min(smallest leading run of ones of their mask rows, max_run of hqt_set_join_run, n_steps - 1), 0 without a keep table; the phase runs on a text handle (the
// joiners' prompts) and wherever L > 0, and draws position L.  Without it (no text, L == 0) a joining row's position 0 is an ordinary step.
static int check_joins(const hqt_handle* h, SampleCtx& c, const hqt_config& cf, int B) {
    const bool text = cf.cond_type == HQT_COND_TEXT;
    int joiners = 0, L = c.keep ? std::min(std::max(h->join_run, 0), c.n_steps - 1) : 0;
    for (int b = 0; b < B; ++b) {
        if (c.roll[b] != 0) continue;
        ++joiners;
        int run = 0;
        while (run < L && c.keep[(size_t)b * c.n_steps + run]) ++run;
        L = run;
    }
    if (!joiners || (!text && L == 0)) return HQT_OK;
    c.n_join = joiners; c.join_len = L;
    if (c.n_join > h->max_joins)
        return fail(HQT_ERR_INVALID, "hqt_set_row_positions: %d rows join at position 0 in this call, the handle's staging holds the prompts of max_joins=%d (hqt_set_max_joins)", c.n_join, h->max_joins);
    const size_t need = (size_t)cf.n_layers * c.n_join * h->staging_rows(L) * cf.embed_dim * 4;
    if (need > h->pg_bytes || !h->pg_k || !h->pg_v || !h->pg_x)
        return fail(HQT_ERR_STATE, "hqt_set_max_joins: the staging buffer holds %d prompts, %d rows join", h->pg_cap, c.n_join);
    return HQT_OK;
}
static int check_rolling(const hqt_handle* h, SampleCtx& c, const hqt_handle::Staged& s, const hqt_config& cf, int B) {
    const int n = c.n_steps;
    if (cf.cond_type == HQT_COND_TEXT && h->max_joins < 1) return fail(HQT_ERR_INVALID, "%s", ROLLING_TEXT_REFUSAL);      // (hqt_set_max_joins(0) behind the staging call)
    if (c.with_prefix) return fail(HQT_ERR_INVALID, "hqt_set_row_positions: the staged positions were taken by a prefix entry point; a rolling pass with a code prefix is not built (hqt_sample / hqt_sample_l3 take the table)");
    if (c.seg) return fail(HQT_ERR_INVALID, "hqt_set_row_positions together with a staged segment (hqt_set_segment) is not built: the k of the table is the call's span");
    if (c.keep && h->join_run < 0) return fail(HQT_ERR_INVALID, "hqt_set_row_positions together with a staged keep table (hqt_set_keep_mask) is not built");      // (unless hqt_set_join_run opted in)
    if (c.groups) return fail(HQT_ERR_INVALID, "hqt_set_row_positions together with a staged prompt-group table (hqt_set_prompt_groups) is not built");
    if ((int)s.roll.size() != B) return fail(HQT_ERR_INVALID, "hqt_set_row_positions staged a table of B=%d, this call has B=%d", (int)s.roll.size(), B);
    if (c.roll_k < 1 || c.roll_k > n) return fail(HQT_ERR_INVALID, "hqt_set_row_positions: k=%d outside [1, n_steps = %d]", c.roll_k, n);
    for (int b = 0; b < B; ++b)
        if (c.roll[b] < -1 || c.roll[b] > n - 1)
            return fail(HQT_ERR_INVALID, "hqt_set_row_positions: pos[%d]=%d outside [-1, n_steps - 1 = %d] (-1: an empty slot)", b, c.roll[b], n - 1);
    for (int i = 0; i < c.n_guide; ++i) {      // (rows outside [0, B) are refused below, by the pair checks of every call)
        const hqt_guide_pair& p = c.guide[i];
        if (p.pos_row < 0 || p.pos_row >= B || p.neg_row < 0 || p.neg_row >= B || c.roll[p.pos_row] == c.roll[p.neg_row]) continue;
        if (c.roll[p.pos_row] < 0 || c.roll[p.neg_row] < 0)
            return fail(HQT_ERR_INVALID, "guidance pair %d: exactly one of rows %d and %d is an empty slot of the rolling pass (positions %d and %d)", i, p.pos_row, p.neg_row, c.roll[p.pos_row], c.roll[p.neg_row]);
        return fail(HQT_ERR_INVALID, "guidance pair %d: rows %d and %d stand at different positions of the rolling pass (%d and %d): both rows of a pair draw one position", i, p.pos_row, p.neg_row,
                    c.roll[p.pos_row], c.roll[p.neg_row]);
    }
    // every slot against the rolling pass this handle holds: empty, a join at 0, or exactly where the slot stands
    const hqt_handle::Rolling& r = h->rolling;
    if (r.live) {
        if (r.B != B) return fail(HQT_ERR_STATE, "hqt_set_row_positions: the rolling pass has B=%d, this call has B=%d", r.B, B);
        if (r.n_steps != n) return fail(HQT_ERR_STATE, "hqt_set_row_positions: the rolling pass has n_steps=%d, this call has n_steps=%d", r.n_steps, n);
        if (r.levels != c.levels) return fail(HQT_ERR_STATE, "hqt_set_row_positions: the rolling pass has %d code levels, this call has %d", r.levels, c.levels);
        if (r.precision != c.precision) return fail(HQT_ERR_STATE, "hqt_set_row_positions: the rolling pass runs in precision %d, this call asks for precision %d (the cache holds that precision's type)", r.precision, c.precision);
    }
    for (int b = 0; b < B; ++b) {
        const int want = r.live ? r.next[b] : -1;
        if (c.roll[b] <= 0 || c.roll[b] == want) continue;
        if (!r.live) return fail(HQT_ERR_STATE, "hqt_set_row_positions: row %d continues at position %d, and this handle holds no rolling pass (none was begun, or another call has "
                                                "overwritten its cache since): every entry must be 0 (join) or -1 (empty)", b, c.roll[b]);
        if (want < 0) return fail(HQT_ERR_STATE, "hqt_set_row_positions: row %d continues at position %d, but the slot is empty in the rolling pass (0 joins, -1 stays empty)", b, c.roll[b]);
        return fail(HQT_ERR_STATE, "hqt_set_row_positions: row %d continues at position %d, but the slot stands at position %d of the rolling pass", b, c.roll[b], want);
    }
    c.start = 0; c.stop = c.roll_k;
    return c.keep ? HQT_OK : check_joins(h, c, cf, B);      // (a keep table: behind its own checks, check_keep)
}
// (the group table is asked about a prefix here, where that test has always stood: behind the rolling table, in front of the prefix's own)
static int check_prefix(const hqt_handle* h, const SampleCtx& c, const hqt_config& cf) {
    if (c.groups && c.with_prefix)
        return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups together with a code prefix (a prefix entry point) is not built: the prompt and the prefix are one prefill whose prefix rows differ per row");
    if (!c.with_prefix) return HQT_OK;
    if (cf.cond_type == HQT_COND_TEXT && c.levels == 3)
        return fail(HQT_ERR_INVALID, "a code prefix with text conditioning and three code levels is not built (two code levels are)");
    if (c.prefix_len < 1 || c.prefix_len >= c.n_steps)
        return fail(HQT_ERR_INVALID, "prefix_len=%d outside [1, n_steps - 1 = %d]: at least one position must be left to draw", c.prefix_len, c.n_steps - 1);
    if (c.prefix_len > h->max_prefix)
        return fail(HQT_ERR_INVALID, "prefix_len=%d exceeds max_prefix=%d of this handle (hqt_set_max_prefix sizes the body workspace for the prefill's rows)", c.prefix_len, h->max_prefix);
    for (int i = 0; i < c.levels; ++i) if (!c.prefix[i]) return fail(HQT_ERR_INVALID, "prefix codes of level %d are NULL", i);
    return HQT_OK;
}
static int check_keep(const hqt_handle* h, SampleCtx& c, const hqt_handle::Staged& s, const hqt_config& cf, int B) {
    if (c.with_prefix) return fail(HQT_ERR_INVALID, "hqt_set_keep_mask: the staged keep table was taken by a prefix entry point; a leading run of the mask is the prefix (hqt_sample / hqt_sample_l3 take the table)");
    if (s.keep_B != B || s.keep_n != c.n_steps)
        return fail(HQT_ERR_INVALID, "hqt_set_keep_mask staged a table of B=%d, n_steps=%d, this call has B=%d, n_steps=%d", s.keep_B, s.keep_n, B, c.n_steps);
    static const char* const fname[2][3] = {{"force_top", "force_bot", ""}, {"force0", "force1", "force2"}};
    for (int i = 0; i < c.levels; ++i)
        if (c.feed[i]) return fail(HQT_ERR_INVALID, "%s together with a keep table is not built: put the forced codes into the kept codes (hqt_set_keep_mask)", fname[c.levels == 3][i]);
    for (int i = 0; i < c.levels; ++i) if (!c.keep_codes[i]) return fail(HQT_ERR_INVALID, "hqt_set_keep_mask: kept codes of level %d are NULL", i);
    // a rolling call: no prefill over all rows; the run its joining rows share goes through the join phase (hqt_set_join_run)
    if (c.roll) return check_joins(h, c, cf, B);
    // the leading run every row shares goes through the one-pass prefix prefill, where it is built (hqt_set_max_prefix; not text with three code levels)
    int L = std::min(h->max_prefix, c.n_steps - 1);
    if (cf.cond_type == HQT_COND_TEXT && c.levels == 3) L = 0;
    for (int b = 0; b < B && L > 0; ++b) {
        int run = 0;
        while (run < L && c.keep[(size_t)b * c.n_steps + run]) ++run;
        L = run;
    }
    c.prefix_len = L;
    return HQT_OK;
}
static int check_groups(const hqt_handle* h, const SampleCtx& c, const hqt_handle::Staged& s, int B) {
    if ((int)s.groups.size() != B) return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups staged a table of B=%d, this call has B=%d", (int)s.groups.size(), B);
    if (c.prefix_len > 0)
        return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups together with a code prefix or a keep table whose rows share a leading run (prefix_len=%d) is not built: "
                                     "the prompt and the prefix are one prefill whose prefix rows differ per row", c.prefix_len);
    // (the staging holds n_groups prompts: the table and the buffer were sized together by hqt_set_prompt_groups)
    if (c.n_groups > h->pg_cap || !h->pg_k || !h->pg_v || !h->pg_x) return fail(HQT_ERR_STATE, "hqt_set_prompt_groups: the staging buffer holds %d prompts, the table has %d", h->pg_cap, c.n_groups);
    return HQT_OK;
}
static int check_samplers(SampleCtx& c, const hqt_handle::Staged& s, const hqt_config& cf, int B) {
    if (c.row_set) {                             // per-row settings replace the scalars of `opts`: those are neither checked nor part of the graph key
        if ((int)s.row_set.size() != B) return fail(HQT_ERR_INVALID, "hqt_set_row_samplers staged %d rows, this call has B=%d", (int)s.row_set.size(), B);
        for (int i = 0; i < 3; ++i) c.lv[i] = SamplerSet();
    }
    for (int b = 0; b < (c.row_set ? B : 1); ++b)
        for (int i = 0; i < c.levels; ++i) {
            const SamplerSet l = c.row_set ? SamplerSet{c.row_set[b].temperature[i], c.row_set[b].top_k[i], c.row_set[b].top_p[i]} : c.lv[i];
            if (!(l.temperature > 0.f)) return fail(HQT_ERR_INVALID, "temperatures must be > 0");
            c.top_p = c.top_p || l.top_p > 0.f;
        }
    if (c.top_p && cf.vocab_top > 8192) return fail(HQT_ERR_INVALID, "top-p needs vocab <= 8192");
    c.row_top_p = c.row_set && c.top_p;
    return HQT_OK;
}
static int check_guidance(const SampleCtx& c, const hqt_config& cf, int B) {
    if (cf.cond_type == HQT_COND_NONE) return fail(HQT_ERR_INVALID, "guidance needs a conditional model: this handle has cond_type HQT_COND_NONE, its rows have no condition to differ in");
    if ((c.row_seeds || c.row_offsets) && (!c.row_seeds || !c.row_offsets)) return fail(HQT_ERR_INVALID, "row_seeds and row_offsets come together");
    std::vector<char> paired(B, 0);
    for (int i = 0; i < c.n_guide; ++i) {
        const hqt_guide_pair& p = c.guide[i];
        if (p.pos_row < 0 || p.pos_row >= B || p.neg_row < 0 || p.neg_row >= B)
            return fail(HQT_ERR_INVALID, "guidance pair %d: rows (%d, %d) outside [0, B=%d)", i, p.pos_row, p.neg_row, B);
        if (p.pos_row == p.neg_row) return fail(HQT_ERR_INVALID, "guidance pair %d: pos_row == neg_row == %d", i, p.pos_row);
        if (paired[p.pos_row] || paired[p.neg_row])
            return fail(HQT_ERR_INVALID, "guidance pair %d: row %d appears in more than one pair", i, paired[p.pos_row] ? p.pos_row : p.neg_row);
        paired[p.pos_row] = paired[p.neg_row] = 1;
        for (int l = 0; l < c.levels; ++l)
            if (!std::isfinite(p.scale[l])) return fail(HQT_ERR_INVALID, "guidance pair %d: scale[%d] is not finite", i, l);
        // both rows must draw the same code from the same (guided) logits: same settings, same Philox key
        if (c.row_set && memcmp(&c.row_set[p.pos_row], &c.row_set[p.neg_row], sizeof(hqt_row_sampler)))
            return fail(HQT_ERR_INVALID, "guidance pair %d: rows %d and %d have different sampler settings in the staged row-sampler table", i, p.pos_row, p.neg_row);
        if (c.keep && memcmp(c.keep + (size_t)p.pos_row * c.n_steps, c.keep + (size_t)p.neg_row * c.n_steps, (size_t)c.n_steps))
            return fail(HQT_ERR_INVALID, "guidance pair %d: rows %d and %d have different rows in the staged keep table (both rows of a pair keep the same positions)", i, p.pos_row, p.neg_row);
        if (c.row_seeds && (c.row_seeds[p.pos_row] != c.row_seeds[p.neg_row] || c.row_offsets[p.pos_row] != c.row_offsets[p.neg_row]))
            return fail(HQT_ERR_INVALID, "guidance pair %d: row_seeds / row_offsets give rows %d and %d different keys (both rows of a pair must draw with one key)", i, p.pos_row, p.neg_row);
    }
    return HQT_OK;
}

// What the hqt_set_* calls staged, as the call reads it: the host tables stay with `s`
static void ctx_from_staged(SampleCtx& c, const hqt_handle::Staged& s) {
    c.row_set = s.row_set.empty() ? nullptr : s.row_set.data();
    c.logprob_out = s.logprob; c.report = s.report;
    c.guide = s.guide.empty() ? nullptr : s.guide.data(); c.n_guide = (int)s.guide.size();
    c.keep = s.keep.empty() ? nullptr : s.keep.data();
    for (int i = 0; i < 3; ++i) c.keep_codes[i] = s.keep_codes[i];
    c.groups = s.groups.empty() ? nullptr : s.groups.data(); c.n_groups = c.groups ? s.groups_G : 0;
    c.seg = s.seg; c.start = c.seg ? s.seg_start : 0; c.stop = c.seg ? s.seg_stop : c.n_steps;
    c.roll = s.roll.empty() ? nullptr : s.roll.data(); c.roll_k = s.roll_k;
}
// Behind a rolling call (`drew`: it ran steps; only empty slots draws and launches nothing): the positions drawn go to the caller's tensors, every slot's next one to the handle
static int finish_rolling(hqt_handle* h, const SampleCtx& c, int64_t* const* out, bool drew) {
    const int B = c.B;
    for (int i = 0; i < (drew ? c.levels : 0); ++i) {
        HIPCHK(launch_copy_row_positions(c.out[i], out[i], h->row_pos_received(), B, c.n_steps, LEVEL_WIDTH[i], 0, c.roll_k, c.st));
        // a row that joined through the join phase passed positions [0, L + 1 + k): those behind the first k through the join table (L for the joiners, -1 for every other row)
        if (c.n_join) HIPCHK(launch_copy_row_positions(c.out[i], out[i], h->row_pos_join(), B, c.n_steps, LEVEL_WIDTH[i], c.roll_k - c.join_len, c.roll_k + 1, c.st));
    }
    hqt_handle::Rolling& r = h->rolling;
    r.B = B; r.n_steps = c.n_steps; r.levels = c.levels; r.precision = c.precision;
    r.next.assign(B, -1);
    for (int b = 0; b < B; ++b) r.next[b] = rolled_to(c.roll[b], c.roll_k, c.n_steps, c.n_join > 0, c.join_len);
    r.live = std::any_of(r.next.begin(), r.next.end(), [](int32_t p) { return p >= 0; });      // every slot empty: the pass is over, nothing is left to match
    return HQT_OK;
}
// Behind a segment: its positions go to the caller's tensors, and a pass that is not finished stays on the handle as the paused one
static int finish_segment(hqt_handle* h, const SampleCtx& c, int64_t* const* out) {
    for (int i = 0; i < c.levels; ++i) HIPCHK(launch_copy_positions(c.out[i], out[i], c.B, c.n_steps, LEVEL_WIDTH[i], c.start, c.stop, c.st));
    if (c.stop < c.n_steps) h->paused = hqt_handle::Paused{true, c.B, c.n_steps, c.levels, c.precision, c.stop};
    return HQT_OK;
}
static int copy_out(const SampleCtx& c, int64_t* const* out) {
    for (int i = 0; i < c.levels; ++i) HIPCHK(hipMemcpyAsync(out[i], c.out[i], (size_t)c.B * c.n_steps * LEVEL_WIDTH[i] * 8, hipMemcpyDeviceToDevice, c.st));
    return HQT_OK;
}

// hqt_sample / hqt_sample_l3 after their null checks: `c` holds the call's options, sampler settings and forced codes (feed); validates them,
// runs the call and copies the drawn codes of every level out
static int sample_call(hqt_handle* h, SampleCtx& c, const int64_t* cond, int64_t* const* out, void* stream) {
    // what was staged belongs to THIS call and to no later one, whatever becomes of the call; `s` owns the host tables until it returns
    const hqt_handle::Staged s = h->take_staged();
    ctx_from_staged(c, s);
    if (!h->finalized) return fail(HQT_ERR_STATE, "hqt_finalize_weights has not run");
    const hqt_config& cf = h->cfg;
    if (c.levels == 2 && !cf.has_stage2) return fail(HQT_ERR_STATE, "handle was created without stage 2");
    if (c.levels == 2 && cf.code_levels == 3) return fail(HQT_ERR_STATE, "three-level model: use hqt_sample_l3");
    if (c.levels == 3 && (!cf.has_stage2 || cf.code_levels != 3)) return fail(HQT_ERR_STATE, "handle does not hold a three-level stage 2");
    const int B = c.B;
    if (B < 1 || B > cf.max_batch) return fail(HQT_ERR_INVALID, "B=%d outside [1, max_batch=%d]", B, cf.max_batch);
    if (c.n_steps < 1 || c.n_steps > cf.max_steps) return fail(HQT_ERR_INVALID, "n_steps=%d outside [1, %d]", c.n_steps, cf.max_steps);
    if (cf.cond_type != HQT_COND_NONE && !cond) return fail(HQT_ERR_INVALID, "cond is required for class/text conditioning");
    if (c.report.top_n > cf.vocab_top)
        return fail(HQT_ERR_INVALID, "hqt_set_draw_report staged top_n=%d, this model's vocabulary has %d codes", c.report.top_n, cf.vocab_top);
    if (c.seg) CHK(check_segment(h, c, B));
    if (c.roll) CHK(check_rolling(h, c, s, cf, B));
    CHK(check_prefix(h, c, cf));
    if (c.keep) CHK(check_keep(h, c, s, cf, B));
    if (c.groups) CHK(check_groups(h, c, s, B));
    CHK(check_samplers(c, s, cf, B));
    if (c.guide) CHK(check_guidance(c, cf, B));
    ON_DEVICE(h);
    // The launch sequence reads cond and writes the drawn codes in buffers owned by the handle, and takes the Philox seed and the global row offset from device memory: nothing
    // that changes from call to call is baked into the captured graph, so a steady stream of batches replays ONE graph (no re-capture, no exec destroyed under pending launches).
    int64_t* codes[3] = {h->codes_top, h->codes_bot, h->codes_l2};
    for (int i = 0; i < c.levels; ++i) { c.out[i] = codes[i]; if (!c.feed[i]) c.feed[i] = codes[i]; }
    c.cond = cond ? h->cond_buf : nullptr; c.st = (hipStream_t)stream;
    CHK(mode_of(c.precision, false, &c.md));
    CHK(layout_check(h, c.md));
    // (a group table: cond is [n_groups, ctx_len_txt], n_groups <= B)
    if (cond) HIPCHK(hipMemcpyAsync(h->cond_buf, cond, (size_t)(c.groups ? c.n_groups : B) * (cf.cond_type == HQT_COND_TEXT ? cf.ctx_len_txt : 1) * 8, hipMemcpyDefault, c.st));
    // the prefix goes into the handle's code buffers (outside any captured graph): the prefill's embedding, the embedding of position
    // prefix_len + 1 and the copies below read it there
    for (int i = 0; i < (c.prefix_len && !c.keep ? c.levels : 0); ++i)
        HIPCHK(launch_copy_prefix(c.prefix[i], codes[i], B, c.prefix_len, c.n_steps, LEVEL_WIDTH[i], cf.vocab_top, c.st));
    // whatever this call is, it writes the body cache and the step state: a paused pass is over, or goes on below and is recorded anew behind its segment
    h->paused.live = false;
    h->rolling.live = false;                     // ... and so is a rolling pass, unless this call is its next one (recorded anew below)
    if (c.roll) {
        c.row_pos = h->row_pos;
        for (int i = 0; i < c.levels; ++i) c.roll_prev[i] = out[i];
        const bool any = std::any_of(c.roll, c.roll + B, [](int32_t p) { return p >= 0; });
        if (any) CHK(sample_run(h, c));
        return finish_rolling(h, c, out, any);
    }
    // a continuation reads the codes of position start - 1 where the caller holds them: a level that is not forced takes them from out_* (the caller may have
    // edited them, or gathered its rows along with hqt_select_rows)
    for (int i = 0; i < (c.start > 0 ? c.levels : 0); ++i)
        if (c.feed[i] == codes[i]) HIPCHK(launch_copy_positions(out[i], codes[i], B, c.n_steps, LEVEL_WIDTH[i], c.start - 1, c.start, c.st));
    CHK(sample_run(h, c));
    return c.seg ? finish_segment(h, c, out) : copy_out(c, out);
}

// the options both entry points share
template <class Opts> static SampleCtx sample_ctx(int levels, int B, const Opts* o, const float* noise, float* logits_out) {
    SampleCtx c{};
    c.levels = levels; c.B = B; c.noise = noise; c.logits_out = logits_out;
    c.precision = o->precision; c.n_steps = o->n_steps; c.use_graph = o->use_graph;
    c.seed = o->seed; c.sample_offset = o->sample_offset; c.row_seeds = o->row_seeds; c.row_offsets = o->row_offsets;
    return c;
}

static_assert(sizeof(hqt_row_sampler) == 36 && sizeof(RowSampler) == sizeof(hqt_row_sampler), "hqt_row_sampler is copied to the device as RowSampler");

extern "C" int hqt_set_logprob_out(hqt_handle* h, float* logprobs) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.logprob = logprobs;                // NULL clears; the shape [B, n_steps, draws] is the taking call's (the caller sizes the buffer for it)
    return HQT_OK;
}

static_assert(sizeof(hqt_draw_report) == 40 && HQT_REPORT_MAX_TOP == 16, "hqt_draw_report: four pointers and top_n; the per-thread taken-mask of the kernel holds 64 bits");

extern "C" int hqt_set_draw_report(hqt_handle* h, const hqt_draw_report* r) {
    if (h) h->staged.report = {nullptr, nullptr, 0, nullptr, nullptr};     // r == NULL, nothing to write, or a struct that is refused: nothing stays staged
    if (!r) return h ? HQT_OK : fail(HQT_ERR_INVALID, "null handle");
    // (the struct first: what is wrong with it does not depend on the handle)
    if (r->top_n < 0 || r->top_n > HQT_REPORT_MAX_TOP)
        return fail(HQT_ERR_INVALID, "hqt_set_draw_report: top_n=%d outside [0, HQT_REPORT_MAX_TOP = %d]", r->top_n, HQT_REPORT_MAX_TOP);
    if (r->top_n > 0 && !r->top_codes) return fail(HQT_ERR_INVALID, "hqt_set_draw_report: top_n=%d and top_codes is NULL", r->top_n);
    if (r->top_n > 0 && !r->top_logprobs) return fail(HQT_ERR_INVALID, "hqt_set_draw_report: top_n=%d and top_logprobs is NULL", r->top_n);
    if (r->top_n == 0 && r->top_codes) return fail(HQT_ERR_INVALID, "hqt_set_draw_report: top_codes is set and top_n is 0");
    if (r->top_n == 0 && r->top_logprobs) return fail(HQT_ERR_INVALID, "hqt_set_draw_report: top_logprobs is set and top_n is 0");
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.report = {r->entropy, r->rank, r->top_n, r->top_codes, r->top_logprobs};     // the shapes are the taking call's (the caller sizes the buffers for it)
    return HQT_OK;
}

static_assert(sizeof(hqt_guide_pair) == 20 && sizeof(GuidePair) == sizeof(hqt_guide_pair), "hqt_guide_pair is copied to the device as GuidePair");

extern "C" int hqt_set_guidance(hqt_handle* h, int n_pairs, const hqt_guide_pair* pairs) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.guide.clear();
    if (n_pairs == 0 || !pairs) return HQT_OK;
    if (n_pairs < 0 || 2 * (long long)n_pairs > h->cfg.max_batch)
        return fail(HQT_ERR_INVALID, "n_pairs=%d outside [0, max_batch / 2 = %d]: a pair takes two rows of the pass", n_pairs, h->cfg.max_batch / 2);
    h->staged.guide.assign(pairs, pairs + n_pairs);      // rows, scales and keys are checked by the call that takes it
    return HQT_OK;
}

extern "C" int hqt_set_keep_mask(hqt_handle* h, int B, int n_steps, const uint8_t* keep, const int64_t* const* codes) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.keep.clear();
    if (B == 0 || !keep) return HQT_OK;
    if (B < 0 || B > h->cfg.max_batch) return fail(HQT_ERR_INVALID, "hqt_set_keep_mask: B=%d outside [0, max_batch=%d]", B, h->cfg.max_batch);
    if (n_steps < 1 || n_steps > h->cfg.max_steps) return fail(HQT_ERR_INVALID, "hqt_set_keep_mask: n_steps=%d outside [1, max_steps=%d]", n_steps, h->cfg.max_steps);
    if (!codes) return fail(HQT_ERR_INVALID, "hqt_set_keep_mask: codes is NULL");
    const int levels = h->cfg.code_levels == 3 ? 3 : 2;
    hqt_handle::Staged& s = h->staged;
    for (int i = 0; i < 3; ++i) s.keep_codes[i] = i < levels ? codes[i] : nullptr;      // a NULL level is refused by the call that takes the table
    s.keep_B = B; s.keep_n = n_steps;
    s.keep.resize((size_t)B * n_steps);
    for (size_t i = 0; i < s.keep.size(); ++i) s.keep[i] = keep[i] ? 1 : 0;
    return HQT_OK;
}

extern "C" int hqt_set_row_samplers(hqt_handle* h, int n, const hqt_row_sampler* rows) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.row_set.clear();
    if (n == 0 || !rows) return HQT_OK;
    if (n < 0 || n > h->cfg.max_batch) return fail(HQT_ERR_INVALID, "n=%d outside [0, max_batch=%d]", n, h->cfg.max_batch);
    h->staged.row_set.assign(rows, rows + n);    // checked against B, the levels and the vocabulary by the call that takes it
    return HQT_OK;
}

// Stages the group table of a shared prefill and sizes the staging for its n_groups prompts (reserve_prompt_staging: grown, never shrunk).  A sampling call
// allocates nothing.
extern "C" int hqt_set_prompt_groups(hqt_handle* h, int B, int n_groups, const int32_t* group_of_row) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.groups.clear();
    const hqt_config& c = h->cfg;
    if (!c.has_stage2 || c.cond_type != HQT_COND_TEXT)
        return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups: the handle is not text-conditional (cond_type %d): one embedding row per sample leaves no prefill to share", c.cond_type);
    if (!group_of_row) return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups: group_of_row is NULL");
    if (B < 1 || B > c.max_batch) return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups: B=%d outside [1, max_batch=%d]", B, c.max_batch);
    if (n_groups < 1 || n_groups > c.max_batch) return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups: n_groups=%d outside [1, max_batch=%d]", n_groups, c.max_batch);
    if (n_groups > B) return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups: n_groups=%d exceeds B=%d (a prompt no row carries would be prefilled for nothing)", n_groups, B);
    for (int b = 0; b < B; ++b)
        if (group_of_row[b] < 0 || group_of_row[b] >= n_groups)
            return fail(HQT_ERR_INVALID, "hqt_set_prompt_groups: group_of_row[%d]=%d outside [0, n_groups=%d)", b, group_of_row[b], n_groups);
    if (!h->finalized) return fail(HQT_ERR_STATE, "hqt_finalize_weights has not run");
    ON_DEVICE(h);
    CHK(reserve_prompt_staging(h, n_groups));
    h->staged.groups_G = n_groups;
    h->staged.groups.assign(group_of_row, group_of_row + B);
    return HQT_OK;
}

// Opt-in sizing of rolling passes on a text handle: the staging that the prompt prefill of up to max_joins joining rows per call needs (the buffers of
// hqt_set_prompt_groups, sized to the larger of the two needs).  0 switches rolling off again and frees nothing.
extern "C" int hqt_set_max_joins(hqt_handle* h, int max_joins) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    const hqt_config& c = h->cfg;
    if (!c.has_stage2 || c.cond_type != HQT_COND_TEXT)
        return fail(HQT_ERR_INVALID, "hqt_set_max_joins: the handle is not text-conditional (cond_type %d): a row of any other model joins a rolling pass without a prefill", c.cond_type);
    if (max_joins < 0 || max_joins > c.max_batch) return fail(HQT_ERR_INVALID, "hqt_set_max_joins: max_joins=%d outside [0, max_batch=%d]", max_joins, c.max_batch);
    if (h->rolling.live) return fail(HQT_ERR_STATE, "hqt_set_max_joins: this handle holds a rolling pass (hqt_set_row_positions); finish it first");
    ON_DEVICE(h);
    if (max_joins > 0) CHK(reserve_prompt_staging(h, max_joins));
    h->max_joins = max_joins;
    return HQT_OK;
}

// Opt-in sizing of rolling calls that take a keep table (hqt_set_keep_mask): up to max_joins rows per call join through the join phase, which prefills a leading kept
// run of up to max_run positions that they share (hqt_set_max_prefix has sized the body workspace for such a pass).  Grows the staging of staged_prompt_prefill to
// max_joins * ((ctx_len_txt | 1) + max_run) rows; without text and with max_run == 0 no join phase ever runs and nothing is allocated.  On a text handle it is also
// hqt_set_max_joins(h, max_joins).  0 joins switch the opt-in off again and free nothing.
extern "C" int hqt_set_join_run(hqt_handle* h, int max_joins, int max_run) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    const hqt_config& c = h->cfg;
    const bool text = c.cond_type == HQT_COND_TEXT;
    if (!c.has_stage2) return fail(HQT_ERR_INVALID, "hqt_set_join_run: the handle was created without stage 2");
    if (max_joins < 0 || max_joins > c.max_batch) return fail(HQT_ERR_INVALID, "hqt_set_join_run: max_joins=%d outside [0, max_batch=%d]", max_joins, c.max_batch);
    if (max_run < 0 || max_run > h->max_prefix)
        return fail(HQT_ERR_INVALID, "hqt_set_join_run: max_run=%d outside [0, max_prefix=%d] of this handle (hqt_set_max_prefix sizes the body workspace for the prefill's rows)", max_run, h->max_prefix);
    if (max_run > 0 && text && c.code_levels == 3)
        return fail(HQT_ERR_INVALID, "hqt_set_join_run: max_run=%d with text conditioning and three code levels is not built (the prefix prefill is not; max_run = 0 is)", max_run);
    if (h->rolling.live) return fail(HQT_ERR_STATE, "hqt_set_join_run: this handle holds a rolling pass (hqt_set_row_positions); finish it first");
    ON_DEVICE(h);
    if (max_joins > 0 && (text || max_run > 0)) CHK(reserve_prompt_staging(h, max_joins, h->staging_rows(max_run)));
    h->join_run = max_joins > 0 ? max_run : -1;
    h->max_joins = max_joins;                    // (a text handle: hqt_set_max_joins(h, max_joins) as well; any other reads it in the join phase only)
    return HQT_OK;
}

extern "C" int hqt_set_row_positions(hqt_handle* h, int B, const int32_t* pos, int k) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.roll.clear();
    h->staged.roll_k = 0;
    if (B == 0 || !pos) return HQT_OK;
    const hqt_config& c = h->cfg;
    if (!c.has_stage2) return fail(HQT_ERR_INVALID, "hqt_set_row_positions: the handle was created without stage 2");
    if (c.cond_type == HQT_COND_TEXT && h->max_joins < 1) return fail(HQT_ERR_INVALID, "%s", ROLLING_TEXT_REFUSAL);
    if (B < 1 || B > c.max_batch) return fail(HQT_ERR_INVALID, "hqt_set_row_positions: B=%d outside [1, max_batch=%d]", B, c.max_batch);
    if (k < 1 || k > c.max_steps) return fail(HQT_ERR_INVALID, "hqt_set_row_positions: k=%d outside [1, n_steps] (n_steps <= max_steps = %d)", k, c.max_steps);
    for (int b = 0; b < B; ++b)
        if (pos[b] < -1 || pos[b] > c.max_steps - 1)
            return fail(HQT_ERR_INVALID, "hqt_set_row_positions: pos[%d]=%d outside [-1, n_steps - 1] (n_steps <= max_steps = %d; -1: an empty slot)", b, pos[b], c.max_steps);
    h->staged.roll.assign(pos, pos + B);         // checked against B, n_steps and the rolling pass by the call that takes it
    h->staged.roll_k = k;
    return HQT_OK;
}

extern "C" int hqt_set_segment(hqt_handle* h, int start, int stop) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    h->staged.seg = true;                        // checked against n_steps and the paused pass by the call that takes it
    h->staged.seg_start = start; h->staged.seg_stop = stop;
    return HQT_OK;
}

// The rows of a paused pass re-mapped: one gather of the live cache rows along the batch axis (K and V of every body layer, in the paused precision's
// type).  Between two positions nothing else of a row lives in the handle: the depth cache is rebuilt every position, the step state is shared by all
// rows, the codes are the caller's.  Allocates nothing: the table travels through the pinned ring into the group table's device buffer (a prefill's, free here).
extern "C" int hqt_select_rows(hqt_handle* h, int B_new, const int32_t* rows_from, void* stream) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    const hqt_config& cf = h->cfg;
    const hqt_handle::Paused& p = h->paused;
    if (h->rolling.live) return fail(HQT_ERR_STATE, "hqt_select_rows: this handle holds a rolling pass (hqt_set_row_positions), whose slots are reused in place; re-mapping its rows is not built");
    if (!p.live) return fail(HQT_ERR_STATE, "hqt_select_rows: this handle holds no paused pass (hqt_set_segment with stop < n_steps leaves one)");
    if (!rows_from) return fail(HQT_ERR_INVALID, "hqt_select_rows: rows_from is NULL");
    if (B_new < 1 || B_new > cf.max_batch) return fail(HQT_ERR_INVALID, "hqt_select_rows: B_new=%d outside [1, max_batch=%d]", B_new, cf.max_batch);
    for (int j = 0; j < B_new; ++j)
        if (rows_from[j] < 0 || rows_from[j] >= p.B)
            return fail(HQT_ERR_INVALID, "hqt_select_rows: rows_from[%d]=%d outside [0, B=%d) of the paused pass", j, rows_from[j], p.B);
    if ((size_t)B_new * 16 > kv_gather_lds_limit())
        return fail(HQT_ERR_INVALID, "hqt_select_rows: B_new=%d rows of 16 bytes do not fit the %d KiB of LDS of a compute unit (at most %d rows)", B_new,
                    (int)(kv_gather_lds_limit() / 1024), (int)(kv_gather_lds_limit() / 16));
    Mode md;
    CHK(mode_of(p.precision, false, &md));
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    // live keys: the step state says (pos, t_base) with t_base = pos for class / no conditioning, ctx_len_txt + pos - 1 for text (the prefill drew position 0)
    const int t_live = cf.cond_type == HQT_COND_TEXT ? cf.ctx_len_txt + p.pos - 1 : p.pos;
    if (t_live < 1 || t_live > h->Tmax) return fail(HQT_ERR_STATE, "hqt_select_rows: %d live cache rows outside [1, %d]", t_live, h->Tmax);
    int slot = 0;
    RingSlot ring;
    CHK(rows_ring_take(h, &slot, &ring));
    CHK(ring_send(ring.groups, rows_from, (size_t)B_new, h->group_of_row, st));
    CHK(ring_sent(h, slot, st));
    {
        Timed t(h, "kv_gather_rows", st);
        const long long row_bytes = (long long)cf.embed_dim * (long long)md.act_sz();
        const KvGatherArgs ga{h->kcache, h->vcache, h->group_of_row, cf.n_layers, B_new, cf.max_batch, (long long)h->Tmax * row_bytes, (long long)t_live * row_bytes};
        HIPCHK(launch_kv_gather_rows(ga, st));
    }
    h->paused.B = B_new;
    return HQT_OK;
}

// prefix_len < 0: no prefix (hqt_sample / hqt_sample_l3); otherwise the call came through a prefix entry point and prefix_len is validated
static int sample2(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts* opts, const float* noise, int prefix_len,
                   const int64_t* prefix_top, const int64_t* prefix_bot, const int64_t* force_top, const int64_t* force_bot,
                   float* logits_out, int64_t* out_top, int64_t* out_bot, void* stream) {
    if (h && (!opts || !out_top || !out_bot)) h->clear_staged();
    if (!h || !opts || !out_top || !out_bot) return fail(HQT_ERR_INVALID, "null argument");
    SampleCtx c = sample_ctx(2, B, opts, noise, logits_out);
    c.lv[0] = {opts->temperature_top, opts->top_k_top, opts->top_p_top};
    c.lv[1] = {opts->temperature_bot, opts->top_k_bot, opts->top_p_bot};
    c.feed[0] = force_top; c.feed[1] = force_bot;
    if (prefix_len >= 0) { c.with_prefix = true; c.prefix_len = prefix_len; c.prefix[0] = prefix_top; c.prefix[1] = prefix_bot; }
    int64_t* const out[2] = {out_top, out_bot};
    return sample_call(h, c, cond, out, stream);
}

static int sample3(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts_l3* opts, const float* noise, int prefix_len,
                   const int64_t* const* prefix, const int64_t* force0, const int64_t* force1, const int64_t* force2, float* logits_out,
                   int64_t* out0, int64_t* out1, int64_t* out2, void* stream) {
    if (h && (!opts || !out0 || !out1 || !out2)) h->clear_staged();
    if (!h || !opts || !out0 || !out1 || !out2) return fail(HQT_ERR_INVALID, "null argument");
    SampleCtx c = sample_ctx(3, B, opts, noise, logits_out);
    for (int i = 0; i < 3; ++i) c.lv[i] = {opts->temperature[i], opts->top_k[i], opts->top_p[i]};
    c.feed[0] = force0; c.feed[1] = force1; c.feed[2] = force2;
    if (prefix_len >= 0) { c.with_prefix = true; c.prefix_len = prefix_len; for (int i = 0; i < 3; ++i) c.prefix[i] = prefix[i]; }
    int64_t* const out[3] = {out0, out1, out2};
    return sample_call(h, c, cond, out, stream);
}

extern "C" int hqt_sample(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts* opts, const float* noise,
                          const int64_t* force_top, const int64_t* force_bot, float* logits_out, int64_t* out_top,
                          int64_t* out_bot, void* stream) {
    return sample2(h, B, cond, opts, noise, -1, nullptr, nullptr, force_top, force_bot, logits_out, out_top, out_bot, stream);
}

extern "C" int hqt_sample_prefix(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts* opts, const float* noise,
                                 int prefix_len, const int64_t* prefix_top, const int64_t* prefix_bot,
                                 const int64_t* force_top, const int64_t* force_bot, float* logits_out,
                                 int64_t* out_top, int64_t* out_bot, void* stream) {
    return sample2(h, B, cond, opts, noise, std::max(prefix_len, 0), prefix_top, prefix_bot, force_top, force_bot, logits_out, out_top, out_bot, stream);
}

extern "C" int hqt_sample_l3(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts_l3* opts, const float* noise,
                             const int64_t* force0, const int64_t* force1, const int64_t* force2, float* logits_out,
                             int64_t* out0, int64_t* out1, int64_t* out2, void* stream) {
    return sample3(h, B, cond, opts, noise, -1, nullptr, force0, force1, force2, logits_out, out0, out1, out2, stream);
}

extern "C" int hqt_sample_prefix_l3(hqt_handle* h, int B, const int64_t* cond, const hqt_sample_opts_l3* opts, const float* noise,
                                    int prefix_len, const int64_t* prefix0, const int64_t* prefix1, const int64_t* prefix2,
                                    const int64_t* force0, const int64_t* force1, const int64_t* force2, float* logits_out,
                                    int64_t* out0, int64_t* out1, int64_t* out2, void* stream) {
    const int64_t* const prefix[3] = {prefix0, prefix1, prefix2};
    return sample3(h, B, cond, opts, noise, std::max(prefix_len, 0), prefix, force0, force1, force2, logits_out, out0, out1, out2, stream);
}

// hqt_score: the log-probability of GIVEN codes in one teacher-forced pass (the reference's eval-mode forward, hierarchical_ar.py:246-426,
// hqtransformer.py:226-407).  Body (score_body): the prefix prefill with P = n - 1 -- copy_prefix, embed_prefix (text: embed_text + the prefix rows), run_body with t_base = 0
// over n (text: T + n - 1) rows per sample, the classic LayerNorm path (a single row per sample, n = 1 without text, is the decode step's embedding and may take the deferred
// one; never the persistent chain: the step state is not where t_base comes from).  Depth (score_depth_chunk): a (sample, position) pair p = b n + t is a depth "sample";
// chunks of at most score_chunk pairs (default max_batch).  Eager, no graph.  score_check: what the call refuses, in this order.
static int score_check(const hqt_handle* h, bool staged, int B, const int64_t* cond, const int64_t* const* codes, int n, const float* logprobs, const ReportOut& report) {
    if (staged) return fail(HQT_ERR_STATE, "hqt_score: a row-sampler table, guidance pair table, keep table, prompt-group table or log-probability buffer was staged on this handle "
                            "(hqt_set_row_samplers / hqt_set_guidance / hqt_set_logprob_out / hqt_set_keep_mask / hqt_set_prompt_groups): they belong to a sampling call and were cleared");
    if (!logprobs) return fail(HQT_ERR_INVALID, "hqt_score: logprobs is NULL");
    if (!codes) return fail(HQT_ERR_INVALID, "hqt_score: codes is NULL");
    if (!h->finalized) return fail(HQT_ERR_STATE, "hqt_finalize_weights has not run");
    const hqt_config& cf = h->cfg;
    if (!cf.has_stage2) return fail(HQT_ERR_STATE, "handle was created without stage 2");
    const int levels = cf.code_levels == 3 ? 3 : 2;
    for (int i = 0; i < levels; ++i) if (!codes[i]) return fail(HQT_ERR_INVALID, "hqt_score: codes of level %d are NULL", i);
    if (cf.depth_decoding == HQT_DEPTH_TOP2MID2BOT)
        return fail(HQT_ERR_INVALID, "hqt_score: the 'top2mid2bot' depth head (21 causal sub-steps per position) is not built for the one-pass score: force the codes through hqt_sample_l3");
    const bool text = cf.cond_type == HQT_COND_TEXT;
    if (text && levels == 3) return fail(HQT_ERR_INVALID, "hqt_score: text conditioning with three code levels is not built (two code levels are)");
    if (B < 1 || B > cf.max_batch) return fail(HQT_ERR_INVALID, "B=%d outside [1, max_batch=%d]", B, cf.max_batch);
    if (n < 1 || n > cf.max_steps) return fail(HQT_ERR_INVALID, "n=%d outside [1, %d]", n, cf.max_steps);
    if (cf.cond_type != HQT_COND_NONE && !cond) return fail(HQT_ERR_INVALID, "cond is required for class/text conditioning");
    if (report.top_n > cf.vocab_top)
        return fail(HQT_ERR_INVALID, "hqt_set_draw_report staged top_n=%d, this model's vocabulary has %d codes", report.top_n, cf.vocab_top);
    if (n - 1 > h->max_prefix)
        return fail(HQT_ERR_STATE, "hqt_score: n=%d positions need max_prefix >= %d, this handle has %d (hqt_set_max_prefix sizes the body workspace for the pass's rows)", n, n - 1, h->max_prefix);
    return HQT_OK;
}
// hqt_score's body pass over the codes in the handle's buffers: n rows per sample (text: the T prompt rows, then the input rows of positions 1 .. n - 1); *Tq: those rows
static int score_body(hqt_handle* h, const SampleCtx& c, int* Tq) {
    if (h->cfg.cond_type == HQT_COND_TEXT || c.n_steps > 1) CHK(embed_prefill(h, c, c.feed, c.n_steps - 1, Tq));
    else CHK(embed_step(h, c));                    // one row per sample (*Tq stays 1): the decode step's embedding at step 0
    bool pfull = false;
    CHK(run_body(h, c, *Tq, 0, false, false, &pfull));
    return fold_pending(h, c, c.B * *Tq);
}
// The depth head over the np = cc.B pairs [p0, p0 + np) of the score pass (pair p = b n + t reads body row b Tq + row_off + t): the sub-step schedule of
// run_depth_head -- input rows, run_depth with the pair count as batch, run_head, the log-probabilities -- with no sampler, no guidance and no draws
static int score_depth_chunk(hqt_handle* h, const SampleCtx& cc, int p0, int Tq, int row_off, float* logprobs, float* const* logits_out, const ReportOut& report) {
    const hqt_config& cf = h->cfg;
    const int D = cf.embed_dim, V = cf.vocab_top, np = cc.B, n = cc.n_steps, draws = h->depth_rows;
    const bool bidir = cf.depth_decoding == HQT_DEPTH_BIDIRECTIONAL;
    const int dmul = cf.depth_decoding == HQT_DEPTH_PARALLEL_REDUCE ? 4 : 1;
    // ln_f of every pair's body row + sos_depth -> the input rows of sub-step 0: M = np, or the bidirectional pass's 5 np, four rows behind each `fill`ed with the depth positions
    auto depth_input = [&](bool dln, int M, const float* fill) {
        Timed t(h, "score_depth_input", cc.st);
        LNArgs ln{h->x, W(h, "ln_f.weight"), W(h, "ln_f.bias"), W(h, "sos_depth"), h->xd, np, D, 1, 0, 1e-5f, DT_F32, 0,
                  nullptr, 0, 0, nullptr, dln ? h->xdpk : nullptr, dln ? packed_mb(M) : 0, h->partsd};
        ln.fill = fill;
        HIPCHK(launch_score_depth_input(ln, p0, n, Tq, row_off, cc.st));
        h->npartsd = 1;
        return (int)HQT_OK;
    };
    void* normed[3] = {nullptr, nullptr, nullptr};
    if (bidir) {                  // one pass of the depth blocks over five rows per pair (run_depth_head)
        const int M = np * h->depth_rows;
        const bool dln = dln_ok(h, cc, h->depth[0], M);
        CHK(depth_input(dln, M, W(h, "pos_emb_depth.weight")));
        CHK(run_bidir_tail(h, cc, dln, normed));
    }
    for (int sub = 0; sub < cc.levels; ++sub) {
        const SubStep s = sub_step(cf, sub);
        const int M = np * s.Tq;
        const bool dln = depth_dln(h, cc, s);
        if (!bidir) {
            bf16_t* xpk = dln ? h->xdpk : nullptr;
            const int pk = dln ? packed_mb(M) : 0;
            if (sub == 0) {
                CHK(depth_input(dln, M, nullptr));
            } else {
                Timed t(h, "embed", cc.st);
                if (sub == 1) HIPCHK(launch_score_depth_embed(cc.feed[0], p0, np, W(h, "tok_emb_top_depth.weight"), W(h, "pos_emb_depth.weight"), h->xd, D, xpk, pk, h->partsd, cc.st, V, dmul * D));
                else HIPCHK(launch_score_depth_embed_l2(cc.feed[0], cc.feed[1], p0, np, cf.depth_decoding == HQT_DEPTH_PARALLEL_ADD ? W(h, "tok_emb_top_depth.weight") : nullptr,
                                                        W(h, "tok_emb_depth_levels.1.weight"), W(h, "pos_emb_depths.1.weight"), h->xd, D, xpk, pk, h->partsd, cc.st, V, dmul * D));
            }
            h->npartsd = 1;
            CHK(run_depth(h, cc, dln, s.Tq, s.tbase));
        }
        // the head GEMM writes the caller's buffer directly where one is given: rows of a level are contiguous over pairs
        float* lg = (logits_out && logits_out[s.lv]) ? logits_out[s.lv] + (size_t)p0 * s.Tq * V : h->logits;
        CHK(run_head(h, cc, head_of(h, s.lv), s.lv, M, dln, normed[s.lv], lg));
        {
            Timed t(h, "score_logprob", cc.st);
            HIPCHK(launch_score_logprob(lg, cc.feed[s.lv] + (size_t)p0 * s.Tq, logprobs + (size_t)p0 * draws, np, V, s.Tq, s.tbase, draws, cc.st));
        }
        if (report.any()) {       // the chunk's (pair, slot) rows of this level in one launch, over the logits the log-probabilities were read from
            Timed t(h, "draw_report", cc.st);
            HIPCHK(launch_score_report(lg, cc.feed[s.lv] + (size_t)p0 * s.Tq, report, p0, np, V, s.Tq, s.tbase, draws, cc.st));
        }
    }
    return HQT_OK;
}

extern "C" int hqt_score(hqt_handle* h, int B, const int64_t* cond, const int64_t* const* codes, int n, int precision, float* logprobs,
                         float* const* logits_out, void* stream) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    // a staged table or buffer belongs to a sampling call: it must not wait for a later one behind this call
    const bool staged = h->staged.holds_table();
    const ReportOut report = h->staged.report;     // a staged draw report is this call's (hqt_set_draw_report); taken and cleared whatever becomes of the call
    h->clear_staged();
    CHK(score_check(h, staged, B, cond, codes, n, logprobs, report));
    const hqt_config& cf = h->cfg;
    const bool text = cf.cond_type == HQT_COND_TEXT;
    SampleCtx c{};
    c.levels = cf.code_levels == 3 ? 3 : 2; c.B = B; c.n_steps = n; c.precision = precision; c.st = (hipStream_t)stream;
    CHK(mode_of(precision, false, &c.md));
    CHK(layout_check(h, c.md));
    ON_DEVICE(h);
    int64_t* const own[3] = {h->codes_top, h->codes_bot, h->codes_l2};
    if (cond) HIPCHK(hipMemcpyAsync(h->cond_buf, cond, (size_t)B * (text ? cf.ctx_len_txt : 1) * 8, hipMemcpyDefault, c.st));
    c.cond = cond ? h->cond_buf : nullptr;
    for (int i = 0; i < c.levels; ++i) {           // [B, n, width]: the handle's code buffers hold the pairs contiguously, pair p at index p
        HIPCHK(launch_copy_prefix(codes[i], own[i], B, n, n, LEVEL_WIDTH[i], cf.vocab_top, c.st));
        c.feed[i] = own[i]; c.out[i] = own[i];
    }
    h->paused.live = false;                        // the pass overwrites the body cache and the step state: a paused pass (hqt_set_segment) is over
    h->rolling.live = false;                       // ... and so is a rolling pass (hqt_set_row_positions)
    HIPCHK(launch_set_step(h->state, 0, 0, c.st));
    int Tq = 1;
    CHK(score_body(h, c, &Tq));
    // the depth head in chunks of pairs; body row of pair (b, t): b Tq + row_off + t
    const int row_off = text ? cf.ctx_len_txt - 1 : 0, chunk = h->score_chunk > 0 ? h->score_chunk : cf.max_batch, total = B * n;
    SampleCtx cc = c;
    for (int p0 = 0; p0 < total; p0 += chunk) {
        cc.B = std::min(chunk, total - p0);
        CHK(score_depth_chunk(h, cc, p0, Tq, row_off, logprobs, logits_out, report));
    }
    return HQT_OK;
}

// Persistent launches need every compute unit of the device: two of them in flight at once (two root handles sampling on two streams)
// would each hold part of the chip and spin until their time limit.  All persistent work of a process on one device is therefore
// ordered by an event chain: the stream about to receive persistent launches first waits for the event behind the previous such
// enqueue (of ANY handle), and records the next one behind its own.  The mutex is held across the enqueue (wait .. record): two host
// threads cannot both wait for the same predecessor.  Kernels of other streams that are not persistent (a decode on another lane)
// only delay a persistent launch -- they end by themselves.
struct PersistOrder {
    static std::mutex& mu() { static std::mutex m; return m; }
    static hipEvent_t& ev(int device) { static std::map<int, hipEvent_t> evs; return evs[device]; }
    std::unique_lock<std::mutex> lock;
    hipStream_t st;
    int device;
    bool active;
    PersistOrder(int device_, hipStream_t st_, bool active_) : st(st_), device(device_), active(active_) {
        if (!active) return;
        lock = std::unique_lock<std::mutex>(mu());
        hipEvent_t& e = ev(device);
        if (!e) { if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; return; } }
        else hipStreamWaitEvent(st, e, 0);
    }
    ~PersistOrder() {
        if (!active) return;
        hipEvent_t e = ev(device);
        if (e) hipEventRecord(e, st);
    }
};

// The host tables of a call (B <= max_batch entries each) through ONE slot of the pinned ring to their device buffers.  Merged steps: per-row Philox keys and / or
// sampler settings; a guided call: its pair table, and ALWAYS the keys -- the implicit ones (seed, sample_offset + b) are built here, the negative row of every pair taking its positive row's
static int send_row_tables(hqt_handle* h, const SampleCtx& c) {
    if (!(c.row_seeds || c.row_set || c.guide || c.keep || c.groups || c.roll)) return HQT_OK;
    const int B = c.B;
    int slot = 0;
    RingSlot ring;
    CHK(rows_ring_take(h, &slot, &ring));
    if (c.row_seeds || c.guide) {
        for (int b = 0; b < B; ++b) {
            ring.keys[b].seed = c.row_seeds ? c.row_seeds[b] : c.seed;
            ring.keys[b].global_row = c.row_offsets ? c.row_offsets[b] : c.sample_offset + b;
        }
        for (int i = 0; i < c.n_guide; ++i) ring.keys[c.guide[i].neg_row] = ring.keys[c.guide[i].pos_row];      // (explicit keys were checked to agree: sample_call)
        CHK(ring_send(ring.keys, (const RowKey*)nullptr, (size_t)B, h->rows, c.st));
    }
    if (c.row_set) CHK(ring_send(ring.samplers, c.row_set, (size_t)B, h->row_set, c.st));
    if (c.guide) CHK(ring_send(ring.pairs, c.guide, (size_t)c.n_guide, h->guide, c.st));
    if (c.keep) CHK(ring_send(ring.keep, c.keep, (size_t)B * c.n_steps, h->keep_mask, c.st));
    if (c.groups) CHK(ring_send(ring.groups, c.groups, (size_t)B, h->group_of_row, c.st));
    if (c.roll) {
        // the positions the rows stand at (moved on between the steps) and the table as received (what finish_rolling copies out by).  Rows that join through a join phase: the live
        // table has them behind it already (position L + 1 behind a kept run of L; past the last position: finished), the join table says L for them, -1 for the rest, the fan-out's groups number them
        int32_t *live = ring.pos, *received = ring.pos + h->cfg.max_batch, *join = ring.pos + 2 * (size_t)h->cfg.max_batch;
        int g = 0;
        for (int b = 0; b < B; ++b) {
            const bool joins = c.n_join && c.roll[b] == 0;
            received[b] = c.roll[b];
            live[b] = joins ? (c.join_len + 1 < c.n_steps ? c.join_len + 1 : -1) : c.roll[b];
            join[b] = joins ? c.join_len : -1;
            ring.groups[b] = joins ? g++ : -1;
        }
        CHK(ring_send(live, (const int32_t*)nullptr, (size_t)B, h->row_pos, c.st));
        CHK(ring_send(received, (const int32_t*)nullptr, (size_t)B, h->row_pos_received(), c.st));
        if (c.n_join) {
            CHK(ring_send(join, (const int32_t*)nullptr, (size_t)B, h->row_pos_join(), c.st));
            CHK(ring_send(ring.groups, (const int32_t*)nullptr, (size_t)B, h->group_of_row, c.st));
        }
    }
    return ring_sent(h, slot, c.st);
}

// A prefill over fewer rows than the pass has, through the staging (hqt_handle::pg_*): shared prompts (the n_prompts distinct prompts of cond [n_prompts, T]) and
// the join phase of a rolling pass (`gathered`: the joiners' rows, read from cond [B, .] and the handle's code buffers through the group table -- their prompts on a text
// handle, their sos / class row otherwise, then the input rows of the `run` leading kept positions they share, the layout of embed_prefill).  A sample's prompt rows depend
// on nothing but its prompt, so the embedding and the body blocks run over the prompts alone, K/V into the staging buffer [n_layers][n_prompts][T][D] -- never cache slot g,
// the destination of row g of the pass, which may carry another prompt --; ONE launch then copies the staged K/V of every row's prompt into its cache slot and gathers its last
// row of x (a negative group: neither); the depth head runs over the B gathered rows (one per sample) under `head_row_pos` and draws position `run` (0 without a kept run).
static int staged_prompt_prefill(hqt_handle* h, const SampleCtx& c, int n_prompts, bool gathered, const int* head_row_pos, int run = 0) {
    const hqt_config& cf = h->cfg;
    const bool text = cf.cond_type == HQT_COND_TEXT;
    const int Tp = text ? cf.ctx_len_txt : 0, T = (text ? Tp : 1) + run, D = cf.embed_dim;      // Tp prompt rows, T rows per prompt in all
    if (!gathered && (!text || run)) return fail(HQT_ERR_INVALID, "staged_prompt_prefill: only the join phase of a rolling pass prefills a kept run or rows without a prompt");
    SampleCtx cg = c;
    cg.B = n_prompts;
    cg.row_pos = nullptr;                            // (the prefill of the prompts knows no positions)
    if (!text || run) {                              // the sos / class row and the rows of the kept run, as embed_prefill lays them out: (text) `run` rows behind the prompt, at step offset 1
        Timed t(h, "embed_prefix", c.st);
        HIPCHK(launch_embed_prefix_rows(embed_args(h, c, c.out), h->group_of_row, n_prompts, T - Tp, T, Tp, text ? 1 : 0, c.st));
    }
    if (text && gathered) HIPCHK(launch_embed_text_rows(c.cond, h->group_of_row, W(h, "tok_emb_txt.weight"), W(h, "pos_emb_txt.weight"), h->x, c.B, n_prompts, Tp, D, c.st, cf.vocab_txt, T));
    else if (text) HIPCHK(launch_embed_text(c.cond, W(h, "tok_emb_txt.weight"), W(h, "pos_emb_txt.weight"), h->x, n_prompts, Tp, D, c.st, cf.vocab_txt, T));
    const KvStage stage{h->pg_k, h->pg_v};
    bool pfull = false;
    CHK(run_body(h, cg, T, 0, false, false, &pfull, &stage));
    CHK(fold_pending(h, cg, n_prompts * T));         // (the staged rows, before the fan-out gathers x)
    {
        Timed t(h, "prompt_fanout", c.st);
        const FanoutArgs fa{h->pg_k, h->pg_v, h->kcache, h->vcache, h->x, h->pg_x, h->group_of_row, cf.n_layers, c.B, n_prompts, T, D,
                            D * (int)c.md.act_sz(), cf.max_batch, h->Tmax};
        HIPCHK(launch_prompt_fanout(fa, c.st));
    }
    SampleCtx ch = c;
    ch.row_pos = head_row_pos;
    return run_depth_head(h, ch, h->pg_x, 1, false);
}

// What a captured graph of G decode steps depends on: a call whose key equals the cached one replays the cached graph
static std::vector<uint64_t> graph_key_of(const hqt_handle* h, const SampleCtx& c, int G) {
    std::vector<uint64_t> key = {(uint64_t)G, (uint64_t)c.B, (uint64_t)(c.cond != nullptr), (uint64_t)c.noise, (uint64_t)c.logits_out, (uint64_t)c.logprob_out,
                                 (uint64_t)c.precision, (uint64_t)c.n_steps, (uint64_t)c.levels, (uint64_t)h->policy + (c.roll ? 16 : 0),      // (+ 16: a rolling pass, never its positions)
                                 (uint64_t)((h->persist_enabled && !h->persist_tripped ? 1 : 0) + (h->single_key ? 0 : 4) + (h->split_kslices ? 0 : 8))};
    for (const int64_t* f : c.feed) key.push_back((uint64_t)f);
    for (const SamplerSet& l : c.lv) {
        uint32_t f[2];
        memcpy(f, &l.top_p, 4); memcpy(f + 1, &l.temperature, 4);
        key.push_back((uint64_t)l.top_k); key.push_back(f[0]); key.push_back(f[1]);
    }
    // a row table: that there is one (two sampler launches per draw where the pass dispatches) and whether a row uses top-p (the LDS of the general kernel) -- never its values, which the kernels read from device memory: a changed table replays the same graph
    key.push_back((uint64_t)((c.row_set ? 1 : 0) + (c.row_top_p ? 2 : 0)));
    // a pair table: that there is one (one more launch per sub-step) and its pair count (that launch's grid), never its rows or scales
    key.push_back((uint64_t)c.n_guide);
    // a keep table: that there is one (the samplers' guard) and the length of its prefill (the positions the graph covers), never its values
    key.push_back(c.keep ? (uint64_t)c.prefix_len + 1 : 0);
    // a draw report: its pointers and top_n (kernel arguments of the launches that take code_logprob's place)
    for (const void* p : {(const void*)c.report.entropy, (const void*)c.report.rank, (const void*)c.report.top_codes, (const void*)c.report.top_logprobs}) key.push_back((uint64_t)p);
    key.push_back((uint64_t)c.report.top_n);
    return key;
}
static int capture_steps(hqt_handle* h, const SampleCtx& c, int G) {      // G decode steps captured on a stream of their own: the handle's graph, in place of the one it held
    if (h->graph_exec) {                             // rare (options or test-only buffers changed): drain before destroying
        HIPCHK(hipStreamSynchronize(c.st));
        hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr;
    }
    SampleCtx cc = c;
    HIPCHK(hipStreamCreateWithFlags(&cc.st, hipStreamNonBlocking));
    h->capture_persist = false;
    HIPCHK(hipStreamBeginCapture(cc.st, hipStreamCaptureModeThreadLocal));
    int rc = HQT_OK;
    for (int gi = 0; gi < G && rc == HQT_OK; ++gi) rc = run_decode_step(h, cc);
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture(cc.st, &graph);
    hipStreamDestroy(cc.st);
    if (rc != HQT_OK) { if (graph) hipGraphDestroy(graph); return rc; }
    HIPCHK(e);
    HIPCHK(hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0));
    hipGraphDestroy(graph);
    h->graph_has_persist = h->capture_persist;
    h->persist_used = false;                         // capturing queued nothing
    return HQT_OK;
}

static int sample_run(hqt_handle* h, const SampleCtx& c) {
    const hqt_config& cf = h->cfg;
    HIPCHK(sampler_configure(cf.vocab_top, c.top_p));
    CHK(persist_bind(h));
    if (c.start == 0) HIPCHK(launch_set_step(h->state, 0, 0, c.st));      // (a continuation goes on from the step state its pass stopped at)
    if ((c.row_seeds || c.row_offsets) && (!c.row_seeds || !c.row_offsets)) return fail(HQT_ERR_INVALID, "row_seeds and row_offsets come together");
    CHK(send_row_tables(h, c));
    // the kept codes go into the handle's code buffers (outside any captured graph) behind the mask: every level's embeddings, the samplers' guard and
    // code_logprob read them there
    for (int i = 0; i < (c.keep && !c.roll ? c.levels : 0); ++i)
        HIPCHK(launch_copy_kept(c.keep_codes[i], c.out[i], h->keep_mask, c.B, c.n_steps, LEVEL_WIDTH[i], cf.vocab_top, c.st));
    if (!c.row_seeds && !c.guide) HIPCHK(launch_set_rows(h->rows, c.B, c.seed, c.sample_offset, c.st));
    int first = c.start;
    // a rolling pass: every continued row reads the codes of its position pos[b] - 1 where the caller holds them, as a segment does (a forced level: force_*)
    for (int i = 0; i < (c.roll ? c.levels : 0); ++i)
        if (c.feed[i] == c.out[i]) HIPCHK(launch_copy_row_positions(c.roll_prev[i], c.out[i], h->row_pos_received(), c.B, c.n_steps, LEVEL_WIDTH[i], -1, 0, c.st));
    // ... and with a keep table every row takes the kept codes of the span it passes in this call, [pos[b], pos[b] + k) and, joining through the join phase, the run in front
    for (int i = 0; i < (c.roll && c.keep ? c.levels : 0); ++i)
        HIPCHK(launch_copy_kept_rows(c.keep_codes[i], c.out[i], h->keep_mask, h->row_pos_received(), c.B, c.n_steps, LEVEL_WIDTH[i], c.roll_k,
                                     c.roll_k + (c.n_join ? c.join_len + 1 : 0), cf.vocab_top, c.st));
    if (c.start > 0) {                           // a continuation (hqt_set_segment): no prefill -- the cache holds the prompt rows and every position below start
    } else if (c.roll) {
        // A rolling pass runs no prefill over its rows; the rows that join a text handle, or join behind a leading kept run L > 0 (check_joins), run the JOIN PHASE, the
        // staged prompt prefill with the joiners as the groups and the depth head under the join table: the joiners draw position L (kept itself: the samplers' guard) under
        // their own key, sampler row and noise slice, every other row is idle (it computes on the finite row it was left with and writes nothing).  The steps below find the
        // joiners at position L + 1, behind (ctx_len_txt | 1) + L cache rows.
        if (c.n_join) CHK(staged_prompt_prefill(h, c, c.n_join, true, h->row_pos_join(), c.join_len));
    } else if (cf.cond_type == HQT_COND_TEXT && c.groups) {
        // shared prompts (P = 0, checked by sample_call): afterwards the cache and the step state are what the unshared prefill leaves
        CHK(staged_prompt_prefill(h, c, c.n_groups, false, nullptr));
        HIPCHK(launch_advance_step(h->state, cf.ctx_len_txt, c.st));
        first = 1;
    } else if (cf.cond_type == HQT_COND_TEXT || c.prefix_len) {
        // The prefill: the text prompt (64-token causal prefill: sampling.py:187-190, layers.py:107-111) and / or a code prefix of P positions as ONE pass
        // over the rows embed_prefill lays out, read from the handle's code buffers.  All body blocks run causally over them -- K/V of all rows go to the cache --, ln_f and
        // the depth head on the last row, which draws position P: the step state says (P, 0) while that pass runs (sampler keys, noise slice, where the codes go) and P + 1 over
        // all the rows afterwards.  The classic path (Tq_body > 1: run_body); the persistent chain first reads the step state in the decode steps below.  Text, P = 0: the plain prompt prefill.
        const int P = c.prefix_len;
        int rows = 0;
        if (P) HIPCHK(launch_set_step(h->state, P, 0, c.st));
        CHK(embed_prefill(h, c, c.out, P, &rows));
        CHK(run_position(h, c, rows, 0, false));
        HIPCHK(launch_advance_step(h->state, rows, c.st));
        first = P + 1;
    }
    const int remaining = c.stop - first;       // (without a segment: stop = n_steps)
    if (remaining <= 0) return HQT_OK;
    if (c.use_graph && !h->timing) {
        // positions per captured graph: the largest divisor of the remaining positions up to HQT_GRAPH_POSITIONS (default 16):
        // one graph launch then covers G positions (fewer host launches and graph-to-graph hand-overs on the device)
        const int gmax = switch_value(SW_GRAPH_POSITIONS);
        int G = 1;
        for (int d = std::min(gmax, remaining); d >= 1; --d) if (remaining % d == 0) { G = d; break; }
        std::vector<uint64_t> key = graph_key_of(h, c, G);
        if (!h->graph_exec || key != h->graph_key) {
            CHK(capture_steps(h, c, G));
            h->graph_key = std::move(key);
        }
        PersistOrder order(h->device, c.st, h->graph_has_persist);
        if (h->graph_has_persist) h->persist_used = true;   // every replay queues the persistent launches the graph holds (hqt_range_check reads their mark)
        for (int s = 0; s < remaining / G; ++s) HIPCHK(hipGraphLaunch(h->graph_exec, c.st));
        return HQT_OK;
    }
    const bool may_persist = c.md.fast && c.B <= 64 && (persist_on(h, c, h->pfull) || persist_on(h, c, h->pbody));
    PersistOrder order(h->device, c.st, may_persist);
    for (int s = 0; s < remaining; ++s) CHK(run_decode_step(h, c));
    return HQT_OK;
}

// ------------------------------------------------------------------------------------------ stage 1
static const float* W1(hqt_handle* h, const std::string& name) { return h->w["stage1." + name].d; }

static GemmArgs conv_args(const void* in, int nimg, int res_out, int cin, int taps, int upsample, void* out, int cout) {
    GemmArgs g{};
    g.A = in; g.conv_taps = taps; g.H = res_out; g.W = res_out; g.Cin = cin; g.upsample = upsample;
    g.M = nimg * res_out * res_out; g.batch = 1;
    g.C = out; g.ldc = cout; g.store = STORE_ROWS;
    return g;
}
static void with_gn(GemmArgs& g, const float* stats, const float* gamma, const float* beta, int swish) {
    g.gn_stats = stats; g.gn_gamma = gamma; g.gn_beta = beta; g.gn_groups = 32; g.gn_swish = swish;
}

// One chunk of images moving through the conv stack (decoder or encoder): the rotating activation buffers and the two
// GroupNorm statistics slots.
struct S1Ctx {
    hqt_handle* h;
    int n;
    Mode md;
    hipStream_t st;
    int adt;
    void *cur, *t1, *t2, *tn;
    float *gn1, *gn2;
    bool cur_planes = false;   // SPLIT: `cur` already holds fp16 hi / lo operand planes (the producing conv's epilogue emitted them: GemmArgs::out_split)
    // per-tile output statistics a 3x3 conv of this chunk left in h->gn_tiles for the GroupNorm of `tensor` (dbl: double partials, SPLIT conv)
    struct { const void* tensor; int tiles; bool dbl; } gn_ready = {nullptr, 0, false};
};

// How the A operand of a stage-1 conv arrives: the tensor as the layer before left it (fp32, or bf16 in FAST), fp16 hi / lo planes
// (an operand pass or the producing conv wrote them), or the fp32 tensor split by the SPLIT GEMM while it stages its tiles
enum S1Operand { S1_TENSOR, S1_PLANES, S1_SPLIT_IN_KERNEL };

// SPLIT: can conv / GEMM `g` (A = an fp32 NHWC tensor) with filters `l` run on the matrix cores?  Shapes the split kernels do
// not take (strided taps, channel counts that are not multiples of 64, ...) fall back to the fp32 vector-ALU kernel.
static bool split_shape_ok(const hqt_handle* h, const GemmArgs& g, const Lin& l) {
    if (!l.w16h) return false;
    GemmArgs t = g;
    lin_args(h, t, l, true);
    return t.conv_taps == 9 ? split_conv3_ok(t) : split_gemm_ok(t);
}
// SPLIT operand pass: fp16 hi / lo planes of (GroupNorm + swish of) the fp32 tensor g->A into `tn`; the conv then reads `tn`.
static int s1_split_pack(S1Ctx& c, GemmArgs* g, const float* stats, const float* gamma, const float* beta, int swish) {
    hqt_handle* h = c.h;
    const int hw_in = g->conv_taps ? ((g->H << g->conv_stride2) >> g->upsample) * ((g->W << g->conv_stride2) >> g->upsample) : 0;
    const int C = g->conv_taps ? g->Cin : g->lda;
    const int rows = g->conv_taps ? c.n : 1, per = g->conv_taps ? hw_in : g->M;
    Timed t(h, "split_pack", c.st);
    HIPCHK(launch_split_pack(reinterpret_cast<const float*>(g->A), reinterpret_cast<half_t*>(c.tn), stats, gamma, beta, rows, per, C, 32, swish, h->range_flag, c.st));
    g->A = c.tn;
    if (!g->conv_taps) g->lda = 2 * C;
    return HQT_OK;
}

// SPLIT: GroupNorm statistics of the fp32 tensor `src`, from the per-tile sums its producing conv left or by a pass over it
static int s1_split_stats(S1Ctx& c, const void* src, int C, int hw, float* stats) {
    Timed t(c.h, "gn_stats", c.st);
    if (c.gn_ready.tensor == src && c.gn_ready.dbl) {
        count_variant(c.h, "variant:gn_stats_tiles:gn");
        HIPCHK(launch_gn_finalize_tiles_d(reinterpret_cast<const double*>(c.h->gn_tiles), stats, c.n, c.gn_ready.tiles, hw, C, 32, 1e-6f, c.st));
    } else {
        count_variant(c.h, "variant:gn_stats_pass:gn");
        HIPCHK(launch_gn_stats_fast(src, stats, c.h->gn_partial, c.n, hw, C, 32, 1e-6f, c.st, DT_F32));
    }
    return HQT_OK;
}

// GroupNorm(+swish) in front of a conv.  EXACT: statistics pass, then the normalisation is applied inside
// the conv's operand loader.  FAST: statistics pass + one bandwidth-bound apply pass into `tn`, so the MFMA
// conv reads a plain bf16 tensor.  SPLIT: statistics (from the producing conv's epilogue when it left them), then the
// operand pass writes the normalised tensor as fp16 hi / lo planes into `tn`; shapes the split kernels do not take run
// the EXACT way.  Sets the tensor the conv must read / fills the loader's GN fields.
static int s1_norm(S1Ctx& c, const void* src, int C, int hw, float* stats, const float* gamma, const float* beta, int swish, GemmArgs* g,
                   const Lin& l, S1Operand* a) {
    hqt_handle* h = c.h;
    hipStream_t st = c.st;
    *a = S1_TENSOR;
    if (c.md.fast) {
        {
            Timed t(h, "gn_stats", st);
            if (c.gn_ready.tensor == src && !c.gn_ready.dbl) {     // the producing conv already reduced its tiles: only the fixed-order finalize is left
                count_variant(h, "variant:gn_stats_tiles:gn");
                HIPCHK(launch_gn_finalize_tiles(h->gn_tiles, stats, c.n, c.gn_ready.tiles, hw, C, 32, 1e-6f, st));
            } else {
                count_variant(h, "variant:gn_stats_pass:gn");
                HIPCHK(launch_gn_stats_fast(src, stats, h->gn_partial, c.n, hw, C, 32, 1e-6f, st));
            }
        }
        { Timed t(h, "gn_apply", st); HIPCHK(launch_gn_apply(src, c.tn, stats, gamma, beta, c.n, hw, C, 32, swish, st)); }
        g->A = c.tn;
    } else if (c.md.split && split_shape_ok(h, *g, l)) {
        CHK(s1_split_stats(c, src, C, hw, stats));
        CHK(s1_split_pack(c, g, stats, gamma, beta, swish));
        *a = S1_PLANES;
    } else {
        { Timed t(h, "gn_stats", st); HIPCHK(launch_gn_stats(src, c.adt, stats, c.n, hw, C, 32, 1e-6f, st)); }
        count_variant(h, "variant:gn_stats_two_pass:gn");
        with_gn(*g, stats, gamma, beta, swish);
    }
    return HQT_OK;
}
// a conv without GroupNorm in front (conv_in, upsample conv, nin_shortcut, proj_out, the 1x1 convs around the quantiser): SPLIT
// needs the operand planes, the other modes read the tensor as it is
static int s1_plain(S1Ctx& c, GemmArgs* g, const Lin& l, S1Operand* a) {
    *a = S1_TENSOR;
    if (!c.md.split) return HQT_OK;
    if (g->conv_taps == 1) {                 // 1x1: the GEMM kernel splits the fp32 tensor while it stages the tile -- no operand pass
        GemmArgs t = *g;
        t.a_f32 = 1;
        if (split_shape_ok(c.h, t, l)) {
            g->a_f32 = 1; g->range_flag = c.h->range_flag; *a = S1_SPLIT_IN_KERNEL;
            return HQT_OK;
        }
    }
    if (!split_shape_ok(c.h, *g, l)) return HQT_OK;
    *a = S1_PLANES;
    return s1_split_pack(c, g, nullptr, nullptr, nullptr, 0);
}

// Stage 1, one convolution (or the 1x1 conv as a GEMM) of filter bank `l` over the chunk; `a`: how its A operand arrives (s1_norm / s1_plain
// checked the shape before they chose anything but S1_TENSOR).  SPLIT kernels for planes, FAST: the MFMA / halo kernels, otherwise the fp32
// vector-ALU kernel.  A 3x3 conv whose output is normalised next also leaves per-tile GroupNorm statistics (c.gn_ready).
static int s1_conv(S1Ctx& c, GemmArgs g, S1Operand a, const Lin& l, int c_dt, const char* tag) {
    hqt_handle* h = c.h;
    lin_args(h, g, l, a != S1_TENSOR);
    Timed t(h, SlotName(tag, g.M).s, c.st);
    if (c.gn_ready.tensor == g.C) c.gn_ready.tensor = nullptr;          // the tensor is being overwritten
    if (a != S1_TENSOR) {
        if (g.conv_taps != 9) { count_variant(h, "variant:split_gemm:%s", tag); HIPCHK(launch_split_gemm(g, c.st)); return HQT_OK; }
        count_variant(h, "variant:split_conv3:%s", tag);
        if (g.store == STORE_ROWS && h->gn_tiles && conv_halo_stats_ok(g.N, 32)) {   // every such output is normalised next
            g.gn_part_out_d = reinterpret_cast<double*>(h->gn_tiles); g.gn_out_groups = 32;
            c.gn_ready = {g.C, split_conv3_tiles_per_image(g), true};
        }
        HIPCHK(launch_split_conv3(g, c.st));
        return HQT_OK;
    }
    if (c.md.fast) {
        g.Bw = l.w16;
        if (!mfma_gemm_ok(g, c.adt, DT_BF16, c_dt)) {
            count_variant(h, "variant:gemm_generic_bf16:%s", tag);
            HIPCHK(launch_gemm_generic(g, c.adt, DT_BF16, c_dt, c.st));
            return HQT_OK;
        }
        if (h->timing) count_variant(h, conv_halo_ok(g, c_dt) ? "variant:halo_conv:%s" : "variant:mfma_gemm:%s", tag);
        // a 3x3 halo conv also leaves per-tile GroupNorm statistics of its output
        if (g.conv_taps == 9 && g.store == STORE_ROWS && h->gn_tiles && conv_halo_ok(g, c_dt) && conv_halo_stats_ok(g.N, 32) &&
            !switch_value(SW_NO_FUSED_GN)) {
            g.gn_part_out = h->gn_tiles; g.gn_out_groups = 32;
            c.gn_ready = {g.C, conv_halo_tiles_per_image(g), false};
        }
        HIPCHK(launch_mfma_gemm(g, c.adt, DT_BF16, c_dt, c.st));
        return HQT_OK;
    }
    g.Bw = l.w32;                                // (k_quarters stays 0: the summation order of the AR loop's nn.Linear is not a convolution's)
    count_variant(h, "variant:gemm_generic_f32:%s", tag);
    HIPCHK(launch_gemm_generic(g, DT_F32, DT_F32, DT_F32, c.st));
    return HQT_OK;
}

// SPLIT: a product of two fp32 ACTIVATION tensors (the attention block's q k^T and softmax v) on the matrix cores -- both operands are
// split while their tiles are staged (split_gemm_kernel<true, true>); shapes it does not take stay on the fp32 vector-ALU kernel
static bool s1_split_product(hqt_handle* h, const Mode& md, GemmArgs& sg) {
    if (!md.split) return false;
    GemmArgs t = sg;
    t.a_f32 = 1; t.b_f32 = 1; t.range_flag = h->range_flag;
    if (!split_gemm_ok(t)) return false;
    sg = t;
    return true;
}

// kinds 0 conv3, 1 ResnetBlock, 2 AttnBlock, 3 upsample conv, 5 Downsample conv (shared by Decoder.forward and Encoder.forward)
static int s1_layer(S1Ctx& c, const DecLayer& l, const DecLayer* next = nullptr) {
    hqt_handle* h = c.h;
    hipStream_t st = c.st;
    const int adt = c.adt, n = c.n;
    void *&cur = c.cur, *&t1 = c.t1, *&t2 = c.t2;
    const int res = l.res, hw = res * res;
    if (l.kind == 0 || l.kind == 3) {
        const int ro = l.kind == 3 ? 2 * res : res;
        GemmArgs g = conv_args(cur, n, ro, l.cin, 9, l.kind == 3, t1, l.cout);
        S1Operand a = S1_PLANES;
        if (c.cur_planes) c.cur_planes = false;                      // the producing conv wrote the planes
        else CHK(s1_plain(c, &g, l.conv1, &a));
        CHK(s1_conv(c, g, a, l.conv1, adt, "conv3x3"));
        std::swap(cur, t1);
    } else if (l.kind == 5) {               // Downsample (stage1/modules/layers.py:56-76): pad right / bottom by one, 3x3 stride 2
        GemmArgs g = conv_args(cur, n, res / 2, l.cin, 9, 0, t1, l.cout);
        g.conv_stride2 = 1; g.conv_nopad = 1;
        CHK(s1_conv(c, g, S1_TENSOR, l.conv1, adt, "conv_down"));
        std::swap(cur, t1);
    } else if (l.kind == 1) {               // ResnetBlock (stage1/modules/layers.py:115-133)
        GemmArgs g = conv_args(cur, n, res, l.cin, 9, 0, t1, l.cout);
        S1Operand a;
        CHK(s1_norm(c, cur, l.cin, hw, c.gn1, l.n1_g, l.n1_b, 1, &g, l.conv1, &a));
        CHK(s1_conv(c, g, a, l.conv1, adt, "conv3x3"));
        const void* shortcut = cur;
        void* outbuf = t2;
        if (l.cin != l.cout) {
            GemmArgs sc = conv_args(cur, n, res, l.cin, 1, 0, t2, l.cout);
            CHK(s1_plain(c, &sc, l.nin, &a));
            CHK(s1_conv(c, sc, a, l.nin, adt, "conv1x1"));
            shortcut = t2;
            outbuf = cur;                   // x is dead once the shortcut is computed
        }
        g = conv_args(t1, n, res, l.cout, 9, 0, outbuf, l.cout);
        g.resid = shortcut;
        CHK(s1_norm(c, t1, l.cout, hw, c.gn2, l.n2_g, l.n2_b, 1, &g, l.conv2, &a));
        // SPLIT: when the block's only consumer is an upsampling conv (no GroupNorm in between) whose operand would be split by a separate pass, this conv's epilogue
        // writes the operand planes instead of the fp32 tensor (same bytes, one pass over the tensor less)
        bool planes = false;
        if (a == S1_PLANES && next && next->kind == 3 && next->cin == l.cout) {
            GemmArgs up = conv_args(outbuf, n, 2 * res, next->cin, 9, 1, t1, next->cout);
            GemmArgs me = g;
            lin_args(h, me, l.conv2, true);
            planes = split_shape_ok(h, up, next->conv1) && split_conv3_emits_planes(me);
        }
        if (planes) { g.out_split = 1; g.range_flag = h->range_flag; }
        CHK(s1_conv(c, g, a, l.conv2, adt, "conv3x3"));
        if (outbuf == t2) std::swap(cur, t2);
        c.cur_planes = planes;
        if (planes) count_variant(h, "variant:conv3x3_planes_out:conv3x3");
    } else if (l.kind == 2) {               // AttnBlock (stage1/modules/layers.py:163-186)
        const int C = l.cin;
        GemmArgs g = conv_args(cur, n, res, C, 1, 0, h->aq, C);
        S1Operand a;
        CHK(s1_norm(c, cur, C, hw, c.gn1, l.n1_g, l.n1_b, 0, &g, l.q, &a));
        const GemmArgs normed = g;           // same normalised input for q, k, v
        CHK(s1_conv(c, g, a, l.q, adt, "conv1x1"));
        g = normed; g.C = h->ak;
        CHK(s1_conv(c, g, a, l.k, adt, "conv1x1"));
        g = normed; g.C = h->av;
        g.store = STORE_NCHW; g.rows_per_image = hw;                 // V^T per image: [C][hw]
        CHK(s1_conv(c, g, a, l.v, adt, "conv1x1"));
        // one product of two activation tensors per image: [M, K] x [N, K]^T
        auto product = [&](const void* A, const void* B, void* out, int M, int N, int K, float alpha) -> int {
            Timed t(h, "attn_gemm", st);
            GemmArgs sg{};
            sg.A = A; sg.lda = K; sg.a_batch_stride = (long long)M * K;
            sg.Bw = B; sg.ldb = K; sg.b_batch_stride = (long long)N * K;
            sg.C = out; sg.ldc = N; sg.c_batch_stride = (long long)M * N;
            sg.M = M; sg.N = N; sg.K = K; sg.batch = n; sg.alpha = alpha; sg.store = STORE_ROWS;
            sg.zero_page = h->zero_page;          // lets the LDS-DMA kernel take the batched product
            if (c.md.fast && mfma_gemm_ok(sg, adt, adt, adt)) {
                count_variant(h, "variant:mfma_gemm:attn_gemm");
                HIPCHK(launch_mfma_gemm(sg, adt, adt, adt, st));
            } else if (s1_split_product(h, c.md, sg)) {
                count_variant(h, "variant:split_gemm:attn_gemm");
                HIPCHK(launch_split_gemm(sg, st));
            } else {
                count_variant(h, c.md.fast ? "variant:gemm_generic_bf16:attn_gemm" : "variant:gemm_generic_f32:attn_gemm");
                HIPCHK(launch_gemm_generic(sg, adt, adt, adt, st));
            }
            return HQT_OK;
        };
        CHK(product(h->aq, h->ak, h->as, hw, hw, C, 1.0f / sqrtf((float)C)));      // S[i, j] = q_i . k_j * C^-0.5
        { Timed t(h, "softmax", st); HIPCHK(launch_softmax_rows(h->as, adt, n * hw, hw, st)); }
        CHK(product(h->as, h->av, h->ao, hw, C, hw, 1.0f));                         // o[i, c] = sum_j w[i, j] v[c, j]
        g = conv_args(h->ao, n, res, C, 1, 0, t1, C);
        g.resid = cur;
        CHK(s1_plain(c, &g, l.proj, &a));
        CHK(s1_conv(c, g, a, l.proj, adt, "conv1x1"));
        std::swap(cur, t1);
    } else {
        return fail(HQT_ERR_INVALID, "s1_layer: kind %d", l.kind);
    }
    return HQT_OK;
}

static int decode_chunk(hqt_handle* h, int n, const int64_t* code_t, const int64_t* code_m, const int64_t* code_b, int seq_layout,
                        float* out, int clamp01, const Mode& md, hipStream_t st) {
    const hqt_config& cf = h->cfg;
    const int adt = md.act_dt();
    const int r = h->dec.front().res, E = cf.s1_embed_dim;
    const bool l3 = cf.code_levels == 3;
    {
        Timed t(h, "quant_gather", st);
        if (l3) {
            QuantArgs3 q{code_t, code_m, code_b, seq_layout, W1(h, "quantizers.0.embedding"), W1(h, "quantizers.1.embedding"),
                         W1(h, "quantizers.2.embedding"), h->quant, n, r, E, adt, cf.s1_n_embed};
            HIPCHK(launch_quant_gather3(q, st));
        } else if (cf.s1_resample) {     // E-wide top level: the codebook itself (nearest x2) or the folded upsample_t table; a missing top level of conv2 is its bias
            const bool conv2 = cf.s1_resample == HQT_RESAMPLE_CONV2;
            QuantRowsArgs q{code_t, code_b, seq_layout, conv2 ? h->up_table : W1(h, "quantize_t.embedding"), conv2 ? 4 : 1,
                            conv2 ? W1(h, "upsample_t.bias") : nullptr, W1(h, "quantize_b.embedding"), h->quant, n, r, E, adt, cf.s1_n_embed};
            HIPCHK(launch_quant_gather_rows(q, st));
        } else {
            QuantArgs q{code_t, code_b, seq_layout, W1(h, "quantize_t.embedding"), W1(h, "quantize_b.embedding"), h->quant, n, r, E, adt, cf.s1_n_embed};
            HIPCHK(launch_quant_gather(q, st));
        }
    }
    S1Ctx c{h, n, md, st, adt, h->act[0], h->act[1], h->act[2], h->act[3], h->gn, h->gn + (size_t)h->dec_chunk * 64};
    {
        GemmArgs g = conv_args(h->quant, n, r, l3 ? E : 2 * E, 1, 0, c.cur, cf.s1_z_channels);
        S1Operand a;
        CHK(s1_plain(c, &g, h->post_quant, &a));
        CHK(s1_conv(c, g, a, h->post_quant, adt, "conv1x1"));
    }
    for (size_t li = 0; li < h->dec.size(); ++li) {
        const DecLayer& l = h->dec[li];
        if (l.kind != 4) { CHK(s1_layer(c, l, li + 1 < h->dec.size() ? &h->dec[li + 1] : nullptr)); continue; }
        // norm_out -> swish -> conv_out, NCHW fp32 (+clamp)
        const int hw = l.res * l.res;
        GemmArgs g = conv_args(c.cur, n, l.res, l.cin, 9, 0, out, l.cout);
        g.store = STORE_NCHW; g.rows_per_image = hw; g.clamp01 = clamp01;
        if (md.split && l.conv1.w32) {       // SPLIT: the fp32 tensor is read once -- GroupNorm + swish + the three output channels in one fp32 kernel
            GemmArgs d = g;
            d.N = l.conv1.N; d.K = l.conv1.K; d.Bw = l.conv1.w32; d.bias = l.conv1.b32; d.alpha = 1.0f;
            with_gn(d, c.gn1, l.n1_g, l.n1_b, 1);
            if (conv_out_direct_ok(d)) {
                CHK(s1_split_stats(c, c.cur, l.cin, hw, c.gn1));
                Timed t(h, "conv_out", st);
                HIPCHK(launch_conv_out_direct(d, st));
                count_variant(h, "variant:conv_out_direct:conv_out");
                continue;
            }
        }
        S1Operand a;
        CHK(s1_norm(c, c.cur, l.cin, hw, c.gn1, l.n1_g, l.n1_b, 1, &g, l.conv1, &a));
        CHK(s1_conv(c, g, a, l.conv1, DT_F32, "conv_out"));
    }
    return HQT_OK;
}

static int decode_impl(hqt_handle* h, int B, const int64_t* code_t, const int64_t* code_m, const int64_t* code_b, int seq_layout, float* out,
                       int clamp01, int precision, void* stream, int levels) {
    if (!h || !out) return fail(HQT_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(HQT_ERR_STATE, "hqt_finalize_weights has not run");
    if (!h->cfg.has_stage1) return fail(HQT_ERR_STATE, "handle was created without stage 1");
    if ((h->cfg.code_levels == 3) != (levels == 3)) return fail(HQT_ERR_STATE, "stage 1 has %d code levels: use the matching decode entry point", h->cfg.code_levels == 3 ? 3 : 2);
    if (!code_t && !code_b && !code_m) return fail(HQT_ERR_INVALID, "every code grid is NULL");
    if (B < 1) return fail(HQT_ERR_INVALID, "B must be >= 1");
    ON_DEVICE(h);
    Mode md;
    CHK(mode_of(precision, true, &md));
    const int r = h->dec.front().res;
    const int rt = levels == 3 ? r / 4 : r / 2, rm = r / 2;
    const size_t out_per = (size_t)h->cfg.s1_out_ch * h->dec.back().res * h->dec.back().res;
    for (int b0 = 0; b0 < B; b0 += h->dec_chunk) {
        const int n = std::min(h->dec_chunk, B - b0);
        const int64_t* ct = code_t ? code_t + (size_t)b0 * rt * rt : nullptr;
        const int64_t* cm = code_m ? code_m + (size_t)b0 * rm * rm : nullptr;       // every layout holds rm*rm / r*r codes per image
        const int64_t* cb = code_b ? code_b + (size_t)b0 * r * r : nullptr;
        CHK(decode_chunk(h, n, ct, cm, cb, seq_layout, out + (size_t)b0 * out_per, clamp01, md, (hipStream_t)stream));
    }
    return HQT_OK;
}
extern "C" int hqt_decode(hqt_handle* h, int B, const int64_t* code_t, const int64_t* code_b, float* out, int clamp01,
                          int precision, void* stream) {
    return decode_impl(h, B, code_t, nullptr, code_b, 0, out, clamp01, precision, stream, 2);
}
extern "C" int hqt_decode_seq(hqt_handle* h, int B, const int64_t* codes_top, const int64_t* codes_bot, float* out,
                              int clamp01, int precision, void* stream) {
    return decode_impl(h, B, codes_top, nullptr, codes_bot, 1, out, clamp01, precision, stream, 2);
}
extern "C" int hqt_decode_l3(hqt_handle* h, int B, const int64_t* code_t, const int64_t* code_m, const int64_t* code_b, float* out,
                             int clamp01, int precision, void* stream) {
    return decode_impl(h, B, code_t, code_m, code_b, 0, out, clamp01, precision, stream, 3);
}
extern "C" int hqt_decode_seq_l3(hqt_handle* h, int B, const int64_t* codes0, const int64_t* codes1, const int64_t* codes2, float* out,
                                 int clamp01, int precision, void* stream) {
    return decode_impl(h, B, codes0, codes1, codes2, 1, out, clamp01, precision, stream, 3);
}

// ------------------------------------------------------------------------------------------ stage 1, encode side
// Encoder.forward + quant_conv_b for one chunk of images: h rows (fp32 NHWC [n, r, r, E]) into h_rows
static int encode_chunk(hqt_handle* h, int n, const float* pixels, float* h_rows, const Mode& md, hipStream_t st) {
    const hqt_config& cf = h->cfg;
    const int adt = md.act_dt();
    S1Ctx c{h, n, md, st, adt, h->act[0], h->act[1], h->act[2], h->act[3], h->gn, h->gn + (size_t)h->dec_chunk * 64};
    for (auto& l : h->enc) {
        if (l.kind == 6) {                  // conv_in (layers.py:212-216): 3x3 stride 1, or 4x4 stride 2 with use_init_downsample
            const int cp = conv_in_cpad(cf), down = cf.s1_use_init_downsample ? 1 : 0;
            { Timed t(h, "image_layout", st); HIPCHK(launch_image_to_nhwc(pixels, c.t2, adt, n, l.res, cp, st)); }
            GemmArgs g = conv_args(c.t2, n, l.res >> down, cp, down ? 16 : 9, 0, c.t1, l.cout);
            g.conv_stride2 = down;
            CHK(s1_conv(c, g, S1_TENSOR, l.conv1, adt, "conv_in"));
            std::swap(c.cur, c.t1);
        } else if (l.kind == 7) {           // norm_out -> swish -> conv_out (layers.py:289-292), then quant_conv_b (generator.py:299) in fp32 rows
            const int hw = l.res * l.res;
            GemmArgs g = conv_args(c.cur, n, l.res, l.cin, 9, 0, c.t1, l.cout);
            S1Operand a;
            CHK(s1_norm(c, c.cur, l.cin, hw, c.gn1, l.n1_g, l.n1_b, 1, &g, l.conv1, &a));
            CHK(s1_conv(c, g, a, l.conv1, adt, "conv3x3"));
            GemmArgs q = conv_args(c.t1, n, l.res, l.cout, 1, 0, h_rows, cf.s1_embed_dim);
            CHK(s1_plain(c, &q, h->quant_conv, &a));
            CHK(s1_conv(c, q, a, h->quant_conv, DT_F32, "conv1x1"));
        } else {
            CHK(s1_layer(c, l));
        }
    }
    return HQT_OK;
}

// Top level of the 'nearest' / 'conv2' variants (generator.py:300-302): h_t = down_t(h_b), nearest code of the E-wide top codebook,
// vq_recon = upsample_t(z + (e - z)) in the bottom layout.  Every product here is fp32 in every precision, like the distance GEMM:
// they decide the codes and are under 0.1 % of an encode's FLOPs.
static int encode_top_resampled(hqt_handle* h, int B, const hqt_encode_out* out, hipStream_t st) {
    const hqt_config& cf = h->cfg;
    const int r = h->dec.front().res, E = cf.s1_embed_dim, rq = r / 2, M = B * rq * rq;
    const bool conv2 = cf.s1_resample == HQT_RESAMPLE_CONV2;
    auto linear = [&](const float* A, const Lin& l, float* C, const char* slot) -> int {        // C[M, N] = A[M, K] W^T + b
        Timed t(h, slot, st);
        GemmArgs g{};
        g.A = A; g.lda = l.K; g.M = M; g.N = l.N; g.K = l.K; g.batch = 1; g.Bw = l.w32; g.ldb = l.K; g.bias = l.b32; g.alpha = 1.0f;
        g.C = C; g.ldc = l.N; g.store = STORE_ROWS; g.zero_page = h->zero_page;
        HIPCHK(launch_gemm_generic(g, DT_F32, DT_F32, DT_F32, st));
        return HQT_OK;
    };
    if (conv2) {      // Conv2d(k 2, stride 2) = a Linear over the pixel-unshuffled rows: the k = 1 gather of vq_rows gives exactly that column order
        VqArgs u{};
        u.h = h->vq_h; u.recon = nullptr; u.B = B; u.r = r; u.E = E; u.k = 1; u.z = h->vq_z; u.z_dtype = DT_F32; u.zz = h->vq_zz;
        { Timed t(h, "vq_rows", st); HIPCHK(launch_vq_rows(u, st)); }
        CHK(linear((const float*)h->vq_z, h->down_lin, h->vq_t, "vq_down_t"));
    } else {
        Timed t(h, "vq_rows", st);
        HIPCHK(launch_vq_avgpool_rows(h->vq_h, h->vq_t, B, r, E, st));
    }
    HIPCHK(launch_row_sumsq(h->vq_t, DT_F32, h->vq_zz, M, E, st));
    if (out->resid[0]) HIPCHK(launch_nhwc_to_nchw_f32(h->vq_t, out->resid[0], B, rq * rq, E, st));
    HIPCHK(hipMemsetAsync(h->vq_best, 0xff, (size_t)M * 8, st));
    const float* emb = W1(h, "quantize_t.embedding");
    {
        Timed t(h, "vq_distance", st);
        GemmArgs g{};
        g.A = h->vq_t; g.lda = E; g.M = M; g.N = cf.s1_n_embed; g.K = E; g.batch = 1; g.ldb = E; g.alpha = 1.0f;
        g.store = STORE_ARGMIN; g.am_rownorm = h->vq_zz; g.am_best = h->vq_best; g.zero_page = h->zero_page;
        g.Bw = emb; g.am_colnorm = h->cb_norm[0];
        HIPCHK(launch_gemm_generic(g, DT_F32, DT_F32, DT_F32, st));
    }
    VqTopArgs a{h->vq_t, h->vq_best, emb, B, r, E, out->codes[0], out->quant[0], conv2 ? h->vq_q : nullptr, conv2 ? nullptr : h->vq_recon, h->vq_err};
    { Timed t(h, "vq_finish", st); HIPCHK(launch_vq_finish_top(a, st)); }
    if (conv2) {      // the straight-through rows are not codebook rows: a real [M, E] x [E, 4E] product + bias, then the 2x2 scatter (every recon element is written)
        CHK(linear(h->vq_q, h->up_lin, (float*)h->vq_z, "vq_upsample_t"));
        Timed t(h, "vq_finish", st);
        HIPCHK(launch_vq_scatter_up((const float*)h->vq_z, h->vq_recon, B, r, E, st));
    }
    if (out->diff) HIPCHK(launch_vq_diff(h->vq_err, M, 0.25f / ((float)M * (float)E), out->diff, st));
    return HQT_OK;
}

extern "C" int hqt_has_encoder(const hqt_handle* h) { return h ? (h->has_encoder ? 1 : 0) : -1; }

extern "C" int hqt_encode(hqt_handle* h, int B, const float* pixels, int precision, const hqt_encode_out* out, void* stream) {
    if (!h || !pixels || !out) return fail(HQT_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(HQT_ERR_STATE, "hqt_finalize_weights has not run");
    if (!h->cfg.has_stage1) return fail(HQT_ERR_STATE, "handle was created without stage 1");
    if (!h->has_encoder) return fail(HQT_ERR_STATE, "the encoder tensors (stage1.encoder.*, stage1.quant_conv_b.*%s) were not set before hqt_finalize_weights",
                                     h->cfg.s1_resample == HQT_RESAMPLE_CONV2 ? ", stage1.down_t.*" : "");
    if (B < 1 || B > h->cfg.max_batch) return fail(HQT_ERR_INVALID, "B must be in [1, max_batch = %d]", h->cfg.max_batch);
    const hqt_config& cf = h->cfg;
    const int L = cf.code_levels == 3 ? 3 : 2;
    for (int l = 0; l < L; ++l) if (!out->codes[l]) return fail(HQT_ERR_INVALID, "codes[%d] is NULL", l);
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    Mode md;
    CHK(mode_of(precision, true, &md));
    const int r = h->dec.front().res, E = cf.s1_embed_dim, R = cf.s1_resolution;
    for (int b0 = 0; b0 < B; b0 += h->dec_chunk) {
        const int n = std::min(h->dec_chunk, B - b0);
        CHK(encode_chunk(h, n, pixels + (size_t)b0 * 3 * R * R, h->vq_h + (size_t)b0 * r * r * E, md, st));
    }
    // residual quantisation, coarse -> fine, over the whole batch (generator.py:300-309 / 541-560)
    const size_t elems = (size_t)B * r * r * E;
    for (int l = 0; l < L; ++l) {
        if (l == 0 && cf.s1_resample) { CHK(encode_top_resampled(h, B, out, st)); continue; }
        const int k = L - 1 - l, rq = r >> k, dim = E << (2 * k), M = B * rq * rq;
        const std::string name = L == 3 ? "quantizers." + std::to_string(l) + ".embedding" : (l == 0 ? "quantize_t.embedding" : "quantize_b.embedding");
        VqArgs a{};
        a.h = h->vq_h; a.recon = l == 0 ? nullptr : h->vq_recon;
        a.B = B; a.r = r; a.E = E; a.k = k;
        a.z = h->vq_z; a.z_dtype = DT_F32; a.zz = h->vq_zz; a.resid_nchw = out->resid[l];
        a.best = h->vq_best; a.emb = W1(h, name); a.codes = out->codes[l]; a.quant_nchw = out->quant[l];
        a.err_rows = h->vq_err + (size_t)l * cf.max_batch * r * r;
        { Timed t(h, "vq_rows", st); HIPCHK(launch_vq_rows(a, st)); }
        HIPCHK(hipMemsetAsync(h->vq_best, 0xff, (size_t)M * 8, st));
        {
            Timed t(h, "vq_distance", st);
            GemmArgs g{};
            g.A = h->vq_z; g.lda = dim; g.M = M; g.N = cf.s1_n_embed; g.K = dim; g.batch = 1; g.ldb = dim; g.alpha = 1.0f;
            g.store = STORE_ARGMIN; g.am_rownorm = h->vq_zz; g.am_best = h->vq_best; g.zero_page = h->zero_page;
            // fp32 in both precisions: h leaves quant_conv_b in fp32 either way, the fp32 vector-ALU GEMM runs these two shapes at
            // ~70 TFLOP/s (1.8 ms of a 8 ms FAST encode at batch 64), and the codes then are the exact nearest ones of the
            // device's own feature map instead of a bf16 approximation of them
            g.Bw = a.emb; g.am_colnorm = h->cb_norm[l];
            HIPCHK(launch_gemm_generic(g, DT_F32, DT_F32, DT_F32, st));
        }
        if (l == 0) {                       // the running reconstruction starts at zero; level 0 reads h alone (generator.py:300-301)
            HIPCHK(hipMemsetAsync(h->vq_recon, 0, elems * 4, st));
            a.recon = h->vq_recon;
            // with recon == 0 the finish pass computes z = h - 0 and recon = q + 0: the same values as the reference's h_t / PS(quant_t)
        }
        { Timed t(h, "vq_finish", st); HIPCHK(launch_vq_finish(a, st)); }
        if (out->diff) HIPCHK(launch_vq_diff(a.err_rows, M, 0.25f / ((float)M * (float)dim), out->diff + l, st));
    }
    if (out->recon) HIPCHK(launch_nhwc_to_nchw_f32(h->vq_recon, out->recon, B, r * r, E, st));
    return HQT_OK;
}

extern "C" int hqt_set_policy(hqt_handle* h, int policy) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    if (policy != HQT_POLICY_LATENCY && policy != HQT_POLICY_THROUGHPUT) return fail(HQT_ERR_INVALID, "unknown policy %d", policy);
    h->policy = policy;
    return HQT_OK;
}

extern "C" int hqt_set_switch(hqt_handle* h, int which, int on) {
    if (!h) return fail(HQT_ERR_INVALID, "null handle");
    if (which == HQT_SWITCH_PERSIST) { h->persist_enabled = on != 0; if (on) h->persist_tripped = false; }
    else if (which == HQT_SWITCH_SINGLE_KEY) h->single_key = on != 0;
    else if (which == HQT_SWITCH_SPLIT_KSLICES) h->split_kslices = on != 0;
    else if (which == HQT_SWITCH_PERSIST_FAULT) {        // test hook: a device word next to the give-up mark (persist.h: err[1]); NOT part of the graph key -- a cached graph replays it
        if (!h->persist_err) return fail(HQT_ERR_STATE, "no persistent chain on this handle (a lane, or a handle without stage 2)");
        ON_DEVICE(h);
        const unsigned v = (unsigned)on;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h->persist_err + 1, &v, sizeof v, hipMemcpyHostToDevice));
    }
    else return fail(HQT_ERR_INVALID, "unknown switch %d", which);
    return HQT_OK;
}

// ------------------------------------------------------------------------------------------ range check of SPLIT calls
extern "C" int hqt_range_check(hqt_handle* h, void* stream) {
    if (!h) return fail(HQT_ERR_INVALID, "null");
    ON_DEVICE(h);
    int flag = 0;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (h->persist_used && h->persist_err) {     // a persistent AR launch that gave up on a barrier (1 s: the GPU was shared with something that kept its workgroups out)
        unsigned pe = 0;
        HIPCHK(hipMemcpy(&pe, h->persist_err, sizeof pe, hipMemcpyDeviceToHost));
        h->persist_used = false;
        if (pe) {
            HIPCHK(hipMemset(h->persist_err, 0, sizeof pe));
            h->persist_tripped = true;           // part of the graph key: the next call captures the launch chain
            return fail(HQT_ERR_STATE, "a persistent AR launch on this handle gave up at the grid barrier in front of phase %u (its workgroups were not all resident within 1 s: the GPU is shared with a process that keeps compute units busy): "
                                       "the codes of that call are invalid; repeat it -- this handle now takes the launch chain (hqt_set_switch(h, HQT_SWITCH_PERSIST, 1) re-arms the persistent launch)", pe - 1);
        }
    }
    HIPCHK(hipMemcpy(&flag, h->range_flag, sizeof flag, hipMemcpyDeviceToHost));
    if (!flag) return HQT_OK;
    HIPCHK(hipMemset(h->range_flag, 0, sizeof flag));
    return fail(HQT_ERR_RANGE, "a SPLIT-precision call on this handle met an activation outside the fp16 range (NaN or |x| >= 65504): its output is "
                               "invalid; repeat the call with HQT_PRECISION_EXACT");
}

// ------------------------------------------------------------------------------------------ introspection
extern "C" int64_t hqt_param_count(const hqt_handle* h, int stage) { return (h && (stage == 1 || stage == 2)) ? h->params[stage] : -1; }
extern "C" int64_t hqt_workspace_bytes(const hqt_handle* h) { return h ? (int64_t)h->workspace_bytes : -1; }
extern "C" int hqt_timing_enable(hqt_handle* h, int on) { if (!h) return fail(HQT_ERR_INVALID, "null"); timing_collect(h); h->timing = on != 0; return HQT_OK; }
extern "C" int hqt_timing_reset(hqt_handle* h) {
    if (!h) return fail(HQT_ERR_INVALID, "null");
    timing_collect(h);
    for (auto& s : h->slots) { s.launches = 0; s.total_ms = 0.0; }
    return HQT_OK;
}
extern "C" int hqt_timing_slots(const hqt_handle* h) { return h ? (int)h->slots.size() : -1; }
extern "C" int hqt_timing_get(hqt_handle* h, int slot, char* name, int name_len, int64_t* launches, double* total_ms) {
    if (!h || slot < 0 || slot >= (int)h->slots.size()) return fail(HQT_ERR_INVALID, "bad slot");
    timing_collect(h);
    const TimingSlot& s = h->slots[slot];
    if (name && name_len > 0) { strncpy(name, s.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (launches) *launches = s.launches;
    if (total_ms) *total_ms = s.total_ms;
    return HQT_OK;
}
