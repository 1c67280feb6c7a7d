// The library's environment switches: ONE table, read through ONE accessor (switches.hip is the only file of csrc/ that asks the
// environment).  DESIGN §7.1 is written from this table and tests/test_switches_host.py holds the two together.
//
// Plain C++, no HIP header: a host compiler builds switches.hip alone (that is how the test runs it).
//
// Parse kinds
//   SWP_PRESENT      1 when the variable is set, whatever its value ("0" included), else 0
//   SWP_ZERO_OFF     0 only when the variable is set and atoi() of it is 0, else 1
//   SWP_INT          atoi() of the variable, the default when it is unset
//   SWP_INT_MIN1     as SWP_INT, but at least 1
//   SWP_INT_8_OR_16  8 or 16 when atoi() gives one of them, else 0 (= not forced)
// Read times
//   SWR_ONCE         the first read of the switch in the process holds for good (thread-safe)
//   SWR_LIVE         every read asks the environment
//
// X(id, variable, parse kind, default, read time, effect, who flips it)
//   default: the value with the variable unset.  who: the tests / tools that set the variable; "A/B only" = nothing in the tree does.
#pragma once

#define SWITCH_TABLE(X)                                                                                                                              \
    /* per-handle values, taken at hqt_create (hqt_set_switch changes the three behind HQT_SWITCH_* afterwards) */                                   \
    X(NO_TILE_GEMM, "HQT_NO_TILE_GEMM", SWP_PRESENT, 0, SWR_LIVE, "merged passes through the streaming GEMMs instead of the tiled ones",             \
      "tools/fast_tile_error.py, tools/ar_pass_time.py, tests/test_gpu_merged_rows.py")                                                              \
    X(PERSIST, "HQT_PERSIST", SWP_ZERO_OFF, 1, SWR_LIVE, "0: the launch chain instead of the persistent AR launch (default of HQT_SWITCH_PERSIST)",  \
      "bench.py, tests/test_gpu_dist.py, tests/dist_gpu_worker.py, tests/test_gpu_persist.py, tools/collect_round_evidence.sh")                      \
    X(NO_SINGLE_KEY, "HQT_NO_SINGLE_KEY", SWP_PRESENT, 0, SWR_LIVE, "depth sub-step 0 the long way round (default of HQT_SWITCH_SINGLE_KEY)",        \
      "A/B only")                                                                                                                                    \
    X(SPLIT_KSLICES_OFF, "HQT_SPLIT_KSLICES_OFF", SWP_PRESENT, 0, SWR_LIVE, "SPLIT AR GEMMs never K-sliced (default of HQT_SWITCH_SPLIT_KSLICES)",   \
      "A/B only")                                                                                                                                    \
    /* at workspace allocation / at finalize / per allocation */                                                                                     \
    X(DEC_CHUNK, "HQT_DEC_CHUNK", SWP_INT, 64, SWR_LIVE, "images per decode pass (the caller clamps to [1, max_batch])", "A/B only")                 \
    X(PERSIST_BUILD_OFF, "HQT_PERSIST_BUILD_OFF", SWP_PRESENT, 0, SWR_LIVE, "no weight streams of the persistent chain packed at finalize",          \
      "A/B only")                                                                                                                                    \
    X(POISON_WORKSPACE, "HQT_POISON_WORKSPACE", SWP_PRESENT, 0, SWR_LIVE, "every workspace buffer filled with 0xFF when it is allocated",            \
      "the poisoned-engine fixtures of tests/test_gpu_*.py")                                                                                         \
    /* hooks that tests flip inside one process between calls: read per launch */                                                                    \
    X(FORCE_TILE128, "HQT_FORCE_TILE128", SWP_PRESENT, 0, SWR_LIVE, "big-tile MFMA kernels (halo conv, LDS-DMA GEMM) on shapes of few tiles",        \
      "tests/test_gpu_parity.py")                                                                                                                    \
    X(NO_HALO, "HQT_NO_HALO", SWP_PRESENT, 0, SWR_LIVE, "FAST 3x3 convs through the generic implicit GEMM instead of the halo-tile kernel",          \
      "tests/test_gpu_parity.py")                                                                                                                    \
    X(HALO_TY, "HQT_HALO_TY", SWP_INT_8_OR_16, 0, SWR_LIVE, "pixel rows per halo-conv tile, 8 or 16, instead of the choice by grid size",            \
      "tests/test_gpu_parity.py")                                                                                                                    \
    X(NO_FUSED_GN, "HQT_NO_FUSED_GN", SWP_PRESENT, 0, SWR_LIVE, "GroupNorm statistics by the separate pass instead of the halo conv's epilogue",     \
      "tests/test_gpu_parity.py, tools/launch_record.py")                                                                                            \
    X(NO_NARROW_OUT, "HQT_NO_NARROW_OUT", SWP_PRESENT, 0, SWR_LIVE, "FAST conv_out on 128-channel tiles instead of the 32-channel variant",          \
      "tests/test_gpu_parity.py")                                                                                                                    \
    X(NO_TILE64, "HQT_NO_TILE64", SWP_PRESENT, 0, SWR_LIVE, "LDS-DMA GEMMs of few tiles on 128-row tiles instead of 64-row ones", "A/B only")        \
    X(PREFILL_TILED, "HQT_PREFILL_TILED", SWP_PRESENT, 0, SWR_LIVE, "causal prefill of 5 .. 64 rows through attention_prefill_tiled_kernel",         \
      "tests/test_gpu_text_prefix.py")                                                                                                               \
    /* per process: the first read holds */                                                                                                          \
    X(TIMING_BY_ROWS, "HQT_TIMING_BY_ROWS", SWP_PRESENT, 0, SWR_ONCE, "one timing slot per (GEMM, row count)", "tools/ar_pass_time.py")              \
    X(PERSIST_NT, "HQT_PERSIST_NT", SWP_ZERO_OFF, 1, SWR_ONCE, "0: persistent chain's weight DMA without the non-temporal hint", "A/B only")         \
    X(NO_DLN, "HQT_NO_DLN", SWP_PRESENT, 0, SWR_ONCE, "classic LayerNorm kernels + split-K slabs instead of the deferred-LayerNorm GEMM epilogues",  \
      "A/B only")                                                                                                                                    \
    X(NO_FUSED_EMBED, "HQT_NO_FUSED_EMBED", SWP_PRESENT, 0, SWR_ONCE, "separate depth_embed_kernel instead of the sampler's fused embedding lookup", \
      "A/B only")                                                                                                                                    \
    X(GRAPH_POSITIONS, "HQT_GRAPH_POSITIONS", SWP_INT_MIN1, 16, SWR_ONCE, "most top positions per captured graph",                                   \
      "tools/sweep_graph_positions.sh")                                                                                                              \
    X(NO_EXACT_MFMA, "HQT_NO_EXACT_MFMA", SWP_PRESENT, 0, SWR_ONCE, "EXACT / SPLIT nn.Linear up to 256 rows through the vector-ALU tile kernel",     \
      "A/B only")                                                                                                                                    \
    X(SPLIT_PLANES_OUT, "HQT_SPLIT_PLANES_OUT", SWP_ZERO_OFF, 1, SWR_ONCE, "0: SPLIT decode with an operand pass instead of planes from the epilogue", \
      "tests/test_gpu_split.py (child processes)")                                                                                                   \
    X(SPLIT_UP, "HQT_SPLIT_UP", SWP_ZERO_OFF, 1, SWR_ONCE, "0: SPLIT upsampling convs as nine taps on the upsampled image",                          \
      "tests/test_gpu_split.py (child processes)")                                                                                                   \
    X(CONV_OUT_DIRECT, "HQT_CONV_OUT_DIRECT", SWP_ZERO_OFF, 1, SWR_ONCE, "0: SPLIT conv_out as operand pass + matrix-core kernel",                   \
      "tests/test_gpu_split.py (child processes)")                                                                                                   \
    X(NO_PLAIN_SAMPLER, "HQT_NO_PLAIN_SAMPLER", SWP_PRESENT, 0, SWR_ONCE, "FAST draws without cut-offs through the general sampler_kernel",          \
      "A/B only")                                                                                                                                    \
    X(NO_FEWQ_ATTN, "HQT_NO_FEWQ_ATTN", SWP_PRESENT, 0, SWR_ONCE, "depth sub-steps through attention_kernel instead of the few-query kernels",       \
      "tests/test_gpu_attention_paths.py (child processes)")                                                                                         \
    X(NO_FEWQ8, "HQT_NO_FEWQ8", SWP_PRESENT, 0, SWR_ONCE, "few-query attention one head per wave instead of eight",                                  \
      "tests/test_gpu_attention_paths.py (child processes)")                                                                                         \
    X(NO_HEADS8, "HQT_NO_HEADS8", SWP_PRESENT, 0, SWR_ONCE, "single-query attention of merged FAST passes through attention_kernel", "A/B only")

enum SwitchParse { SWP_PRESENT, SWP_ZERO_OFF, SWP_INT, SWP_INT_MIN1, SWP_INT_8_OR_16 };
enum SwitchRead { SWR_ONCE, SWR_LIVE };

enum Switch {
#define X(id, var, parse, dflt, read, effect, who) SW_##id,
    SWITCH_TABLE(X)
#undef X
    SW_COUNT
};

// the value of switch `s` under its row's parse kind and read time
int switch_value(Switch s);
