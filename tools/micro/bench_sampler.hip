// Micro-benchmark: the fused sampler at merged-pass row counts (V = 8192), plain / top-k / top-k + top-p, and a row table (hqt_set_row_samplers)
// that mixes them: FAST runs both kernels over the pass, each leaving the other one's rows at once.
#include "../../hqtransformer_amd/csrc/kernels.hip"
#include "../../hqtransformer_amd/csrc/switches.hip"
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
int main() {
    hipStream_t st; CK(hipStreamCreate(&st));
    const int V = 8192, B = 2048;
    float* logits; CK(hipMalloc(&logits, (size_t)4 * B * V * 4));
    {
        std::vector<float> h((size_t)4 * B * V);
        unsigned s = 99u;
        for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 9) - (1 << 22)) * (4.0f / (1 << 22)); }
        CK(hipMemcpy(logits, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    StepState* state; CK(hipMalloc(&state, sizeof(StepState))); CK(hipMemset(state, 0, sizeof(StepState)));
    RowKey* rows; CK(hipMalloc(&rows, B * sizeof(RowKey)));
    CK(launch_set_rows(rows, B, 1234, 0, st));
    int64_t* out; CK(hipMalloc(&out, (size_t)B * 64 * 4 * 8));
    for (int fm = 0; fm < 2; ++fm)
    for (int mode = 0; mode < 3; ++mode) {
        for (int slots : {1, 4})
        for (int B : {512, 2048}) {
            if (slots == 1 && B != 512) continue;
            SamplerArgs a{};
            a.fast_math = fm;
            a.logits = logits; a.R = B * slots; a.V = V; a.slots = slots; a.B = B; a.temperature = 1.0f;
            a.top_k = mode >= 1 ? 2048 : 0; a.top_p = mode >= 2 ? 1.0f : 0.0f; a.draw0 = slots == 1 ? 0 : 1;
            a.state = state; a.rows = rows; a.n_steps = 64; a.out = out; a.draws = 5;
            CK(sampler_configure(V, a.top_p > 0.0f));
            CK(launch_sampler(a, st)); CK(hipStreamSynchronize(st));
            hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
            CK(hipEventRecord(e0, st));
            for (int r = 0; r < 20; ++r) CK(launch_sampler(a, st));
            CK(hipEventRecord(e1, st)); CK(hipStreamSynchronize(st));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            printf("%-22s %-10s rows %4d : %8.2f us per launch\n", mode == 0 ? "plain" : (mode == 1 ? "top_k 2048" : "top_k 2048 + top_p 1"), fm ? "fast-math" : "IEEE", a.R, 1000.f * ms / 20);
        }
    }
    // mixed passes: half of the samples without a cut-off, half with top_k 2048 at T 0.95 (alternating steps of 64 samples); then the same with one top-p
    // sample per 64 (the general kernel is launched with 99 KB of LDS per workgroup: also for the workgroups that leave at once).  "all plain" and
    // "all top_k" tables show what the second launch costs over the uniform figures above.
    RowSampler* table; CK(hipMalloc(&table, B * sizeof(RowSampler)));
    for (int fm = 0; fm < 2; ++fm)
    for (int mix = 0; mix < 4; ++mix) {
        std::vector<RowSampler> h(B);
        for (int b = 0; b < B; ++b) {
            const bool cut = mix == 1 || (mix >= 2 && (b / 64) % 2 == 1), p = mix == 3 && b % 64 == 63;
            for (int l = 0; l < 3; ++l) { h[b].temperature[l] = cut ? 0.95f : 1.0f; h[b].top_k[l] = cut ? 2048 : 0; h[b].top_p[l] = p ? 0.9f : 0.0f; }
        }
        CK(hipMemcpy(table, h.data(), B * sizeof(RowSampler), hipMemcpyHostToDevice));
        for (int slots : {1, 4})
        for (int B : {512, 2048}) {
            if (slots == 1 && B != 512) continue;
            SamplerArgs a{};
            a.fast_math = fm;
            a.logits = logits; a.R = B * slots; a.V = V; a.slots = slots; a.B = B; a.temperature = 1.0f; a.draw0 = slots == 1 ? 0 : 1;
            a.state = state; a.rows = rows; a.n_steps = 64; a.out = out; a.draws = 5;
            a.row_set = table; a.row_lv_t = a.row_lv_k = slots == 1 ? 0 : 1; a.row_top_p = mix == 3;
            CK(sampler_configure(V, mix == 3));
            CK(launch_sampler(a, st)); CK(hipStreamSynchronize(st));
            hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
            CK(hipEventRecord(e0, st));
            for (int r = 0; r < 20; ++r) CK(launch_sampler(a, st));
            CK(hipEventRecord(e1, st)); CK(hipStreamSynchronize(st));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            static const char* const names[4] = {"table: all plain", "table: all top_k", "table: half / half", "table: half / half + top_p"};
            printf("%-28s %-10s rows %4d : %8.2f us per pass\n", names[mix], fm ? "fast-math" : "IEEE", a.R, 1000.f * ms / 20);
        }
    }
    return 0;
}
