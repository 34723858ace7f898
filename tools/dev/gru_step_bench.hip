// Dev timing of the one-step GRU kernels (one GRU time step of many streams; not part of the product):
//   dfx_k_gru_step_h3  — fp16-split: 64 vs 32 hidden units per workgroup;
//   dfx_k_gru_step_x32 — exact fp32: the same two shapes, against the two-launch form it replaces (dfx_k_proj256 writes gi, dfx_k_gru_rec_x32
//                        runs one step from it), with the two forms' new states compared.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 [-DDFX_GST_ABLATE=n] -I../../include
//         -I../../deepfilternet_amd/csrc/env_hip -I../../deepfilternet_amd/csrc gru_step_bench.hip -o gru_step_bench;  ./gru_step_bench [streams]
#include "dfx_nn_kernels.h"
#include <algorithm>
#include <functional>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
void dfx_set_error(const char *, ...) {}
bool dfx_prof_on(int) { return false; }
void dfx_prof_begin(int, hipStream_t) {}
void dfx_prof_end(int, hipStream_t) {}
struct Times { float lo, med, hi; };   // us per step: fastest, median and slowest of 15 timed runs of 10 back-to-back steps
static Times time_steps(const std::function<void()> &step) {
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<float> t;
    for (int it = 0; it < 16; ++it) {
        CK(hipEventRecord(a, 0));
        for (int r = 0; r < 10; ++r) step();
        CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (it > 0) t.push_back(ms * 100.f);   // (the first run warms up)
    }
    CK(hipGetLastError());
    std::sort(t.begin(), t.end());
    return Times{t.front(), t[t.size() / 2], t.back()};
}
template <typename K> static Times run(K kern, DfxGstArgs A, int nu, size_t smem) {
    CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int nblk = (int)(((A.B + DFX_PH_BM - 1) / DFX_PH_BM + 7) / 8 * 8) * nu;
    return time_steps([&] { hipLaunchKernelGGL(kern, dim3(nblk), dim3(DFX_PH_THREADS), smem, 0, A); });
}
static float frand() { return (float)rand() / (float)RAND_MAX - 0.5f; }
int main(int argc, char **argv) {
    const int64_t B = argc > 1 ? atoll(argv[1]) : 4096;
    const int H = 256;
    float *x, *hin, *ho4, *ho2, *y, *bi, *bhn; dfx_h8 *wi, *wh;
    const size_t wbytes = (size_t)12 * DFX_PH_CHUNK_H8 * 16;
    CK(hipMalloc(&x, B * 1024)); CK(hipMalloc(&hin, B * 1024)); CK(hipMalloc(&ho4, B * 1024)); CK(hipMalloc(&ho2, B * 1024)); CK(hipMalloc(&y, B * 1024));
    CK(hipMalloc(&bi, 3072)); CK(hipMalloc(&bhn, 1024)); CK(hipMalloc(&wi, wbytes)); CK(hipMalloc(&wh, wbytes));
    std::vector<float> h(B * 256); for (auto &v : h) v = frand();
    CK(hipMemcpy(x, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    for (auto &v : h) v = frand();
    CK(hipMemcpy(hin, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint16_t> w(wbytes / 2); for (size_t i = 0; i < w.size(); ++i) w[i] = dfx_f32_to_f16_bits(frand() * ((i / 512) & 1 ? 1e-3f : 1.f));
    CK(hipMemcpy(wi, w.data(), wbytes, hipMemcpyHostToDevice));
    for (size_t i = 0; i < w.size(); ++i) w[i] = dfx_f32_to_f16_bits(frand() * ((i / 512) & 1 ? 1e-3f : 1.f));
    CK(hipMemcpy(wh, w.data(), wbytes, hipMemcpyHostToDevice));
    CK(hipMemset(bi, 0, 3072)); CK(hipMemset(bhn, 0, 1024));
    DfxGstArgs A; A.x = x; A.h_in = hin; A.h_out = ho4; A.y = y; A.wif = wi; A.whf = wh; A.bias_i = bi; A.bhn = bhn; A.unscale_i = 1.f / 16; A.unscale_h = 1.f / 16;
    A.B = B; A.xrm = DfxRowMap{0, 0, 0}; A.yrm = DfxRowMap{0, 0, 0};
    const Times t4 = run(dfx_k_gru_step_h3<4>, A, 4, DFX_PH_SMEM);
    A.h_out = ho2;
    const Times t2 = run(dfx_k_gru_step_h3<2>, A, 8, DFX_PH_SMEM / 2);
    std::vector<float> a4(B * 256), a2(B * 256);
    CK(hipMemcpy(a4.data(), ho4, B * 1024, hipMemcpyDeviceToHost)); CK(hipMemcpy(a2.data(), ho2, B * 1024, hipMemcpyDeviceToHost));
    size_t diff = 0; double sum = 0; for (size_t i = 0; i < a4.size(); ++i) { diff += memcmp(&a4[i], &a2[i], 4) != 0; sum += fabs(a4[i]); }
    printf("B=%lld split: 64 units per workgroup %.2f us, 32 units per workgroup %.2f us per launch (back to back); outputs differ in %zu of %zu values, mean |h| %.4f\n",
           (long long)B, t4.lo, t2.lo, diff, a4.size(), sum / a4.size());
    // ---- exact fp32: weights W[768][256] (PyTorch's layout) scaled like a trained layer's, packed the way prep_gru packs them
    std::vector<float> wih((size_t)3 * H * H), whh((size_t)3 * H * H), bias(3 * H), bh(H);
    for (auto &v : wih) v = 0.125f * frand();
    for (auto &v : whh) v = 0.125f * frand();
    for (auto &v : bias) v = 0.2f * frand();
    for (auto &v : bh) v = 0.2f * frand();
    auto pack_x32 = [&](const std::vector<float> &W) {   // [16-unit tile][k-chunk][gate][half][lane][4]
        std::vector<float> d((size_t)3 * H * H);
        for (int ut = 0; ut < 16; ++ut)
            for (int kc = 0; kc < 8; ++kc)
                for (int gate = 0; gate < 3; ++gate)
                    for (int half = 0; half < 2; ++half)
                        for (int l = 0; l < 64; ++l)
                            for (int i = 0; i < 4; ++i) {
                                const int unit = 16 * ut + (l & 15), k = 32 * kc + 8 * (l >> 4) + 4 * half + i;
                                d[(((((size_t)ut * 8 + kc) * 3 + gate) * 2 + half) * 64 + l) * 4 + i] = W[(size_t)(gate * H + unit) * H + k];
                            }
        return d;
    };
    std::vector<float> wt((size_t)3 * H * H);   // W_ih^T [256][768] (dfx_k_proj256)
    for (int n = 0; n < 3 * H; ++n)
        for (int k = 0; k < H; ++k) wt[(size_t)k * 3 * H + n] = wih[(size_t)n * H + k];
    float *wix, *whx, *wtd, *gi, *hr, *yr;
    CK(hipMalloc(&wix, wih.size() * 4)); CK(hipMalloc(&whx, whh.size() * 4)); CK(hipMalloc(&wtd, wt.size() * 4));
    CK(hipMalloc(&gi, B * 3 * H * 4)); CK(hipMalloc(&hr, B * 1024)); CK(hipMalloc(&yr, B * 1024));
    const std::vector<float> pi = pack_x32(wih), ph = pack_x32(whh);
    CK(hipMemcpy(wix, pi.data(), pi.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(whx, ph.data(), ph.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(wtd, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(bi, bias.data(), 3072, hipMemcpyHostToDevice)); CK(hipMemcpy(bhn, bh.data(), 1024, hipMemcpyHostToDevice));
    A.wif = reinterpret_cast<const dfx_h8 *>(wix), A.whf = reinterpret_cast<const dfx_h8 *>(whx), A.unscale_i = A.unscale_h = 1.f;
    A.h_out = ho4;
    const Times x4 = run(dfx_k_gru_step_x32<4>, A, 4, DFX_PH_SMEM);
    A.h_out = ho2;
    const Times x2 = run(dfx_k_gru_step_x32<2>, A, 8, DFX_PH_SMEM / 2);
    // the two-launch form with the grids launch_proj / launch_gru_h3 give it (one step: T = 1, no XCD mask)
    DfxPjArgs P; P.a = x; P.w = wtd; P.bias = bi; P.out = gi; P.M = B; P.N = 3 * H; P.ncol = 3 * H / DFX_PJ_BN;
    int ncu = 256;
    { hipDeviceProp_t pr; CK(hipGetDeviceProperties(&pr, 0)); ncu = pr.multiProcessorCount; }
    const int64_t max_groups = ((B + 15) / 16 + DFX_PJ_THREADS / 64 - 1) / (DFX_PJ_THREADS / 64);
    int64_t rg = (int64_t)16 * ((ncu / 8) / P.ncol);
    rg = std::min<int64_t>(std::max<int64_t>(rg, 8), max_groups);
    P.rgroups = (int)rg;
    const int pblk = (int)((rg + 7) / 8 * 8 * P.ncol);
    DfxGhArgs G; G.gi = gi; G.whf = reinterpret_cast<const dfx_h8 *>(whx); G.bhn = bhn; G.h_in = hin; G.h_out = hr; G.y = yr; G.B = B; G.T = 1; G.t0 = 0; G.t1 = 1;
    G.unscale = 1.f; G.xcd_mask = 0;
    CK(hipFuncSetAttribute((const void *)dfx_k_proj256<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DFX_PJ_SMEM));
    CK(hipFuncSetAttribute((const void *)dfx_k_gru_rec_x32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DFX_GH_SMEM));
    const int gblk = (int)((B + DFX_GH_ROWS - 1) / DFX_GH_ROWS);
    const Times tp = time_steps([&] { hipLaunchKernelGGL(dfx_k_proj256<0>, dim3(pblk), dim3(DFX_PJ_THREADS), DFX_PJ_SMEM, 0, P); });
    const Times tr = time_steps([&] { hipLaunchKernelGGL(dfx_k_gru_rec_x32, dim3(gblk), dim3(DFX_GH_THREADS), DFX_GH_SMEM, 0, G); });
    const Times tw = time_steps([&] {
        hipLaunchKernelGGL(dfx_k_proj256<0>, dim3(pblk), dim3(DFX_PJ_THREADS), DFX_PJ_SMEM, 0, P);
        hipLaunchKernelGGL(dfx_k_gru_rec_x32, dim3(gblk), dim3(DFX_GH_THREADS), DFX_GH_SMEM, 0, G);
    });
    // the two decoders' stacks run side by side on two streams (run_gru_stack's `twin`): a pair of steps in each form, second stream's outputs discarded
    hipStream_t s1, s2; CK(hipStreamCreate(&s1)); CK(hipStreamCreate(&s2));
    hipEvent_t fork, join; CK(hipEventCreateWithFlags(&fork, hipEventDisableTiming)); CK(hipEventCreateWithFlags(&join, hipEventDisableTiming));
    float *ho_b, *y_b, *gi_b; CK(hipMalloc(&ho_b, B * 1024)); CK(hipMalloc(&y_b, B * 1024)); CK(hipMalloc(&gi_b, B * 3 * H * 4));
    auto pair = [&](const std::function<void(hipStream_t, bool)> &one) {
        return time_steps([&] {
            CK(hipEventRecord(fork, 0)); CK(hipStreamWaitEvent(s1, fork, 0)); CK(hipStreamWaitEvent(s2, fork, 0));
            one(s1, false); one(s2, true);
            CK(hipEventRecord(join, s1)); CK(hipStreamWaitEvent(0, join, 0)); CK(hipEventRecord(join, s2)); CK(hipStreamWaitEvent(0, join, 0));
        });
    };
    const int rb8 = (int)(((B + DFX_PH_BM - 1) / DFX_PH_BM + 7) / 8 * 8);
    const Times p4 = pair([&](hipStream_t st, bool second) {
        DfxGstArgs A2 = A; A2.h_out = second ? ho_b : ho4; A2.y = second ? y_b : y;
        hipLaunchKernelGGL(dfx_k_gru_step_x32<4>, dim3(rb8 * 4), dim3(DFX_PH_THREADS), DFX_PH_SMEM, st, A2);
    });
    const Times p2 = pair([&](hipStream_t st, bool second) {
        DfxGstArgs A2 = A; A2.h_out = second ? ho_b : ho2; A2.y = second ? y_b : y;
        hipLaunchKernelGGL(dfx_k_gru_step_x32<2>, dim3(rb8 * 8), dim3(DFX_PH_THREADS), DFX_PH_SMEM / 2, st, A2);
    });
    const Times pw = pair([&](hipStream_t st, bool second) {
        DfxPjArgs P2 = P; DfxGhArgs G2 = G;
        if (second) P2.out = gi_b, G2.gi = gi_b, G2.h_out = ho_b, G2.y = y_b;
        hipLaunchKernelGGL(dfx_k_proj256<0>, dim3(pblk), dim3(DFX_PJ_THREADS), DFX_PJ_SMEM, st, P2);
        hipLaunchKernelGGL(dfx_k_gru_rec_x32, dim3(gblk), dim3(DFX_GH_THREADS), DFX_GH_SMEM, st, G2);
    });
    CK(hipDeviceSynchronize());
    printf("B=%lld exact, two stacks side by side, us per pair of steps min / median / max (fork and join included): fused 64 units %.2f / %.2f / %.2f, "
           "fused 32 units %.2f / %.2f / %.2f, two launches %.2f / %.2f / %.2f\n",
           (long long)B, p4.lo, p4.med, p4.hi, p2.lo, p2.med, p2.hi, pw.lo, pw.med, pw.hi);
    std::vector<float> ar(B * 256);
    CK(hipMemcpy(a4.data(), ho4, B * 1024, hipMemcpyDeviceToHost)); CK(hipMemcpy(a2.data(), ho2, B * 1024, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ar.data(), hr, B * 1024, hipMemcpyDeviceToHost));
    double d42 = 0, d4r = 0; sum = 0;
    for (size_t i = 0; i < a4.size(); ++i) d42 = std::max(d42, (double)fabs(a4[i] - a2[i])), d4r = std::max(d4r, (double)fabs(a4[i] - ar[i])), sum += fabs(ar[i]);
    printf("B=%lld exact (ablate %d), us per step min / median / max of 15 runs: fused 64 units %.2f / %.2f / %.2f, fused 32 units %.2f / %.2f / %.2f, "
           "two launches %.2f / %.2f / %.2f (projection alone %.2f, recurrence alone %.2f)\n",
           (long long)B, (int)DFX_GST_ABLATE, x4.lo, x4.med, x4.hi, x2.lo, x2.med, x2.hi, tw.lo, tw.med, tw.hi, tp.lo, tr.lo);
    printf("B=%lld exact: max |h' fused 64 - fused 32| %.3g, max |h' fused 64 - two launches| %.3g, mean |h'| %.4f\n", (long long)B, d42, d4r, sum / ar.size());
    return 0;
}
