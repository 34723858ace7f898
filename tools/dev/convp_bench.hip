// Dev: dfx_k_df_convp_h3<64, 5> alone at the benchmark's shape (256 clips x 1002 frames x 96 bins, segments of 40 frames): the PS instance
// (pre-split patches, the batch passes' frame loop) against the unsplit instance (the loop as it was), outputs compared bit for bit, ms per
// launch of each, and — built with -DDFX_CPH_TRACE=1 — the s_memtime ticks per frame of the loop's parts.
//   -DDFX_CPH_ABLATE=1 / 2    no output stores / no patch loads (the comparison then only says that both forms were ablated alike)
//   -DDFX_CPH_VALU_C0=n -DDFX_CPH_VALU_TAPS=n   the vector instructions asked for in the shadow of each matrix op
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -Xclang -target-feature -Xclang -packed-fp32-ops
//        -Iinclude -Ideepfilternet_amd/csrc/env_hip -Ideepfilternet_amd/csrc tools/dev/convp_bench.hip -o tools/dev/_build/convp_bench
// usage: convp_bench [B [T [reps]]]
#include "dfx_nn_kernels.h"
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
void dfx_set_error(const char *, ...) {}
bool dfx_prof_on(int) { return false; }
void dfx_prof_begin(int, hipStream_t) {}
void dfx_prof_end(int, hipStream_t) {}
static float rnd() { return (float)rand() / (float)RAND_MAX - 0.5f; }
int main(int argc, char **argv) {
    constexpr int C = 64, KT = 5, KC = C / 32, NT = C / 16;
    const int64_t B = argc > 1 ? atoll(argv[1]) : 256, T = argc > 2 ? atoll(argv[2]) : 1002;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    const int Fd = 96, NO = 10, L = 2;
    if (B * T * Fd >= ((int64_t)1 << 29)) { printf("B * T * Fd must stay below 2^29 (32-bit element offsets)\n"); return 1; }
    srand(1);
    const size_t nfeat = (size_t)B * T * Fd;
    std::vector<float> hf(nfeat * 2);
    for (auto &v : hf) v = 2.f * rnd();
    std::vector<uint32_t> hps(nfeat * 2);   // dfx_pack_h3's layout: word 0 = f16 hi(re), hi(im); word 1 = the lo halves
    for (size_t i = 0; i < nfeat; ++i) {
        uint16_t h[2], l[2];
        for (int c = 0; c < 2; ++c) {
            const float x = hf[2 * i + c];
            h[c] = dfx_f32_to_f16_bits(x);
            l[c] = dfx_f32_to_f16_bits(x - dfx_f16_bits_to_f32(h[c]));
        }
        hps[2 * i] = h[0] | ((uint32_t)h[1] << 16), hps[2 * i + 1] = l[0] | ((uint32_t)l[1] << 16);
    }
    auto frags = [](size_t n, float scale) {
        std::vector<uint16_t> w(n * 8);
        for (auto &v : w) v = dfx_f32_to_f16_bits(rnd() * scale);
        return w;
    };
    const std::vector<uint16_t> hw0 = frags((size_t)NT * 2 * 64, 0.5f), hw = frags((size_t)KT * KC * 2 * 64, 0.25f);
    std::vector<float> hb0(C), hb(16);
    for (auto &v : hb0) v = 0.2f * rnd();
    for (auto &v : hb) v = 0.2f * rnd();
    float *feat, *bias0, *bias, *out[2];
    uint2 *fps;
    dfx_h8 *w0f, *wf;
    unsigned int *err;
    const size_t nout = (size_t)B * (NO / 2) * T * Fd * 2;
    CK(hipMalloc(&feat, hf.size() * 4)); CK(hipMalloc(&fps, hps.size() * 4)); CK(hipMalloc(&w0f, hw0.size() * 2)); CK(hipMalloc(&wf, hw.size() * 2));
    CK(hipMalloc(&bias0, C * 4)); CK(hipMalloc(&bias, 64)); CK(hipMalloc(&err, 256)); CK(hipMemset(err, 0, 256));
    for (auto &o : out) { CK(hipMalloc(&o, nout * 4)); CK(hipMemset(o, 0xff, nout * 4)); }
    CK(hipMemcpy(feat, hf.data(), hf.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(fps, hps.data(), hps.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w0f, hw0.data(), hw0.size() * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(wf, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(bias0, hb0.data(), C * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(bias, hb.data(), 64, hipMemcpyHostToDevice));
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    DfxCphArgs A;   // as launch_convp_h3 fills it (DFX_CONVP_GRAIN = 16)
    A.feat = feat; A.feat_ps = nullptr; A.w0f = w0f; A.bias0 = bias0; A.wf = wf; A.bias = bias; A.out = out[0];
    A.B = B; A.T = T; A.Fd = Fd; A.NO = NO; A.L = L; A.t_begin = 0; A.t_zero = 0; A.t_end = T; A.unscale0 = 1.f / 16.f; A.unscale = 1.f / 32.f; A.err = err;
    A.nfb = (Fd + 15) / 16;
    int64_t nseg = ((int64_t)cus * 4 * 4 * 16 + B * A.nfb - 1) / (B * A.nfb);
    nseg = std::max<int64_t>(1, std::min(nseg, (T + 8 * KT - 1) / (8 * KT)));
    const int64_t tseg = (((T + nseg - 1) / nseg) + KT - 1) / KT * KT;
    A.tseg = (int)tseg; A.nseg = (int)((T + tseg - 1) / tseg);
    const int64_t nruns = B * A.nfb * A.nseg;
    const int grid = (int)std::min<int64_t>((nruns + 3) / 4, (int64_t)cus * 32);
    printf("%lld clips x %lld frames: %d segments of %d frames, %lld runs on %d workgroups, %d CUs\n", (long long)B, (long long)T, A.nseg, A.tseg,
           (long long)nruns, grid, cus);
#if DFX_CPH_TRACE
    unsigned long long *trace; CK(hipMalloc(&trace, (size_t)grid * 5 * 8)); CK(hipMemset(trace, 0, (size_t)grid * 5 * 8));
#endif
    auto run = [&](int form) -> std::vector<float> {   // form 0: the unsplit instance, 1: the PS instance; ms of every repetition, sorted
        DfxCphArgs R = A;
        R.out = out[form]; R.feat_ps = form ? fps : nullptr;
#if DFX_CPH_TRACE
        R.trace = trace;
#endif
        std::vector<float> ms(reps);
        hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
        for (int it = 0; it < reps; ++it) {
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(a, 0));
            if (form) hipLaunchKernelGGL((dfx_k_df_convp_h3<C, KT, true>), dim3(grid), dim3(256), 0, 0, R);
            else hipLaunchKernelGGL((dfx_k_df_convp_h3<C, KT, false>), dim3(grid), dim3(256), 0, 0, R);
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            CK(hipGetLastError());
            CK(hipEventElapsedTime(&ms[it], a, b));
        }
        std::sort(ms.begin(), ms.end());
        return ms;
    };
    for (int form = 0; form < 2; ++form) {
        const std::vector<float> ms = run(form);
        printf("%s instance: median %.3f min %.3f max %.3f ms of %d launches\n", form ? "PS" : "unsplit", ms[reps / 2], ms[0], ms[reps - 1], reps);
#if DFX_CPH_TRACE
        std::vector<unsigned long long> h((size_t)grid * 5);
        CK(hipMemcpy(h.data(), trace, h.size() * 8, hipMemcpyDeviceToHost));
        double s[5] = {0, 0, 0, 0, 0};
        for (int g = 0; g < grid; ++g)
            for (int i = 0; i < 5; ++i) s[i] += (double)h[(size_t)g * 5 + i];
        printf("  s_memtime ticks per frame, wave 0 of every workgroup (%.0f frames): patch wait %.1f, c0%s %.1f, taps %.1f, stores %.1f, all %.1f\n", s[4],
               s[0] / s[4], form ? " + taps (one block)" : "", s[1] / s[4], s[2] / s[4], s[3] / s[4], (s[0] + s[1] + s[2] + s[3]) / s[4]);
#endif
    }
    std::vector<float> h0(nout), h1(nout);
    CK(hipMemcpy(h0.data(), out[0], nout * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h1.data(), out[1], nout * 4, hipMemcpyDeviceToHost));
    size_t nbad = 0, nz = 0;
    for (size_t j = 0; j < nout; ++j) nbad += memcmp(&h0[j], &h1[j], 4) != 0, nz += h0[j] != 0.f;
    unsigned int herr[4]; CK(hipMemcpy(herr, err, 16, hipMemcpyDeviceToHost));
    printf("outputs: %zu of %zu values differ between the instances (%zu non-zero); range guard raised %u\n", nbad, nout, nz, herr[1]);
    return nbad != 0;
}
