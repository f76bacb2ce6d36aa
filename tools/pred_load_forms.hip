// pred_load_forms.hip — the two ways to put ONE sample's counts (already in HBM) into the k-mer-major genotype matrix G[nk][ns]
// (include/dbtk_pred.h: dbtk_pred_load_ctx), timed by HIP events:
//   (a) column   one lane per k-mer, nk 4-byte stores at a stride of 4 * ns bytes               (what the library does)
//   (b) staged   the sample's 8 * nk bytes are copied into a staging buffer of T samples; when T wait, one launch of the
//                LDS-turned tile kernel (k_pred_load's shape: 64 k-mers x 32 samples per wave) writes runs of 128 bytes
// k_col and k_tile are COPIES of k_pred_load_col and k_pred_load (danbing-tk_amd/csrc/dbtk_pred.hip): keep them in step with the
// library's kernels, or the figures in DESIGN 7 speak of something else.
// Usage: pred_load_forms [nk = 14750000] [T = 32] [ns ...  = 64 879]      (one JSON line per ns; DESIGN 7 has the figures)
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/pred_load_forms tools/pred_load_forms.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void __launch_bounds__(256) k_col(const uint64_t* __restrict__ counts, float depth, float* __restrict__ G, uint64_t nk, uint64_t ns, uint64_t sample) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < nk; k += (uint64_t)gridDim.x * 256) G[k * ns + sample] = (float)counts[k] / depth;
}
constexpr int PT_K = 64, PT_S = 32;
__global__ void __launch_bounds__(64) k_tile(const uint64_t* __restrict__ counts, const float* __restrict__ depth, float* __restrict__ G, uint64_t nk, uint64_t ns,
                                             uint64_t first, uint32_t n) {
    __shared__ float tile[PT_K][PT_S + 1];
    const int lane = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * PT_K;
    for (uint32_t i0 = blockIdx.y * PT_S; i0 < n; i0 += gridDim.y * PT_S) {
        const uint32_t ni = n - i0 < (uint32_t)PT_S ? n - i0 : (uint32_t)PT_S;
        for (uint32_t i = 0; i < ni; ++i) {
            const uint64_t k = k0 + lane;
            tile[lane][i] = k < nk ? (float)counts[(uint64_t)(i0 + i) * nk + k] / depth[i0 + i] : 0.f;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int r = lane / PT_S; r < PT_K; r += 64 / PT_S) {
            const uint32_t i = lane % PT_S;
            if (k0 + r < nk && i < ni) G[(k0 + r) * ns + first + i0 + i] = tile[r][i];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}
__global__ void k_fill(uint64_t* c, uint64_t n, uint64_t salt) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) c[i] = (i * 2654435761ull + salt) % 977;
}
// order-independent digest of the first T columns of G (the two forms must leave the same bits)
__global__ void k_digest(const float* G, uint64_t nk, uint64_t ns, uint64_t T, unsigned long long* out) {
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nk * T; i += (uint64_t)gridDim.x * 256) {
        const uint64_t k = i / T, s = i % T;
        acc += (unsigned long long)__float_as_uint(G[k * ns + s]) * (i | 1);
    }
    atomicAdd(out, acc);
}

int main(int argc, char** argv) {
    const uint64_t nk = argc > 1 ? strtoull(argv[1], nullptr, 10) : 14750000ull;
    const uint64_t T = argc > 2 ? strtoull(argv[2], nullptr, 10) : 32;
    std::vector<uint64_t> nss;
    for (int i = 3; i < argc; ++i) nss.push_back(strtoull(argv[i], nullptr, 10));
    if (nss.empty()) nss = {64, 879};
    if (!nk || !T || T > 4096) { fprintf(stderr, "bad arguments\n"); return 1; }
    hipStream_t s;
    CHK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    uint64_t *d_counts = nullptr, *d_stage = nullptr;
    float* d_depth = nullptr;
    unsigned long long* d_dig = nullptr;
    CHK(hipMalloc(&d_counts, nk * 8)); CHK(hipMalloc(&d_stage, T * nk * 8)); CHK(hipMalloc(&d_depth, T * 4)); CHK(hipMalloc(&d_dig, 8));
    std::vector<float> depth(T);
    for (uint64_t i = 0; i < T; ++i) depth[i] = 20.f + (float)i * 0.37f;
    CHK(hipMemcpy(d_depth, depth.data(), T * 4, hipMemcpyHostToDevice));
    const uint32_t nb = (uint32_t)std::min<uint64_t>((nk + 255) / 256, 1u << 16);
    for (uint64_t ns : nss) {
        if (ns < T) { fprintf(stderr, "ns %llu < T\n", (unsigned long long)ns); continue; }
        float* G = nullptr;
        CHK(hipMalloc(&G, nk * ns * 4));
        unsigned long long dig[2] = {0, 0};
        float ms_a = 0, ms_b = 0, ms_copy = 0, ms_tile = 0;
        for (int form = 0; form < 2; ++form) {
            CHK(hipMemsetAsync(G, 0, nk * ns * 4, s));
            for (int rep = 0; rep < 2; ++rep) {  // the second pass is the one reported
                float tot = 0, tcopy = 0, ttile = 0;
                for (uint64_t i = 0; i < T; ++i) {
                    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, s, d_counts, nk, i * 7919);  // "the context's accumulators" of sample i
                    float ms = 0;
                    CHK(hipEventRecord(e0, s));
                    if (form == 0) hipLaunchKernelGGL(k_col, dim3(nb), dim3(256), 0, s, d_counts, depth[i], G, nk, ns, i);
                    else CHK(hipMemcpyAsync(d_stage + i * nk, d_counts, nk * 8, hipMemcpyDeviceToDevice, s));
                    CHK(hipEventRecord(e1, s));
                    CHK(hipStreamSynchronize(s));
                    CHK(hipEventElapsedTime(&ms, e0, e1));
                    tot += ms; tcopy += form ? ms : 0;
                }
                if (form == 1) {
                    float ms = 0;
                    CHK(hipEventRecord(e0, s));
                    hipLaunchKernelGGL(k_tile, dim3((uint32_t)((nk + PT_K - 1) / PT_K), (uint32_t)((T + PT_S - 1) / PT_S)), dim3(64), 0, s, d_stage, d_depth, G, nk, ns, (uint64_t)0, (uint32_t)T);
                    CHK(hipEventRecord(e1, s));
                    CHK(hipStreamSynchronize(s));
                    CHK(hipEventElapsedTime(&ms, e0, e1));
                    tot += ms; ttile = ms;
                }
                CHK(hipGetLastError());
                if (form == 0) ms_a = tot / T; else { ms_b = tot / T; ms_copy = tcopy / T; ms_tile = ttile / T; }
            }
            CHK(hipMemsetAsync(d_dig, 0, 8, s));
            hipLaunchKernelGGL(k_digest, dim3(4096), dim3(256), 0, s, G, nk, ns, T, d_dig);
            CHK(hipMemcpyAsync(&dig[form], d_dig, 8, hipMemcpyDeviceToHost, s));
            CHK(hipStreamSynchronize(s));
        }
        printf("{\"nk\": %llu, \"ns\": %llu, \"T\": %llu, \"column_ms_per_sample\": %.4f, \"staged_ms_per_sample\": %.4f, \"staged_copy_ms\": %.4f, \"staged_tile_ms\": %.4f, "
               "\"stage_bytes\": %llu, \"same_bits\": %s}\n",
               (unsigned long long)nk, (unsigned long long)ns, (unsigned long long)T, ms_a, ms_b, ms_copy, ms_tile, (unsigned long long)(T * nk * 8), dig[0] == dig[1] ? "true" : "false");
        fflush(stdout);
        CHK(hipFree(G));
    }
    return 0;
}
