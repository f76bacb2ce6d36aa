// danbing-tk-pred on the GPU (include/dbtk_pred.h): the cohort's genotype matrix G[nk][ns] (float32) stays in HBM; three
// streaming kernels restate src/pred.h:204-233 of the reference.  HBM-bound float column work: no MFMA, nothing to tile
// but the transposition of the per-sample count vectors into the sample-minor matrix.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dbtk_pred.h"
#include "dbtk_dev.h"
#include "dbtk_internal.h"
#include "dbtk_pred_plan.h"

using namespace dbtk;

// ---- locus t of ikmer.meta: its k-mers [si, ei) and its invariant k-mers [isi, iei).  bias_correction leaves a locus that lacks
// either alone (pred.h:219-220): its Bias row stays 0, its columns are not divided.
struct LocusSpan {
    uint32_t si, ei, isi, iei;
    __host__ __device__ bool skipped() const { return si == ei || isi == iei; }
};
__host__ __device__ __forceinline__ LocusSpan locus_span(const uint32_t* __restrict__ nk_cum, const uint32_t* __restrict__ nik_cum, uint64_t t) {
    return LocusSpan{t ? nk_cum[t - 1] : 0u, nk_cum[t], t ? nik_cum[t - 1] : 0u, nik_cum[t]};
}

// ---- load_eachBinGT + norm_rd (pred.h:166-186, 204-209): counts[i][k] (u64, sample-major as the files are) ->
// (float)count / depth[i], handed to store(k, i, value).  One wave per tile of 64 k-mers x 32 samples: the counts are read along k
// (coalesced), turned in LDS, and stored along the samples (runs of 128 bytes); the blocks of a column of the grid stride over the
// samples.  N: the width of the sample index (n samples, of `rows` counts each).
constexpr int PT_K = 64, PT_S = 32;
template <class N, class Store>
__device__ __forceinline__ void pred_tile(const uint64_t* __restrict__ counts, const float* __restrict__ depth, uint64_t rows, N n, Store store) {
    __shared__ float tile[PT_K][PT_S + 1];
    const int lane = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * PT_K;
    for (N i0 = (N)blockIdx.y * PT_S; i0 < n; i0 += (N)gridDim.y * PT_S) {
        const uint32_t ni = n - i0 < (N)PT_S ? (uint32_t)(n - i0) : (uint32_t)PT_S;
        for (uint32_t i = 0; i < ni; ++i) {
            const uint64_t k = k0 + lane;
            // uint64 -> float and the division are each one correctly rounded IEEE operation, as Eigen's cast<float>() and operator/
            tile[lane][i] = k < rows ? (float)counts[(uint64_t)(i0 + i) * rows + k] / depth[i0 + i] : 0.f;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int r = lane / PT_S; r < PT_K; r += 64 / PT_S) {  // two rows per pass: lanes 0-31 / 32-63 along the samples
            const uint32_t i = lane % PT_S;
            if (k0 + r < rows && i < ni) store(k0 + r, i0 + i, tile[r][i]);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}
// n samples from `first` on into the matrix: G[k][first + i]
__global__ void __launch_bounds__(64) k_pred_load(const uint64_t* __restrict__ counts, const float* __restrict__ depth, float* __restrict__ G,
                                                  uint64_t nk, uint64_t ns, uint64_t first, uint32_t n) {
    pred_tile(counts, depth, nk, n, [=](uint64_t k, uint32_t i, float g) { G[k * ns + first + i] = g; });
}

// ---- one sample whose counts are already in HBM (dbtk_pred_load_ctx / dbtk_pred_load_device with n = 1): column `sample` of G.
// One lane per k-mer: the counts are read coalesced (8 bytes per lane), every store is 4 bytes into a row of its own (row stride
// 4 * ns bytes), so the column costs nk partial-line writes.  Measured against the staged, LDS-turned form: kept,
// because next to a sample's batch loop neither is visible and this one needs no staging buffer and no flush before G is read.
// The arithmetic is k_pred_load's: one conversion, one division, both correctly rounded.
__global__ void __launch_bounds__(256) k_pred_load_col(const uint64_t* __restrict__ counts, float depth, float* __restrict__ G, uint64_t nk, uint64_t ns, uint64_t sample) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < nk; k += (uint64_t)gridDim.x * 256)
        G[k * ns + sample] = (float)counts[k] / depth;
}

// ---- bias_correction, first half (pred.h:217-228): B(s, j) = gt(s, iki[j]) / ikmc[j]; bias(s) = B.rowwise().mean(): the sum
// over the locus' invariant k-mers in their order, per sample, then / n.  One lane per sample: row iki[j] of G is read
// coalesced, the adds of a lane are sequential (the order Eigen's scalar reduction takes).
__global__ void __launch_bounds__(64) k_pred_bias(const float* __restrict__ G, const uint32_t* __restrict__ nk_cum, const uint32_t* __restrict__ nik_cum,
                                                  const uint32_t* __restrict__ iki, const float* __restrict__ ikmc, float* __restrict__ bias, uint64_t ns,
                                                  uint32_t tri0, uint32_t row0) {
    const uint32_t tri = tri0 + blockIdx.x;
    const uint64_t s = (uint64_t)blockIdx.y * 64 + threadIdx.x;
    const LocusSpan L = locus_span(nk_cum, nik_cum, tri);
    if (L.skipped() || s >= ns) return;
    float acc = 0.f;
    for (uint32_t j = L.isi; j < L.iei; ++j) acc += G[(uint64_t)(iki[j] - row0) * ns + s] / ikmc[j];
    bias[(uint64_t)tri * ns + s] = acc / (float)(L.iei - L.isi);
}
// second half (pred.h:229-231): bias /= bias.mean() over the samples.  One block per locus; the mean is a pairwise tree.
__global__ void __launch_bounds__(256) k_pred_bias_norm(const uint32_t* __restrict__ nk_cum, const uint32_t* __restrict__ nik_cum, float* __restrict__ bias, uint64_t ns,
                                                        uint32_t tri0) {
    __shared__ float part[256];
    const uint32_t tri = tri0 + blockIdx.x;
    if (locus_span(nk_cum, nik_cum, tri).skipped()) return;
    float* b = bias + (uint64_t)tri * ns;
    float acc = 0.f;
    for (uint64_t s = threadIdx.x; s < ns; s += 256) acc += b[s];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    const float mean = part[0] / (float)ns;
    for (uint64_t s = threadIdx.x; s < ns; s += 256) b[s] = b[s] / mean;
}
// the correcting pass (pred.h:230): every k-mer column of the locus divided by the locus' bias, sample by sample.  G is
// streamed once, read and written in place: a wave takes PR_ROWS consecutive rows (a row = one k-mer, ns floats) and walks
// the samples 64 at a time, so that PR_ROWS independent loads are in flight per lane; loc[k] = the row's locus (NOLOC: left alone).
constexpr int PR_ROWS = 8;
constexpr uint32_t NOLOC = 0xFFFFFFFFu;
__global__ void __launch_bounds__(256) k_pred_correct(float* __restrict__ G, const uint32_t* __restrict__ loc, const float* __restrict__ bias, uint64_t nk, uint64_t ns) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + w) * PR_ROWS;
    if (r0 >= nk) return;
    uint32_t tri[PR_ROWS];
#pragma unroll
    for (int r = 0; r < PR_ROWS; ++r) tri[r] = r0 + r < nk ? loc[r0 + r] : NOLOC;
    for (uint64_t s = lane; s < ns; s += 64) {
        float g[PR_ROWS], b[PR_ROWS];
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) {
            const bool on = tri[r] != NOLOC;
            g[r] = on ? G[(r0 + r) * ns + s] : 0.f;
            b[r] = on ? bias[(uint64_t)tri[r] * ns + s] : 1.f;
        }
#pragma unroll
        for (int r = 0; r < PR_ROWS; ++r) if (tri[r] != NOLOC) G[(r0 + r) * ns + s] = g[r] / b[r];
    }
}

// ---- a window's fused pass (dbtk_pred.h: dbtk_pred_window_submit).  The window's counts of ALL samples are staged in HBM,
// sample-major: wc[s * rows + r] = count of k-mer row0 + r in sample s.  Two kernels and k_pred_bias_norm between them make the raw
// window, the corrected window and the window's Bias rows without G: 8 bytes read and 8 written per entry, once.
//
// The raw bias sums from the counts: k_pred_bias with G(k, s) replaced by the expression that made it, (float)count / depth — then
// / ikmc[j], the adds sequential in j from 0.f, / (float)n: the same operations on the same values, so the same bits.  One wave per
// locus and 64 samples.  A lane of k_pred_bias reads G along the samples; here the samples are the slow axis, so the wave reads a
// sample's counts along j (lane = invariant k-mer: neighbours in iki are neighbours in the file), turns the terms in LDS, and lane s
// then adds its column in j order.  WB_J invariant k-mers per turn; the running sum stays in the lane's register across turns.
constexpr int WB_J = 64, WB_S = 64;
__global__ void __launch_bounds__(64) k_pred_wbias(const uint64_t* __restrict__ wc, const float* __restrict__ depth, const uint32_t* __restrict__ nk_cum,
                                                   const uint32_t* __restrict__ nik_cum, const uint32_t* __restrict__ iki, const float* __restrict__ ikmc,
                                                   float* __restrict__ bias, uint64_t ns, uint64_t rows, uint32_t tri0, uint32_t row0) {
    __shared__ float terms[WB_J][WB_S + 1];
    const uint32_t lane = threadIdx.x;
    const uint32_t tri = tri0 + blockIdx.x;
    const uint64_t s0 = (uint64_t)blockIdx.y * WB_S;
    const LocusSpan L = locus_span(nk_cum, nik_cum, tri);
    if (L.skipped() || s0 >= ns) return;  // (uniform in the wave)
    const uint32_t isi = L.isi, iei = L.iei;
    const uint32_t nsl = ns - s0 < (uint64_t)WB_S ? (uint32_t)(ns - s0) : (uint32_t)WB_S;
    float acc = 0.f;
    for (uint32_t j0 = isi; j0 < iei; j0 += WB_J) {
        const uint32_t nj = iei - j0 < (uint32_t)WB_J ? iei - j0 : (uint32_t)WB_J;
        if (lane < nj) {
            const uint64_t r = (uint64_t)(iki[j0 + lane] - row0);  // (create_windowed: an invariant k-mer lies inside its locus, so 0 <= r < rows)
            const float kc = ikmc[j0 + lane];
            for (uint32_t i = 0; i < nsl; ++i) terms[lane][i] = ((float)wc[(s0 + i) * rows + r] / depth[s0 + i]) / kc;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < nsl) for (uint32_t j = 0; j < nj; ++j) acc += terms[j][lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < nsl) bias[(uint64_t)tri * ns + s0 + lane] = acc / (float)(iei - isi);
}
// Both matrices of the window from one pass over its counts: k_pred_load's tile, and where that stores G the raw value goes to
// raw[r][s] and raw / Bias(locus of r, s) to cor[r][s] — the division of k_pred_correct on the value k_pred_load would have stored.
// A row of no corrected locus (loc = NOLOC) is copied.  loc = d_loc + row0 (the window's rows), bias the whole [ntr][ns] table after
// k_pred_bias_norm.
__global__ void __launch_bounds__(64) k_pred_wfused(const uint64_t* __restrict__ wc, const float* __restrict__ depth, const uint32_t* __restrict__ loc,
                                                    const float* __restrict__ bias, float* __restrict__ raw, float* __restrict__ cor, uint64_t rows, uint64_t ns) {
    pred_tile(wc, depth, rows, ns, [=](uint64_t r, uint64_t s, float g) {
        const uint32_t tri = loc[r];
        const uint64_t at = r * ns + s;
        raw[at] = g;
        cor[at] = tri != NOLOC ? g / bias[(uint64_t)tri * ns + s] : g;
    });
}

// ---- the dosage tables (dbtk_pred.h, ABI v10): one sample's counts -> its kms and raw-bias entries, locus by locus, in one pass.
// The host cuts the k-mer axis into work items at locus boundaries (dosage_items): an item is a run of whole loci of at most DS_CH
// k-mers together, or one DS_CH-sized part of a locus larger than that.  One block per item:
//   1. the item's counts are read coalesced (8 bytes per lane) into LDS;
//   2. an inclusive prefix sum over them, in uint64: a thread scans DS_E consecutive values, the thread totals are scanned across
//      the wave with shuffles and across the four waves through LDS;
//   3. one lane per locus: sum = P[end - 1] - P[begin - 1].  Exact (integers; the differences are exact modulo 2^64 whatever the
//      running total does), and every lane works whether the item holds one locus of 2000 k-mers or 400 loci of 5;
//      a part of a large locus writes its total to a partial slot instead, and k_dosage_fold adds the parts up;
//   4. the raw bias of the item's loci.  The terms ((float)count[iki[j]] / depth) / ikmc[j] of the item's invariant k-mers — one
//      contiguous range of j, the loci being consecutive — are gathered by all lanes into LDS, DS_TB at a time; then one lane
//      per locus adds its terms from LDS sequentially in j and divides by n: the operations and the add order of k_pred_load_col
//      + k_pred_bias (acc = 0; acc += G / ikmc; acc / n), so the result has the same bits.  Only the adds are ordered.
// LDS: 18 KB of prefix sums (padded by one value per DS_E: the scan's 72-byte lane stride is 2-way conflicted instead of 16-way)
// + 4 KB of terms.  No atomics: a column loaded again is simply overwritten.
// DosItem, DS_T, DS_E, DS_CH and the host's dosage_items: dbtk_pred_plan.h.
using dbtk_pred_plan::DosItem;
using dbtk_pred_plan::DS_T;
using dbtk_pred_plan::DS_E;
using dbtk_pred_plan::DS_CH;
using dbtk_pred_plan::NOPART;
constexpr int DS_TB = 1024;
__device__ __forceinline__ int ds_pad(uint32_t k) { return (int)(k + (k >> 3)); }

__global__ void __launch_bounds__(DS_T) k_dosage_sample(const uint64_t* __restrict__ counts, float depth, const DosItem* __restrict__ items,
                                                        const uint32_t* __restrict__ nk_cum, const uint32_t* __restrict__ nik_cum,
                                                        const uint32_t* __restrict__ iki, const float* __restrict__ ikmc, uint64_t* __restrict__ kms,
                                                        float* __restrict__ raw, uint64_t* __restrict__ part, uint64_t ns, uint64_t sample) {
    __shared__ uint64_t P[DS_CH + DS_CH / DS_E];
    __shared__ uint64_t wtot[DS_T / 64];
    __shared__ float terms[DS_TB];
    const DosItem it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (it.nkm) {
#pragma unroll
        for (int i = 0; i < DS_E; ++i) {
            const uint32_t k = (uint32_t)i * DS_T + tid;
            P[ds_pad(k)] = k < it.nkm ? counts[(uint64_t)it.k0 + k] : 0ull;
        }
        __syncthreads();
        uint64_t v[DS_E], acc = 0;
#pragma unroll
        for (int i = 0; i < DS_E; ++i) { acc += P[ds_pad(tid * DS_E + i)]; v[i] = acc; }
        uint64_t sc = acc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t t = __shfl_up(sc, d);
            if ((int)lane >= d) sc += t;
        }
        if (lane == 63u) wtot[w] = sc;
        __syncthreads();
        uint64_t off = sc - acc;
#pragma unroll
        for (uint32_t q = 0; q < DS_T / 64 - 1; ++q) if (q < w) off += wtot[q];
#pragma unroll
        for (int i = 0; i < DS_E; ++i) P[ds_pad(tid * DS_E + i)] = off + v[i];
        __syncthreads();
    }
    for (uint32_t j = tid; j < it.nl; j += DS_T) {
        const uint32_t l = it.l0 + j;
        const LocusSpan L = locus_span(nk_cum, nik_cum, l);
        const uint32_t b = L.si - it.k0, e = L.ei - it.k0;
        kms[(uint64_t)l * ns + sample] = (e ? P[ds_pad(e - 1)] : 0ull) - (b ? P[ds_pad(b - 1)] : 0ull);
    }
    if (it.part != NOPART && tid == 0) part[it.part] = it.nkm ? P[ds_pad(it.nkm - 1)] : 0ull;
    for (uint32_t lg = 0; lg < it.nlb; lg += DS_T) {  // (every bound of the loops with barriers is the same in all threads)
        const uint32_t gl0 = it.l0 + lg, gn = it.nlb - lg < (uint32_t)DS_T ? it.nlb - lg : (uint32_t)DS_T;
        const uint32_t J0 = gl0 ? nik_cum[gl0 - 1] : 0u, J1 = nik_cum[gl0 + gn - 1];
        const bool on = tid < gn;
        const uint32_t l = gl0 + (on ? tid : 0u);
        const LocusSpan L = locus_span(nk_cum, nik_cum, l);
        const uint32_t isi = L.isi, iei = on ? L.iei : isi;
        const bool empty = L.si == L.ei;
        float acc = 0.f;
        for (uint32_t jt = J0; jt < J1; jt += DS_TB) {
            const uint32_t nt = J1 - jt < (uint32_t)DS_TB ? J1 - jt : (uint32_t)DS_TB;
            __syncthreads();
            for (uint32_t jj = tid; jj < nt; jj += DS_T) terms[jj] = ((float)counts[iki[jt + jj]] / depth) / ikmc[jt + jj];
            __syncthreads();
            const uint32_t lo = isi > jt ? isi : jt, hi = iei < jt + nt ? iei : jt + nt;
            for (uint32_t j = lo; j < hi; ++j) acc += terms[j - jt];
        }
        if (on && iei > isi && !empty) raw[(uint64_t)l * ns + sample] = acc / (float)(iei - isi);
    }
}
// the loci larger than DS_CH k-mers: their parts' totals (part[fbeg[q]] .. part[fbeg[q + 1] - 1]) added up, one lane per locus
__global__ void __launch_bounds__(64) k_dosage_fold(const uint32_t* __restrict__ floc, const uint32_t* __restrict__ fbeg, const uint64_t* __restrict__ part,
                                                    uint64_t* __restrict__ kms, uint64_t ns, uint64_t sample, uint32_t nfold) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nfold) return;
    uint64_t acc = 0;
    for (uint32_t i = fbeg[q]; i < fbeg[q + 1]; ++i) acc += part[i];
    kms[(uint64_t)floc[q] * ns + sample] = acc;
}
// values (dbtk_pred.h): v = (float)kms / depth; / Bias where the locus has k-mers and invariant k-mers; 0 without k-mers
__global__ void __launch_bounds__(256) k_dosage_values(const uint64_t* __restrict__ kms, const float* __restrict__ bias, const float* __restrict__ depth,
                                                       const uint32_t* __restrict__ nk_cum, const uint32_t* __restrict__ nik_cum, float* __restrict__ out, uint64_t ns) {
    const uint32_t tri = blockIdx.x;
    const uint64_t s = (uint64_t)blockIdx.y * 256 + threadIdx.x;
    if (s >= ns) return;
    const LocusSpan L = locus_span(nk_cum, nik_cum, tri);
    const uint64_t at = (uint64_t)tri * ns + s;
    const float v = (float)kms[at] / depth[s];
    out[at] = L.si == L.ei ? 0.f : (L.isi == L.iei ? v : v / bias[at]);
}

// what both handles ask of their metadata arguments and of the device, before anything is allocated; leaves the device current
static dbtk_status_t check_ikmer_meta(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                                      uint64_t nik, const uint32_t* iki, const uint8_t* ikmc) {
    if (!nk_cum || !nik_cum || (nik && (!iki || !ikmc))) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!ns || !nk || !ntr) { set_error("empty cohort / RPGG"); return DBTK_ERR_ARG; }
    if (nk > 0xFFFFFFFFull || ntr > 0xFFFFFFFFull) { set_error("ikmer.meta holds 32-bit k-mer indices"); return DBTK_ERR_ARG; }
    for (uint64_t t = 0; t < ntr; ++t) {
        const LocusSpan L = locus_span(nk_cum, nik_cum, t);
        if (L.ei < L.si || L.ei > nk || L.iei < L.isi || L.iei > nik) { set_error("ikmer.meta: the cumulative counts must not decrease or pass the totals"); return DBTK_ERR_FORMAT; }
    }
    for (uint64_t j = 0; j < nik; ++j) if (iki[j] >= nk) { set_error("ikmer.meta: invariant k-mer index out of range"); return DBTK_ERR_FORMAT; }
    int ndev = 0;
    if (const dbtk_status_t nd = device_count(&ndev)) return nd;
    if (device_id < 0 || device_id >= ndev) { set_error("device_id out of range"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(device_id));
    return DBTK_OK;
}
// `ikmer.meta` (dbtk_pred.h: dbtk_pred_create_from_file) into host vectors
struct IkmerMeta { uint64_t nk = 0, nik = 0, ntr = 0; std::vector<uint32_t> nkc, nikc, iki; std::vector<uint8_t> kc; };
static dbtk_status_t read_ikmer_meta(const char* ikmer_meta, IkmerMeta* m) {
    FILE* f = fopen(ikmer_meta, "rb");
    if (!f) { set_error(std::string("cannot open ") + ikmer_meta); return DBTK_ERR_IO; }
    uint64_t hdr[3];
    dbtk_status_t st = DBTK_OK;
    if (fread(hdr, 8, 3, f) != 3) { set_error(std::string("truncated ") + ikmer_meta); st = DBTK_ERR_IO; }
    if (!st && (hdr[0] > 0xFFFFFFFFull || hdr[1] > hdr[0] || hdr[2] > 0xFFFFFFFFull)) { set_error(std::string(ikmer_meta) + ": implausible header"); st = DBTK_ERR_FORMAT; }
    if (!st) {
        const uint64_t nik = hdr[1], ntr = hdr[2];
        m->nk = hdr[0]; m->nik = nik; m->ntr = ntr;
        m->nkc.resize(ntr); m->nikc.resize(ntr); m->iki.resize(nik); m->kc.resize(nik);
        std::vector<uint8_t> rec(nik * 5);
        if (fread(m->nkc.data(), 4, ntr, f) != ntr || fread(m->nikc.data(), 4, ntr, f) != ntr || (nik && fread(rec.data(), 5, nik, f) != nik)) {
            set_error(std::string("truncated ") + ikmer_meta); st = DBTK_ERR_IO;
        }
        for (uint64_t j = 0; j < nik && !st; ++j) { memcpy(&m->iki[j], &rec[5 * j], 4); m->kc[j] = rec[5 * j + 4]; }
    }
    fclose(f);
    return st;
}

// ---- what the two handles share
// the steps of a handle's creation.  Once one has failed the rest are skipped (STEP), so st and dbtk_last_error() keep the first
// failure; what was allocated is remembered, and the handle's free releases it however far the creation came.
struct Setup {
    dbtk_status_t st = DBTK_OK;
    std::vector<void*> dev, pinned;  // of hipMalloc / hipHostMalloc
    Setup() { dev.reserve(16); pinned.reserve(8); }  // (more than either handle allocates: taking one in never throws)
    // oom: what does not fit, for DBTK_ERR_NOMEM and the state of the HBM instead of the plain error when the device is out of memory
    bool ok(hipError_t e, const char* what, const std::string* oom = nullptr) {
        if (e == hipSuccess) return true;
        if (e == hipErrorOutOfMemory && oom) {
            (void)hipGetLastError();
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            set_error(*oom + " do not fit, " + std::to_string(fr) + " of " + std::to_string(tot) + " bytes of HBM are free");
            st = DBTK_ERR_NOMEM;
        } else { set_error(std::string(what) + ": " + hipGetErrorString(e)); st = DBTK_ERR_HIP; }
        return false;
    }
    template <class T> void device(T** p, uint64_t bytes, const char* what = "hipMalloc", const std::string* oom = nullptr) {
        if (!st && ok(hipMalloc(p, bytes), what, oom)) dev.push_back(*p);
    }
    template <class T> void host(T** p, uint64_t bytes, const char* what, const std::string* oom) {
        if (!st && ok(hipHostMalloc(p, bytes), what, oom)) pinned.push_back(*p);
    }
    void upload(void* dst, const void* src, uint64_t bytes, hipStream_t s) {
        if (!st && bytes) ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), "hipMemcpy");
    }
    void release() { for (void* q : dev) (void)hipFree(q); for (void* q : pinned) (void)hipHostFree(q); }
};
#define STEP(m, call, ...) do { if (!(m).st) (m).ok((call), __VA_ARGS__); } while (0)

// ikmer.meta's four arrays in HBM, as the kernels read them (iki and ikmc padded by one entry: never empty)
struct IkmerDev {
    uint32_t *nk = nullptr, *nik = nullptr, *iki = nullptr;
    float* ikmc = nullptr;  // the expected counts as floats: what the bias sums divide by
};
static void ikmer_upload(Setup& m, IkmerDev* d, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum, uint64_t nik, const uint32_t* iki,
                         const uint8_t* ikmc, hipStream_t s, const char* what = "hipMalloc", const std::string* oom = nullptr) {
    std::vector<float> kc(nik);
    for (uint64_t j = 0; j < nik; ++j) kc[j] = (float)ikmc[j];
    m.device(&d->nk, ntr * 4, what, oom);
    m.device(&d->nik, ntr * 4, what, oom);
    m.device(&d->iki, (nik + 1) * 4, what, oom);
    m.device(&d->ikmc, (nik + 1) * 4, what, oom);
    m.upload(d->nk, nk_cum, ntr * 4, s);
    m.upload(d->nik, nik_cum, ntr * 4, s);
    m.upload(d->iki, iki, nik * 4, s);
    m.upload(d->ikmc, kc.data(), nik * 4, s);
    STEP(m, hipStreamSynchronize(s), "hipStreamSynchronize");  // (kc ends here)
}

static dbtk_status_t check_sample_range(uint64_t first, uint64_t n, uint64_t ns) {
    if (first > ns || n > ns - first || n > 0xFFFFFFFFull) { set_error("sample range outside the cohort"); return DBTK_ERR_ARG; }
    return DBTK_OK;
}
static dbtk_status_t check_device_counts(const void* d_counts, int device, const char* who) {
    if (is_device_memory_of(d_counts, device)) return DBTK_OK;
    set_error(std::string(who) + ": d_counts is not device memory of the handle's device");
    return DBTK_ERR_ARG;
}
// a context's accumulated counts as one sample's count vector in HBM (*base): the context is of the handle's RPGG build (nk k-mers)
// and device, has nothing unflushed, every batch of it is done, its counter replicas are folded, and a pending sticky error word is
// reported instead of tainted counts.  whose[0]: who holds the nk ("ikmer.meta has"), whose[1]: what lives on the device ("the matrix").
static dbtk_status_t ctx_counts_ready(dbtk_ctx_t* ctx, int device, uint64_t nk, const char* const whose[2], const uint64_t** base) {
    CtxFacts f;
    { const dbtk_status_t st = ctx_facts(ctx, &f); if (st) return st; }  // (fails on a null context alone: refused by the callers)
    if (f.ntrkmers != nk) { set_error("the context counts " + std::to_string(f.ntrkmers) + " TR k-mers, " + whose[0] + " " + std::to_string(nk) + ": not the same RPGG build"); return DBTK_ERR_ARG; }
    if (f.device != device) { set_error("the context is on device " + std::to_string(f.device) + ", " + whose[1] + " on device " + std::to_string(device)); return DBTK_ERR_ARG; }
    if (f.unflushed_pairs) { set_error(std::to_string(f.unflushed_pairs) + " pairs appended by dbtk_ingest_align_merged are not aligned yet: flush them first (slot = ~0u, flush = 1)"); return DBTK_ERR_ARG; }
    { const dbtk_status_t st = dbtk_ctx_synchronize(ctx); if (st) return st; }
    void* b = nullptr; uint64_t n64 = 0;
    { const dbtk_status_t st = dbtk_ctx_accum_buffer(ctx, &b, &n64); if (st) return st; }
    if (!b || n64 < nk) { set_error("the context has no accumulators"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(device));
    *base = (const uint64_t*)b;
    return DBTK_OK;
}
// one launch of a tile kernel (pred_tile) over rows x n: a block per PT_K k-mers, at most 64 blocks striding the samples
template <class... P, class... A>
static dbtk_status_t launch_tile(void (*kernel)(P...), hipStream_t s, uint64_t rows, uint64_t n, A... args) {
    const uint64_t kt = (rows + PT_K - 1) / PT_K;
    if (kt > 0x7FFFFFFFull) { set_error("too many k-mers for one launch"); return DBTK_ERR_ARG; }
    const uint32_t gy = (uint32_t)std::min<uint64_t>((n + PT_S - 1) / PT_S, 64);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)kt, gy), dim3(64), 0, s, args...);
    DEVCHK(hipGetLastError());
    return DBTK_OK;
}

struct dbtk_pred {
    int device = 0;
    uint64_t ns = 0, nk = 0, ntr = 0, nik = 0;
    float* d_G = nullptr;
    float* d_bias = nullptr;
    IkmerDev meta;
    uint32_t* d_loc = nullptr;  // d_loc[k]: locus of k-mer k, NOLOC where bias_correction skips it
    Setup mem;                  // the creation's allocations (dbtk_pred_free releases them; the owners below go when the handle does,
                                // last to first: the loads' buffers, the events, the streams)
    DevStream stream2;          // ws[1] (ws[0] = stream): a window's copies and kernels run on its buffer's stream
    DevStream stream;
    DevEvent ev[4];
    DevArr<float> d_depth2;     // the depths of dbtk_pred_load_device, regrown by it
    DevArr<float> d_depth;      // staging of dbtk_pred_load_samples, regrown by it: n depths
    DevArr<uint64_t> d_counts;  //   ... and n * nk counts
    float ms[3] = {0, 0, 0};
    // the rows of d_G, the current window: loci [w_first, w_end), k-mers [w_row0, w_row0 + w_rows); on its stream ws(cur).  A handle of
    // dbtk_pred_create has one window for good: everything, on `stream`
    uint64_t w_first = 0, w_end = 0, w_row0 = 0, w_rows = 0;
    int cur = 0;                                     // a windowed handle's buffer of the window: d_wc[cur]
    // ---- a windowed handle (dbtk_pred_create_windowed): d_G holds max_rows x ns floats
    bool windowed = false;
    uint64_t max_rows = 0;
    std::vector<uint32_t> nkc;                       // host copy of nk_cum: the window planning
    uint64_t* d_wc[2] = {nullptr, nullptr};          // the window's staged counts, [ns][w_rows] u64 (sample-major like the files)
    float* d_wdepth[2] = {nullptr, nullptr};         // [ns]
    float* h_depth[2] = {nullptr, nullptr};          // pinned [ns]: 1 until the sample is loaded into the window
    float *d_raw = nullptr, *d_cor = nullptr;        // what the fused pass writes, [w_rows][ns] each (one set: one window's outputs are in flight at a time)
    uint64_t* h_stage = nullptr;                     // pinned, PW_STAGE x max_rows counts: what dbtk_pred_load_samples sends from
    float *h_raw = nullptr, *h_cor = nullptr;        // pinned, max_rows x ns: where the fused pass' outputs land
    std::vector<uint8_t> dirty;                      // [ns]: staged into the window since d_G was last made from the staged counts
    int pending = -1;                                // the buffer whose fused pass was submitted and not collected yet
    uint64_t pend_rows = 0;
    hipStream_t ws(int slot) const { return slot ? stream2 : stream; }
};
constexpr uint64_t PW_STAGE = 4;  // samples per transfer of dbtk_pred_load_samples on a windowed handle (host memory is what windows are for)

// the window that starts at locus `first` becomes the current one, on the buffer that holds no submitted window; its staged counts,
// its depths and its part of G are zeroed.  Returns with the buffer's stream idle.
static dbtk_status_t pred_open_window(dbtk_pred* p, uint64_t first) {
    uint64_t end = 0, row0 = 0, rows = 0;
    if (first >= p->ntr) { set_error("dbtk_pred_window: first_locus " + std::to_string(first) + " >= ntr " + std::to_string(p->ntr)); return DBTK_ERR_ARG; }
    if (!dbtk_pred_plan::window(p->nkc.data(), p->ntr, p->nk, p->max_rows, first, &end, &row0, &rows)) { set_error("dbtk_pred_window: locus does not fit"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(p->device));
    const int slot = p->pending == (p->cur ^ 1) ? p->cur : p->cur ^ 1;
    hipStream_t s = p->ws(slot);
    if (rows) {
        DEVCHK(hipMemsetAsync(p->d_wc[slot], 0, p->ns * rows * 8, s));
        DEVCHK(hipMemsetAsync(p->d_G, 0, p->ns * rows * sizeof(float), s));
    }
    for (uint64_t i = 0; i < p->ns; ++i) p->h_depth[slot][i] = 1.f;
    std::fill(p->dirty.begin(), p->dirty.end(), (uint8_t)0);
    DEVCHK(hipStreamSynchronize(s));
    p->cur = slot; p->w_first = first; p->w_end = end; p->w_row0 = row0; p->w_rows = rows;
    return DBTK_OK;
}
// a windowed handle's d_G is made from the staged counts when somebody asks for it (dbtk_pred_matrix, dbtk_pred_correct): the columns
// staged since the last time, run by run, through the whole-matrix handle's tile kernel.  Asynchronous on the window's stream.
static dbtk_status_t pred_window_materialize(dbtk_pred* p) {
    hipStream_t s = p->ws(p->cur);
    const uint64_t rows = p->w_rows, ns = p->ns;
    bool sent = false;
    for (uint64_t a = 0; a < ns;) {
        if (!p->dirty[a]) { ++a; continue; }
        uint64_t b = a;
        while (b < ns && p->dirty[b]) p->dirty[b++] = 0;
        if (rows) {
            if (!sent) { DEVCHK(hipMemcpyAsync(p->d_wdepth[p->cur], p->h_depth[p->cur], ns * 4, hipMemcpyHostToDevice, s)); sent = true; }
            const dbtk_status_t st = launch_tile(k_pred_load, s, rows, b - a, p->d_wc[p->cur] + a * rows, p->d_wdepth[p->cur] + a, p->d_G, rows, ns, a, (uint32_t)(b - a));
            if (st) return st;
        }
        a = b;
    }
    if (sent) DEVCHK(hipStreamSynchronize(s));  // (h_depth may change with the next load)
    return DBTK_OK;
}
// host counts into the current window: counts[i * rows + r].  Sent PW_STAGE samples at a time from the pinned staging buffer; a caller
// that filled that buffer itself (dbtk_pred_window_stage) skips the copy into it.
static dbtk_status_t pred_window_load_host(dbtk_pred* p, uint64_t first, uint64_t n, const uint64_t* counts, const float* read_depth) {
    hipStream_t s = p->ws(p->cur);
    const uint64_t rows = p->w_rows;
    for (uint64_t i0 = 0; i0 < n && rows; i0 += PW_STAGE) {
        const uint64_t ni = std::min<uint64_t>(PW_STAGE, n - i0);
        const uint64_t* src = counts + i0 * rows;
        if (src != p->h_stage) memcpy(p->h_stage, src, ni * rows * 8);
        DEVCHK(hipMemcpyAsync(p->d_wc[p->cur] + (first + i0) * rows, p->h_stage, ni * rows * 8, hipMemcpyHostToDevice, s));
        DEVCHK(hipStreamSynchronize(s));  // (the staging buffer is free again)
    }
    for (uint64_t i = 0; i < n; ++i) { p->h_depth[p->cur][first + i] = read_depth[i]; p->dirty[first + i] = 1; }
    return DBTK_OK;
}

extern "C" {

static dbtk_status_t dbtk_pred_create_impl(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                               uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, bool windowed, uint64_t max_rows, dbtk_pred_t** out) {
    if (!out) { set_error("null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    { const dbtk_status_t cs = check_ikmer_meta(device_id, ns, nk, ntr, nk_cum, nik_cum, nik, iki, ikmc); if (cs) return cs; }
    if (windowed) {
        if (!max_rows) { set_error("max_rows must be positive"); return DBTK_ERR_ARG; }
        if (max_rows > nk) max_rows = nk;
        uint64_t size = 0;
        const uint64_t big = dbtk_pred_plan::first_oversized(nk_cum, ntr, nk, max_rows, &size);
        if (big < ntr) {
            set_error("locus " + std::to_string(big) + " has " + std::to_string(size) + " k-mers, a window holds max_rows = " + std::to_string(max_rows));
            return DBTK_ERR_ARG;
        }
        // a window holds whole loci and nothing else: the bias of a locus may read that locus' columns only (as every ikmer.meta has it)
        for (uint64_t t = 0; t < ntr; ++t) {
            const LocusSpan L = locus_span(nk_cum, nik_cum, t);
            for (uint32_t j = L.isi; j < L.iei; ++j)
                if (iki[j] < L.si || iki[j] >= L.ei) { set_error("ikmer.meta: invariant k-mer " + std::to_string(j) + " lies outside its locus " + std::to_string(t) + ": no windows over this build"); return DBTK_ERR_FORMAT; }
        }
    }
    const uint64_t grows = windowed ? max_rows : nk;  // rows of d_G
    std::vector<uint32_t> loc(nk, NOLOC);  // (k-mers past the last locus' cumulative count belong to no locus, like in the reference's loop)
    for (uint64_t t = 0; t < ntr; ++t) {
        const LocusSpan L = locus_span(nk_cum, nik_cum, t);
        if (!L.skipped()) std::fill(loc.begin() + L.si, loc.begin() + L.ei, (uint32_t)t);
    }
    std::unique_ptr<dbtk_pred, void (*)(dbtk_pred*)> hold(new dbtk_pred, dbtk_pred_free);  // (freed, should a vector or a string below throw)
    dbtk_pred* p = hold.get();
    p->device = device_id; p->ns = ns; p->nk = nk; p->ntr = ntr; p->nik = nik;
    p->windowed = windowed; p->w_end = ntr; p->w_rows = nk;  // (a windowed handle opens its first window below)
    if (windowed) { p->max_rows = max_rows; p->nkc.assign(nk_cum, nk_cum + ntr); p->dirty.assign(ns, 0); }
    Setup& m = p->mem;
    STEP(m, p->stream.create(hipStreamDefault), "hipStreamCreate");
    for (DevEvent& e : p->ev) STEP(m, e.create(hipEventDefault), "hipEventCreate");
    // the one allocation of a whole-matrix handle that competes with an aligner's tables for the HBM
    const std::string gfit = std::string("genotype matrix: 4 * ") + (windowed ? "max_rows" : "nk") + " * ns = " + std::to_string(grows * ns * sizeof(float)) + " bytes";
    m.device(&p->d_G, grows * ns * sizeof(float), "hipMalloc (genotype matrix)", &gfit);
    if (windowed) {  // the window buffers, device and pinned host, sized once: 24 * max_rows * ns bytes of HBM beside the matrix' 4
        const std::string win = " of a window of max_rows = " + std::to_string(max_rows) + " x ns = " + std::to_string(ns);
        auto dev = [&](auto** q, uint64_t bytes, const char* what) { const std::string fit = what + win; m.device(q, bytes, what, &fit); };
        auto pin = [&](auto** q, uint64_t bytes, const char* what) { const std::string fit = what + win; m.host(q, bytes, what, &fit); };
        const std::string sfit = "hipStreamCreate" + win;
        const uint64_t cells = max_rows * ns;
        STEP(m, p->stream2.create(hipStreamDefault), "hipStreamCreate", &sfit);
        for (int i = 0; i < 2; ++i) {
            dev(&p->d_wc[i], cells * 8, "hipMalloc (staged counts)");
            dev(&p->d_wdepth[i], ns * 4, "hipMalloc (depths)");
            pin(&p->h_depth[i], ns * 4, "hipHostMalloc (depths)");
            for (uint64_t s = 0; s < ns && !m.st; ++s) p->h_depth[i][s] = 1.f;
        }
        dev(&p->d_raw, cells * 4, "hipMalloc (raw window)");
        dev(&p->d_cor, cells * 4, "hipMalloc (corrected window)");
        pin(&p->h_stage, PW_STAGE * max_rows * 8, "hipHostMalloc (count staging)");
        pin(&p->h_raw, cells * 4, "hipHostMalloc (raw window)");
        pin(&p->h_cor, cells * 4, "hipHostMalloc (corrected window)");
    }
    m.device(&p->d_bias, ntr * ns * sizeof(float), "hipMalloc (bias matrix)");
    ikmer_upload(m, &p->meta, ntr, nk_cum, nik_cum, nik, iki, ikmc, p->stream);
    m.device(&p->d_loc, nk * 4);
    m.upload(p->d_loc, loc.data(), nk * 4, p->stream);
    STEP(m, hipMemsetAsync(p->d_G, 0, grows * ns * sizeof(float), p->stream), "hipMemset");
    STEP(m, hipMemsetAsync(p->d_bias, 0, ntr * ns * sizeof(float), p->stream), "hipMemset");
    STEP(m, hipStreamSynchronize(p->stream), "hipStreamSynchronize");
    if (!m.st && windowed) m.st = pred_open_window(p, 0);  // a windowed handle always has a current window
    if (m.st) return m.st;
    *out = hold.release();
    return DBTK_OK;
}

void dbtk_pred_free(dbtk_pred_t* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->stream2) (void)hipStreamSynchronize(p->stream2);  // (a submitted window that nobody collected)
    p->mem.release();
    delete p;
}

static dbtk_status_t dbtk_pred_create_from_file_impl(int device_id, uint64_t ns, const char* ikmer_meta, bool windowed, uint64_t max_rows, dbtk_pred_t** out) {
    if (!ikmer_meta || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    IkmerMeta m;
    { const dbtk_status_t st = read_ikmer_meta(ikmer_meta, &m); if (st) return st; }
    return dbtk_pred_create_impl(device_id, ns, m.nk, m.ntr, m.nkc.data(), m.nikc.data(), m.nik, m.iki.data(), m.kc.data(), windowed, max_rows, out);
}

uint64_t dbtk_pred_nk(const dbtk_pred_t* p) { return p ? p->nk : 0; }
uint64_t dbtk_pred_ntr(const dbtk_pred_t* p) { return p ? p->ntr : 0; }

static dbtk_status_t dbtk_pred_load_samples_impl(dbtk_pred_t* p, uint64_t first_sample, uint64_t n, const uint64_t* counts, const float* read_depth) {
    if (!p || !counts || !read_depth) { set_error("null argument"); return DBTK_ERR_ARG; }
    { const dbtk_status_t st = check_sample_range(first_sample, n, p->ns); if (st) return st; }
    if (!n) return DBTK_OK;
    DEVCHK(hipSetDevice(p->device));
    if (p->windowed) return pred_window_load_host(p, first_sample, n, counts, read_depth);
    DEVCHK(p->d_counts.reserve(n * p->nk, n * p->nk));
    DEVCHK(p->d_depth.reserve(n, n));
    DEVCHK(hipMemcpyAsync(p->d_counts, counts, n * p->nk * 8, hipMemcpyHostToDevice, p->stream));
    DEVCHK(hipMemcpyAsync(p->d_depth, read_depth, n * 4, hipMemcpyHostToDevice, p->stream));
    { const dbtk_status_t st = launch_tile(k_pred_load, p->stream, p->nk, n, p->d_counts.get(), p->d_depth.get(), p->d_G, p->nk, p->ns, first_sample, (uint32_t)n); if (st) return st; }
    DEVCHK(hipStreamSynchronize(p->stream));  // (the caller's buffers are free again)
    return DBTK_OK;
}

// counts of n samples in device memory -> their columns; asynchronous on p->stream.  One sample: the column kernel; more: the tile
// kernel (the depths travel through p->d_depth2, a buffer of its own: p->d_depth belongs to dbtk_pred_load_samples' staging and is
// sized with it).
static dbtk_status_t pred_load_device_async(dbtk_pred_t* p, uint64_t first_sample, uint64_t n, const uint64_t* d_counts, const float* read_depth) {
    if (n == 1) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>((p->nk + 255) / 256, 1u << 16);
        hipLaunchKernelGGL(k_pred_load_col, dim3(nb), dim3(256), 0, p->stream, d_counts, read_depth[0], p->d_G, p->nk, p->ns, first_sample);
        DEVCHK(hipGetLastError());
        return DBTK_OK;
    }
    DEVCHK(p->d_depth2.reserve(n, n));
    DEVCHK(hipMemcpyAsync(p->d_depth2, read_depth, n * 4, hipMemcpyHostToDevice, p->stream));
    return launch_tile(k_pred_load, p->stream, p->nk, n, d_counts, p->d_depth2.get(), p->d_G, p->nk, p->ns, first_sample, (uint32_t)n);
}

dbtk_status_t dbtk_pred_load_device(dbtk_pred_t* p, uint64_t first_sample, uint64_t n, const uint64_t* d_counts, const float* read_depth) {
    if (!p || !d_counts || !read_depth) { set_error("null argument"); return DBTK_ERR_ARG; }
    { const dbtk_status_t st = check_sample_range(first_sample, n, p->ns); if (st) return st; }
    if (!n) return DBTK_OK;
    DEVCHK(hipSetDevice(p->device));
    { const dbtk_status_t st = check_device_counts(d_counts, p->device, "dbtk_pred_load_device"); if (st) return st; }
    if (p->windowed) {  // the window's counts are staged (the fused pass reads all samples at once): one copy inside HBM
        hipStream_t s = p->ws(p->cur);
        if (p->w_rows) DEVCHK(hipMemcpyAsync(p->d_wc[p->cur] + first_sample * p->w_rows, d_counts, n * p->w_rows * 8, hipMemcpyDeviceToDevice, s));
        DEVCHK(hipStreamSynchronize(s));  // (d_counts is no longer being read)
        for (uint64_t i = 0; i < n; ++i) { p->h_depth[p->cur][first_sample + i] = read_depth[i]; p->dirty[first_sample + i] = 1; }
        return DBTK_OK;
    }
    const dbtk_status_t st = pred_load_device_async(p, first_sample, n, d_counts, read_depth);
    if (st) return st;
    DEVCHK(hipStreamSynchronize(p->stream));  // (d_counts is no longer being read)
    return DBTK_OK;
}

dbtk_status_t dbtk_pred_load_ctx(dbtk_pred_t* p, uint64_t sample, dbtk_ctx_t* ctx, float read_depth) {
    if (!p || !ctx) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (p->windowed) { set_error("dbtk_pred_load_ctx: a context holds one sample's whole count vector, a windowed handle takes a window's counts of every sample: use dbtk_pred_load_device"); return DBTK_ERR_ARG; }
    if (sample >= p->ns) { set_error("sample outside the cohort"); return DBTK_ERR_ARG; }
    static const char* const whose[2] = {"ikmer.meta has", "the matrix"};
    const uint64_t* base = nullptr;
    { const dbtk_status_t st = ctx_counts_ready(ctx, p->device, p->nk, whose, &base); if (st) return st; }
    const dbtk_status_t st = pred_load_device_async(p, sample, 1, base, &read_depth);
    if (st) return st;
    DEVCHK(hipStreamSynchronize(p->stream));  // (d_accum is no longer being read: dbtk_ctx_reset may follow)
    return DBTK_OK;
}

dbtk_status_t dbtk_pred_correct(dbtk_pred_t* p) {
    if (!p) { set_error("null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(p->device));
    // the loci and rows at work: the current window's (everything on a whole-matrix handle); its Bias rows alone are made again
    const uint64_t t0 = p->w_first, nl = p->w_end - p->w_first, row0 = p->w_row0, rows = p->w_rows;
    hipStream_t s = p->ws(p->cur);
    if (p->windowed) { const dbtk_status_t st = pred_window_materialize(p); if (st) return st; }
    DEVCHK(hipMemsetAsync(p->d_bias + t0 * p->ns, 0, nl * p->ns * sizeof(float), s));
    DEVCHK(hipEventRecord(p->ev[0], s));
    hipLaunchKernelGGL(k_pred_bias, dim3((uint32_t)nl, (uint32_t)((p->ns + 63) / 64)), dim3(64), 0, s, p->d_G, p->meta.nk, p->meta.nik, p->meta.iki, p->meta.ikmc, p->d_bias, p->ns,
                       (uint32_t)t0, (uint32_t)row0);
    DEVCHK(hipGetLastError());
    DEVCHK(hipEventRecord(p->ev[1], s));
    hipLaunchKernelGGL(k_pred_bias_norm, dim3((uint32_t)nl), dim3(256), 0, s, p->meta.nk, p->meta.nik, p->d_bias, p->ns, (uint32_t)t0);
    DEVCHK(hipGetLastError());
    DEVCHK(hipEventRecord(p->ev[2], s));
    if (rows) {
        const uint64_t nb = (rows + 4 * PR_ROWS - 1) / (4 * PR_ROWS);
        hipLaunchKernelGGL(k_pred_correct, dim3((uint32_t)nb), dim3(256), 0, s, p->d_G, p->d_loc + row0, p->d_bias, rows, p->ns);
        DEVCHK(hipGetLastError());
    }
    DEVCHK(hipEventRecord(p->ev[3], s));
    DEVCHK(hipStreamSynchronize(s));
    for (int i = 0; i < 3; ++i) DEVCHK(hipEventElapsedTime(&p->ms[i], p->ev[i], p->ev[i + 1]));
    return DBTK_OK;
}

dbtk_status_t dbtk_pred_matrix(dbtk_pred_t* p, float* out) {
    if (!p || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(p->device));
    if (p->windowed) {
        { const dbtk_status_t st = pred_window_materialize(p); if (st) return st; }
        DEVCHK(hipStreamSynchronize(p->ws(p->cur)));
    }
    if (p->w_rows) DEVCHK(hipMemcpy(out, p->d_G, p->w_rows * p->ns * sizeof(float), hipMemcpyDeviceToHost));
    return DBTK_OK;
}

// ---- the calls of a windowed handle alone
static dbtk_status_t need_windowed(const dbtk_pred_t* p, const char* who) {
    if (!p) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!p->windowed) { set_error(std::string(who) + ": not a windowed handle (dbtk_pred_create_windowed)"); return DBTK_ERR_ARG; }
    return DBTK_OK;
}
dbtk_status_t dbtk_pred_window(dbtk_pred_t* p, uint64_t first_locus, uint64_t* end_locus, uint64_t* first_row, uint64_t* rows) {
    { const dbtk_status_t st = need_windowed(p, "dbtk_pred_window"); if (st) return st; }
    { const dbtk_status_t st = pred_open_window(p, first_locus); if (st) return st; }
    if (end_locus) *end_locus = p->w_end;
    if (first_row) *first_row = p->w_row0;
    if (rows) *rows = p->w_rows;
    return DBTK_OK;
}
uint64_t dbtk_pred_max_rows(const dbtk_pred_t* p) { return p && p->windowed ? p->max_rows : 0; }
dbtk_status_t dbtk_pred_window_stage(dbtk_pred_t* p, uint64_t** buf, uint64_t* cap_samples) {
    { const dbtk_status_t st = need_windowed(p, "dbtk_pred_window_stage"); if (st) return st; }
    if (!buf || !cap_samples) { set_error("null argument"); return DBTK_ERR_ARG; }
    *buf = p->h_stage; *cap_samples = PW_STAGE;
    return DBTK_OK;
}
dbtk_status_t dbtk_pred_window_submit(dbtk_pred_t* p) {
    { const dbtk_status_t st = need_windowed(p, "dbtk_pred_window_submit"); if (st) return st; }
    if (p->pending >= 0) { set_error("dbtk_pred_window_submit: the outputs of the window submitted before have not been taken (dbtk_pred_window_outputs)"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(p->device));
    const int c = p->cur;
    hipStream_t s = p->ws(c);
    const uint64_t ns = p->ns, rows = p->w_rows, nl = p->w_end - p->w_first;
    DEVCHK(hipMemcpyAsync(p->d_wdepth[c], p->h_depth[c], ns * 4, hipMemcpyHostToDevice, s));
    DEVCHK(hipMemsetAsync(p->d_bias + p->w_first * ns, 0, nl * ns * sizeof(float), s));
    if (rows) {
        if (nl > 0x7FFFFFFFull) { set_error("window too large for one launch"); return DBTK_ERR_ARG; }
        hipLaunchKernelGGL(k_pred_wbias, dim3((uint32_t)nl, (uint32_t)((ns + WB_S - 1) / WB_S)), dim3(64), 0, s, p->d_wc[c], p->d_wdepth[c], p->meta.nk, p->meta.nik, p->meta.iki, p->meta.ikmc,
                           p->d_bias, ns, rows, (uint32_t)p->w_first, (uint32_t)p->w_row0);
        DEVCHK(hipGetLastError());
        hipLaunchKernelGGL(k_pred_bias_norm, dim3((uint32_t)nl), dim3(256), 0, s, p->meta.nk, p->meta.nik, p->d_bias, ns, (uint32_t)p->w_first);
        DEVCHK(hipGetLastError());
        { const dbtk_status_t st = launch_tile(k_pred_wfused, s, rows, ns, p->d_wc[c], p->d_wdepth[c], p->d_loc + p->w_row0, p->d_bias, p->d_raw, p->d_cor, rows, ns); if (st) return st; }
        DEVCHK(hipMemcpyAsync(p->h_raw, p->d_raw, rows * ns * sizeof(float), hipMemcpyDeviceToHost, s));
        DEVCHK(hipMemcpyAsync(p->h_cor, p->d_cor, rows * ns * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    p->pending = c; p->pend_rows = rows;
    return DBTK_OK;
}
dbtk_status_t dbtk_pred_window_outputs_pinned(dbtk_pred_t* p, const float** raw, const float** corrected, uint64_t* rows) {
    { const dbtk_status_t st = need_windowed(p, "dbtk_pred_window_outputs"); if (st) return st; }
    if (p->pending < 0) { const dbtk_status_t st = dbtk_pred_window_submit(p); if (st) return st; }
    DEVCHK(hipSetDevice(p->device));
    const int c = p->pending;
    p->pending = -1;  // (whatever the wait says: a failed window is not waited for twice)
    DEVCHK(hipStreamSynchronize(p->ws(c)));
    if (raw) *raw = p->h_raw;
    if (corrected) *corrected = p->h_cor;
    if (rows) *rows = p->pend_rows;
    return DBTK_OK;
}
dbtk_status_t dbtk_pred_window_outputs(dbtk_pred_t* p, float* raw_out, float* corrected_out) {
    const float *r = nullptr, *c = nullptr;
    uint64_t rows = 0;
    { const dbtk_status_t st = dbtk_pred_window_outputs_pinned(p, &r, &c, &rows); if (st) return st; }
    if (raw_out) memcpy(raw_out, r, rows * p->ns * sizeof(float));
    if (corrected_out) memcpy(corrected_out, c, rows * p->ns * sizeof(float));
    return DBTK_OK;
}
dbtk_status_t dbtk_pred_bias(dbtk_pred_t* p, float* out) {
    if (!p || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(p->device));
    DEVCHK(hipMemcpy(out, p->d_bias, p->ntr * p->ns * sizeof(float), hipMemcpyDeviceToHost));
    return DBTK_OK;
}
dbtk_status_t dbtk_pred_times(dbtk_pred_t* p, float ms[3]) {
    if (!p || !ms) { set_error("null argument"); return DBTK_ERR_ARG; }
    for (int i = 0; i < 3; ++i) ms[i] = p->ms[i];
    return DBTK_OK;
}

// ---- the entry points above that parse files or allocate host memory, behind the exception barrier (dbtk_internal.h: guarded)
dbtk_status_t dbtk_pred_create(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                               uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, dbtk_pred_t** out) {
    return dbtk::guarded([&] { return dbtk_pred_create_impl(device_id, ns, nk, ntr, nk_cum, nik_cum, nik, iki, ikmc, false, 0, out); });
}
dbtk_status_t dbtk_pred_create_from_file(int device_id, uint64_t ns, const char* ikmer_meta, dbtk_pred_t** out) {
    return dbtk::guarded([&] { return dbtk_pred_create_from_file_impl(device_id, ns, ikmer_meta, false, 0, out); });
}
dbtk_status_t dbtk_pred_create_windowed(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                                        uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, uint64_t max_rows, dbtk_pred_t** out) {
    return dbtk::guarded([&] { return dbtk_pred_create_impl(device_id, ns, nk, ntr, nk_cum, nik_cum, nik, iki, ikmc, true, max_rows, out); });
}
dbtk_status_t dbtk_pred_create_windowed_from_file(int device_id, uint64_t ns, const char* ikmer_meta, uint64_t max_rows, dbtk_pred_t** out) {
    return dbtk::guarded([&] { return dbtk_pred_create_from_file_impl(device_id, ns, ikmer_meta, true, max_rows, out); });
}
dbtk_status_t dbtk_pred_load_samples(dbtk_pred_t* p, uint64_t first_sample, uint64_t n, const uint64_t* counts, const float* read_depth) {
    return dbtk::guarded([&] { return dbtk_pred_load_samples_impl(p, first_sample, n, counts, read_depth); });
}

}  // extern "C"

// ---- the dosage handle (dbtk_pred.h, ABI v10)
struct dbtk_dosage {
    int device = 0;
    uint64_t ns = 0, nk = 0, ntr = 0, nik = 0;
    uint64_t* d_kms = nullptr;                   // [ntr][ns]
    float *d_raw = nullptr, *d_bias = nullptr;   // [ntr][ns]: the raw bias of the loads; normalised by dbtk_dosage_finish
    float* d_values = nullptr;                   // [ntr][ns]: what dbtk_dosage_values reads back (made by the call)
    float* d_depth = nullptr;                    // [ns]
    IkmerDev meta;
    uint32_t *d_floc = nullptr, *d_fbeg = nullptr;
    DosItem* d_items = nullptr;
    uint64_t* d_part = nullptr;
    Setup mem;                                   // the creation's allocations (all above)
    uint32_t nitems = 0, nfold = 0;
    uint64_t bytes = 0;
    std::vector<float> depth;                    // host copy: what the next load sends along
    bool finished = false;
    float ms[2] = {0, 0};
    // (gone with the handle, last to first: the staging, the events, the stream)
    DevStream stream;
    DevEvent ev[4];
    DevArr<uint64_t> d_stage;                    // 16 samples' counts of dbtk_dosage_load_samples, allocated by its first call
};
constexpr uint64_t DS_STAGE = 16;  // samples per transfer of dbtk_dosage_load_samples (what danbing-tk-pred stages for the matrix, too)

extern "C" {

void dbtk_dosage_free(dbtk_dosage_t* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    d->mem.release();
    delete d;
}

static dbtk_status_t dbtk_dosage_create_impl(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                                             uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, dbtk_dosage_t** out) {
    if (!out) { set_error("null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    { const dbtk_status_t cs = check_ikmer_meta(device_id, ns, nk, ntr, nk_cum, nik_cum, nik, iki, ikmc); if (cs) return cs; }
    std::vector<DosItem> items;
    std::vector<uint32_t> floc, fbeg;
    dbtk_pred_plan::dosage_items(ntr, nk_cum, nik != 0, &items, &floc, &fbeg);  // the work list of k_dosage_sample
    if (items.size() > 0x7FFFFFFFull) { set_error("too many work items for one launch"); return DBTK_ERR_ARG; }
    std::unique_ptr<dbtk_dosage, void (*)(dbtk_dosage*)> hold(new dbtk_dosage, dbtk_dosage_free);  // (freed, should a vector or a string below throw)
    dbtk_dosage* d = hold.get();
    d->depth.assign(ns, 1.f);
    d->device = device_id; d->ns = ns; d->nk = nk; d->ntr = ntr; d->nik = nik;
    d->nitems = (uint32_t)items.size(); d->nfold = (uint32_t)floc.size();
    const uint64_t cells = ntr * ns, nparts = fbeg.back();
    const struct { void** slot; uint64_t bytes; } tabs[] = {
        {(void**)&d->d_kms, cells * 8}, {(void**)&d->d_raw, cells * 4}, {(void**)&d->d_bias, cells * 4}, {(void**)&d->d_values, cells * 4}, {(void**)&d->d_depth, ns * 4},
        {(void**)&d->d_floc, (floc.size() + 1) * 4}, {(void**)&d->d_fbeg, fbeg.size() * 4}, {(void**)&d->d_items, (items.size() + 1) * sizeof(DosItem)}, {(void**)&d->d_part, (nparts + 1) * 8}};
    d->bytes = 2 * ntr * 4 + 2 * (nik + 1) * 4;  // (ikmer_upload's four)
    for (auto& t : tabs) d->bytes += t.bytes;
    const char* const what = "hipMalloc (dosage tables)";
    const std::string fit = "dosage tables: " + std::to_string(d->bytes) + " bytes (20 * ntr * ns = " + std::to_string(cells * 20) + " of them)";
    Setup& m = d->mem;
    DevStream& s = d->stream;
    STEP(m, s.create(hipStreamDefault), "hipStreamCreate");
    for (DevEvent& e : d->ev) STEP(m, e.create(hipEventDefault), "hipEventCreate");
    for (auto& t : tabs) m.device(t.slot, t.bytes, what, &fit);
    ikmer_upload(m, &d->meta, ntr, nk_cum, nik_cum, nik, iki, ikmc, s, what, &fit);
    STEP(m, hipMemsetAsync(d->d_kms, 0, cells * 8, s), "hipMemset");
    STEP(m, hipMemsetAsync(d->d_raw, 0, cells * 4, s), "hipMemset");
    STEP(m, hipMemsetAsync(d->d_bias, 0, cells * 4, s), "hipMemset");
    m.upload(d->d_depth, d->depth.data(), ns * 4, s);
    m.upload(d->d_items, items.data(), items.size() * sizeof(DosItem), s);
    m.upload(d->d_floc, floc.data(), floc.size() * 4, s);
    m.upload(d->d_fbeg, fbeg.data(), fbeg.size() * 4, s);
    STEP(m, hipStreamSynchronize(s), "hipStreamSynchronize");
    if (m.st) return m.st;
    *out = hold.release();
    return DBTK_OK;
}

static dbtk_status_t dbtk_dosage_create_from_file_impl(int device_id, uint64_t ns, const char* ikmer_meta, dbtk_dosage_t** out) {
    if (!ikmer_meta || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    IkmerMeta m;
    { const dbtk_status_t st = read_ikmer_meta(ikmer_meta, &m); if (st) return st; }
    return dbtk_dosage_create_impl(device_id, ns, m.nk, m.ntr, m.nkc.data(), m.nikc.data(), m.nik, m.iki.data(), m.kc.data(), out);
}

static dbtk_status_t dbtk_dosage_create_from_rpgg_impl(const dbtk_rpgg_t* g, int device_id, uint64_t ns, dbtk_dosage_t** out) {
    if (!g || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    if (!g->order_done || g->out_beg.size() != g->nloci + 1) { set_error("the RPGG handle has no output order"); return DBTK_ERR_ARG; }
    std::vector<uint32_t> nkc(g->nloci), nikc(g->nloci, 0u);
    for (uint64_t l = 0; l < g->nloci; ++l) nkc[l] = (uint32_t)g->out_beg[l + 1];  // (finish_order: below 2^32)
    return dbtk_dosage_create_impl(device_id, ns, g->out_kmer.size(), g->nloci, nkc.data(), nikc.data(), 0, nullptr, nullptr, out);
}

uint64_t dbtk_dosage_nk(const dbtk_dosage_t* d) { return d ? d->nk : 0; }
uint64_t dbtk_dosage_ntr(const dbtk_dosage_t* d) { return d ? d->ntr : 0; }
uint64_t dbtk_dosage_bytes(const dbtk_dosage_t* d) { return d ? d->bytes : 0; }

// n samples' counts in device memory -> their kms and raw entries, waited for; the kernels' time (ev[0] to ev[1]) is added to *ms_sum
static dbtk_status_t dosage_load(dbtk_dosage_t* d, uint64_t first, uint64_t n, const uint64_t* d_counts, const float* read_depth, float* ms_sum) {
    hipStream_t s = d->stream;
    for (uint64_t i = 0; i < n; ++i) d->depth[first + i] = read_depth[i];
    d->finished = false;
    DEVCHK(hipMemcpyAsync(d->d_depth + first, d->depth.data() + first, n * 4, hipMemcpyHostToDevice, s));
    DEVCHK(hipEventRecord(d->ev[0], s));
    for (uint64_t i = 0; i < n && d->nitems; ++i) {
        hipLaunchKernelGGL(k_dosage_sample, dim3(d->nitems), dim3(DS_T), 0, s, d_counts + i * d->nk, read_depth[i], d->d_items, d->meta.nk, d->meta.nik, d->meta.iki, d->meta.ikmc,
                           d->d_kms, d->d_raw, d->d_part, d->ns, first + i);
        DEVCHK(hipGetLastError());
        if (d->nfold) {
            hipLaunchKernelGGL(k_dosage_fold, dim3((d->nfold + 63) / 64), dim3(64), 0, s, d->d_floc, d->d_fbeg, d->d_part, d->d_kms, d->ns, first + i, d->nfold);
            DEVCHK(hipGetLastError());
        }
    }
    DEVCHK(hipEventRecord(d->ev[1], s));
    DEVCHK(hipStreamSynchronize(s));  // (d_counts is no longer being read)
    float ms = 0;
    DEVCHK(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    *ms_sum += ms;
    return DBTK_OK;
}

dbtk_status_t dbtk_dosage_load_device(dbtk_dosage_t* d, uint64_t first_sample, uint64_t n, const uint64_t* d_counts, const float* read_depth) {
    if (!d || !d_counts || !read_depth) { set_error("null argument"); return DBTK_ERR_ARG; }
    { const dbtk_status_t st = check_sample_range(first_sample, n, d->ns); if (st) return st; }
    if (!n) return DBTK_OK;
    DEVCHK(hipSetDevice(d->device));
    { const dbtk_status_t st = check_device_counts(d_counts, d->device, "dbtk_dosage_load_device"); if (st) return st; }
    float ms = 0;
    { const dbtk_status_t st = dosage_load(d, first_sample, n, d_counts, read_depth, &ms); if (st) return st; }
    d->ms[0] = ms;
    return DBTK_OK;
}

dbtk_status_t dbtk_dosage_load_ctx(dbtk_dosage_t* d, uint64_t sample, dbtk_ctx_t* ctx, float read_depth) {
    if (!d || !ctx) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (sample >= d->ns) { set_error("sample outside the cohort"); return DBTK_ERR_ARG; }
    static const char* const whose[2] = {"the dosage handle", "the dosage tables"};
    const uint64_t* base = nullptr;
    { const dbtk_status_t st = ctx_counts_ready(ctx, d->device, d->nk, whose, &base); if (st) return st; }
    float ms = 0;
    { const dbtk_status_t st = dosage_load(d, sample, 1, base, &read_depth, &ms); if (st) return st; }  // (d_accum is no longer being read: dbtk_ctx_reset may follow)
    d->ms[0] = ms;
    return DBTK_OK;
}

static dbtk_status_t dbtk_dosage_load_samples_impl(dbtk_dosage_t* d, uint64_t first_sample, uint64_t n, const uint64_t* counts, const float* read_depth) {
    if (!d || !counts || !read_depth) { set_error("null argument"); return DBTK_ERR_ARG; }
    { const dbtk_status_t st = check_sample_range(first_sample, n, d->ns); if (st) return st; }
    if (!n) return DBTK_OK;
    DEVCHK(hipSetDevice(d->device));
    if (!d->d_stage) {
        DEVCHK(d->d_stage.alloc(DS_STAGE * d->nk));
        d->bytes += DS_STAGE * d->nk * 8;
    }
    float ms = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += DS_STAGE) {
        const uint64_t ni = std::min<uint64_t>(DS_STAGE, n - i0);
        DEVCHK(hipMemcpyAsync(d->d_stage, counts + i0 * d->nk, ni * d->nk * 8, hipMemcpyHostToDevice, d->stream));
        { const dbtk_status_t st = dosage_load(d, first_sample + i0, ni, d->d_stage, read_depth + i0, &ms); if (st) return st; }  // (the staging buffer is free again)
    }
    d->ms[0] = ms;
    return DBTK_OK;
}

dbtk_status_t dbtk_dosage_finish(dbtk_dosage_t* d) {
    if (!d) { set_error("null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(d->device));
    hipStream_t s = d->stream;
    DEVCHK(hipEventRecord(d->ev[2], s));
    DEVCHK(hipMemcpyAsync(d->d_bias, d->d_raw, d->ntr * d->ns * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_pred_bias_norm, dim3((uint32_t)d->ntr), dim3(256), 0, s, d->meta.nk, d->meta.nik, d->d_bias, d->ns, 0u);
    DEVCHK(hipGetLastError());
    DEVCHK(hipEventRecord(d->ev[3], s));
    DEVCHK(hipStreamSynchronize(s));
    DEVCHK(hipEventElapsedTime(&d->ms[1], d->ev[2], d->ev[3]));
    d->finished = true;
    return DBTK_OK;
}

dbtk_status_t dbtk_dosage_kms(dbtk_dosage_t* d, uint64_t* out) {
    if (!d || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(d->device));
    DEVCHK(hipMemcpy(out, d->d_kms, d->ntr * d->ns * 8, hipMemcpyDeviceToHost));
    return DBTK_OK;
}
dbtk_status_t dbtk_dosage_bias(dbtk_dosage_t* d, float* out) {
    if (!d || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!d->finished) { set_error("dbtk_dosage_bias: samples were loaded since the last dbtk_dosage_finish (or it was never called)"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(d->device));
    DEVCHK(hipMemcpy(out, d->d_bias, d->ntr * d->ns * sizeof(float), hipMemcpyDeviceToHost));
    return DBTK_OK;
}
dbtk_status_t dbtk_dosage_values(dbtk_dosage_t* d, float* out) {
    if (!d || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!d->finished) { set_error("dbtk_dosage_values: samples were loaded since the last dbtk_dosage_finish (or it was never called)"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(d->device));
    hipLaunchKernelGGL(k_dosage_values, dim3((uint32_t)d->ntr, (uint32_t)((d->ns + 255) / 256)), dim3(256), 0, d->stream, d->d_kms, d->d_bias, d->d_depth, d->meta.nk, d->meta.nik, d->d_values, d->ns);
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpyAsync(out, d->d_values, d->ntr * d->ns * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    DEVCHK(hipStreamSynchronize(d->stream));
    return DBTK_OK;
}
dbtk_status_t dbtk_dosage_times(dbtk_dosage_t* d, float ms[2]) {
    if (!d || !ms) { set_error("null argument"); return DBTK_ERR_ARG; }
    ms[0] = d->ms[0]; ms[1] = d->ms[1];
    return DBTK_OK;
}

// ---- behind the exception barrier (dbtk_internal.h: guarded), like their dbtk_pred_* twins
dbtk_status_t dbtk_dosage_create(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                                 uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, dbtk_dosage_t** out) {
    return dbtk::guarded([&] { return dbtk_dosage_create_impl(device_id, ns, nk, ntr, nk_cum, nik_cum, nik, iki, ikmc, out); });
}
dbtk_status_t dbtk_dosage_create_from_file(int device_id, uint64_t ns, const char* ikmer_meta, dbtk_dosage_t** out) {
    return dbtk::guarded([&] { return dbtk_dosage_create_from_file_impl(device_id, ns, ikmer_meta, out); });
}
dbtk_status_t dbtk_dosage_create_from_rpgg(const dbtk_rpgg_t* rpgg, int device_id, uint64_t ns, dbtk_dosage_t** out) {
    return dbtk::guarded([&] { return dbtk_dosage_create_from_rpgg_impl(rpgg, device_id, ns, out); });
}
dbtk_status_t dbtk_dosage_load_samples(dbtk_dosage_t* d, uint64_t first_sample, uint64_t n, const uint64_t* counts, const float* read_depth) {
    return dbtk::guarded([&] { return dbtk_dosage_load_samples_impl(d, first_sample, n, counts, read_depth); });
}

}  // extern "C"

// ---- the rows of the two handles for the association scan (dbtk_internal.h)
namespace dbtk {
static dbtk_status_t rows_meta(RowsView* out, const IkmerDev& meta, uint64_t ntr, hipStream_t s) {
    out->nk_cum.resize(ntr);
    DEVCHK(hipMemcpyAsync(out->nk_cum.data(), meta.nk, ntr * 4, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    return DBTK_OK;
}
dbtk_status_t pred_rows(dbtk_pred* p, RowsView* out) {
    if (!p || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (p->windowed) { set_error("a windowed handle holds a part of the rows at a time: the association scan needs the whole matrix (dbtk_pred_create)"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(p->device));
    out->device = p->device; out->ns = p->ns; out->nrows = p->nk; out->ntr = p->ntr; out->d_rows = p->d_G;
    return rows_meta(out, p->meta, p->ntr, p->stream);
}
dbtk_status_t dosage_rows(dbtk_dosage* d, RowsView* out) {
    if (!d || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!d->finished) { set_error("the dosage handle is unfinished: samples were loaded since the last dbtk_dosage_finish (or it was never called)"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(d->device));
    hipLaunchKernelGGL(k_dosage_values, dim3((uint32_t)d->ntr, (uint32_t)((d->ns + 255) / 256)), dim3(256), 0, d->stream, d->d_kms, d->d_bias, d->d_depth, d->meta.nk, d->meta.nik, d->d_values, d->ns);
    DEVCHK(hipGetLastError());
    out->device = d->device; out->ns = d->ns; out->nrows = d->ntr; out->ntr = d->ntr; out->d_rows = d->d_values;
    { const dbtk_status_t st = rows_meta(out, d->meta, d->ntr, d->stream); if (st) return st; }
    for (uint64_t t = 0; t < d->ntr; ++t) out->nk_cum[t] = (uint32_t)(t + 1);  // a row per locus
    return DBTK_OK;
}
}  // namespace dbtk
