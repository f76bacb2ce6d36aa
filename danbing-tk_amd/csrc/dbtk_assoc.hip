// dbtk_assoc.hip — the association scan (include/dbtk_assoc.h) and its covariates (include/dbtk_assoc_covar.h): the phenotype centring,
// the phenotypes' projections on the covariate basis, the scan kernel, the handle and the host fold.  The permutation pass
// (include/dbtk_assoc_perm.h) is dbtk_assoc_perm_dev.h, included at the end of this file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dbtk_assoc.h"
#include "../../include/dbtk_assoc_covar.h"
#include "../../include/dbtk_assoc_perm.h"
#include "dbtk_assoc_covar_host.h"
#include "dbtk_assoc_host.h"
#include "dbtk_dev.h"
#include "dbtk_internal.h"

using namespace dbtk;

namespace {

// ---- the shape of the scan (DESIGN.md 7.3 has the table; tests/test_assoc_gpu.py crosses every one of them)
constexpr uint32_t AS_TILE = 4;                     // rows a wave holds in registers
constexpr uint32_t AS_WAVES = 8;                    // waves of a workgroup: AS_TILE * AS_WAVES rows share the staged phenotypes
constexpr uint32_t AS_CHUNK = 8;                    // phenotypes staged in LDS at a time
constexpr uint32_t AS_REG = 8;                      // samples of a row a lane holds
constexpr uint32_t AS_SEG = 64 * AS_REG;            // samples of a segment; up to this n a row tile stays in registers for all its passes
constexpr uint32_t AS_ITEM_ROWS = 256;              // rows of a work item at most (one candidate per item and phenotype leaves the kernel)
constexpr uint64_t AS_HITS_DEFAULT = 1ull << 20;    // entries of the hit buffer without DBTK_ASSOC_HITS
constexpr uint32_t AS_ROWS = AS_TILE * AS_WAVES;    // rows of a workgroup's pass
constexpr uint32_t AS_ACC = AS_TILE * AS_CHUNK;     // accumulators of a wave
constexpr uint32_t AS_GRID = 2048;                  // workgroups at most; the items are taken round robin
constexpr uint32_t AS_COVAR_MAX = 128;              // covariates at most: the a_j of a pass' rows take AS_ROWS * AS_COVAR_MAX * 8 bytes of LDS
constexpr double AS_COLLINEAR = DBTK_ASSOC_COVAR_COLLINEAR;
static_assert(AS_COVAR_MAX == DBTK_ASSOC_COVAR_MAX && AS_COVAR_MAX == dbtk_assoc_host::COVAR_MAX && AS_COLLINEAR == dbtk_assoc_host::COVAR_COLLINEAR, "one cap and one threshold");
static_assert(AS_ACC == 32, "as_reduce hands element e to lanes 2e and 2e + 1: 32 elements over 64 lanes");
static_assert(AS_ITEM_ROWS % AS_ROWS == 0 && AS_WAVES * 64 == AS_SEG, "a workgroup stages one segment with one value per thread");

// rows [row0, row0 + nrows) against the phenotypes ph_idx[ph_off .. ph_off + ph_n) (the identity without a pair list); the item's
// candidates are cand[cand_off .. cand_off + ph_n)
struct AsItem { uint64_t ph_off, cand_off; uint32_t row0, nrows, ph_n, pad; };
// the best tested row of an item for one phenotype (row == DBTK_ASSOC_NONE: none), and the item's tested and skipped rows
struct AsCand { double r; uint32_t row, tested, skipped, pad; };
struct AsHit { uint32_t row, ph; double r; };

struct AsArgs {
    const float* G;          // [nrows][ns]
    uint64_t ns;
    uint32_t n;              // samples of the mask
    const uint32_t* sidx;    // [n] ascending (not read when the mask is everything)
    const double* yc;        // [P][n] centred phenotypes
    const double* syy;       // [P] their sums of squares (with covariates: Syy', what the covariates leave of them)
    const AsItem* items;
    uint32_t nitems;
    const uint32_t* ph_idx;  // null: the identity
    AsCand* cand;
    AsHit* hits;
    unsigned long long* nhits;
    uint64_t hit_cap;
    double r2crit;           // above 1: no hits are collected
    // the covariates, read by the COVAR instances alone (behind everything else: the other instances keep the argument layout they had)
    const double* Q;         // [q][n] the orthonormal basis of the centred covariates
    const double* bt;        // [P][q] b_j = sum dy Q_j of every phenotype
    uint32_t q;              // covariates (0: none)
};

// The one summation tree of the scan: a lane adds its samples lane, lane + 64, ... in ascending order, the wave adds the lanes by
// xor 32, 16, 8, 4, 2, 1.  Rows and phenotypes go through the same tree, so a row that equals a phenotype has Sxy == Sxx == Syy.
__device__ __forceinline__ double as_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// The same tree for AS_ACC sums at once, in a sixth of the shuffles: at every step a lane keeps half of its values and sends the other
// half to its partner.  Lanes 2e and 2e + 1 return the sum of element e.  (Every stage has its own array and reads its two operands
// before it chooses between them: a select between two elements of ONE array is turned into an indexed load, and the accumulators
// then live in scratch memory.)
__device__ __forceinline__ double as_reduce(const double (&a)[AS_ACC], uint32_t lane) {
    const bool u32 = (lane & 32u) != 0, u16 = (lane & 16u) != 0, u8 = (lane & 8u) != 0, u4 = (lane & 4u) != 0, u2 = (lane & 2u) != 0;
    double b[16], c[8], d[4], e[2];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double lo = a[k], hi = a[k + 16]; b[k] = (u32 ? hi : lo) + __shfl_xor(u32 ? lo : hi, 32); }
#pragma unroll
    for (int k = 0; k < 8; ++k) { const double lo = b[k], hi = b[k + 8]; c[k] = (u16 ? hi : lo) + __shfl_xor(u16 ? lo : hi, 16); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double lo = c[k], hi = c[k + 4]; d[k] = (u8 ? hi : lo) + __shfl_xor(u8 ? lo : hi, 8); }
#pragma unroll
    for (int k = 0; k < 2; ++k) { const double lo = d[k], hi = d[k + 2]; e[k] = (u4 ? hi : lo) + __shfl_xor(u4 ? lo : hi, 4); }
    const double f = (u2 ? e[1] : e[0]) + __shfl_xor(u2 ? e[0] : e[1], 2);
    return f + __shfl_xor(f, 1);
}

// One wave per phenotype: y[p][0 .. n) becomes y - mean in place, syy[p] its sum of squares.
__global__ void __launch_bounds__(64) k_assoc_pheno(double* __restrict__ y, double* __restrict__ syy, uint32_t n) {
    const uint32_t lane = threadIdx.x;
    double* v = y + (uint64_t)blockIdx.x * n;
    double sum = 0.0;
    for (uint32_t j = lane; j < n; j += 64) sum += v[j];
    const double mu = as_wave_sum(sum) / (double)n;
    double ss = 0.0;
    for (uint32_t j = lane; j < n; j += 64) {
        const double d = v[j] - mu;
        v[j] = d;
        ss = fma(d, d, ss);
    }
    ss = as_wave_sum(ss);
    if (lane == 0) syy[blockIdx.x] = ss;
}

// One wave per phenotype, beside k_assoc_pheno: bt[p][j] = sum_i yc[p][i] Q[j][i] through the rows' summation tree (a lane's samples
// ascending by fma, then as_wave_sum), and syyr[p] = syy[p] - sum_j b_j^2, j ascending by fma.
__global__ void __launch_bounds__(64) k_assoc_covar_pheno(const double* __restrict__ yc, const double* __restrict__ syy, const double* __restrict__ Q,
                                                          double* __restrict__ bt, double* __restrict__ syyr, uint32_t n, uint32_t q) {
    const uint32_t lane = threadIdx.x;
    const double* v = yc + (uint64_t)blockIdx.x * n;
    double left = syy[blockIdx.x];
    for (uint32_t j = 0; j < q; ++j) {
        const double* c = Q + (uint64_t)j * n;
        double s = 0.0;
        for (uint32_t i = lane; i < n; i += 64) s = fma(v[i], c[i], s);
        const double b = as_wave_sum(s);
        left = fma(-b, b, left);
        if (lane == 0) bt[(uint64_t)blockIdx.x * q + j] = b;
    }
    if (lane == 0) syyr[blockIdx.x] = left;
}

// the register slots of a lane that a segment fills: 64 samples each (the same for every thread; the slots behind them are not touched)
__device__ __forceinline__ uint32_t as_slots(uint32_t n, uint32_t seg0) { return (min(n - seg0, AS_SEG) + 63u) / 64u; }

// the samples seg0 + lane + 64 i of the wave's AS_TILE rows; 0 past the mask's end
template <bool IDENT>
__device__ __forceinline__ void as_load(const AsArgs& a, const uint64_t (&base)[AS_TILE], uint32_t seg0, uint32_t lane, float (&x)[AS_TILE][AS_REG]) {
    const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
    for (uint32_t i = 0; i < AS_REG; ++i) {
        if (i >= ni) break;
        const uint32_t j = seg0 + lane + 64 * i;
        const bool in = j < a.n;
        const uint32_t s = in ? (IDENT ? j : a.sidx[j]) : 0u;
#pragma unroll
        for (uint32_t t = 0; t < AS_TILE; ++t) x[t][i] = in ? a.G[base[t] + s] : 0.f;
    }
}

// A workgroup takes an item AS_ROWS rows at a time, AS_TILE rows per wave.  Per pass: the mean, the min == max / finite test and Sxx of
// every row (the row tile in registers when n <= AS_SEG, read again segment by segment otherwise); then, AS_CHUNK phenotypes at a
// time, the workgroup stages a segment of the centred phenotypes in LDS and every wave adds it to its AS_TILE x AS_CHUNK
// accumulators: a staged value serves AS_TILE multiply-adds.  The accumulators are summed across the wave (as_reduce), a lane per
// (row, phenotype) makes r and enters a hit under one atomic counter add per wave, and thread c folds the pass' rows into the
// item's candidate of phenotype c in row order (strict >: a tie stays with the lower row).
// COVAR: in front of the phenotype chunks the q columns of Q go through the same chunk machinery, AS_CHUNK at a time, as phenotypes that
// every row meets: their sums are the rows' a_j, kept in LDS.  Sxx' = Sxx - sum a_j^2 then replaces Sxx, a row that the covariates
// explain leaves the tested ones (so tst is written only now), and the lane that makes r first takes sum_j a_j b_j off Sxy.
template <bool IDENT, bool COVAR>
__global__ void __launch_bounds__(AS_WAVES * 64) k_assoc_scan(const AsArgs a) {
    __shared__ double zl[AS_CHUNK][AS_SEG];
    __shared__ double aj[COVAR ? AS_COVAR_MAX : 1][AS_ROWS];  // (the rows of a wave side by side: its lanes read AS_TILE neighbours; not referenced without COVAR)
    __shared__ double rbuf[AS_WAVES][AS_ACC];
    __shared__ uint32_t tst[AS_WAVES][AS_TILE];  // 0: no row, 1: tested, 2: skipped
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const bool resident = a.n <= AS_SEG;
    const double dn = (double)a.n;
    for (uint32_t q = blockIdx.x; q < a.nitems; q += gridDim.x) {  // (the same trips for every thread: the barriers are uniform)
        const AsItem it = a.items[q];
        for (uint32_t sub = 0; sub < it.nrows; sub += AS_ROWS) {
            __syncthreads();  // the fold of the pass before is done with tst and rbuf
            uint64_t base[AS_TILE];
            bool on[AS_TILE], tested[AS_TILE];
#pragma unroll
            for (uint32_t t = 0; t < AS_TILE; ++t) {
                const uint32_t k = sub + w * AS_TILE + t;
                on[t] = k < it.nrows;
                base[t] = (uint64_t)(it.row0 + (on[t] ? k : it.nrows - 1)) * a.ns;  // (a row off the item reads the item's last row and is ignored)
            }
            float x[AS_TILE][AS_REG];
            double mu[AS_TILE], sxx[AS_TILE];
            {
                double sum[AS_TILE];
                float mn[AS_TILE], mx[AS_TILE];
                bool fin[AS_TILE];
#pragma unroll
                for (uint32_t t = 0; t < AS_TILE; ++t) { sum[t] = 0.0; mn[t] = INFINITY; mx[t] = -INFINITY; fin[t] = true; }
                for (uint32_t seg0 = 0; seg0 < a.n; seg0 += AS_SEG) {
                    as_load<IDENT>(a, base, seg0, lane, x);
                    const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
                    for (uint32_t i = 0; i < AS_REG; ++i) {
                        if (i >= ni) break;
                        const bool in = seg0 + lane + 64 * i < a.n;
#pragma unroll
                        for (uint32_t t = 0; t < AS_TILE; ++t) {
                            const float v = x[t][i];
                            sum[t] += (double)v;  // (0 past the end)
                            if (in) { mn[t] = fminf(mn[t], v); mx[t] = fmaxf(mx[t], v); fin[t] = fin[t] && isfinite(v); }
                        }
                    }
                }
#pragma unroll
                for (uint32_t t = 0; t < AS_TILE; ++t) {
                    mu[t] = as_wave_sum(sum[t]) / dn;
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) { mn[t] = fminf(mn[t], __shfl_xor(mn[t], d)); mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], d)); }
                    tested[t] = on[t] && __all(fin[t]) && mn[t] != mx[t];
                    sxx[t] = 0.0;
                }
            }
            for (uint32_t seg0 = 0; seg0 < a.n; seg0 += AS_SEG) {
                if (!resident) as_load<IDENT>(a, base, seg0, lane, x);
                const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
                for (uint32_t i = 0; i < AS_REG; ++i) {
                    if (i >= ni) break;
                    const bool in = seg0 + lane + 64 * i < a.n;
#pragma unroll
                    for (uint32_t t = 0; t < AS_TILE; ++t) {
                        const double d = in ? (double)x[t][i] - mu[t] : 0.0;
                        sxx[t] = fma(d, d, sxx[t]);
                    }
                }
            }
#pragma unroll
            for (uint32_t t = 0; t < AS_TILE; ++t) {
                sxx[t] = as_wave_sum(sxx[t]);
                if (!COVAR && lane == t) tst[w][t] = on[t] ? (tested[t] ? 1u : 2u) : 0u;
            }
            const uint32_t qpad = COVAR ? (a.q + AS_CHUNK - 1) / AS_CHUNK * AS_CHUNK : 0u;  // the covariate chunks come first
            for (uint32_t cc = 0; cc < qpad + it.ph_n; cc += AS_CHUNK) {
                const bool cov = COVAR && cc < qpad;
                const uint32_t c0 = cc - (cov ? 0u : qpad);
                const uint32_t cn = min(AS_CHUNK, (cov ? a.q : it.ph_n) - c0);
                double acc[AS_ACC];
#pragma unroll
                for (uint32_t e = 0; e < AS_ACC; ++e) acc[e] = 0.0;
                for (uint32_t seg0 = 0; seg0 < a.n; seg0 += AS_SEG) {
                    if (!resident) as_load<IDENT>(a, base, seg0, lane, x);
                    __syncthreads();  // the segment before has been read (and, the first time, the fold before is done with rbuf)
                    for (uint32_t c = 0; c < cn; ++c) {
                        if (cov) { zl[c][tid] = seg0 + tid < a.n ? a.Q[(uint64_t)(c0 + c) * a.n + seg0 + tid] : 0.0; continue; }
                        const uint64_t ph = a.ph_idx ? a.ph_idx[it.ph_off + c0 + c] : c0 + c;
                        zl[c][tid] = seg0 + tid < a.n ? a.yc[ph * a.n + seg0 + tid] : 0.0;  // (0 past the end: adds nothing)
                    }
                    __syncthreads();
                    const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
                    for (uint32_t i = 0; i < AS_REG; ++i) {
                        if (i >= ni) break;
                        double dx[AS_TILE];
#pragma unroll
                        for (uint32_t t = 0; t < AS_TILE; ++t) dx[t] = (double)x[t][i] - mu[t];
#pragma unroll
                        for (uint32_t c = 0; c < AS_CHUNK; ++c) {
                            if (c < cn) {
                                const double z = zl[c][lane + 64 * i];
#pragma unroll
                                for (uint32_t t = 0; t < AS_TILE; ++t) acc[t * AS_CHUNK + c] = fma(dx[t], z, acc[t * AS_CHUNK + c]);
                            }
                        }
                    }
                }
                double sxy = as_reduce(acc, lane);
                const uint32_t e = lane >> 1, t = e / AS_CHUNK, c = e % AS_CHUNK;
                if constexpr (COVAR) {
                    if (cov) {
                        if (!(lane & 1u) && c < cn) aj[c0 + c][w * AS_TILE + t] = sxy;
                        if (cc + AS_CHUNK < qpad) continue;
                        __syncthreads();  // the a_j of every chunk are in LDS (each wave reads its own rows only)
#pragma unroll
                        for (uint32_t u = 0; u < AS_TILE; ++u) {
                            double left = sxx[u];
                            for (uint32_t j = 0; j < a.q; ++j) { const double v = aj[j][w * AS_TILE + u]; left = fma(-v, v, left); }
                            tested[u] = tested[u] && left > AS_COLLINEAR * sxx[u];
                            sxx[u] = left;
                            if (lane == u) tst[w][u] = on[u] ? (tested[u] ? 1u : 2u) : 0u;
                        }
                        continue;
                    }
                }
                const double sx = t == 0 ? sxx[0] : t == 1 ? sxx[1] : t == 2 ? sxx[2] : sxx[3];
                const bool tt = t == 0 ? tested[0] : t == 1 ? tested[1] : t == 2 ? tested[2] : tested[3];
                const bool mine = !(lane & 1u) && c < cn && tt;
                uint32_t ph = 0;
                double r = 0.0;
                if (mine) {
                    ph = a.ph_idx ? a.ph_idx[it.ph_off + c0 + c] : c0 + c;
                    if constexpr (COVAR) {
                        const double* b = a.bt + (uint64_t)ph * a.q;
                        for (uint32_t j = 0; j < a.q; ++j) sxy = fma(-aj[j][w * AS_TILE + t], b[j], sxy);
                    }
                    r = sxy / sqrt(sx * a.syy[ph]);
                    r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
                }
                if (!(lane & 1u)) rbuf[w][e] = r;
                const bool hit = mine && r * r >= a.r2crit;
                const unsigned long long m = __ballot(hit);
                if (m) {  // (uniform in the wave)
                    unsigned long long at = 0;
                    if (lane == 0) at = atomicAdd(a.nhits, (unsigned long long)__popcll(m));
                    at = __shfl(at, 0) + __popcll(m & ((1ull << lane) - 1ull));
                    if (hit && at < a.hit_cap) a.hits[at] = AsHit{it.row0 + sub + w * AS_TILE + t, ph, r};
                }
                __syncthreads();
                if (tid < cn) {
                    AsCand* out = &a.cand[it.cand_off + c0 + tid];
                    AsCand b = sub ? *out : AsCand{0.0, DBTK_ASSOC_NONE, 0u, 0u, 0u};  // (this thread wrote it in the pass before)
                    for (uint32_t ww = 0; ww < AS_WAVES; ++ww)
                        for (uint32_t u = 0; u < AS_TILE; ++u) {
                            const uint32_t s = tst[ww][u];
                            b.skipped += s == 2u;
                            if (s != 1u) continue;
                            ++b.tested;
                            const double rr = rbuf[ww][u * AS_CHUNK + tid];
                            if (b.row == DBTK_ASSOC_NONE || rr * rr > b.r * b.r) { b.r = rr; b.row = it.row0 + sub + ww * AS_TILE + u; }
                        }
                    *out = b;
                }
            }
        }
    }
}

uint64_t hits_capacity(bool* ok) {
    *ok = true;
    const char* e = getenv("DBTK_ASSOC_HITS");
    if (!e || !*e) return AS_HITS_DEFAULT;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (*end || !v || (v & (v - 1)) || v > (1ull << 32)) { *ok = false; return 0; }
    return v;
}

}  // namespace

struct dbtk_assoc {
    int device = 0;
    uint64_t ns = 0, P = 0, n = 0;
    bool ident = false;               // the mask is every sample: no index list
    std::vector<std::string> names;
    uint64_t hit_cap = 0;
    // the pair list (d_idx)
    bool pairs = false;
    uint64_t ntr = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> idx;
    // the covariates (dbtk_assoc_covar.h; d_Q, d_bt, d_syyr); q == 0: none
    std::vector<uint64_t> ord;        // ord[j]: the position in sample_of of the j-th sample in ascending order
    uint64_t q = 0;
    // the device side (destroyed last to first: the tables from d_sidx on, then the events, the stream behind them all)
    DevStream stream;
    DevEvent ev[2];
    DevEvent pev[2];                  // around the permutation kernel (made with the first permutations)
    DevArr<double> d_yres;            // the permutations (dbtk_assoc_perm.h, dbtk_assoc_perm_dev.h): with covariates the phenotypes' residuals,
    DevArr<unsigned long long> d_T;   // the P (B + 1) maxima,
    DevArr<uint32_t> d_perm;          // the table, the identity in front
    DevArr<double> d_syyr, d_bt, d_Q;
    DevArr<AsCand> d_cand;            // per scan, regrown (and d_items)
    DevArr<AsItem> d_items;
    DevArr<uint32_t> d_idx;
    DevArr<unsigned long long> d_nhits;
    DevArr<AsHit> d_hits;
    DevArr<double> d_syy, d_yc;
    DevArr<uint32_t> d_sidx;
    // the scan made last
    bool scanned = false, with_hits = false;
    std::vector<dbtk_assoc_best_t> best;
    std::vector<dbtk_assoc_hit_t> hits;
    double ms[2] = {0, 0};
    std::vector<AsItem> items;        // its work items, which the permutation pass takes again
    // the permutations and the permutation scan made last
    uint64_t B = 0;
    std::vector<uint32_t> perm;
    bool perm_done = false;
    std::vector<double> T;
    std::vector<dbtk_assoc_perm_result_t> pres;
    double pms[2] = {0, 0};
};

namespace {

uint32_t locus_of(const std::vector<uint32_t>& nkc, uint64_t row) {
    const auto it = std::upper_bound(nkc.begin(), nkc.end(), (uint32_t)row);  // the first locus whose cumulative count passes the row
    return it == nkc.end() ? DBTK_ASSOC_NONE : (uint32_t)(it - nkc.begin());
}
template <class T> dbtk_status_t regrow(DevArr<T>& a, uint64_t need, const char* what) {
    const hipError_t e = a.reserve(need, need);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        set_error(std::string(what) + ": " + std::to_string(need * sizeof(T)) + " bytes do not fit, " + std::to_string(fr) + " of " + std::to_string(tot) + " bytes of HBM are free");
        return DBTK_ERR_NOMEM;
    }
    if (e != hipSuccess) { set_error(std::string("hipMalloc (") + what + "): " + hipGetErrorString(e)); return DBTK_ERR_HIP; }
    return DBTK_OK;
}

dbtk_status_t assoc_create_impl(int device_id, uint64_t ns, uint64_t P, uint64_t n, const uint64_t* sample_of, const double* pheno, const char* const* names, dbtk_assoc_t** out) {
    if (!out) { set_error("null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    if (!sample_of || !pheno) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!P) { set_error("dbtk_assoc_create: no phenotype"); return DBTK_ERR_ARG; }
    if (n < 3) { set_error("dbtk_assoc_create: " + std::to_string(n) + " samples: a test needs at least 3 (n - 2 degrees of freedom)"); return DBTK_ERR_ARG; }
    if (ns > 0xFFFFFFFFull || P > 0xFFFFFFFFull) { set_error("dbtk_assoc_create: more than 2^32 samples or phenotypes"); return DBTK_ERR_ARG; }
    bool cap_ok = true;
    const uint64_t hit_cap = hits_capacity(&cap_ok);
    if (!cap_ok) { set_error("DBTK_ASSOC_HITS must be a power of two between 1 and 2^32"); return DBTK_ERR_ARG; }
    // the samples in ascending order, the columns of the table with them
    std::vector<uint64_t> ord(n);
    for (uint64_t j = 0; j < n; ++j) ord[j] = j;
    std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return sample_of[a] < sample_of[b]; });
    std::vector<uint32_t> sidx(n);
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t s = sample_of[ord[j]];
        if (s >= ns) { set_error("dbtk_assoc_create: sample " + std::to_string(s) + " >= the cohort's " + std::to_string(ns)); return DBTK_ERR_ARG; }
        if (j && s == sample_of[ord[j - 1]]) { set_error("dbtk_assoc_create: sample " + std::to_string(s) + " is given twice"); return DBTK_ERR_ARG; }
        sidx[j] = (uint32_t)s;
    }
    std::unique_ptr<dbtk_assoc, void (*)(dbtk_assoc*)> hold(new dbtk_assoc, dbtk_assoc_free);
    dbtk_assoc* h = hold.get();
    h->names.resize(P);
    for (uint64_t p = 0; p < P; ++p) h->names[p] = names && names[p] ? names[p] : "p" + std::to_string(p);
    std::vector<double> y(P * n);
    for (uint64_t p = 0; p < P; ++p) {
        double mn = INFINITY, mx = -INFINITY;
        for (uint64_t j = 0; j < n; ++j) {
            const double v = pheno[p * n + ord[j]];
            if (!std::isfinite(v)) { set_error("dbtk_assoc_create: phenotype " + h->names[p] + " has a value that is not finite (sample " + std::to_string(sidx[j]) + ")"); return DBTK_ERR_ARG; }
            mn = std::min(mn, v); mx = std::max(mx, v);
            y[p * n + j] = v;
        }
        if (mn == mx) { set_error("dbtk_assoc_create: phenotype " + h->names[p] + " is constant over the " + std::to_string(n) + " samples"); return DBTK_ERR_ARG; }
        // (the values go up as they are: the device centres them in the order in which it sums a row, k_assoc_pheno)
        double mean = 0.0, ss = 0.0;
        for (uint64_t j = 0; j < n; ++j) mean += y[p * n + j];
        mean /= (double)n;
        for (uint64_t j = 0; j < n; ++j) ss += (y[p * n + j] - mean) * (y[p * n + j] - mean);
        if (!(ss > 0.0) || !std::isfinite(ss)) { set_error("dbtk_assoc_create: phenotype " + h->names[p] + " has a sum of squares that is 0 or overflows in float64"); return DBTK_ERR_ARG; }
    }
    int ndev = 0;
    if (const dbtk_status_t nd = device_count(&ndev)) return nd;
    if (device_id < 0 || device_id >= ndev) { set_error("device_id out of range"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(device_id));
    h->device = device_id; h->ns = ns; h->P = P; h->n = n; h->hit_cap = hit_cap;
    h->ident = n == ns;
    h->ord = ord;
    DEVCHK(h->stream.create(hipStreamDefault));
    for (DevEvent& e : h->ev) DEVCHK(e.create(hipEventDefault));
    const std::string what = "association tables (phenotypes 8 * P * n = " + std::to_string(8 * P * n) + " bytes, hit buffer 16 * DBTK_ASSOC_HITS = " + std::to_string(16 * hit_cap) + " bytes)";
    { const dbtk_status_t st = regrow(h->d_yc, P * n, what.c_str()); if (st) return st; }
    { const dbtk_status_t st = regrow(h->d_syy, P, what.c_str()); if (st) return st; }
    { const dbtk_status_t st = regrow(h->d_sidx, n, what.c_str()); if (st) return st; }
    { const dbtk_status_t st = regrow(h->d_hits, hit_cap, what.c_str()); if (st) return st; }
    { const dbtk_status_t st = regrow(h->d_nhits, 1, what.c_str()); if (st) return st; }
    DEVCHK(hipMemcpyAsync(h->d_yc, y.data(), P * n * 8, hipMemcpyHostToDevice, h->stream));
    DEVCHK(hipMemcpyAsync(h->d_sidx, sidx.data(), n * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_assoc_pheno, dim3((uint32_t)P), dim3(64), 0, h->stream, h->d_yc.get(), h->d_syy.get(), (uint32_t)n);
    DEVCHK(hipGetLastError());
    DEVCHK(hipStreamSynchronize(h->stream));
    *out = hold.release();
    return DBTK_OK;
}

dbtk_status_t assoc_set_pairs_impl(dbtk_assoc_t* h, uint64_t ntr, const uint64_t* off, const uint32_t* pheno_idx) {
    if (!h) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!ntr) { h->pairs = false; h->ntr = 0; h->off.clear(); h->idx.clear(); return DBTK_OK; }
    if (!off || (off[ntr] && !pheno_idx)) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (off[0]) { set_error("dbtk_assoc_set_pairs: off[0] must be 0"); return DBTK_ERR_ARG; }
    for (uint64_t t = 0; t < ntr; ++t)
        if (off[t + 1] < off[t]) { set_error("dbtk_assoc_set_pairs: off decreases at locus " + std::to_string(t)); return DBTK_ERR_ARG; }
    for (uint64_t i = 0; i < off[ntr]; ++i)
        if (pheno_idx[i] >= h->P) { set_error("dbtk_assoc_set_pairs: phenotype index " + std::to_string(pheno_idx[i]) + " >= P = " + std::to_string(h->P)); return DBTK_ERR_ARG; }
    std::vector<uint64_t> o(ntr + 1, 0);
    std::vector<uint32_t> x;
    x.reserve(off[ntr]);
    for (uint64_t t = 0; t < ntr; ++t) {  // sorted within the locus, each once
        std::vector<uint32_t> v(pheno_idx + off[t], pheno_idx + off[t + 1]);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        x.insert(x.end(), v.begin(), v.end());
        o[t + 1] = x.size();
    }
    DEVCHK(hipSetDevice(h->device));
    DevArr<uint32_t> d_idx;  // (made whole before the handle sees it: a failure leaves the old pair list as it was)
    DEVCHK(d_idx.alloc(x.size() + 1));
    if (!x.empty()) DEVCHK(hipMemcpy(d_idx, x.data(), x.size() * 4, hipMemcpyHostToDevice));
    h->d_idx = std::move(d_idx); h->pairs = true; h->ntr = ntr; h->off.swap(o); h->idx.swap(x);
    return DBTK_OK;
}

dbtk_status_t assoc_scan_impl(dbtk_assoc_t* h, const float* d_rows, uint64_t nrows, uint64_t ntr, const uint32_t* nk_cum, double p_threshold) {
    if (!h || !d_rows) { set_error("null argument"); return DBTK_ERR_ARG; }
    h->scanned = false; h->perm_done = false;
    if (std::isnan(p_threshold)) { set_error("dbtk_assoc_scan: p_threshold is not a number"); return DBTK_ERR_ARG; }
    if (!nrows || nrows > 0xFFFFFFFEull) { set_error("dbtk_assoc_scan: " + std::to_string(nrows) + " rows (1 .. 2^32 - 2)"); return DBTK_ERR_ARG; }
    if (h->pairs && ntr != h->ntr) { set_error("dbtk_assoc_scan: the pair list is over " + std::to_string(h->ntr) + " loci, the matrix has " + std::to_string(ntr)); return DBTK_ERR_ARG; }
    if (h->pairs && !nk_cum) { set_error("dbtk_assoc_scan: a pair list needs the loci's cumulative row counts"); return DBTK_ERR_ARG; }
    if (!h->pairs && h->P > DBTK_ASSOC_ALL_PAIRS_MAX) {
        set_error("dbtk_assoc_scan: " + std::to_string(h->P) + " phenotypes against every row need a pair list (all against all is allowed up to " + std::to_string(DBTK_ASSOC_ALL_PAIRS_MAX) + ")");
        return DBTK_ERR_ARG;
    }
    std::vector<uint32_t> nkc;
    if (nk_cum) {
        nkc.assign(nk_cum, nk_cum + ntr);
        for (uint64_t t = 0; t < ntr; ++t)
            if (nkc[t] > nrows || (t && nkc[t] < nkc[t - 1])) { set_error("dbtk_assoc_scan: the cumulative row counts decrease or pass the " + std::to_string(nrows) + " rows at locus " + std::to_string(t)); return DBTK_ERR_ARG; }
    }
    if (!is_device_memory_of(d_rows, h->device)) { set_error("dbtk_assoc_scan: the rows are not device memory of the handle's device"); return DBTK_ERR_ARG; }
    // the work items
    std::vector<AsItem> items;
    uint64_t ncand = 0;
    auto add = [&](uint64_t r0, uint64_t r1, uint64_t ph_off, uint64_t ph_n) {
        for (uint64_t r = r0; r < r1 && ph_n; r += AS_ITEM_ROWS) {
            items.push_back(AsItem{ph_off, ncand, (uint32_t)r, (uint32_t)std::min<uint64_t>(AS_ITEM_ROWS, r1 - r), (uint32_t)ph_n, 0u});
            ncand += ph_n;
        }
    };
    if (h->pairs) for (uint64_t t = 0; t < ntr; ++t) add(t ? nkc[t - 1] : 0, nkc[t], h->off[t], h->off[t + 1] - h->off[t]);
    else add(0, nrows, 0, h->P);
    if (items.size() > 0xFFFFFFFFull) { set_error("dbtk_assoc_scan: too many work items"); return DBTK_ERR_ARG; }
    const bool want_hits = p_threshold >= 0.0;
    const uint64_t neff = h->n - h->q;  // with covariates every test has n - 2 - q degrees of freedom: the closed forms take n - q for n
    const double r2crit = want_hits ? dbtk_assoc_host::r2_threshold(p_threshold, neff) : 2.0;
    DEVCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    std::vector<AsCand> cand(ncand);
    unsigned long long nhits = 0;
    h->ms[0] = 0;
    if (!items.empty()) {
        { const dbtk_status_t st = regrow(h->d_items, items.size(), "association work items"); if (st) return st; }
        { const dbtk_status_t st = regrow(h->d_cand, ncand, "association candidates"); if (st) return st; }
        DEVCHK(hipMemcpyAsync(h->d_items, items.data(), items.size() * sizeof(AsItem), hipMemcpyHostToDevice, s));
        DEVCHK(hipMemsetAsync(h->d_nhits, 0, 8, s));
        AsArgs a;
        a.G = d_rows; a.ns = h->ns; a.n = (uint32_t)h->n; a.sidx = h->d_sidx; a.yc = h->d_yc; a.syy = h->q ? h->d_syyr.get() : h->d_syy.get();
        a.q = (uint32_t)h->q; a.Q = h->d_Q; a.bt = h->d_bt;
        a.items = h->d_items; a.nitems = (uint32_t)items.size(); a.ph_idx = h->pairs ? h->d_idx.get() : nullptr; a.cand = h->d_cand;
        a.hits = h->d_hits; a.nhits = h->d_nhits; a.hit_cap = h->hit_cap; a.r2crit = r2crit;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(items.size(), AS_GRID);
        DEVCHK(hipEventRecord(h->ev[0], s));
        if (h->q) {
            if (h->ident) hipLaunchKernelGGL((k_assoc_scan<true, true>), dim3(grid), dim3(AS_WAVES * 64), 0, s, a);
            else hipLaunchKernelGGL((k_assoc_scan<false, true>), dim3(grid), dim3(AS_WAVES * 64), 0, s, a);
        } else if (h->ident) hipLaunchKernelGGL((k_assoc_scan<true, false>), dim3(grid), dim3(AS_WAVES * 64), 0, s, a);
        else hipLaunchKernelGGL((k_assoc_scan<false, false>), dim3(grid), dim3(AS_WAVES * 64), 0, s, a);
        DEVCHK(hipGetLastError());
        DEVCHK(hipEventRecord(h->ev[1], s));
        DEVCHK(hipMemcpyAsync(cand.data(), h->d_cand, ncand * sizeof(AsCand), hipMemcpyDeviceToHost, s));
        DEVCHK(hipMemcpyAsync(&nhits, h->d_nhits, 8, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
        float ms = 0;
        DEVCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->ms[0] = ms;
    }
    const auto t0 = std::chrono::steady_clock::now();
    // the fold: the items in row order, a strict > keeps the lower row on a tie
    struct Acc { uint64_t tested = 0, skipped = 0; uint32_t row = DBTK_ASSOC_NONE; double r = 0; };
    std::vector<Acc> acc(h->P);
    for (const AsItem& it : items)
        for (uint32_t c = 0; c < it.ph_n; ++c) {
            const AsCand& k = cand[it.cand_off + c];
            Acc& b = acc[h->pairs ? h->idx[it.ph_off + c] : c];
            b.tested += k.tested; b.skipped += k.skipped;
            if (k.row != DBTK_ASSOC_NONE && (b.row == DBTK_ASSOC_NONE || k.r * k.r > b.r * b.r)) { b.row = k.row; b.r = k.r; }
        }
    h->best.assign(h->P, dbtk_assoc_best_t{});
    std::vector<double> pb;
    std::vector<uint64_t> who;
    const double df = (double)(neff - 2);
    for (uint64_t p = 0; p < h->P; ++p) {
        dbtk_assoc_best_t& o = h->best[p];
        o.n_tests = acc[p].tested; o.skipped = acc[p].skipped; o.row = DBTK_ASSOC_NONE; o.locus = DBTK_ASSOC_NONE;
        if (!o.n_tests) continue;
        o.row = acc[p].row; o.locus = locus_of(nkc, o.row); o.r = acc[p].r;
        o.se = sqrt((1.0 - o.r * o.r) / df);
        o.t = o.r / o.se;
        o.p = dbtk_assoc_host::pvalue(o.r, neff);
        o.p_bonf = o.p * (double)o.n_tests;
        pb.push_back(o.p_bonf); who.push_back(p);
    }
    std::vector<double> q(pb.size());
    dbtk_assoc_host::bh(pb.data(), pb.size(), q.data());
    for (size_t i = 0; i < who.size(); ++i) h->best[who[i]].q = q[i];
    h->hits.clear();
    h->with_hits = want_hits;
    dbtk_status_t st = DBTK_OK;
    if (want_hits && nhits > h->hit_cap) {
        set_error("dbtk_assoc_scan: " + std::to_string(nhits) + " hits, the buffer holds DBTK_ASSOC_HITS = " + std::to_string(h->hit_cap) + ": set it to a power of two >= " + std::to_string(nhits));
        h->with_hits = false;
        st = DBTK_ERR_OVERFLOW;
    } else if (want_hits && nhits) {
        std::vector<AsHit> raw(nhits);
        DEVCHK(hipMemcpy(raw.data(), h->d_hits, nhits * sizeof(AsHit), hipMemcpyDeviceToHost));
        std::sort(raw.begin(), raw.end(), [](const AsHit& a, const AsHit& b) { return a.ph != b.ph ? a.ph < b.ph : a.row < b.row; });
        h->hits.resize(nhits);
        for (uint64_t i = 0; i < nhits; ++i) {
            dbtk_assoc_hit_t& o = h->hits[i];
            o.pheno = raw[i].ph; o.row = raw[i].row; o.locus = locus_of(nkc, o.row); o.pad = 0; o.r = raw[i].r;
            o.t = o.r / sqrt((1.0 - o.r * o.r) / df);
            o.p = dbtk_assoc_host::pvalue(o.r, neff);
        }
    }
    h->ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->items.swap(items);
    h->scanned = true;
    return st;
}

dbtk_status_t assoc_covar_set_impl(dbtk_assoc_t* h, uint64_t q, const double* covar, const char* const* names) {
    if (!h) { set_error("null argument"); return DBTK_ERR_ARG; }
    h->scanned = false; h->perm_done = false;
    if (!q) {
        DEVCHK(hipSetDevice(h->device));
        DEVCHK(hipStreamSynchronize(h->stream));
        h->d_Q.drop(); h->d_bt.drop(); h->d_syyr.drop();
        h->q = 0;
        return DBTK_OK;
    }
    if (!covar) { set_error("null argument"); return DBTK_ERR_ARG; }
    const uint64_t n = h->n, P = h->P;
    if (q > DBTK_ASSOC_COVAR_MAX) { set_error("dbtk_assoc_covar_set: " + std::to_string(q) + " covariates: at most DBTK_ASSOC_COVAR_MAX = " + std::to_string(DBTK_ASSOC_COVAR_MAX)); return DBTK_ERR_ARG; }
    if (n < q + 3) {
        set_error("dbtk_assoc_covar_set: " + std::to_string(n) + " samples and " + std::to_string(q) + " covariates: a test needs at least q + 3 samples (n - 2 - q degrees of freedom)");
        return DBTK_ERR_ARG;
    }
    auto name = [&](uint64_t j) { return names && names[j] ? std::string(names[j]) : "c" + std::to_string(j); };
    std::vector<double> c(q * n), Q(q * n);  // the samples in ascending order, as the phenotypes lie on the device
    for (uint64_t j = 0; j < q; ++j)
        for (uint64_t i = 0; i < n; ++i) c[j * n + i] = covar[j * n + h->ord[i]];
    uint64_t bad = 0;
    bool finite = true;
    if (!dbtk_assoc_host::covar_basis(n, q, c.data(), Q.data(), &bad, &finite)) {
        set_error("dbtk_assoc_covar_set: covariate " + name(bad) + (finite ? " is constant or collinear with the intercept and the covariates in front of it" : " has a value that is not finite"));
        return DBTK_ERR_ARG;
    }
    DEVCHK(hipSetDevice(h->device));
    DevArr<double> dQ, dbt, dsy;
    const std::string what = "covariate tables (basis 8 * q * n = " + std::to_string(8 * q * n) + " bytes, projections 8 * P * q = " + std::to_string(8 * P * q) + " bytes)";
    { const dbtk_status_t st = regrow(dQ, q * n, what.c_str()); if (st) return st; }
    { const dbtk_status_t st = regrow(dbt, P * q, what.c_str()); if (st) return st; }
    { const dbtk_status_t st = regrow(dsy, P, what.c_str()); if (st) return st; }
    std::vector<double> syy(P), left(P);
    DEVCHK(hipMemcpyAsync(dQ, Q.data(), q * n * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_assoc_covar_pheno, dim3((uint32_t)P), dim3(64), 0, h->stream, h->d_yc.get(), h->d_syy.get(), dQ.get(), dbt.get(), dsy.get(), (uint32_t)n, (uint32_t)q);
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpyAsync(syy.data(), h->d_syy, P * 8, hipMemcpyDeviceToHost, h->stream));
    DEVCHK(hipMemcpyAsync(left.data(), dsy, P * 8, hipMemcpyDeviceToHost, h->stream));
    DEVCHK(hipStreamSynchronize(h->stream));
    for (uint64_t p = 0; p < P; ++p)
        if (!(left[p] > DBTK_ASSOC_COVAR_COLLINEAR * syy[p])) {
            char share[32];
            snprintf(share, sizeof share, "%.3g", left[p] / syy[p]);
            set_error("dbtk_assoc_covar_set: phenotype " + h->names[p] + " is explained by the covariates: they leave " + share + " of its sum of squares, a test needs more than DBTK_ASSOC_COVAR_COLLINEAR = 1e-6");
            return DBTK_ERR_ARG;
        }
    h->d_Q = std::move(dQ); h->d_bt = std::move(dbt); h->d_syyr = std::move(dsy);
    h->q = q;
    return DBTK_OK;
}

dbtk_status_t assoc_write_impl(dbtk_assoc_t* h, const char* out_prefix) {
    if (!h || !out_prefix) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!h->scanned) { set_error("dbtk_assoc_write: no scan was made"); return DBTK_ERR_ARG; }
    auto num = [](uint32_t v) { return v == DBTK_ASSOC_NONE ? std::string("NA") : std::to_string(v); };
    {
        const std::string fn = std::string(out_prefix) + ".assoc.best.tsv";
        FILE* f = fopen(fn.c_str(), "w");
        if (!f) { set_error("cannot create " + fn); return DBTK_ERR_IO; }
        fprintf(f, "pheno\tn_tests\tskipped\tlocus\trow\tr\tse\tt\tp\tp_bonf\tq\n");
        for (uint64_t p = 0; p < h->P; ++p) {
            const dbtk_assoc_best_t& o = h->best[p];
            fprintf(f, "%s\t%llu\t%llu\t", h->names[p].c_str(), (unsigned long long)o.n_tests, (unsigned long long)o.skipped);
            if (!o.n_tests) fprintf(f, "NA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n");
            else fprintf(f, "%s\t%u\t%.6e\t%.6e\t%.6e\t%.6e\t%.6e\t%.6e\n", num(o.locus).c_str(), o.row, o.r, o.se, o.t, o.p, o.p_bonf, o.q);
        }
        if (fclose(f)) { set_error("write error on " + fn); return DBTK_ERR_IO; }
    }
    if (h->with_hits) {
        const std::string fn = std::string(out_prefix) + ".assoc.hits.tsv";
        FILE* f = fopen(fn.c_str(), "w");
        if (!f) { set_error("cannot create " + fn); return DBTK_ERR_IO; }
        fprintf(f, "pheno\tlocus\trow\tr\tt\tp\n");
        for (const dbtk_assoc_hit_t& o : h->hits) fprintf(f, "%s\t%s\t%u\t%.6e\t%.6e\t%.6e\n", h->names[o.pheno].c_str(), num(o.locus).c_str(), o.row, o.r, o.t, o.p);
        if (fclose(f)) { set_error("write error on " + fn); return DBTK_ERR_IO; }
    }
    return DBTK_OK;
}

}  // namespace

extern "C" {

uint32_t dbtk_assoc_api_version(void) { return DBTK_ASSOC_API_VERSION; }

void dbtk_assoc_free(dbtk_assoc_t* h) {
    if (!h) return;
    if (h->stream || h->d_yc) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

dbtk_status_t dbtk_assoc_create(int device_id, uint64_t ns, uint64_t P, uint64_t n, const uint64_t* sample_of, const double* pheno, const char* const* names,
                                dbtk_assoc_t** out) {
    return guarded([&] { return assoc_create_impl(device_id, ns, P, n, sample_of, pheno, names, out); });
}
dbtk_status_t dbtk_assoc_set_pairs(dbtk_assoc_t* h, uint64_t ntr, const uint64_t* off, const uint32_t* pheno_idx) {
    return guarded([&] { return assoc_set_pairs_impl(h, ntr, off, pheno_idx); });
}
dbtk_status_t dbtk_assoc_scan_device(dbtk_assoc_t* h, const float* d_rows, uint64_t nrows, uint64_t ntr, const uint32_t* nk_cum, double p_threshold) {
    return guarded([&] { return assoc_scan_impl(h, d_rows, nrows, ntr, nk_cum, p_threshold); });
}
static dbtk_status_t scan_view(dbtk_assoc_t* h, const RowsView& v, const char* whose, double p_threshold) {
    if (v.device != h->device) { set_error(std::string("dbtk_assoc_scan: ") + whose + " is on device " + std::to_string(v.device) + ", the phenotypes on device " + std::to_string(h->device)); return DBTK_ERR_ARG; }
    if (v.ns != h->ns) { set_error(std::string("dbtk_assoc_scan: ") + whose + " holds " + std::to_string(v.ns) + " samples, the phenotype table was made for " + std::to_string(h->ns)); return DBTK_ERR_ARG; }
    return assoc_scan_impl(h, v.d_rows, v.nrows, v.ntr, v.nk_cum.data(), p_threshold);
}
dbtk_status_t dbtk_assoc_scan_pred(dbtk_assoc_t* h, dbtk_pred_t* pred, double p_threshold) {
    return guarded([&]() -> dbtk_status_t {
        if (!h || !pred) { set_error("null argument"); return DBTK_ERR_ARG; }
        RowsView v;
        { const dbtk_status_t st = pred_rows(pred, &v); if (st) return st; }
        return scan_view(h, v, "the genotype matrix", p_threshold);
    });
}
dbtk_status_t dbtk_assoc_scan_dosage(dbtk_assoc_t* h, dbtk_dosage_t* dosage, double p_threshold) {
    return guarded([&]() -> dbtk_status_t {
        if (!h || !dosage) { set_error("null argument"); return DBTK_ERR_ARG; }
        RowsView v;
        { const dbtk_status_t st = dosage_rows(dosage, &v); if (st) return st; }
        return scan_view(h, v, "the dosage table", p_threshold);
    });
}
dbtk_status_t dbtk_assoc_best(dbtk_assoc_t* h, dbtk_assoc_best_t* out) {
    if (!h || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!h->scanned) { set_error("dbtk_assoc_best: no scan was made"); return DBTK_ERR_ARG; }
    std::copy(h->best.begin(), h->best.end(), out);
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_hits(dbtk_assoc_t* h, dbtk_assoc_hit_t* out, uint64_t cap, uint64_t* n) {
    if (!h || !n || (cap && !out)) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!h->scanned || !h->with_hits) { set_error("dbtk_assoc_hits: no scan with a threshold was made (or its hit list overflowed)"); return DBTK_ERR_ARG; }
    *n = h->hits.size();
    std::copy(h->hits.begin(), h->hits.begin() + std::min<uint64_t>(cap, h->hits.size()), out);
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_write(dbtk_assoc_t* h, const char* out_prefix) {
    return guarded([&] { return assoc_write_impl(h, out_prefix); });
}
dbtk_status_t dbtk_assoc_times(dbtk_assoc_t* h, double ms[2]) {
    if (!h || !ms) { set_error("null argument"); return DBTK_ERR_ARG; }
    ms[0] = h->ms[0]; ms[1] = h->ms[1];
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_pvalue(double r, uint64_t n, double* p) {
    if (!p) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (n < 3 || !(fabs(r) <= 1.0)) { set_error("dbtk_assoc_pvalue: n >= 3 and |r| <= 1"); return DBTK_ERR_ARG; }
    *p = dbtk_assoc_host::pvalue(r, n);
    return DBTK_OK;
}
uint32_t dbtk_assoc_covar_api_version(void) { return DBTK_ASSOC_COVAR_API_VERSION; }
dbtk_status_t dbtk_assoc_covar_basis(uint64_t n, uint64_t q, const double* covar, double* Q, uint64_t* bad_column) {
    if (!bad_column || (q && n && (!covar || !Q))) { set_error("null argument"); return DBTK_ERR_ARG; }
    return guarded([&]() -> dbtk_status_t {
        bool finite = true;
        if (dbtk_assoc_host::covar_basis(n, q, covar, Q, bad_column, &finite)) return DBTK_OK;
        set_error("dbtk_assoc_covar_basis: column " + std::to_string(*bad_column) + (finite ? " is constant or collinear with the intercept and the columns in front of it" : " has a value that is not finite"));
        return DBTK_ERR_ARG;
    });
}
dbtk_status_t dbtk_assoc_covar_set(dbtk_assoc_t* h, uint64_t q, const double* covar, const char* const* names) {
    return guarded([&] { return assoc_covar_set_impl(h, q, covar, names); });
}
dbtk_status_t dbtk_assoc_covar_get(const dbtk_assoc_t* h, uint64_t* q, uint64_t* dof) {
    if (!h || !q || !dof) { set_error("null argument"); return DBTK_ERR_ARG; }
    *q = h->q; *dof = h->n - 2 - h->q;
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_bh(const double* p, uint64_t m, double* q) {
    if (m && (!p || !q)) { set_error("null argument"); return DBTK_ERR_ARG; }
    return guarded([&] { dbtk_assoc_host::bh(p, m, q); return DBTK_OK; });
}
dbtk_status_t dbtk_assoc_r2_threshold(double p_threshold, uint64_t n, double* r2) {
    if (!r2) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (n < 3 || std::isnan(p_threshold)) { set_error("dbtk_assoc_r2_threshold: n >= 3 and a threshold that is a number"); return DBTK_ERR_ARG; }
    *r2 = dbtk_assoc_host::r2_threshold(p_threshold, n);
    return DBTK_OK;
}

}  // extern "C"

#include "dbtk_assoc_perm_dev.h"  // the permutation pass: dbtk_assoc_perm_*
