// dbtk_assoc_perm_dev.h — the device side of the permutation p-values (include/dbtk_assoc_perm.h): the residuals of the phenotypes, the
// permutation kernel, and the entry points.  Included by dbtk_assoc.hip behind the scan: it shares the scan's work items, its row
// statistics and its summation tree, and the handle.
#ifndef DBTK_ASSOC_PERM_DEV_H_
#define DBTK_ASSOC_PERM_DEV_H_

#include "../../include/dbtk_assoc_perm.h"
#include "dbtk_assoc_perm_host.h"

namespace {

// ---- the shape of the permutation pass (DESIGN.md 7.3 "Permutations" has the table; tests/test_assoc_perm_gpu.py crosses every one)
constexpr uint32_t PM_CHUNK = 8;   // columns, that is (phenotype, permutation) pairs, staged in LDS at a time
constexpr uint32_t PM_BUF = 2;     // staging buffers: the gather of the next step is in flight while this one is multiplied
static_assert(PM_CHUNK == AS_CHUNK && AS_TILE * PM_CHUNK == AS_ACC, "as_reduce sums AS_TILE x PM_CHUNK accumulators");
static_assert(DBTK_ASSOC_PERM_MAX == dbtk_assoc_host::PERM_MAX, "one cap");

struct PmArgs {
    AsArgs s;                // what the scan read; yc holds the residuals of the phenotypes when there are covariates, bt is not read
    const uint32_t* perm;    // [B + 1][n]; row 0 is the identity
    unsigned long long* T;   // [P][B + 1] the maxima as the bit patterns of non-negative doubles, zeroed before the launch
    uint32_t B1;             // B + 1 columns per phenotype
};

// One block per phenotype: yres[p] = yc[p] - sum_j bt[p][j] Q[j], j ascending by fma.
__global__ void __launch_bounds__(256) k_assoc_perm_resid(const double* __restrict__ yc, const double* __restrict__ Q, const double* __restrict__ bt,
                                                          double* __restrict__ yres, uint32_t n, uint32_t q) {
    const uint64_t p = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        double v = yc[p * n + i];
        for (uint32_t j = 0; j < q; ++j) v = fma(-bt[p * q + j], Q[(uint64_t)j * n + i], v);
        yres[p * n + i] = v;
    }
}

// the centred (COVAR: residualised) samples seg0 + lane + 64 i of the wave's AS_TILE rows as float64; the slots behind the segment's are
// not touched, and a slot past the mask's end meets a staged 0
template <bool IDENT, bool COVAR>
__device__ __forceinline__ void pm_make_dx(const AsArgs& a, const uint64_t (&base)[AS_TILE], uint32_t seg0, uint32_t lane, uint32_t w, const double (&mu)[AS_TILE],
                                           const double (*aj)[AS_ROWS], double (&dx)[AS_TILE][AS_REG]) {
    const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
    for (uint32_t i = 0; i < AS_REG; ++i) {  // (as_load's addresses and zeros, a slot at a time: the float32 tile is never whole in registers beside dx)
        if (i >= ni) break;
        const uint32_t j = seg0 + lane + 64 * i;
        const bool in = j < a.n;
        const uint32_t s = in ? (IDENT ? j : a.sidx[j]) : 0u;
#pragma unroll
        for (uint32_t t = 0; t < AS_TILE; ++t) dx[t][i] = (double)(in ? a.G[base[t] + s] : 0.f) - mu[t];
    }
    if constexpr (COVAR) {
#pragma unroll
        for (uint32_t i = 0; i < AS_REG; ++i) {  // (a slot at a time, j inside: Q's values do not pile up in registers beside the accumulators)
            if (i >= ni) break;
            const uint32_t at = seg0 + lane + 64 * i;
            const double* c = a.Q + (at < a.n ? at : 0u);
            const double keep = at < a.n ? 1.0 : 0.0;
            for (uint32_t j = 0; j < a.q; ++j) {
                const double qv = keep * c[(uint64_t)j * a.n];
#pragma unroll
                for (uint32_t t = 0; t < AS_TILE; ++t) dx[t][i] = fma(-aj[j][w * AS_TILE + t], qv, dx[t][i]);
            }
        }
    }
}

// The scan's work items and its passes of AS_ROWS rows, AS_TILE rows per wave; a COLUMN is a (phenotype of the item, b) pair, b = 0 .. B,
// column phslot * (B + 1) + b.  Per pass the row statistics are made exactly as k_assoc_scan makes them (the same tested rows, the same
// Sxx and, with COVAR, the same a_j and Sxx'); then the row tile is centred, with COVAR residualised explicitly (x~ = dx - sum a_j Q_j),
// and held as float64 in registers for all columns while n <= AS_SEG (above that it is made again for every segment).  PM_CHUNK columns at
// a time, all of one phenotype, a thread per sample gathers y[pi_b[i]] (the identity is row 0 of the table: slot 0 takes the same path) into one of two LDS
// buffers while the waves multiply the other: one barrier per step.  as_reduce sums the AS_TILE x PM_CHUNK accumulators in the scan's tree,
// a lane per (row, column) makes r^2, two shuffles take the maximum over the wave's rows, the waves' maxima meet in LDS and thread c
// folds them into T with one integer atomic max per pass and column.  No floating-point atomic, no sum whose order depends on anything
// but n.
// RES: n <= AS_SEG, an instance of its own, so that the resident loop carries nothing of the other one's row addresses and means.
template <bool IDENT, bool COVAR, bool RES>
__global__ void __launch_bounds__(AS_WAVES * 64) k_assoc_perm(const PmArgs pa) {
    __shared__ double zl[PM_BUF][PM_CHUNK][AS_SEG];
    __shared__ double aj[COVAR ? AS_COVAR_MAX : 1][AS_ROWS];
    __shared__ double wmax[2][AS_WAVES][PM_CHUNK];
    const AsArgs& a = pa.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    constexpr bool resident = RES;
    const uint32_t nseg = RES ? 1u : (a.n + AS_SEG - 1) / AS_SEG, B1 = pa.B1;
    const double dn = (double)a.n;
    for (uint32_t q = blockIdx.x; q < a.nitems; q += gridDim.x) {  // (the same trips for every thread: the barriers are uniform)
        const AsItem it = a.items[q];
        // a chunk holds columns of ONE phenotype, cpp chunks each: its phenotype is uniform (the host refuses a product past 2^32)
        const uint32_t cpp = (B1 + PM_CHUNK - 1) / PM_CHUNK, nchunk = it.ph_n * cpp;
        auto pheno_of = [&](uint32_t ps) -> uint32_t { return __builtin_amdgcn_readfirstlane(a.ph_idx ? a.ph_idx[it.ph_off + ps] : ps); };
        // thread c < PM_CHUNK folds column b0 + c of phenotype ph: the waves' maxima of this pass (buffer par) into T
        auto flush = [&](uint32_t par, uint32_t ph, uint32_t b0) {
            if (tid >= PM_CHUNK || b0 + tid >= B1) return;
            double m = 0.0;
            for (uint32_t ww = 0; ww < AS_WAVES; ++ww) m = fmax(m, wmax[par][ww][tid]);
            if (!(m > 0.0)) return;  // (T starts at 0)
            atomicMax(&pa.T[(uint64_t)ph * B1 + b0 + tid], (unsigned long long)__double_as_longlong(m));
        };
        for (uint32_t sub = 0; sub < it.nrows; sub += AS_ROWS) {
            __syncthreads();  // the pass before is done with zl, aj and wmax
            uint32_t ln = lane;  // the lane for the row statistics: what they derive from it (the samples' columns, the addresses in Q) is made
            asm volatile("" : "+v"(ln));  // again in every pass and does not sit in registers through the column loop
            uint64_t base[AS_TILE];
            bool on[AS_TILE], tested[AS_TILE];
#pragma unroll
            for (uint32_t t = 0; t < AS_TILE; ++t) {
                const uint32_t k = sub + w * AS_TILE + t;
                on[t] = k < it.nrows;
                base[t] = (uint64_t)(it.row0 + (on[t] ? k : it.nrows - 1)) * a.ns;  // (a row off the item reads the item's last row and is ignored)
            }
            double mu[AS_TILE], sxx[AS_TILE];
            {   // the statistics of the rows, statement for statement those of k_assoc_scan
                float x[AS_TILE][AS_REG];
                double sum[AS_TILE];
                float mn[AS_TILE], mx[AS_TILE];
                bool fin[AS_TILE];
#pragma unroll
                for (uint32_t t = 0; t < AS_TILE; ++t) { sum[t] = 0.0; mn[t] = INFINITY; mx[t] = -INFINITY; fin[t] = true; }
                for (uint32_t seg0 = 0; seg0 < a.n; seg0 += AS_SEG) {
                    as_load<IDENT>(a, base, seg0, ln, x);
                    const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
                    for (uint32_t i = 0; i < AS_REG; ++i) {
                        if (i >= ni) break;
                        const bool in = seg0 + ln + 64 * i < a.n;
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
                for (uint32_t seg0 = 0; seg0 < a.n; seg0 += AS_SEG) {
                    if (!resident) as_load<IDENT>(a, base, seg0, ln, x);
                    const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
                    for (uint32_t i = 0; i < AS_REG; ++i) {
                        if (i >= ni) break;
                        const bool in = seg0 + ln + 64 * i < a.n;
#pragma unroll
                        for (uint32_t t = 0; t < AS_TILE; ++t) {
                            const double d = in ? (double)x[t][i] - mu[t] : 0.0;
                            sxx[t] = fma(d, d, sxx[t]);
                        }
                    }
                }
#pragma unroll
                for (uint32_t t = 0; t < AS_TILE; ++t) sxx[t] = as_wave_sum(sxx[t]);
                if constexpr (COVAR) {
                    // a_j = sum dx Q_j in the scan's order (a lane's samples ascending by fma, the wave by the tree), Sxx' = Sxx - sum a_j^2
                    double left[AS_TILE];
#pragma unroll
                    for (uint32_t t = 0; t < AS_TILE; ++t) left[t] = sxx[t];
                    for (uint32_t j = 0; j < a.q; ++j) {
                        double s[AS_TILE];
#pragma unroll
                        for (uint32_t t = 0; t < AS_TILE; ++t) s[t] = 0.0;
                        for (uint32_t seg0 = 0; seg0 < a.n; seg0 += AS_SEG) {
                            if (!resident) as_load<IDENT>(a, base, seg0, ln, x);
                            const uint32_t ni = as_slots(a.n, seg0);
#pragma unroll
                            for (uint32_t i = 0; i < AS_REG; ++i) {
                                if (i >= ni) break;
                                const uint32_t at = seg0 + ln + 64 * i;
                                const double z = at < a.n ? a.Q[(uint64_t)j * a.n + at] : 0.0;
#pragma unroll
                                for (uint32_t t = 0; t < AS_TILE; ++t) s[t] = fma((double)x[t][i] - mu[t], z, s[t]);
                            }
                        }
#pragma unroll
                        for (uint32_t t = 0; t < AS_TILE; ++t) {
                            const double v = as_wave_sum(s[t]);
                            left[t] = fma(-v, v, left[t]);
                            if (lane == t) aj[j][w * AS_TILE + t] = v;
                        }
                    }
#pragma unroll
                    for (uint32_t t = 0; t < AS_TILE; ++t) {
                        tested[t] = tested[t] && left[t] > AS_COLLINEAR * sxx[t];
                        sxx[t] = left[t];
                    }
                    __syncthreads();  // the a_j are in LDS (each wave reads its own rows only)
                }
            }
            double dx[AS_TILE][AS_REG];
            if (resident) pm_make_dx<IDENT, COVAR>(a, base, 0u, ln, w, mu, aj, dx);
            // thread tid gathers sample sg * AS_SEG + tid of the columns b0 .. b0 + PM_CHUNK - 1 of phenotype ph: the indices, then the values
            // (every address is inside the tables, so that no load waits behind a branch; what is past an end becomes 0 and adds nothing)
            double v[PM_CHUNK];
            uint32_t tg = tid;
            asm volatile("" : "+v"(tg));  // (as ln: the first gather's addresses are the same in every pass and would be kept for all of them)
            auto gather = [&](uint32_t ph, uint32_t b0, uint32_t sg) {
                const uint32_t at = sg * AS_SEG + tg, atc = min(at, a.n - 1u);
                const double* y = a.yc + (uint64_t)ph * a.n;
                uint32_t ix[PM_CHUNK];
#pragma unroll
                for (uint32_t c = 0; c < PM_CHUNK; ++c) ix[c] = pa.perm[(uint64_t)min(b0 + c, B1 - 1u) * a.n + atc];
#pragma unroll
                for (uint32_t c = 0; c < PM_CHUNK; ++c) {
                    const double val = y[ix[c]];
                    v[c] = at < a.n && b0 + c < B1 ? val : 0.0;
                }
            };
            uint32_t ps = 0, kb = 0, ph = pheno_of(0u);  // this chunk: the phenotype's slot in the item's list, the chunk within it, the phenotype
            gather(ph, 0u, 0u);
#pragma unroll
            for (uint32_t c = 0; c < PM_CHUNK; ++c) zl[0][c][tid] = v[c];
            uint32_t step = 0, ph_before = 0, b0_before = 0;
            for (uint32_t k = 0; k < nchunk; ++k) {
                uint32_t nkb = kb + 1, nps = ps, nph = ph;  // the chunk after this one
                if (nkb == cpp) { nkb = 0; ++nps; if (nps < it.ph_n) nph = pheno_of(nps); }
                double acc[AS_ACC];
#pragma unroll
                for (uint32_t e = 0; e < AS_ACC; ++e) acc[e] = 0.0;
                for (uint32_t sg = 0; sg < nseg; ++sg, ++step) {
                    __syncthreads();  // this step's columns are staged, and everyone has read the other buffer (and written the chunk before's maxima)
                    if (sg == 0 && k) flush((k - 1) & 1u, ph_before, b0_before);
                    const bool last = sg + 1 == nseg, more = !last || nps < it.ph_n;
                    if (more) gather(last ? nph : ph, (last ? nkb : kb) * PM_CHUNK, last ? 0u : sg + 1);  // in flight during the multiply-adds
                    const uint32_t seg0 = sg * AS_SEG;
                    if constexpr (!RES) {  // the rows' segment is in flight beside the gather; the gathered values do not wait in registers
                        if (more) {
#pragma unroll
                            for (uint32_t c = 0; c < PM_CHUNK; ++c) zl[(step + 1) & 1u][c][tid] = v[c];
                        }
                        asm volatile("" : "+v"(ln));
                        pm_make_dx<IDENT, COVAR>(a, base, seg0, ln, w, mu, aj, dx);
                    }
                    const uint32_t ni = as_slots(a.n, seg0);
                    const double (*z)[AS_SEG] = zl[step & 1u];
#pragma unroll
                    for (uint32_t i = 0; i < AS_REG; ++i) {
                        if (i >= ni) break;
#pragma unroll
                        for (uint32_t c = 0; c < PM_CHUNK; ++c) {
                            const double zv = z[c][lane + 64 * i];
#pragma unroll
                            for (uint32_t t = 0; t < AS_TILE; ++t) acc[t * PM_CHUNK + c] = fma(dx[t][i], zv, acc[t * PM_CHUNK + c]);
                        }
                    }
                    if (RES && more) {
#pragma unroll
                        for (uint32_t c = 0; c < PM_CHUNK; ++c) zl[(step + 1) & 1u][c][tid] = v[c];
                    }
                }
                const double sxy = as_reduce(acc, lane);
                const uint32_t e = lane >> 1, t = e / PM_CHUNK, c = e % PM_CHUNK;
                const double sx = t == 0 ? sxx[0] : t == 1 ? sxx[1] : t == 2 ? sxx[2] : sxx[3];
                const bool tt = t == 0 ? tested[0] : t == 1 ? tested[1] : t == 2 ? tested[2] : tested[3];
                double r2 = 0.0;
                if (tt && kb * PM_CHUNK + c < B1) {
                    double r = sxy / sqrt(sx * a.syy[ph]);
                    r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
                    r2 = r * r;
                    r2 = r2 >= 0.0 ? r2 : 0.0;  // (not a number: no statistic)
                }
                r2 = fmax(r2, __shfl_xor(r2, 16));  // the wave's AS_TILE rows of a column sit 16 lanes apart
                r2 = fmax(r2, __shfl_xor(r2, 32));
                if (lane < 2 * PM_CHUNK && !(lane & 1u)) wmax[k & 1u][w][c] = r2;
                ph_before = ph; b0_before = kb * PM_CHUNK;
                kb = nkb; ps = nps; ph = nph;
            }
            __syncthreads();
            flush((nchunk - 1) & 1u, ph_before, b0_before);
        }
    }
}

template <class T> dbtk_status_t perm_regrow(DevArr<T>& a, uint64_t need, const std::string& what) { return regrow(a, need, what.c_str()); }

dbtk_status_t assoc_perm_set_impl(dbtk_assoc_t* h, uint64_t B, const uint32_t* perm) {
    if (!h) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!B) {
        DEVCHK(hipSetDevice(h->device));
        DEVCHK(hipStreamSynchronize(h->stream));
        h->perm_done = false;
        h->d_perm.drop(); h->d_T.drop(); h->d_yres.drop();
        h->B = 0; h->perm.clear(); h->T.clear();
        return DBTK_OK;
    }
    if (!perm) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (B > DBTK_ASSOC_PERM_MAX) { set_error("dbtk_assoc_perm_set: " + std::to_string(B) + " permutations: at most DBTK_ASSOC_PERM_MAX = " + std::to_string(DBTK_ASSOC_PERM_MAX)); return DBTK_ERR_ARG; }
    const uint64_t n = h->n, P = h->P;
    uint64_t bad = 0;
    if (!dbtk_assoc_host::perm_valid(n, B, perm, &bad)) {
        set_error("dbtk_assoc_perm_set: row " + std::to_string(bad) + " is not a permutation of 0 .. " + std::to_string(n - 1));
        return DBTK_ERR_ARG;
    }
    DEVCHK(hipSetDevice(h->device));
    const uint64_t table = 4 * (B + 1) * n, maxima = 8 * P * (B + 1);
    size_t fr = 0, tot = 0;
    DEVCHK(hipMemGetInfo(&fr, &tot));
    const std::string what = "permutation tables (table 4 * (B + 1) * n = " + std::to_string(table) + " bytes, maxima 8 * P * (B + 1) = " + std::to_string(maxima) + " bytes)";
    if (table + maxima > fr) {
        set_error(what + " do not fit, " + std::to_string(fr) + " of " + std::to_string(tot) + " bytes of HBM are free");
        return DBTK_ERR_NOMEM;
    }
    std::vector<uint32_t> tab((B + 1) * n);  // the identity in front: slot 0 takes the path of every other slot
    for (uint64_t i = 0; i < n; ++i) tab[i] = (uint32_t)i;
    std::copy(perm, perm + B * n, tab.begin() + n);
    DevArr<uint32_t> d_perm;  // (made whole before the handle sees them: a failure leaves the old permutations as they were)
    DevArr<unsigned long long> d_T;
    { const dbtk_status_t st = perm_regrow(d_perm, tab.size(), what); if (st) return st; }
    { const dbtk_status_t st = perm_regrow(d_T, P * (B + 1), what); if (st) return st; }
    for (DevEvent& e : h->pev)
        if (!e) DEVCHK(e.create(hipEventDefault));
    DEVCHK(hipStreamSynchronize(h->stream));
    DEVCHK(hipMemcpy(d_perm, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    h->perm_done = false;
    h->d_perm = std::move(d_perm); h->d_T = std::move(d_T);
    h->B = B; h->perm.assign(perm, perm + B * n); h->T.clear();
    return DBTK_OK;
}

// the permutation pass over the rows and the work items of the scan just made
dbtk_status_t assoc_perm_pass_impl(dbtk_assoc_t* h, const float* d_rows) {
    const uint64_t B1 = h->B + 1, P = h->P, n = h->n;
    for (const AsItem& it : h->items)
        if ((uint64_t)it.ph_n * (B1 + PM_CHUNK) > 0xFFFFFFFFull) {
            set_error("dbtk_assoc_perm_scan: " + std::to_string(it.ph_n) + " phenotypes of one locus times " + std::to_string(B1) + " columns pass 2^32");
            return DBTK_ERR_ARG;
        }
    DEVCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->pms[0] = 0;
    h->T.assign(P * B1, 0.0);
    if (!h->items.empty()) {
        if (h->q) {
            { const dbtk_status_t st = perm_regrow(h->d_yres, P * n, "residuals of the phenotypes"); if (st) return st; }
            hipLaunchKernelGGL(k_assoc_perm_resid, dim3((uint32_t)P), dim3(256), 0, s, h->d_yc.get(), h->d_Q.get(), h->d_bt.get(), h->d_yres.get(), (uint32_t)n, (uint32_t)h->q);
            DEVCHK(hipGetLastError());
        }
        PmArgs pa;
        AsArgs& a = pa.s;
        a.G = d_rows; a.ns = h->ns; a.n = (uint32_t)n; a.sidx = h->d_sidx; a.yc = h->q ? h->d_yres.get() : h->d_yc.get(); a.syy = h->q ? h->d_syyr.get() : h->d_syy.get();
        a.q = (uint32_t)h->q; a.Q = h->d_Q; a.bt = nullptr;
        a.items = h->d_items; a.nitems = (uint32_t)h->items.size(); a.ph_idx = h->pairs ? h->d_idx.get() : nullptr;
        a.cand = nullptr; a.hits = nullptr; a.nhits = nullptr; a.hit_cap = 0; a.r2crit = 2.0;
        pa.perm = h->d_perm; pa.T = h->d_T; pa.B1 = (uint32_t)B1;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(h->items.size(), AS_GRID);
        DEVCHK(hipMemsetAsync(h->d_T, 0, P * B1 * 8, s));
        DEVCHK(hipEventRecord(h->pev[0], s));
        void (*kern)(const PmArgs) = nullptr;
        const bool res = n <= AS_SEG;
        if (h->q) kern = h->ident ? (res ? k_assoc_perm<true, true, true> : k_assoc_perm<true, true, false>) : (res ? k_assoc_perm<false, true, true> : k_assoc_perm<false, true, false>);
        else kern = h->ident ? (res ? k_assoc_perm<true, false, true> : k_assoc_perm<true, false, false>) : (res ? k_assoc_perm<false, false, true> : k_assoc_perm<false, false, false>);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(AS_WAVES * 64), 0, s, pa);
        DEVCHK(hipGetLastError());
        DEVCHK(hipEventRecord(h->pev[1], s));
        DEVCHK(hipMemcpyAsync(h->T.data(), h->d_T, P * B1 * 8, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
        float ms = 0;
        DEVCHK(hipEventElapsedTime(&ms, h->pev[0], h->pev[1]));
        h->pms[0] = ms;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> has(P);
    std::vector<uint64_t> n_ge(P);
    std::vector<double> pp(P), qq(P);
    for (uint64_t p = 0; p < P; ++p) has[p] = h->best[p].n_tests != 0;
    dbtk_assoc_host::perm_fold(P, h->B, h->T.data(), has.data(), n_ge.data(), pp.data(), qq.data());
    h->pres.assign(P, dbtk_assoc_perm_result_t{});
    for (uint64_t p = 0; p < P; ++p) {
        dbtk_assoc_perm_result_t& o = h->pres[p];
        o.n_perm = h->B; o.n_ge = n_ge[p]; o.row = h->best[p].row; o.pad = 0;
        o.r2 = has[p] ? h->T[p * B1] : 0.0; o.p_perm = pp[p]; o.q_perm = qq[p];
    }
    h->pms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->perm_done = true;
    return DBTK_OK;
}

// scan: the twin (it refuses what it refuses and leaves the best rows, the hits and the work items in the handle)
template <class Scan> dbtk_status_t assoc_perm_scan_impl(dbtk_assoc_t* h, Scan scan) {
    if (!h) { set_error("null argument"); return DBTK_ERR_ARG; }
    h->perm_done = false;
    if (!h->B) { set_error("dbtk_assoc_perm_scan: no permutations are set (dbtk_assoc_perm_set, dbtk_assoc_perm_seed)"); return DBTK_ERR_ARG; }
    const float* d_rows = nullptr;
    const dbtk_status_t st = scan(&d_rows);
    if (st != DBTK_OK && !(st == DBTK_ERR_OVERFLOW && h->scanned)) return st;  // (a hit list that overflowed leaves the best rows whole, as in the twin)
    const std::string kept = st ? dbtk_last_error() : "";
    const dbtk_status_t ps = assoc_perm_pass_impl(h, d_rows);
    if (ps) return ps;
    if (st) set_error(kept);
    return st;
}

dbtk_status_t assoc_perm_write_impl(dbtk_assoc_t* h, const char* out_prefix) {
    if (!h || !out_prefix) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!h->perm_done) { set_error("dbtk_assoc_perm_write: no permutation scan was made"); return DBTK_ERR_ARG; }
    const std::string fn = std::string(out_prefix) + ".assoc.perm.tsv";
    FILE* f = fopen(fn.c_str(), "w");
    if (!f) { set_error("cannot create " + fn); return DBTK_ERR_IO; }
    fprintf(f, "pheno\tn_tests\trow\tr2\tn_perm\tn_ge\tp_perm\tq_perm\n");
    for (uint64_t p = 0; p < h->P; ++p) {
        const dbtk_assoc_perm_result_t& o = h->pres[p];
        const unsigned long long nt = h->best[p].n_tests;
        if (!nt) fprintf(f, "%s\t0\tNA\tNA\t%llu\tNA\tNA\tNA\n", h->names[p].c_str(), (unsigned long long)o.n_perm);
        else fprintf(f, "%s\t%llu\t%u\t%.6e\t%llu\t%llu\t%.6e\t%.6e\n", h->names[p].c_str(), nt, o.row, o.r2, (unsigned long long)o.n_perm, (unsigned long long)o.n_ge, o.p_perm, o.q_perm);
    }
    if (fclose(f)) { set_error("write error on " + fn); return DBTK_ERR_IO; }
    return DBTK_OK;
}

}  // namespace

extern "C" {

uint32_t dbtk_assoc_perm_api_version(void) { return DBTK_ASSOC_PERM_API_VERSION; }

dbtk_status_t dbtk_assoc_perm_generate(uint64_t n, uint64_t B, uint64_t seed, uint32_t* perm) {
    if (n && B && !perm) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (n > 0xFFFFFFFFull) { set_error("dbtk_assoc_perm_generate: more than 2^32 positions"); return DBTK_ERR_ARG; }
    return guarded([&] { dbtk_assoc_host::perm_generate(n, B, seed, perm); return DBTK_OK; });
}
dbtk_status_t dbtk_assoc_perm_set(dbtk_assoc_t* h, uint64_t B, const uint32_t* perm) {
    return guarded([&] { return assoc_perm_set_impl(h, B, perm); });
}
dbtk_status_t dbtk_assoc_perm_seed(dbtk_assoc_t* h, uint64_t B, uint64_t seed) {
    return guarded([&]() -> dbtk_status_t {
        if (!h) { set_error("null argument"); return DBTK_ERR_ARG; }
        if (B > DBTK_ASSOC_PERM_MAX) { set_error("dbtk_assoc_perm_seed: " + std::to_string(B) + " permutations: at most DBTK_ASSOC_PERM_MAX = " + std::to_string(DBTK_ASSOC_PERM_MAX)); return DBTK_ERR_ARG; }
        std::vector<uint32_t> perm(B * h->n + 1);
        dbtk_assoc_host::perm_generate(h->n, B, seed, perm.data());
        return assoc_perm_set_impl(h, B, perm.data());
    });
}
dbtk_status_t dbtk_assoc_perm_get(const dbtk_assoc_t* h, uint64_t* B, uint32_t* perm, uint64_t cap) {
    if (!h || !B) { set_error("null argument"); return DBTK_ERR_ARG; }
    *B = h->B;
    if (perm) std::copy(h->perm.begin(), h->perm.begin() + std::min<uint64_t>(cap, h->B) * h->n, perm);
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_perm_scan_device(dbtk_assoc_t* h, const float* d_rows, uint64_t nrows, uint64_t ntr, const uint32_t* nk_cum, double p_threshold) {
    return guarded([&] {
        return assoc_perm_scan_impl(h, [&](const float** rows) { *rows = d_rows; return assoc_scan_impl(h, d_rows, nrows, ntr, nk_cum, p_threshold); });
    });
}
dbtk_status_t dbtk_assoc_perm_scan_pred(dbtk_assoc_t* h, dbtk_pred_t* pred, double p_threshold) {
    return guarded([&]() -> dbtk_status_t {
        if (!h || !pred) { set_error("null argument"); return DBTK_ERR_ARG; }
        return assoc_perm_scan_impl(h, [&](const float** rows) -> dbtk_status_t {
            RowsView v;
            { const dbtk_status_t st = pred_rows(pred, &v); if (st) return st; }
            *rows = v.d_rows;
            return scan_view(h, v, "the genotype matrix", p_threshold);
        });
    });
}
dbtk_status_t dbtk_assoc_perm_scan_dosage(dbtk_assoc_t* h, dbtk_dosage_t* dosage, double p_threshold) {
    return guarded([&]() -> dbtk_status_t {
        if (!h || !dosage) { set_error("null argument"); return DBTK_ERR_ARG; }
        return assoc_perm_scan_impl(h, [&](const float** rows) -> dbtk_status_t {
            RowsView v;
            { const dbtk_status_t st = dosage_rows(dosage, &v); if (st) return st; }
            *rows = v.d_rows;
            return scan_view(h, v, "the dosage table", p_threshold);
        });
    });
}
dbtk_status_t dbtk_assoc_perm_results(dbtk_assoc_t* h, dbtk_assoc_perm_result_t* out) {
    if (!h || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!h->perm_done) { set_error("dbtk_assoc_perm_results: no permutation scan was made (or permutations or covariates were set after it)"); return DBTK_ERR_ARG; }
    std::copy(h->pres.begin(), h->pres.end(), out);
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_perm_stats(dbtk_assoc_t* h, uint64_t p, double* T) {
    if (!h || !T) { set_error("null argument"); return DBTK_ERR_ARG; }
    if (!h->perm_done) { set_error("dbtk_assoc_perm_stats: no permutation scan was made (or permutations or covariates were set after it)"); return DBTK_ERR_ARG; }
    if (p >= h->P) { set_error("dbtk_assoc_perm_stats: phenotype " + std::to_string(p) + " >= P = " + std::to_string(h->P)); return DBTK_ERR_ARG; }
    std::copy(h->T.begin() + p * (h->B + 1), h->T.begin() + (p + 1) * (h->B + 1), T);
    return DBTK_OK;
}
dbtk_status_t dbtk_assoc_perm_write(dbtk_assoc_t* h, const char* out_prefix) {
    return guarded([&] { return assoc_perm_write_impl(h, out_prefix); });
}
dbtk_status_t dbtk_assoc_perm_times(dbtk_assoc_t* h, double ms[2]) {
    if (!h || !ms) { set_error("null argument"); return DBTK_ERR_ARG; }
    ms[0] = h->pms[0]; ms[1] = h->pms[1];
    return DBTK_OK;
}

}  // extern "C"
#endif
