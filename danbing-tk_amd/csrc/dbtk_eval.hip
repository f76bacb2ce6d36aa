// dbtk_eval.hip — the genotype score (include/dbtk_eval.h): truth counts from the assembly, per-locus regression sums, the handle.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dbtk_eval.h"
#include "dbtk_eval.h"
#include "dbtk_dev.h"
#include "dbtk_internal.h"

using namespace dbtk;

namespace {

struct EvalTruthArgs {
    const uint8_t* arena;
    const EvalItem* items;
    uint32_t nitems, k;
    EvalTables T;
    uint64_t nk;
    uint64_t* truth;    // [nk]
    uint64_t* windows;  // [nloci]
    uint64_t* lookups;  // one word
};

// One wave per item (workgroups of one wave, taking the items round robin).  The wave packs the item's bases into LDS once, 16 per
// lane and step; then every lane takes the windows j = lane, lane + 64, ...: funnel shift out of LDS, canonical form, one probe of
// the class table in HBM, and an atomic add on the k-mer's counter where the k-mer is a TR k-mer of the item's locus.  The windows
// of the item are added up across the wave and leave in one atomic per item.
__global__ void __launch_bounds__(64) k_eval_truth(const EvalTruthArgs a) {
    __shared__ uint32_t pk[EV_WORDS];
    __shared__ uint16_t vd[EV_WORDS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < a.nitems; it += gridDim.x) {  // (the same trips for every lane: the barriers are uniform)
        const EvalItem item = a.items[it];
        const uint32_t n = item.n < EV_CH ? item.n : EV_CH;
        const uint32_t nw = eval_item_words(n, a.k);
        __syncthreads();  // the windows of the item before are done with the words
        for (uint32_t w = lane; w < nw + 2; w += 64) {
            if (w < nw) eval_stage_word(a.arena + item.off, w, pk, vd);
            else { pk[w] = 0; vd[w] = 0; }
        }
        __syncthreads();
        uint32_t cnt = 0;
        for (uint32_t j = lane; j < n; j += 64) {
            bool valid;
            const uint32_t c = eval_window(pk, vd, j, a.k, a.T, item.locus, &valid);
            cnt += valid ? 1u : 0u;
            if (c != NAN32 && c < a.nk) atomicAdd((unsigned long long*)&a.truth[c], 1ull);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
        if (lane == 0 && cnt) {
            atomicAdd((unsigned long long*)&a.windows[item.locus], (unsigned long long)cnt);
            atomicAdd((unsigned long long*)a.lookups, (unsigned long long)cnt);
        }
    }
}

// The TR k-mers the class table calls flank (EvalTables::both), found once per handle: every TR k-mer of the RPGG in file order
// (ks[i] with counter slot[i]; fbeg[l] = the first of locus l) is looked up; a hit on CLS_FLANK is appended to list[0 .. cap) — the
// first launch, with cap = 0, only counts them.
__global__ void __launch_bounds__(256) k_eval_both(const uint64_t* __restrict__ ks, const uint64_t* __restrict__ slot, const uint64_t* __restrict__ fbeg, uint32_t nloci, uint64_t n,
                                                   const ClsSlot* __restrict__ cls, uint64_t cls_mask, uint32_t cls_shift, ClsSlot* __restrict__ list, uint64_t cap,
                                                   unsigned long long* __restrict__ count) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = nloci;  // the locus: the last one whose first k-mer is not behind i
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (fbeg[mid] <= i) lo = mid; else hi = mid;
        }
        const uint64_t km = ks[i];
        if (kl_lookup(cls, cls_mask, cls_shift, km, lo) != CLS_FLANK) continue;
        const unsigned long long at = atomicAdd(count, 1ull);
        if (at < cap) list[at] = ClsSlot{km, (uint64_t)lo << 32 | (uint32_t)slot[i]};
    }
}

constexpr uint32_t EV_SMALL = 512;  // k-mers up to which a locus is a wave's; above, a workgroup's
constexpr uint32_t EV_NOVF = 0xFFFFFFFFu;

__device__ __forceinline__ bool eval_wave_merge(EvalSums& s, bool ok) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        EvalSums o;
        o.n1 = __shfl_xor(s.n1, d); o.Sx = __shfl_xor(s.Sx, d); o.Sy = __shfl_xor(s.Sy, d); o.Sy1 = __shfl_xor(s.Sy1, d);
        o.Sxy = __shfl_xor(s.Sxy, d); o.Sxx = __shfl_xor(s.Sxx, d); o.Syy = __shfl_xor(s.Syy, d); o.Syy1 = __shfl_xor(s.Syy1, d);
        ok &= eval_merge(s, o);
    }
    return __all(ok);
}

// The loci list[0 .. nlist): BLOCK = false, one wave per locus (four to a workgroup); BLOCK = true, one workgroup of four waves per
// locus.  Every lane adds up its share (eval_locus_part), the shares are merged across the wave by shuffles and, for a workgroup,
// across its waves through LDS.  A locus whose sums left 64 bits anywhere on the way enters its number into *ovf (the lowest wins).
template <bool BLOCK>
__global__ void __launch_bounds__(256) k_eval_sums(const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, const uint64_t* __restrict__ beg,
                                                   const uint32_t* __restrict__ list, uint32_t nlist, EvalSums* __restrict__ out, uint32_t* __restrict__ ovf) {
    __shared__ EvalSums part[4];
    __shared__ uint32_t part_ok[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t q = BLOCK ? blockIdx.x : blockIdx.x * 4 + w;
    const bool on = q < nlist;  // (uniform in the wave; in the workgroup when BLOCK)
    const uint32_t l = on ? list[q] : 0u;
    EvalSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = true;
    if (on) ok = eval_locus_part(x, y, beg[l], beg[l + 1], BLOCK ? threadIdx.x : lane, BLOCK ? 256u : 64u, &s);
    ok = eval_wave_merge(s, ok);
    if (!BLOCK) {
        if (on && lane == 0) {
            out[l] = s;
            if (!ok) atomicMin(ovf, l);
        }
        return;
    }
    if (lane == 0) { part[w] = s; part_ok[w] = ok ? 1u : 0u; }
    __syncthreads();
    if (on && threadIdx.x == 0) {
        EvalSums t = part[0];
        bool tok = part_ok[0] != 0;
        for (int i = 1; i < 4; ++i) { tok &= eval_merge(t, part[i]); tok &= part_ok[i] != 0; }
        out[l] = t;
        if (!tok) atomicMin(ovf, l);
    }
}

}  // namespace

struct dbtk_eval {
    const dbtk_rpgg* g = nullptr;
    int device = -1, num_cu = 1;
    uint64_t nk = 0, nloci = 0;
    uint32_t ksize = 0;
    void* tables = nullptr;  // tables_release
    EvalTables T{nullptr, 0, 0, nullptr, 0, 0};  // the shared class table, and the handle's own table of the k-mers in both sets
    uint64_t nboth = 0;
    uint32_t nsmall = 0, nlarge = 0;
    // (members are destroyed last to first: the buffers from d_both on, then the events, the stream behind them all)
    DevStream stream;
    DevEvent ev[2];
    DevArr<uint64_t> d_scratch;  // [nk]: dbtk_eval_score_host
    DevArr<uint32_t> d_ovf;
    DevArr<EvalSums> d_sums;     // [nloci]
    DevArr<uint32_t> d_list;     // the loci of up to EV_SMALL k-mers, then the others
    DevArr<uint64_t> d_beg;      // [nloci + 1]
    DevArr<uint64_t> d_windows;  // [nloci]
    DevArr<uint64_t> d_truth;    // [nk], then the look-up counter
    DevArr<ClsSlot> d_both;
    bool windows_given = true;      // false after dbtk_eval_truth_set without windows: windows = Sx
    bool scored = false;
    std::vector<dbtk_eval_sums_t> sums;
    double ms[2] = {0, 0};
};

namespace {

void eval_release(dbtk_eval* e) {
    if (e->device >= 0) (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    void* const tables = e->tables;
    delete e;
    tables_release(tables);
}

template <class T> dbtk_status_t eval_alloc(DevArr<T>& a, uint64_t n, const char* what) {
    if (a.alloc(std::max<uint64_t>(n, 1)) == hipSuccess) return DBTK_OK;  // (never empty)
    (void)hipGetLastError();
    set_error(std::string("genotype score: no device memory for ") + what + " (" + std::to_string(n * sizeof(T)) + " bytes)");
    return DBTK_ERR_NOMEM;
}

// EvalTables::both of a handle whose class table stands: the both-set k-mers found on the device (k_eval_both), hashed on the host
// (they are few) and uploaded.
dbtk_status_t eval_build_both(dbtk_eval* e) {
    const dbtk_rpgg* g = e->g;
    const uint64_t n = g->tr_ks.size();
    std::vector<ClsSlot> found;
    if (n) {
        if (g->out_slot.size() != n || g->tr_cnt.size() != e->nloci) { set_error("dbtk_eval_create: the RPGG handle's output order does not match its TR k-mers"); return DBTK_ERR_ARG; }
        std::vector<uint64_t> fbeg(e->nloci + 1, 0);
        for (uint64_t l = 0; l < e->nloci; ++l) fbeg[l + 1] = fbeg[l] + g->tr_cnt[l];
        DevArr<uint64_t> d_ks, d_slot, d_fbeg;
        DevArr<unsigned long long> d_cnt;
        DevArr<ClsSlot> d_list;
        dbtk_status_t a;
        if ((a = eval_alloc(d_ks, n, "the TR k-mers"))) return a;
        if ((a = eval_alloc(d_slot, n, "the TR k-mers' counters"))) return a;
        if ((a = eval_alloc(d_fbeg, e->nloci + 1, "the loci's first TR k-mers"))) return a;
        if ((a = eval_alloc(d_cnt, 1, "a counter"))) return a;
        DEVCHK(hipMemcpy(d_ks, g->tr_ks.data(), n * 8, hipMemcpyHostToDevice));
        DEVCHK(hipMemcpy(d_slot, g->out_slot.data(), n * 8, hipMemcpyHostToDevice));
        DEVCHK(hipMemcpy(d_fbeg, fbeg.data(), (e->nloci + 1) * 8, hipMemcpyHostToDevice));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)e->num_cu * 8);
        unsigned long long cnt = 0;
        for (int pass = 0; pass < 2; ++pass) {
            const uint64_t cap = pass ? cnt : 0;
            if (pass && !cnt) break;
            if (pass && (a = eval_alloc(d_list, cap, "the k-mers in both sets"))) return a;
            DEVCHK(hipMemsetAsync(d_cnt, 0, 8, e->stream));
            hipLaunchKernelGGL(k_eval_both, dim3(grid), dim3(256), 0, e->stream, d_ks.get(), d_slot.get(), d_fbeg.get(), (uint32_t)e->nloci, n, e->T.cls, e->T.cls_mask, e->T.cls_shift,
                               d_list.get(), cap, d_cnt.get());
            DEVCHK(hipGetLastError());
            DEVCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, e->stream));
            DEVCHK(hipStreamSynchronize(e->stream));
            if (pass && cnt != cap) { set_error("dbtk_eval_create: the class table changed between two passes"); return DBTK_ERR_HIP; }
        }
        found.resize(cnt);
        if (cnt) DEVCHK(hipMemcpy(found.data(), d_list, cnt * sizeof(ClsSlot), hipMemcpyDeviceToHost));
    }
    std::sort(found.begin(), found.end(), [](const ClsSlot& x, const ClsSlot& y) { return x.lc != y.lc ? x.lc < y.lc : x.kmer < y.kmer; });
    uint64_t cap = 2;
    while (cap < 2 * found.size() + 2) cap <<= 1;
    uint32_t shift = 64;
    for (uint64_t c = cap; c > 1; c >>= 1) --shift;
    std::vector<ClsSlot> tab(cap, ClsSlot{NAN64, ~0ull});
    for (const ClsSlot& s : found) {
        uint64_t at = hash_cls(s.kmer, (uint32_t)(s.lc >> 32), shift);
        while (tab[at].kmer != NAN64) at = (at + 1) & (cap - 1);
        tab[at] = s;
    }
    const dbtk_status_t a = eval_alloc(e->d_both, cap, "the table of the k-mers in both sets");
    if (a) return a;
    DEVCHK(hipMemcpy(e->d_both, tab.data(), cap * sizeof(ClsSlot), hipMemcpyHostToDevice));
    e->T.both = e->d_both; e->T.both_mask = cap - 1; e->T.both_shift = shift;
    e->nboth = found.size();
    return DBTK_OK;
}

dbtk_status_t eval_create_impl(const dbtk_rpgg_t* g, int device_id, dbtk_eval_t** out) {
    if (!out) { set_error("dbtk_eval_create: null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    if (!g) { set_error("dbtk_eval_create: null argument"); return DBTK_ERR_ARG; }
    if (!g->order_done || g->out_beg.size() != g->nloci + 1 || g->nloci == 0) { set_error("dbtk_eval_create: the RPGG handle has no output order (DBTK_LOAD_INDEX_ONLY?)"); return DBTK_ERR_ARG; }
    if (g->ksize < 2 || g->ksize > 31) { set_error("dbtk_eval_create: ksize outside 2..31"); return DBTK_ERR_ARG; }
    if (device_id < 0) { set_error("dbtk_eval_create: device " + std::to_string(device_id)); return DBTK_ERR_ARG; }
    int ndev = 0;
    if (const dbtk_status_t nd = device_count(&ndev)) return nd;
    if (device_id >= ndev) { set_error("dbtk_eval_create: device " + std::to_string(device_id) + " of " + std::to_string(ndev)); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(device_id));
    std::unique_ptr<dbtk_eval, void (*)(dbtk_eval*)> hold(new dbtk_eval, eval_release);  // (released on every way out but the last)
    dbtk_eval* e = hold.get();
    e->g = g; e->device = device_id; e->nk = g->out_kmer.size(); e->nloci = g->nloci; e->ksize = g->ksize;
    DEVCHK(device_cus(device_id, &e->num_cu));
    dbtk_status_t a;
    ClsView cv;
    if ((a = tables_acquire(g, device_id, &cv, &e->tables))) return a;
    e->T.cls = (const ClsSlot*)cv.cls; e->T.cls_mask = cv.mask; e->T.cls_shift = cv.shift;
    DEVCHK(e->stream.create(hipStreamNonBlocking));
    for (DevEvent& v : e->ev) DEVCHK(v.create(hipEventDefault));
    if ((a = eval_build_both(e))) return a;
    if ((a = eval_alloc(e->d_truth, e->nk + 1, "the truth counts"))) return a;
    if ((a = eval_alloc(e->d_windows, e->nloci, "the windows"))) return a;
    if ((a = eval_alloc(e->d_beg, e->nloci + 1, "the loci's first counters"))) return a;
    if ((a = eval_alloc(e->d_list, e->nloci, "the locus lists"))) return a;
    if ((a = eval_alloc(e->d_sums, e->nloci, "the sums"))) return a;
    if ((a = eval_alloc(e->d_ovf, 1, "the overflow word"))) return a;
    std::vector<uint32_t> list(e->nloci);
    uint32_t ns = 0;
    for (uint64_t l = 0; l < e->nloci; ++l) if (g->out_beg[l + 1] - g->out_beg[l] <= EV_SMALL) list[ns++] = (uint32_t)l;
    e->nsmall = ns;
    for (uint64_t l = 0; l < e->nloci; ++l) if (g->out_beg[l + 1] - g->out_beg[l] > EV_SMALL) list[ns++] = (uint32_t)l;
    e->nlarge = (uint32_t)e->nloci - e->nsmall;
    DEVCHK(hipMemcpy(e->d_list, list.data(), e->nloci * 4, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(e->d_beg, g->out_beg.data(), (e->nloci + 1) * 8, hipMemcpyHostToDevice));
    // (waited for: the truth pass runs on a sim handle's stream, which is ordered against no other)
    DEVCHK(hipMemsetAsync(e->d_truth, 0, (e->nk + 1) * 8, e->stream));
    DEVCHK(hipMemsetAsync(e->d_windows, 0, e->nloci * 8, e->stream));
    DEVCHK(hipStreamSynchronize(e->stream));
    *out = hold.release();
    return DBTK_OK;
}

dbtk_status_t eval_truth_sim_impl(dbtk_eval_t* e, dbtk_sim_t* sim) {
    if (!e || !sim) { set_error("dbtk_eval_truth_sim: null argument"); return DBTK_ERR_ARG; }
    SimSeam ss;
    dbtk_status_t st;
    if ((st = sim_seam(sim, &ss))) return st;
    if (ss.device < 0) { set_error("dbtk_eval_truth_sim: the sim handle is not attached (dbtk_sim_attach first)"); return DBTK_ERR_ARG; }
    if (ss.device != e->device) { set_error("dbtk_eval_truth_sim: the sim handle is on device " + std::to_string(ss.device) + ", the evaluator on device " + std::to_string(e->device)); return DBTK_ERR_ARG; }
    if (ss.nloci != e->nloci) { set_error("dbtk_eval_truth_sim: the sim handle was opened for " + std::to_string(ss.nloci) + " loci, the RPGG has " + std::to_string(e->nloci)); return DBTK_ERR_ARG; }
    if (!e->windows_given) { set_error("dbtk_eval_truth_sim: the truth was set without windows (dbtk_eval_truth_set): dbtk_eval_truth_reset first"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)ss.stream;
    const uint32_t k = e->ksize;
    std::vector<SimSpan> spans;
    std::vector<EvalItem> items;
    DevArr<EvalItem> d_items;
    float total = 0;
    st = [&]() -> dbtk_status_t {
        for (uint32_t g = 0; g < ss.ngroups; ++g) {
            dbtk_status_t a;
            if ((a = sim_group_spans(sim, g, &spans))) return a;
            items.clear();
            for (const SimSpan& sp : spans) {
                if (sp.n < k) continue;  // (no window)
                const uint64_t npos = sp.n - k + 1;
                for (uint64_t p = 0; p < npos; p += EV_CH) items.push_back(EvalItem{sp.off + p, (uint32_t)std::min<uint64_t>(EV_CH, npos - p), sp.locus});
            }
            if (items.empty()) continue;
            if (items.size() > 0xFFFFFFFFull) { set_error("dbtk_eval_truth_sim: more than 2^32 - 1 work items in one contig group"); return DBTK_ERR_UNSUPPORTED; }
            if ((a = sim_group_load(sim, g))) return a;
            if (items.size() > d_items.cap()) {
                if (d_items) DEVCHK(hipStreamSynchronize(s));
                if ((a = eval_alloc(d_items, items.size() + items.size() / 4, "the truth pass's work items"))) return a;
            } else {
                DEVCHK(hipStreamSynchronize(s));  // (the launch before reads the items this copy overwrites)
            }
            DEVCHK(hipMemcpy(d_items, items.data(), items.size() * sizeof(EvalItem), hipMemcpyHostToDevice));
            EvalTruthArgs a2{ss.d_arena, d_items.get(), (uint32_t)items.size(), k, e->T, e->nk, e->d_truth, e->d_windows, e->d_truth + e->nk};
            const uint32_t grid = (uint32_t)std::min<uint64_t>(items.size(), (uint64_t)e->num_cu * 32);
            DEVCHK(hipEventRecord(e->ev[0], s));
            hipLaunchKernelGGL(k_eval_truth, dim3(grid), dim3(64), 0, s, a2);
            DEVCHK(hipGetLastError());
            DEVCHK(hipEventRecord(e->ev[1], s));
            DEVCHK(hipEventSynchronize(e->ev[1]));
            float ms = 0;
            DEVCHK(hipEventElapsedTime(&ms, e->ev[0], e->ev[1]));
            total += ms;
        }
        return DBTK_OK;
    }();
    if (d_items) (void)hipStreamSynchronize(s);  // (the last launch reads the items: d_items is freed behind it)
    e->ms[0] += total;
    e->scored = false;
    return st;
}

dbtk_status_t eval_score_impl(dbtk_eval_t* e, const uint64_t* d_y) {
    DEVCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    DEVCHK(hipMemsetAsync(e->d_ovf, 0xFF, 4, s));  // EV_NOVF
    DEVCHK(hipEventRecord(e->ev[0], s));
    if (e->nsmall) hipLaunchKernelGGL(k_eval_sums<false>, dim3((e->nsmall + 3) / 4), dim3(256), 0, s, e->d_truth.get(), d_y, e->d_beg.get(), e->d_list.get(), e->nsmall, e->d_sums.get(), e->d_ovf.get());
    if (e->nlarge) hipLaunchKernelGGL(k_eval_sums<true>, dim3(e->nlarge), dim3(256), 0, s, e->d_truth.get(), d_y, e->d_beg.get(), e->d_list + e->nsmall, e->nlarge, e->d_sums.get(), e->d_ovf.get());
    DEVCHK(hipGetLastError());
    DEVCHK(hipEventRecord(e->ev[1], s));
    std::vector<EvalSums> raw(e->nloci);
    std::vector<uint64_t> win(e->nloci);
    uint32_t ovf = EV_NOVF;
    DEVCHK(hipMemcpyAsync(raw.data(), e->d_sums, e->nloci * sizeof(EvalSums), hipMemcpyDeviceToHost, s));
    DEVCHK(hipMemcpyAsync(win.data(), e->d_windows, e->nloci * 8, hipMemcpyDeviceToHost, s));
    DEVCHK(hipMemcpyAsync(&ovf, e->d_ovf, 4, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    float ms = 0;
    DEVCHK(hipEventElapsedTime(&ms, e->ev[0], e->ev[1]));
    e->ms[1] += ms;
    e->scored = false;
    if (ovf != EV_NOVF) {
        set_error("genotype score: the sums of locus " + std::to_string(ovf) + " do not fit 64 bits (a product x * y, x * x or y * y, or one of their sums)");
        return DBTK_ERR_OVERFLOW;
    }
    e->sums.resize(e->nloci);
    for (uint64_t l = 0; l < e->nloci; ++l) {
        const EvalSums& r = raw[l];
        e->sums[l] = dbtk_eval_sums_t{e->g->out_beg[l + 1] - e->g->out_beg[l], e->windows_given ? win[l] : r.Sx, r.n1, r.Sx, r.Sy, r.Sy1, r.Sxy, r.Sxx, r.Syy, r.Syy1};
    }
    e->scored = true;
    return DBTK_OK;
}

dbtk_status_t eval_score_ctx_impl(dbtk_eval_t* e, dbtk_ctx_t* ctx) {
    if (!e || !ctx) { set_error("dbtk_eval_score_ctx: null argument"); return DBTK_ERR_ARG; }
    CtxFacts f;
    dbtk_status_t st;
    if ((st = ctx_facts(ctx, &f))) return st;
    if (f.ntrkmers != e->nk) { set_error("dbtk_eval_score_ctx: the context counts " + std::to_string(f.ntrkmers) + " TR k-mers, the evaluator's RPGG has " + std::to_string(e->nk) + ": not the same RPGG build"); return DBTK_ERR_ARG; }
    if (f.device != e->device) { set_error("dbtk_eval_score_ctx: the context is on device " + std::to_string(f.device) + ", the evaluator on device " + std::to_string(e->device)); return DBTK_ERR_ARG; }
    if (f.unflushed_pairs) { set_error("dbtk_eval_score_ctx: " + std::to_string(f.unflushed_pairs) + " pairs appended by dbtk_ingest_align_merged are not aligned yet: flush them first (slot = ~0u, flush = 1)"); return DBTK_ERR_ARG; }
    if ((st = dbtk_ctx_synchronize(ctx))) return st;
    void* b = nullptr;
    uint64_t n64 = 0;
    if ((st = dbtk_ctx_accum_buffer(ctx, &b, &n64))) return st;
    if (!b || n64 < e->nk) { set_error("dbtk_eval_score_ctx: the context has no accumulators"); return DBTK_ERR_ARG; }
    return eval_score_impl(e, (const uint64_t*)b);
}

dbtk_status_t eval_score_device_impl(dbtk_eval_t* e, const void* d_counts) {
    if (!e || !d_counts) { set_error("dbtk_eval_score_device: null argument"); return DBTK_ERR_ARG; }
    if (((uintptr_t)d_counts & 7) != 0) { set_error("dbtk_eval_score_device: d_counts must be 8-byte aligned"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(e->device));
    if (!is_device_memory_of(d_counts, e->device)) { set_error("dbtk_eval_score_device: d_counts is not device memory of the handle's device"); return DBTK_ERR_ARG; }
    return eval_score_impl(e, (const uint64_t*)d_counts);
}

dbtk_status_t eval_score_host_impl(dbtk_eval_t* e, const uint64_t* counts) {
    if (!e || !counts) { set_error("dbtk_eval_score_host: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(e->device));
    if (!e->d_scratch) { const dbtk_status_t a = eval_alloc(e->d_scratch, e->nk, "a count vector"); if (a) return a; }
    if (e->nk) DEVCHK(hipMemcpy(e->d_scratch, counts, e->nk * 8, hipMemcpyHostToDevice));
    return eval_score_impl(e, e->d_scratch);
}

dbtk_status_t eval_write_impl(dbtk_eval_t* e, const char* prefix) {
    if (!e || !prefix) { set_error("dbtk_eval_write: null argument"); return DBTK_ERR_ARG; }
    if (!e->scored) { set_error("dbtk_eval_write: nothing is scored yet (dbtk_eval_score_ctx / _device / _host first)"); return DBTK_ERR_ARG; }
    std::vector<dbtk_eval_cols_t> cols(e->nloci);
    const dbtk_status_t st = dbtk_eval_columns(e->sums.data(), e->nloci, cols.data());
    if (st) return st;
    const std::string ft = std::string(prefix) + ".eval.tsv", fp = std::string(prefix) + ".pred";
    FILE* t = fopen(ft.c_str(), "wb");
    if (!t) { set_error("cannot create " + ft); return DBTK_ERR_IO; }
    FILE* p = fopen(fp.c_str(), "wb");
    if (!p) { fclose(t); set_error("cannot create " + fp); return DBTK_ERR_IO; }
    fprintf(t, "#locus\tnk\tnk_present\twindows\tSx\tSy\tSy_present\tSxy\tSxx\tSyy\tSyy_present\tslope\tpred\tr2\tpred_present\tr2_present\n");
    fprintf(p, "# TrueDosage\tPredDosage\tSlope\tr^2\n");
    for (uint64_t l = 0; l < e->nloci; ++l) {
        const dbtk_eval_sums_t& s = e->sums[l];
        const dbtk_eval_cols_t& c = cols[l];
        fprintf(t, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.2f\t%.1f\t%.4f\t%.1f\t%.4f\n", (unsigned long long)l, (unsigned long long)s.nk,
                (unsigned long long)s.n1, (unsigned long long)s.windows, (unsigned long long)s.Sx, (unsigned long long)s.Sy, (unsigned long long)s.Sy1, (unsigned long long)s.Sxy,
                (unsigned long long)s.Sxx, (unsigned long long)s.Syy, (unsigned long long)s.Syy1, c.slope, c.pred, c.r2, c.pred_present, c.r2_present);
        fprintf(p, "%llu\t%.1f\t%.2f\t%.4f\n", (unsigned long long)s.windows, c.pred_present, c.slope, c.r2_present);
    }
    const bool bad = ferror(t) || ferror(p);
    const bool closed_t = fclose(t) == 0, closed_p = fclose(p) == 0;
    if (bad || !closed_t || !closed_p) { set_error("writing " + ft + " / " + fp + " failed"); return DBTK_ERR_IO; }
    return DBTK_OK;
}

}  // namespace

extern "C" {

uint32_t dbtk_eval_api_version(void) { return DBTK_EVAL_API_VERSION; }

dbtk_status_t dbtk_eval_create(const dbtk_rpgg_t* rpgg, int device_id, dbtk_eval_t** out) {
    return guarded([&] { return eval_create_impl(rpgg, device_id, out); });
}

void dbtk_eval_free(dbtk_eval_t* e) {
    if (e) eval_release(e);
}

dbtk_status_t dbtk_eval_truth_sim(dbtk_eval_t* e, dbtk_sim_t* sim) {
    return guarded([&] { return eval_truth_sim_impl(e, sim); });
}

dbtk_status_t dbtk_eval_truth_set(dbtk_eval_t* e, const uint64_t* counts, const uint64_t* windows) {
    if (!e || !counts) { set_error("dbtk_eval_truth_set: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(e->device));
    if (e->nk) DEVCHK(hipMemcpy(e->d_truth, counts, e->nk * 8, hipMemcpyHostToDevice));
    if (windows) DEVCHK(hipMemcpy(e->d_windows, windows, e->nloci * 8, hipMemcpyHostToDevice));
    else { DEVCHK(hipMemsetAsync(e->d_windows, 0, e->nloci * 8, e->stream)); DEVCHK(hipStreamSynchronize(e->stream)); }
    e->windows_given = windows != nullptr;
    e->scored = false;
    return DBTK_OK;
}

dbtk_status_t dbtk_eval_truth(dbtk_eval_t* e, uint64_t* counts, uint64_t* windows) {
    if (!e) { set_error("dbtk_eval_truth: null argument"); return DBTK_ERR_ARG; }
    return guarded([&]() -> dbtk_status_t {
        DEVCHK(hipSetDevice(e->device));
        if (counts && e->nk) DEVCHK(hipMemcpy(counts, e->d_truth, e->nk * 8, hipMemcpyDeviceToHost));
        if (windows && e->windows_given) DEVCHK(hipMemcpy(windows, e->d_windows, e->nloci * 8, hipMemcpyDeviceToHost));
        if (windows && !e->windows_given) {  // windows = Sx
            std::vector<uint64_t> x(e->nk);
            if (e->nk) DEVCHK(hipMemcpy(x.data(), e->d_truth, e->nk * 8, hipMemcpyDeviceToHost));
            for (uint64_t l = 0; l < e->nloci; ++l) {
                uint64_t sx = 0;
                for (uint64_t i = e->g->out_beg[l]; i < e->g->out_beg[l + 1]; ++i) sx += x[i];
                windows[l] = sx;
            }
        }
        return DBTK_OK;
    });
}

dbtk_status_t dbtk_eval_truth_reset(dbtk_eval_t* e) {
    if (!e) { set_error("dbtk_eval_truth_reset: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(e->device));
    if (e->nk) DEVCHK(hipMemsetAsync(e->d_truth, 0, e->nk * 8, e->stream));  // (the look-up counter behind it stays: dbtk_eval_times counts since creation)
    DEVCHK(hipMemsetAsync(e->d_windows, 0, e->nloci * 8, e->stream));
    DEVCHK(hipStreamSynchronize(e->stream));
    e->windows_given = true;
    e->scored = false;
    return DBTK_OK;
}

dbtk_status_t dbtk_eval_score_ctx(dbtk_eval_t* e, dbtk_ctx_t* ctx) {
    return guarded([&] { return eval_score_ctx_impl(e, ctx); });
}
dbtk_status_t dbtk_eval_score_device(dbtk_eval_t* e, const void* d_counts) {
    return guarded([&] { return eval_score_device_impl(e, d_counts); });
}
dbtk_status_t dbtk_eval_score_host(dbtk_eval_t* e, const uint64_t* counts) {
    return guarded([&] { return eval_score_host_impl(e, counts); });
}

dbtk_status_t dbtk_eval_sums(dbtk_eval_t* e, dbtk_eval_sums_t* out) {
    if (!e || !out) { set_error("dbtk_eval_sums: null argument"); return DBTK_ERR_ARG; }
    if (!e->scored) { set_error("dbtk_eval_sums: nothing is scored yet (dbtk_eval_score_ctx / _device / _host first)"); return DBTK_ERR_ARG; }
    memcpy(out, e->sums.data(), e->nloci * sizeof(dbtk_eval_sums_t));
    return DBTK_OK;
}

dbtk_status_t dbtk_eval_columns(const dbtk_eval_sums_t* sums, uint64_t n, dbtk_eval_cols_t* out) {
    if ((!sums || !out) && n) { set_error("dbtk_eval_columns: null argument"); return DBTK_ERR_ARG; }
    for (uint64_t l = 0; l < n; ++l) {
        const dbtk_eval_sums_t& s = sums[l];
        dbtk_eval_cols_t c = {0, 0, 0, 0, 0};
        if (s.Sxy != 0) {
            const double sxy = (double)s.Sxy, sxx = (double)s.Sxx;
            c.slope = sxy / sxx;
            c.pred = (double)s.Sy / c.slope;
            c.r2 = (sxy * sxy) / (sxx * (double)s.Syy);
            c.pred_present = (double)s.Sy1 / c.slope;
            c.r2_present = (sxy * sxy) / (sxx * (double)s.Syy1);
        }
        out[l] = c;
    }
    return DBTK_OK;
}

dbtk_status_t dbtk_eval_write(dbtk_eval_t* e, const char* out_prefix) {
    return guarded([&] { return eval_write_impl(e, out_prefix); });
}

dbtk_status_t dbtk_eval_times(dbtk_eval_t* e, double ms[2], uint64_t* lookups) {
    if (!e) { set_error("dbtk_eval_times: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(e->device));
    if (ms) { ms[0] = e->ms[0]; ms[1] = e->ms[1]; }
    if (lookups) DEVCHK(hipMemcpy(lookups, e->d_truth + e->nk, 8, hipMemcpyDeviceToHost));
    return DBTK_OK;
}

}  // extern "C"
