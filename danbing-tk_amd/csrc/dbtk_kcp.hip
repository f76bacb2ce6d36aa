// dbtk_kcp.hip — the bait k-mer count profiles on the device (include/dbtk_kcp.h): the table's kernels and its handle.
// The slot layout, the claim protocol and the multiplicity step are in dbtk_kcp.h (compiled for the host too).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dbtk_kcp.h"
#include "dbtk_dev.h"
#include "dbtk_internal.h"
#include "dbtk_kcp.h"

using namespace dbtk;

namespace {

// the accessor kcp_insert is instantiated with on the GPU: ordinary global atomics
struct KcpDevX {
    __device__ uint64_t atomic_cas(uint64_t* p, uint64_t e, uint64_t d) const {
        return atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)e, (unsigned long long)d);
    }
    __device__ uint32_t atomic_cas32(uint32_t* p, uint32_t e, uint32_t d) const { return atomicCAS(p, e, d); }
    __device__ void atomic_add(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
    __device__ void atomic_add(uint64_t* p, uint64_t v) const { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
    __device__ void atomic_min32(uint32_t* p, uint32_t v) const { atomicMin(p, v); }
    __device__ void atomic_max32(uint32_t* p, uint32_t v) const { atomicMax(p, v); }
};

struct KcpSel { uint32_t pair, lc1; };  // a pair the batch counts, with its (assigned locus + 1) | class << 31

__device__ void kcp_tally(unsigned long long* words, uint32_t took, uint32_t failed, uint32_t ins) {
    if (took) atomicAdd(words + KCP_W_OCC, (unsigned long long)took);
    if (failed) atomicMax(words + KCP_W_FAIL, 1ull);
    if (ins) atomicAdd(words + KCP_W_INS, (unsigned long long)ins);
}

__global__ void __launch_bounds__(256) k_kcp_fill(KcpSlot* t, uint64_t nslots) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) t[i] = KCP_EMPTY;
}

// One wave per mate: read w of the list is mate w & 1 of pair sel[w >> 1].  The wave stages the read's bytes and its canonical
// k-mers in LDS; every lane then takes the positions lane, lane + 64, ...: the multiplicity of its k-mer in this read, and — at the
// k-mer's first occurrence — one insert of (n += 1, sum += c, sumsq += c * c, min, max).  The host has checked that every listed
// read lies inside seq and is no longer than DBTK_MAX_READ_LEN.
__global__ void __launch_bounds__(64) k_kcp_add(const uint8_t* seq, const uint64_t* off, uint64_t base, const KcpSel* sel, uint64_t w0, uint64_t w1, uint32_t k,
                                                KcpSlot* tab, uint64_t mask, uint32_t shift, unsigned long long* words) {
    __shared__ uint8_t s_seq[DBTK_MAX_READ_LEN];
    __shared__ uint64_t s_km[DBTK_MAX_READ_LEN];
    KcpDevX x;
    const uint32_t lane = threadIdx.x;
    uint32_t took = 0, failed = 0, ins = 0;
    for (uint64_t w = w0 + blockIdx.x; w < w1; w += gridDim.x) {
        const KcpSel e = sel[w >> 1];
        const uint64_t r = 2 * (uint64_t)e.pair + (w & 1);
        const uint64_t o0 = off[r] - base;
        const uint32_t len = (uint32_t)(off[r + 1] - off[r]);
        const uint32_t nk = len >= k ? len - k + 1 : 0;
        if (nk == 0) continue;  // (wave-uniform)
        for (uint32_t i = lane; i < len; i += 64) s_seq[i] = seq[o0 + i];
        __syncthreads();
        for (uint32_t i = lane; i < nk; i += 64) s_km[i] = kcp_kmer_at(s_seq, len, i, k);
        __syncthreads();
        for (uint32_t i = lane; i < nk; i += 64) {
            uint32_t c;
            bool first;
            kcp_multiplicity(s_km, nk, i, &c, &first);
            if (!first) continue;
            ++ins;
            if (!kcp_insert(x, tab, mask, shift, s_km[i], e.lc1, 1u, (uint64_t)c, (uint64_t)c * c, c, c, took)) ++failed;
        }
        __syncthreads();  // the next read's bytes overwrite what the slowest lane may still compare
    }
    kcp_tally(words, took, failed, ins);
}

// every entry of the old table into the new one (growth by doubling); the new table's occupancy is counted again
__global__ void __launch_bounds__(256) k_kcp_rehash(const KcpSlot* old, uint64_t nold, KcpSlot* t, uint64_t mask, uint32_t shift, unsigned long long* words) {
    KcpDevX x;
    uint32_t took = 0, failed = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nold; i += (uint64_t)gridDim.x * blockDim.x)
        if (!kcp_move(x, old[i], t, mask, shift, took)) ++failed;
    kcp_tally(words, took, failed, 0);
}

// the entries of class cls, appended to `out` one list per wave (out = nullptr: counted only).  nslots is a multiple of 64: the lanes
// of a wave stay together.
__global__ void __launch_bounds__(256) k_kcp_compact(const KcpSlot* t, uint64_t nslots, uint32_t cls, KcpSlot* out, uint64_t cap, unsigned long long* nout) {
    const int lane = (int)(threadIdx.x & 63);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        const KcpSlot s = t[i];
        const bool keep = kcp_is_entry(s) && (s.lc1 >> 31) == cls;
        const uint64_t b = __ballot(keep);
        if (!b) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(nout, (unsigned long long)__builtin_popcountll(b));
        const uint32_t blo = (uint32_t)__shfl((int)(uint32_t)base, 0, 64), bhi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0, 64);
        const uint64_t at = (((uint64_t)bhi << 32) | blo) + (uint64_t)__builtin_popcountll(b & ((1ull << lane) - 1));
        if (keep && out && at < cap) out[at] = s;
    }
}

// ---- the FP-specific filter (dbtk_kcp_fps_*): csrc/dbtk_kcp.h has the candidate, its state word and the step

// the compacted FP entries into candidates: k-mer, locus, the FP mean as `ktools fps` would parse it; (255, 0), alive
__global__ void __launch_bounds__(256) k_kcp_fps_begin(const KcpSlot* ent, uint64_t n, KcpCand* cand, uint32_t* state) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const KcpSlot s = ent[i];
        cand[i] = KcpCand{s.kmer, (s.lc1 & 0x7FFFFFFFu) - 1u, kcp_mean_text(s)};
        state[i] = kcp_cand_fresh();
    }
}

// One lane per candidate; a dead one costs its 4-byte state word.  Every candidate has one owner and the table is only read: plain
// loads and stores, no atomics but the two tallies at the end (words[0] += living candidates looked up, words[1] += those that died).
__global__ void __launch_bounds__(256) k_kcp_fps_apply(const KcpCand* cand, uint32_t* state, uint64_t n, const KcpSlot* tab, uint64_t mask, uint32_t shift,
                                                       unsigned long long* words) {
    uint32_t looked = 0, died = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t st = state[i];
        if (!(st & KCP_CAND_ALIVE)) continue;
        ++looked;
        const uint32_t nst = kcp_fps_step(tab, mask, shift, cand[i], st);
        if (nst != st) state[i] = nst;
        died += nst == 0u;
    }
    if (looked) atomicAdd(words, (unsigned long long)looked);
    if (died) atomicAdd(words + 1, (unsigned long long)died);
}

__global__ void __launch_bounds__(256) k_kcp_text_stats(const uint32_t* n, const uint64_t* sum, const uint64_t* sumsq, uint64_t count, float* mean, float* sd) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const KcpSlot s{0, 1u, n[i], sum[i], sumsq[i], 0u, 0u};
        mean[i] = kcp_mean_text(s);
        sd[i] = kcp_sd_text(s);
    }
}

constexpr uint64_t KCP_SLOTS_DEFAULT = 1ull << 22;  // 168 MB (DBTK_KCP_SLOTS); grows by doubling
constexpr uint64_t KCP_PIECE_MIN = 1ull << 20;      // k-mer positions of a batch's piece, where a quarter of the table is less

uint32_t log2u64(uint64_t v) { uint32_t l = 0; while ((1ull << l) < v) ++l; return l; }

}  // namespace

struct dbtk_kcp {
    int device = 0, num_cu = 1;
    uint32_t k = 0, flags = 0;
    uint64_t nloci = 0;
    // (members are destroyed last to first: the events, the table, the words, the staging, and the stream behind them all)
    DevStream stream;
    DevArr<KcpSel> d_sel;  // a batch's list of counted pairs, its offsets and reads (grown, never shrunk)
    DevArr<uint64_t> d_off;
    DevArr<uint8_t> d_seq;
    DevArr<unsigned long long> d_words;
    DevArr<KcpSlot> d_tab;
    std::vector<DevEvent> ev;  // a pair per piece of the batch in flight
    uint64_t slots = 0;
    uint64_t occ_ub = 0;  // no fewer than the slots taken: the last reading plus the bounds of the pieces launched since
    double add_ms = 0;
};

// The candidates of the FP-specific filter: a list of its own in HBM (the handle it was begun from may be reset or freed).
struct dbtk_kcp_fps {
    int device = 0, num_cu = 1;
    uint32_t k = 0;
    uint64_t nloci = 0;
    DevStream stream;  // (destroyed last: behind the buffers, which go behind the events)
    DevArr<unsigned long long> d_words;  // living candidates looked up | candidates that died, over all applies
    DevArr<uint32_t> d_state;
    DevArr<KcpCand> d_cand;
    DevEvent ev1, ev0;
    uint64_t n = 0, alive = 0, lookups = 0;
    double apply_ms = 0;
};

namespace {

uint32_t grid_cu(int num_cu, uint64_t n, uint32_t per_block) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, (uint64_t)num_cu * 8)); }
uint32_t grid_for(const dbtk_kcp* c, uint64_t n, uint32_t per_block) { return grid_cu(c->num_cu, n, per_block); }

// (a failure leaves nothing behind: the table is *out's only once it is being filled)
dbtk_status_t kcp_new_table(dbtk_kcp* c, uint64_t slots, DevArr<KcpSlot>* out) {
    DevArr<KcpSlot> t;
    if (t.alloc(slots) != hipSuccess) {
        (void)hipGetLastError();
        set_error("bait profile table: no device memory for " + std::to_string(slots) + " slots (" + std::to_string(slots * sizeof(KcpSlot)) + " bytes)");
        return DBTK_ERR_NOMEM;
    }
    hipLaunchKernelGGL(k_kcp_fill, dim3(grid_for(c, slots, 256)), dim3(256), 0, c->stream, t.get(), slots);
    DEVCHK(hipGetLastError());
    *out = std::move(t);
    return DBTK_OK;
}

// waits for the handle's kernels and reads the words; the sticky word is an error
dbtk_status_t kcp_words(dbtk_kcp* c, unsigned long long w[KCP_WORDS]) {
    DEVCHK(hipStreamSynchronize(c->stream));
    DEVCHK(hipMemcpy(w, c->d_words, sizeof(unsigned long long) * KCP_WORDS, hipMemcpyDeviceToHost));
    c->occ_ub = w[KCP_W_OCC];
    if (w[KCP_W_FAIL]) {
        set_error("bait profile table overflow: an insert found none of " + std::to_string(c->slots) +
                  " slots free (observations are missing until dbtk_kcp_reset); start with more slots (DBTK_KCP_SLOTS, a power of two)");
        return DBTK_ERR_OVERFLOW;
    }
    return DBTK_OK;
}

// Room for `bound` new keys at a load of 1/2 at the most: 2 * (occupied + bound) <= slots, doubling and rehashing until it holds.
dbtk_status_t kcp_room(dbtk_kcp* c, uint64_t bound) {
    if (2 * (c->occ_ub + bound) > c->slots) {  // (occ_ub is an upper bound: look at the real occupancy before growing)
        unsigned long long w[KCP_WORDS];
        const dbtk_status_t st = kcp_words(c, w);
        if (st) return st;
    }
    if (2 * (c->occ_ub + bound) > c->slots) {
        uint64_t cap = c->slots;
        while (2 * (c->occ_ub + bound) > cap) cap <<= 1;
        DevArr<KcpSlot> nt;
        dbtk_status_t st = kcp_new_table(c, cap, &nt);
        if (st) return st;
        DEVCHK(hipMemsetAsync(c->d_words + KCP_W_OCC, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_kcp_rehash, dim3(grid_for(c, c->slots, 256)), dim3(256), 0, c->stream, (const KcpSlot*)c->d_tab, c->slots, nt.get(), cap - 1, 64 - log2u64(cap), c->d_words.get());
        DEVCHK(hipGetLastError());
        const uint64_t old_slots = c->slots;
        std::swap(c->d_tab, nt);  // (nt: the old table from here on, freed behind kcp_words' wait)
        c->slots = cap;
        unsigned long long w[KCP_WORDS];
        st = kcp_words(c, w);
        if (st) return st;
        if (getenv("DBTK_VERBOSE")) fprintf(stderr, "bait profile table: grown from %llu to %llu slots, %llu taken\n", (unsigned long long)old_slots, (unsigned long long)cap, w[KCP_W_OCC]);
    }
    c->occ_ub += bound;
    return DBTK_OK;
}

// fn(t) on nt host threads (the export's sort and formatting: pure CPU work over tens of millions of entries)
unsigned kcp_host_threads() { return std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }
template <class F> void kcp_parallel(unsigned nt, F fn) {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto& x : th) x.join();
}

// by (locus, k-mer): one pass that puts every entry into its locus' run, then the runs sorted by k-mer, a share of the entries per thread
void kcp_sort(std::vector<KcpSlot>& v, uint64_t nloci) {
    const size_t n = v.size();
    if (n < (1u << 12)) {
        std::sort(v.begin(), v.end(), [](const KcpSlot& a, const KcpSlot& b) {
            const uint32_t la = a.lc1 & 0x7FFFFFFFu, lb = b.lc1 & 0x7FFFFFFFu;
            return la != lb ? la < lb : a.kmer < b.kmer;
        });
        return;
    }
    std::vector<uint64_t> beg(nloci + 2, 0);  // beg[l1] = where the run of locus l1 - 1 starts (l1 = 1 .. nloci)
    for (const KcpSlot& s : v) ++beg[(s.lc1 & 0x7FFFFFFFu) + 1];
    for (size_t i = 1; i < beg.size(); ++i) beg[i] += beg[i - 1];
    {
        std::vector<KcpSlot> w(n);
        std::vector<uint64_t> at(beg.begin(), beg.end() - 1);
        for (const KcpSlot& s : v) w[at[s.lc1 & 0x7FFFFFFFu]++] = s;
        v.swap(w);
    }
    const unsigned nt = kcp_host_threads();
    kcp_parallel(nt, [&](unsigned t) {
        // the loci whose runs start inside this thread's share of the entries
        const uint64_t lo = n * t / nt, hi = n * (t + 1) / nt;
        size_t l1 = std::lower_bound(beg.begin() + 1, beg.end() - 1, lo) - beg.begin();
        for (; l1 <= nloci && beg[l1] < hi; ++l1)
            std::sort(v.begin() + beg[l1], v.begin() + beg[l1 + 1], [](const KcpSlot& a, const KcpSlot& b) { return a.kmer < b.kmer; });
    });
}

template <class T> dbtk_status_t kcp_reserve(DevArr<T>& a, size_t n) {
    const size_t want = n + n / 4;
    if (a.reserve(n, want) == hipSuccess) return DBTK_OK;
    (void)hipGetLastError();
    set_error("bait profile: no device memory for a batch's staging (" + std::to_string(want * sizeof(T)) + " bytes)");
    return DBTK_ERR_NOMEM;
}

dbtk_status_t kcp_create_impl(uint32_t ksize, uint64_t nloci, int device_id, uint32_t flags, dbtk_kcp_t** out) {
    if (!out) { set_error("dbtk_kcp_create: null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    if (ksize < 2 || ksize > 31) { set_error("dbtk_kcp_create: ksize must be 2..31"); return DBTK_ERR_ARG; }
    if (nloci == 0 || nloci > 0x7FFFFFFEull) { set_error("dbtk_kcp_create: nloci must be 1..2^31-2"); return DBTK_ERR_ARG; }
    if (flags & ~DBTK_KCP_TP_ONLY) { set_error("dbtk_kcp_create: unknown flags"); return DBTK_ERR_ARG; }
    uint64_t slots0 = KCP_SLOTS_DEFAULT;
    if (const char* e = getenv("DBTK_KCP_SLOTS")) {
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v < 64 || v > (1ull << 32) || (v & (v - 1))) { set_error("DBTK_KCP_SLOTS: a power of two from 64 to 2^32"); return DBTK_ERR_ARG; }
        slots0 = v;
    }
    int ndev = 0;
    if (const dbtk_status_t nd = device_count(&ndev)) return nd;
    if (device_id < 0 || device_id >= ndev) { set_error("dbtk_kcp_create: device " + std::to_string(device_id) + " of " + std::to_string(ndev)); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(device_id));
    dbtk_kcp* c = new dbtk_kcp;
    c->device = device_id; c->k = ksize; c->flags = flags; c->nloci = nloci;
    dbtk_status_t st = DBTK_OK;
    do {
        if (device_cus(device_id, &c->num_cu) != hipSuccess) { set_error("hipGetDeviceProperties failed"); st = DBTK_ERR_HIP; break; }
        if (c->stream.create(hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); st = DBTK_ERR_HIP; break; }
        if (c->d_words.alloc(KCP_WORDS) != hipSuccess) { set_error("hipMalloc of the table's words failed"); st = DBTK_ERR_HIP; break; }
        if (hipMemsetAsync(c->d_words, 0, sizeof(unsigned long long) * KCP_WORDS, c->stream) != hipSuccess) { set_error("hipMemsetAsync failed"); st = DBTK_ERR_HIP; break; }
        if ((st = kcp_new_table(c, slots0, &c->d_tab))) break;
        c->slots = slots0;
        if (hipStreamSynchronize(c->stream) != hipSuccess) { set_error("bait profile table: the fill kernel failed"); st = DBTK_ERR_HIP; break; }
    } while (0);
    if (st) { dbtk_kcp_free(c); return st; }
    *out = c;
    return DBTK_OK;
}

// seq == nullptr: the reads and their offsets are in device memory already (d_seq, indexed by the offsets as they are; d_off), and
// off / src are the host's copies of the offsets and sources (dbtk_kcp_add_device)
dbtk_status_t kcp_add_impl(dbtk_kcp_t* c, const uint8_t* seq, const uint64_t* off, uint64_t npairs, const uint32_t* src, const uint32_t* dst, const uint8_t* d_seq = nullptr,
                           const uint64_t* d_off = nullptr) {
    if (!c || (npairs && ((!seq && !d_seq) || !off || !src || !dst))) { set_error("dbtk_kcp_add: null argument"); return DBTK_ERR_ARG; }
    if (npairs > 0x7FFFFFFFull) { set_error("dbtk_kcp_add: more than 2^31 - 1 pairs in one call"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(c->device));
    {  // a failed insert of an earlier call
        unsigned long long w[KCP_WORDS];
        const dbtk_status_t st = kcp_words(c, w);
        if (st) return st;
    }
    if (!npairs) return DBTK_OK;
    // the pairs to count, and per pair the k-mer positions of its mates (the bound on its new keys)
    std::vector<KcpSel> sel;
    std::vector<uint32_t> npos;
    for (uint64_t r = 0; r < 2 * npairs; ++r)
        if (off[r + 1] < off[r]) { set_error("dbtk_kcp_add: seq_offsets must not decrease (read " + std::to_string(r) + ")"); return DBTK_ERR_ARG; }
    for (uint64_t p = 0; p < npairs; ++p) {
        if (dst[p] >= c->nloci) continue;
        const uint32_t cls = src[p] == dst[p] ? 0u : 1u;
        if (cls && (c->flags & DBTK_KCP_TP_ONLY)) continue;
        uint32_t np = 0;
        for (int m = 0; m < 2; ++m) {
            const uint64_t len = off[2 * p + m + 1] - off[2 * p + m];
            if (len > DBTK_MAX_READ_LEN) {
                set_error("dbtk_kcp_add: read " + std::to_string(2 * p + m) + " has " + std::to_string(len) + " bases (at most " + std::to_string(DBTK_MAX_READ_LEN) + ")");
                return DBTK_ERR_READ_TOO_LONG;
            }
            if (len >= c->k) np += (uint32_t)(len - c->k + 1);
        }
        if (!np) continue;
        sel.push_back(KcpSel{(uint32_t)p, kcp_lc1(dst[p], cls)});
        npos.push_back(np);
    }
    if (sel.empty()) return DBTK_OK;
    const uint64_t base = seq ? off[0] : 0, nbytes = off[2 * npairs] - base;
    dbtk_status_t st;
    if (seq && (st = kcp_reserve(c->d_seq, (size_t)nbytes + 1))) return st;
    if (seq && (st = kcp_reserve(c->d_off, (size_t)(2 * npairs + 1)))) return st;
    if ((st = kcp_reserve(c->d_sel, sel.size()))) return st;
    // (the stream is idle — kcp_words above waited for it — and these copies return when they are done)
    if (seq) {
        DEVCHK(hipMemcpy(c->d_seq, seq + base, nbytes, hipMemcpyHostToDevice));
        DEVCHK(hipMemcpy(c->d_off, off, sizeof(uint64_t) * (2 * npairs + 1), hipMemcpyHostToDevice));
        d_seq = c->d_seq; d_off = c->d_off;
    }
    DEVCHK(hipMemcpy(c->d_sel, sel.data(), sizeof(KcpSel) * sel.size(), hipMemcpyHostToDevice));
    // piece by piece: room first, then the kernel
    size_t nev = 0;
    for (size_t i = 0; i < sel.size();) {
        const uint64_t piece = std::max(c->slots / 4, KCP_PIECE_MIN);
        uint64_t bound = 0;
        size_t j = i;
        while (j < sel.size() && (j == i || bound + npos[j] <= piece)) bound += npos[j++];
        if ((st = kcp_room(c, bound))) return st;
        while (c->ev.size() < nev + 2) {
            DevEvent e;
            DEVCHK(e.create(hipEventDefault));
            c->ev.push_back(std::move(e));
        }
        const uint64_t w0 = 2 * (uint64_t)i, w1 = 2 * (uint64_t)j;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(w1 - w0, (uint64_t)c->num_cu * 32);
        DEVCHK(hipEventRecord(c->ev[nev], c->stream));
        hipLaunchKernelGGL(k_kcp_add, dim3(grid), dim3(64), 0, c->stream, d_seq, d_off, base, (const KcpSel*)c->d_sel, w0, w1, c->k, c->d_tab.get(),
                           c->slots - 1, 64 - log2u64(c->slots), c->d_words.get());
        DEVCHK(hipGetLastError());
        DEVCHK(hipEventRecord(c->ev[nev + 1], c->stream));
        nev += 2;
        i = j;
    }
    DEVCHK(hipStreamSynchronize(c->stream));
    for (size_t e = 0; e < nev; e += 2) {
        float ms = 0;
        DEVCHK(hipEventElapsedTime(&ms, c->ev[e], c->ev[e + 1]));
        c->add_ms += ms;
    }
    return DBTK_OK;
}

// the entries of class cls compacted into a device array (want_out false: counted only, *d_out stays empty)
dbtk_status_t kcp_compact(dbtk_kcp_t* c, uint32_t cls, bool want_out, DevArr<KcpSlot>* d_out, uint64_t* count) {
    d_out->drop();
    if (!c || cls > 1) { set_error("bait profile: null handle or a class other than 0 (TP) and 1 (FP)"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(c->device));
    unsigned long long w[KCP_WORDS];
    dbtk_status_t st = kcp_words(c, w);
    if (st) return st;
    const uint64_t cap = want_out ? w[KCP_W_OCC] : 0;  // (no class has more entries than the table has slots taken)
    DevArr<unsigned long long> d_n;
    DevArr<KcpSlot> out;
    DEVCHK(d_n.alloc(1));
    unsigned long long n = 0;
    DEVCHK(hipMemsetAsync(d_n, 0, sizeof(unsigned long long), c->stream));
    if (cap) DEVCHK(out.alloc(cap));
    hipLaunchKernelGGL(k_kcp_compact, dim3(grid_for(c, c->slots, 256)), dim3(256), 0, c->stream, (const KcpSlot*)c->d_tab, c->slots, cls, out.get(), cap, d_n.get());
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, c->stream));
    DEVCHK(hipStreamSynchronize(c->stream));
    if (want_out && n > cap) { set_error("bait profile: the table holds more entries than slots taken"); return DBTK_ERR_HIP; }
    *d_out = std::move(out);
    *count = n;
    return DBTK_OK;
}

// the entries of class cls, sorted by (locus, k-mer)
dbtk_status_t kcp_entries(dbtk_kcp_t* c, uint32_t cls, std::vector<KcpSlot>* out, uint64_t* count) {
    DevArr<KcpSlot> d_out;
    uint64_t n = 0;
    const dbtk_status_t st = kcp_compact(c, cls, out != nullptr, &d_out, &n);
    if (st) return st;
    if (out) {
        out->resize(n);
        if (n && hipMemcpy(out->data(), d_out, n * sizeof(KcpSlot), hipMemcpyDeviceToHost) != hipSuccess) { set_error("bait profile: copying the entries to the host failed"); return DBTK_ERR_HIP; }
    }
    if (count) *count = n;
    if (out) kcp_sort(*out, c->nloci);
    return DBTK_OK;
}

dbtk_status_t kcp_write_class(dbtk_kcp_t* c, uint32_t cls, const std::string& fn) {
    std::vector<KcpSlot> ent;
    const dbtk_status_t st = kcp_entries(c, cls, &ent, nullptr);
    if (st) return st;
    FILE* f = fopen(fn.c_str(), "wb");
    if (!f) { set_error("cannot create " + fn); return DBTK_ERR_IO; }
    // rounds of one piece of the entries per thread, formatted side by side and written in order (a piece opens a locus' section
    // where its first entry's locus differs from the entry before it)
    const unsigned nt = kcp_host_threads();
    const size_t PIECE = 1u << 18;
    std::vector<std::string> text(nt);
    bool ok = true;
    for (size_t r0 = 0; r0 < ent.size() && ok; r0 += (size_t)nt * PIECE) {
        kcp_parallel(nt, [&](unsigned t) {
            std::string& buf = text[t];
            buf.clear();
            char line[128];
            const size_t b = std::min(ent.size(), r0 + (size_t)t * PIECE), e = std::min(ent.size(), b + PIECE);
            uint32_t cur = b ? ent[b - 1].lc1 & 0x7FFFFFFFu : 0;  // locus + 1 of the open section
            for (size_t i = b; i < e; ++i) {
                const KcpSlot& s = ent[i];
                const uint32_t l1 = s.lc1 & 0x7FFFFFFFu;
                if (l1 != cur) { cur = l1; buf += '>'; buf += std::to_string(l1 - 1); buf += '\n'; }
                const int n = snprintf(line, sizeof line, "%llu\t%u\t%u\t%.4f\t%.4f\n", (unsigned long long)s.kmer, s.mn, s.mx, kcp_mean(s), kcp_sd(s));
                buf.append(line, (size_t)n);
            }
        });
        for (unsigned t = 0; t < nt && ok; ++t) ok = fwrite(text[t].data(), 1, text[t].size(), f) == text[t].size();
    }
    if (fclose(f) || !ok) { set_error("write error on " + fn); return DBTK_ERR_IO; }
    return DBTK_OK;
}

void kcp_fps_free_impl(dbtk_kcp_fps* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    delete f;
}

dbtk_status_t kcp_fps_begin_impl(dbtk_kcp_t* c, dbtk_kcp_fps_t** out) {
    if (!c || !out) { set_error("dbtk_kcp_fps_begin: null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    if (c->flags & DBTK_KCP_TP_ONLY) { set_error("dbtk_kcp_fps_begin: the handle counts true positives only (DBTK_KCP_TP_ONLY): it has no FP class to take candidates from"); return DBTK_ERR_ARG; }
    DevArr<KcpSlot> d_ent;
    uint64_t n = 0;
    const dbtk_status_t st = kcp_compact(c, 1, true, &d_ent, &n);
    if (st) return st;
    std::unique_ptr<dbtk_kcp_fps, void (*)(dbtk_kcp_fps*)> hold(new dbtk_kcp_fps, kcp_fps_free_impl);  // (waits for its stream and goes before d_ent does)
    dbtk_kcp_fps* f = hold.get();
    f->device = c->device; f->num_cu = c->num_cu; f->k = c->k; f->nloci = c->nloci; f->n = f->alive = n;
    DEVCHK(f->stream.create(hipStreamNonBlocking));
    DEVCHK(f->ev0.create(hipEventDefault));
    DEVCHK(f->ev1.create(hipEventDefault));
    DEVCHK(f->d_words.alloc(2));
    DEVCHK(hipMemsetAsync(f->d_words, 0, 2 * sizeof(unsigned long long), f->stream));
    if (n) {
        if (f->d_cand.alloc(n) != hipSuccess || f->d_state.alloc(n) != hipSuccess) {
            (void)hipGetLastError();
            set_error("bait fps: no device memory for " + std::to_string(n) + " candidates (" + std::to_string(n * (sizeof(KcpCand) + sizeof(uint32_t))) + " bytes)");
            return DBTK_ERR_NOMEM;
        }
        // (d_ent is complete: kcp_compact waited for the handle's stream)
        hipLaunchKernelGGL(k_kcp_fps_begin, dim3(grid_cu(f->num_cu, n, 256)), dim3(256), 0, f->stream, (const KcpSlot*)d_ent, n, f->d_cand.get(), f->d_state.get());
        DEVCHK(hipGetLastError());
    }
    DEVCHK(hipStreamSynchronize(f->stream));
    *out = hold.release();
    return DBTK_OK;
}

dbtk_status_t kcp_fps_apply_impl(dbtk_kcp_fps_t* f, dbtk_kcp_t* c) {
    if (!f || !c) { set_error("dbtk_kcp_fps_apply: null argument"); return DBTK_ERR_ARG; }
    if (c->device != f->device || c->k != f->k || c->nloci != f->nloci) {
        set_error("dbtk_kcp_fps_apply: the table (device " + std::to_string(c->device) + ", k " + std::to_string(c->k) + ", " + std::to_string(c->nloci) + " loci) does not match the candidates' (device " +
                  std::to_string(f->device) + ", k " + std::to_string(f->k) + ", " + std::to_string(f->nloci) + " loci)");
        return DBTK_ERR_ARG;
    }
    DEVCHK(hipSetDevice(f->device));
    unsigned long long w[KCP_WORDS];
    const dbtk_status_t st = kcp_words(c, w);  // the table is quiescent from here on (and whole: no insert failed)
    if (st) return st;
    if (!f->n) return DBTK_OK;
    DEVCHK(hipEventRecord(f->ev0, f->stream));
    hipLaunchKernelGGL(k_kcp_fps_apply, dim3(grid_cu(f->num_cu, f->n, 256)), dim3(256), 0, f->stream, (const KcpCand*)f->d_cand, f->d_state.get(), f->n, (const KcpSlot*)c->d_tab,
                       c->slots - 1, 64 - log2u64(c->slots), f->d_words.get());
    DEVCHK(hipGetLastError());
    DEVCHK(hipEventRecord(f->ev1, f->stream));
    unsigned long long fw[2];
    DEVCHK(hipMemcpyAsync(fw, f->d_words, sizeof fw, hipMemcpyDeviceToHost, f->stream));
    DEVCHK(hipStreamSynchronize(f->stream));
    float ms = 0;
    DEVCHK(hipEventElapsedTime(&ms, f->ev0, f->ev1));
    f->apply_ms += ms;
    f->lookups = fw[0];
    f->alive = f->n - fw[1];
    return DBTK_OK;
}

struct FpsLine { uint32_t locus; uint64_t kmer; uint8_t mi, ma; };

// the living candidates sorted by (locus, k-mer); `seen` (where not null): the loci that had a candidate, ascending
dbtk_status_t kcp_fps_lines(dbtk_kcp_fps_t* f, std::vector<FpsLine>* lines, std::vector<uint32_t>* seen) {
    if (!f) { set_error("bait fps: null handle"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(f->device));
    std::vector<KcpCand> cand(f->n);
    std::vector<uint32_t> state(f->n);
    if (f->n) {
        DEVCHK(hipMemcpy(cand.data(), f->d_cand, f->n * sizeof(KcpCand), hipMemcpyDeviceToHost));
        DEVCHK(hipMemcpy(state.data(), f->d_state, f->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    lines->clear();
    for (uint64_t i = 0; i < f->n; ++i) {
        if (seen) seen->push_back(cand[i].locus);
        if (state[i] & KCP_CAND_ALIVE) lines->push_back(FpsLine{cand[i].locus, cand[i].kmer, (uint8_t)(state[i] & 255u), (uint8_t)((state[i] >> 8) & 255u)});
    }
    std::sort(lines->begin(), lines->end(), [](const FpsLine& a, const FpsLine& b) { return a.locus != b.locus ? a.locus < b.locus : a.kmer < b.kmer; });
    if (seen) {
        std::sort(seen->begin(), seen->end());
        seen->erase(std::unique(seen->begin(), seen->end()), seen->end());
    }
    if (lines->size() != f->alive) { set_error("bait fps: the candidate list and its tally of the living disagree"); return DBTK_ERR_HIP; }
    return DBTK_OK;
}

dbtk_status_t kcp_text_stats_impl(int device_id, const uint32_t* n, const uint64_t* sum, const uint64_t* sumsq, uint64_t count, float* mean_out, float* sd_out) {
    if (count && (!n || !sum || !sumsq || !mean_out || !sd_out)) { set_error("dbtk_kcp_text_stats: null argument"); return DBTK_ERR_ARG; }
    for (uint64_t i = 0; i < count; ++i)
        if (!n[i] || (unsigned __int128)n[i] * sumsq[i] < (unsigned __int128)sum[i] * sum[i]) {
            set_error("dbtk_kcp_text_stats: entry " + std::to_string(i) + " is not the moments of any counts (n >= 1 and n * sumsq >= sum^2)");
            return DBTK_ERR_ARG;
        }
    int ndev = 0;
    if (const dbtk_status_t nd = device_count(&ndev)) return nd;
    if (device_id < 0 || device_id >= ndev) { set_error("dbtk_kcp_text_stats: device " + std::to_string(device_id) + " of " + std::to_string(ndev)); return DBTK_ERR_ARG; }
    if (!count) return DBTK_OK;
    DEVCHK(hipSetDevice(device_id));
    int num_cu = 1;
    DEVCHK(device_cus(device_id, &num_cu));
    // one allocation: sum | sumsq | n | mean | sd
    DevArr<uint8_t> d;
    DEVCHK(d.alloc(count * 28));
    uint64_t *d_sum = (uint64_t*)d.get(), *d_sq = d_sum + count;
    uint32_t* d_n = (uint32_t*)(d_sq + count);
    float *d_mean = (float*)(d_n + count), *d_sd = d_mean + count;
    DEVCHK(hipMemcpy(d_sum, sum, count * 8, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_sq, sumsq, count * 8, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_n, n, count * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_kcp_text_stats, dim3(grid_cu(num_cu, count, 256)), dim3(256), 0, nullptr, (const uint32_t*)d_n, (const uint64_t*)d_sum, (const uint64_t*)d_sq, count, d_mean, d_sd);
    DEVCHK(hipGetLastError());
    DEVCHK(hipDeviceSynchronize());
    DEVCHK(hipMemcpy(mean_out, d_mean, count * 4, hipMemcpyDeviceToHost));
    DEVCHK(hipMemcpy(sd_out, d_sd, count * 4, hipMemcpyDeviceToHost));
    return DBTK_OK;
}

}  // namespace

extern "C" {

uint32_t dbtk_kcp_api_version(void) { return DBTK_KCP_API_VERSION; }

dbtk_status_t dbtk_kcp_set_tp_only(dbtk_kcp_t* c, int on) {
    if (!c) { set_error("dbtk_kcp_set_tp_only: null argument"); return DBTK_ERR_ARG; }
    c->flags = on ? (c->flags | DBTK_KCP_TP_ONLY) : (c->flags & ~DBTK_KCP_TP_ONLY);
    return DBTK_OK;
}

dbtk_status_t dbtk_kcp_fps_begin(dbtk_kcp_t* c, dbtk_kcp_fps_t** out) { return guarded([&] { return kcp_fps_begin_impl(c, out); }); }
dbtk_status_t dbtk_kcp_fps_apply(dbtk_kcp_fps_t* f, dbtk_kcp_t* c) { return guarded([&] { return kcp_fps_apply_impl(f, c); }); }
void dbtk_kcp_fps_free(dbtk_kcp_fps_t* f) { kcp_fps_free_impl(f); }

dbtk_status_t dbtk_kcp_fps_count(dbtk_kcp_fps_t* f, uint64_t* candidates, uint64_t* alive) {
    if (!f) { set_error("dbtk_kcp_fps_count: null argument"); return DBTK_ERR_ARG; }
    if (candidates) *candidates = f->n;
    if (alive) *alive = f->alive;
    return DBTK_OK;
}

dbtk_status_t dbtk_kcp_fps_read(dbtk_kcp_fps_t* f, uint32_t* loci, uint64_t* kmers, uint8_t* mi, uint8_t* ma, uint64_t cap) {
    return guarded([&]() -> dbtk_status_t {
        std::vector<FpsLine> v;
        const dbtk_status_t st = kcp_fps_lines(f, &v, nullptr);
        if (st) return st;
        if (v.size() > cap) { set_error("dbtk_kcp_fps_read: " + std::to_string(v.size()) + " living candidates, room for " + std::to_string(cap)); return DBTK_ERR_OVERFLOW; }
        for (size_t i = 0; i < v.size(); ++i) {
            if (loci) loci[i] = v[i].locus;
            if (kmers) kmers[i] = v[i].kmer;
            if (mi) mi[i] = v[i].mi;
            if (ma) ma[i] = v[i].ma;
        }
        return DBTK_OK;
    });
}

dbtk_status_t dbtk_kcp_fps_write(dbtk_kcp_fps_t* f, const char* path) {
    if (!f || !path) { set_error("dbtk_kcp_fps_write: null argument"); return DBTK_ERR_ARG; }
    return guarded([&]() -> dbtk_status_t {
        std::vector<FpsLine> v;
        std::vector<uint32_t> seen;
        const dbtk_status_t st = kcp_fps_lines(f, &v, &seen);
        if (st) return st;
        std::string text;
        size_t i = 0;
        for (uint32_t l : seen) {  // (a header also for a locus all of whose candidates died, as the reference writes it)
            text += '>'; text += std::to_string(l); text += '\n';
            for (; i < v.size() && v[i].locus == l; ++i) {
                text += std::to_string(v[i].kmer); text += '\t'; text += std::to_string((int)v[i].mi); text += '\t'; text += std::to_string((int)v[i].ma); text += '\n';
            }
        }
        FILE* out = fopen(path, "wb");
        if (!out) { set_error(std::string("cannot create ") + path); return DBTK_ERR_IO; }
        const bool ok = fwrite(text.data(), 1, text.size(), out) == text.size();
        if (fclose(out) || !ok) { set_error(std::string("write error on ") + path); return DBTK_ERR_IO; }
        return DBTK_OK;
    });
}

dbtk_status_t dbtk_kcp_fps_times(dbtk_kcp_fps_t* f, double* apply_ms, uint64_t* lookups) {
    if (!f) { set_error("dbtk_kcp_fps_times: null argument"); return DBTK_ERR_ARG; }
    if (apply_ms) *apply_ms = f->apply_ms;
    if (lookups) *lookups = f->lookups;
    return DBTK_OK;
}

dbtk_status_t dbtk_kcp_text_stats(int device_id, const uint32_t* n, const uint64_t* sum, const uint64_t* sumsq, uint64_t count, float* mean_out, float* sd_out) {
    return guarded([&] { return kcp_text_stats_impl(device_id, n, sum, sumsq, count, mean_out, sd_out); });
}

dbtk_status_t dbtk_kcp_create(uint32_t ksize, uint64_t nloci, int device_id, uint32_t flags, dbtk_kcp_t** out) {
    return guarded([&] { return kcp_create_impl(ksize, nloci, device_id, flags, out); });
}

void dbtk_kcp_free(dbtk_kcp_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

dbtk_status_t dbtk_kcp_add(dbtk_kcp_t* c, const uint8_t* seq_bytes, const uint64_t* seq_offsets, uint64_t npairs, const uint32_t* src, const uint32_t* dst) {
    return guarded([&] { return kcp_add_impl(c, seq_bytes, seq_offsets, npairs, src, dst); });
}

dbtk_status_t dbtk_kcp_add_device(dbtk_kcp_t* c, const void* d_seq, const void* d_offsets, uint64_t npairs, const void* d_src, const uint32_t* dst) {
    return guarded([&]() -> dbtk_status_t {
        if (!c || (npairs && (!d_seq || !d_offsets || !d_src || !dst))) { set_error("dbtk_kcp_add_device: null argument"); return DBTK_ERR_ARG; }
        if (npairs > 0x7FFFFFFFull) { set_error("dbtk_kcp_add_device: more than 2^31 - 1 pairs in one call"); return DBTK_ERR_ARG; }
        if (!npairs) return kcp_add_impl(c, nullptr, nullptr, 0, nullptr, nullptr);
        DEVCHK(hipSetDevice(c->device));
        // what decides which pairs are counted, and the bound on their new keys, comes to the host: 20 bytes per pair; the reads stay
        std::vector<uint64_t> off(2 * npairs + 1);
        std::vector<uint32_t> src(npairs);
        DEVCHK(hipMemcpy(off.data(), d_offsets, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        DEVCHK(hipMemcpy(src.data(), d_src, src.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return kcp_add_impl(c, nullptr, off.data(), npairs, src.data(), dst, (const uint8_t*)d_seq, (const uint64_t*)d_offsets);
    });
}

dbtk_status_t dbtk_kcp_count(dbtk_kcp_t* c, uint32_t cls, uint64_t* n) {
    if (!n) { set_error("dbtk_kcp_count: null argument"); return DBTK_ERR_ARG; }
    return guarded([&] { return kcp_entries(c, cls, nullptr, n); });
}

dbtk_status_t dbtk_kcp_read(dbtk_kcp_t* c, uint32_t cls, uint32_t* loci, uint64_t* kmers, uint32_t* n, uint64_t* sum, uint64_t* sumsq, uint32_t* mn, uint32_t* mx,
                            uint64_t cap) {
    return guarded([&]() -> dbtk_status_t {
        std::vector<KcpSlot> ent;
        const dbtk_status_t st = kcp_entries(c, cls, &ent, nullptr);
        if (st) return st;
        if (ent.size() > cap) { set_error("dbtk_kcp_read: " + std::to_string(ent.size()) + " entries, room for " + std::to_string(cap)); return DBTK_ERR_OVERFLOW; }
        for (size_t i = 0; i < ent.size(); ++i) {
            const KcpSlot& s = ent[i];
            if (loci) loci[i] = (s.lc1 & 0x7FFFFFFFu) - 1;
            if (kmers) kmers[i] = s.kmer;
            if (n) n[i] = s.n;
            if (sum) sum[i] = s.sum;
            if (sumsq) sumsq[i] = s.sumsq;
            if (mn) mn[i] = s.mn;
            if (mx) mx[i] = s.mx;
        }
        return DBTK_OK;
    });
}

dbtk_status_t dbtk_kcp_write(dbtk_kcp_t* c, const char* out_prefix) {
    if (!c || !out_prefix) { set_error("dbtk_kcp_write: null argument"); return DBTK_ERR_ARG; }
    return guarded([&]() -> dbtk_status_t {
        const std::string pref(out_prefix);
        dbtk_status_t st = kcp_write_class(c, 0, pref + ".TP_pf.txt");
        if (!st && !(c->flags & DBTK_KCP_TP_ONLY)) st = kcp_write_class(c, 1, pref + ".FP_pf.txt");
        return st;
    });
}

dbtk_status_t dbtk_kcp_reset(dbtk_kcp_t* c) {
    if (!c) { set_error("dbtk_kcp_reset: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_kcp_fill, dim3(grid_for(c, c->slots, 256)), dim3(256), 0, c->stream, c->d_tab.get(), c->slots);
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemsetAsync(c->d_words, 0, sizeof(unsigned long long) * KCP_WORDS, c->stream));
    DEVCHK(hipStreamSynchronize(c->stream));
    c->occ_ub = 0;
    c->add_ms = 0;
    return DBTK_OK;
}

dbtk_status_t dbtk_kcp_stats(dbtk_kcp_t* c, uint64_t* table_bytes, uint64_t* slots, uint64_t* occupied) {
    if (!c) { set_error("dbtk_kcp_stats: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(c->device));
    unsigned long long w[KCP_WORDS];
    const dbtk_status_t st = kcp_words(c, w);
    if (st) return st;
    if (table_bytes) *table_bytes = c->slots * sizeof(KcpSlot);
    if (slots) *slots = c->slots;
    if (occupied) *occupied = w[KCP_W_OCC];
    return DBTK_OK;
}

dbtk_status_t dbtk_kcp_times(dbtk_kcp_t* c, double* add_ms, uint64_t* inserts) {
    if (!c) { set_error("dbtk_kcp_times: null argument"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(c->device));
    unsigned long long w[KCP_WORDS];
    const dbtk_status_t st = kcp_words(c, w);
    if (st) return st;
    if (add_ms) *add_ms = c->add_ms;
    if (inserts) *inserts = w[KCP_W_INS];
    return DBTK_OK;
}

}  // extern "C"
