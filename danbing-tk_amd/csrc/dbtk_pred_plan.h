// dbtk_pred_plan.h — which loci fall into which window of a windowed dbtk_pred_t, and into which work item of the dosage tables
// (include/dbtk_pred.h).  Host only, no HIP: the library (dbtk_pred.hip) and two stand-alone sanitizer programs
// (tests/pred_plan_check.cpp for the windows, tests/dosage_plan_check.cpp for the work list) include it.
//
// The k-mer axis: locus t owns the columns [begin(t), end(t)), begin(t) = nk_cum[t - 1] (0 for t = 0), end(t) = nk_cum[t].  Columns
// past nk_cum[ntr - 1] (nk may be larger; they belong to no locus and are never corrected) travel with the last locus: end(ntr - 1) = nk.
#ifndef DBTK_PRED_PLAN_H_
#define DBTK_PRED_PLAN_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dbtk_pred_plan {

inline uint64_t locus_begin(const uint32_t* nk_cum, uint64_t t) { return t ? nk_cum[t - 1] : 0u; }
inline uint64_t locus_end(const uint32_t* nk_cum, uint64_t ntr, uint64_t nk, uint64_t t) { return t + 1 == ntr ? nk : nk_cum[t]; }

// the first locus that no window of max_rows columns can hold (ntr: every locus fits); *size = its columns
inline uint64_t first_oversized(const uint32_t* nk_cum, uint64_t ntr, uint64_t nk, uint64_t max_rows, uint64_t* size) {
    for (uint64_t t = 0; t < ntr; ++t) {
        const uint64_t n = locus_end(nk_cum, ntr, nk, t) - locus_begin(nk_cum, t);
        if (n > max_rows) { *size = n; return t; }
    }
    *size = 0;
    return ntr;
}

// The window that starts at locus `first`: the longest run of loci [first, *end) whose columns together are at most max_rows.  Loci
// without columns cost nothing, so a run of them after the last locus that fits belongs to the window too.  *row0 = the window's first
// column, *rows = their number (0 when every locus of the window is empty).  false: first >= ntr, or locus `first` alone is larger
// than max_rows (then *end = first).
inline bool window(const uint32_t* nk_cum, uint64_t ntr, uint64_t nk, uint64_t max_rows, uint64_t first, uint64_t* end, uint64_t* row0, uint64_t* rows) {
    *end = first; *row0 = 0; *rows = 0;
    if (first >= ntr) return false;
    const uint64_t b = locus_begin(nk_cum, first);
    uint64_t e = first, last = b;
    while (e < ntr) {
        const uint64_t le = locus_end(nk_cum, ntr, nk, e);
        if (le - b > max_rows) break;
        last = le;
        ++e;
    }
    *end = e; *row0 = b; *rows = last - b;
    return e > first;
}

// number of windows that cover [0, ntr) (0: some locus does not fit)
inline uint64_t count_windows(const uint32_t* nk_cum, uint64_t ntr, uint64_t nk, uint64_t max_rows) {
    uint64_t n = 0, first = 0, end, row0, rows;
    while (first < ntr) {
        if (!window(nk_cum, ntr, nk, max_rows, first, &end, &row0, &rows)) return 0;
        first = end;
        ++n;
    }
    return n;
}

// ---- the work list of the dosage tables' kernel (dbtk_pred.hip: k_dosage_sample).  A block of DS_T threads scans DS_E counts per
// thread, so a work item holds at most DS_CH k-mers: a run of whole loci, or one DS_CH-sized part of a locus larger than that.
constexpr int DS_T = 256, DS_E = 8, DS_CH = DS_T * DS_E;
constexpr uint32_t NOPART = 0xFFFFFFFFu;
struct DosItem {
    uint32_t k0, nkm;   // the item's k-mers: [k0, k0 + nkm), nkm <= DS_CH
    uint32_t l0, nl;    // whole loci l0 .. l0 + nl - 1 lie in that range (nl = 0: a part of locus l0)
    uint32_t part;      // NOPART, or the partial slot the range's total goes to
    uint32_t nlb;       // loci from l0 on whose raw bias this item makes (nl; 1 for the first part of a large locus; 0 else, or without invariant k-mers)
};

// whole loci packed greedily into items of at most DS_CH k-mers, larger loci cut into parts; locus floc[q] is the sum of the partial
// slots fbeg[q] .. fbeg[q + 1] - 1.  with_bias: the metadata has invariant k-mers at all.
inline void dosage_items(uint64_t ntr, const uint32_t* nk_cum, bool with_bias, std::vector<DosItem>* items, std::vector<uint32_t>* floc, std::vector<uint32_t>* fbeg) {
    DosItem cur{0, 0, 0, 0, NOPART, 0};
    auto flush = [&] { if (cur.nl) { cur.nlb = with_bias ? cur.nl : 0; items->push_back(cur); } cur = DosItem{0, 0, 0, 0, NOPART, 0}; };
    uint32_t nparts = 0;
    fbeg->push_back(0);
    for (uint64_t t = 0; t < ntr; ++t) {
        const uint32_t a = (uint32_t)locus_begin(nk_cum, t), n = nk_cum[t] - a;
        if (n > (uint32_t)DS_CH) {
            flush();
            for (uint32_t o = 0; o < n; o += DS_CH)
                items->push_back(DosItem{a + o, std::min<uint32_t>(DS_CH, n - o), (uint32_t)t, 0, nparts++, (with_bias && !o) ? 1u : 0u});
            floc->push_back((uint32_t)t);
            fbeg->push_back(nparts);
            continue;
        }
        if (cur.nl && cur.nkm + n > (uint32_t)DS_CH) flush();
        if (!cur.nl) { cur.k0 = a; cur.l0 = (uint32_t)t; }
        cur.nkm += n; ++cur.nl;
    }
    flush();
}

}  // namespace dbtk_pred_plan
#endif
