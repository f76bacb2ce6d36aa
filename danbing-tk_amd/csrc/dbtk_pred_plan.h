// dbtk_pred_plan.h — which loci fall into which window of a windowed dbtk_pred_t (include/dbtk_pred.h).  Host only, no HIP: the
// library (dbtk_pred.hip) and a stand-alone sanitizer program (tests/pred_plan_check.cpp) both include it.
//
// The k-mer axis: locus t owns the columns [begin(t), end(t)), begin(t) = nk_cum[t - 1] (0 for t = 0), end(t) = nk_cum[t].  Columns
// past nk_cum[ntr - 1] (nk may be larger; they belong to no locus and are never corrected) travel with the last locus: end(ntr - 1) = nk.
#ifndef DBTK_PRED_PLAN_H_
#define DBTK_PRED_PLAN_H_

#include <stdint.h>

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

}  // namespace dbtk_pred_plan
#endif
