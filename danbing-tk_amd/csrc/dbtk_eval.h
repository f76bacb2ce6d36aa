// dbtk_eval.h — the bodies of the two kernels of the genotype score (include/dbtk_eval.h), written once and compiled twice: by hipcc
// into k_eval_truth / k_eval_sums (dbtk_eval.hip), and by the host compiler for tests/eval_check.cpp.
#ifndef DBTK_EVAL_BODIES_H_
#define DBTK_EVAL_BODIES_H_

#include <stdint.h>
#include <string.h>

#include "dbtk_tables.h"

namespace dbtk {

// ---- truth: an item is a run of at most EV_CH consecutive start positions of one interval
constexpr uint32_t EV_CH = 1024;
constexpr uint32_t EV_WORDS = (EV_CH + 31 - 1 + 15) / 16 + 2;  // 16 bases per word, k <= 31, two words of zero padding (window_kmer)
struct EvalItem {
    uint64_t off;    // of the first start position, in the resident group's arena
    uint32_t n;      // start positions: 1 .. EV_CH; the bases [off, off + n + k - 1) belong to the interval
    uint32_t locus;
};
// words the item's bases take once packed
DBTK_HD uint32_t eval_item_words(uint32_t n, uint32_t k) { return (n + k - 1 + 15) / 16; }
// word w of the packed item: the 16 bases at src + 16 w, upper-cased (the arena holds ACGTNacgtn only), 2 bits each, with their
// validity bits.  Reads 16 bytes whatever the item's length: the arena is allocated with that much slack behind its last base.
DBTK_HD void eval_stage_word(const uint8_t* src, uint32_t w, uint32_t* pk, uint16_t* vd) {
    uint32_t v[4], valid;
    __builtin_memcpy(v, src + 16ull * w, 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] &= 0xDFDFDFDFu;
    pk[w] = pack16(v, &valid);
    vd[w] = (uint16_t)valid;
}
// (locus, k-mer) -> counter.  The aligner's class table answers CLS_FLANK for a k-mer that is in the flank set AND the TR set of a
// locus (flank beats TR, as assignTRkmc tests them) — the k-mer of a repeat that goes on one base into a flank, one time in four.  The
// truth counts those as TR k-mers, as fa2kmers does, so the few of them have a table of their own (`both`, same slots and probing,
// value = the counter): only a window that the class table calls flank pays the second probe.
struct EvalTables {
    const ClsSlot* cls; uint64_t cls_mask; uint32_t cls_shift;
    const ClsSlot* both; uint64_t both_mask; uint32_t both_shift;
};
// The window at start position j of a packed item: *valid = all k bases are ACGT (it counts as a window of the locus); returns the
// counter of its canonical k-mer when that is a TR k-mer of the locus, NAN32 otherwise (flank only, another locus' only, in no table).
DBTK_HD uint32_t eval_window(const uint32_t* pk, const uint16_t* vd, uint32_t j, uint32_t k, const EvalTables& T, uint32_t locus, bool* valid) {
    const uint64_t km = window_kmer(pk, vd, j, k, nullptr, nullptr);
    *valid = km != NAN64;
    if (km == NAN64) return NAN32;
    uint32_t c = kl_lookup(T.cls, T.cls_mask, T.cls_shift, km, locus);
    if (c == CLS_FLANK) c = kl_lookup(T.both, T.both_mask, T.both_shift, km, locus);
    return c == CLS_NONE ? NAN32 : c;
}

// ---- sums: eight exact integers per locus; `ok` turns false, and stays false, once a product or a sum leaves 64 bits
struct EvalSums {
    uint64_t n1, Sx, Sy, Sy1, Sxy, Sxx, Syy, Syy1;
};
DBTK_HD bool eval_add(uint64_t* a, uint64_t b) { return !__builtin_add_overflow(*a, b, a); }
DBTK_HD bool eval_term(EvalSums& s, uint64_t x, uint64_t y) {
    uint64_t xy = 0, xx = 0, yy = 0;
    bool ok = !__builtin_mul_overflow(x, y, &xy);
    ok &= !__builtin_mul_overflow(x, x, &xx);
    ok &= !__builtin_mul_overflow(y, y, &yy);
    ok &= eval_add(&s.Sx, x);
    ok &= eval_add(&s.Sy, y);
    ok &= eval_add(&s.Sxy, xy);
    ok &= eval_add(&s.Sxx, xx);
    ok &= eval_add(&s.Syy, yy);
    if (x) {
        ++s.n1;
        ok &= eval_add(&s.Sy1, y);
        ok &= eval_add(&s.Syy1, yy);
    }
    return ok;
}
DBTK_HD bool eval_merge(EvalSums& a, const EvalSums& b) {
    bool ok = eval_add(&a.n1, b.n1);
    ok &= eval_add(&a.Sx, b.Sx);
    ok &= eval_add(&a.Sy, b.Sy);
    ok &= eval_add(&a.Sy1, b.Sy1);
    ok &= eval_add(&a.Sxy, b.Sxy);
    ok &= eval_add(&a.Sxx, b.Sxx);
    ok &= eval_add(&a.Syy, b.Syy);
    ok &= eval_add(&a.Syy1, b.Syy1);
    return ok;
}
// The share of lane `lane` of `nlanes` in the locus whose k-mers are [b, e): every nlanes-th of them (consecutive lanes read
// consecutive k-mers: 8 + 8 bytes per lane, coalesced).
DBTK_HD bool eval_locus_part(const uint64_t* x, const uint64_t* y, uint64_t b, uint64_t e, uint32_t lane, uint32_t nlanes, EvalSums* out) {
    EvalSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = true;
    for (uint64_t i = b + lane; i < e; i += nlanes) ok &= eval_term(s, x[i], y[i]);
    *out = s;
    return ok;
}

}  // namespace dbtk
#endif
