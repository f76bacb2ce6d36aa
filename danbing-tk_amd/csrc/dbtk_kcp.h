// dbtk_kcp.h — the k-mer count profile table of --bait-profile (include/dbtk_kcp.h): per (canonical k-mer, assigned locus, class)
// the exact moments of the k-mer's per-read count c over the reads assigned to the locus, in HBM:
//   n = reads that held the k-mer, sum = Σ c, sumsq = Σ c², min c, max c        (class 0: source == assigned locus, 1: any other source)
// What the reference's baitBuilder v1.pf keeps as a vector of counts per key (bait.cpp:75-81, 117-138) and reduces to min / max /
// mean / sd when it writes: the five integers give the same four numbers.
//
// Open addressing, linear probing, 40-byte slots.  A slot is claimed in the two steps of bub_insert (dbtk_bubtab.h), neither of which
// ever waits for a word another lane has yet to write:
//   1. old = CAS64(kmer, NAN64, km): the k-mer word is ours or already km — else next slot;
//   2. l = CAS32(lc1, 0, (locus + 1) | class << 31): the locus word is ours or already ours — else next slot;
//   3. atomic add on n, sum, sumsq; atomic min / max.
// Words only go empty -> value, once, so every inserter of one key stops at the same slot, and the same k-mer at two loci or in both
// classes ends in separate slots.  The host keeps the load at or under 1/2 inside a batch (dbtk_kcp.hip: kcp_room), so an insert walks
// until it finds its slot; one that has seen every slot reports failure and has added nothing.
//
// Written once, compiled twice: by hipcc for gfx950 and by the host compiler for tests/kcp_table_check.cpp (X = the accessor with
// the atomics: atomic_cas, atomic_cas32, atomic_add (32 and 64 bit), atomic_min32, atomic_max32).
#ifndef DBTK_KCP_TAB_H_
#define DBTK_KCP_TAB_H_

#include <math.h>

#include "dbtk_tables.h"

namespace dbtk {

struct KcpSlot {
    uint64_t kmer;   // NAN64 = empty (a canonical k-mer of k <= 31 bases is below 2^62)
    uint32_t lc1;    // (locus + 1) | class << 31; 0 = not yet written
    uint32_t n;      // 0 in a slot that is claimed and not yet counted: not an entry
    uint64_t sum;
    uint64_t sumsq;
    uint32_t mn;     // ~0 in a fresh slot
    uint32_t mx;
};
static_assert(sizeof(KcpSlot) == 40, "five counters behind a 12-byte key");

constexpr KcpSlot KCP_EMPTY = {NAN64, 0u, 0u, 0ull, 0ull, 0xFFFFFFFFu, 0u};
// 64-bit words beside the table: slots taken | sticky "an insert found no slot" | first occurrences inserted
constexpr int KCP_W_OCC = 0, KCP_W_FAIL = 1, KCP_W_INS = 2, KCP_WORDS = 3;

DBTK_HD uint32_t kcp_lc1(uint32_t locus, uint32_t cls) { return (locus + 1u) | (cls << 31); }
DBTK_HD bool kcp_is_entry(const KcpSlot& s) { return s.kmer != NAN64 && s.lc1 != 0 && s.n != 0; }

// The canonical k-mer that starts at base `pos` of seq[0, len), NAN64 when the window leaves the read or holds a byte other than
// upper-case ACGT — the k-mers of read2kmers / buildNuKmers (kmer.hpp:95-200), position by position.
DBTK_HD uint64_t kcp_kmer_at(const uint8_t* seq, uint32_t len, uint32_t pos, uint32_t k) {
    if (len < k || pos > len - k) return NAN64;
    uint64_t fw = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const uint8_t c = seq[pos + i];
        const uint32_t code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
        if (code == 4u) return NAN64;
        fw = (fw << 2) | code;
    }
    const uint64_t rc = revcomp2(fw, k);
    return fw < rc ? fw : rc;
}

// The multiplicity step: how often km[pos] occurs in km[0, n), and whether pos is its first occurrence (the position that inserts).
// A NAN64 hole counts nothing.  Quadratic over a read's <= 236 positions.
DBTK_HD void kcp_multiplicity(const uint64_t* km, uint32_t n, uint32_t pos, uint32_t* count, bool* first) {
    const uint64_t v = km[pos];
    uint32_t c = 0, before = 0;
    if (v != NAN64)
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t eq = km[j] == v;
            c += eq;
            before += eq & (uint32_t)(j < pos);
        }
    *count = c;
    *first = c != 0 && before == 0;
}

// profile[(km, lc1)] gains n observations with these moments.  false: every slot was looked at and none was the key's (nothing was
// added).  `claimed` counts the empty slots this lane took.  (The plain loads are hints: a stale "empty" only sends the lane to the
// CAS, which decides.)
template <class X>
DBTK_HD bool kcp_insert(X& x, KcpSlot* tab, uint64_t mask, uint32_t shift, uint64_t km, uint32_t lc1, uint32_t n, uint64_t sum, uint64_t sumsq,
                        uint32_t mn, uint32_t mx, uint32_t& claimed) {
    uint64_t i = hash_cls(km, lc1, shift);
    for (uint64_t p = 0; p <= mask; ++p, i = (i + 1) & mask) {
        KcpSlot* s = tab + i;
        uint64_t old = s->kmer;
        if (old == NAN64) {
            old = x.atomic_cas(&s->kmer, NAN64, km);
            if (old == NAN64) { ++claimed; old = km; }
        }
        if (old != km) continue;
        uint32_t l = s->lc1;
        if (l == 0) {
            l = x.atomic_cas32(&s->lc1, 0u, lc1);
            if (l == 0) l = lc1;
        }
        if (l != lc1) continue;
        x.atomic_add(&s->n, n);
        x.atomic_add(&s->sum, sum);
        x.atomic_add(&s->sumsq, sumsq);
        x.atomic_min32(&s->mn, mn);
        x.atomic_max32(&s->mx, mx);
        return true;
    }
    return false;
}

// One slot of the old table into the new one (growth by doubling): all five counters move.
template <class X>
DBTK_HD bool kcp_move(X& x, const KcpSlot& s, KcpSlot* tab, uint64_t mask, uint32_t shift, uint32_t& claimed) {
    if (!kcp_is_entry(s)) return true;
    return kcp_insert(x, tab, mask, shift, s.kmer, s.lc1, s.n, s.sum, s.sumsq, s.mn, s.mx, claimed);
}

// MEAN and SD as the profile files print them: sum / n, and sqrt((n * sumsq - sum^2) / n^2) with the numerator exact.
inline double kcp_mean(const KcpSlot& s) { return (double)s.sum / (double)s.n; }
inline double kcp_sd(const KcpSlot& s) {
    const unsigned __int128 num = (unsigned __int128)s.n * s.sumsq - (unsigned __int128)s.sum * s.sum;
    return sqrt((double)num / ((double)s.n * (double)s.n));
}

// ---- The statistics as `ktools fps` / baitBuilder v2 (bait.cpp:177-220) see them: not the moments but the floats strtof makes of the
// "%.4f" text of MEAN and SD.  From a slot's integers, without text, bit for bit; for the host and for the device (no 128-bit division
// or conversion: the device has no runtime support for either).

// The integer whose digits snprintf("%.4f", v) prints, 0 <= v < 2^32 / 10^4: v * 10^4 rounded to nearest on the exact binary value of
// v, ties to even (1/32 prints 0.0312, 3/32 prints 0.0938).  t + r is the product exactly (r: the rounding error of t, from one fma).
// t, floor(t) and 0.5 are multiples of ulp(t), so t - floor(t) - 0.5 is zero or at least ulp(t) away from it — more than
// |r| <= ulp(t) / 2 — and its sign (which the subtractions keep) decides alone; where it is zero the sign of r decides, and r == 0 is
// the tie.
DBTK_HD uint32_t kcp_dec4(double v) {
    const double t = v * 1e4, r = fma(v, 1e4, -t);
    const double f = floor(t), d = t - f - 0.5;
    const uint32_t D = (uint32_t)f;
    if (d != 0.0) return d > 0.0 ? D + 1u : D;
    if (r != 0.0) return r > 0.0 ? D + 1u : D;
    return D + (D & 1u);
}
// strtof of those digits with the point four places in: D < 2^24 is a float, 10^4 is one, and IEEE division rounds the exact quotient
// once, which is what strtof does to the decimal number.
DBTK_HD float kcp_text_float(uint32_t D) { return (float)D / 10000.0f; }

DBTK_HD void kcp_mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
    *lo = a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    *hi = (uint64_t)(p >> 64);
    *lo = (uint64_t)p;
#endif
}
// (double)(hi * 2^64 + lo), rounded once: the 64 leading bits, whatever lies below them ORed into bit 0 (eleven places under the bit
// that rounds), converted and scaled.
DBTK_HD double kcp_u128_to_double(uint64_t hi, uint64_t lo) {
    if (!hi) return (double)lo;
    const int sh = __builtin_clzll(hi);
    uint64_t m = hi, lost = 0;
    if (sh) { m = (hi << sh) | (lo >> (64 - sh)); lost = lo << sh; } else lost = lo;
    if (lost) m |= 1ull;
    return ldexp((double)m, 64 - sh);
}

DBTK_HD float kcp_mean_text(const KcpSlot& s) { return kcp_text_float(kcp_dec4((double)s.sum / (double)s.n)); }
// kcp_sd's value: the numerator n * sumsq - sum^2 exact in two words (it can pass 2^64), rounded to double once
DBTK_HD float kcp_sd_text(const KcpSlot& s) {
    uint64_t ahi, alo, bhi, blo;
    kcp_mul64((uint64_t)s.n, s.sumsq, &ahi, &alo);
    kcp_mul64(s.sum, s.sum, &bhi, &blo);
    const uint64_t lo = alo - blo, hi = ahi - bhi - (uint64_t)(alo < blo);
    return kcp_text_float(kcp_dec4(sqrt(kcp_u128_to_double(hi, lo) / ((double)s.n * (double)s.n))));
}
// testAndFilter's test (bait.cpp:196-203), in float as the reference evaluates it: the FP mean inside the TP profile's mean +- 2 sd
DBTK_HD bool kcp_fps_inside(float fp_mean, float tp_mean, float tp_sd) {
    const float w = 2.0f * tp_sd;
    return tp_mean - w <= fp_mean && fp_mean <= tp_mean + w;
}

// A candidate of the FP-specific filter (dbtk_kcp_fps_*): what stays of an FP entry, and beside it its one mutable word.
struct KcpCand { uint64_t kmer; uint32_t locus; float mean; };
static_assert(sizeof(KcpCand) == 16, "a candidate is one 16-byte load");
constexpr uint32_t KCP_CAND_ALIVE = 1u << 16;  // state = mi | ma << 8 | alive << 16; fresh: 255 | 0 << 8 | alive
DBTK_HD uint32_t kcp_cand_fresh() { return 255u | KCP_CAND_ALIVE; }

// One candidate against one quiescent TP table: the walk from hash_cls ends at an empty k-mer word (absent: state unchanged) or at
// the entry (k-mer, locus, class 0).  Inside mean +- 2 sd: dead for good (0).  Outside: (mi, ma) becomes the entry's (min, max) where
// mi is still 255, else widens by it.  The table is only read.
DBTK_HD uint32_t kcp_fps_step(const KcpSlot* tab, uint64_t mask, uint32_t shift, const KcpCand& c, uint32_t state) {
    const uint32_t lc1 = kcp_lc1(c.locus, 0u);
    uint64_t i = hash_cls(c.kmer, lc1, shift);
    for (uint64_t p = 0; p <= mask; ++p, i = (i + 1) & mask) {
        const KcpSlot s = tab[i];
        if (s.kmer == NAN64) return state;
        if (s.kmer != c.kmer || s.lc1 != lc1 || s.n == 0) continue;
        if (kcp_fps_inside(c.mean, kcp_mean_text(s), kcp_sd_text(s))) return 0u;
        uint32_t mi = state & 255u, ma = (state >> 8) & 255u;
        const uint32_t tmi = s.mn & 255u, tma = s.mx & 255u;  // (uint8_t in the reference; a count per read is at most 236)
        if (mi == 255u) { mi = tmi; ma = tma; }
        else { mi = tmi < mi ? tmi : mi; ma = tma > ma ? tma : ma; }
        return mi | (ma << 8) | KCP_CAND_ALIVE;
    }
    return state;
}

}  // namespace dbtk
#endif
