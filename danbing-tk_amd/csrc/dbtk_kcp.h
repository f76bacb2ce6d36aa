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

}  // namespace dbtk
#endif
