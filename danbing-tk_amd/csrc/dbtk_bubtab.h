// dbtk_bubtab.h — the device table of novel edges (params.bubbles = DBTK_BUBBLES_TABLE): (locus, edge) -> uint32 count in HBM,
// filled by the general resolve kernel (dbtk_kernels.h: body_pair<NS, RECS, true>) instead of the event log of params.bubbles = 1.
//
// Open addressing, linear probing, 16-byte slots.  The key is 96 bits (a (k+1)-mer of up to 64 bits and the locus) and there is no
// 128-bit atomic, so a slot is claimed in two steps, neither of which ever waits for another lane (a lane that spun on a word a
// lane of its own wave has yet to write would wait for ever):
//   1. old = CAS64(edge, NAN64, e): the slot's edge word is ours (old == NAN64) or already e (old == e) — else next slot;
//   2. l = CAS32(locus1, 0, locus + 1): the slot's locus is ours (l == 0) or already ours (l == locus + 1) — else next slot;
//   3. atomic add on the count.
// Every lane that passes step 1 goes straight on to step 2, so a slot whose edge word is set gets a locus from SOME inserter of that
// edge; the loser of step 2 (the same edge at another locus) simply moves on.  Words only ever go empty -> value, once: the slots a
// key passes on its way stay "not mine" for ever, so every inserter of one key stops at the same slot and a key never has two.
// The same edge at two loci therefore ends in two slots, each with its exact count (DESIGN: the plain-C++ model).
#ifndef DBTK_BUBTAB_H_
#define DBTK_BUBTAB_H_

namespace dbtk {

struct BubSlot {
    uint64_t edge;    // NAN64 = empty (a read (k+1)-mer with a non-ACGT base is NAN64 and is never counted)
    uint32_t locus1;  // locus + 1; 0 = not yet written
    uint32_t count;
};
static_assert(sizeof(BubSlot) == 16, "two slots per 32-byte sector");

// slots an insert looks at before it gives up (a table kept under half full has no run that long; one that filled up inside a
// batch sends the insert to the spill log instead of walking the whole table)
constexpr uint32_t BUB_PROBE_MAX = 128;
// words beside the table (dbtk_ctx::d_nevents): entries in the spill log | slots taken | sticky "the spill log overflowed" |
// inserts of a rehash / list insert that found no slot
constexpr int BUB_W_SPILL = 0, BUB_W_OCC = 1, BUB_W_OVF = 2, BUB_W_FAIL = 3, BUB_WORDS = 4;

// count[(locus, e)] += n.  false: no slot within BUB_PROBE_MAX (nothing was added).  `claimed` counts the empty slots this lane took.
// (The plain loads are hints: a stale "empty" only sends the lane to the CAS, which decides.)
template <class X>
DBTK_HD bool bub_insert(X& x, BubSlot* tab, uint64_t mask, uint32_t shift, uint64_t e, uint32_t locus, uint32_t n, uint32_t& claimed) {
    uint64_t i = hash_cls(e, locus, shift);
    const uint32_t l1 = locus + 1;
    const uint32_t lim = mask + 1 < BUB_PROBE_MAX ? (uint32_t)(mask + 1) : BUB_PROBE_MAX;
    for (uint32_t p = 0; p < lim; ++p, i = (i + 1) & mask) {
        BubSlot* s = tab + i;
        uint64_t old = s->edge;
        if (old == NAN64) {
            old = x.atomic_cas(&s->edge, NAN64, e);
            if (old == NAN64) { ++claimed; old = e; }
        }
        if (old != e) continue;
        uint32_t l = s->locus1;
        if (l == 0) {
            l = x.atomic_cas32(&s->locus1, 0u, l1);
            if (l == 0) l = l1;
        }
        if (l != l1) continue;
        x.atomic_add(&s->count, n);
        return true;
    }
    return false;
}

}  // namespace dbtk
#endif
