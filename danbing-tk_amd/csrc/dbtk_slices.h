// dbtk_slices.h — how dbtk_align_batch_device cuts one large device batch into slices of whole pairs (dbtk_hip.hip: each slice is
// enqueued as the complete batch it is, slices alternating between two streams, so that one slice's encode kernel runs beside the
// slice before's probe and resolve kernels).  Host only, no HIP: the library and a stand-alone sanitizer program
// (tests/slice_plan_check.cpp) include it.
#ifndef DBTK_SLICES_H_
#define DBTK_SLICES_H_

#include <stdint.h>

#include <vector>

namespace dbtk_slices {

constexpr uint64_t TILE = 16;        // pairs per tile of the encode kernel (dbtk_kernels.h: K1_TP): a slice boundary is a tile boundary
constexpr uint64_t MAX_SLICES = 64;  // per batch: a tiny forced slice on a huge batch must not enqueue thousands of launches

struct Slice { uint64_t p0, n; };    // pairs [p0, p0 + n) of the batch

// Pairs per slice for a batch of npairs: slice_pairs rounded up to whole tiles, grown until at most max_slices slices cover the
// batch.  0: the batch stays whole (slicing is off, or the batch does not hold two slices of that size).
inline uint64_t slice_size(uint64_t npairs, uint64_t slice_pairs, uint64_t max_slices = MAX_SLICES) {
    if (!slice_pairs || max_slices < 2) return 0;
    uint64_t sz = slice_pairs > ~0ull - TILE ? ~0ull / TILE * TILE : (slice_pairs + TILE - 1) / TILE * TILE;
    if (npairs / 2 < sz) return 0;
    if ((npairs + sz - 1) / sz > max_slices) sz = ((npairs + max_slices - 1) / max_slices + TILE - 1) / TILE * TILE;
    return sz;
}

// The slices of a batch, in order: contiguous, none empty, together [0, npairs); every slice but the last has slice_size() pairs (a
// multiple of TILE), the last one the rest.  A batch that stays whole is one slice; an empty batch has none.
inline std::vector<Slice> plan(uint64_t npairs, uint64_t slice_pairs, uint64_t max_slices = MAX_SLICES) {
    std::vector<Slice> out;
    if (!npairs) return out;
    const uint64_t sz = slice_size(npairs, slice_pairs, max_slices);
    if (!sz) { out.push_back(Slice{0, npairs}); return out; }
    for (uint64_t p0 = 0; p0 < npairs; p0 += sz) out.push_back(Slice{p0, npairs - p0 < sz ? npairs - p0 : sz});
    return out;
}

// ---- the decision without DBTK_SLICE_PAIRS: were the launches before WGS-like?  A context keeps two sets of hint words, one that
// whole batches report to and one that slices report to (a slice reports its own survivors, 1/S of a batch's, and which launch a word
// came from cannot be told afterwards), and reads the set of the kind it launched last.
constexpr uint32_t NO_HINT = 0xFFFFFFFFu;
struct Hint { uint32_t surv, took, flag; };  // survivors | pairs the lean probe kernel took | "the list was sorted", of a launch of `of` pairs

// The launch's survivors scaled to a batch of npairs (NO_HINT or of = 0: unknown, "many").
inline uint64_t scaled_survivors(Hint h, uint64_t of, uint64_t npairs) {
    if (h.surv == NO_HINT || !of) return ~0ull;
    return (uint64_t)h.surv * npairs / of;  // (both below 2^32)
}
// WGS-like: the list was not sorted, and a batch of npairs would have fewer survivors than a sorted list has (sort_min_per_locus ·
// nloci / 2 per batch) and fewer than half its pairs (the encode stage is not lazy).  No hint: not WGS-like.
inline bool wgs_like(Hint h, uint64_t of, uint64_t npairs, uint64_t nloci, uint64_t sort_min_per_locus) {
    if (h.flag) return false;
    const uint64_t est = scaled_survivors(h, of, npairs);
    return est != ~0ull && 2 * est < sort_min_per_locus * nloci && 2 * est < npairs;
}
// The hint words the first slices of sz pairs read when a context goes from whole batches to slices: the whole batch's, scaled down.
inline Hint seed_slice_hint(Hint whole, uint64_t of, uint64_t sz) {
    const uint64_t took = whole.took < whole.surv ? whole.took : whole.surv;
    return Hint{(uint32_t)((uint64_t)whole.surv * sz / of), (uint32_t)(took * sz / of), 0u};
}
// One step of a context's state.  sliced: the batches before were cut.  Returns whether this batch is cut; *reseed: the context goes
// from whole batches to slices (seed the slices' words); *forget: it goes back (the whole batches' words are "no hint" again until a
// whole batch has reported, so a stale "WGS-like" does not send it straight back).
inline bool decide(bool sliced, Hint h, uint64_t of, uint64_t npairs, uint64_t nloci, uint64_t sort_min_per_locus, bool* reseed, bool* forget) {
    const bool wgs = wgs_like(h, of, npairs, nloci, sort_min_per_locus);
    *reseed = wgs && !sliced;
    *forget = !wgs && sliced;
    return wgs;
}

}  // namespace dbtk_slices
#endif
