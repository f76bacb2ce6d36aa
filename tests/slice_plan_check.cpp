// slice_plan_check.cpp — the slice plan of dbtk_align_batch_device (danbing-tk_amd/csrc/dbtk_slices.h) under the address and
// undefined-behaviour sanitizers: a stand-alone program, built and run by tests/test_slice_plan.py.
//   slice_plan_check                  every property below over the grid of batch sizes and slice sizes; prints "slice planning ok"
//   slice_plan_check NPAIRS SLICE     prints the number of slices of that batch (what tests/test_slices.py expects the launcher to enqueue)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dbtk_slices.h"

using dbtk_slices::Slice;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++fails; } } while (0)

// the properties of every plan; returns the number of slices
static uint64_t check_plan(uint64_t npairs, uint64_t slice, uint64_t max_slices) {
    const std::vector<Slice> p = dbtk_slices::plan(npairs, slice, max_slices);
    const uint64_t sz = dbtk_slices::slice_size(npairs, slice, max_slices);
    uint64_t at = 0;
    for (size_t i = 0; i < p.size(); ++i) {
        CHECK(p[i].p0 == at, "npairs %llu slice %llu: slice %zu begins at %llu, not %llu", (unsigned long long)npairs, (unsigned long long)slice, i, (unsigned long long)p[i].p0, (unsigned long long)at);
        CHECK(p[i].n > 0, "npairs %llu slice %llu: slice %zu is empty", (unsigned long long)npairs, (unsigned long long)slice, i);
        if (i + 1 < p.size()) {
            CHECK(p[i].n % 16 == 0, "npairs %llu slice %llu: slice %zu of %llu pairs", (unsigned long long)npairs, (unsigned long long)slice, i, (unsigned long long)p[i].n);
            CHECK(p[i].n == sz, "npairs %llu slice %llu: slice %zu of %llu pairs, slice_size %llu", (unsigned long long)npairs, (unsigned long long)slice, i, (unsigned long long)p[i].n, (unsigned long long)sz);
        } else CHECK(p.size() == 1 || p[i].n <= sz, "npairs %llu slice %llu: last slice of %llu pairs", (unsigned long long)npairs, (unsigned long long)slice, (unsigned long long)p[i].n);
        at += p[i].n;
    }
    CHECK(at == npairs, "npairs %llu slice %llu: the slices hold %llu pairs", (unsigned long long)npairs, (unsigned long long)slice, (unsigned long long)at);
    CHECK(p.size() <= max_slices || p.size() == 1, "npairs %llu slice %llu: %zu slices", (unsigned long long)npairs, (unsigned long long)slice, p.size());
    CHECK((npairs == 0) == p.empty(), "npairs %llu: %zu slices", (unsigned long long)npairs, p.size());
    CHECK((sz == 0) == (p.size() <= 1), "npairs %llu slice %llu: slice_size %llu, %zu slices", (unsigned long long)npairs, (unsigned long long)slice, (unsigned long long)sz, p.size());
    // fewer than two full slices of the configured size (whole tiles): the batch stays whole
    const uint64_t conf = slice > (1ull << 40) ? 1ull << 40 : (slice + 15) / 16 * 16;  // (no batch has 2^40 pairs)
    if (slice && npairs < 2 * conf) CHECK(p.size() <= 1, "npairs %llu slice %llu: cut into %zu", (unsigned long long)npairs, (unsigned long long)slice, p.size());
    if (slice && max_slices >= 2 && npairs >= 2 * conf) CHECK(p.size() >= 2, "npairs %llu slice %llu: not cut", (unsigned long long)npairs, (unsigned long long)slice);
    return p.size();
}

int main(int argc, char** argv) {
    if (argc == 3) {
        printf("%zu\n", dbtk_slices::plan(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10)).size());
        return 0;
    }
    const uint64_t sizes[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 95, 96, 97, 200, 1023, 1024, 1025, 64 * 16, 64 * 16 + 1, 65 * 16, (1ull << 20) - 1, 1ull << 20,
                              (1ull << 21) - 1, 1ull << 21, (1ull << 21) + 1, 5000000, (1ull << 32) - 2};
    const uint64_t slices[] = {0, 1, 16, 48, 1ull << 19, 1ull << 20, 1ull << 21, ~0ull};
    for (uint64_t n : sizes)
        for (uint64_t s : slices)
            for (uint64_t m : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, dbtk_slices::MAX_SLICES}) check_plan(n, s, m);
    // the cases spelled out
    CHECK(check_plan(16, 16, 64) == 1 && check_plan(17, 16, 64) == 1 && check_plan(31, 16, 64) == 1, "fewer than two slices of 16");
    CHECK(check_plan(32, 16, 64) == 2 && check_plan(47, 16, 64) == 3 && check_plan(48, 16, 64) == 3 && check_plan(49, 16, 64) == 4, "slices of 16");
    CHECK(dbtk_slices::plan(49, 16).back().n == 1, "a last slice of one pair");
    CHECK(check_plan(200, 16, 64) == 13 && check_plan(200, 48, 64) == 5 && check_plan(95, 48, 64) == 1 && check_plan(97, 48, 64) == 3, "slices of 16 and 48");
    CHECK(check_plan(200, 1, 64) == 13, "a slice of one pair is one tile");
    // the cap: 64 slices of 16 pairs hold 1024; one pair more and the slice grows by a tile
    CHECK(check_plan(1024, 16, 64) == 64 && dbtk_slices::slice_size(1024, 16) == 16, "64 slices");
    CHECK(check_plan(1025, 16, 64) == 33 && dbtk_slices::slice_size(1025, 16) == 32, "the slice grows past 64 slices");
    CHECK(check_plan((1ull << 32) - 2, 1, 64) == 64 && check_plan((1ull << 32) - 2, 1ull << 20, 64) == 64, "the cap on the largest batch");
    CHECK(dbtk_slices::slice_size((1ull << 32) - 2, 1ull << 20) == 1ull << 26, "2^32 - 2 pairs: 64 slices of 2^26");
    // the headline batch at the three sizes measured
    CHECK(check_plan(5000000, 1ull << 19, 64) == 10 && check_plan(5000000, 1ull << 20, 64) == 5 && check_plan(5000000, 1ull << 21, 64) == 3, "5 M pairs");
    // ... and under the cap of two slices the library sets itself without DBTK_SLICE_PAIRS (one slice per stream): halves, whatever
    // the smallest slice, from twice the smallest slice on
    for (uint64_t s : {1ull << 19, 1ull << 20, 1ull << 21}) {
        CHECK(check_plan(5000000, s, 2) == 2 && dbtk_slices::slice_size(5000000, s, 2) == 2500000, "5 M pairs in halves");
        CHECK(check_plan(2 * s - 1, s, 2) == 1 && check_plan(2 * s, s, 2) == 2 && check_plan(2 * s + 1, s, 2) == 2, "cut from two slices on");
        CHECK(dbtk_slices::plan(2 * s + 1, s, 2).back().n == s - 15, "2 s + 1 pairs: s + 16 and the rest");
    }
    // ---- the decision without the override (dbtk_slices::decide): release scale, 80 000 loci, sort threshold 4 per locus = 160 000
    // survivors per batch; the headline batch has 5 M pairs and ~100 000 survivors
    {
        using dbtk_slices::Hint; using dbtk_slices::NO_HINT;
        const uint64_t NL = 80000, SM = 4, B = 5000000, H = 2500000;
        bool reseed, forget;
        auto dec = [&](bool sliced, Hint h, uint64_t of, uint64_t np) { return dbtk_slices::decide(sliced, h, of, np, NL, SM, &reseed, &forget); };
        // a fresh context (no hint, flag set): whole, and stays whole
        CHECK(!dec(false, Hint{NO_HINT, NO_HINT, 1}, 0, B) && !reseed && !forget, "no hint");
        CHECK(!dec(false, Hint{NO_HINT, NO_HINT, 0}, B, B) && !dec(false, Hint{100000, 100000, 0}, 0, B), "no survivors known, or no launch size");
        // the whole headline batch has reported: cut, and the slices' words are seeded with a half's share
        CHECK(dec(false, Hint{100000, 100000, 0}, B, B) && reseed && !forget, "WGS-like whole batch");
        const Hint s = dbtk_slices::seed_slice_hint(Hint{100000, 100000, 0}, B, H);
        CHECK(s.surv == 50000 && s.took == 50000 && s.flag == 0, "seed: %u %u %u", s.surv, s.took, s.flag);
        CHECK(dbtk_slices::seed_slice_hint(Hint{100000, NO_HINT, 0}, B, H).took == 50000, "seed: took is at most the survivors");
        // steady state in halves: a half reports 50 000 of 2.5 M, scaled to the batch 100 000: still cut, nothing changes
        CHECK(dec(true, s, H, B) && !reseed && !forget, "halves stay");
        CHECK(dbtk_slices::scaled_survivors(s, H, B) == 100000, "a half's survivors scaled to the batch");
        // unscaled, a half of a batch at the threshold would look WGS-like for ever: 90 000 of a half are 180 000 of the batch
        CHECK(!dec(true, Hint{90000, 90000, 0}, H, B) && forget && !reseed, "dense halves go back to whole batches");
        CHECK(dec(true, Hint{79999, 79999, 0}, H, B) && !dec(true, Hint{80000, 80000, 0}, H, B), "the sort's threshold, per batch");
        // a sorted launch (all-hit, genome-like) is never WGS-like, whatever its count; nor is a batch most of which survives (lazy K1)
        CHECK(!dec(false, Hint{100000, 100000, 1}, B, B) && !reseed, "sorted whole batches are never cut");
        CHECK(!dec(true, Hint{10, 10, 1}, H, B) && forget, "a sorted slice sends the context back");
        CHECK(!dbtk_slices::wgs_like(Hint{600, 600, 0}, 1000, 1000, 1000000, SM), "more than half survive");
        CHECK(dbtk_slices::wgs_like(Hint{499, 499, 0}, 1000, 1000, 1000000, SM) && !dbtk_slices::wgs_like(Hint{500, 500, 0}, 1000, 1000, 1000000, SM), "half the pairs");
        // batches of another size than the launch that reported: the same density decides
        CHECK(dec(false, Hint{100000, 100000, 0}, B, 2 * B) == false && dec(false, Hint{100000, 100000, 0}, B, B / 2), "scaled to this call's pairs");
        // the largest words do not overflow: 2^32 - 2 survivors of 2^32 - 2 pairs, scaled to 2^32 - 2
        CHECK(dbtk_slices::scaled_survivors(Hint{0xFFFFFFFEu, 0, 0}, 0xFFFFFFFEull, 0xFFFFFFFEull) == 0xFFFFFFFEull, "no overflow");
    }
    if (fails) return 1;
    printf("slice planning ok\n");
    return 0;
}
