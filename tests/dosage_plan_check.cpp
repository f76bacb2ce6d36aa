// Stand-alone check of the dosage tables' work list (dosage_items, danbing-tk_amd/csrc/dbtk_pred_plan.h), built with
// -fsanitize=address,undefined and run on the CPU by tests/test_pred_edges.py, as tests/pred_plan_check.cpp is for the window planning
// of the same header.  Every array is a heap allocation of exactly its size, so that a read past either end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dbtk_pred_plan.h"

namespace pl = dbtk_pred_plan;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// the dosage tables' work list (dosage_items) over the given locus sizes: the items tile the k-mer axis in order, every locus lies in
// exactly one whole-loci item or is exactly the parts fbeg[q] .. fbeg[q + 1] - 1 of one floc[q], the packing is greedy, and nlb follows
// its rules.  Returns the number of items.
static uint64_t items_of(const std::vector<uint32_t>& sizes, bool with_bias, uint64_t* max_nl = nullptr, uint64_t* nfold = nullptr) {
    const uint64_t ntr = sizes.size();
    uint32_t* cum = (uint32_t*)malloc(ntr * sizeof(uint32_t));
    uint64_t nk = 0;
    for (uint64_t t = 0; t < ntr; ++t) { nk += sizes[t]; cum[t] = (uint32_t)nk; }
    std::vector<pl::DosItem> items;
    std::vector<uint32_t> floc, fbeg;
    pl::dosage_items(ntr, cum, with_bias, &items, &floc, &fbeg);
    CHECK(fbeg.size() == floc.size() + 1 && fbeg[0] == 0);
    uint64_t next_k = 0, next_l = 0, q = 0, nparts = 0, big = 0;
    for (size_t i = 0; i < items.size(); ++i) {
        const pl::DosItem& it = items[i];
        CHECK(it.k0 == next_k && it.nkm <= (uint32_t)pl::DS_CH && it.l0 == next_l && it.l0 < ntr);
        if (it.k0 != next_k || it.l0 != next_l || it.l0 >= ntr) break;   // (what follows would read past cum)
        next_k += it.nkm;
        if (it.nl) {  // whole loci
            CHECK(it.part == pl::NOPART && it.nlb == (with_bias ? it.nl : 0u) && it.l0 + (uint64_t)it.nl <= ntr);
            if (it.l0 + (uint64_t)it.nl > ntr) break;
            CHECK(it.k0 == pl::locus_begin(cum, it.l0) && next_k == cum[it.l0 + it.nl - 1]);
            for (uint32_t j = 0; j < it.nl; ++j) CHECK(sizes[it.l0 + j] <= (uint32_t)pl::DS_CH);
            next_l += it.nl;
            if (next_l < ntr && sizes[next_l] <= (uint32_t)pl::DS_CH) CHECK((uint64_t)it.nkm + sizes[next_l] > (uint64_t)pl::DS_CH);   // greedy: the next locus did not fit
            if (max_nl && it.nl > *max_nl) *max_nl = it.nl;
        } else {      // a part of locus l0
            const uint64_t b = pl::locus_begin(cum, it.l0), e = cum[it.l0];
            const bool first = it.k0 == b, last = next_k == e;
            CHECK(sizes[it.l0] > (uint32_t)pl::DS_CH && it.part == nparts && it.nkm > 0 && next_k <= e);
            CHECK(last || it.nkm == (uint32_t)pl::DS_CH);
            CHECK(it.nlb == (with_bias && first ? 1u : 0u));
            if (first) { CHECK(q < floc.size() && floc[q] == it.l0 && fbeg[q] == nparts); }
            ++nparts;
            if (last) { CHECK(q < floc.size() && fbeg[q + 1] == nparts); ++q; ++next_l; ++big; }
        }
    }
    CHECK(next_l == ntr && next_k == (ntr ? cum[ntr - 1] : 0u) && q == floc.size() && fbeg.back() == nparts);
    if (nfold) *nfold = big;
    free(cum);
    return items.size();
}

static uint32_t lcg_state = 12345u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static void dosage_lists() {
    // the list of tests/test_pred_edges.py, case (c)
    std::vector<uint32_t> c(300, 0u);
    c.insert(c.end(), 40, 1u);
    for (int i = 0; i < 60; ++i) for (uint32_t v : {0u, 2u, 0u, 0u, 3u}) c.push_back(v);
    c.insert(c.end(), 34, 60u);
    for (uint32_t v : {2048u, 2049u, 0u, 4096u, 4097u}) c.push_back(v);
    c.insert(c.end(), 66, 2049u);
    for (uint32_t v : {5u, 0u, 0u}) c.push_back(v);
    for (bool with_bias : {true, false}) {
        uint64_t max_nl = 0, nfold = 0;
        CHECK(c.size() == 748 && items_of(c, with_bias, &max_nl, &nfold) == 144 && max_nl == 668 && nfold == 69);
    }
    CHECK(items_of({}, true) == 0);
    CHECK(items_of({0}, true) == 1);                                      // an item of an empty locus
    CHECK(items_of({0, 0, 0}, false) == 1);
    CHECK(items_of({2048}, true) == 1);
    CHECK(items_of({2049}, true) == 2);
    CHECK(items_of({2048, 1}, true) == 2);
    CHECK(items_of({0, 4096, 0}, true) == 4);                             // empty loci on both sides of a large one: an item each
    CHECK(items_of({1, 4097, 2047, 1, 1}, true) == 6);
    CHECK(items_of({0x7FFFF801u}, false) == (0x7FFFF801u + 2047u) / 2048u);   // a locus of nearly 2^31 k-mers: 32-bit offsets do not wrap
    // random lists: sizes 0 .. 5000 with runs of empty loci and many small loci between the large ones
    for (int rep = 0; rep < 4000; ++rep) {
        std::vector<uint32_t> sizes;
        const uint32_t n = lcg() % 90;
        while (sizes.size() < n) {
            const uint32_t kind = lcg() % 8;
            if (kind == 0) sizes.insert(sizes.end(), 1 + lcg() % 300, 0u);                              // a run of empty loci
            else if (kind == 1) sizes.push_back(2040 + lcg() % 20);                                   // around DS_CH
            else if (kind == 2) sizes.push_back((uint32_t)pl::DS_CH * (1 + lcg() % 2) + lcg() % 3);   // a multiple of DS_CH and its neighbours
            else if (kind <= 4) sizes.push_back(lcg() % 5001);
            else sizes.push_back(lcg() % 70);
        }
        items_of(sizes, rep % 2 == 0);
    }
}

int main() {
    dosage_lists();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("dosage work list ok\n");
    return 0;
}
