// Stand-alone check of the window planning (danbing-tk_amd/csrc/dbtk_pred_plan.h), built with -fsanitize=address,undefined and run
// on the CPU by tests/test_pred_window_host.py.  Every array is a heap allocation of exactly its size, so that a read past either
// end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dbtk_pred_plan.h"

namespace pl = dbtk_pred_plan;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// walks all windows; checks that they tile [0, ntr) and [0, nk) and that each is maximal
static uint64_t walk(const std::vector<uint32_t>& sizes, uint64_t tail, uint64_t max_rows) {
    const uint64_t ntr = sizes.size();
    uint32_t* cum = (uint32_t*)malloc(ntr * sizeof(uint32_t));
    uint64_t nk = 0;
    for (uint64_t t = 0; t < ntr; ++t) { nk += sizes[t]; cum[t] = (uint32_t)nk; }
    nk += tail;
    uint64_t first = 0, next_row = 0, n = 0, end, row0, rows;
    while (first < ntr) {
        if (!pl::window(cum, ntr, nk, max_rows, first, &end, &row0, &rows)) { CHECK(end == first); n = 0; break; }
        CHECK(end > first && end <= ntr && rows <= max_rows && row0 == next_row);
        CHECK(row0 + rows == pl::locus_end(cum, ntr, nk, end - 1));
        if (end < ntr) {  // maximal: the next locus has k-mers and does not fit
            CHECK(pl::locus_end(cum, ntr, nk, end) - row0 > max_rows);
            CHECK(pl::locus_end(cum, ntr, nk, end) > pl::locus_begin(cum, end));
        }
        next_row = row0 + rows;
        first = end;
        ++n;
    }
    if (n) CHECK(next_row == nk);
    CHECK(n == pl::count_windows(cum, ntr, nk, max_rows));
    uint64_t size = 0;
    const uint64_t big = pl::first_oversized(cum, ntr, nk, max_rows, &size);
    CHECK((big == ntr) == (n != 0));
    if (big < ntr) CHECK(size > max_rows);
    CHECK(!pl::window(cum, ntr, nk, max_rows, ntr, &end, &row0, &rows));
    CHECK(!pl::window(cum, ntr, nk, max_rows, ntr + 7, &end, &row0, &rows));
    CHECK(!pl::window(cum, ntr, nk, max_rows, ~0ull, &end, &row0, &rows));
    free(cum);
    return n;
}

int main() {
    const std::vector<uint32_t> mix = {0, 1, 2, 63, 64, 65, 7, 300, 12, 0, 0, 33, 5, 90, 0};
    uint64_t total = 0;
    for (uint32_t v : mix) total += v;
    CHECK(walk(mix, 0, 300) > 1);                 // the largest locus alone in a window somewhere
    CHECK(walk(mix, 0, 299) == 0);                // one locus too large
    CHECK(walk(mix, 0, total) == 1);              // a single window
    CHECK(walk(mix, 0, total - 1) == 2);
    CHECK(walk(mix, 0, ~0ull) == 1);
    CHECK(walk(mix, 0, 202) == 0);
    CHECK(walk(mix, 0, 514) == 2);                // 0 + 1 + 2 + 63 + 64 + 65 + 7 + 300 + 12 = 514: ends on a locus boundary, the empty loci after it included
    CHECK(walk(mix, 0, 513) == 2);                // (locus 8 no longer fits: the second window starts there)
    CHECK(walk(mix, 5, 300) > 1);                 // k-mers past the last locus travel with it
    CHECK(walk(mix, 300, 300) > 1);
    CHECK(walk(mix, 301, 300) == 0);              // ... and count towards its size
    CHECK(walk({0, 0, 0}, 0, 1) == 1);            // nothing but empty loci
    CHECK(walk({0}, 0, 1) == 1);
    CHECK(walk({1}, 0, 1) == 1);
    CHECK(walk({1, 1, 1, 1}, 0, 1) == 4);
    CHECK(walk({0, 1, 0, 0, 1, 0}, 0, 1) == 2);
    CHECK(walk({5}, 0, 0) == 0);                  // max_rows = 0 holds no locus with k-mers
    CHECK(walk({0, 0}, 0, 0) == 1);
    CHECK(walk({0xFFFFFFF0u}, 0, 0xFFFFFFF0ull) == 1);   // sizes near 2^32: the sums are 64-bit
    CHECK(walk({0x7FFFFFFFu, 0x7FFFFFFFu}, 1, 0x80000000ull) == 2);
    {   // window 2 of the mix at 514: starts after the empty loci
        uint32_t* cum = (uint32_t*)malloc(mix.size() * sizeof(uint32_t));
        uint64_t nk = 0, end, row0, rows;
        for (size_t t = 0; t < mix.size(); ++t) { nk += mix[t]; cum[t] = (uint32_t)nk; }
        CHECK(pl::window(cum, mix.size(), nk, 514, 0, &end, &row0, &rows) && end == 11 && row0 == 0 && rows == 514);
        CHECK(pl::window(cum, mix.size(), nk, 514, 11, &end, &row0, &rows) && end == mix.size() && row0 == 514 && rows == 128);
        CHECK(pl::window(cum, mix.size(), nk, 514, 9, &end, &row0, &rows) && end == mix.size() && row0 == 514 && rows == 128);   // from an empty locus
        free(cum);
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("window planning ok\n");
    return 0;
}
