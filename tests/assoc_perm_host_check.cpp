// assoc_perm_host_check.cpp — the host half of the permutation p-values of the association scan (csrc/dbtk_assoc_perm_host.h)
// stand-alone: built with -fsanitize=address,undefined and run by tests/test_assoc_perm_host.py.  The generator (its first values
// against the published splitmix64 stream, prefixes, n = 1 and 2), the validation of bad rows, p_perm and the fold at its edges.
// Prints "ok" and returns 0, or the first failed check and 1.
#include <stdio.h>

#include <string>
#include <vector>

#include "dbtk_assoc_perm_host.h"

using namespace dbtk_assoc_host;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    {   // splitmix64 from seed 0: the reference values of the published generator
        SplitMix64 g{0};
        CHECK(g.next() == 0xE220A8397B1DCDAFull);
        CHECK(g.next() == 0x6E789E6AA1B965F4ull);
        CHECK(g.next() == 0x06C45D188009454Full);
    }
    for (uint64_t n : {1, 2, 3, 7, 64, 1100})
        for (uint64_t B : {1, 2, 9})
            for (uint64_t seed : {0ull, 1ull, 0xFFFFFFFFFFFFFFFFull}) {
                std::vector<uint32_t> p(B * n, 77u), q((B + 3) * n, 78u);
                perm_generate(n, B, seed, p.data());
                perm_generate(n, B + 3, seed, q.data());
                uint64_t bad = 99;
                CHECK(perm_valid(n, B, p.data(), &bad) && bad == 99);
                CHECK(std::equal(p.begin(), p.end(), q.begin()));   // the first B rows of a longer run
                if (n == 1) CHECK(p[0] == 0);
            }
    {   // n = 2: the one draw per permutation is the top bit of the stream's value
        SplitMix64 g{5};
        std::vector<uint32_t> p(8 * 2);
        perm_generate(2, 8, 5, p.data());
        for (int b = 0; b < 8; ++b) {
            const uint64_t j = g.next() >> 63;   // (next() * 2) >> 64
            CHECK(p[2 * b + 1] == (j == 1 ? 1u : 0u) && p[2 * b] == (j == 1 ? 0u : 1u));
        }
    }
    {   // different seeds differ
        std::vector<uint32_t> a(3 * 64), b(3 * 64);
        perm_generate(64, 3, 1, a.data());
        perm_generate(64, 3, 2, b.data());
        CHECK(a != b);
    }
    {   // rows that are no permutations: the first one is named
        const uint64_t n = 5;
        std::vector<uint32_t> p(4 * n);
        perm_generate(n, 4, 3, p.data());
        uint64_t bad = 99;
        std::vector<uint32_t> x = p;
        x[2 * n + 1] = x[2 * n + 3];                  // a value twice
        CHECK(!perm_valid(n, 4, x.data(), &bad) && bad == 2);
        x = p; x[3 * n] = (uint32_t)n;                 // off the end
        CHECK(!perm_valid(n, 4, x.data(), &bad) && bad == 3);
        x = p; x[0] = 0xFFFFFFFFu; x[3 * n] = 9;      // two bad rows: the first
        CHECK(!perm_valid(n, 4, x.data(), &bad) && bad == 0);
        CHECK(perm_valid(n, 0, nullptr, &bad));
        CHECK(perm_valid(0, 0, nullptr, &bad));
    }
    {   // p_perm and the fold: B = 1; ties count as >=; a phenotype without tests; Benjamini-Hochberg over the others
        CHECK(perm_pvalue(0, 1) == 0.5 && perm_pvalue(1, 1) == 1.0 && perm_pvalue(0, 999) == 1.0 / 1000.0 && perm_pvalue(999, 999) == 1.0);
        const double t1[2] = {0.5, 0.5}, t2[2] = {0.5, 0.25};
        CHECK(perm_count_ge(t1, 1) == 1 && perm_count_ge(t2, 1) == 0);
        const uint64_t P = 4, B = 3;
        const double T[P * (B + 1)] = {0.9, 0.1, 0.2, 0.3,   0.0, 0.0, 0.0, 0.0,   0.4, 0.4, 0.5, 0.1,   0.2, 0.9, 0.9, 0.9};
        const uint8_t has[P] = {1, 0, 1, 1};
        uint64_t n_ge[P];
        double pp[P], qq[P];
        perm_fold(P, B, T, has, n_ge, pp, qq);
        CHECK(n_ge[0] == 0 && n_ge[1] == 0 && n_ge[2] == 2 && n_ge[3] == 3);
        CHECK(pp[0] == 0.25 && pp[1] == 0.0 && pp[2] == 0.75 && pp[3] == 1.0);
        CHECK(qq[0] == 0.75 && qq[1] == 0.0 && qq[2] == 1.0 && qq[3] == 1.0);   // 0.25 * 3 / 1, 0.75 * 3 / 2 clipped, 1
        perm_fold(0, B, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    {   // the seed's text
        uint64_t v = 0;
        CHECK(whole_u64("18446744073709551615", &v) && v == 0xFFFFFFFFFFFFFFFFull);
        CHECK(whole_u64("0", &v) && v == 0);
        CHECK(!whole_u64("18446744073709551616", &v) && !whole_u64("", &v) && !whole_u64("-1", &v) && !whole_u64("1e3", &v) && !whole_u64("99999999999999999999", &v));
    }
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}
