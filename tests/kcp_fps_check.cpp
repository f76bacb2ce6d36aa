// kcp_fps_check.cpp — the text-exact statistics of csrc/dbtk_kcp.h (kcp_dec4, kcp_text_float, kcp_mean_text, kcp_sd_text,
// kcp_fps_inside, kcp_fps_step) compiled for the host, under AddressSanitizer and UndefinedBehaviorSanitizer, against what they stand
// for: snprintf("%.4f") of kcp_mean / kcp_sd and strtof of that text — the floats `ktools fps` and the reference's baitBuilder v2
// compare.  Built and run by tests/test_kcp_fps_host.py; prints "kcp fps ok" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <numeric>
#include <random>
#include <vector>

#include "dbtk_kcp.h"

using namespace dbtk;

#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) {                                                            \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

// the digits "%.4f" prints, as the integer they spell without the point
static uint32_t printed(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", v);
    char* dot = strchr(buf, '.');
    CHECK(dot && strlen(dot + 1) == 4);
    return (uint32_t)(strtoull(buf, nullptr, 10) * 10000 + strtoull(dot + 1, nullptr, 10));
}
static float parsed(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", v);
    return strtof(buf, nullptr);
}
static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static KcpSlot slot(uint32_t n, uint64_t sum, uint64_t sumsq) { return KcpSlot{7, kcp_lc1(0, 0), n, sum, sumsq, 1, 1}; }

static void check_value(double v) {
    CHECK(kcp_dec4(v) == printed(v));
    CHECK(same_bits(kcp_text_float(kcp_dec4(v)), parsed(v)));
}

static void check_means() {
    // every mean of n <= 128 reads with counts 1 .. 4; the exact ties among them (sum * 10^4 / n ends in one half: round to even)
    uint32_t ties = 0;
    for (uint32_t n = 1; n <= 128; ++n)
        for (uint64_t sum = n; sum <= 4ull * n; ++sum) {
            const KcpSlot s = slot(n, sum, sum * 4);
            CHECK(same_bits(kcp_mean_text(s), parsed(kcp_mean(s))));
            check_value(kcp_mean(s));
            // a tie: sum / n is a double exactly (in lowest terms its denominator is a power of two) and 2 * 10^4 times it is odd
            const uint64_t den = n / std::gcd<uint64_t, uint64_t>(sum, n);
            if ((den & (den - 1)) == 0 && (2 * sum * 10000) % n == 0 && ((2 * sum * 10000) / n) % 2 == 1) ++ties;
        }
    CHECK(ties >= 100);
    CHECK(kcp_dec4(1.0 / 32) == 312 && kcp_dec4(3.0 / 32) == 938 && kcp_dec4(33.0 / 32) == 10312 && kcp_dec4(35.0 / 32) == 10938);
    // near ties: the decimal number ends in ...5 and the double lies just under or over it
    for (uint32_t i = 1; i < 40000; i += 2) {
        const double v = i / 20000.0;
        check_value(v);
        check_value(nextafter(v, 0.0));
        check_value(nextafter(v, 1e9));
        check_value(236.0 - v);
    }
    check_value(0.0);
    check_value(236.0);
    check_value(0.00005);
    check_value(0.99995);
    std::mt19937_64 rng(20251019);
    for (int i = 0; i < 100000; ++i) {
        const uint32_t n = 1 + (uint32_t)(rng() % 0x7FFFFFFFull);
        const uint64_t sum = n + rng() % (235ull * n + 1);  // counts per read 1 .. 236
        const KcpSlot s = slot(n, sum, sum);
        CHECK(same_bits(kcp_mean_text(s), parsed(kcp_mean(s))));
    }
    // D < 2^24: (float)D / 10000.0f is strtof of the digits
    for (int i = 0; i < 200000; ++i) {
        const uint32_t D = (uint32_t)(rng() % (1u << 24));
        char buf[32];
        snprintf(buf, sizeof buf, "%u.%04u", D / 10000, D % 10000);
        CHECK(same_bits(kcp_text_float(D), strtof(buf, nullptr)));
    }
}

static void check_one_sd(uint32_t n, uint64_t sum, uint64_t sumsq) {
    const KcpSlot s = slot(n, sum, sumsq);
    CHECK((unsigned __int128)n * sumsq >= (unsigned __int128)sum * sum);
    CHECK(same_bits(kcp_sd_text(s), parsed(kcp_sd(s))));
}

static void check_sds() {
    std::mt19937_64 rng(99);
    // the moments of n counts of 1 .. 236
    for (int i = 0; i < 20000; ++i) {
        const uint32_t n = 1 + (uint32_t)(rng() % 300);
        uint64_t sum = 0, sumsq = 0;
        const uint32_t top = 1 + (uint32_t)(rng() % 236);
        for (uint32_t j = 0; j < n; ++j) { const uint64_t c = 1 + rng() % top; sum += c; sumsq += c * c; }
        check_one_sd(n, sum, sumsq);
    }
    // n * sumsq == sum^2: every count the same, sd 0
    for (uint32_t n = 1; n <= 300; ++n)
        for (uint64_t c : {1ull, 2ull, 7ull, 236ull}) {
            check_one_sd(n, n * c, n * c * c);
            CHECK(kcp_sd_text(slot(n, n * c, n * c * c)) == 0.0f);
        }
    // numerators above 2^64: large n with two count values, and moments no reads give (both words of the difference in play)
    uint32_t big = 0;
    for (int i = 0; i < 20000; ++i) {
        const uint32_t n = 0x40000000u + (uint32_t)(rng() % 0x3FFFFFFFull);
        const uint64_t a = rng() % n, c0 = 1 + rng() % 100, c1 = c0 + 1 + rng() % 136;  // a reads of count c0, n - a of count c1
        const uint64_t sum = a * c0 + (n - a) * c1, sumsq = a * c0 * c0 + (n - a) * c1 * c1;
        if (((unsigned __int128)n * sumsq - (unsigned __int128)sum * sum) >> 64) ++big;
        check_one_sd(n, sum, sumsq);
    }
    CHECK(big > 1000);
    for (int i = 0; i < 20000; ++i) {
        const uint32_t n = 1 + (uint32_t)(rng() >> 32);
        const uint64_t sum = rng() >> (16 + rng() % 20);
        const unsigned __int128 need = ((unsigned __int128)sum * sum + n - 1) / n;
        if (need >> 63) continue;
        const uint64_t sumsq = (uint64_t)need + rng() % ((uint64_t)n * 2000000);  // sd^2 < 2 * 10^6 + 1: the digits stay below 2^24
        if (((unsigned __int128)n * sumsq - (unsigned __int128)sum * sum) >> 64) ++big;
        check_one_sd(n, sum, sumsq);
    }
    CHECK(big > 10000);
    CHECK(kcp_u128_to_double(0, 5) == 5.0 && kcp_u128_to_double(1, 0) == 18446744073709551616.0);
    CHECK(kcp_u128_to_double(1, 1) == 18446744073709551616.0);                      // far below half an ulp
    CHECK(kcp_u128_to_double(0x8000000000000000ull, 0x400) == ldexp(1.0, 127));      // 2^127 + 2^10: rounds down
    CHECK(kcp_u128_to_double(0x8000000000000400ull, 0) == ldexp(1.0, 127));          // a tie at bit 74: to even (down)
    CHECK(kcp_u128_to_double(0x8000000000000400ull, 1) > ldexp(1.0, 127));           // the sticky bit breaks it: up
    CHECK(kcp_u128_to_double(0x8000000000000C00ull, 0) == ldexp(1.0, 127) + ldexp(1.0, 76));  // a tie with an odd last place: up
}

static void check_inside_and_step() {
    // both equalities belong to the interval; one float ulp beyond does not
    const float m = 1.5f, sd = 0.25f;
    CHECK(kcp_fps_inside(1.0f, m, sd) && kcp_fps_inside(2.0f, m, sd) && kcp_fps_inside(1.5f, m, sd));
    CHECK(!kcp_fps_inside(nextafterf(1.0f, 0.0f), m, sd) && !kcp_fps_inside(nextafterf(2.0f, 3.0f), m, sd));
    CHECK(kcp_fps_inside(3.0f, 3.0f, 0.0f) && !kcp_fps_inside(3.0001f, 3.0f, 0.0f));
    // the step over a 64-slot table: absent, dropped, widened, widened again; a k-mer under another locus or class is not the entry
    struct NoX {
        uint64_t atomic_cas(uint64_t* p, uint64_t e, uint64_t d) { const uint64_t o = *p; if (o == e) *p = d; return o; }
        uint32_t atomic_cas32(uint32_t* p, uint32_t e, uint32_t d) { const uint32_t o = *p; if (o == e) *p = d; return o; }
        void atomic_add(uint32_t* p, uint32_t v) { *p += v; }
        void atomic_add(uint64_t* p, uint64_t v) { *p += v; }
        void atomic_min32(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
        void atomic_max32(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    } x;
    const uint64_t slots = 64;
    std::vector<KcpSlot> tab(slots, KCP_EMPTY);
    uint32_t claimed = 0;
    auto put = [&](uint64_t km, uint32_t locus, uint32_t cls, uint32_t n, uint64_t sum, uint64_t sumsq, uint32_t mn, uint32_t mx) {
        CHECK(kcp_insert(x, tab.data(), slots - 1, 64 - 6, km, kcp_lc1(locus, cls), n, sum, sumsq, mn, mx, claimed));
    };
    for (uint64_t i = 0; i < 28; ++i) put(1000 + i, 3, 1, 1, 1, 1, 1, 1);  // fillers of the other class: walks pass over them
    put(1000, 3, 0, 4, 10, 30, 1, 4);   // mean 2.5, sd sqrt(1.25) = 1.1180: inside for 0.264 .. 4.736
    put(1001, 2, 0, 2, 4, 8, 2, 2);     // the k-mer under another locus
    put(1002, 3, 0, 2, 6, 18, 3, 3);    // mean 3, sd 0
    const uint32_t fresh = kcp_cand_fresh();
    CHECK(fresh == (255u | KCP_CAND_ALIVE));
    auto step = [&](uint64_t km, uint32_t locus, float mean, uint32_t st) { return kcp_fps_step(tab.data(), slots - 1, 64 - 6, KcpCand{km, locus, mean}, st); };
    CHECK(step(999, 3, 1.0f, fresh) == fresh);             // absent
    CHECK(step(1001, 3, 1.0f, fresh) == fresh);            // held under locus 2 and in class 1 only
    CHECK(step(1000, 3, 1.0f, fresh) == 0u);               // inside: dead
    CHECK(step(1000, 3, 5.0f, fresh) == (1u | 4u << 8 | KCP_CAND_ALIVE));
    CHECK(step(1002, 3, 3.0f, fresh) == 0u);               // sd 0, equal means
    CHECK(step(1002, 3, 2.0f, fresh) == (3u | 3u << 8 | KCP_CAND_ALIVE));
    CHECK(step(1002, 3, 2.0f, 1u | 2u << 8 | KCP_CAND_ALIVE) == (1u | 3u << 8 | KCP_CAND_ALIVE));  // widens
    CHECK(step(1002, 3, 2.0f, 4u | 9u << 8 | KCP_CAND_ALIVE) == (3u | 9u << 8 | KCP_CAND_ALIVE));
    // a full table without the key: the walk ends after one round
    for (uint64_t i = 0; claimed < slots; ++i) put(5000 + i, 1, 0, 1, 1, 1, 1, 1);
    CHECK(step(999, 3, 1.0f, fresh) == fresh);
}

int main() {
    check_means();
    check_sds();
    check_inside_and_step();
    printf("kcp fps ok\n");
    return 0;
}
