// kcp_table_check.cpp — the host-compiled half of csrc/dbtk_kcp.h (the profile table of --bait-profile) under AddressSanitizer and
// UndefinedBehaviorSanitizer: the multiplicity step, the canonical k-mers, kcp_insert from 8 threads against a std::map, one k-mer
// at two loci and in both classes, a rehash that keeps all five counters, and a full table reported as failure with nothing added.
// Built and run by tests/test_kcp_host.py; prints "kcp table ok" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <tuple>
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

// the accessor of a host thread: the same atomics the device accessor gives kcp_insert
struct HostX {
    uint64_t atomic_cas(uint64_t* p, uint64_t e, uint64_t d) { __atomic_compare_exchange_n(p, &e, d, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST); return e; }
    uint32_t atomic_cas32(uint32_t* p, uint32_t e, uint32_t d) { __atomic_compare_exchange_n(p, &e, d, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST); return e; }
    void atomic_add(uint32_t* p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
    void atomic_add(uint64_t* p, uint64_t v) { __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
    void atomic_min32(uint32_t* p, uint32_t v) { uint32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {} }
    void atomic_max32(uint32_t* p, uint32_t v) { uint32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST); while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {} }
};

typedef std::pair<uint64_t, uint32_t> Key;                   // (k-mer, lc1)
typedef std::array<uint64_t, 5> Val;                         // n, sum, sumsq, min, max
typedef std::map<Key, Val> Model;

static uint32_t shift_of(uint64_t slots) { uint32_t l = 0; while ((1ull << l) < slots) ++l; return 64 - l; }

static void model_add(Model& m, uint64_t km, uint32_t lc1, uint32_t c) {
    auto it = m.find(Key(km, lc1));
    if (it == m.end()) { m[Key(km, lc1)] = Val{1, c, (uint64_t)c * c, c, c}; return; }
    Val& v = it->second;
    v[0] += 1; v[1] += c; v[2] += (uint64_t)c * c; v[3] = std::min<uint64_t>(v[3], c); v[4] = std::max<uint64_t>(v[4], c);
}

static Model model_of(const std::vector<KcpSlot>& t) {
    Model m;
    for (const KcpSlot& s : t)
        if (kcp_is_entry(s)) {
            CHECK(!m.count(Key(s.kmer, s.lc1)));  // a key never has two slots
            m[Key(s.kmer, s.lc1)] = Val{s.n, s.sum, s.sumsq, s.mn, s.mx};
        }
    return m;
}

static void check_multiplicity() {
    auto at = [](const std::vector<uint64_t>& km, uint32_t pos, uint32_t want_c, bool want_first) {
        uint32_t c = 99; bool f = !want_first;
        kcp_multiplicity(km.data(), (uint32_t)km.size(), pos, &c, &f);
        CHECK(c == want_c && f == want_first);
    };
    const std::vector<uint64_t> same(130, 7);   // a homopolymer's k-mers
    for (uint32_t p = 0; p < same.size(); ++p) at(same, p, 130, p == 0);
    std::vector<uint64_t> distinct(236);
    for (uint32_t p = 0; p < distinct.size(); ++p) distinct[p] = 1000 + 3 * p;
    for (uint32_t p = 0; p < distinct.size(); ++p) at(distinct, p, 1, true);
    const std::vector<uint64_t> holes = {NAN64, 5, NAN64, 5, 7, NAN64, 7, 7, 5, NAN64};
    const uint32_t want_c[] = {0, 3, 0, 3, 3, 0, 3, 3, 3, 0};
    const bool want_f[] = {false, true, false, false, true, false, false, false, false, false};
    for (uint32_t p = 0; p < holes.size(); ++p) at(holes, p, want_c[p], want_f[p]);
    const std::vector<uint64_t> one = {42};
    at(one, 0, 1, true);
    const std::vector<uint64_t> alt = {1, 2, 1, 2, 1};  // a dinucleotide repeat's two k-mers
    at(alt, 0, 3, true); at(alt, 1, 2, true); at(alt, 2, 3, false); at(alt, 3, 2, false); at(alt, 4, 3, false);
}

static void check_kmers() {
    const std::string a(30, 'A');
    const uint8_t* s = (const uint8_t*)a.data();
    CHECK(kcp_kmer_at(s, 30, 0, 21) == 0 && kcp_kmer_at(s, 30, 9, 21) == 0);
    CHECK(kcp_kmer_at(s, 30, 10, 21) == NAN64);  // the window leaves the read
    CHECK(kcp_kmer_at(s, 20, 0, 21) == NAN64 && kcp_kmer_at(s, 0, 0, 21) == NAN64);
    const std::string t(31, 'T');
    CHECK(kcp_kmer_at((const uint8_t*)t.data(), 31, 0, 31) == 0);  // canonical: the reverse complement
    std::string r = "ACGTTGCAGGATCCATAGCAAGTC";
    const uint64_t k0 = kcp_kmer_at((const uint8_t*)r.data(), 24, 0, 21), k3 = kcp_kmer_at((const uint8_t*)r.data(), 24, 3, 21);
    CHECK(k0 != NAN64 && k3 != NAN64 && k0 != k3 && k0 < (1ull << 42));
    std::string rc(r.rbegin(), r.rend());
    for (char& c : rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    CHECK(kcp_kmer_at((const uint8_t*)rc.data(), 24, 3, 21) == k0 && kcp_kmer_at((const uint8_t*)rc.data(), 24, 0, 21) == k3);
    r[5] = 'N';
    for (uint32_t p = 0; p < 4; ++p) CHECK(kcp_kmer_at((const uint8_t*)r.data(), 24, p, 21) == NAN64);
    r[5] = 'g';
    CHECK(kcp_kmer_at((const uint8_t*)r.data(), 24, 0, 21) == NAN64);
    CHECK(kcp_kmer_at((const uint8_t*)"ACG", 3, 1, 2) == 6 /* CG */ && kcp_kmer_at((const uint8_t*)"ACG", 3, 0, 2) == 1 /* AC < GT */);
}

// 8 threads, 64 slots, 30 keys (a load under 1/2), 4 000 inserts each: the table against the map of the same inserts
static void check_threads() {
    const uint64_t slots = 64;
    std::vector<KcpSlot> tab(slots, KCP_EMPTY);
    std::vector<Key> keys;
    for (uint32_t i = 0; i < 30; ++i) keys.push_back(Key(0x1234567ull * (i / 3 + 1), kcp_lc1(i % 3, (i / 3) & 1)));  // k-mers shared by loci and classes
    const int NT = 8, PER = 4000;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> ops(NT);
    Model want;
    std::mt19937_64 rng(20250921);
    for (int t = 0; t < NT; ++t)
        for (int i = 0; i < PER; ++i) {
            const uint32_t ki = (uint32_t)(rng() % keys.size()), c = 1 + (uint32_t)(rng() % 236);
            ops[t].push_back(std::make_pair(ki, c));
            model_add(want, keys[ki].first, keys[ki].second, c);
        }
    std::vector<uint32_t> claimed(NT, 0), failed(NT, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < NT; ++t)
        th.emplace_back([&, t] {
            HostX x;
            for (const auto& o : ops[t])
                if (!kcp_insert(x, tab.data(), slots - 1, shift_of(slots), keys[o.first].first, keys[o.first].second, 1u, o.second, (uint64_t)o.second * o.second, o.second,
                                o.second, claimed[t]))
                    ++failed[t];
        });
    for (auto& t : th) t.join();
    uint32_t nclaimed = 0, taken = 0;
    for (int t = 0; t < NT; ++t) { CHECK(failed[t] == 0); nclaimed += claimed[t]; }
    for (const KcpSlot& s : tab) taken += s.kmer != NAN64;
    CHECK(model_of(tab) == want);
    CHECK(nclaimed == taken && taken == want.size());  // every slot taken is an entry: the occupancy the host reads is exact
}

static void check_two_loci_two_classes_and_rehash() {
    const uint64_t slots = 64;
    std::vector<KcpSlot> tab(slots, KCP_EMPTY);
    HostX x;
    uint32_t claimed = 0;
    Model want;
    const uint64_t km = 0x2AAAAAAAAAAull;
    for (uint32_t locus = 0; locus < 2; ++locus)
        for (uint32_t cls = 0; cls < 2; ++cls)
            for (uint32_t c = 1 + locus; c <= 9; c += 2 + cls) {
                CHECK(kcp_insert(x, tab.data(), slots - 1, shift_of(slots), km, kcp_lc1(locus, cls), 1u, c, (uint64_t)c * c, c, c, claimed));
                model_add(want, km, kcp_lc1(locus, cls), c);
            }
    CHECK(want.size() == 4 && claimed == 4 && model_of(tab) == want);
    CHECK((kcp_lc1(5, 1) >> 31) == 1 && (kcp_lc1(5, 1) & 0x7FFFFFFFu) == 6 && kcp_lc1(5, 0) == 6);
    // more keys, with large counters, then every slot into a table of twice the size
    std::mt19937_64 rng(7);
    for (uint32_t i = 0; i < 26; ++i) {
        const uint64_t k2 = rng() >> 2;
        const uint32_t lc1 = kcp_lc1((uint32_t)(rng() % 1000), (uint32_t)(rng() & 1)), n = 1 + (uint32_t)(rng() % 100000);
        const uint64_t sum = (uint64_t)n * 100 + rng() % 1000, sumsq = sum * 200 + (1ull << 40);
        CHECK(kcp_insert(x, tab.data(), slots - 1, shift_of(slots), k2, lc1, n, sum, sumsq, 3, 200, claimed));
        want[Key(k2, lc1)] = Val{n, sum, sumsq, 3, 200};
    }
    CHECK(model_of(tab) == want);
    std::vector<KcpSlot> big(2 * slots, KCP_EMPTY);
    uint32_t claimed2 = 0;
    KcpSlot half = KCP_EMPTY;  // a slot claimed and never counted is not an entry and does not move
    half.kmer = 99; half.lc1 = kcp_lc1(1, 0);
    CHECK(kcp_move(x, half, big.data(), 2 * slots - 1, shift_of(2 * slots), claimed2) && claimed2 == 0);
    for (const KcpSlot& s : tab) CHECK(kcp_move(x, s, big.data(), 2 * slots - 1, shift_of(2 * slots), claimed2));
    CHECK(claimed2 == want.size() && model_of(big) == want);
}

static void check_full_table() {
    const uint64_t slots = 64;
    std::vector<KcpSlot> tab(slots, KCP_EMPTY);
    HostX x;
    uint32_t claimed = 0;
    for (uint32_t i = 0; i < slots; ++i) CHECK(kcp_insert(x, tab.data(), slots - 1, shift_of(slots), 1000 + i, kcp_lc1(i % 5, 0), 1u, 2, 4, 2, 2, claimed));
    CHECK(claimed == slots);
    const std::vector<KcpSlot> before = tab;
    CHECK(!kcp_insert(x, tab.data(), slots - 1, shift_of(slots), 5000, kcp_lc1(0, 0), 1u, 2, 4, 2, 2, claimed));   // a new k-mer
    CHECK(!kcp_insert(x, tab.data(), slots - 1, shift_of(slots), 1000, kcp_lc1(0, 1), 1u, 2, 4, 2, 2, claimed));   // a k-mer it holds, in the other class
    CHECK(claimed == slots && memcmp(before.data(), tab.data(), slots * sizeof(KcpSlot)) == 0);
    CHECK(kcp_insert(x, tab.data(), slots - 1, shift_of(slots), 1000, kcp_lc1(0, 0), 1u, 5, 25, 5, 5, claimed));    // a key it holds still counts
    const KcpSlot one{7, kcp_lc1(0, 0), 4, 10, 30, 1, 4};
    CHECK(kcp_mean(one) == 2.5 && kcp_sd(one) == sqrt(1.25));
}

int main() {
    check_multiplicity();
    check_kmers();
    check_threads();
    check_two_loci_two_classes_and_rehash();
    check_full_table();
    printf("kcp table ok\n");
    return 0;
}
