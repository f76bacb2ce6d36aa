// dbtk_assoc_perm_host.h — the host half of the permutation p-values of the association scan (include/dbtk_assoc_perm.h) that needs no
// device: the seeded generator, the validation of a caller's permutations, and the fold of the maxima into n_ge, p_perm and q_perm.
// Header only, so that tests/assoc_perm_host_check.cpp compiles it alone under the sanitizers.
#ifndef DBTK_ASSOC_PERM_HOST_H_
#define DBTK_ASSOC_PERM_HOST_H_

#include <stdint.h>

#include <vector>

#include "dbtk_assoc_host.h"

namespace dbtk_assoc_host {

constexpr uint64_t PERM_MAX = 1000000;  // permutations of a handle at most (DBTK_ASSOC_PERM_MAX)

// all of s is an unsigned 64-bit integer in decimal digits (whole_uint stops at 19 digits; a seed may take 20)
inline bool whole_u64(const std::string& s, uint64_t* v) {
    if (s.empty() || s.size() > 20) return false;
    uint64_t x = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        const uint64_t d = (uint64_t)(c - '0');
        if (x > (UINT64_MAX - d) / 10) return false;
        x = x * 10 + d;
    }
    *v = x;
    return true;
}

// one splitmix64 stream (the header states it word for word)
struct SplitMix64 {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

// perm[B][n]: permutations 1 .. B in that order from the one stream, each from the identity by i = n - 1 down to 1,
// j = high half of next() * (i + 1), swap
inline void perm_generate(uint64_t n, uint64_t B, uint64_t seed, uint32_t* perm) {
    SplitMix64 g{seed};
    for (uint64_t b = 0; b < B; ++b) {
        uint32_t* p = perm + b * n;
        for (uint64_t i = 0; i < n; ++i) p[i] = (uint32_t)i;
        for (uint64_t i = n; i-- > 1;) {
            const uint64_t j = (uint64_t)(((unsigned __int128)g.next() * (unsigned __int128)(i + 1)) >> 64);
            const uint32_t t = p[i]; p[i] = p[j]; p[j] = t;
        }
    }
}

// true when every row of perm[B][n] is a permutation of 0 .. n - 1; otherwise *bad_row is the first row that is not
inline bool perm_valid(uint64_t n, uint64_t B, const uint32_t* perm, uint64_t* bad_row) {
    std::vector<uint8_t> seen(n);
    for (uint64_t b = 0; b < B; ++b) {
        std::fill(seen.begin(), seen.end(), (uint8_t)0);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t v = perm[b * n + i];
            if (v >= n || seen[v]) { *bad_row = b; return false; }
            seen[v] = 1;
        }
    }
    return true;
}

// T[B + 1] of one phenotype: the permutations b in 1 .. B with T_b >= T_0
inline uint64_t perm_count_ge(const double* T, uint64_t B) {
    uint64_t k = 0;
    for (uint64_t b = 1; b <= B; ++b) k += T[b] >= T[0];
    return k;
}
inline double perm_pvalue(uint64_t n_ge, uint64_t B) { return (double)(n_ge + 1) / (double)(B + 1); }

// T[P][B + 1] and has_tests[P] -> n_ge[P], p_perm[P], q_perm[P]: Benjamini-Hochberg over the phenotypes that have tests, 0 for the others
inline void perm_fold(uint64_t P, uint64_t B, const double* T, const uint8_t* has_tests, uint64_t* n_ge, double* p_perm, double* q_perm) {
    std::vector<double> pv, qv;
    std::vector<uint64_t> who;
    for (uint64_t p = 0; p < P; ++p) {
        n_ge[p] = 0; p_perm[p] = 0.0; q_perm[p] = 0.0;
        if (!has_tests[p]) continue;
        n_ge[p] = perm_count_ge(T + p * (B + 1), B);
        p_perm[p] = perm_pvalue(n_ge[p], B);
        pv.push_back(p_perm[p]); who.push_back(p);
    }
    qv.resize(pv.size());
    bh(pv.data(), pv.size(), qv.data());
    for (size_t i = 0; i < who.size(); ++i) q_perm[who[i]] = qv[i];
}

}  // namespace dbtk_assoc_host
#endif
