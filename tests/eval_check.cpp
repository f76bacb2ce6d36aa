// eval_check.cpp — the per-window and per-locus bodies of the genotype score (csrc/dbtk_eval.h) on the host, stand-alone: built with
// -fsanitize=address,undefined by tests/test_eval_host.py and run as a child process.  Reads a case from the file named on the command
// line, works through it the way k_eval_truth and k_eval_sums do (items of EV_CH start positions packed 16 bases a word; a locus
// shared out over 1, 64 and 256 lanes and merged), and prints truth, windows and the sums for the test to compare with its model.
//
//   k nloci nk
//   nintervals, then per interval: locus bases
//   nclass, then per entry: locus k-mer class both     (class: the counter, or -1 for a flank k-mer, which beats TR; both: the counter
//                                                       of a k-mer that is a flank k-mer and a TR k-mer of the locus, else -1)
//   nk values of x, nk values of y, nloci + 1 values of beg
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dbtk_eval.h"

using namespace dbtk;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned k = 0;
    unsigned long long nloci = 0, nk = 0, n = 0;
    if (fscanf(f, "%u %llu %llu", &k, &nloci, &nk) != 3) return 2;
    if (fscanf(f, "%llu", &n) != 1) return 2;
    std::vector<std::pair<uint32_t, std::string>> ivs(n);
    std::vector<char> buf(1 << 20);
    for (auto& iv : ivs) {
        if (fscanf(f, "%u %1048575s", &iv.first, buf.data()) != 2) return 2;
        iv.second = buf.data();
    }
    if (fscanf(f, "%llu", &n) != 1) return 2;
    uint64_t cap = 64;
    while (cap < 2 * n + 2) cap <<= 1;
    uint32_t shift = 64;
    for (uint64_t c = cap; c > 1; c >>= 1) --shift;
    std::vector<ClsSlot> cls(cap, ClsSlot{NAN64, ~0ull}), both(cap, ClsSlot{NAN64, ~0ull});
    auto insert = [&](std::vector<ClsSlot>& tab, uint64_t km, uint32_t l, uint32_t value) {
        uint64_t at = hash_cls(km, l, shift);
        while (tab[at].kmer != NAN64) at = (at + 1) & (cap - 1);
        tab[at] = ClsSlot{km, (uint64_t)l << 32 | value};
    };
    for (unsigned long long i = 0; i < n; ++i) {
        unsigned long long l, km;
        long long c, b;
        if (fscanf(f, "%llu %llu %lld %lld", &l, &km, &c, &b) != 4) return 2;
        insert(cls, km, (uint32_t)l, c < 0 ? CLS_FLANK : (uint32_t)c);
        if (b >= 0) insert(both, km, (uint32_t)l, (uint32_t)b);
    }
    const EvalTables T{cls.data(), cap - 1, shift, both.data(), cap - 1, shift};
    std::vector<uint64_t> x(nk), y(nk), beg(nloci + 1);
    for (auto* v : {&x, &y, &beg})
        for (uint64_t& e : *v) { unsigned long long t; if (fscanf(f, "%llu", &t) != 1) return 2; e = t; }
    fclose(f);

    // ---- truth: every interval cut into items as dbtk_eval_truth_sim cuts it; the arena has 16 bytes behind its last base, no more
    std::vector<uint64_t> truth(nk, 0), windows(nloci, 0);
    for (const auto& iv : ivs) {
        const std::string& s = iv.second;
        if (s.size() < k) continue;
        std::vector<uint8_t> arena(s.size() + 16, 0xAB);
        memcpy(arena.data(), s.data(), s.size());
        const uint64_t npos = s.size() - k + 1;
        for (uint64_t p = 0; p < npos; p += EV_CH) {
            const EvalItem item{p, (uint32_t)(npos - p < EV_CH ? npos - p : EV_CH), iv.first};
            std::vector<uint32_t> pk(EV_WORDS, 0xDEADBEEFu);
            std::vector<uint16_t> vd(EV_WORDS, 0xFFFFu);
            const uint32_t nw = eval_item_words(item.n, k);
            if (nw + 2 > EV_WORDS) return 3;
            for (uint32_t w = 0; w < nw + 2; ++w) {
                if (w < nw) eval_stage_word(arena.data() + item.off, w, pk.data(), vd.data());
                else { pk[w] = 0; vd[w] = 0; }
            }
            for (uint32_t j = 0; j < item.n; ++j) {
                bool valid = false;
                const uint32_t c = eval_window(pk.data(), vd.data(), j, k, T, item.locus, &valid);
                windows[item.locus] += valid ? 1 : 0;
                if (c != NAN32) { if (c >= nk) return 3; ++truth[c]; }
            }
        }
    }
    printf("truth");
    for (uint64_t v : truth) printf(" %llu", (unsigned long long)v);
    printf("\nwindows");
    for (uint64_t v : windows) printf(" %llu", (unsigned long long)v);
    printf("\n");

    // ---- sums: a locus shared out over 1, 64 and 256 lanes must give the same integers and the same verdict
    for (uint64_t l = 0; l < nloci; ++l) {
        EvalSums first{};
        bool first_ok = true;
        for (uint32_t nl : {1u, 64u, 256u}) {
            EvalSums t = {0, 0, 0, 0, 0, 0, 0, 0};
            bool ok = true;
            for (uint32_t lane = 0; lane < nl; ++lane) {
                EvalSums part;
                ok &= eval_locus_part(x.data(), y.data(), beg[l], beg[l + 1], lane, nl, &part);
                ok &= eval_merge(t, part);
            }
            if (nl == 1) { first = t; first_ok = ok; }
            else if (ok != first_ok || (ok && memcmp(&t, &first, sizeof t) != 0)) { printf("lanes disagree at locus %llu\n", (unsigned long long)l); return 4; }
        }
        if (!first_ok) { printf("sums %llu overflow\n", (unsigned long long)l); continue; }
        printf("sums %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)l, (unsigned long long)first.n1, (unsigned long long)first.Sx, (unsigned long long)first.Sy,
               (unsigned long long)first.Sy1, (unsigned long long)first.Sxy, (unsigned long long)first.Sxx, (unsigned long long)first.Syy, (unsigned long long)first.Syy1);
    }
    return 0;
}
