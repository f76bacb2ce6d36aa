// assoc_host_check.cpp — the host half of the association scan (csrc/dbtk_assoc_host.h) stand-alone: built with -fsanitize=address,undefined
// and run by tests/test_assoc_host.py.  The parsers on hostile text, Benjamini-Hochberg, the p-value at its edges, the r^2 threshold.
// Prints "ok" and returns 0, or the first failed check and 1.
#include <stdio.h>

#include <string>
#include <vector>

#include "dbtk_assoc_host.h"

using namespace dbtk_assoc_host;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool pheno_fails(const std::string& text, const std::string& part) {
    PhenoTable T;
    std::string err;
    if (parse_pheno(text, "P", &T, &err)) { printf("  accepted: %s\n", text.c_str()); return false; }
    if (err.find(part) == std::string::npos) { printf("  message \"%s\" lacks \"%s\"\n", err.c_str(), part.c_str()); return false; }
    return true;
}
static bool pairs_fails(const std::string& text, const std::string& part) {
    std::vector<uint64_t> off;
    std::vector<uint32_t> idx;
    std::string err;
    if (parse_pairs(text, "Q", {"a", "b", "c"}, 4, &off, &idx, &err)) { printf("  accepted: %s\n", text.c_str()); return false; }
    if (err.find(part) == std::string::npos) { printf("  message \"%s\" lacks \"%s\"\n", err.c_str(), part.c_str()); return false; }
    return true;
}

int main() {
    {   // a table as it should be: CRLF, an empty line, samples in any order, exponents and signs
        PhenoTable T;
        std::string err;
        CHECK(parse_pheno("id\ta\tb\r\n5\t1.5\t-2e3\r\n\r\n0\t+0.25\t7\n3\t1e-300\t.5", "P", &T, &err));
        CHECK(T.names.size() == 2 && T.names[1] == "b" && T.sample_of.size() == 3 && T.sample_of[0] == 5 && T.sample_of[2] == 3);
        CHECK(T.values.size() == 6 && T.values[0] == 1.5 && T.values[1] == 0.25 && T.values[3] == -2000.0 && T.values[5] == 0.5);
    }
    CHECK(pheno_fails("", "no header"));
    CHECK(pheno_fails("\n\n", "no header"));
    CHECK(pheno_fails("sample\ta\n", "line 1: the header"));
    CHECK(pheno_fails("id\n", "line 1: the header"));
    CHECK(pheno_fails("id\ta\ta\n", "named twice"));
    CHECK(pheno_fails("id\ta\t\n", "empty phenotype name"));
    CHECK(pheno_fails("id\ta\n0\t1\n1\tNA\n", "line 3: phenotype a: \"NA\""));
    CHECK(pheno_fails("id\ta\tb\n0\t1\t\n", "line 2: phenotype b: \"\""));
    CHECK(pheno_fails("id\ta\n0\t1x\n", "line 2"));
    CHECK(pheno_fails("id\ta\n0\tnan\n", "not a finite number"));
    CHECK(pheno_fails("id\ta\n0\tinf\n", "not a finite number"));
    CHECK(pheno_fails("id\ta\n0\t1e999\n", "not a finite number"));
    CHECK(pheno_fails("id\ta\n0\t 1\n", "line 2"));
    CHECK(pheno_fails("id\ta\n0\t1\t2\n", "line 2: 3 fields, the header has 2"));
    CHECK(pheno_fails("id\ta\tb\n0\t1\n", "line 2: 2 fields"));
    CHECK(pheno_fails("id\ta\n-1\t1\n", "line 2: the sample"));
    CHECK(pheno_fails("id\ta\n1.0\t1\n", "line 2: the sample"));
    CHECK(pheno_fails("id\ta\n99999999999999999999\t1\n", "line 2: the sample"));
    CHECK(pheno_fails("id\ta\n\t1\n", "line 2: the sample"));
    CHECK(pheno_fails("id\ta\n4\t1\n\n4\t2\n", "line 4: sample 4 is given twice (first on line 2)"));
    CHECK(pheno_fails(std::string("id\ta\n0\t1") + '\0' + "\n", "line 2"));
    {   // a long line and a long field do not trouble it
        std::string big = "id";
        for (int i = 0; i < 3000; ++i) big += "\tn" + std::to_string(i);
        big += "\n7";
        for (int i = 0; i < 3000; ++i) big += "\t" + std::to_string(i) + ".5";
        PhenoTable T;
        std::string err;
        CHECK(parse_pheno(big, "P", &T, &err) && T.names.size() == 3000 && T.values[2999] == 2999.5);
        CHECK(pheno_fails("id\ta\n0\t" + std::string(100000, '9') + "\n", "not a finite number"));
    }
    {   // pairs: duplicates count once, any order, sorted within the locus, loci without a line are empty
        std::vector<uint64_t> off;
        std::vector<uint32_t> idx;
        std::string err;
        CHECK(parse_pairs("3\tc\n0\tb\r\n3\ta\n\n3\tc\n0\tb\n", "Q", {"a", "b", "c"}, 4, &off, &idx, &err));
        CHECK(off == (std::vector<uint64_t>{0, 1, 1, 1, 3}) && idx == (std::vector<uint32_t>{1, 0, 2}));
        CHECK(parse_pairs("", "Q", {"a"}, 2, &off, &idx, &err) && off == (std::vector<uint64_t>{0, 0, 0}) && idx.empty());
    }
    {   // the form and the names alone, before the build is known: nothing is built, whatever the bound
        std::string err;
        CHECK(parse_pairs("7\ta\n4000000000\tb\n", "Q", {"a", "b"}, 0xFFFFFFFFull, nullptr, nullptr, &err));
        CHECK(!parse_pairs("7\ta\n1\tz\n", "Q", {"a", "b"}, 0xFFFFFFFFull, nullptr, nullptr, &err) && err.find("line 2: unknown phenotype z") != std::string::npos);
    }
    CHECK(pairs_fails("0\ta\n4\ta\n", "line 2: locus 4 >= the build's 4 loci"));
    CHECK(pairs_fails("0\td\n", "line 1: unknown phenotype d"));
    CHECK(pairs_fails("0\n", "line 1: expected LOCUS"));
    CHECK(pairs_fails("0\ta\tb\n", "line 1: expected LOCUS"));
    CHECK(pairs_fails("x\ta\n", "line 1: \"x\" is not a locus"));
    CHECK(pairs_fails("-0\ta\n", "is not a locus"));
    {   // Benjamini-Hochberg
        const double p[5] = {0.01, 0.04, 0.03, 0.5, 3.0};
        double q[5];
        bh(p, 5, q);
        CHECK(q[0] == 0.05 && q[1] == 0.04 * 5 / 3 && q[2] == 0.04 * 5 / 3 && q[3] == 0.5 * 5 / 4 && q[4] == 1.0);
        bh(p, 0, q);
        const double one[1] = {0.2};
        bh(one, 1, q);
        CHECK(q[0] == 0.2);
        const double ties[4] = {0.02, 0.02, 0.0, 0.02};
        bh(ties, 4, q);
        CHECK(q[2] == 0.0 && q[0] == 0.02 && q[1] == 0.02 && q[3] == 0.02);
    }
    {   // the p-value at its edges
        CHECK(pvalue(1.0, 3) == 0.0 && pvalue(-1.0, 4000) == 0.0 && pvalue(0.0, 3) == 1.0 && pvalue(0.0, 4000) == 1.0);
        CHECK(pvalue(1e-300, 10) == 1.0 && pvalue(0.5, 3) > 0.66 && pvalue(0.5, 3) < 0.67);   // n = 3: p = 1 - 2 asin(r) / pi = 2 / 3
        CHECK(pvalue(1.0 - 1e-16, 3) > 0.0 && pvalue(1.0 - 1e-16, 3) < 1e-7);
        CHECK(pvalue(0.999999999999, 4000) == 0.0);                                            // below the subnormals
        double last = 1.0;
        for (int i = 1; i < 1000; ++i) { const double v = pvalue(i / 1000.0, 50); CHECK(v < last && v > 0.0); last = v; }
        CHECK(pvalue(0.3, 10) == pvalue(-0.3, 10));
    }
    {   // the r^2 threshold brackets its p-value
        for (uint64_t n : {3, 10, 879})
            for (double pt : {0.5, 0.05, 1e-8, 1e-100}) {
                if (n < 100 && pt < 1e-8) continue;  // (1 - r^2 of that p is below the spacing of doubles at 1: the threshold is 1 itself)
                const double r2 = r2_threshold(pt, n);
                CHECK(r2 > 0.0 && r2 < 1.0 && pvalue(sqrt(r2), n) <= pt && pvalue(sqrt(r2 * (1 - 1e-12)), n) > pt);
            }
        CHECK(r2_threshold(1.0, 10) == 0.0 && r2_threshold(2.0, 10) == 0.0 && r2_threshold(0.0, 10) == 1.0);
    }
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}
