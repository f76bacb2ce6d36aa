// assoc_covar_host_check.cpp — the host half of the covariates of the association scan (csrc/dbtk_assoc_covar_host.h) stand-alone: built
// with -fsanitize=address,undefined and run by tests/test_assoc_covar_host.py.  The basis routine on good and on collinear columns,
// COVAR.tsv through the table parser on hostile text, and its matching to the samples of PHENO.tsv.
// Prints "ok" and returns 0, or the first failed check and 1.
#include <math.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "dbtk_assoc_covar_host.h"

using namespace dbtk_assoc_host;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static double dot(const double* a, const double* b, uint64_t n) {
    long double s = 0;
    for (uint64_t i = 0; i < n; ++i) s += (long double)a[i] * b[i];
    return (double)s;
}
// a small generator of its own, so that the columns are the same on every machine
static double next(uint64_t* s) {
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(*s >> 11) / 9007199254740992.0 - 0.5;
}
static bool covar_fails(const std::string& pheno, const std::string& covar, const std::string& part) {
    PhenoTable T, C;
    Covariates out;
    std::string err;
    if (!parse_pheno(pheno, "P", &T, &err)) { printf("  the phenotype table itself: %s\n", err.c_str()); return false; }
    if (parse_pheno(covar, "C", &C, &err) && match_covar(T, C, "C", &out, &err)) { printf("  accepted: %s\n", covar.c_str()); return false; }
    if (err.find(part) == std::string::npos) { printf("  message \"%s\" lacks \"%s\"\n", err.c_str(), part.c_str()); return false; }
    return true;
}

int main() {
    const double u = ldexp(1.0, -53);
    for (uint64_t n : {4, 17, 64, 300})
        for (uint64_t q : {0, 1, 2, 9, 128}) {
            if (n < q + 3) continue;
            uint64_t seed = n * 1000 + q;
            std::vector<double> c(q * n), Q(q * n, 7.0), Q2(q * n, 9.0);
            for (double& v : c) v = 3.0 * next(&seed) + floor(4.0 * next(&seed));
            uint64_t bad = 99;
            CHECK(covar_basis(n, q, c.data(), Q.data(), &bad));
            CHECK(covar_basis(n, q, c.data(), Q2.data(), &bad) && Q == Q2);   // the same bytes on a second call
            std::vector<double> one(n, 1.0);
            for (uint64_t j = 0; j < q; ++j) {
                CHECK(fabs(dot(&Q[j * n], one.data(), n)) <= 8 * u * sqrt((double)n));   // orthogonal to the intercept
                for (uint64_t k = 0; k <= j; ++k) CHECK(fabs(dot(&Q[j * n], &Q[k * n], n) - (j == k)) <= 8 * q * u);
            }
        }
    {   // the refusals, each with its column
        const uint64_t n = 9;
        uint64_t seed = 5, bad = 99;
        std::vector<double> c(4 * n), Q(4 * n);
        auto fill = [&] { for (double& v : c) v = next(&seed); };
        bool finite = false;
        fill(); for (uint64_t i = 0; i < n; ++i) c[2 * n + i] = 0.1;                                   // constant (0.1 has no exact mean)
        CHECK(!covar_basis(n, 4, c.data(), Q.data(), &bad, &finite) && bad == 2 && finite);
        fill(); for (uint64_t i = 0; i < n; ++i) c[3 * n + i] = c[1 * n + i];                          // a column given twice
        CHECK(!covar_basis(n, 4, c.data(), Q.data(), &bad, &finite) && bad == 3 && finite);
        fill(); for (uint64_t i = 0; i < n; ++i) c[2 * n + i] = c[i] + c[1 * n + i] + 5.0;             // the sum of two others and the intercept
        CHECK(!covar_basis(n, 4, c.data(), Q.data(), &bad, &finite) && bad == 2 && finite);
        fill(); for (uint64_t i = 0; i < n; ++i) c[1 * n + i] = 2.0 * c[i] + 1e-5 * c[1 * n + i];      // all but a 2.5e-11 share explained
        CHECK(!covar_basis(n, 4, c.data(), Q.data(), &bad, &finite) && bad == 1);
        fill(); for (uint64_t i = 0; i < n; ++i) c[1 * n + i] = 2.0 * c[i] + 1e-1 * c[1 * n + i];      // a 2.5e-3 share is left: fine
        CHECK(covar_basis(n, 4, c.data(), Q.data(), &bad, &finite));
        fill(); c[3 * n + 4] = NAN;
        CHECK(!covar_basis(n, 4, c.data(), Q.data(), &bad, &finite) && bad == 3 && !finite);
        fill(); c[0] = INFINITY;
        CHECK(!covar_basis(n, 4, c.data(), Q.data(), &bad, &finite) && bad == 0 && !finite);
        fill(); c[5] = 1e200; c[6] = -1e200;                                                           // a squared norm that overflows
        CHECK(!covar_basis(n, 1, c.data(), Q.data(), &bad, &finite) || std::isfinite(Q[5]));
        CHECK(covar_basis(0, 0, nullptr, nullptr, &bad));
    }
    const std::string pheno = "id\tg\n4\t1\n0\t2\n7\t4\n2\t8\n9\t3\n";
    {   // a covariate file as it should be: other line order, CRLF; the columns come out in the phenotype table's sample order
        PhenoTable T, C;
        Covariates out;
        std::string err;
        CHECK(parse_pheno(pheno, "P", &T, &err));
        CHECK(parse_pheno("id\tsex\tpc1\r\n0\t1\t0.5\r\n2\t0\t-1.5\r\n\r\n9\t1\t2.5\n7\t0\t0.25\n4\t1\t-3\n", "C", &C, &err));
        CHECK(match_covar(T, C, "C", &out, &err));
        CHECK(out.names.size() == 2 && out.names[1] == "pc1" && out.values.size() == 10);
        CHECK(out.values[0] == 1 && out.values[1] == 1 && out.values[2] == 0 && out.values[3] == 0 && out.values[4] == 1);
        CHECK(out.values[5] == -3 && out.values[6] == 0.5 && out.values[7] == 0.25 && out.values[8] == -1.5 && out.values[9] == 2.5);
    }
    CHECK(covar_fails(pheno, "", "no header"));
    CHECK(covar_fails(pheno, "id\n", "line 1: the header"));
    CHECK(covar_fails(pheno, "id\ta\n0\t1\n2\tNA\n", "line 3: phenotype a: \"NA\""));
    CHECK(covar_fails(pheno, "id\ta\n0\t\n", "line 2: phenotype a: \"\""));
    CHECK(covar_fails(pheno, "id\ta\n0\t1\n2\tx\n", "line 3"));
    CHECK(covar_fails(pheno, "id\ta\n0\t1\n0\t2\n", "line 3: sample 0 is given twice"));
    CHECK(covar_fails(pheno, "id\ta\n0\t1\n2\t2\n4\t3\n7\t5\n9\t1\n3\t1\n", "sample 3 is not listed in the phenotype table"));
    CHECK(covar_fails(pheno, "id\ta\n0\t1\n2\t2\n4\t3\n9\t1\n", "sample 7 of the phenotype table is missing"));
    CHECK(covar_fails(pheno, "id\ta\tb\tc\n0\t1\t2\t3\n2\t2\t1\t1\n4\t3\t3\t0\n7\t5\t1\t2\n9\t1\t0\t7\n", "5 samples and 3 covariates"));
    CHECK(covar_fails(pheno, "id\ta\tb\n0\t1\t2\n2\t2\t2\n4\t3\t2\n7\t5\t2\n9\t1\t2\n", "covariate b is constant or collinear"));
    CHECK(covar_fails(pheno, "id\ta\tb\n0\t1\t3\n2\t2\t5\n4\t3\t7\n7\t5\t11\n9\t1\t3\n", "covariate b is constant or collinear"));
    {   // more columns than the cap, over enough samples
        std::string ph = "id\tg\n", cv = "id";
        for (int j = 0; j < 129; ++j) cv += "\tc" + std::to_string(j);
        cv += "\n";
        uint64_t seed = 9;
        for (int s = 0; s < 140; ++s) {
            ph += std::to_string(s) + "\t" + std::to_string(s % 7) + "\n";
            cv += std::to_string(s);
            for (int j = 0; j < 129; ++j) cv += "\t" + std::to_string(next(&seed));
            cv += "\n";
        }
        CHECK(covar_fails(ph, cv, "holds 129 covariates: at most 128"));
    }
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}
