// dbtk_assoc_covar_host.h — the host half of the covariates of the association scan (include/dbtk_assoc_covar.h) that needs no device:
// the orthonormal basis of the centred covariate columns with its collinearity test, and COVAR.tsv matched to the samples of its
// PHENO.tsv.  Header only, so that tests/assoc_covar_host_check.cpp compiles it alone under the sanitizers.
#ifndef DBTK_ASSOC_COVAR_HOST_H_
#define DBTK_ASSOC_COVAR_HOST_H_

#include <math.h>
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "dbtk_assoc_host.h"

namespace dbtk_assoc_host {

constexpr uint64_t COVAR_MAX = 128;        // covariates of a table at most (DBTK_ASSOC_COVAR_MAX)
constexpr double COVAR_COLLINEAR = 1e-6;   // the residual share at or below which a column, a row or a phenotype counts as explained

// covar[q][n] -> Q[q][n]: column j is centred and cleared of columns 0 .. j - 1 by modified Gram-Schmidt applied twice, then scaled to
// norm 1.  Every dot product and norm is summed in ascending sample order in long double, so that what is left of the orthogonality
// error is the rounding of the stored float64 entries.  false with *bad the first column (in file order) that has a value that is not
// finite, is constant (min == max: collinear with the intercept), or keeps a squared norm <= COVAR_COLLINEAR x its centred squared norm
// after the columns before it are projected out; *finite tells the first case from the other two for the message.
inline bool covar_basis(uint64_t n, uint64_t q, const double* covar, double* Q, uint64_t* bad, bool* finite = nullptr) {
    std::vector<long double> v(n);
    if (finite) *finite = true;
    for (uint64_t j = 0; j < q; ++j) {
        const double* c = covar + j * n;
        *bad = j;
        double mn = INFINITY, mx = -INFINITY;
        long double sum = 0.0L;
        for (uint64_t i = 0; i < n; ++i) {
            if (!std::isfinite(c[i])) { if (finite) *finite = false; return false; }
            mn = c[i] < mn ? c[i] : mn; mx = c[i] > mx ? c[i] : mx;
            sum += c[i];
        }
        if (!(mn < mx)) return false;
        const long double mean = sum / (long double)n;
        long double norm0 = 0.0L;
        for (uint64_t i = 0; i < n; ++i) { v[i] = (long double)c[i] - mean; norm0 += v[i] * v[i]; }
        for (int pass = 0; pass < 2; ++pass)
            for (uint64_t k = 0; k < j; ++k) {
                const double* qk = Q + k * n;
                long double dot = 0.0L;
                for (uint64_t i = 0; i < n; ++i) dot += v[i] * (long double)qk[i];
                for (uint64_t i = 0; i < n; ++i) v[i] -= dot * (long double)qk[i];
            }
        long double rem = 0.0L;
        for (uint64_t i = 0; i < n; ++i) rem += v[i] * v[i];
        if (!(rem > (long double)COVAR_COLLINEAR * norm0) || !std::isfinite((double)rem)) return false;
        const long double s = sqrtl(rem);
        double* out = Q + j * n;
        for (uint64_t i = 0; i < n; ++i) out[i] = (double)(v[i] / s);
    }
    return true;
}

// The covariates of a table as dbtk_assoc_covar_set takes them: values[q][n], sample j = T.sample_of[j] of the phenotype table.
struct Covariates {
    std::vector<std::string> names;
    std::vector<double> values;
};
// COVAR.tsv (parsed by parse_pheno: the same layout) against its PHENO.tsv: the same samples, in any order; q <= COVAR_MAX; n >= q + 3;
// no constant or collinear column.  what: the file's name for the messages.
inline bool match_covar(const PhenoTable& pheno, const PhenoTable& covar, const std::string& what, Covariates* out, std::string* err) {
    const uint64_t n = pheno.sample_of.size(), q = covar.names.size(), nc = covar.sample_of.size();
    std::unordered_map<uint64_t, uint64_t> at;
    for (uint64_t j = 0; j < nc; ++j) at[covar.sample_of[j]] = j;
    std::unordered_map<uint64_t, int> listed;
    for (uint64_t s : pheno.sample_of) listed[s] = 1;
    for (uint64_t s : covar.sample_of)
        if (!listed.count(s)) { *err = what + ": sample " + std::to_string(s) + " is not listed in the phenotype table"; return false; }
    for (uint64_t s : pheno.sample_of)
        if (!at.count(s)) { *err = what + ": sample " + std::to_string(s) + " of the phenotype table is missing"; return false; }
    if (q > COVAR_MAX) { *err = what + " holds " + std::to_string(q) + " covariates: at most " + std::to_string(COVAR_MAX) + " are allowed"; return false; }
    if (n < q + 3) {
        *err = what + ": " + std::to_string(n) + " samples and " + std::to_string(q) + " covariates: a test needs at least q + 3 samples (n - 2 - q degrees of freedom)";
        return false;
    }
    out->names = covar.names;
    out->values.resize(q * n);
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t src = at[pheno.sample_of[j]];
        for (uint64_t c = 0; c < q; ++c) out->values[c * n + j] = covar.values[c * nc + src];
    }
    std::vector<double> Q(q * n);
    uint64_t bad = 0;
    if (!covar_basis(n, q, out->values.data(), Q.data(), &bad)) {
        *err = what + ": covariate " + covar.names[bad] + " is constant or collinear with the intercept and the covariates in front of it";
        return false;
    }
    return true;
}

}  // namespace dbtk_assoc_host
#endif
