// dbtk_assoc_host.h — the host half of the association scan (include/dbtk_assoc.h) that needs no device and no other part of the
// library: the two-sided Student-t tail of a correlation, Benjamini-Hochberg, the r^2 bound of a p-value threshold, and the parsers
// of PHENO.tsv and PAIRS.tsv.  Header only, so that tests/assoc_host_check.cpp compiles it alone under the sanitizers.
#ifndef DBTK_ASSOC_HOST_H_
#define DBTK_ASSOC_HOST_H_

#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

namespace dbtk_assoc_host {

constexpr uint64_t ALL_PAIRS_MAX = 64;  // phenotypes up to which a table may be scanned without a pair list

// The continued fraction of the regularised incomplete beta function (modified Lentz), for x < (a + 1) / (a + b + 2).
inline double beta_cf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 10000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < eps) break;
    }
    return h;
}
// ln Gamma(a + 1/2) - ln Gamma(a) without the cancellation of two lgamma calls: the asymptotic series in 1/a above a = 16,
// the recurrence Gamma(z + 1) = z Gamma(z) below (a is a multiple of 1/2 and >= 1/2 here).
inline double lgamma_half_ratio(double a) {
    double shift = 0.0;
    while (a < 16.0) { shift += log(a / (a + 0.5)); a += 1.0; }  // ratio(a) = ratio(a + 1) * a / (a + 1/2)
    const double i = 1.0 / a, i2 = i * i;
    // ln(Gamma(a + 1/2) / Gamma(a)) = ln(a)/2 - 1/(8a) + 1/(192a^3) - 1/(640a^5) + 17/(14336a^7) - 31/(18432a^9) + ...
    const double s = i * (-1.0 / 8 + i2 * (1.0 / 192 + i2 * (-1.0 / 640 + i2 * (17.0 / 14336 + i2 * (-31.0 / 18432 + i2 * (691.0 / 180224))))));
    return 0.5 * log(a) + s + shift;
}
// I_x(a, 1/2) given x and y = 1 - x, both exact to rounding (the caller forms them without cancellation)
inline double ibeta_half(double a, double x, double y) {
    if (x <= 0.0) return 0.0;
    if (y <= 0.0) return 1.0;
    const double b = 0.5;
    // ln of x^a y^b / B(a, b), B(a, 1/2) = Gamma(a) sqrt(pi) / Gamma(a + 1/2)
    const double lnfront = a * log(x) + b * log(y) + lgamma_half_ratio(a) - 0.5 * log(M_PI);
    if (x < (a + 1.0) / (a + b + 2.0)) return exp(lnfront) * beta_cf(a, b, x) / a;
    return 1.0 - exp(lnfront) * beta_cf(b, a, y) / b;
}
// Two-sided tail of Student's t with n - 2 degrees of freedom at t = r sqrt((n - 2) / (1 - r^2)): I_{1 - r^2}((n - 2) / 2, 1 / 2).
// n >= 3 and |r| <= 1 are the caller's to check; 0 where |r| = 1.
inline double pvalue(double r, uint64_t n) {
    const double ar = fabs(r);
    if (ar >= 1.0) return 0.0;
    const double x = (1.0 - ar) * (1.0 + ar);  // 1 - r^2 without the cancellation near |r| = 1
    const double p = ibeta_half(0.5 * (double)(n - 2), x, r * r);
    return p > 1.0 ? 1.0 : p;
}
// The smallest r^2 whose p-value is <= p_threshold (pvalue falls as r^2 grows): what the kernel compares with.  p_threshold >= 1
// gives 0 (every tested pair), p_threshold <= 0 gives 1 (|r| = 1 alone).
inline double r2_threshold(double p_threshold, uint64_t n) {
    if (!(p_threshold < 1.0)) return 0.0;
    if (!(p_threshold > 0.0)) return 1.0;
    double lo = 0.0, hi = 1.0;  // pvalue(sqrt(lo)) > p_threshold >= pvalue(sqrt(hi))
    for (int i = 0; i < 200 && lo < hi; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        if (pvalue(sqrt(mid), n) <= p_threshold) hi = mid; else lo = mid;
    }
    return hi;
}
// Benjamini-Hochberg as statsmodels' fdrcorrection and scipy's false_discovery_control: p sorted ascending, p_(i) m / i, the
// running minimum from the largest down, clipped at 1.  Ties keep their input order (a stable sort), which does not change q.
inline void bh(const double* p, uint64_t m, double* q) {
    std::vector<uint64_t> ord(m);
    std::iota(ord.begin(), ord.end(), (uint64_t)0);
    std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return p[a] < p[b]; });
    double run = INFINITY;
    for (uint64_t i = m; i-- > 0;) {
        const double v = p[ord[i]] * (double)m / (double)(i + 1);
        if (v < run) run = v;
        q[ord[i]] = run > 1.0 ? 1.0 : run;
    }
}

// ---- the two text files
struct PhenoTable {
    std::vector<std::string> names;    // P
    std::vector<uint64_t> sample_of;   // n: the sample of each line, in file order
    std::vector<double> values;        // [P][n]
};
inline void split_tabs(const std::string& line, std::vector<std::string>* out) {
    out->clear();
    size_t at = 0;
    for (;;) {
        const size_t t = line.find('\t', at);
        out->push_back(line.substr(at, t == std::string::npos ? std::string::npos : t - at));
        if (t == std::string::npos) break;
        at = t + 1;
    }
}
inline bool whole_uint(const std::string& s, uint64_t* v) {
    if (s.empty() || s.size() > 19) return false;
    uint64_t x = 0;
    for (char c : s) { if (c < '0' || c > '9') return false; x = x * 10 + (uint64_t)(c - '0'); }
    *v = x;
    return true;
}
inline bool whole_double(const std::string& s, double* v) {
    if (s.empty() || s[0] == ' ' || s[0] == '\t') return false;
    errno = 0;
    char* e = nullptr;
    const double x = strtod(s.c_str(), &e);
    if (e != s.c_str() + s.size() || !std::isfinite(x)) return false;  // (all of the field: a NUL inside it does not end it)
    *v = x;
    return true;
}
// PHENO.tsv from its text.  Header `id <TAB> NAME_1 ... NAME_P`, then `SAMPLE <TAB> v_1 ... v_P`; empty lines are skipped, a '\r' in
// front of the line end is dropped.  what: the file's name for the messages.
inline bool parse_pheno(const std::string& text, const std::string& what, PhenoTable* T, std::string* err) {
    std::istringstream in(text);
    std::string line;
    std::vector<std::string> f;
    std::vector<std::vector<double>> rows;
    std::unordered_map<uint64_t, uint64_t> seen;
    uint64_t ln = 0;
    bool header = false;
    T->names.clear(); T->sample_of.clear(); T->values.clear();
    while (std::getline(in, line)) {
        ++ln;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string at = what + ": line " + std::to_string(ln) + ": ";
        split_tabs(line, &f);
        if (!header) {
            if (f[0] != "id" || f.size() < 2) { *err = at + "the header must be id <TAB> NAME_1 <TAB> ... <TAB> NAME_P"; return false; }
            std::unordered_map<std::string, int> names;
            for (size_t i = 1; i < f.size(); ++i) {
                if (f[i].empty()) { *err = at + "empty phenotype name in column " + std::to_string(i + 1); return false; }
                if (names.count(f[i])) { *err = at + "phenotype " + f[i] + " is named twice"; return false; }
                names[f[i]] = 1;
                T->names.push_back(f[i]);
            }
            header = true;
            continue;
        }
        const size_t P = T->names.size();
        if (f.size() != P + 1) { *err = at + std::to_string(f.size()) + " fields, the header has " + std::to_string(P + 1); return false; }
        uint64_t s = 0;
        if (!whole_uint(f[0], &s)) { *err = at + "the sample must be its 0-based position in the cohort, not \"" + f[0] + "\""; return false; }
        if (seen.count(s)) { *err = at + "sample " + std::to_string(s) + " is given twice (first on line " + std::to_string(seen[s]) + ")"; return false; }
        seen[s] = ln;
        std::vector<double> v(P);
        for (size_t i = 0; i < P; ++i)
            if (!whole_double(f[i + 1], &v[i])) {
                *err = at + "phenotype " + T->names[i] + ": \"" + f[i + 1] + "\" is not a finite number (NA and empty fields are refused: impute beforehand)";
                return false;
            }
        T->sample_of.push_back(s);
        rows.push_back(std::move(v));
    }
    if (!header) { *err = what + ": no header line"; return false; }
    const size_t P = T->names.size(), n = rows.size();
    T->values.resize(P * n);
    for (size_t j = 0; j < n; ++j) for (size_t i = 0; i < P; ++i) T->values[i * n + j] = rows[j][i];
    return true;
}
// PAIRS.tsv from its text: lines of LOCUS <TAB> NAME, into CSR over the loci (off[ntr + 1], idx sorted within a locus); a line
// given twice counts once.  off == nullptr: the lines are checked and nothing is built (ntr may then be any bound).
inline bool parse_pairs(const std::string& text, const std::string& what, const std::vector<std::string>& names, uint64_t ntr, std::vector<uint64_t>* off,
                        std::vector<uint32_t>* idx, std::string* err) {
    std::unordered_map<std::string, uint32_t> id;
    for (size_t i = 0; i < names.size(); ++i) id[names[i]] = (uint32_t)i;
    std::vector<std::pair<uint64_t, uint32_t>> pr;
    std::istringstream in(text);
    std::string line;
    std::vector<std::string> f;
    uint64_t ln = 0;
    while (std::getline(in, line)) {
        ++ln;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string at = what + ": line " + std::to_string(ln) + ": ";
        split_tabs(line, &f);
        if (f.size() != 2) { *err = at + "expected LOCUS <TAB> NAME"; return false; }
        uint64_t l = 0;
        if (!whole_uint(f[0], &l)) { *err = at + "\"" + f[0] + "\" is not a locus number"; return false; }
        if (l >= ntr) { *err = at + "locus " + std::to_string(l) + " >= the build's " + std::to_string(ntr) + " loci"; return false; }
        const auto it = id.find(f[1]);
        if (it == id.end()) { *err = at + "unknown phenotype " + f[1]; return false; }
        pr.emplace_back(l, it->second);
    }
    if (!off || !idx) return true;
    std::sort(pr.begin(), pr.end());
    pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
    off->assign(ntr + 1, 0);
    idx->clear();
    for (const auto& q : pr) { ++(*off)[q.first + 1]; idx->push_back(q.second); }
    for (uint64_t t = 0; t < ntr; ++t) (*off)[t + 1] += (*off)[t];
    return true;
}
inline bool read_text(const std::string& fn, std::string* text, std::string* err) {
    std::ifstream f(fn, std::ios::binary);
    if (!f) { *err = "cannot open " + fn; return false; }
    std::ostringstream ss;
    ss << f.rdbuf();
    *text = ss.str();
    return true;
}

}  // namespace dbtk_assoc_host
#endif
