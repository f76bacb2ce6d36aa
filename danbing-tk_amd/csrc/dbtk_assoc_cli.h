// dbtk_assoc_cli.h — the --assoc flags as both command lines take them (danbing-tk-pred and danbing-tk --cohort): the flag group, what
// is checked at parse time before a device is touched, and the scans of one resident matrix table after table.
//   --assoc PHENO.tsv OUTPREF [--assoc-covar COVAR.tsv] [--assoc-pairs PAIRS.tsv] [--assoc-p X] [--assoc-raw] [--assoc-perm B [--assoc-seed S]]
//                                                                                                                  (the group may be repeated)
#ifndef DBTK_ASSOC_CLI_H_
#define DBTK_ASSOC_CLI_H_

#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/dbtk_assoc.h"
#include "../../include/dbtk_assoc_covar.h"
#include "../../include/dbtk_assoc_perm.h"
#include "dbtk_assoc_covar_host.h"
#include "dbtk_assoc_host.h"
#include "dbtk_assoc_perm_host.h"

namespace dbtk_assoc_cli {

struct Group {
    std::string pheno, prefix, pairs, pairs_text, covar;
    double p = -1.0;   // --assoc-p; negative: no hit list
    bool raw = false;  // --assoc-raw: the matrix before the bias correction
    uint64_t perm = 0, seed = 1;  // --assoc-perm B (0: none) and --assoc-seed S
    bool has_seed = false;
    dbtk_assoc_host::PhenoTable table;
    dbtk_assoc_host::Covariates covariates;  // --assoc-covar: the columns of COVAR.tsv in the table's sample order
};
struct Options {
    std::vector<Group> groups;
    bool any() const { return !groups.empty(); }
    bool any_raw() const { for (const Group& g : groups) if (g.raw) return true; return false; }
};

// Takes argv[argi] when it is one of the flags: returns the number of arguments used, 0 when it is not one, -1 with *err set.
inline int take_flag(Options* o, int argc, char** argv, int argi, std::string* err) {
    const std::string a = argv[argi];
    if (a.compare(0, 7, "--assoc") != 0) return 0;
    auto last = [&]() -> Group* {
        if (o->groups.empty()) { *err = a + " needs --assoc PHENO.tsv OUTPREF in front of it"; return nullptr; }
        return &o->groups.back();
    };
    if (a == "--assoc") {
        if (argi + 2 >= argc) { *err = "--assoc: expected PHENO.tsv OUTPREF"; return -1; }
        Group g;
        g.pheno = argv[argi + 1]; g.prefix = argv[argi + 2];
        o->groups.push_back(g);
        return 3;
    }
    if (a == "--assoc-pairs") {
        Group* g = last();
        if (!g) return -1;
        if (argi + 1 >= argc) { *err = "--assoc-pairs: expected PAIRS.tsv"; return -1; }
        g->pairs = argv[argi + 1];
        return 2;
    }
    if (a == "--assoc-covar") {
        Group* g = last();
        if (!g) return -1;
        if (argi + 1 >= argc) { *err = "--assoc-covar: expected COVAR.tsv"; return -1; }
        if (!g->covar.empty()) { *err = std::string("--assoc-covar: given twice for ") + g->pheno + " (" + g->covar + " and " + argv[argi + 1] + "): one covariate file per --assoc"; return -1; }
        if (!*argv[argi + 1]) { *err = "--assoc-covar: empty file name"; return -1; }
        g->covar = argv[argi + 1];
        return 2;
    }
    if (a == "--assoc-p") {
        Group* g = last();
        if (!g) return -1;
        if (argi + 1 >= argc) { *err = "--assoc-p: expected a p-value"; return -1; }
        double v = 0;
        if (!dbtk_assoc_host::whole_double(argv[argi + 1], &v) || v < 0.0 || v > 1.0) { *err = std::string("--assoc-p: not a p-value in [0, 1]: ") + argv[argi + 1]; return -1; }
        g->p = v;
        return 2;
    }
    if (a == "--assoc-perm") {
        Group* g = last();
        if (!g) return -1;
        if (argi + 1 >= argc) { *err = "--assoc-perm: expected the number of permutations"; return -1; }
        if (g->perm) { *err = std::string("--assoc-perm: given twice for ") + g->pheno + ": one number of permutations per --assoc"; return -1; }
        uint64_t v = 0;
        if (!dbtk_assoc_host::whole_uint(argv[argi + 1], &v) || v < 1 || v > DBTK_ASSOC_PERM_MAX) {
            *err = std::string("--assoc-perm: not an integer in 1 .. ") + std::to_string(DBTK_ASSOC_PERM_MAX) + ": " + argv[argi + 1];
            return -1;
        }
        g->perm = v;
        return 2;
    }
    if (a == "--assoc-seed") {
        Group* g = last();
        if (!g) return -1;
        if (argi + 1 >= argc) { *err = "--assoc-seed: expected a seed"; return -1; }
        if (!dbtk_assoc_host::whole_u64(argv[argi + 1], &g->seed)) { *err = std::string("--assoc-seed: not an unsigned 64-bit integer: ") + argv[argi + 1]; return -1; }
        g->has_seed = true;
        return 2;
    }
    if (a == "--assoc-raw") {
        Group* g = last();
        if (!g) return -1;
        g->raw = true;
        return 1;
    }
    return 0;
}

// Everything that can be refused without a device: the tables are read and parsed, the pair files are read and parsed for their form
// and their names (their loci are checked against the build in run()), the output files are created and removed again.
inline bool load(Options* o, bool dosage, std::string* err) {
    for (Group& g : o->groups) {
        std::string text;
        if (g.has_seed && !g.perm) { *err = "--assoc-seed: needs --assoc-perm in the same --assoc group (" + g.pheno + ")"; return false; }
        if (dosage && g.raw) { *err = "--assoc-raw: the dosage values have no uncorrected form to scan (--assoc-raw goes with the genotype matrix)"; return false; }
        if (!dbtk_assoc_host::read_text(g.pheno, &text, err)) { *err = "--assoc: " + *err; return false; }
        if (!dbtk_assoc_host::parse_pheno(text, g.pheno, &g.table, err)) { *err = "--assoc: " + *err; return false; }
        if (g.table.sample_of.size() < 3) { *err = "--assoc: " + g.pheno + " lists " + std::to_string(g.table.sample_of.size()) + " samples: a test needs at least 3"; return false; }
        if (g.pairs.empty() && g.table.names.size() > DBTK_ASSOC_ALL_PAIRS_MAX) {
            *err = "--assoc: " + g.pheno + " holds " + std::to_string(g.table.names.size()) + " phenotypes: more than " + std::to_string(DBTK_ASSOC_ALL_PAIRS_MAX) +
                   " need --assoc-pairs (every phenotype against every row is allowed up to that number)";
            return false;
        }
        if (!g.pairs.empty()) {
            if (!dbtk_assoc_host::read_text(g.pairs, &g.pairs_text, err)) { *err = "--assoc-pairs: " + *err; return false; }
            if (!dbtk_assoc_host::parse_pairs(g.pairs_text, g.pairs, g.table.names, 0xFFFFFFFFull, nullptr, nullptr, err)) { *err = "--assoc-pairs: " + *err; return false; }
        }
        if (!g.covar.empty()) {  // the same layout and parser as PHENO.tsv; the basis needs no device, so a collinear covariate is refused here
            dbtk_assoc_host::PhenoTable C;
            if (!dbtk_assoc_host::read_text(g.covar, &text, err)) { *err = "--assoc-covar: " + *err; return false; }
            if (!dbtk_assoc_host::parse_pheno(text, g.covar, &C, err)) { *err = "--assoc-covar: " + *err; return false; }
            if (!dbtk_assoc_host::match_covar(g.table, C, g.covar, &g.covariates, err)) { *err = "--assoc-covar: " + *err; return false; }
        }
        for (const char* ext : {".assoc.best.tsv", ".assoc.hits.tsv", ".assoc.perm.tsv"}) {
            if (!g.perm && std::string(ext) == ".assoc.perm.tsv") continue;
            const std::string fn = g.prefix + ext;
            FILE* f = fopen(fn.c_str(), "w");
            if (!f) { *err = "--assoc: cannot create " + fn; return false; }
            fclose(f);
            (void)remove(fn.c_str());
        }
    }
    return true;
}

// The scans of the groups with raw == raw_stage over one resident matrix: scan(handle, p_threshold, perm) is dbtk_assoc_scan_pred or
// dbtk_assoc_scan_dosage on the caller's handle, with perm their dbtk_assoc_perm_scan_ twins.  A line per table goes to `log`.
template <class Scan>
inline bool run(Options* o, bool raw_stage, int device, uint64_t ns, uint64_t ntr, Scan scan, FILE* log, std::string* err) {
    for (Group& g : o->groups) {
        if (g.raw != raw_stage) continue;
        const dbtk_assoc_host::PhenoTable& T = g.table;
        std::vector<const char*> names;
        for (const std::string& s : T.names) names.push_back(s.c_str());
        for (uint64_t s : T.sample_of)
            if (s >= ns) { *err = "--assoc: " + g.pheno + " names sample " + std::to_string(s) + ", the cohort has " + std::to_string(ns); return false; }
        dbtk_assoc_t* h = nullptr;
        if (dbtk_assoc_create(device, ns, T.names.size(), T.sample_of.size(), T.sample_of.data(), T.values.data(), names.data(), &h)) { *err = "--assoc: " + g.pheno + ": " + dbtk_last_error(); return false; }
        bool ok = true;
        if (!g.pairs.empty()) {
            std::vector<uint64_t> off;
            std::vector<uint32_t> idx;
            if (!dbtk_assoc_host::parse_pairs(g.pairs_text, g.pairs, T.names, ntr, &off, &idx, err)) { *err = "--assoc-pairs: " + *err; ok = false; }
            else if (dbtk_assoc_set_pairs(h, ntr, off.data(), idx.data())) { *err = "--assoc-pairs: " + std::string(dbtk_last_error()); ok = false; }
        }
        if (ok && !g.covar.empty()) {
            std::vector<const char*> cn;
            for (const std::string& s : g.covariates.names) cn.push_back(s.c_str());
            uint64_t q = 0, dof = 0;
            if (dbtk_assoc_covar_set(h, cn.size(), g.covariates.values.data(), cn.data()) || dbtk_assoc_covar_get(h, &q, &dof)) { *err = "--assoc-covar: " + g.covar + ": " + dbtk_last_error(); ok = false; }
            else fprintf(stderr, "# assoc %s: n %zu, %llu covariates, dof %llu\n", g.prefix.c_str(), T.sample_of.size(), (unsigned long long)q, (unsigned long long)dof);
        }
        if (ok && g.perm && dbtk_assoc_perm_seed(h, g.perm, g.seed)) { *err = "--assoc-perm: " + g.pheno + ": " + dbtk_last_error(); ok = false; }
        if (ok && scan(h, g.p, g.perm != 0)) { *err = "--assoc: " + g.pheno + ": " + dbtk_last_error(); ok = false; }
        if (ok && dbtk_assoc_write(h, g.prefix.c_str())) { *err = "--assoc: " + std::string(dbtk_last_error()); ok = false; }
        if (ok && g.perm) {
            double pms[2] = {0, 0};
            if (dbtk_assoc_perm_write(h, g.prefix.c_str()) || dbtk_assoc_perm_times(h, pms)) { *err = "--assoc-perm: " + std::string(dbtk_last_error()); ok = false; }
            else fprintf(stderr, "# assoc %s: %llu permutations, seed %llu, %.3f ms\n", g.prefix.c_str(), (unsigned long long)g.perm, (unsigned long long)g.seed, pms[0]);
        }
        if (ok && log) {
            double ms[2] = {0, 0};
            dbtk_assoc_times(h, ms);
            fprintf(log, "association scan of %s (%zu phenotypes, %zu samples%s): %.3f ms on the GPU, written to %s.assoc.best.tsv\n", g.pheno.c_str(), T.names.size(),
                    T.sample_of.size(), g.raw ? ", raw matrix" : "", ms[0], g.prefix.c_str());
        }
        dbtk_assoc_free(h);
        if (!ok) return false;
    }
    return true;
}

inline const char* usage() {
    return "  --assoc <PHENO.tsv> <OUTPREF> [--assoc-covar <COVAR.tsv>] [--assoc-pairs <PAIRS.tsv>] [--assoc-p <X>] [--assoc-raw]\n"
           "          [--assoc-perm <B> [--assoc-seed <S>]]\n"
           "                  association scan of the matrix (or the dosage values) while it lies in HBM: every row against the\n"
           "                  phenotypes of PHENO.tsv (id <TAB> NAME_1 ... / sample position <TAB> values; samples not listed are\n"
           "                  masked out), or against the phenotypes PAIRS.tsv (LOCUS <TAB> NAME) gives its locus; writes\n"
           "                  OUTPREF.assoc.best.tsv (best row per phenotype, Bonferroni and Benjamini-Hochberg) and, with\n"
           "                  --assoc-p, OUTPREF.assoc.hits.tsv (every pair with p <= X); --assoc-raw scans before the bias\n"
           "                  correction; --assoc-covar regresses the covariates of COVAR.tsv (the layout of PHENO.tsv, the same\n"
           "                  samples, at most 128 columns) out of the rows and the phenotypes on the device: r is then the partial\n"
           "                  correlation, t and p those of y ~ 1 + C + x with n - 2 - q degrees of freedom; the group may be\n"
           "                  repeated, one scan per table, each with its own covariates; --assoc-perm permutes the phenotypes (with\n"
           "                  covariates their residuals) over the samples B times on the device, seeded by S (default 1), and\n"
           "                  writes OUTPREF.assoc.perm.tsv: per phenotype the best r^2, the permutations that reach it and the\n"
           "                  permutation p-value (n_ge + 1) / (B + 1) with its Benjamini-Hochberg q\n";
}

}  // namespace dbtk_assoc_cli
#endif
