/* dbtk_assoc_perm.h — permutation p-values for the association scan of dbtk_assoc.h (`--assoc PHENO.tsv OUTPREF --assoc-perm B`): the
 * phenotypes are permuted over the samples B times on the device, the best r^2 over the SAME tested rows is taken each time, and a
 * phenotype's p-value is the share of permutations whose best statistic reaches the observed one.  This is how FastQTL, tensorQTL and
 * GTEx call an eGene; the Bonferroni p of dbtk_assoc.h over the strongly correlated rows of a locus is very conservative beside it.
 *
 * Adds to the reference's workflow what script/eqtl.noPerm.py leaves out by name.
 *
 * The statistic.  The mask M has n samples, taken in ascending order as in dbtk_assoc.h: positions 0 .. n - 1.
 *   A permutation pi is a bijection of these positions; the permuted phenotype is (y o pi)[i] = y[pi[i]].
 *   With covariates (dbtk_assoc_covar_set) what is permuted is the phenotype's RESIDUAL y~ = dy - sum_j b_j Q_j after the intercept and
 *     the covariates; the rows are residualised as the scan does, x~ = dx - sum_j a_j Q_j.  The residual is NOT projected again after
 *     the permutation: this is FastQTL's scheme (the permuted residual is no longer exactly orthogonal to the covariates).
 *   For phenotype p and permutation b, T_b(p) = max over the tested rows paired with p of r_b^2,
 *     r_b = Sxy_b / sqrt(Sxx Syy)           Sxy_b = sum_i dx_i dy[pi_b[i]]           without covariates,
 *     r_b = Sxy_b / sqrt(Sxx' Syy')         Sxy_b = sum_i x~_i y~[pi_b[i]]           with them,
 *     in float64 on the widened float32 entries, r clamped to [-1, 1] before it is squared.  Sxx, Syy (Sxx', Syy'), which rows are
 *     tested or skipped and n_tests are those of the scan and do not depend on b.
 *   Slot b = 0 is the identity.  It goes through the same kernel code and the same summation order as every other slot (the table on
 *     the device carries the identity as its row 0), so a permutation with y o pi_b byte-equal to y ties with T_0 bit for bit and
 *     counts as >=.
 *   Per phenotype: n_ge = #{b in 1 .. B : T_b >= T_0}, p_perm = (n_ge + 1) / (B + 1), q_perm = Benjamini-Hochberg (dbtk_assoc_bh) over
 *     the p_perm of the phenotypes that have tests.  A phenotype without tests has n_ge = 0 and p_perm = q_perm = 0 (NA in the file).
 *   Left out: FastQTL's beta approximation of the null and adaptive (early-stopping) permutation.
 *
 * The permutations are shared by all phenotypes of a handle (as in tensorQTL).  They come from the caller, or from a seed:
 *   The generator is one splitmix64 stream, all in uint64:
 *     s = seed
 *     next(): s += 0x9E3779B97F4A7C15; z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *             return z ^ (z >> 31)
 *   Permutations b = 1 .. B are drawn in that order from the one stream.  Each starts from the identity; for i = n - 1 down to 1:
 *     j = (next() * (i + 1)) >> 64, the high half of the 128-bit product, then pi[i] and pi[j] are exchanged.
 *   So the first B' permutations of a B-run are the B'-run's.
 *
 * Determinism.  Every sum's order depends on n alone; the maxima are folded with an integer atomic max on the bit pattern of the
 * non-negative float64, whose result does not depend on the order: the same inputs give the same bytes on every run.
 *
 * This header has a version of its own: DBTK_ASSOC_API_VERSION, DBTK_ASSOC_COVAR_API_VERSION and DBTK_ABI_VERSION did not move when it
 * was added, and nothing that dbtk_assoc.h and dbtk_assoc_covar.h give changes by a byte.
 */
#ifndef DBTK_ASSOC_PERM_H_
#define DBTK_ASSOC_PERM_H_

#include <stdint.h>

#include "dbtk_assoc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBTK_ASSOC_PERM_API_VERSION 1u
uint32_t dbtk_assoc_perm_api_version(void);

#define DBTK_ASSOC_PERM_MAX 1000000u

typedef struct dbtk_assoc_perm_result {
    uint64_t n_perm;  /* B */
    uint64_t n_ge;    /* permutations b in 1 .. B with T_b >= T_0 */
    uint32_t row;     /* the best row of the ordinary scan made by the same call (DBTK_ASSOC_NONE: no tests) */
    uint32_t pad;
    double r2;        /* T_0 as the permutation kernel made it */
    double p_perm;    /* (n_ge + 1) / (B + 1) */
    double q_perm;    /* Benjamini-Hochberg over the phenotypes that have tests */
} dbtk_assoc_perm_result_t;

/* Host only, no device: perm[(b - 1) * n + i] = pi_b[i] for b = 1 .. B by the generator above. */
dbtk_status_t dbtk_assoc_perm_generate(uint64_t n, uint64_t B, uint64_t seed, uint32_t* perm);

/* perm[B][n] over the positions 0 .. n - 1 of the handle's mask in ascending sample order; the data are copied.  B == 0 removes the
 * permutations.  DBTK_ERR_ARG: B > DBTK_ASSOC_PERM_MAX, a row that is not a permutation of 0 .. n - 1 (the message names the first).
 * DBTK_ERR_NOMEM with the sizes (the table, the P (B + 1) maxima, free HBM) before any work.  The last permutation result is no longer
 * valid afterwards (setting covariates invalidates it too).  A refused call leaves the permutations the handle had. */
dbtk_status_t dbtk_assoc_perm_set(dbtk_assoc_t* h, uint64_t B, const uint32_t* perm);
/* The same with the permutations of dbtk_assoc_perm_generate(n, B, seed). */
dbtk_status_t dbtk_assoc_perm_seed(dbtk_assoc_t* h, uint64_t B, uint64_t seed);
/* *B the permutations of the handle (0: none); perm, when not NULL, receives the first min(cap, B) rows. */
dbtk_status_t dbtk_assoc_perm_get(const dbtk_assoc_t* h, uint64_t* B, uint32_t* perm, uint64_t cap);

/* The twins of dbtk_assoc_scan_device, _pred and _dosage with the same arguments: they make the ordinary scan first, so dbtk_assoc_best,
 * _hits and _write give exactly what the twin gives, and then the permutation pass over the same rows.  They refuse what the twin
 * refuses, and DBTK_ERR_ARG when no permutations are set. */
dbtk_status_t dbtk_assoc_perm_scan_device(dbtk_assoc_t* h, const float* d_rows, uint64_t nrows, uint64_t ntr, const uint32_t* nk_cum, double p_threshold);
dbtk_status_t dbtk_assoc_perm_scan_pred(dbtk_assoc_t* h, dbtk_pred_t* pred, double p_threshold);
dbtk_status_t dbtk_assoc_perm_scan_dosage(dbtk_assoc_t* h, dbtk_dosage_t* dosage, double p_threshold);

/* out[P] in table order. */
dbtk_status_t dbtk_assoc_perm_results(dbtk_assoc_t* h, dbtk_assoc_perm_result_t* out);
/* T[B + 1]: all maxima of phenotype p, T[0] the observed one (all 0 for a phenotype without tests). */
dbtk_status_t dbtk_assoc_perm_stats(dbtk_assoc_t* h, uint64_t p, double* T);
/* PREFIX.assoc.perm.tsv: pheno n_tests row r2 n_perm n_ge p_perm q_perm, doubles as %.6e, in table order; NA for a phenotype without tests. */
dbtk_status_t dbtk_assoc_perm_write(dbtk_assoc_t* h, const char* out_prefix);
/* ms[0]: the permutation kernel by HIP events, ms[1]: the host fold, of the last permutation scan. */
dbtk_status_t dbtk_assoc_perm_times(dbtk_assoc_t* h, double ms[2]);

#ifdef __cplusplus
}
#endif
#endif
