/* dbtk_assoc_covar.h — covariates for the association scan of dbtk_assoc.h (`--assoc PHENO.tsv OUTPREF --assoc-covar COVAR.tsv`): the
 * scan regresses the covariates out of the rows AND of the phenotypes on the device and reports, for every tested (row, phenotype)
 * pair, the PARTIAL correlation given the covariates and the intercept.  t and p are those of x's coefficient in the multiple
 * regression y ~ 1 + C + x (Frisch-Waugh-Lovell); the degrees of freedom are dof = n - 2 - q.
 *
 * Replaces, in the reference's workflow: script/eqtl.noPerm.py (getTisSNPResTpmMat), which regresses the covariates out of the
 * expression matrix alone, (1 - C (C'C)^-1 C') Y.  That is not the multiple regression: the genotype row must be residualised too and
 * the test loses q degrees of freedom, and the rows exist in HBM only.
 *
 * The statistic.  The mask M has n samples, taken in ascending order as in dbtk_assoc.h.  C is n x q float64, column j covariate j
 * over M.
 *   dx and dy are the centred row and the centred phenotype, Sxx and Syy their sums of squares, exactly as in dbtk_assoc.h.
 *   Basis.  A host routine (dbtk_assoc_covar_basis) makes an orthonormal basis Q (n x q, float64) of the centred covariate columns,
 *     taken in file order, by modified Gram-Schmidt applied twice; deterministic.  Covariate j is COLLINEAR when the squared norm left
 *     after projecting out columns 0 .. j - 1 is <= DBTK_ASSOC_COVAR_COLLINEAR x its centred squared norm.  A constant covariate is
 *     collinear with the intercept.  A collinear covariate is refused by name.
 *   Projections.  a_j = sum_i dx_i Q_ij and b_j = sum_i dy_i Q_ij.
 *     Sxx' = Sxx - sum_j a_j^2     Syy' = Syy - sum_j b_j^2     Sxy' = Sxy - sum_j a_j b_j
 *     All three subtractions take j ascending, by fma, in the same order.
 *   Result per pair.  r = Sxy' / sqrt(Sxx' Syy'), clamped to [-1, 1]; slope = r; se = sqrt((1 - r^2) / dof); t = r / se; p is the
 *     two-sided t tail with dof degrees of freedom, that is dbtk_assoc_pvalue(r, n - q): the existing function with n - q in place of
 *     n.  The hit filter uses dbtk_assoc_r2_threshold(p, n - q).
 *   Rows not tested.  A row is not tested, and is counted in `skipped`, under the two conditions of dbtk_assoc.h (min == max, not
 *     finite), and also when Sxx' <= DBTK_ASSOC_COVAR_COLLINEAR x Sxx: the covariates explain it.
 *   Phenotypes refused.  A phenotype with Syy' <= DBTK_ASSOC_COVAR_COLLINEAR x Syy is refused by name when the covariates are set
 *     (DBTK_ERR_ARG).
 *   Refusals at set time.  n < q + 3; q > DBTK_ASSOC_COVAR_MAX.
 *   DBTK_ASSOC_COVAR_COLLINEAR is 1e-6.  It is a definition, not a tuning knob: the error bound of r grows as 1 / share; at a share of
 *     1e-6 and n + q of a few thousand the bound is still near 1e-6, so r keeps about six digits; a float32 row that is an exact
 *     combination of the covariates has a share of about 1e-13 from rounding alone; the threshold stands seven orders of magnitude
 *     away from both.
 *   DBTK_ASSOC_COVAR_MAX is 128 (GTEx's largest tissues carry 68 covariates): the a_j of a workgroup's 32 rows then take 32 KB of LDS
 *     beside the 32 KB of staged phenotypes, inside the CU's 160 KiB.
 *   Unchanged: n_tests, best row (largest r * r, ties to the lowest row), p_bonf, q, the sorted hit list, the columns and formats of
 *     both TSV files.
 *
 * Exactness.  The phenotypes' b_j come out of the same summation tree as the rows' a_j (a lane's samples ascending, lanes by xor
 * 32 ... 1, products by fma): a row that equals a phenotype bit for bit over M has a_j == b_j and Sxy' == Sxx' == Syy' bit for bit,
 * r == 1 and p == 0 exactly; duplicate rows tie bit for bit and the lower row wins.
 *
 * dbtk_assoc_scan_device, _pred, _dosage, dbtk_assoc_best, _hits and _write work unchanged on a handle that has covariates; without
 * covariates every byte is what dbtk_assoc.h alone gives.  This header has a version of its own: DBTK_ASSOC_API_VERSION and
 * DBTK_ABI_VERSION did not move when it was added.
 */
#ifndef DBTK_ASSOC_COVAR_H_
#define DBTK_ASSOC_COVAR_H_

#include <stdint.h>

#include "dbtk_assoc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBTK_ASSOC_COVAR_API_VERSION 1u
uint32_t dbtk_assoc_covar_api_version(void);

#define DBTK_ASSOC_COVAR_MAX 128u
#define DBTK_ASSOC_COVAR_COLLINEAR 1e-6

/* Host only, no device: covar[j * n + i] is covariate j in sample i, Q[j * n + i] the basis in the same layout.  DBTK_ERR_ARG with
 * *bad_column set: a value that is not finite, a constant or collinear column (the first such column in file order).  Q's columns
 * behind *bad_column are then not written. */
dbtk_status_t dbtk_assoc_covar_basis(uint64_t n, uint64_t q, const double* covar, double* Q, uint64_t* bad_column);

/* covar[j * n + i] is covariate j in sample sample_of[i] of dbtk_assoc_create; names[q] may be NULL (then "c0", "c1", ...).  The data
 * are copied.  q == 0 removes the covariates.  Computes Q, sends it to the device and makes the b_j and Syy' of every phenotype there.
 * The last scan's results are no longer valid afterwards.  DBTK_ERR_ARG: n < q + 3, q > DBTK_ASSOC_COVAR_MAX, a value that is not
 * finite, a constant or collinear covariate, a phenotype that the covariates explain (the message names it); the handle then keeps
 * the covariates it had.  DBTK_ERR_NOMEM with the sizes when the tables do not fit. */
dbtk_status_t dbtk_assoc_covar_set(dbtk_assoc_t* h, uint64_t q, const double* covar, const char* const* names);

/* *q the covariates of the handle (0: none), *dof = n - 2 - q the degrees of freedom of its tests. */
dbtk_status_t dbtk_assoc_covar_get(const dbtk_assoc_t* h, uint64_t* q, uint64_t* dof);

#ifdef __cplusplus
}
#endif
#endif
