/* dbtk_assoc.h — C-ABI of the association scan (`--assoc PHENO.tsv OUTPREF`), on one MI355X: every row of a float32 matrix that
 * lies in HBM (the cohort's genotype matrix of dbtk_pred_t, the dosage values of dbtk_dosage_t, or any [nrows][ns] matrix) is tested
 * against phenotype vectors, without the matrix leaving the device.
 *
 * Replaces, in the reference's workflow: script/eqtl.noPerm.py (runRegressionZ3), which z-scores a (locus, gene) pair, fits
 * sm.OLS(y, add_constant(x)), keeps slope, standard error and p-value and the best TR per gene after Bonferroni correction, and runs
 * Benjamini-Hochberg over the genes.
 *
 * The statistic.  Rows are float32 vectors over the cohort's ns samples.  A table gives P float64 phenotype vectors over a subset M of
 * the samples, n = |M|; samples outside M are ignored for every phenotype of the table (one mask per table).  For row x and
 * phenotype y over s in M, in float64, the matrix entry widened first:
 *   mx = sum x / n   Sxx = sum (x - mx)^2   (likewise my, Syy)   r = sum (x - mx)(y - my) / sqrt(Sxx Syy), clamped to [-1, 1]
 *   slope = r   se = sqrt((1 - r^2) / (n - 2))   t = r / se   p = two-sided Student-t tail, n - 2 degrees of freedom; 0 where |r| = 1
 * which is what ordinary least squares with an intercept gives on the z-scored pair (np.std, ddof 0).  They are closed forms, not a
 * statsmodels run.  A row is NOT TESTED when its entries over M are all equal (min == max) or any of them is not finite; such rows
 * are counted in `skipped`, never in `n_tests`.  Per phenotype: n_tests = the tested rows paired with it; best = the tested row with
 * the largest r^2 (float64 compare of r * r; a tie goes to the lowest row); p_bonf = p * n_tests, not clipped; q = Benjamini-Hochberg
 * over the p_bonf of the phenotypes that have tests, clipped at 1.  (The script's Bonferroni count includes the pairs it skips.)
 *
 * Pairs.  Without a pair list every phenotype is tested against every row: allowed for P <= DBTK_ASSOC_ALL_PAIRS_MAX.  With a pair
 * list (CSR over the loci: off[ntr + 1], pheno_idx[]) every row of a locus is tested against that locus' phenotypes; rows past
 * nk_cum[ntr - 1] belong to no locus and are not tested.
 *
 * Determinism.  The same inputs give the same bytes on every run: no floating-point atomic is used, the order of every sum depends
 * on n alone, and the hit list is sorted by (phenotype, row).  The samples of M are taken in ascending order whatever the order of
 * sample_of.
 *
 * All entry points return dbtk_status_t (dbtk.h); dbtk_last_error() holds the message.  No CPU path: DBTK_ERR_NO_DEVICE without a HIP
 * device, except dbtk_assoc_pvalue, dbtk_assoc_bh and dbtk_assoc_r2_threshold, which need none.  A handle belongs to one thread at a
 * time.  This header has a version of its own: DBTK_ABI_VERSION (dbtk.h) did not move when it was added.
 */
#ifndef DBTK_ASSOC_H_
#define DBTK_ASSOC_H_

#include <stdint.h>

#include "dbtk.h"
#include "dbtk_pred.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBTK_ASSOC_API_VERSION 1u
uint32_t dbtk_assoc_api_version(void);

#define DBTK_ASSOC_ALL_PAIRS_MAX 64u
#define DBTK_ASSOC_NONE 0xFFFFFFFFu /* row / locus of a phenotype without tests; locus of a row that belongs to none */

typedef struct dbtk_assoc dbtk_assoc_t;

typedef struct dbtk_assoc_best {
    uint64_t n_tests, skipped;
    uint32_t row, locus;
    double r, se, t, p, p_bonf, q; /* 0 where n_tests == 0 */
} dbtk_assoc_best_t;

typedef struct dbtk_assoc_hit {
    uint32_t pheno, locus, row, pad;
    double r, t, p;
} dbtk_assoc_hit_t;

/* pheno[p * n + j] is the value of phenotype p in sample sample_of[j]; names[P] may be NULL (then "p0", "p1", ...).  The values are
 * checked here and sent to the device, where they are centred in the kernel's own summation order (so that a row that equals a
 * phenotype gives r = 1 exactly).  DBTK_ERR_ARG: n < 3, P == 0, a sample_of entry >= ns or given twice, a value that is not finite,
 * a phenotype that is constant over M (the message names it).  DBTK_ERR_NOMEM with the sizes when the tables do not fit.  The
 * hit buffer holds DBTK_ASSOC_HITS entries (environment, a power of two, default 2^20). */
dbtk_status_t dbtk_assoc_create(int device_id, uint64_t ns, uint64_t P, uint64_t n, const uint64_t* sample_of, const double* pheno, const char* const* names,
                                dbtk_assoc_t** out);
void dbtk_assoc_free(dbtk_assoc_t* h);

/* The pair list, copied.  A phenotype listed twice for a locus counts once.  ntr == 0 removes the list.  DBTK_ERR_ARG: an index >= P,
 * off[0] != 0, an off that decreases. */
dbtk_status_t dbtk_assoc_set_pairs(dbtk_assoc_t* h, uint64_t ntr, const uint64_t* off, const uint32_t* pheno_idx);

/* p_threshold: pairs with p <= p_threshold enter the hit list; negative: no hit list.
 * _device: d_rows is float32 [nrows][ns] on the handle's device, complete before the call; nk_cum[ntr] are the loci's cumulative row
 *   counts in HOST memory (needed with a pair list, otherwise optional: NULL leaves every locus DBTK_ASSOC_NONE).  DBTK_ERR_ARG: a
 *   pair list of another ntr, nk_cum that decreases or passes nrows, P > DBTK_ASSOC_ALL_PAIRS_MAX without a pair list.
 *   DBTK_ERR_OVERFLOW: more hits than the buffer holds; the message names DBTK_ASSOC_HITS and the number needed, and no list is kept
 *   (dbtk_assoc_best is complete all the same).
 * _pred: the k-mers of a whole-matrix dbtk_pred_t as it stands: raw before dbtk_pred_correct, corrected after.  DBTK_ERR_ARG: a
 *   windowed handle (a window holds a part of the rows), another device, another ns.
 * _dosage: the rows are loci, the values those of dbtk_dosage_values, locus l's group is l.  DBTK_ERR_ARG on an unfinished handle. */
dbtk_status_t dbtk_assoc_scan_device(dbtk_assoc_t* h, const float* d_rows, uint64_t nrows, uint64_t ntr, const uint32_t* nk_cum, double p_threshold);
dbtk_status_t dbtk_assoc_scan_pred(dbtk_assoc_t* h, dbtk_pred_t* pred, double p_threshold);
dbtk_status_t dbtk_assoc_scan_dosage(dbtk_assoc_t* h, dbtk_dosage_t* dosage, double p_threshold);

/* Of the scan made last (DBTK_ERR_ARG when there is none): out[P]; the hits sorted by (phenotype, row), *n their number, at most cap
 * of them copied (out may be NULL with cap 0). */
dbtk_status_t dbtk_assoc_best(dbtk_assoc_t* h, dbtk_assoc_best_t* out);
dbtk_status_t dbtk_assoc_hits(dbtk_assoc_t* h, dbtk_assoc_hit_t* out, uint64_t cap, uint64_t* n);

/* PREFIX.assoc.best.tsv: `pheno n_tests skipped locus row r se t p p_bonf q` (tab-separated) and one line per phenotype in table
 * order, doubles as %.6e, NA from `locus` on for a phenotype without tests (and for the locus of a row that belongs to none).
 * PREFIX.assoc.hits.tsv, only when the scan had a threshold: `pheno locus row r t p`, sorted. */
dbtk_status_t dbtk_assoc_write(dbtk_assoc_t* h, const char* out_prefix);
/* Of the scan made last: ms[0] milliseconds in k_assoc_scan (HIP events), ms[1] in the host fold. */
dbtk_status_t dbtk_assoc_times(dbtk_assoc_t* h, double ms[2]);

/* Host only, no device. */
dbtk_status_t dbtk_assoc_pvalue(double r, uint64_t n, double* p);               /* DBTK_ERR_ARG: n < 3, |r| > 1 or NaN */
dbtk_status_t dbtk_assoc_bh(const double* p, uint64_t m, double* q);
dbtk_status_t dbtk_assoc_r2_threshold(double p_threshold, uint64_t n, double* r2); /* the kernel's filter: r * r >= *r2 */

#ifdef __cplusplus
}
#endif
#endif
