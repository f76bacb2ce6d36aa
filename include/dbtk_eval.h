/* dbtk_eval.h — C-ABI of the genotype score (`danbing-tk --eval PREFIX`), on one MI355X.
 *
 * Replaces, in the reference's pipelines (rules EvalRawGenomeGraph and EvalGenotypeQuality): cutting a per-locus FASTA out of the
 * assembly, `fa2kmers -tr` over it, OUT.tr.kmers as text, and script/kmers.linreg.py, which regresses per locus the k-mer counts
 * taken from reads (y) on the k-mer counts of the genome's own assembly (x, the TRUTH) and reports slope, r^2 and predicted dosage.
 *
 * Truth.  For an RPGG with k-mer size k and an assembly with BED lines CTG <TAB> START <TAB> END <TAB> LOCUS (dbtk_sim.h), the truth
 * count of TR k-mer K of locus L is the number of positions p such that some BED line of L on a kept contig has
 * START <= p and p + k <= min(END, contig size), the k bases at p are all of ACGTacgt, and the canonical k-mer of their upper-cased
 * form is K.  Summed over all lines of L (several lines may name one locus, lines of different loci may overlap) and over every
 * assembly added.  windows[L] counts those positions whatever their k-mer is (a flank k-mer, a TR k-mer of another locus only, a
 * k-mer in no table).  That is what `fa2kmers -tr -fsi F` counts over the records ctg[START - F, END + F).  The (locus, k-mer)
 * look-up is the aligner's class table.  There a k-mer that is in the flank set AND the TR set of one locus is a flank k-mer (flank
 * beats TR, as in assignTRkmc: reads never count it, its y is 0 as in the reference's own files); the truth counts it all the same,
 * through a small table of those k-mers that the handle makes for itself.
 *
 * Sums.  Per locus, over its TR k-mers in OUT.trkmc.ar order, with x = truth and y = a count vector, eight exact integers:
 *   n1 = #{x > 0}   Sx = sum x   Sy = sum y   Sy1 = sum of y where x > 0   Sxy = sum x y   Sxx = sum x^2   Syy = sum y^2
 *   Syy1 = sum of y^2 where x > 0
 * A product or sum that does not fit 64 bits is detected, never wrapped: DBTK_ERR_OVERFLOW, the message names the locus.
 *
 * Columns.  Made on the host in double from the integers, by these formulas and no others:
 *   slope = (double)Sxy / (double)Sxx        pred = (double)Sy / slope        r2 = ((double)Sxy * (double)Sxy) / ((double)Sxx * (double)Syy)
 *   pred_present, r2_present: the same with Sy1 and Syy1 (the script's --mapkmer mode).  Where Sxy == 0 all five are 0.
 * These are the closed forms of an ordinary least squares fit without intercept and of its uncentred r^2, which is what
 * sm.OLS(y, x).fit() reports; they are not a statsmodels run, and agreement to the last printed digit is not claimed.  (With
 * Sxy == 0 the script's answer depends on statsmodels' pseudo-inverse; 0 is this project's rule.)
 *
 * All entry points return dbtk_status_t (dbtk.h); dbtk_last_error() holds the message.  Every argument is checked before a device
 * is asked for.  No CPU path: DBTK_ERR_NO_DEVICE without a HIP device (dbtk_eval_columns needs none).  A handle belongs to one
 * thread at a time.  This header has a version of its own: DBTK_ABI_VERSION (dbtk.h) did not move when it was added.
 */
#ifndef DBTK_EVAL_H_
#define DBTK_EVAL_H_

#include <stdint.h>

#include "dbtk.h"
#include "dbtk_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBTK_EVAL_API_VERSION 1u
uint32_t dbtk_eval_api_version(void);

typedef struct dbtk_eval dbtk_eval_t;

/* nk = TR k-mers of the locus; windows as above (after dbtk_eval_truth_set without windows: Sx); then the eight sums */
typedef struct dbtk_eval_sums {
    uint64_t nk, windows, n1, Sx, Sy, Sy1, Sxy, Sxx, Syy, Syy1;
} dbtk_eval_sums_t;

typedef struct dbtk_eval_cols {
    double slope, pred, r2, pred_present, r2_present;
} dbtk_eval_cols_t;

/* The handle holds truth[ntrkmers] and windows[nloci] in HBM, zeroed, and shares the class table of (rpgg, device) with the
 * contexts of that pair (the first of them to come builds it).  DBTK_ERR_ARG: a handle loaded with DBTK_LOAD_INDEX_ONLY (it has no
 * output order), device_id out of range.  The RPGG handle must outlive the evaluator. */
dbtk_status_t dbtk_eval_create(const dbtk_rpgg_t* rpgg, int device_id, dbtk_eval_t** out);
void dbtk_eval_free(dbtk_eval_t* e);

/* Adds the truth counts and windows of an attached sim handle's assembly (k_eval_truth).  A pass of its own over the assembly, on
 * the sim handle's stream and in its arena: group after group of contigs, a group that is resident already is not uploaded again.
 * The counts do not depend on DBTK_SIM_ARENA_BYTES.  Returns when they are added.  DBTK_ERR_ARG: a sim handle that is not attached,
 * that is on another device, or that was opened for another number of loci. */
dbtk_status_t dbtk_eval_truth_sim(dbtk_eval_t* e, dbtk_sim_t* sim);
/* Sets the truth from the host: counts[ntrkmers] in OUT.trkmc.ar order, windows[nloci] or NULL (then windows[L] = Sx of L). */
dbtk_status_t dbtk_eval_truth_set(dbtk_eval_t* e, const uint64_t* counts, const uint64_t* windows);
/* Reads them back in the same order; each may be null. */
dbtk_status_t dbtk_eval_truth(dbtk_eval_t* e, uint64_t* counts, uint64_t* windows);
dbtk_status_t dbtk_eval_truth_reset(dbtk_eval_t* e);

/* Scores a count vector against the truth (k_eval_sums) and keeps the sums in the handle.  _ctx: the accumulators of a context of
 * the same RPGG build and device; a context with pairs appended by dbtk_ingest_align_merged and not yet aligned is refused
 * (DBTK_ERR_ARG), as dbtk_pred_load_ctx refuses it.  _device: any uint64[ntrkmers] on the handle's device, complete before the call.
 * _host: the same from host memory.  DBTK_ERR_OVERFLOW (no sums kept): see above. */
dbtk_status_t dbtk_eval_score_ctx(dbtk_eval_t* e, dbtk_ctx_t* ctx);
dbtk_status_t dbtk_eval_score_device(dbtk_eval_t* e, const void* d_counts);
dbtk_status_t dbtk_eval_score_host(dbtk_eval_t* e, const uint64_t* counts);
/* out[nloci] of the score made last (DBTK_ERR_ARG when there is none). */
dbtk_status_t dbtk_eval_sums(dbtk_eval_t* e, dbtk_eval_sums_t* out);
/* The derived columns of n loci; needs no handle and no device. */
dbtk_status_t dbtk_eval_columns(const dbtk_eval_sums_t* sums, uint64_t n, dbtk_eval_cols_t* out);

/* PREFIX.eval.tsv: the line
 *   #locus nk nk_present windows Sx Sy Sy_present Sxy Sxx Syy Syy_present slope pred r2 pred_present r2_present
 * (tab-separated) and one row per locus: the integers as decimals, slope %.2f, the two pred %.1f, the two r2 %.4f.
 * PREFIX.pred: what kmers.linreg.py --mapkmer writes: "# TrueDosage\tPredDosage\tSlope\tr^2", then per locus
 * windows, pred_present, slope, r2_present as %i\t%.1f\t%.2f\t%.4f (the script's TrueDosage is the sum over all k-mers of the
 * assembly's TR region: windows, not Sx). */
dbtk_status_t dbtk_eval_write(dbtk_eval_t* e, const char* out_prefix);
/* Of all calls since creation: ms[0] milliseconds in k_eval_truth, ms[1] in k_eval_sums (HIP events), and the class-table
 * look-ups of k_eval_truth (one per window). */
dbtk_status_t dbtk_eval_times(dbtk_eval_t* e, double ms[2], uint64_t* lookups);

#ifdef __cplusplus
}
#endif
#endif
