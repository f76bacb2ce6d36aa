/* dbtk_pred.h — C-ABI of the `danbing-tk-pred` step: read-depth normalisation and invariant-k-mer
 * bias correction of a cohort's OUT.trkmc.ar count vectors, on one MI355X.
 *
 * Replaces, in /root/reference:  src/pred.cpp:52-82 (main's compute part) and src/pred.h:166-233
 *   load_eachBinGT  pred.h:166-186   counts (u64, one file per sample) -> float matrix
 *   norm_rd         pred.h:204-209   gt(sample, kmer) = count / read depth of the sample
 *   bias_correction pred.h:212-233   per locus: bias(sample) = mean_j gt(sample, ikmer_j) / ikmc_j, divided by its mean
 *                                    over the samples; the locus' k-mer columns are divided by it; Bias(sample, locus) kept
 *   save_matrix     pred.h:236-258   layouts of the three outputs
 *
 * Arithmetic: IEEE float32, as the reference's Eigen::ArrayXXf.  The raw matrix (one conversion and one division per entry)
 * is bit-exact; the sums of a bias are taken in k-mer order per sample (Eigen's scalar order); the mean over the samples is
 * a pairwise tree here and a packet reduction in Eigen, so the corrected matrix and Bias agree to float32 rounding
 * (tests: relative 2e-6), not bit for bit.  PARITY UNPINNED: the reference's pred.cpp needs Eigen, which this image
 * lacks (.gitmodules: the submodule directory is empty), so the oracle (oracle/pred_oracle.py) restates pred.h and could
 * not be checked against a run of the reference.
 *
 * All entry points return dbtk_status_t (dbtk.h); dbtk_last_error() holds the message.  No CPU path: dbtk_pred_create
 * fails with DBTK_ERR_NO_DEVICE without a HIP device.
 */
#ifndef DBTK_PRED_H_
#define DBTK_PRED_H_

#include <stdint.h>

#include "dbtk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dbtk_pred dbtk_pred_t;

/* The invariant-k-mer metadata of an RPGG build (read_ikmer, pred.h:64-126: `ikmer.meta`): per locus the CUMULATIVE number
 * of k-mers (nk_cum[ntr], nk_cum[ntr-1] == nk) and of invariant k-mers (nik_cum[ntr], nik_cum[ntr-1] == nik); per invariant
 * k-mer its column (iki[nik] < nk) and its expected count (ikmc[nik]).  The matrix G[nk][ns] (float32, 4*nk*ns bytes) lives
 * in HBM.  DBTK_ERR_NOMEM (ABI v9; DBTK_ERR_HIP before) when the matrix does not fit into the device's free HBM: the message
 * holds its size and the free and total bytes of the device; every other failed HIP call stays DBTK_ERR_HIP. */
dbtk_status_t dbtk_pred_create(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                               uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, dbtk_pred_t** out);
void dbtk_pred_free(dbtk_pred_t* p);

/* Reads `ikmer.meta` (little endian: u64 nk, u64 nik, u64 ntr, u32 nk_cum[ntr], u32 nik_cum[ntr], nik x {u32 ki, u8 kc}) and
 * creates the handle for ns samples. */
dbtk_status_t dbtk_pred_create_from_file(int device_id, uint64_t ns, const char* ikmer_meta, dbtk_pred_t** out);
uint64_t dbtk_pred_nk(const dbtk_pred_t* p);
uint64_t dbtk_pred_ntr(const dbtk_pred_t* p);

/* Samples first_sample .. first_sample + n - 1: counts[i * nk + k] = count of k-mer k in sample i (the body of its
 * OUT.trkmc.ar), read_depth[i] its depth.  load_eachBinGT + norm_rd for these columns: G[k][s] = (float)count / depth. */
dbtk_status_t dbtk_pred_load_samples(dbtk_pred_t* p, uint64_t first_sample, uint64_t n, const uint64_t* counts, const float* read_depth);

/* The same for counts that are already in DEVICE memory of the handle's device (ABI v9): d_counts[i * nk + k], sample-major like
 * the host form; read_depth[n] is HOST memory.  Bit-identical to dbtk_pred_load_samples fed the same counts.  Samples may be
 * loaded in any order and a column may be loaded again (the later load wins).  n == 1 takes the column kernel (nk 4-byte stores
 * at a stride of 4 * ns bytes), n > 1 the LDS-turned tiles of dbtk_pred_load_samples; nothing is staged inside the handle, so
 * dbtk_pred_correct / _matrix / _bias always see every load that has returned.
 * Stream ordering: the kernel runs on the handle's own stream, which is NOT ordered against the stream that produced d_counts:
 * the counts must be complete before the call.  The call returns when d_counts is no longer being read. */
dbtk_status_t dbtk_pred_load_device(dbtk_pred_t* p, uint64_t first_sample, uint64_t n, const uint64_t* d_counts, const float* read_depth);
/* Column `sample` of G from the context's accumulated counts — what dbtk_ctx_counts would copy to the host, in OUT.trkmc.ar
 * order — divided by read_depth, without the counts leaving HBM.  Goes through dbtk_ctx_synchronize and dbtk_ctx_accum_buffer:
 * every batch launched on the context is waited for; a pending sticky error word (DBTK_ERR_READ_TOO_LONG, ...) is returned, once,
 * INSTEAD of loading the tainted counts.  DBTK_ERR_ARG when the context's ntrkmers differs from the handle's nk, when the two are
 * on different devices, when sample >= ns — and when pairs appended by dbtk_ingest_align_merged have not been aligned yet: the
 * call REFUSES rather than flushes them (the flush belongs to the ingest that holds the blocks; dbtk_ctx_synchronize does not
 * see those pairs): call dbtk_ingest_align_merged(ing, ~0u, ctx, 0, 1) first.  The column is not touched by a refused call.
 * Returns when the context's accumulators are no longer being read: a dbtk_ctx_reset right after it is safe.  Like every call
 * on a context, it must come from the one thread that owns the context at the time. */
dbtk_status_t dbtk_pred_load_ctx(dbtk_pred_t* p, uint64_t sample, dbtk_ctx_t* ctx, float read_depth);

/* bias_correction (pred.h:212-233) on the loaded matrix, in place; fills the bias matrix.  A locus without k-mers or
 * without invariant k-mers is left alone (the reference `continue`s and leaves its Bias column uninitialised: 0 here). */
dbtk_status_t dbtk_pred_correct(dbtk_pred_t* p);

/* The matrix as save_matrix lays it out (pred.h:236-249): ns x nk, column-major = nk runs of ns floats (before
 * dbtk_pred_correct: the raw genotype matrix, after: the corrected one).  out holds ns * nk floats. */
dbtk_status_t dbtk_pred_matrix(dbtk_pred_t* p, float* out);
/* Bias, ns x ntr column-major (Bias(s, tri) at tri * ns + s). */
dbtk_status_t dbtk_pred_bias(dbtk_pred_t* p, float* out);

/* Kernel times of the last dbtk_pred_correct in milliseconds: bias sums, bias normalisation, the correcting pass. */
dbtk_status_t dbtk_pred_times(dbtk_pred_t* p, float ms[3]);

/* ---- Windows: matrices larger than HBM or the host (added within ABI v11; the version number did not move).
 *
 * bias_correction is independent per locus: the bias of a locus reads that locus' invariant k-mers and divides that locus' columns.
 * A windowed handle therefore holds a run of whole loci at a time — at most max_rows k-mer columns — and makes the same bits as the
 * whole-matrix handle, window after window.  save_matrix writes nk runs of ns floats, so a window is one contiguous piece of each
 * output file.
 *
 * dbtk_pred_create_windowed is dbtk_pred_create with G[max_rows][ns] instead of G[nk][ns] (max_rows above nk is taken as nk); Bias
 * [ntr][ns] and the metadata stay whole.  Beside G the handle holds two buffers of staged counts (8 * max_rows * ns bytes each) and
 * one pair of output windows (2 * 4 * max_rows * ns), 28 * max_rows * ns bytes of HBM in all, and pinned host memory for one pair of
 * output windows and PW = 4 samples' counts: (8 * ns + 32) * max_rows bytes.  Everything is sized by this call and never again.
 * DBTK_ERR_ARG when a locus has more than max_rows k-mers (the message names the locus and its size) or max_rows is 0;
 * DBTK_ERR_FORMAT when an invariant k-mer lies outside its locus (no ikmer.meta has that; a window could not hold what the bias
 * reads); DBTK_ERR_NOMEM as dbtk_pred_create.  K-mers past nk_cum[ntr - 1] (they belong to no locus) travel with the last locus.
 * The new handle's current window is the one that starts at locus 0. */
dbtk_status_t dbtk_pred_create_windowed(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                                        uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, uint64_t max_rows, dbtk_pred_t** out);
dbtk_status_t dbtk_pred_create_windowed_from_file(int device_id, uint64_t ns, const char* ikmer_meta, uint64_t max_rows, dbtk_pred_t** out);
/* max_rows of a windowed handle as it was taken; 0 for a handle of dbtk_pred_create. */
uint64_t dbtk_pred_max_rows(const dbtk_pred_t* p);

/* The current window becomes the longest run of loci [first_locus, *end_locus) whose k-mers fit into max_rows.  Loci without k-mers
 * cost nothing; a run of them at the end of the window belongs to it.  *first_row = the window's first k-mer column, *rows = their
 * number (0: only empty loci).  The window's part of G, its staged counts and its depths (1.0) are reset: a sample that is not
 * loaded into the window reads as all-zero counts, like the zeroed column of a new whole-matrix handle.  Bias rows of other windows
 * are kept.  The window takes the buffer that holds no submitted window (dbtk_pred_window_submit), so the loads of window w + 1 run
 * beside the kernels and the copies of window w.  DBTK_ERR_ARG for first_locus >= ntr and for a handle of dbtk_pred_create.
 *
 * On a windowed handle
 *   dbtk_pred_load_samples / _load_device  take the window's counts only: counts[i * rows + r] = count of k-mer first_row + r in sample
 *                            first_sample + i.  A refused call leaves the window unchanged; any order of samples; loaded twice: the later
 *                            load wins.  The counts are staged in HBM (the fused pass needs all samples of a window at once).
 *   dbtk_pred_load_ctx       is refused (DBTK_ERR_ARG): a context holds one sample's whole vector.
 *   dbtk_pred_matrix         returns ns x rows floats, the save_matrix layout of the window's rows.
 *   dbtk_pred_correct        corrects the window's loci in G and fills their Bias rows.
 *   dbtk_pred_bias           returns the whole ns x ntr table; loci that no window has visited are 0.
 * These separate calls give the same bits as the fused pass below; they make G from the staged counts when first asked. */
dbtk_status_t dbtk_pred_window(dbtk_pred_t* p, uint64_t first_locus, uint64_t* end_locus, uint64_t* first_row, uint64_t* rows);

/* The fused pass over the current window: the raw bias sums straight from the staged counts, the normalisation kernel of
 * dbtk_pred_correct, then ONE kernel that reads the counts once and writes the window of the raw matrix and the window of the
 * corrected matrix; G is neither written nor read.  Fills the window's Bias rows.
 * dbtk_pred_window_submit starts it on the window's stream, the copies to pinned host memory included, and returns at once: the next
 * dbtk_pred_window and its loads may follow while it runs.  One window can be submitted at a time (DBTK_ERR_ARG otherwise).
 * dbtk_pred_window_outputs waits for the submitted window — or, when none is, submits the current one — and copies its outputs:
 * rows * ns floats each, in the layout of dbtk_pred_matrix (either pointer may be NULL).  dbtk_pred_window_outputs_pinned hands out the
 * pinned buffers themselves instead (valid until the next submit), with the window's rows. */
dbtk_status_t dbtk_pred_window_submit(dbtk_pred_t* p);
dbtk_status_t dbtk_pred_window_outputs(dbtk_pred_t* p, float* raw_out, float* corrected_out);
dbtk_status_t dbtk_pred_window_outputs_pinned(dbtk_pred_t* p, const float** raw, const float** corrected, uint64_t* rows);
/* The handle's pinned staging buffer: room for *cap_samples samples' counts of a window.  Counts that dbtk_pred_load_samples is given
 * at this address are sent as they lie (no copy through the staging buffer). */
dbtk_status_t dbtk_pred_window_stage(dbtk_pred_t* p, uint64_t** buf, uint64_t* cap_samples);

/* ---- Per-locus dosage tables without the matrix (ABI v10).
 *
 * What most users take from the matrix is one number per sample and locus: "the sum of k-mer counts normalised to VNTR dosage"
 * (the reference's README; the `.kms` table of `ktools sum`, read by script/kmc2length.py).  A dbtk_dosage_t holds exactly that for
 * ns samples and ntr loci, in HBM:
 *   kms   u64 [ntr][ns]   the exact sum of the locus' counts (what `ktools sum` writes)
 *   raw   f32 [ntr][ns]   the raw bias of bias_correction's first half: sum_j ((float)count[iki[j]] / depth) / ikmc[j], in j order, / n
 *   Bias  f32 [ntr][ns]   raw divided by its mean over the samples (dbtk_dosage_finish)
 * plus a buffer of that size for dbtk_dosage_values, the depths, the invariant-k-mer tables and a work list of a few bytes per
 * locus: 20 * ntr * ns bytes and nothing of size
 * nk * ns, so the cohort's size is not bounded by the matrix.  DBTK_ERR_NOMEM when the tables do not fit; the message holds their
 * size and the free and total bytes of the device.
 *
 * Arithmetic.  kms is integer and exact.  raw takes the operations of the matrix path one by one — (float)count / depth (the
 * column loaders), / ikmc[j], the adds sequential in j, / (float)n (the bias sums) — and dbtk_dosage_finish runs the matrix path's
 * own normalisation kernel, so dbtk_dosage_bias is BIT-IDENTICAL to dbtk_pred_bias after dbtk_pred_correct on the same counts and
 * depths.  values(s, l) = v = (float)kms / depth (one conversion, one division); where the locus has k-mers and invariant k-mers
 * v / Bias(s, l), otherwise v stays uncorrected (as bias_correction leaves such a locus' columns); 0 for a locus without k-mers.
 * A Bias of exactly 0 (every invariant k-mer of the locus uncounted in that sample) gives what IEEE division gives: +inf, or NaN
 * for 0 / 0.  The reference has the same caveat one step earlier: it divides the k-mer columns by biases near zero without a guard.
 * A sample that was never loaded reads as all-zero counts at depth 1, like the zeroed column of the matrix handle. */
typedef struct dbtk_dosage dbtk_dosage_t;

/* The metadata arguments of dbtk_pred_create, with the same checks. */
dbtk_status_t dbtk_dosage_create(int device_id, uint64_t ns, uint64_t nk, uint64_t ntr, const uint32_t* nk_cum, const uint32_t* nik_cum,
                                 uint64_t nik, const uint32_t* iki, const uint8_t* ikmc, dbtk_dosage_t** out);
dbtk_status_t dbtk_dosage_create_from_file(int device_id, uint64_t ns, const char* ikmer_meta, dbtk_dosage_t** out);
/* Locus boundaries from a loaded RPGG (its OUT.trkmc.ar order), no invariant k-mers: every locus counts as "skipped", so kms is
 * complete, Bias is 0 and values is kms / depth.  What `danbing-tk --cohort --kms` uses: it needs no ikmer.meta and no depths. */
dbtk_status_t dbtk_dosage_create_from_rpgg(const dbtk_rpgg_t* rpgg, int device_id, uint64_t ns, dbtk_dosage_t** out);
void dbtk_dosage_free(dbtk_dosage_t* d);
uint64_t dbtk_dosage_nk(const dbtk_dosage_t* d);
uint64_t dbtk_dosage_ntr(const dbtk_dosage_t* d);
/* Bytes of HBM the handle holds (tables, metadata, work list; the staging of dbtk_dosage_load_samples once it was used). */
uint64_t dbtk_dosage_bytes(const dbtk_dosage_t* d);

/* The three loaders keep the contracts of their dbtk_pred_load_* twins above, word for word: the refusals (DBTK_ERR_ARG for another
 * nk, another device, sample >= ns, pairs of dbtk_ingest_align_merged not flushed; a pending sticky error word returned once INSTEAD
 * of loading), "the tables are not touched by a refused call", the handle's own stream that is not ordered against the producer of
 * d_counts, the return once the counts are no longer read, any order of samples, and "loaded twice: the later load wins".
 * One kernel pass over a sample's 8 * nk bytes of counts makes its kms and raw entries; dbtk_dosage_load_samples stages the host
 * counts 16 samples at a time. */
dbtk_status_t dbtk_dosage_load_ctx(dbtk_dosage_t* d, uint64_t sample, dbtk_ctx_t* ctx, float read_depth);
dbtk_status_t dbtk_dosage_load_device(dbtk_dosage_t* d, uint64_t first_sample, uint64_t n, const uint64_t* d_counts, const float* read_depth);
dbtk_status_t dbtk_dosage_load_samples(dbtk_dosage_t* d, uint64_t first_sample, uint64_t n, const uint64_t* counts, const float* read_depth);

/* Bias = raw normalised over the samples (raw itself is kept: the call may be repeated, and samples may be loaded after it; a load
 * makes the handle "unfinished" again).  dbtk_dosage_bias and dbtk_dosage_values return DBTK_ERR_ARG on an unfinished handle. */
dbtk_status_t dbtk_dosage_finish(dbtk_dosage_t* d);
/* ns x ntr column-major, the layout of dbtk_pred_bias: entry (s, tri) at tri * ns + s. */
dbtk_status_t dbtk_dosage_kms(dbtk_dosage_t* d, uint64_t* out);
dbtk_status_t dbtk_dosage_bias(dbtk_dosage_t* d, float* out);
dbtk_status_t dbtk_dosage_values(dbtk_dosage_t* d, float* out);
/* Kernel times in milliseconds: ms[0] the kernels of the last load call (all of its samples), ms[1] the last dbtk_dosage_finish. */
dbtk_status_t dbtk_dosage_times(dbtk_dosage_t* d, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
