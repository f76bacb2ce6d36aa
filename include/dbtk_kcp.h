/* dbtk_kcp.h — C-ABI of the bait k-mer count profiles (`danbing-tk --bait-profile`), on one MI355X.
 *
 * Replaces, in the reference:  src/bait.cpp:75-81, 117-138, 382-412 (`baitBuilder v1.pf`): for every read pair that
 * `danbing-tk -s` assigned to a locus, the canonical k-mers of both mates with their per-read counts, kept per (assigned locus,
 * k-mer) apart for true positives (source locus == assigned locus) and false positives, and written as min / max / mean / sd.
 * The reference keeps a vector of counts per key on the host and reads the pairs back from the gzipped kam text; here the
 * reads go to the device as they are and the table holds five exact integers per key:
 *   n      reads in which the k-mer occurred (a k-mer in both mates of a pair: two observations, as read2kcp is called per mate)
 *   sum    of its per-read count c (1 <= c <= 236)          sumsq  of c * c          min, max  of c
 * The canonical k-mers are those of read2kmers / buildNuKmers (kmer.hpp:95-200): upper-case ACGT only, any other byte resets the
 * window, a read shorter than k contributes nothing.
 *
 * File format (what `baitBuilder v2` and `ktools fps` parse): `>LOCUS` for every locus with an entry, loci ascending, then
 * `KMER\tMIN\tMAX\tMEAN\tSD` with MEAN and SD as %.4f.  MEAN = sum / n; SD = sqrt((n * sumsq - sum^2) / n^2), the numerator exact.
 * Inside a locus the lines ascend by k-mer (the reference's order there is that of a hash map and depends on the order of the reads).
 *
 * All entry points return dbtk_status_t (dbtk.h); dbtk_last_error() holds the message.  No CPU path: dbtk_kcp_create fails with
 * DBTK_ERR_NO_DEVICE without a HIP device.  A handle belongs to one thread at a time; several handles may be alive at once.
 * This header has a version of its own: DBTK_ABI_VERSION (dbtk.h) did not move when it was added.
 */
#ifndef DBTK_KCP_H_
#define DBTK_KCP_H_

#include <stdint.h>

#include "dbtk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBTK_KCP_API_VERSION 1u
uint32_t dbtk_kcp_api_version(void);

#define DBTK_KCP_TP_ONLY 1u /* flags: drop the pairs with src != dst (baitBuilder's -tp) */

typedef struct dbtk_kcp dbtk_kcp_t;

/* DBTK_ERR_ARG: ksize outside 2..31, nloci 0 or above 2^31 - 2, unknown flags, DBTK_KCP_SLOTS in the environment not a power of two
 * from 64 to 2^32.  The table starts with DBTK_KCP_SLOTS slots of 40 bytes (default 2^22) and grows by doubling: before a batch,
 * with `bound` = the sum of max(0, L - k + 1) over the reads it will count, the table is doubled until 2 * (occupied + bound) is
 * no more than its slots, so its load stays at or under 1/2 inside a batch.  (dbtk_kcp_add cuts a large batch into pieces whose
 * bound is at most a quarter of the table, or 2^20 where that is more, so that a table the profile does not need is not made.)
 * DBTK_ERR_NOMEM when a table does not fit. */
dbtk_status_t dbtk_kcp_create(uint32_t ksize, uint64_t nloci, int device_id, uint32_t flags, dbtk_kcp_t** out);
void dbtk_kcp_free(dbtk_kcp_t* kcp);

/* Host buffers in the layout of dbtk_align_batch: read r = seq_bytes[seq_offsets[r], seq_offsets[r + 1]), reads 2p and 2p + 1 are
 * pair p; src[p] / dst[p] = the pair's source and assigned locus.  Pairs with dst >= nloci are skipped; src == dst is a true
 * positive, anything else a false positive (dropped under DBTK_KCP_TP_ONLY).  Returns when the batch is counted.
 * DBTK_ERR_READ_TOO_LONG (nothing counted) when a counted read is longer than DBTK_MAX_READ_LEN.  DBTK_ERR_OVERFLOW when an insert
 * of an earlier call found no slot (the growth rule excludes it; the message names DBTK_KCP_SLOTS): the table then lacks
 * observations until dbtk_kcp_reset. */
dbtk_status_t dbtk_kcp_add(dbtk_kcp_t* kcp, const uint8_t* seq_bytes, const uint64_t* seq_offsets, uint64_t npairs, const uint32_t* src,
                           const uint32_t* dst);

/* The same for a batch that lies in device memory in the layout of dbtk_align_batch_device: d_seq (indexed by the offsets as they
 * are), d_offsets = uint64[2 * npairs + 1], d_src = uint32[npairs], all on the handle's device and complete before the call (the
 * handle's stream is not ordered against the one that made them); dst[npairs] is a host array (>= nloci: skip the pair).  The reads
 * and sources stay in HBM: the offsets and sources (20 bytes per pair) are copied to the host to choose the pairs and bound their
 * keys, the counting kernel is dbtk_kcp_add's.  Returns when the batch is counted.  Added without moving DBTK_KCP_API_VERSION
 * (nothing that existed changed); its presence goes with dbtk_sim.h (DBTK_SIM_API_VERSION 1). */
dbtk_status_t dbtk_kcp_add_device(dbtk_kcp_t* kcp, const void* d_seq, const void* d_offsets, uint64_t npairs, const void* d_src, const uint32_t* dst);

/* cls 0: true positives, 1: false positives.  *n = entries of the class. */
dbtk_status_t dbtk_kcp_count(dbtk_kcp_t* kcp, uint32_t cls, uint64_t* n);
/* The entries of the class sorted by (locus, k-mer) into the arrays (each may be null).  DBTK_ERR_OVERFLOW (nothing copied) when
 * cap is smaller than dbtk_kcp_count. */
dbtk_status_t dbtk_kcp_read(dbtk_kcp_t* kcp, uint32_t cls, uint32_t* loci, uint64_t* kmers, uint32_t* n, uint64_t* sum, uint64_t* sumsq,
                            uint32_t* min, uint32_t* max, uint64_t cap);
/* PREFIX.TP_pf.txt and, unless DBTK_KCP_TP_ONLY, PREFIX.FP_pf.txt. */
dbtk_status_t dbtk_kcp_write(dbtk_kcp_t* kcp, const char* out_prefix);
/* Empties the table (it keeps its size) and clears the sticky word. */
dbtk_status_t dbtk_kcp_reset(dbtk_kcp_t* kcp);

/* Bytes of the table in HBM, its slots and how many are taken. */
dbtk_status_t dbtk_kcp_stats(dbtk_kcp_t* kcp, uint64_t* table_bytes, uint64_t* slots, uint64_t* occupied);
/* Of all dbtk_kcp_add calls since creation or reset: milliseconds in the add kernel (HIP events) and first occurrences inserted. */
dbtk_status_t dbtk_kcp_times(dbtk_kcp_t* kcp, double* add_ms, uint64_t* inserts);

/* Switches the handle's class filter between batches: on != 0 as if created with DBTK_KCP_TP_ONLY (later dbtk_kcp_add calls drop
 * the pairs with src != dst, dbtk_kcp_write writes no FP file), 0 counts both classes again.  What the table holds stays.  One
 * handle whose filter moves, rather than a second TP-only handle beside the first: a second handle is a second table in HBM, and
 * a run that counts genome after genome (`--bait-fps --genome`) needs one table at a time. */
dbtk_status_t dbtk_kcp_set_tp_only(dbtk_kcp_t* kcp, int on);

/* ---- The FP-specific bait k-mers (`danbing-tk --bait-fps`), filtered on the device.
 * Replaces, in the reference:  src/bait.cpp:177-241, 254-305 (`baitBuilder v2`, here also `ktools fps`), which parse one FP profile
 * and one TP profile per genome from text.  Here the FP entries of a table become a list of candidates in HBM, and every TP table
 * is looked up where it lies: no profile text is written or parsed.  The comparison is the reference's, on the floats that strtof
 * makes of the "%.4f" text of MEAN and SD; the device computes those floats from an entry's five integers, bit for bit
 * (csrc/dbtk_kcp.h: kcp_mean_text, kcp_sd_text).
 *
 * A candidate: k-mer, locus, the FP mean as float, (mi, ma) = (255, 0), alive.  dbtk_kcp_fps_apply looks every living candidate up
 * as (k-mer, locus, class 0) in one table: absent — nothing; present and tp_mean - 2 sd <= fp_mean <= tp_mean + 2 sd — the
 * candidate dies for good; present and outside — (mi, ma) becomes the entry's (min, max) where mi is still 255, else widens by it.
 * The result of several applies does not depend on their order. */
typedef struct dbtk_kcp_fps dbtk_kcp_fps_t;

/* The FP class of kcp's table becomes the candidate list (DBTK_ERR_ARG for a handle that is DBTK_KCP_TP_ONLY).  The list lives on its
 * own: kcp may be reset or freed afterwards. */
dbtk_status_t dbtk_kcp_fps_begin(dbtk_kcp_t* kcp, dbtk_kcp_fps_t** out);
/* kcp_tp: the handle the list was begun from or any other on the same device with the same ksize and nloci (else DBTK_ERR_ARG).
 * Its table is only read.  Returns when the kernel is done. */
dbtk_status_t dbtk_kcp_fps_apply(dbtk_kcp_fps_t* fps, dbtk_kcp_t* kcp_tp);
dbtk_status_t dbtk_kcp_fps_count(dbtk_kcp_fps_t* fps, uint64_t* candidates, uint64_t* alive);
/* The living candidates sorted by (locus, k-mer) into the arrays (each may be null).  DBTK_ERR_OVERFLOW when cap is too small. */
dbtk_status_t dbtk_kcp_fps_read(dbtk_kcp_fps_t* fps, uint32_t* loci, uint64_t* kmers, uint8_t* mi, uint8_t* ma, uint64_t cap);
/* The file `ktools fps` writes, byte for byte: `>LOCUS` for every locus that had a candidate (also when all of them died), loci
 * ascending, then `KMER\tMI\tMA` ascending by k-mer. */
dbtk_status_t dbtk_kcp_fps_write(dbtk_kcp_fps_t* fps, const char* path);
/* Of all applies: milliseconds in k_kcp_fps_apply (HIP events) and living candidates looked up. */
dbtk_status_t dbtk_kcp_fps_times(dbtk_kcp_fps_t* fps, double* apply_ms, uint64_t* lookups);
void dbtk_kcp_fps_free(dbtk_kcp_fps_t* fps);

/* kcp_mean_text / kcp_sd_text evaluated on the device over host arrays of moments (n[i] >= 1, n[i] * sumsq[i] >= sum[i]^2, else
 * DBTK_ERR_ARG): the floats `ktools fps` would parse from a profile line of such an entry.  For tests and bindings: moments like
 * these cannot all be produced by adding reads. */
dbtk_status_t dbtk_kcp_text_stats(int device_id, const uint32_t* n, const uint64_t* sum, const uint64_t* sumsq, uint64_t count, float* mean_out, float* sd_out);
/* (All of the above were added without moving DBTK_KCP_API_VERSION: nothing that existed changed.) */

#ifdef __cplusplus
}
#endif
#endif
