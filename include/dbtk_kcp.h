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

#ifdef __cplusplus
}
#endif
#endif
