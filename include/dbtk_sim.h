/* dbtk_sim.h — C-ABI of the simulated read source (`danbing-tk --sim ASSEMBLY BED`), on one MI355X.
 *
 * Replaces, in the reference's mismap-QC workflow (test/QC/fn1a.sim.sh -> fn1b.annot.sh -> fn1c.extract.sh -> fn2a1.raw.map.sh):
 * `sim_reads -pe -no-err` (src/sim_reads.cpp:225-231), `bedtools map ... -o distinct_sort_num`, the `-e 1` pre-filter and the two gzip
 * round trips.  Every byte of that FASTA is a function of (contig, offset): the assembly goes to HBM once and a kernel tiles it into
 * the batch layout of dbtk_align_batch_device, with the source locus of every pair beside it.
 *
 * Only the deterministic mode of sim_reads: paired ends, no errors, no -uni.  With SHFT = 2 * RLEN / cv and NBEG = FLEN - RLEN, a
 * contig of `size` bases (the sequence lines of a FASTA record concatenated; a record shorter than ML is skipped) gives the fragments
 * beg = 0, SHFT, 2 SHFT, ... while beg + FLEN <= size: nfrag(size) = size < FLEN ? 0 : (size - FLEN) / SHFT + 1.  Fragments are
 * numbered through the kept contigs in file order.  Fragment f = pair f:
 *   HEADER:beg-(beg+FLEN)/1   upper(ctg[beg .. beg + RLEN))
 *   HEADER:beg-(beg+FLEN)/2   the upper-cased reverse complement of ctg[beg + NBEG .. beg + FLEN)            (N / n give N)
 * In a batch read 2p is the /2 record and read 2p + 1 the /1 record: the order in which the host reader of the command line hands
 * an interleaved file to dbtk_align_batch (the record that completed the pair first).
 *
 * Source locus (BED lines CTG <TAB> START <TAB> END <TAB> LOCUS, half-open, 0-based; CTG = the header without '>' up to the first
 * blank): the lowest LOCUS among the intervals of the fragment's contig with START < beg + FLEN && beg < END, or nloci when there is
 * none.  That is bedtools map's default overlap (1 bp) with distinct_sort_num followed by the reference's stoull of the title field,
 * which stops at the first comma (src/aQueryFasta_thread.cpp:492-506).  Built once on the host as a step function over beg per
 * contig; the device and dbtk_sim_describe answer by binary search in the same table.
 *
 * All entry points return dbtk_status_t (dbtk.h); dbtk_last_error() holds the message.  dbtk_sim_open / _info / _describe / _contig
 * need no device; there is no CPU path for the rest: dbtk_sim_attach fails with DBTK_ERR_NO_DEVICE without a HIP device.  A handle
 * belongs to one thread at a time.  This header has a version of its own: DBTK_ABI_VERSION (dbtk.h) did not move when it was added.
 */
#ifndef DBTK_SIM_H_
#define DBTK_SIM_H_

#include <stdint.h>

#include "dbtk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBTK_SIM_API_VERSION 1u
uint32_t dbtk_sim_api_version(void);

typedef struct dbtk_sim dbtk_sim_t;

/* Reads the FASTA (line ends stripped, '\r' too) and the BED.  On stderr, for every record shorter than ml, the reference's line
 * "Contig >NAME ignored, size = N < MIN_CTG_LEN".
 * DBTK_ERR_ARG: rlen >= flen (the reference segfaults at rlen == flen), rlen > DBTK_MAX_READ_LEN, rlen == 0, cv == 0, cv > 2 * rlen
 * (SHFT = 0: the reference loops for ever), nloci 0 or above 2^32 - 2.  DBTK_ERR_IO: a file cannot be read.  DBTK_ERR_FORMAT: a
 * header line without '>'; a sequence byte outside ACGTNacgtn (the message names contig and offset; the reference prints byte 127
 * or reads past its table for those); a BED line with fewer than four fields, START >= END or LOCUS >= nloci (the message names the
 * line).  BED lines naming a contig that is absent or was skipped are ignored. */
dbtk_status_t dbtk_sim_open(const char* fasta, const char* bed, uint32_t flen, uint32_t rlen, uint32_t cv, uint64_t ml, uint64_t nloci, dbtk_sim_t** out);
void dbtk_sim_free(dbtk_sim_t* sim);

typedef struct dbtk_sim_facts {
    uint64_t ncontigs;    /* contigs kept */
    uint64_t nskipped;    /* records shorter than ml */
    uint64_t nfrags;      /* fragments = pairs */
    uint64_t arena_bytes; /* bases of the kept contigs */
    uint64_t nbreaks;     /* breakpoints of the source-locus step functions (at least one per contig) */
    uint32_t flen, rlen, shft, ngroups; /* ngroups: contig groups the arena goes to the device in (0 before dbtk_sim_attach) */
} dbtk_sim_facts_t;
dbtk_status_t dbtk_sim_info(const dbtk_sim_t* sim, dbtk_sim_facts_t* out);
/* Kept contig c: its header line ('>' and description included, NUL-terminated) and its bases as read (not upper-cased); both
 * valid while the handle lives. */
dbtk_status_t dbtk_sim_contig(const dbtk_sim_t* sim, uint64_t c, const char** header, const uint8_t** bases, uint64_t* size, uint64_t* first_frag);
/* Fragments first_frag .. first_frag + n - 1: index of the kept contig, beg, source locus (nloci: none); each array may be null. */
dbtk_status_t dbtk_sim_describe(const dbtk_sim_t* sim, uint64_t first_frag, uint64_t n, uint32_t* contig, uint64_t* beg, uint32_t* src);
/* Every locus with an interval that overlaps fragment `frag`, ascending and distinct — the list distinct_sort_num prints into the
 * title (its first entry is the source locus).  *n = how many there are; the first min(*n, cap) go to loci (may be null). */
dbtk_status_t dbtk_sim_labels(const dbtk_sim_t* sim, uint64_t frag, uint32_t* loci, uint32_t cap, uint32_t* n);

/* Uploads the tables and makes room for the arena.  An assembly with more bases than DBTK_SIM_ARENA_BYTES (environment; default
 * 2^30, any value >= flen) goes through in groups of whole contigs, one group in HBM at a time (a batch that needs another group
 * waits, in stream order, for its upload).  DBTK_ERR_NOMEM, with the sizes in the message, when a single contig is larger than the
 * arena or HBM does not suffice. */
dbtk_status_t dbtk_sim_attach(dbtk_sim_t* sim, int device_id);
/* Tiles pairs first_frag .. first_frag + npairs - 1 into one of two alternating buffer sets, asynchronously on the handle's stream:
 * batch i + 1 may be made while batch i is aligned (the set is written only after the batch aligned from it two calls ago has
 * finished: dbtk_sim_align leaves an event).  *d_seq: the reads back to back, 16-byte aligned, readable (and zeroed) up to the next
 * multiple of 16; *d_offsets: uint64[2 * npairs + 1]; *d_src: uint32[npairs]; *max_read_len = rlen.  The pointers (each may be
 * null) stay valid until the second next dbtk_sim_batch.  A batch may span any number of contigs and contig groups.
 * DBTK_ERR_ARG: npairs 0 or above 2^31 - 1, or the range exceeds the fragments. */
dbtk_status_t dbtk_sim_batch(dbtk_sim_t* sim, uint64_t first_frag, uint64_t npairs, void** d_seq, void** d_offsets, void** d_src, uint32_t* max_read_len);
/* Waits until the batch made last is complete (what a consumer other than dbtk_sim_align needs before it reads the buffers). */
dbtk_status_t dbtk_sim_batch_wait(dbtk_sim_t* sim);
/* The batch made last through the hot path of `ctx` (a context on the same device).  sync = 0: as dbtk_align_batch_device — the
 * context's stream waits for the tiling by an event, nothing waits on the host, no records.  sync = 1: as dbtk_ingest_align with
 * sync = 1 — run to completion, records in pair order. */
dbtk_status_t dbtk_sim_align(dbtk_sim_t* sim, dbtk_ctx_t* ctx, int sync, dbtk_pair_rec_t* recs, uint64_t rec_cap, uint64_t* nrec);
/* Of all dbtk_sim_batch calls since dbtk_sim_attach: milliseconds in k_sim_tile (HIP events; synchronises the handle's stream), the
 * bytes of reads it wrote, and the bytes of arena uploaded. */
dbtk_status_t dbtk_sim_times(dbtk_sim_t* sim, double* tile_ms, uint64_t* bytes_written, uint64_t* bytes_uploaded);

#ifdef __cplusplus
}
#endif
#endif
