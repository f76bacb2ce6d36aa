// dbtk_internal.h — host-side structures and seams shared by every translation unit of the library: dbtk_rpgg.cpp, dbtk_hip.hip and
// the side modules (dbtk_pred.hip, dbtk_kcp.hip, dbtk_sim.hip, dbtk_eval.hip, dbtk_assoc.hip) with their dbtk_dev.h.
#ifndef DBTK_INTERNAL_H_
#define DBTK_INTERNAL_H_

#include <stdint.h>

#include <atomic>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/dbtk.h"

// The RPGG exactly as the reference's loaders see it (flat, file-equivalent),
// plus the output order derived once at load time.
inline uint64_t dbtk_next_uid() { static std::atomic<uint64_t> n{0}; return ++n; }
struct dbtk_rpgg {
    // Process-unique, never reused: what the per-device caches of the tables built from this handle are keyed by (a freed
    // handle's ADDRESS can come back with the next `new`; its id cannot, so a context leaked with its tables can never lend
    // them to another RPGG).
    const uint64_t uid = dbtk_next_uid();
    uint32_t ksize = 0;
    uint64_t nloci = 0;
    std::vector<uint64_t> keys;   // PREF.kmers.dbi
    std::vector<uint32_t> vals;
    std::vector<uint32_t> vv;
    std::vector<uint64_t> fl_cnt, fl_ks;    // PREF.fl.kdb
    std::vector<uint64_t> tre_cnt, tre_ks;  // PREF.tre.kdb (may be empty)
    std::vector<uint64_t> tr_cnt, tr_ks;    // PREF.tr.kmers, file order
    std::vector<uint8_t> qc;                // empty or nloci
    std::vector<uint64_t> bt_cnt, bt_ks;    // PREF.bt.kmdb (may be empty)
    std::vector<uint16_t> bt_vs;
    std::vector<uint64_t> gr_cnt, gr_ks;    // PREF.graph.kmers / PREF.graph.umap (empty: no graph loaded)
    std::vector<uint8_t> gr_ms;
    // derived
    bool order_done = false;          // out_slot / out_beg / out_kmer are made (finish_order: the loader runs it beside the index file's read)
    std::vector<uint64_t> out_slot;   // file index -> position in OUT.trkmc.ar
    std::vector<uint64_t> out_kmer;   // position -> k-mer
    std::vector<uint64_t> out_beg;    // nloci+1: first position of each locus
    // sidecar of the GPU-layout per-locus index images (dbtk_locus.h; dbtk_rpgg_set_index_cache): its file and what to do with it
    std::string idx_cache;
    int idx_cache_mode = 0;           // 0: none; 1: load it when present and valid; 2: that, and write it after a build
};

struct dbtk_sim;
namespace dbtk {
void set_error(const std::string& msg);
dbtk_status_t finish_rpgg(dbtk_rpgg* g);  // validation + output order
// No exception crosses the C-ABI: an entry point that parses files or allocates host memory runs its body through this
// (a count field of a damaged file can ask for terabytes: std::bad_alloc / std::length_error become status codes).
template <class F> dbtk_status_t guarded(F&& f) noexcept {
    try { return f(); }
    catch (const std::bad_alloc&) { set_error("out of host memory (a damaged file, or a batch too large for this host)"); return DBTK_ERR_NOMEM; }
    catch (const std::exception& e) { set_error(std::string("internal error: ") + e.what()); return DBTK_ERR_FORMAT; }
    catch (...) { set_error("internal error"); return DBTK_ERR_FORMAT; }
}
// What dbtk_pred_load_ctx (dbtk_pred.hip) must know of a context and the public seam does not say: its device, the length of the
// counts part of its accumulators, and the pairs appended by dbtk_ingest_align_merged (on any lane) that no batch has taken yet.
struct CtxFacts { int device; uint64_t ntrkmers, unflushed_pairs; };
dbtk_status_t ctx_facts(const dbtk_ctx_t* c, CtxFacts* out);
// A batch another part of the library made in HBM on a stream of its own (dbtk_sim.hip), through the hot path of `c` (on `device`): the
// context's stream waits for `ready` (a hipEvent_t) before its kernels and records `done` (a hipEvent_t) behind them.  sync = 0: as
// dbtk_align_batch_device; sync = 1: as dbtk_ingest_align with sync = 1 (run to completion, records in pair order, no reads on the host).
dbtk_status_t ctx_align_device(dbtk_ctx_t* c, int device, const uint8_t* d_seq, const uint64_t* d_off, uint64_t npairs, uint32_t max_read_len, int sync, void* ready,
                               void* done, dbtk_pair_rec_t* recs, uint64_t rec_cap, uint64_t* nrec);
// ---- what the genotype score (dbtk_eval.hip) needs of the rest of the library
// The class table of (g, device), shared with the contexts of that pair: built by whoever comes first, freed by whoever leaves last
// (dbtk_hip.hip: the table shares).  *ref goes back to tables_release.
struct ClsView { const void* cls; uint64_t mask; uint32_t shift; };
dbtk_status_t tables_acquire(const dbtk_rpgg* g, int device, ClsView* out, void** ref);
void tables_release(void* ref);
// An attached sim handle (dbtk_sim.hip): where it lives, and its assembly group by group.  A span is one BED line clipped to its
// contig, ctg[START, min(END, size)), as an offset into the group's arena.  sim_group_load makes group g the resident one, in the
// order of the handle's stream (nothing is uploaded when it is resident already).
struct SimSeam { int device; uint64_t nloci; uint32_t ngroups; void* stream; const uint8_t* d_arena; };
struct SimSpan { uint64_t off, n; uint32_t locus; };
dbtk_status_t sim_seam(dbtk_sim* s, SimSeam* out);
dbtk_status_t sim_group_spans(const dbtk_sim* s, uint32_t g, std::vector<SimSpan>* out);
dbtk_status_t sim_group_load(dbtk_sim* s, uint32_t g);
}  // namespace dbtk

// ---- what the association scan (dbtk_assoc.hip) needs of the matrix and dosage handles (dbtk_pred.hip): the float32 rows as they
// lie in HBM, [nrows][ns], complete when the call returns, with the loci's cumulative row counts on the host.  pred_rows refuses a
// windowed handle; dosage_rows makes the values of dbtk_dosage_values in the handle's buffer and refuses an unfinished handle.
struct dbtk_pred;
struct dbtk_dosage;
namespace dbtk {
struct RowsView { int device = 0; uint64_t ns = 0, nrows = 0, ntr = 0; const float* d_rows = nullptr; std::vector<uint32_t> nk_cum; };
dbtk_status_t pred_rows(dbtk_pred* p, RowsView* out);
dbtk_status_t dosage_rows(dbtk_dosage* d, RowsView* out);
}  // namespace dbtk

#endif
