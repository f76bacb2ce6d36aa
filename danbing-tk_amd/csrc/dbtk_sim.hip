// dbtk_sim.hip — the simulated read source (include/dbtk_sim.h): the host pass over assembly and BED, the tiling kernel, the handle.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dbtk_sim.h"
#include "dbtk_dev.h"
#include "dbtk_internal.h"

using namespace dbtk;

namespace {

// a kept contig as the kernel sees it: where its bases lie in the arena of its group, and its part of the tables
struct SimContig {
    uint64_t off, len;    // bytes into the group's arena; bases
    uint64_t first_frag;  // number of its first fragment (contigs without fragments share the next one's)
    uint32_t brk0, brk1;  // its breakpoints: brk_pos / brk_src [brk0, brk1), brk_pos[brk0] == 0
};

struct SimTile {
    const uint8_t* arena;
    const SimContig* ctg;
    const uint64_t* brk_pos;
    const uint32_t* brk_src;
    uint32_t c0, c1;       // the contigs of the resident group
    uint64_t batch_first;  // fragment number of the batch's pair 0
    uint64_t q0, q1;       // pairs of the batch (relative to pair 0) this launch tiles: all of them in contigs c0 .. c1 - 1
    uint64_t npairs;       // of the batch (q1 == npairs: this launch closes the batch)
    uint32_t flen, rlen, shft;
    uint8_t* seq;
    uint64_t* offs;
    uint32_t* src;
};

// complement of an upper-case base by the bits that tell A C G T N apart: (c >> 1) & 7 = 0, 1, 3, 2, 7
constexpr uint64_t SIM_COMP = (uint64_t)'T' | (uint64_t)'G' << 8 | (uint64_t)'A' << 16 | (uint64_t)'C' << 24 | (uint64_t)'N' << 56;
__host__ __device__ inline uint32_t sim_comp(uint32_t up) { return (uint32_t)(SIM_COMP >> (((up >> 1) & 7u) << 3)) & 0xFFu; }

struct SimAt { const uint8_t* base; uint64_t beg; uint32_t ci; };  // a pair's contig (its bases, its index) and beg

// the contig of fragment `frag`: the last one of [c0, c1) whose first fragment is not above it
__device__ inline SimAt sim_locate(const SimTile& a, uint64_t frag) {
    uint32_t lo = a.c0, hi = a.c1;  // (first_frag[lo] <= frag holds for the launch's pairs)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.ctg[mid].first_frag <= frag) lo = mid; else hi = mid;
    }
    const SimContig c = a.ctg[lo];
    return SimAt{a.arena + c.off, (frag - c.first_frag) * a.shft, lo};
}

// what the lane owning a pair's first byte writes beside it: the two offsets, and the source locus by the step function of the contig
__device__ inline void sim_pair_meta(const SimTile& a, uint64_t q, const SimAt& at) {
    const uint64_t o = q * 2 * a.rlen;
    a.offs[2 * q] = o;
    a.offs[2 * q + 1] = o + a.rlen;
    uint32_t lo = a.ctg[at.ci].brk0, hi = a.ctg[at.ci].brk1;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.brk_pos[mid] <= at.beg) lo = mid; else hi = mid;
    }
    a.src[q] = a.brk_src[lo];
}

// One lane per 16 consecutive bytes of d_seq.  Pair q of the batch lies at [q * 2 RLEN, (q + 1) * 2 RLEN): first the /2 record (the
// reverse complement of the fragment's last RLEN bases), then the /1 record (its first RLEN bases).  A lane whose 16 bytes lie inside
// one read loads them with one 16-byte read; any other assembles them byte by byte.  Either way the 16 bytes leave in one store,
// except in the first and last chunk of a launch that does not begin or end on a chunk boundary (a batch cut by a contig group).
__global__ void __launch_bounds__(256) k_sim_tile(const SimTile a) {
    const uint64_t twoR = 2ull * a.rlen;
    const uint64_t r0 = a.q0 * twoR, r1 = a.q1 * twoR;
    const uint64_t c = r0 / 16 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t cb = c * 16;
    const uint64_t lo = cb > r0 ? cb : r0, hi = cb + 16 < r1 ? cb + 16 : r1;
    if (lo >= hi) return;
    const bool closes = a.q1 == a.npairs && hi == r1;          // the lane that owns the batch's last byte
    const uint64_t shi = closes ? cb + 16 : hi;                // ... also zeroes the tail up to the multiple of 16
    uint64_t q = lo / twoR;
    uint32_t within = (uint32_t)(lo - q * twoR);
    SimAt at = sim_locate(a, a.batch_first + q);
    uint32_t w[4] = {0, 0, 0, 0};
    const uint32_t pos0 = within >= a.rlen ? within - a.rlen : within;
    if (hi - lo == 16 && pos0 + 16 <= a.rlen) {
        if (within == 0) sim_pair_meta(a, q, at);
        uint32_t v[4];
        if (within >= a.rlen) {  // /1: ascending
            __builtin_memcpy(v, at.base + at.beg + pos0, 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = v[i] & 0xDFDFDFDFu;
        } else {                 // /2: descending and complemented; byte i of the chunk = comp(ctg[beg + FLEN - 1 - pos0 - i])
            __builtin_memcpy(v, at.base + at.beg + a.flen - 16 - pos0, 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t u = __builtin_bswap32(v[3 - i]) & 0xDFDFDFDFu;
                w[i] = sim_comp(u & 0xFFu) | sim_comp((u >> 8) & 0xFFu) << 8 | sim_comp((u >> 16) & 0xFFu) << 16 | sim_comp(u >> 24) << 24;
            }
        }
    } else {
        const uint32_t i0 = (uint32_t)(lo - cb), i1 = (uint32_t)(hi - cb);
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            if (i < i0 || i >= i1) continue;
            if (within == twoR) { within = 0; ++q; at = sim_locate(a, a.batch_first + q); }
            if (within == 0) sim_pair_meta(a, q, at);
            uint32_t b;
            if (within >= a.rlen) b = at.base[at.beg + (within - a.rlen)] & 0xDFu;
            else b = sim_comp(at.base[at.beg + a.flen - 1 - within] & 0xDFu);
            w[i >> 2] |= b << (8 * (i & 3));
            ++within;
        }
    }
    if (closes) a.offs[2 * a.npairs] = r1;
    if (lo == cb && shi == cb + 16) {
        *reinterpret_cast<uint4*>(a.seq + cb) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const uint32_t i0 = (uint32_t)(lo - cb), i1 = (uint32_t)(shi - cb);
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i)
            if (i >= i0 && i < i1) a.seq[cb + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

constexpr uint64_t SIM_ARENA_DEFAULT = 1ull << 30;

// a BED interval as the fragments see it: it covers those with beg in [from, to); beside it the line's own START and END
struct SimIv { uint64_t from, to; uint32_t locus; uint64_t start, end; };

struct HostContig {
    std::string header;          // the header line, '>' included
    uint64_t off = 0, len = 0;   // into `bases`
    uint64_t first_frag = 0, nfrag = 0;
    uint32_t brk0 = 0, brk1 = 0;
    uint64_t iv0 = 0, iv1 = 0, iv_span = 0;  // its intervals (dbtk_sim::ivs, ascending by `from`) and the longest to - from among them
};

struct BufSet {  // (destroyed last to first: the buffers, then the events)
    DevEvent consumed, made;
    DevArr<uint32_t> d_src;
    DevArr<uint64_t> d_off;
    DevArr<uint8_t> d_seq;
    bool in_use = false;  // `consumed` has been recorded since the set was last filled
    uint64_t npairs = 0;
};

}  // namespace

struct dbtk_sim {
    uint32_t flen = 0, rlen = 0, cv = 0, shft = 0;
    uint64_t ml = 0, nloci = 0, nfrags = 0, nskipped = 0;
    std::vector<uint8_t> bases;  // the kept contigs back to back, as read
    std::vector<HostContig> ctg;
    std::vector<uint64_t> brk_pos;
    std::vector<uint32_t> brk_src;
    std::vector<SimIv> ivs;      // every kept contig's intervals (dbtk_sim_labels)
    // device side
    int device = -1, num_cu = 1;
    std::vector<uint32_t> group_c0;  // contigs [group_c0[g], group_c0[g + 1]) form group g
    int64_t resident = -1;
    uint64_t arena_cap = 0;
    int cur = -1;  // the set of the batch made last
    // (destroyed last to first, as sim_release_device lets go of them: the batch sets, the timing events, the tables, the stream)
    DevStream stream;
    DevArr<uint32_t> d_brk_src;
    DevArr<uint64_t> d_brk_pos;
    DevArr<SimContig> d_ctg;
    DevArr<uint8_t> d_arena;
    std::vector<DevEvent> spare;
    std::deque<std::pair<DevEvent, DevEvent>> timing;  // around launches whose time is not yet taken
    BufSet set[2];
    double tile_ms = 0;
    uint64_t bytes_written = 0, bytes_uploaded = 0;
};

namespace {

bool read_file(const char* fn, std::string* out) {
    FILE* f = fopen(fn, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
    const bool ok = !ferror(f);
    fclose(f);
    return ok;
}

uint64_t sim_nfrag(uint64_t size, uint32_t flen, uint32_t shft) { return size < flen ? 0 : (size - flen) / shft + 1; }

dbtk_status_t sim_open_impl(const char* fasta, const char* bed, uint32_t flen, uint32_t rlen, uint32_t cv, uint64_t ml, uint64_t nloci, dbtk_sim_t** out) {
    if (!out) { set_error("dbtk_sim_open: null argument"); return DBTK_ERR_ARG; }
    *out = nullptr;
    if (!fasta || !bed) { set_error("dbtk_sim_open: null argument"); return DBTK_ERR_ARG; }
    if (rlen == 0 || rlen >= flen) { set_error("dbtk_sim_open: the read length must be at least 1 and below the fragment length (RLEN " + std::to_string(rlen) + ", FLEN " + std::to_string(flen) + ")"); return DBTK_ERR_ARG; }
    if (rlen > DBTK_MAX_READ_LEN) { set_error("dbtk_sim_open: the read length " + std::to_string(rlen) + " exceeds DBTK_MAX_READ_LEN (" + std::to_string(DBTK_MAX_READ_LEN) + ")"); return DBTK_ERR_ARG; }
    if (cv == 0 || cv > 2 * rlen) { set_error("dbtk_sim_open: the coverage must be 1 .. 2 * RLEN (cv " + std::to_string(cv) + ", RLEN " + std::to_string(rlen) + "): the step 2 * RLEN / cv would be 0"); return DBTK_ERR_ARG; }
    if (nloci == 0 || nloci > 0xFFFFFFFEull) { set_error("dbtk_sim_open: nloci must be 1..2^32-2"); return DBTK_ERR_ARG; }
    std::unique_ptr<dbtk_sim> s(new dbtk_sim);
    s->flen = flen; s->rlen = rlen; s->cv = cv; s->shft = 2 * rlen / cv; s->ml = ml; s->nloci = nloci;
    std::string text;
    if (!read_file(fasta, &text)) { set_error(std::string("cannot read ") + fasta); return DBTK_ERR_IO; }
    s->bases.reserve(text.size());
    std::unordered_map<std::string, std::vector<uint32_t>> by_name;
    // ---- the FASTA: a header line, then sequence lines up to the next line that begins with '>' (src/sim_reads.cpp:164-167)
    size_t at = 0;
    auto next_line = [&](size_t* b, size_t* e) {
        if (at >= text.size()) return false;
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        *b = at; *e = nl;
        if (*e > *b && text[*e - 1] == '\r') --*e;
        at = nl + 1;
        return true;
    };
    size_t b, e;
    bool have = next_line(&b, &e);
    while (have) {
        if (e == b) { have = next_line(&b, &e); continue; }  // (an empty line between records)
        if (text[b] != '>') { set_error(std::string(fasta) + ": a record's header line does not begin with '>' (byte " + std::to_string(b) + ")"); return DBTK_ERR_FORMAT; }
        HostContig c;
        c.header.assign(text, b, e - b);
        c.off = s->bases.size();
        while ((have = next_line(&b, &e)) && !(e > b && text[b] == '>')) {
            for (size_t i = b; i < e; ++i) {
                const uint8_t ch = (uint8_t)text[i];
                const uint8_t up = ch & 0xDFu;
                if (!(up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N') || !((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'))) {
                    set_error(std::string(fasta) + ": contig " + c.header + " offset " + std::to_string(s->bases.size() - c.off + (i - b)) + ": byte " + std::to_string((unsigned)ch) +
                              " is none of ACGTNacgtn");
                    return DBTK_ERR_FORMAT;
                }
            }
            s->bases.insert(s->bases.end(), text.begin() + b, text.begin() + e);
        }
        c.len = s->bases.size() - c.off;
        if (c.len < ml) {
            fprintf(stderr, "Contig %s ignored, size = %llu < MIN_CTG_LEN\n", c.header.c_str(), (unsigned long long)c.len);
            s->bases.resize(c.off);
            ++s->nskipped;
            continue;
        }
        c.nfrag = sim_nfrag(c.len, flen, s->shft);
        c.first_frag = s->nfrags;
        s->nfrags += c.nfrag;
        size_t ne = 1;
        while (ne < c.header.size() && c.header[ne] != ' ' && c.header[ne] != '\t') ++ne;
        if (s->ctg.size() >= 0x7FFFFFFFull) { set_error(std::string(fasta) + ": more than 2^31 - 1 contigs"); return DBTK_ERR_FORMAT; }
        by_name[c.header.substr(1, ne - 1)].push_back((uint32_t)s->ctg.size());
        s->ctg.push_back(std::move(c));
    }
    text.clear(); text.shrink_to_fit();
    // ---- the BED: per contig the intervals; each covers the fragments with beg in [max(0, START - FLEN + 1), END)
    typedef SimIv Iv;
    std::vector<std::vector<Iv>> ivs(s->ctg.size());
    if (!read_file(bed, &text)) { set_error(std::string("cannot read ") + bed); return DBTK_ERR_IO; }
    at = 0;
    for (uint64_t lineno = 1; next_line(&b, &e); ++lineno) {
        if (e == b) continue;
        const std::string where = std::string(bed) + " line " + std::to_string(lineno) + ": ";
        size_t f[5], nf = 1;
        f[0] = b;
        for (size_t i = b; i < e && nf < 5; ++i) if (text[i] == '\t') f[nf++] = i + 1;
        if (nf < 4) { set_error(where + "expected CTG <TAB> START <TAB> END <TAB> LOCUS"); return DBTK_ERR_FORMAT; }
        auto num = [&](size_t fb, size_t fe, uint64_t* v) {
            if (fb >= fe) return false;
            *v = 0;
            for (size_t i = fb; i < fe; ++i) { if (text[i] < '0' || text[i] > '9' || *v > (1ull << 60)) return false; *v = *v * 10 + (uint64_t)(text[i] - '0'); }
            return true;
        };
        uint64_t st = 0, en = 0, lc = 0;
        const size_t f3e = nf > 4 ? f[4] - 1 : e;
        if (!num(f[1], f[2] - 1, &st) || !num(f[2], f[3] - 1, &en) || !num(f[3], f3e, &lc)) { set_error(where + "START, END and LOCUS must be non-negative integers"); return DBTK_ERR_FORMAT; }
        if (st >= en) { set_error(where + "START " + std::to_string(st) + " is not below END " + std::to_string(en)); return DBTK_ERR_FORMAT; }
        if (lc >= nloci) { set_error(where + "LOCUS " + std::to_string(lc) + " is not below the number of loci (" + std::to_string(nloci) + ")"); return DBTK_ERR_FORMAT; }
        const auto it = by_name.find(text.substr(b, f[1] - 1 - b));
        if (it == by_name.end()) continue;  // a contig that is absent or was skipped
        for (uint32_t ci : it->second) ivs[ci].push_back(Iv{st + 1 > flen ? st + 1 - flen : 0, en, (uint32_t)lc, st, en});
    }
    // ---- the step functions: a sweep over the interval ends; a breakpoint wherever the lowest covering locus changes
    for (size_t ci = 0; ci < s->ctg.size(); ++ci) {
        HostContig& c = s->ctg[ci];
        std::vector<std::pair<uint64_t, int64_t>> ev;  // (position, +(locus + 1) opens | -(locus + 1) closes)
        for (const Iv& v : ivs[ci]) { ev.emplace_back(v.from, (int64_t)v.locus + 1); ev.emplace_back(v.to, -((int64_t)v.locus + 1)); }
        std::sort(ev.begin(), ev.end());
        if (s->brk_pos.size() + ev.size() + 1 > 0xFFFFFFFFull) { set_error(std::string(bed) + ": too many intervals"); return DBTK_ERR_FORMAT; }
        c.brk0 = (uint32_t)s->brk_pos.size();
        std::multiset<uint32_t> open;
        uint32_t cur = (uint32_t)nloci;
        s->brk_pos.push_back(0); s->brk_src.push_back(cur);
        for (size_t i = 0; i < ev.size();) {
            const uint64_t pos = ev[i].first;
            for (; i < ev.size() && ev[i].first == pos; ++i) {
                if (ev[i].second > 0) open.insert((uint32_t)(ev[i].second - 1));
                else open.erase(open.find((uint32_t)(-ev[i].second - 1)));
            }
            const uint32_t v = open.empty() ? (uint32_t)nloci : *open.begin();
            if (v == cur) continue;
            cur = v;
            if (pos == 0) s->brk_src.back() = v;
            else { s->brk_pos.push_back(pos); s->brk_src.push_back(v); }
        }
        c.brk1 = (uint32_t)s->brk_pos.size();
        std::sort(ivs[ci].begin(), ivs[ci].end(), [](const Iv& x, const Iv& y) { return x.from < y.from; });
        c.iv0 = s->ivs.size();
        for (const Iv& v : ivs[ci]) { c.iv_span = std::max(c.iv_span, v.to - v.from); s->ivs.push_back(v); }
        c.iv1 = s->ivs.size();
    }
    *out = s.release();
    return DBTK_OK;
}

// the kept contig of fragment f (f < nfrags)
size_t host_contig_of(const dbtk_sim* s, uint64_t f) {
    size_t lo = 0, hi = s->ctg.size();
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (s->ctg[mid].first_frag <= f) lo = mid; else hi = mid;
    }
    return lo;
}

dbtk_status_t sim_describe_impl(const dbtk_sim_t* s, uint64_t first, uint64_t n, uint32_t* contig, uint64_t* beg, uint32_t* src) {
    if (!s) { set_error("dbtk_sim_describe: null argument"); return DBTK_ERR_ARG; }
    if (first > s->nfrags || n > s->nfrags - first) { set_error("dbtk_sim_describe: fragments " + std::to_string(first) + " + " + std::to_string(n) + " of " + std::to_string(s->nfrags)); return DBTK_ERR_ARG; }
    if (!n) return DBTK_OK;
    size_t ci = host_contig_of(s, first);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t f = first + i;
        while (f >= s->ctg[ci].first_frag + s->ctg[ci].nfrag) ++ci;
        const HostContig& c = s->ctg[ci];
        const uint64_t bg = (f - c.first_frag) * s->shft;
        if (contig) contig[i] = (uint32_t)ci;
        if (beg) beg[i] = bg;
        if (src) {
            const auto it = std::upper_bound(s->brk_pos.begin() + c.brk0, s->brk_pos.begin() + c.brk1, bg);
            src[i] = s->brk_src[(size_t)(it - s->brk_pos.begin()) - 1];
        }
    }
    return DBTK_OK;
}

// every locus whose interval covers the fragment, ascending and distinct: the list bedtools map -o distinct_sort_num prints
dbtk_status_t sim_labels_impl(const dbtk_sim_t* s, uint64_t frag, uint32_t* loci, uint32_t cap, uint32_t* n) {
    if (!s || !n) { set_error("dbtk_sim_labels: null argument"); return DBTK_ERR_ARG; }
    if (frag >= s->nfrags) { set_error("dbtk_sim_labels: fragment " + std::to_string(frag) + " of " + std::to_string(s->nfrags)); return DBTK_ERR_ARG; }
    const HostContig& c = s->ctg[host_contig_of(s, frag)];
    const uint64_t beg = (frag - c.first_frag) * s->shft;
    // candidates: from <= beg, and from > beg - iv_span (an interval that starts earlier has ended)
    const auto b = s->ivs.begin() + c.iv0, e = s->ivs.begin() + c.iv1;
    auto hi = std::upper_bound(b, e, beg, [](uint64_t v, const SimIv& x) { return v < x.from; });
    std::vector<uint32_t> got;
    for (auto it = hi; it != b;) {
        --it;
        if (beg - it->from >= c.iv_span) break;
        if (beg < it->to) got.push_back(it->locus);
    }
    std::sort(got.begin(), got.end());
    got.erase(std::unique(got.begin(), got.end()), got.end());
    *n = (uint32_t)got.size();
    if (loci) for (size_t i = 0; i < got.size() && i < cap; ++i) loci[i] = got[i];
    return DBTK_OK;
}

void sim_release_device(dbtk_sim* s) {
    if (s->device < 0) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (BufSet& b : s->set) {
        if (b.in_use && b.consumed) (void)hipEventSynchronize(b.consumed);
        b = BufSet();
    }
    s->timing.clear();
    s->spare.clear();
    s->d_arena.drop(); s->d_ctg.drop(); s->d_brk_pos.drop(); s->d_brk_src.drop();
    s->stream = DevStream();
    s->device = -1; s->resident = -1; s->cur = -1; s->group_c0.clear();
}

dbtk_status_t sim_nomem(hipError_t e, const char* what, uint64_t bytes) {
    if (e == hipSuccess) return DBTK_OK;
    (void)hipGetLastError();
    set_error(std::string("simulated reads: no device memory for ") + what + " (" + std::to_string(bytes) + " bytes)");
    return DBTK_ERR_NOMEM;
}
template <class T> dbtk_status_t sim_alloc(DevArr<T>& a, uint64_t n, const char* what) {
    return sim_nomem(a.alloc(std::max<uint64_t>(n, 1)), what, n * sizeof(T));  // (never empty)
}

dbtk_status_t sim_attach_impl(dbtk_sim_t* s, int device_id) {
    if (!s) { set_error("dbtk_sim_attach: null argument"); return DBTK_ERR_ARG; }
    if (s->device >= 0) { set_error("dbtk_sim_attach: the handle is attached already"); return DBTK_ERR_ARG; }
    uint64_t arena = SIM_ARENA_DEFAULT;
    if (const char* e = getenv("DBTK_SIM_ARENA_BYTES")) {
        arena = strtoull(e, nullptr, 10);
        if (arena < s->flen) { set_error("DBTK_SIM_ARENA_BYTES: at least the fragment length (" + std::to_string(s->flen) + ")"); return DBTK_ERR_ARG; }
    }
    int ndev = 0;
    if (const dbtk_status_t nd = device_count(&ndev)) return nd;
    if (device_id < 0 || device_id >= ndev) { set_error("dbtk_sim_attach: device " + std::to_string(device_id) + " of " + std::to_string(ndev)); return DBTK_ERR_ARG; }
    // groups of whole contigs, each within the arena; the device table holds every contig's offset inside its group
    std::vector<SimContig> tab(s->ctg.size());
    std::vector<uint32_t> g0{0};
    uint64_t used = 0, largest = 0;
    for (size_t ci = 0; ci < s->ctg.size(); ++ci) {
        const HostContig& c = s->ctg[ci];
        if (c.len > arena) {
            set_error("simulated reads: contig " + c.header + " has " + std::to_string(c.len) + " bases, the arena holds " + std::to_string(arena) + " (DBTK_SIM_ARENA_BYTES)");
            return DBTK_ERR_NOMEM;
        }
        if (used + c.len > arena) { g0.push_back((uint32_t)ci); used = 0; }
        tab[ci] = SimContig{used, c.len, c.first_frag, c.brk0, c.brk1};
        used += c.len;
        largest = std::max(largest, used);
    }
    g0.push_back((uint32_t)s->ctg.size());
    DEVCHK(hipSetDevice(device_id));
    s->device = device_id;
    dbtk_status_t st = [&]() -> dbtk_status_t {
        DEVCHK(device_cus(device_id, &s->num_cu));
        DEVCHK(s->stream.create(hipStreamNonBlocking));
        dbtk_status_t a;
        // (16 bytes of slack: the 16-byte read of a chunk never leaves its read, but the allocation is never empty either)
        if ((a = sim_alloc(s->d_arena, largest + 16, "the assembly's arena"))) return a;
        s->arena_cap = largest;
        if ((a = sim_alloc(s->d_ctg, tab.size(), "the contig table"))) return a;
        if ((a = sim_alloc(s->d_brk_pos, s->brk_pos.size(), "the source-locus breakpoints"))) return a;
        if ((a = sim_alloc(s->d_brk_src, s->brk_src.size(), "the source-locus breakpoints"))) return a;
        if (!tab.empty()) DEVCHK(hipMemcpy(s->d_ctg, tab.data(), tab.size() * sizeof(SimContig), hipMemcpyHostToDevice));
        if (!s->brk_pos.empty()) {
            DEVCHK(hipMemcpy(s->d_brk_pos, s->brk_pos.data(), s->brk_pos.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
            DEVCHK(hipMemcpy(s->d_brk_src, s->brk_src.data(), s->brk_src.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        for (BufSet& b : s->set) {
            DEVCHK(b.made.create(hipEventDisableTiming));
            DEVCHK(b.consumed.create(hipEventDisableTiming));
        }
        return DBTK_OK;
    }();
    if (st) { sim_release_device(s); return st; }
    s->group_c0 = g0;
    return DBTK_OK;
}

template <class T> dbtk_status_t sim_reserve(DevArr<T>& a, uint64_t n, const char* what) {
    const uint64_t want = n + n / 8 + 16;
    return sim_nomem(a.reserve(n, want), what, want * sizeof(T));
}

// the times of the launches that have finished (all of them with `all`)
dbtk_status_t sim_take_times(dbtk_sim* s, bool all) {
    while (!s->timing.empty()) {
        if (all) DEVCHK(hipEventSynchronize(s->timing.front().second));
        else if (hipEventQuery(s->timing.front().second) != hipSuccess) { (void)hipGetLastError(); break; }
        float ms = 0;
        DEVCHK(hipEventElapsedTime(&ms, s->timing.front().first, s->timing.front().second));
        s->tile_ms += ms;
        s->spare.push_back(std::move(s->timing.front().first));
        s->spare.push_back(std::move(s->timing.front().second));
        s->timing.pop_front();
    }
    return DBTK_OK;
}

// group g's bases into the arena, in stream order behind the launches that read the group before it
dbtk_status_t sim_make_resident(dbtk_sim* s, size_t g) {
    if (s->resident == (int64_t)g) return DBTK_OK;
    const uint32_t c0 = s->group_c0[g], c1 = s->group_c0[g + 1];
    if (c0 == c1) return DBTK_OK;  // (an assembly without a kept contig)
    const uint64_t b0 = s->ctg[c0].off, b1 = s->ctg[c1 - 1].off + s->ctg[c1 - 1].len;
    if (b1 - b0 > s->arena_cap) { set_error("simulated reads: a contig group outgrew the arena"); return DBTK_ERR_HIP; }
    if (b1 > b0) DEVCHK(hipMemcpyAsync(s->d_arena, s->bases.data() + b0, b1 - b0, hipMemcpyHostToDevice, s->stream));
    s->resident = (int64_t)g;
    s->bytes_uploaded += b1 - b0;
    return DBTK_OK;
}

dbtk_status_t sim_batch_impl(dbtk_sim_t* s, uint64_t first, uint64_t npairs, void** d_seq, void** d_offsets, void** d_src, uint32_t* max_read_len) {
    if (!s) { set_error("dbtk_sim_batch: null argument"); return DBTK_ERR_ARG; }
    if (s->device < 0) { set_error("dbtk_sim_batch: dbtk_sim_attach first"); return DBTK_ERR_ARG; }
    if (npairs == 0 || npairs > 0x7FFFFFFFull) { set_error("dbtk_sim_batch: 1 .. 2^31 - 1 pairs in one batch"); return DBTK_ERR_ARG; }
    if (first > s->nfrags || npairs > s->nfrags - first) { set_error("dbtk_sim_batch: fragments " + std::to_string(first) + " + " + std::to_string(npairs) + " of " + std::to_string(s->nfrags)); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(s->device));
    dbtk_status_t st;
    if ((st = sim_take_times(s, false))) return st;
    const int k = s->cur < 0 ? 0 : 1 - s->cur;
    BufSet& B = s->set[k];
    const uint64_t nbytes = npairs * 2 * s->rlen, padded = (nbytes + 15) & ~15ull;
    const bool grows = padded > B.d_seq.cap() || 2 * npairs + 1 > B.d_off.cap() || npairs > B.d_src.cap();
    if (B.in_use) {
        // the batch aligned from this set two calls ago: its kernels first (in stream order; on the host only where the set must grow)
        if (grows) DEVCHK(hipEventSynchronize(B.consumed));
        else DEVCHK(hipStreamWaitEvent(s->stream, B.consumed, 0));
        B.in_use = false;
    }
    if (grows) DEVCHK(hipStreamSynchronize(s->stream));  // (our own launches into the old buffers)
    if ((st = sim_reserve(B.d_seq, padded, "a batch of reads"))) return st;
    if ((st = sim_reserve(B.d_off, 2 * npairs + 1, "a batch's offsets"))) return st;
    if ((st = sim_reserve(B.d_src, npairs, "a batch's source loci"))) return st;
    B.npairs = npairs;
    // group by group: the group's bases into the arena (in stream order behind the launches that read the group before), then its pairs
    const size_t ca = host_contig_of(s, first), cz = host_contig_of(s, first + npairs - 1);
    size_t g = (size_t)(std::upper_bound(s->group_c0.begin(), s->group_c0.end(), (uint32_t)ca) - s->group_c0.begin()) - 1;
    for (;; ++g) {
        const uint32_t c0 = s->group_c0[g], c1 = s->group_c0[g + 1];
        const uint64_t gf0 = s->ctg[c0].first_frag, gf1 = c1 < s->ctg.size() ? s->ctg[c1].first_frag : s->nfrags;
        const uint64_t f0 = std::max(first, gf0), f1 = std::min(first + npairs, gf1);
        if (f0 < f1) {
            if ((st = sim_make_resident(s, g))) return st;
            SimTile a;
            a.arena = s->d_arena; a.ctg = s->d_ctg; a.brk_pos = s->d_brk_pos; a.brk_src = s->d_brk_src;
            a.c0 = c0; a.c1 = c1; a.batch_first = first; a.q0 = f0 - first; a.q1 = f1 - first; a.npairs = npairs;
            a.flen = s->flen; a.rlen = s->rlen; a.shft = s->shft;
            a.seq = B.d_seq; a.offs = B.d_off; a.src = B.d_src;
            const uint64_t r0 = a.q0 * 2 * s->rlen, r1 = a.q1 * 2 * s->rlen;
            const uint64_t nchunks = (r1 + 15) / 16 - r0 / 16;
            const uint64_t grid = (nchunks + 255) / 256;  // (at most 2^31 - 1 pairs of 512 bytes: 2^28 workgroups)
            DevEvent ev[2];
            for (DevEvent& e : ev) {
                if (!s->spare.empty()) { e = std::move(s->spare.back()); s->spare.pop_back(); }
                else DEVCHK(e.create(hipEventDefault));
            }
            s->timing.emplace_back(std::move(ev[0]), std::move(ev[1]));
            DEVCHK(hipEventRecord(s->timing.back().first, s->stream));
            hipLaunchKernelGGL(k_sim_tile, dim3((uint32_t)grid), dim3(256), 0, s->stream, a);
            DEVCHK(hipGetLastError());
            DEVCHK(hipEventRecord(s->timing.back().second, s->stream));
            s->bytes_written += r1 - r0;
        }
        if (c1 > cz) break;
    }
    DEVCHK(hipEventRecord(B.made, s->stream));
    s->cur = k;
    if (d_seq) *d_seq = B.d_seq;
    if (d_offsets) *d_offsets = B.d_off;
    if (d_src) *d_src = B.d_src;
    if (max_read_len) *max_read_len = s->rlen;
    return DBTK_OK;
}

dbtk_status_t sim_align_impl(dbtk_sim_t* s, dbtk_ctx_t* ctx, int sync, dbtk_pair_rec_t* recs, uint64_t rec_cap, uint64_t* nrec) {
    if (nrec) *nrec = 0;
    if (!s || !ctx) { set_error("dbtk_sim_align: null argument"); return DBTK_ERR_ARG; }
    if (s->device < 0 || s->cur < 0) { set_error("dbtk_sim_align: dbtk_sim_batch first"); return DBTK_ERR_ARG; }
    BufSet& B = s->set[s->cur];
    const dbtk_status_t st = ctx_align_device(ctx, s->device, B.d_seq, B.d_off, B.npairs, s->rlen, sync, (void*)B.made, (void*)B.consumed, recs, rec_cap, nrec);
    if (st == DBTK_OK || st == DBTK_ERR_OVERFLOW) B.in_use = true;
    return st;
}

}  // namespace

// ---- dbtk_internal.h: for dbtk_eval_truth_sim
dbtk_status_t dbtk::sim_seam(dbtk_sim* s, dbtk::SimSeam* out) {
    if (!s || !out) { set_error("null argument"); return DBTK_ERR_ARG; }
    out->device = s->device; out->nloci = s->nloci; out->ngroups = s->group_c0.empty() ? 0 : (uint32_t)s->group_c0.size() - 1;
    out->stream = (void*)s->stream; out->d_arena = s->d_arena;
    return DBTK_OK;
}
dbtk_status_t dbtk::sim_group_spans(const dbtk_sim* s, uint32_t g, std::vector<dbtk::SimSpan>* out) {
    if (!s || !out || (size_t)g + 1 >= s->group_c0.size()) { set_error("sim_group_spans: no such contig group"); return DBTK_ERR_ARG; }
    out->clear();
    for (uint32_t ci = s->group_c0[g]; ci < s->group_c0[g + 1]; ++ci) {
        const HostContig& c = s->ctg[ci];
        const uint64_t goff = c.off - s->ctg[s->group_c0[g]].off;  // (the group's contigs lie back to back, in `bases` as in the arena)
        for (uint64_t i = c.iv0; i < c.iv1; ++i) {
            const SimIv& v = s->ivs[i];
            const uint64_t end = std::min(v.end, c.len);
            if (v.start < end) out->push_back(dbtk::SimSpan{goff + v.start, end - v.start, v.locus});
        }
    }
    return DBTK_OK;
}
dbtk_status_t dbtk::sim_group_load(dbtk_sim* s, uint32_t g) {
    if (!s || s->device < 0 || (size_t)g + 1 >= s->group_c0.size()) { set_error("sim_group_load: an unattached handle or no such contig group"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(s->device));
    return sim_make_resident(s, g);
}

extern "C" {

uint32_t dbtk_sim_api_version(void) { return DBTK_SIM_API_VERSION; }

dbtk_status_t dbtk_sim_open(const char* fasta, const char* bed, uint32_t flen, uint32_t rlen, uint32_t cv, uint64_t ml, uint64_t nloci, dbtk_sim_t** out) {
    return guarded([&] { return sim_open_impl(fasta, bed, flen, rlen, cv, ml, nloci, out); });
}

void dbtk_sim_free(dbtk_sim_t* s) {
    if (!s) return;
    sim_release_device(s);
    delete s;
}

dbtk_status_t dbtk_sim_info(const dbtk_sim_t* s, dbtk_sim_facts_t* out) {
    if (!s || !out) { set_error("dbtk_sim_info: null argument"); return DBTK_ERR_ARG; }
    out->ncontigs = s->ctg.size(); out->nskipped = s->nskipped; out->nfrags = s->nfrags; out->arena_bytes = s->bases.size();
    out->nbreaks = s->brk_pos.size(); out->flen = s->flen; out->rlen = s->rlen; out->shft = s->shft;
    out->ngroups = s->group_c0.empty() ? 0 : (uint32_t)s->group_c0.size() - 1;
    return DBTK_OK;
}

dbtk_status_t dbtk_sim_contig(const dbtk_sim_t* s, uint64_t c, const char** header, const uint8_t** bases, uint64_t* size, uint64_t* first_frag) {
    if (!s || c >= s->ctg.size()) { set_error("dbtk_sim_contig: null handle or no such contig"); return DBTK_ERR_ARG; }
    const HostContig& h = s->ctg[c];
    if (header) *header = h.header.c_str();
    if (bases) *bases = s->bases.data() + h.off;
    if (size) *size = h.len;
    if (first_frag) *first_frag = h.first_frag;
    return DBTK_OK;
}

dbtk_status_t dbtk_sim_describe(const dbtk_sim_t* s, uint64_t first_frag, uint64_t n, uint32_t* contig, uint64_t* beg, uint32_t* src) {
    return guarded([&] { return sim_describe_impl(s, first_frag, n, contig, beg, src); });
}

dbtk_status_t dbtk_sim_labels(const dbtk_sim_t* s, uint64_t frag, uint32_t* loci, uint32_t cap, uint32_t* n) {
    return guarded([&] { return sim_labels_impl(s, frag, loci, cap, n); });
}

dbtk_status_t dbtk_sim_attach(dbtk_sim_t* s, int device_id) {
    return guarded([&] { return sim_attach_impl(s, device_id); });
}

dbtk_status_t dbtk_sim_batch(dbtk_sim_t* s, uint64_t first_frag, uint64_t npairs, void** d_seq, void** d_offsets, void** d_src, uint32_t* max_read_len) {
    return guarded([&] { return sim_batch_impl(s, first_frag, npairs, d_seq, d_offsets, d_src, max_read_len); });
}

dbtk_status_t dbtk_sim_batch_wait(dbtk_sim_t* s) {
    if (!s || s->device < 0) { set_error("dbtk_sim_batch_wait: null or unattached handle"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(s->device));
    DEVCHK(hipStreamSynchronize(s->stream));
    return DBTK_OK;
}

dbtk_status_t dbtk_sim_align(dbtk_sim_t* s, dbtk_ctx_t* ctx, int sync, dbtk_pair_rec_t* recs, uint64_t rec_cap, uint64_t* nrec) {
    return guarded([&] { return sim_align_impl(s, ctx, sync, recs, rec_cap, nrec); });
}

dbtk_status_t dbtk_sim_times(dbtk_sim_t* s, double* tile_ms, uint64_t* bytes_written, uint64_t* bytes_uploaded) {
    if (!s || s->device < 0) { set_error("dbtk_sim_times: null or unattached handle"); return DBTK_ERR_ARG; }
    DEVCHK(hipSetDevice(s->device));
    const dbtk_status_t st = sim_take_times(s, true);
    if (st) return st;
    if (tile_ms) *tile_ms = s->tile_ms;
    if (bytes_written) *bytes_written = s->bytes_written;
    if (bytes_uploaded) *bytes_uploaded = s->bytes_uploaded;
    return DBTK_OK;
}

}  // extern "C"
