// dbtk_ktools.cpp — the ktools subcommands this repository provides (host only):
//   serialize PREF                    over the C-ABI (include/dbtk.h: dbtk_rpgg_serialize), the index producer of the align path
//   ksi  <pan.tr.kmers>               the cumulative k-mer count of every locus, one per line: the index of `sum`
//   sum  [-f] <.ksi> <in> <out.kms>   per-locus sums of one count file, or of every count file a list names (row = sample)
//   fps  NLOCI K OUT FP_PF TP_PF...   the FP-specific k-mers of `danbing-tk --bait-profile` profiles: what the reference's `baitBuilder v2`
//                                     does (src/bait.cpp:177-241, 254-305), the lines of a locus in ascending order of the k-mer
//   serialize-bt BAIT NLOCI OUTPREF   OUTPREF.bt.kmdb from that text, byte for byte the reference's (src/kmertools.cpp:346-371)
// Same usage texts, exit statuses and output bytes as the reference's tool for these subcommands (src/kmertools.cpp:38-137 and
// 221-345) on well-formed input; the others are not part of this repository.  Where the reference reads past the end of its index
// (a single-locus .ksi, a leading empty locus, a count file of another length) this tool is defined: see the usage texts.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dbtk.h"

namespace {

const int EXIT_ASSERT = 134;  // the reference asserts on files it cannot open

// a whole text file, line by line, without the final newline of a line
struct Lines {
    std::string text;
    size_t at = 0;
    bool open(const char* fn) {
        FILE* f = fopen(fn, "rb");
        if (!f) return false;
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
        fclose(f);
        return true;
    }
    bool next(const char** b, size_t* len) {
        if (at >= text.size()) return false;
        const char* e = (const char*)memchr(text.data() + at, '\n', text.size() - at);
        const size_t stop = e ? (size_t)(e - text.data()) : text.size();
        *b = text.data() + at; *len = stop - at;
        at = stop + 1;
        return true;
    }
};

// an unsigned decimal number, alone on its line (stoul's reading: blanks may lead, anything may trail a digit run)
bool number(const char* b, size_t len, uint64_t* v) {
    const std::string s(b, len);
    char* endp = nullptr;
    errno = 0;
    *v = strtoull(s.c_str(), &endp, 10);
    return endp != s.c_str() && !errno;
}

int fail(const std::string& m, int code = 1) { fprintf(stderr, "ktools: %s\n", m.c_str()); return code; }

// ---- ksi: a '>' line opens a locus, every other line is one of its k-mers
int cmd_ksi(const char* kmers) {
    Lines in;
    if (!in.open(kmers)) return fail(std::string("cannot open ") + kmers, EXIT_ASSERT);
    std::vector<uint64_t> cum;  // per locus opened so far: k-mer lines up to its end
    uint64_t n = 0;
    const char* b; size_t len;
    while (in.next(&b, &len)) {
        if (len && b[0] == '>') { if (!cum.empty()) cum.back() = n; cum.push_back(n); }
        else ++n;
    }
    if (!cum.empty()) cum.back() = n;
    std::string out;
    for (uint64_t c : cum) out += std::to_string(c) + '\n';
    if (fwrite(out.data(), 1, out.size(), stdout) != out.size() || fflush(stdout)) return fail("write to stdout failed");
    return 0;
}

// ---- sum
bool read_ksi(const char* fn, std::vector<uint64_t>* ksi, int* code) {
    Lines in;
    if (!in.open(fn)) { *code = fail(std::string("cannot open ") + fn, EXIT_ASSERT); return false; }
    const char* b; size_t len;
    while (in.next(&b, &len)) {
        uint64_t v;
        if (!number(b, len, &v)) { *code = fail(std::string(fn) + ": line " + std::to_string(ksi->size() + 1) + " is not a number"); return false; }
        if (!ksi->empty() && v < ksi->back()) { *code = fail(std::string(fn) + ": line " + std::to_string(ksi->size() + 1) + ": the cumulative counts must not decrease"); return false; }
        ksi->push_back(v);
    }
    fprintf(stderr, "%zu loci in %s\n", ksi->size(), fn);
    if (ksi->empty()) { *code = fail(std::string(fn) + " names no locus"); return false; }
    return true;
}

// the per-locus sums of one count file (one count per line, ksi.back() lines); modulo 2^64 like the reference's size_t
bool locus_sums(const char* fn, const std::vector<uint64_t>& ksi, std::vector<uint64_t>* sums, int* code) {
    Lines in;
    if (!in.open(fn)) { *code = fail(std::string("cannot open ") + fn, EXIT_ASSERT); return false; }
    sums->assign(ksi.size(), 0);
    uint64_t ki = 0;
    size_t l = 0;
    bool more = false;
    const char* b; size_t len;
    while (in.next(&b, &len)) {
        uint64_t v;
        if (!number(b, len, &v)) { *code = fail(std::string(fn) + ": line " + std::to_string(ki + 1) + " is not a count"); return false; }
        while (l < ksi.size() && ksi[l] <= ki) ++l;  // (empty loci are passed over: their sum stays 0)
        if (l == ksi.size()) { more = true; break; }
        (*sums)[l] += v;
        ++ki;
    }
    if (ki != ksi.back() || more) {
        *code = fail(std::string(fn) + ": the index expects " + std::to_string(ksi.back()) + " counts, the file holds " + (more ? "more" : std::to_string(ki)));
        return false;
    }
    return true;
}

int cmd_sum(int argc, char** argv) {
    const bool many = !strcmp(argv[2], "-f");
    if (argc < (many ? 6 : 5)) return fail("sum: expected [-f] <.ksi> <input> <out.kms>");
    const char *ksif = argv[many ? 3 : 2], *inf = argv[many ? 4 : 3], *outf = argv[many ? 5 : 4];
    std::vector<uint64_t> ksi, sums;
    int code = 0;
    if (!read_ksi(ksif, &ksi, &code)) return code;
    std::vector<std::string> files;
    if (many) {
        Lines fofn;
        if (!fofn.open(inf)) return fail(std::string("cannot open ") + inf, EXIT_ASSERT);
        const char* b; size_t len;
        while (fofn.next(&b, &len)) files.emplace_back(b, len);
        fprintf(stderr, "%zu samples in %s\n", files.size(), inf);
    } else files.push_back(inf);
    FILE* out = fopen(outf, "wb");
    if (!out) return fail(std::string("cannot create ") + outf, EXIT_ASSERT);
    const char sep = many ? '\t' : '\n';  // -f: a row per sample; without: a line per locus
    for (const std::string& fn : files) {
        if (!locus_sums(fn.c_str(), ksi, &sums, &code)) { fclose(out); (void)remove(outf); return code; }
        std::string row;
        for (size_t l = 0; l < sums.size(); ++l) { row += std::to_string(sums[l]); row += l + 1 < sums.size() ? sep : '\n'; }
        if (fwrite(row.data(), 1, row.size(), out) != row.size()) { fclose(out); return fail(std::string("write error on ") + outf); }
    }
    if (fclose(out)) return fail(std::string("write error on ") + outf);
    if (many) fprintf(stderr, "%llu kmers processed in each file\n", (unsigned long long)ksi.back());
    else fprintf(stderr, "%zu loci and %llu kmers processed in %s\n", ksi.size(), (unsigned long long)ksi.back(), inf);
    return 0;
}

// ---- fps: baitBuilder v2.  The FP profile is read locus by locus; every TP profile is read forward to that locus and tested in
// turn.  An FP k-mer that a TP profile holds is dropped when its FP mean lies inside that profile's mean +- 2 sd (float arithmetic,
// as the reference parses and compares); otherwise its (min, max) — 255, 0 until then — widens by that profile's.
struct FpStat { uint8_t mi, ma; float mn; };
struct TpStat { uint8_t mi, ma; float mn, sd; };
struct TpFile { std::ifstream f; uint64_t tri; };

bool locus_of(const std::string& line, uint64_t* tri) { return number(line.c_str() + 1, line.size() - 1, tri); }

// KMER MIN MAX MEAN SD
bool profile_line(const std::string& line, uint64_t* km, uint64_t* mi, uint64_t* ma, float* mn, float* sd) {
    const char* p = line.c_str();
    char* e = nullptr;
    errno = 0;
    *km = strtoull(p, &e, 10); if (e == p) return false; p = e;
    *mi = strtoull(p, &e, 10); if (e == p) return false; p = e;
    *ma = strtoull(p, &e, 10); if (e == p) return false; p = e;
    *mn = strtof(p, &e); if (e == p) return false; p = e;
    *sd = strtof(p, &e); if (e == p) return false;
    return !errno || errno == ERANGE;
}

int cmd_fps(int argc, char** argv) {
    if (argc < 7) return fail("fps: expected <nloci> <ksize> <out> <FP_pf> <TP_pf> [<TP_pf> ...]");
    uint64_t nloci = 0;
    if (!number(argv[2], strlen(argv[2]), &nloci) || !nloci) return fail("fps: <nloci> must be a positive number");
    std::ifstream fp(argv[5]);
    if (!fp) return fail(std::string("cannot open ") + argv[5], EXIT_ASSERT);
    std::vector<TpFile> tps(argc - 6);
    std::string line;
    for (int i = 6; i < argc; ++i) {
        TpFile& t = tps[i - 6];
        t.f.open(argv[i]);
        if (!t.f) return fail(std::string("cannot open ") + argv[i], EXIT_ASSERT);
        t.tri = nloci;  // (an empty profile: at its end from the start)
        if (std::getline(t.f, line) && !line.empty()) {
            if (line[0] != '>' || !locus_of(line, &t.tri)) return fail(std::string(argv[i]) + ": the first line is not >LOCUS");
        }
    }
    FILE* out = fopen(argv[4], "wb");
    if (!out) return fail(std::string("cannot create ") + argv[4], EXIT_ASSERT);
    std::unordered_map<uint64_t, FpStat> k2s;
    std::string err;
    // the FP k-mers of locus tri against every TP profile in turn, then the survivors
    auto finish_locus = [&](uint64_t tri) {
        for (size_t fi = 0; fi < tps.size() && err.empty(); ++fi) {
            TpFile& t = tps[fi];
            while (t.tri < tri) {  // skipUntil
                if (!std::getline(t.f, line) || line.empty()) t.tri = nloci;
                else if (line[0] == '>' && !locus_of(line, &t.tri)) err = std::string(argv[6 + fi]) + ": not a locus: " + line;
            }
            if (t.tri != tri) continue;
            std::unordered_map<uint64_t, TpStat> tp;  // readLocusProfile: the locus' lines of this profile that name an FP k-mer
            t.tri = nloci;
            while (std::getline(t.f, line) && !line.empty()) {
                if (line[0] == '>') { if (!locus_of(line, &t.tri)) err = std::string(argv[6 + fi]) + ": not a locus: " + line; break; }
                uint64_t km, mi, ma; float mn, sd;
                if (!profile_line(line, &km, &mi, &ma, &mn, &sd)) { err = std::string(argv[6 + fi]) + ": not a profile line: " + line; break; }
                if (k2s.count(km)) tp[km] = TpStat{(uint8_t)mi, (uint8_t)ma, mn, sd};
            }
            for (const auto& p : tp) {  // testAndFilter
                const TpStat& T = p.second;
                FpStat& F = k2s[p.first];
                const float fsd = 2.0f * T.sd;
                if (T.mn - fsd <= F.mn && F.mn <= T.mn + fsd) { k2s.erase(p.first); continue; }
                if (F.mi != 255) { F.mi = std::min(T.mi, F.mi); F.ma = std::max(T.ma, F.ma); }
                else { F.mi = T.mi; F.ma = T.ma; }
            }
        }
        std::vector<std::pair<uint64_t, FpStat>> v(k2s.begin(), k2s.end());
        std::sort(v.begin(), v.end(), [](const std::pair<uint64_t, FpStat>& a, const std::pair<uint64_t, FpStat>& b) { return a.first < b.first; });
        std::string text = ">" + std::to_string(tri) + "\n";  // (written for a locus whose k-mers were all dropped too, as the reference does)
        for (const auto& p : v) text += std::to_string(p.first) + '\t' + std::to_string((int)p.second.mi) + '\t' + std::to_string((int)p.second.ma) + '\n';
        if (fwrite(text.data(), 1, text.size(), out) != text.size()) err = std::string("write error on ") + argv[4];
        k2s.clear();
    };
    bool any = false;
    uint64_t cur = 0, nr = 0;
    while (err.empty() && std::getline(fp, line)) {
        ++nr;
        if (line.empty()) continue;
        if (line[0] == '>') {
            uint64_t tri;
            if (!locus_of(line, &tri)) { err = std::string(argv[5]) + ": line " + std::to_string(nr) + " is not >LOCUS"; break; }
            if (any && tri <= cur) { err = std::string(argv[5]) + ": line " + std::to_string(nr) + ": the loci must ascend"; break; }
            if (!k2s.empty()) finish_locus(cur);
            cur = tri; any = true;
        } else {
            uint64_t km, mi, ma; float mn, sd;
            if (!any || !profile_line(line, &km, &mi, &ma, &mn, &sd)) { err = std::string(argv[5]) + ": line " + std::to_string(nr) + " is not a profile line of a locus"; break; }
            k2s[km] = FpStat{255, 0, mn};
        }
    }
    if (err.empty() && any) finish_locus(cur);
    if (fclose(out) && err.empty()) err = std::string("write error on ") + argv[4];
    if (!err.empty()) { (void)remove(argv[4]); return fail(err); }
    fprintf(stderr, "done\n");
    return 0;
}

// ---- serialize-bt: readFPSKmersV2 + flattenKmapDB + serializeKmapDB.  The order of a locus' k-mers in the file is the iteration
// order of the reference's std::unordered_map<uint64_t, uint16_t> filled in file order: the same container, filled the same way.
int cmd_serialize_bt(int argc, char** argv) {
    if (argc < 5) return fail("serialize-bt: expected <bait> <nloci> <outPref>");
    uint64_t nloci = 0;
    if (!number(argv[3], strlen(argv[3]), &nloci) || !nloci) return fail("serialize-bt: <nloci> must be a positive number");
    std::ifstream f(argv[2]);
    if (!f) return fail(std::string("cannot open ") + argv[2], EXIT_ASSERT);
    std::vector<std::unordered_map<uint64_t, uint16_t>> db(nloci);
    std::string line;
    uint64_t tri = nloci, nr = 0;
    while (std::getline(f, line)) {
        ++nr;
        if (line.empty()) continue;
        if (line[0] == '>') {
            if (!locus_of(line, &tri) || tri >= nloci) return fail(std::string(argv[2]) + ": line " + std::to_string(nr) + ": not a locus below " + std::to_string(nloci));
            continue;
        }
        const char* p = line.c_str();
        char* e = nullptr;
        const uint64_t km = strtoull(p, &e, 10); const bool ok0 = e != p; p = e;
        const uint64_t mi = strtoull(p, &e, 10); const bool ok1 = e != p; p = e;
        const uint64_t ma = strtoull(p, &e, 10); const bool ok2 = e != p;
        if (tri >= nloci || !ok0 || !ok1 || !ok2) return fail(std::string(argv[2]) + ": line " + std::to_string(nr) + " is not KMER<TAB>MIN<TAB>MAX of a locus");
        db[tri][km] = (uint16_t)((mi << 8) + ma);
    }
    std::vector<uint64_t> index(nloci), ks;
    std::vector<uint16_t> vs;
    for (uint64_t l = 0; l < nloci; ++l) {
        for (const auto& p : db[l]) { ks.push_back(p.first); vs.push_back(p.second); }
        index[l] = db[l].size();
    }
    const uint64_t nk = ks.size(), szv = sizeof(uint16_t);
    const std::string fn = std::string(argv[4]) + ".bt.kmdb";
    FILE* out = fopen(fn.c_str(), "wb");
    if (!out) return fail("cannot create " + fn, EXIT_ASSERT);
    bool ok = fwrite(&nloci, 8, 1, out) == 1 && fwrite(index.data(), 8, nloci, out) == nloci && fwrite(&nk, 8, 1, out) == 1 && fwrite(&szv, 8, 1, out) == 1;
    ok = ok && fwrite(ks.data(), 8, nk, out) == nk && fwrite(vs.data(), 2, nk, out) == nk;
    if (fclose(out) || !ok) return fail("write error on " + fn);
    fprintf(stderr, "%llu bait k-mers of %llu loci in %s\n", (unsigned long long)nk, (unsigned long long)nloci, fn.c_str());
    return 0;
}

}  // namespace

int main(int argc, char* argv[]) {
    if (argc < 2) {
        fprintf(stderr, "Usage: ktools <commands> [options]\n\nCommands:\n"
                        "  ksi           generate ksi index for ktools sum\n"
                        "  sum           acculumate kmer counts for each locus\n"
                        "  serialize     generate kmer index using pan.(graph|ntr|tr).kmers\n"
                        "  fps           FP-specific bait k-mers from the k-mer count profiles of danbing-tk --bait-profile\n"
                        "  serialize-bt  generate serialized bait.kmers\n\n"
                        "  (the reference's other commands are not provided here)\n");
        return 0;
    }
    const std::string cmd = argv[1];
    if (cmd == "ksi") {
        if (argc == 2) {
            fprintf(stderr, "Usage: ktools ksi <pan.tr.kmers> >$OUT.ksi  Generate ksi index for ktools sum\n"
                            "  One line per locus: the number of k-mer lines up to its end.  A file with a single locus gets its\n"
                            "  one line here (the reference prints nothing for it).\n");
            return 0;
        }
        return cmd_ksi(argv[2]);
    }
    if (cmd == "sum") {
        if (argc == 2) {
            fprintf(stderr, "Usage 1: ktools sum <.ksi> <.kmers> <out.kms>\n"
                            "  Read a single .kmers file and write a single column output.\n"
                            "Usage 2: ktools sum -f <.ksi> <.txt> <out.kms>\n"
                            "  Read all kmer files specified in .txt and output a kms table (row=sample, col=locus).\n"
                            "  A count file holds one count per line.  Here every locus of the .ksi gets its sum: a single-locus\n"
                            "  index and a leading empty locus (sum 0) too, where the reference reads past its index or writes\n"
                            "  nothing.  A count file with more or fewer lines than the index' last entry is refused (status 1).\n");
            return 0;
        }
        return cmd_sum(argc, argv);
    }
    if (cmd == "serialize") {
        if (argc == 2) {
            fprintf(stderr, "Usage: ktools serialize <pref>\n\n  PREF     prefix of *.(graph|fl|tr).kmers\n");
            return 0;
        }
        if (dbtk_rpgg_serialize(argv[2]) != DBTK_OK) {
            fprintf(stderr, "ktools: %s\n", dbtk_last_error());
            return 134;  // the reference asserts on unusable files
        }
        fprintf(stderr, "done\n");
        return 0;
    }
    if (cmd == "fps") {
        if (argc == 2) {
            fprintf(stderr, "Usage: ktools fps <nloci> <ksize> <out> <FP_pf> <TP_pf> [<TP_pf> ...]\n"
                            "  FP_pf / TP_pf  PREF.FP_pf.txt / PREF.TP_pf.txt of danbing-tk --bait-profile (loci ascending; one TP profile per genome)\n"
                            "  out            >locus, then kmer<TAB>c0<TAB>c1 for every FP k-mer whose FP mean lies outside mean +- 2 sd of every TP\n"
                            "                 profile that holds it; c0/c1: min/max count in those TP profiles, 255/0 when none holds it.\n"
                            "                 The lines of a locus ascend by k-mer (the reference's `baitBuilder v2` writes them in a hash map's order).\n");
            return 0;
        }
        return cmd_fps(argc, argv);
    }
    if (cmd == "serialize-bt") {
        if (argc == 2) {
            fprintf(stderr, "Usage: ktools serialize-bt <bait> <nloci> <outPref>\n\n"
                            "  bait     Path to bait kmers.\n"
                            "           File format (tab delimited):\n"
                            "             >locus_index\n"
                            "             kmer\tc0\tc1\n"
                            "           c0/c1: min/max observed kmer count in TP reads. If kmer not present in any TP read, c0/c1=255/0\n"
                            "  nloci    # of loci in RPGG\n"
                            "  outPref  output file name = $outPref.bt.kmdb\n\n");
            return 0;
        }
        return cmd_serialize_bt(argc, argv);
    }
    fprintf(stderr, "ktools: unknown command '%s' (ksi, sum, serialize, fps and serialize-bt are provided here)\n", argv[1]);
    return 1;
}
