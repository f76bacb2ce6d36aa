// dbtk_ktools.cpp — the ktools subcommands this repository provides (host only):
//   serialize PREF                    over the C-ABI (include/dbtk.h: dbtk_rpgg_serialize), the index producer of the align path
//   ksi  <pan.tr.kmers>               the cumulative k-mer count of every locus, one per line: the index of `sum`
//   sum  [-f] <.ksi> <in> <out.kms>   per-locus sums of one count file, or of every count file a list names (row = sample)
// Same usage texts, exit statuses and output bytes as the reference's tool for these subcommands (src/kmertools.cpp:38-137 and
// 221-345) on well-formed input; the others are not part of this repository.  Where the reference reads past the end of its index
// (a single-locus .ksi, a leading empty locus, a count file of another length) this tool is defined: see the usage texts.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
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

}  // namespace

int main(int argc, char* argv[]) {
    if (argc < 2) {
        fprintf(stderr, "Usage: ktools <commands> [options]\n\nCommands:\n"
                        "  ksi           generate ksi index for ktools sum\n"
                        "  sum           acculumate kmer counts for each locus\n"
                        "  serialize     generate kmer index using pan.(graph|ntr|tr).kmers\n\n"
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
    fprintf(stderr, "ktools: unknown command '%s' (ksi, sum and serialize are provided here)\n", argv[1]);
    return 1;
}
