// danbing-tk-pred, the command line (host C++ over include/dbtk_pred.h): same arguments, same three output files as the
// reference's src/pred.cpp:14-84.  The cohort's count vectors go to the GPU a few samples at a time; the matrix stays in HBM.
//   danbing-tk-pred <INPUT1: trkmc.ar files + read depths> <INPUT2: ikmer.meta> <OUTPUT1: raw matrix> <OUTPUT2: corrected> <OUTPUT3: bias.tsv>
//   danbing-tk-pred --dosage <OUT.dosage.tsv> [--kms <OUT.kms>] <INPUT1> <INPUT2> <OUTPUT3: bias.tsv>
// The second form makes the per-locus tables alone (dbtk_dosage_*): the matrix is never allocated, in HBM or on the host.
//   danbing-tk-pred --window-rows R | --window-bytes N <INPUT1> <INPUT2> <OUTPUT1> <OUTPUT2> <OUTPUT3>
// The first form for a cohort whose matrix fits neither: whole loci of at most R k-mers at a time (windowed()), the same three files.
//   danbing-tk-pred --assoc PHENO.tsv OUTPREF [--assoc-covar COVAR.tsv] [--assoc-pairs PAIRS.tsv] [--assoc-p X] [--assoc-raw] [--assoc-perm B [--assoc-seed S]] ... <either of the first two forms>
// The association scan of the resident matrix or dosage table (dbtk_assoc_cli.h); the other outputs are unchanged by it.
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../include/dbtk_pred.h"
#include "dbtk_assoc_cli.h"
#include "dbtk_pred_io.h"

static void die(const std::string& m, int code = 1) { fprintf(stderr, "%s\n", m.c_str()); exit(code); }

// the two file layouts live in dbtk_pred_io.h (shared with `danbing-tk --cohort --pred`); a failure ends the process here
static void save_matrix(const std::string& fn, const float* d, uint64_t nrow, uint64_t ncol) {
    std::string err;
    if (!dbtk_pred_io::save_matrix(fn, d, nrow, ncol, stdout, &err)) die(err);
}

// read_gt_meta (pred.h:41-49): name <tab> read depth per line
static void read_gt_meta(const std::string& fn, std::vector<std::string>* fns, std::vector<float>* rds) {
    std::ifstream fin(fn);
    if (!fin) die("cannot open " + fn);
    std::string f1, f2;
    while (std::getline(fin, f1, '\t') && std::getline(fin, f2)) { fns->push_back(f1); rds->push_back(std::stof(f2)); }
    if (fns->empty()) die(fn + ": no samples");
}
// load_eachBinGT (pred.h:166-186), one file: 8 bytes (nk) | 8 * nk bytes (counts).  The file, open behind a header of this RPGG build
static FILE* check_nk_header(const std::string& fn, uint64_t nk) {
    FILE* f = fopen(fn.c_str(), "rb");
    if (!f) die("cannot open " + fn, 134);
    uint64_t nkf = 0;
    if (fread(&nkf, 8, 1, f) != 1 || nkf != nk) { fprintf(stderr, "nk %llu != nk_ %llu\n", (unsigned long long)nkf, (unsigned long long)nk); exit(134); }  // the reference asserts
    return f;
}
static void read_counts(const std::string& fn, uint64_t nk, uint64_t* out) {
    FILE* f = check_nk_header(fn, nk);
    if (fread(out, 8, nk, f) != nk) die("truncated " + fn, 134);
    fclose(f);
}
// the cohort's count files to the GPU, 16 samples per transfer: load(first sample, n, their counts, their depths) hands a batch to the handle
template <class Load>
static void load_batches(const std::vector<std::string>& fns, const std::vector<float>& rds, uint64_t nk, Load load) {
    const uint64_t B = 16, ns = fns.size();
    std::vector<uint64_t> buf(B * nk);
    for (uint64_t s0 = 0; s0 < ns; s0 += B) {
        const uint64_t n = std::min<uint64_t>(B, ns - s0);
        for (uint64_t i = 0; i < n; ++i) read_counts(fns[s0 + i], nk, buf.data() + i * nk);
        if (load(s0, n, buf.data(), rds.data() + s0)) die(dbtk_last_error());
    }
}

// --dosage: the count files go to the GPU like below, but into the per-locus tables
static int dosage_tables(int device, const std::string& finGtMeta, const std::string& finIkMeta, const std::string& foutBias, const std::string& foutDosage,
                         const std::string& foutKms, dbtk_assoc_cli::Options& assoc) {
    printf("metadata of *.trkmc.ar: %s\ninvariant kmers: %s\ndosage table will be written to: %s\nbias matrix will be written to: %s\n",
           finGtMeta.c_str(), finIkMeta.c_str(), foutDosage.c_str(), foutBias.c_str());
    std::vector<std::string> fns;
    std::vector<float> rds;
    read_gt_meta(finGtMeta, &fns, &rds);
    const uint64_t ns = fns.size();
    dbtk_dosage_t* D = nullptr;
    if (dbtk_dosage_create_from_file(device, ns, finIkMeta.c_str(), &D)) die(dbtk_last_error());
    const uint64_t nk = dbtk_dosage_nk(D), ntr = dbtk_dosage_ntr(D);
    printf("%llu loci in total.\nreading %llu gt files\n", (unsigned long long)ntr, (unsigned long long)ns);
    float load_ms = 0, ms[2];
    load_batches(fns, rds, nk, [&](uint64_t s0, uint64_t n, const uint64_t* counts, const float* depths) {
        const dbtk_status_t st = dbtk_dosage_load_samples(D, s0, n, counts, depths);
        dbtk_dosage_times(D, ms);
        load_ms += ms[0];
        return st;
    });
    if (dbtk_dosage_finish(D)) die(dbtk_last_error());
    dbtk_dosage_times(D, ms);
    printf("finished in %.3f ms on the GPU (per-locus sums and raw bias %.3f, bias normalisation %.3f)\n", load_ms + ms[1], load_ms, ms[1]);
    std::vector<float> tab(ns * ntr);
    std::string err;
    if (dbtk_dosage_values(D, tab.data())) die(dbtk_last_error());
    if (!dbtk_pred_io::save_bias_tsv(foutDosage, tab.data(), ns, ntr, stdout, &err)) die(err);
    if (dbtk_dosage_bias(D, tab.data())) die(dbtk_last_error());
    if (!dbtk_pred_io::save_bias_tsv(foutBias, tab.data(), ns, ntr, stdout, &err)) die(err);
    if (!foutKms.empty()) {
        std::vector<uint64_t> kms(ns * ntr);
        if (dbtk_dosage_kms(D, kms.data())) die(dbtk_last_error());
        if (!dbtk_pred_io::save_kms(foutKms, kms.data(), ns, ntr, stdout, &err)) die(err);
    }
    if (!dbtk_assoc_cli::run(&assoc, false, device, ns, ntr, [&](dbtk_assoc_t* h, double p, bool perm) { return perm ? dbtk_assoc_perm_scan_dosage(h, D, p) : dbtk_assoc_scan_dosage(h, D, p); }, stdout, &err)) die(err);
    dbtk_dosage_free(D);
    return 0;
}

// --window-rows / --window-bytes: the two matrices one window of loci at a time.  Every window reads its slice of every sample's
// count file (pread), sends it a few samples at a time through the handle's pinned staging buffer, and appends the window of the raw
// and of the corrected matrix to the two files, whose headers were written first.  While window w computes and copies, the slices of
// window w + 1 are read and sent.  Host memory: the handle's pinned buffers (one pair of output windows, four samples' slices).
static int windowed(int device, const std::string& finGtMeta, const std::string& finIkMeta, const std::string& foutRaw, const std::string& fout,
                    const std::string& foutBias, const std::vector<std::string>& fns, const std::vector<float>& rds, uint64_t max_rows) {
    const uint64_t ns = fns.size();
    dbtk_pred_t* P = nullptr;
    if (dbtk_pred_create_windowed_from_file(device, ns, finIkMeta.c_str(), max_rows, &P)) die(dbtk_last_error());
    const uint64_t nk = dbtk_pred_nk(P), ntr = dbtk_pred_ntr(P);
    printf("%llu loci in total.\n", (unsigned long long)ntr);
    printf("reading %llu gt files in windows of at most %llu k-mers\n", (unsigned long long)ns, (unsigned long long)dbtk_pred_max_rows(P));
    for (uint64_t s = 0; s < ns; ++s) fclose(check_nk_header(fns[s], nk));  // load_eachBinGT's assertion, once per file and before anything is written
    FILE* fo[2] = {fopen(foutRaw.c_str(), "wb"), fopen(fout.c_str(), "wb")};
    const std::string* fon[2] = {&foutRaw, &fout};
    for (int i = 0; i < 2; ++i) {
        if (!fo[i]) die("cannot create " + *fon[i]);
        const uint32_t r = (uint32_t)ns, c = (uint32_t)nk;  // save_matrix' header, with the full dimensions
        if (fwrite(&r, 4, 1, fo[i]) != 1 || fwrite(&c, 4, 1, fo[i]) != 1) die("write error on " + *fon[i]);
    }
    uint64_t* stage = nullptr;
    uint64_t B = 0;
    if (dbtk_pred_window_stage(P, &stage, &B)) die(dbtk_last_error());
    auto take = [&] {  // the submitted window's two pieces, appended
        const float* out[2] = {nullptr, nullptr};
        uint64_t rows = 0;
        if (dbtk_pred_window_outputs_pinned(P, &out[0], &out[1], &rows)) die(dbtk_last_error());
        for (int i = 0; i < 2; ++i) if (rows && fwrite(out[i], 4, rows * ns, fo[i]) != rows * ns) die("write error on " + *fon[i]);
    };
    uint64_t nwin = 0;
    for (uint64_t first = 0, end = 0; first < ntr; first = end, ++nwin) {
        uint64_t row0 = 0, rows = 0;
        if (dbtk_pred_window(P, first, &end, &row0, &rows)) die(dbtk_last_error());
        for (uint64_t s0 = 0; s0 < ns && rows; s0 += B) {
            const uint64_t n = std::min<uint64_t>(B, ns - s0);
            for (uint64_t i = 0; i < n; ++i) {
                const std::string& fn = fns[s0 + i];
                const int fd = open(fn.c_str(), O_RDONLY);
                if (fd < 0) die("cannot open " + fn, 134);
                char* dst = (char*)(stage + i * rows);
                for (uint64_t got = 0; got < rows * 8;) {
                    const ssize_t k = pread(fd, dst + got, rows * 8 - got, (off_t)(8 + row0 * 8 + got));
                    if (k <= 0) die("truncated " + fn, 134);
                    got += (uint64_t)k;
                }
                close(fd);
            }
            if (dbtk_pred_load_samples(P, s0, n, stage, rds.data() + s0)) die(dbtk_last_error());
        }
        if (nwin) take();  // (window nwin - 1: it ran while this one's slices were read and sent)
        if (dbtk_pred_window_submit(P)) die(dbtk_last_error());
    }
    take();
    printf("normalizaing read depth\ncomputing/correcting bias\n%llu windows\n", (unsigned long long)nwin);
    for (int i = 0; i < 2; ++i) {
        printf("saving matrix to %s\n", fon[i]->c_str());
        if (fclose(fo[i])) die("write error on " + *fon[i]);
        printf("matrix dim: (%llu,%llu) size: %llu bytes\n", (unsigned long long)ns, (unsigned long long)nk, (unsigned long long)(ns * nk * 4));
    }
    std::vector<float> bias(ns * ntr);
    if (dbtk_pred_bias(P, bias.data())) die(dbtk_last_error());
    std::string err;
    if (!dbtk_pred_io::save_bias_tsv(foutBias, bias.data(), ns, ntr, stdout, &err)) die(err);
    dbtk_pred_free(P);
    return 0;
}

// a positive integer, all of the argument
static uint64_t positive(const std::string& flag, const char* v) {
    char* e = nullptr;
    const unsigned long long x = strtoull(v, &e, 10);
    if (!*v || *v == '-' || *e) die(flag + ": not a number: " + v);
    if (!x) die(flag + " must be positive");
    return x;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "\nUsage: danbing-tk-pred <INPUT1> <INPUT2> <OUTPUT1> <OUTPUT2> <OUTPUT3>\n"
                        "INPUT1      metadata of *.trkmc.ar files, consisting of 2 columns.\n"
                        " col1       *.trkmc.ar file name\n"
                        " col2       read depth\n"
                        "INPUT2      invariant kmers of an RPGG build\n"
                        "OUTPUT1     raw genotype matrix. Row: sample. Column: kmer.\n"
                        "OUTPUT2     bias-corrected genotype matrix. Row: sample. Column: kmer.\n"
                        "OUTPUT3     bias matrix. Row: sample. Column: TR locus.\n"
                        "MI355X build:\n"
                        "  --device <INT>  GPU to use [0]\n"
                        "  --dosage <OUT.dosage.tsv> [--kms <OUT.kms>] <INPUT1> <INPUT2> <OUTPUT3>\n"
                        "                  per-locus tables only, without the two matrices: the bias-corrected dosage\n"
                        "                  (sum of the locus' k-mer counts / read depth / bias; uncorrected where the locus has\n"
                        "                  no invariant k-mers) in the layout of OUTPUT3, and the plain sums as `ktools sum -f` writes them\n"
                        "  --window-rows <INT>   the two matrices one window of whole loci at a time, at most INT k-mers each: the same\n"
                        "                  three files from O(window) of device and host memory (no locus may have more k-mers)\n"
                        "  --window-bytes <INT>  the same, as the size of a window's device matrix: INT / (4 * samples) k-mers\n%s\n", dbtk_assoc_cli::usage());
        return 0;
    }
    int argi = 1, device = 0;
    std::string foutDosage, foutKms;
    uint64_t winRows = 0, winBytes = 0;
    dbtk_assoc_cli::Options assoc;
    while (argi < argc && argv[argi][0] == '-') {
        const std::string a = argv[argi];
        {
            std::string err;
            const int used = dbtk_assoc_cli::take_flag(&assoc, argc, argv, argi, &err);
            if (used < 0) die(err);
            if (used) { argi += used; continue; }
        }
        if (a == "--device" && argi + 1 < argc) { device = atoi(argv[argi + 1]); argi += 2; }
        else if (a == "--dosage" && argi + 1 < argc) { foutDosage = argv[argi + 1]; argi += 2; }
        else if (a == "--kms" && argi + 1 < argc) { foutKms = argv[argi + 1]; argi += 2; }
        else if (a == "--window-rows" && argi + 1 < argc) { winRows = positive(a, argv[argi + 1]); argi += 2; }
        else if (a == "--window-bytes" && argi + 1 < argc) { winBytes = positive(a, argv[argi + 1]); argi += 2; }
        else if (a == "-f" && argi + 1 < argc) argi += 2;  // developer flag of the reference (its body is commented out there): accepted, ignored
        else die("invalid option: " + a);
    }
    if (!foutKms.empty() && foutDosage.empty()) die("--kms needs --dosage");
    if (assoc.any()) {  // everything of --assoc that can be refused before a device is touched
        if (winRows || winBytes) die("--assoc: not with --window-rows / --window-bytes: a window holds a part of the rows, and the best row of a phenotype across windows is not made yet");
        std::string err;
        if (!dbtk_assoc_cli::load(&assoc, !foutDosage.empty(), &err)) die(err);
    }
    if (!foutDosage.empty()) {
        if (argc - argi != 3) die("--dosage: expected 3 file arguments (INPUT1 INPUT2 OUTPUT3)");
        return dosage_tables(device, argv[argi], argv[argi + 1], argv[argi + 2], foutDosage, foutKms, assoc);
    }
    if (argc - argi < 5) die("expected 5 file arguments");
    const std::string finGtMeta = argv[argi], finIkMeta = argv[argi + 1], foutRaw = argv[argi + 2], fout = argv[argi + 3], foutBias = argv[argi + 4];
    printf("metadata of *.trkmc.ar: %s\ninvariant kmers: %s\nraw genotype matrix will be written to: %s\n"
           "bias-corrected genotype matrix will be written to: %s\nbias matrix will be written to: %s\n",
           finGtMeta.c_str(), finIkMeta.c_str(), foutRaw.c_str(), fout.c_str(), foutBias.c_str());
    std::vector<std::string> fns;
    std::vector<float> rds;
    read_gt_meta(finGtMeta, &fns, &rds);
    const uint64_t ns = fns.size();
    if (winRows || winBytes) {
        const uint64_t fromBytes = winBytes / (4 * ns);
        if (winBytes && !fromBytes) die("--window-bytes " + std::to_string(winBytes) + " holds no k-mer of " + std::to_string(ns) + " samples");
        if (winRows && winBytes && winRows != fromBytes)
            die("--window-rows " + std::to_string(winRows) + " and --window-bytes " + std::to_string(winBytes) + " (" + std::to_string(fromBytes) + " k-mers of " + std::to_string(ns) + " samples) disagree");
        return windowed(device, finGtMeta, finIkMeta, foutRaw, fout, foutBias, fns, rds, winRows ? winRows : fromBytes);
    }
    dbtk_pred_t* P = nullptr;
    if (dbtk_pred_create_from_file(device, ns, finIkMeta.c_str(), &P)) die(dbtk_last_error());
    const uint64_t nk = dbtk_pred_nk(P), ntr = dbtk_pred_ntr(P);
    printf("%llu loci in total.\n", (unsigned long long)ntr);
    printf("reading %llu gt files\n", (unsigned long long)ns);
    load_batches(fns, rds, nk, [&](uint64_t s0, uint64_t n, const uint64_t* counts, const float* depths) { return dbtk_pred_load_samples(P, s0, n, counts, depths); });
    std::vector<float> mat(ns * nk);
    printf("normalizaing read depth\n");
    if (dbtk_pred_matrix(P, mat.data())) die(dbtk_last_error());
    save_matrix(foutRaw, mat.data(), ns, nk);
    auto scan = [&](dbtk_assoc_t* h, double p, bool perm) { return perm ? dbtk_assoc_perm_scan_pred(h, P, p) : dbtk_assoc_scan_pred(h, P, p); };
    {
        std::string err;
        if (!dbtk_assoc_cli::run(&assoc, true, device, ns, ntr, scan, stdout, &err)) die(err);
    }
    printf("computing/correcting bias\n");
    if (dbtk_pred_correct(P)) die(dbtk_last_error());
    float ms[3];
    dbtk_pred_times(P, ms);
    printf("finished in %.3f ms on the GPU (bias sums %.3f, bias normalisation %.3f, correction %.3f)\n", ms[0] + ms[1] + ms[2], ms[0], ms[1], ms[2]);
    if (dbtk_pred_matrix(P, mat.data())) die(dbtk_last_error());
    save_matrix(fout, mat.data(), ns, nk);
    std::vector<float> bias(ns * ntr);
    if (dbtk_pred_bias(P, bias.data())) die(dbtk_last_error());
    {
        std::string err;
        if (!dbtk_pred_io::save_bias_tsv(foutBias, bias.data(), ns, ntr, stdout, &err)) die(err);
        if (!dbtk_assoc_cli::run(&assoc, false, device, ns, ntr, scan, stdout, &err)) die(err);
    }
    dbtk_pred_free(P);
    return 0;
}
