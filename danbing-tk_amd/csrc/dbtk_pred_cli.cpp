// danbing-tk-pred, the command line (host C++ over include/dbtk_pred.h): same arguments, same three output files as the
// reference's src/pred.cpp:14-84.  The cohort's count vectors go to the GPU a few samples at a time; the matrix stays in HBM.
//   danbing-tk-pred <INPUT1: trkmc.ar files + read depths> <INPUT2: ikmer.meta> <OUTPUT1: raw matrix> <OUTPUT2: corrected> <OUTPUT3: bias.tsv>
//   danbing-tk-pred --dosage <OUT.dosage.tsv> [--kms <OUT.kms>] <INPUT1> <INPUT2> <OUTPUT3: bias.tsv>
// The second form makes the per-locus tables alone (dbtk_dosage_*): the matrix is never allocated, in HBM or on the host.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../include/dbtk_pred.h"
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
// load_eachBinGT (pred.h:166-186), one file: 8 bytes (nk) | 8 * nk bytes (counts)
static void read_counts(const std::string& fn, uint64_t nk, uint64_t* out) {
    FILE* f = fopen(fn.c_str(), "rb");
    if (!f) die("cannot open " + fn, 134);
    uint64_t nkf = 0;
    if (fread(&nkf, 8, 1, f) != 1 || nkf != nk) { fprintf(stderr, "nk %llu != nk_ %llu\n", (unsigned long long)nkf, (unsigned long long)nk); exit(134); }  // the reference asserts
    if (fread(out, 8, nk, f) != nk) die("truncated " + fn, 134);
    fclose(f);
}

// --dosage: the count files go to the GPU 16 samples at a time like below, but into the per-locus tables
static int dosage_tables(int device, const std::string& finGtMeta, const std::string& finIkMeta, const std::string& foutBias, const std::string& foutDosage,
                         const std::string& foutKms) {
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
    const uint64_t B = 16;
    std::vector<uint64_t> buf(B * nk);
    float load_ms = 0, ms[2];
    for (uint64_t s0 = 0; s0 < ns; s0 += B) {
        const uint64_t n = std::min<uint64_t>(B, ns - s0);
        for (uint64_t i = 0; i < n; ++i) read_counts(fns[s0 + i], nk, buf.data() + i * nk);
        if (dbtk_dosage_load_samples(D, s0, n, buf.data(), rds.data() + s0)) die(dbtk_last_error());
        dbtk_dosage_times(D, ms);
        load_ms += ms[0];
    }
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
    dbtk_dosage_free(D);
    return 0;
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
                        "                  no invariant k-mers) in the layout of OUTPUT3, and the plain sums as `ktools sum -f` writes them\n\n");
        return 0;
    }
    int argi = 1, device = 0;
    std::string foutDosage, foutKms;
    while (argi < argc && argv[argi][0] == '-') {
        const std::string a = argv[argi];
        if (a == "--device" && argi + 1 < argc) { device = atoi(argv[argi + 1]); argi += 2; }
        else if (a == "--dosage" && argi + 1 < argc) { foutDosage = argv[argi + 1]; argi += 2; }
        else if (a == "--kms" && argi + 1 < argc) { foutKms = argv[argi + 1]; argi += 2; }
        else if (a == "-f" && argi + 1 < argc) argi += 2;  // developer flag of the reference (its body is commented out there): accepted, ignored
        else die("invalid option: " + a);
    }
    if (!foutKms.empty() && foutDosage.empty()) die("--kms needs --dosage");
    if (!foutDosage.empty()) {
        if (argc - argi != 3) die("--dosage: expected 3 file arguments (INPUT1 INPUT2 OUTPUT3)");
        return dosage_tables(device, argv[argi], argv[argi + 1], argv[argi + 2], foutDosage, foutKms);
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
    dbtk_pred_t* P = nullptr;
    if (dbtk_pred_create_from_file(device, ns, finIkMeta.c_str(), &P)) die(dbtk_last_error());
    const uint64_t nk = dbtk_pred_nk(P), ntr = dbtk_pred_ntr(P);
    printf("%llu loci in total.\n", (unsigned long long)ntr);
    printf("reading %llu gt files\n", (unsigned long long)ns);
    const uint64_t B = 16;  // samples per transfer
    std::vector<uint64_t> buf(B * nk);
    for (uint64_t s0 = 0; s0 < ns; s0 += B) {
        const uint64_t n = std::min<uint64_t>(B, ns - s0);
        for (uint64_t i = 0; i < n; ++i) read_counts(fns[s0 + i], nk, buf.data() + i * nk);
        if (dbtk_pred_load_samples(P, s0, n, buf.data(), rds.data() + s0)) die(dbtk_last_error());
    }
    std::vector<float> mat(ns * nk);
    printf("normalizaing read depth\n");
    if (dbtk_pred_matrix(P, mat.data())) die(dbtk_last_error());
    save_matrix(foutRaw, mat.data(), ns, nk);
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
    }
    dbtk_pred_free(P);
    return 0;
}
