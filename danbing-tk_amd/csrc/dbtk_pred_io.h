// dbtk_pred_io.h — the output files of the `danbing-tk-pred` step (src/pred.h:236-258 of the reference) and of the dosage tables, shared by the two command
// lines that write them: danbing-tk-pred (dbtk_pred_cli.cpp) and `danbing-tk --cohort ... --pred` (dbtk_cli.cpp).  Host only.
// Both return false (with *err set) instead of ending the process: the callers end differently.
#ifndef DBTK_PRED_IO_H_
#define DBTK_PRED_IO_H_

#include <stdint.h>
#include <stdio.h>

#include <string>

namespace dbtk_pred_io {

// save_matrix (pred.h:236-249): the low 4 bytes of rows and columns, then the column-major float32 data.  `log`: where the
// reference's two progress lines go (its stdout).
inline bool save_matrix(const std::string& fn, const float* d, uint64_t nrow, uint64_t ncol, FILE* log, std::string* err) {
    fprintf(log, "saving matrix to %s\n", fn.c_str());
    FILE* f = fopen(fn.c_str(), "wb");
    if (!f) { *err = "cannot create " + fn; return false; }
    const uint32_t r = (uint32_t)nrow, c = (uint32_t)ncol;
    const bool ok = fwrite(&r, 4, 1, f) == 1 && fwrite(&c, 4, 1, f) == 1 && fwrite(d, 4, nrow * ncol, f) == nrow * ncol;
    if (fclose(f) || !ok) { *err = "write error on " + fn; return false; }
    fprintf(log, "matrix dim: (%llu,%llu) size: %llu bytes\n", (unsigned long long)nrow, (unsigned long long)ncol, (unsigned long long)(nrow * ncol * 4));
    return true;
}

// save_matrix with the tsv format (pred.cpp:51, pred.h:251-258): rows = samples, tab-separated, default stream precision, no final
// newline.  bias is ns x ntr column-major (Bias(s, tri) at tri * ns + s), as dbtk_pred_bias hands it out.
inline bool save_bias_tsv(const std::string& fn, const float* bias, uint64_t ns, uint64_t ntr, FILE* log, std::string* err) {
    fprintf(log, "saving matrix to %s\n", fn.c_str());
    FILE* f = fopen(fn.c_str(), "w");
    if (!f) { *err = "cannot create " + fn; return false; }
    std::string line;
    char num[64];
    bool ok = true;
    for (uint64_t s = 0; s < ns; ++s) {
        line.clear();
        for (uint64_t t = 0; t < ntr; ++t) {
            snprintf(num, sizeof num, "%g", (double)bias[t * ns + s]);
            if (t) line += '\t';
            line += num;
        }
        if (s + 1 < ns) line += '\n';
        ok = fwrite(line.data(), 1, line.size(), f) == line.size() && ok;
    }
    if (fclose(f) || !ok) { *err = "write error on " + fn; return false; }
    return true;
}

// a .kms table in the layout of the reference's `ktools sum -f` (kmertools.cpp:92-106): a row per sample, the loci tab-separated, every
// row ended by a newline.  kms is ns x ntr column-major (entry (s, tri) at tri * ns + s), as dbtk_dosage_kms hands it out.
inline bool save_kms(const std::string& fn, const uint64_t* kms, uint64_t ns, uint64_t ntr, FILE* log, std::string* err) {
    fprintf(log, "saving kms table to %s\n", fn.c_str());
    FILE* f = fopen(fn.c_str(), "w");
    if (!f) { *err = "cannot create " + fn; return false; }
    std::string line;
    bool ok = true;
    for (uint64_t s = 0; s < ns; ++s) {
        line.clear();
        for (uint64_t t = 0; t < ntr; ++t) { line += std::to_string(kms[t * ns + s]); line += t + 1 < ntr ? '\t' : '\n'; }
        ok = fwrite(line.data(), 1, line.size(), f) == line.size() && ok;
    }
    if (fclose(f) || !ok) { *err = "write error on " + fn; return false; }
    return true;
}

}  // namespace dbtk_pred_io
#endif
