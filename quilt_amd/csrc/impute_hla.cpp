// impute_hla.cpp -- qa_impute_samples_hla (include/quilt_amd.h): hla_run = TRUE on the range call.  The loop is csrc/impute.cpp's
// (qa::impute_samples_product); this file only hands it the entry point that returns the gamma columns
// (qa_fullpass_reads_select_gamma_batch), so that impute.cpp itself names no device entry point beyond those it always called.
// qa_impute_samples_reads is the same call with hla optional and the per-read outputs (output_read_label_prob).
#include "impute_testhook.h"

namespace qa {
void set_error(const char *fmt, ...);
__attribute__((visibility("hidden"))) int impute_samples_product(qa_panel_t *const *panels, int32_t n_panels, const qa_impute_params_t *params,
                                                                int32_t n_sample, int64_t sample_offset, const int32_t *read_off,
                                                                const int32_t *read_ptr, const int32_t *u, const int32_t *bq,
                                                                const int32_t *wif, double *dosage, double *gp_t, double *phasing_haps,
                                                                int32_t *read_labels, int32_t *nDosage, int64_t *stats,
                                                                const qa_impute_hla_t *hla, qa_fullpass_select_gamma_fn select_gamma,
                                                                const qa_impute_reads_out_t *reads_out);
__attribute__((visibility("hidden"))) int gamma_column_check(const qa_panel *p, const char *who);   // (fullpass.hip)
}

namespace {

int be_fullpass_select_gamma(void *h, int32_t n_chain, int32_t n_label, int32_t n_sample, const int32_t *cs, const int32_t *read_off,
                             const int32_t *read_ptr, const int32_t *u, const int32_t *bq, const int32_t *H, const int32_t *wd,
                             const int32_t *wt, const int32_t *cols, int32_t Ktop, double minGL, double *dosage, int32_t top_width,
                             int32_t *top_idx, float *top_val, int32_t *top_cnt, int32_t Ksubset, int32_t Knew, const int32_t *which,
                             const uint64_t *seed, int32_t *which_next, int32_t *status, int32_t gamma_grid, double *gamma_col) {
    return qa_fullpass_reads_select_gamma_batch(static_cast<qa_panel_t *>(h), n_chain, n_label, n_sample, cs, read_off, read_ptr, u, bq,
                                                H, wd, wt, cols, Ktop, minGL, dosage, top_width, top_idx, top_val, top_cnt, Ksubset, Knew,
                                                which, seed, which_next, status, gamma_grid, gamma_col);
}

}   // namespace

extern "C" int qa_impute_samples_hla(qa_panel_t *const *panels, int32_t n_panels, const qa_impute_params_t *params, int32_t n_sample,
                                     int64_t sample_offset, const int32_t *read_off, const int32_t *read_ptr, const int32_t *u,
                                     const int32_t *bq, const int32_t *wif, double *dosage, double *gp_t, double *phasing_haps,
                                     int32_t *read_labels, int32_t *nDosage, int64_t *stats, const qa_impute_hla_t *hla) {
    if (!hla) {
        qa::set_error("qa_impute_samples_hla: hla is NULL");
        return QA_ERR_INVALID;
    }
    return qa_impute_samples_reads(panels, n_panels, params, n_sample, sample_offset, read_off, read_ptr, u, bq, wif, dosage, gp_t,
                                   phasing_haps, read_labels, nDosage, stats, hla, nullptr);
}

extern "C" int qa_impute_samples_reads(qa_panel_t *const *panels, int32_t n_panels, const qa_impute_params_t *params, int32_t n_sample,
                                       int64_t sample_offset, const int32_t *read_off, const int32_t *read_ptr, const int32_t *u,
                                       const int32_t *bq, const int32_t *wif, double *dosage, double *gp_t, double *phasing_haps,
                                       int32_t *read_labels, int32_t *nDosage, int64_t *stats, const qa_impute_hla_t *hla,
                                       const qa_impute_reads_out_t *reads_out) {
    if (!hla)
        return qa::impute_samples_product(panels, n_panels, params, n_sample, sample_offset, read_off, read_ptr, u, bq, wif, dosage, gp_t,
                                          phasing_haps, read_labels, nDosage, stats, nullptr, nullptr, reads_out);
    // every handle must keep the gamma column: refused here, before any sample is imputed, not at the last seek iteration
    if (panels && n_panels >= 1 && n_panels <= 16 && qa_device_count() >= 1)
        for (int i = 0; i < n_panels; i++)
            if (panels[i]) {
                const int st = qa::gamma_column_check(panels[i], "qa_impute_samples_hla");
                if (st != QA_OK) return st;
            }
    return qa::impute_samples_product(panels, n_panels, params, n_sample, sample_offset, read_off, read_ptr, u, bq, wif, dosage, gp_t,
                                      phasing_haps, read_labels, nDosage, stats, hla, be_fullpass_select_gamma, reads_out);
}
