// bamrange_entry.cpp -- the product's entry points of the range call (include/quilt_amd_io.h): qa_impute_bam_range_ex, and the
// two earlier entries as calls of it.  The host code is csrc/bamrange.cpp's (qa::bam_range_impl); this file hands it the
// library's own imputation call and applies the refusals that need a panel handle.
#include "bamrange_impl.hpp"

namespace qa {
void set_error(const char *fmt, ...);
__attribute__((visibility("hidden"))) int gamma_column_check(const qa_panel *p, const char *who);   // (fullpass.hip)
}

extern "C" {

int qa_impute_bam_range(qa_panel_t *const *panels, int32_t n_panels, const qa_impute_params_t *params, const qa_bam_range_io_t *io,
                        int32_t n_sample, const char *const *bam_paths, const int64_t *sample_index, const double *ff,
                        qa_bam_range_result_t **out) {
    const qa_bam_range_extras_t ex{0, 0, 0, -1};
    return qa_impute_bam_range_ex(panels, n_panels, params, io, &ex, n_sample, bam_paths, sample_index, ff, out);
}

int qa_impute_bam_range_bx(qa_panel_t *const *panels, int32_t n_panels, const qa_impute_params_t *params, const qa_bam_range_io_t *io,
                           int32_t use_bx_tag, int32_t bxTagUpperLimit, int32_t n_sample, const char *const *bam_paths,
                           const int64_t *sample_index, const double *ff, qa_bam_range_result_t **out) {
    const qa_bam_range_extras_t ex{use_bx_tag, bxTagUpperLimit, 0, -1};
    return qa_impute_bam_range_ex(panels, n_panels, params, io, &ex, n_sample, bam_paths, sample_index, ff, out);
}

int qa_impute_bam_range_ex(qa_panel_t *const *panels, int32_t n_panels, const qa_impute_params_t *params, const qa_bam_range_io_t *io,
                           const qa_bam_range_extras_t *ex, int32_t n_sample, const char *const *bam_paths, const int64_t *sample_index,
                           const double *ff, qa_bam_range_result_t **out) {
    if (!panels || n_panels < 1 || !panels[0]) {
        if (out) *out = nullptr;
        qa::set_error("qa_impute_bam_range: no panel handle");
        return QA_ERR_INVALID;
    }
    int32_t K = 0, G = 0, T = 0;
    if (ex && ex->hla_grid >= 0) {   // hla_run: the panel's dimensions for the refusals, and every handle must keep the gamma column
        if (out) *out = nullptr;
        if (qa_panel_get_dims(panels[0], &K, &G, &T) != QA_OK) return QA_ERR_INVALID;
        if (n_panels <= 16 && qa_device_count() >= 1)
            for (int i = 0; i < n_panels; i++)
                if (panels[i]) {
                    const int st = qa::gamma_column_check(panels[i], "qa_impute_bam_range_ex");
                    if (st != QA_OK) return st;
                }
    }
    return qa::bam_range_impl(
        [&](const qa_impute_params_t *P, int32_t n, const int32_t *ro, const int32_t *rp, const int32_t *u, const int32_t *bq, const int32_t *wif,
            double *dosage, double *gp_t, double *haps, int32_t *labels, int32_t *nDosage, int64_t *stats, const qa_impute_hla_t *hla,
            const qa_impute_reads_out_t *reads_out) {
            if (!hla && !reads_out)   // (no option: the call this entry has always made)
                return qa_impute_samples(panels, n_panels, P, n, 0, ro, rp, u, bq, wif, dosage, gp_t, haps, labels, nDosage, stats);
            return qa_impute_samples_reads(panels, n_panels, P, n, 0, ro, rp, u, bq, wif, dosage, gp_t, haps, labels, nDosage, stats, hla,
                                           reads_out);
        },
        params, io, ex, K, G, n_sample, bam_paths, sample_index, ff, out);
}

}   // extern "C"
