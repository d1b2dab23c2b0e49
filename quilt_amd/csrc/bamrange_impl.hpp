// bamrange_impl.hpp -- the range call's host code (csrc/bamrange.cpp) as its entry points reach it: the product's
// (csrc/bamrange_entry.cpp, over qa_impute_samples / qa_impute_samples_reads) and the test hook's (csrc/bamrange.cpp itself, over
// a checker's table).  Internal to the library.
#pragma once
#include <cstdint>
#include <functional>

#include "../../include/quilt_amd.h"
#include "../../include/quilt_amd_io.h"

namespace qa {

// qa_impute_samples_reads, or the test hook's form of it, on the kept samples (hla / reads_out NULL: the plain call)
using BamRangeImputeFn = std::function<int(const qa_impute_params_t *, int32_t, const int32_t *, const int32_t *, const int32_t *, const int32_t *,
                                           const int32_t *, double *, double *, double *, int32_t *, int32_t *, int64_t *,
                                           const qa_impute_hla_t *, const qa_impute_reads_out_t *)>;

// K, G: the panel's haplotypes and grids (read with ex->hla_grid >= 0 only)
__attribute__((visibility("hidden"))) int bam_range_impl(const BamRangeImputeFn &impute, const qa_impute_params_t *params,
                                                        const qa_bam_range_io_t *io, const qa_bam_range_extras_t *ex, int32_t K, int32_t G,
                                                        int32_t n_sample, const char *const *bam_paths, const int64_t *sample_index,
                                                        const double *ff, qa_bam_range_result_t **out);

}   // namespace qa
