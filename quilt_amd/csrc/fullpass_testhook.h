/* fullpass_testhook.h -- PRIVATE to the library's build and to tests/ (not part of the public ABI of include/quilt_amd.h).
 *
 * What the launch planner of the full-panel passes (csrc/fullpass.hip: PassLayout, plan_chunk) decided for the calling
 * thread's last launch set, and what run_passes then took from the arena: tests/test_fullpass_plan_gpu.py holds the two
 * against each other.  Nothing in the product -- quilt_amd/, shim/, bench.py -- uses it.
 */
#ifndef QA_FULLPASS_TESTHOOK_H
#define QA_FULLPASS_TESTHOOK_H
#include <stdint.h>
#include "../../include/quilt_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out[0] = passes of the launch set (P), out[1] = planned bytes per pass, out[2] = the plan's fixed term in bytes,
 * out[3] = arena bytes carved when the launch set returned, out[4] = buffers in the layout, out[5] = the kind of kernels
 * that ran it (PassKind, pass_layout.hpp).  All 0 before the thread's first launch set. */
int qa_fullpass_last_plan(int64_t out[6]);

/* What the host tables (csrc/fullpass.hip: pick_geometry; csrc/fullpass64.hip: geo64 and each launcher's own choice between <4, 3>
 * and <5, 2>) decide for a panel of K haplotypes and a PassKind (pass_layout.hpp), without a device: out[0] = NT, out[1] = NCH
 * (chunks per lane; the fp64 ranking / dosage kinds: chunk rows of 8 192 haplotypes, streamed ones included), out[2] = NR (rows in
 * registers), out[3] = NL (rows in LDS), out[4] = n_last (lanes of the last row), out[5] = NS (rows streamed through HBM) -- 2 .. 5
 * are 0 for the other kinds --, out[6] = Kq (haplotypes of the padded layout), out[7] = 1 when the library holds that
 * build (the kinds' built lists: all of what the tables choose from, fewer with QA_FAST_BUILD).  All 0 when the kind does not take this K.  For KIND_F64_DOS the fields are those of launch_fb64_dosage, after its
 * lds_bytes_d adjustment.  tests/k_cases.py derives its table of K values and the edge haplotypes of each K from it. */
int qa_fullpass_geometry(int32_t K, int32_t kind, int32_t out[8]);

/* ONE launch set of n_pass passes on the kernels behind the handle's dosage passes, with what the batched entries of the public
 * ABI do not let a caller choose or see: the per-pass flags in one launch set (flags[i] = 1: a dosage pass, 0: a pass for its
 * best-haplotype lists only; with K_top_matches > 0 every pass yields lists), always_normalize, and c (n_pass x nGrids).
 * gl, dosage, best_* as qa_fullpass_batch.  QA_ERR_CAPACITY when the passes do not fit one launch set.
 * tests/test_sum_order_batched_gpu.py holds the two forms of the reference-order kernels against each other through it. */
int qa_fullpass_launch_set(qa_panel_t *panel, int32_t n_pass, const double *gl, const int32_t *flags,
                           const int32_t *gammaSmall_cols_to_get, int32_t K_top_matches, int32_t always_normalize,
                           double *dosage, double *c, int32_t *best_ptr, int32_t *best_idx, double *best_val, int64_t best_cap);

/* The selection kernel (csrc/select.hip: qa::launch_select) on lists the CALLER supplies, without a full-panel pass in front:
 * top [n_chain][n_label][n_thin][top_width] 0-based haplotypes, best first, -1 = no entry; which [n_chain][Ksubset] 1-based;
 * seed, want [n_chain]; which_next [n_chain][Ksubset] and status [n_chain] as qa_fullpass_reads_select_batch returns them (a row
 * of which_next whose chain is not wanted, or is handed back with status 1 before anything was written, keeps what the caller
 * put there).  The argument checks are those of the public entry.  tests/test_support_geometry_gpu.py steers the kernel through
 * it to the list shapes a real pass cannot be made to produce. */
int qa_select_from_lists(int32_t n_chain, int32_t n_label, int32_t n_thin, int32_t top_width, int32_t K_top_matches, int32_t K,
                         int32_t Ksubset, int32_t Knew, const int32_t *top, const int32_t *which, const uint64_t *seed,
                         const int32_t *want, int32_t *which_next, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif
