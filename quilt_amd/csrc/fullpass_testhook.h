/* fullpass_testhook.h -- PRIVATE to the library's build and to tests/ (not part of the public ABI of include/quilt_amd.h).
 *
 * What the launch planner of the full-panel passes (csrc/fullpass.hip: PassLayout, plan_chunk) decided for the calling
 * thread's last launch set, and what run_passes then took from the arena: tests/test_fullpass_plan_gpu.py holds the two
 * against each other.  Nothing in the product -- quilt_amd/, shim/, bench.py -- uses it.
 */
#ifndef QA_FULLPASS_TESTHOOK_H
#define QA_FULLPASS_TESTHOOK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* out[0] = passes of the launch set (P), out[1] = planned bytes per pass, out[2] = the plan's fixed term in bytes,
 * out[3] = arena bytes carved when the launch set returned, out[4] = buffers in the layout, out[5] = the kind of kernels
 * that ran it (PassKind, pass_layout.hpp).  All 0 before the thread's first launch set. */
int qa_fullpass_last_plan(int64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
