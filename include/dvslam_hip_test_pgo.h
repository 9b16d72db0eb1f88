/*
 * dvslam_hip_test_pgo.h — the test hooks of the pose-graph solver (csrc/pose_graph.hip), part of dvslam_hip_test.h, which includes it:
 * exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.
 * Why a header of its own: tests/test_host_logic.py::test_exports_every_declared_symbol pins the list of dvs_test_* declarations in the
 * text of dvslam_hip_test.h itself, and existing tests stay as they are (dvslam_hip_test_loop.h is the precedent).
 */
#ifndef DVSLAM_HIP_TEST_PGO_H
#define DVSLAM_HIP_TEST_PGO_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* (need a GPU) both work at the linearisation of the handle's current poses, with D = clamp(diag(H), 1e-6, 1e32) rebuilt from it, through
 * the kernels and device functions the solve itself runs.
 * the operator on a given vector: y = (H + D / radius) p, p and y [6 N]; rows of fixed nodes of y are 0 and those of p are not read */
dvs_status dvs_test_pgo_apply(dvs_pgo* h, double radius, const double* p, double* y);
/* one linear solve (preconditioner build, then the PCG kernel): x [6 N], the iterations run, and the recurrence's |r| and |g| at the end */
dvs_status dvs_test_pgo_pcg(dvs_pgo* h, double radius, double eta, int32_t max_it, double* x, int32_t* iterations, double* rnorm, double* gnorm);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_PGO_H */
