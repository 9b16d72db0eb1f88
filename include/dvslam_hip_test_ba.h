/*
 * dvslam_hip_test_ba.h — the test hooks of the global bundle-adjustment solver (csrc/ba.hip, dvs_ba_solve_global): exported by
 * libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.  A header of its own for the reason
 * dvslam_hip_test_pgo.h gives.
 */
#ifndef DVSLAM_HIP_TEST_BA_H
#define DVSLAM_HIP_TEST_BA_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* (need a GPU) both work at the problem's current point, with the Jacobi scaling and D = clamp(diag, 1e-6, 1e32) rebuilt from it,
 * through the kernels the solve itself runs (include/dvslam_hip.h, "Global BA", defines S, M and b).
 * S applied once: y = S x (x, y, b [6 K]; Minv [K][36] row-major).  Rows of fixed cameras are zero and those of x are not read. */
dvs_status dvs_ba_schur_probe(dvs_ba* h, double radius, const double* x_in, double* y_out, double* Minv_out, double* b_out);
/* one linear solve: the PCG's x [6 K] (scaled, as solved), the iterations run, the recurrence's |r| / |b|, and ok = 0 when the solve
 * stopped before its first iteration.  max_pcg_iterations 0: max(100, 12 x free cameras). */
dvs_status dvs_ba_pcg_probe(dvs_ba* h, double radius, double eta, int32_t max_pcg_iterations, double* x_out, int32_t* iterations,
                            double* rel_residual, int32_t* ok);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_BA_H */
