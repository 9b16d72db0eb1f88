/*
 * dvslam_hip_test_ba.h — the test hooks of the global bundle-adjustment solver (csrc/ba.hip, dvs_ba_solve_global) and the step
 * hook of the sliding-window solver (dvs_ba_solve_device): exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.  A header of its own for the reason
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
 * stopped by breakdown before its first iteration (|b| = 0 is no breakdown: zero iterations, ok = 1).  max_pcg_iterations 0:
 * max(100, 12 x free cameras). */
dvs_status dvs_ba_pcg_probe(dvs_ba* h, double radius, double eta, int32_t max_pcg_iterations, double* x_out, int32_t* iterations,
                            double* rel_residual, int32_t* ok);

/* (needs a GPU) ONE trial step of dvs_ba_solve_device (the sliding-window solver; dvs_ba_set_device_window's rule decides between the
 * in-LDS and the tiled factorisation) at `radius`, through the functions that solver's loop itself calls to enqueue its launches.
 * The first call after dvs_ba_set_problem (or after a dvs_ba_solve_device / dvs_ba_set_device_window on the handle) first runs the
 * loop's prologue at the problem's parameters: upload, the point, its blocks, cost and gradient norm, the Jacobi scaling.  Later
 * calls keep the scaling and the point, as later iterations of the loop do.
 *   refresh  the loop's "rebuild the LM diagonal" flag (0 after a rejected step: the diagonal of the call before is reused)
 *   commit   non-zero: if the device's verdict accepts, the candidate becomes the point as in the loop (gated full evaluation and
 *            gradient norm behind the trial); the next call is then the loop's next iteration
 *   function_tolerance, parameter_tolerance   as dvs_ba_solve_device takes them (they enter the verdict)
 * Outputs, each may be NULL.  N = 6 K + 3 L, n = 6 x (free cameras with an observation), slots in camera order:
 *   scale, diag [N]   Jacobi scaling and LM diagonal (of the scaled system)
 *   Vinv [L][9]       per active landmark (zero rows otherwise)
 *   S [n][n], rhs [n] the reduced system as the factorisation assembles it: the H_pp part minus the four split sums in split order;
 *                     the block lower triangle (6 x 6 blocks, diagonal blocks whole), zero above it
 *   step [N]          the step as the candidate applies it: in parameter units (scaled back), camera rows negated
 *   cand_q [K][4], cand_t [K][3], cand_X [L][3]   the candidate point
 *   rec               the trial's status record; gmax and x_cost are those of the point the step was taken from
 * The handle's parameters (dvs_ba_get_parameters) stay those of dvs_ba_set_problem. */
typedef struct dvs_ba_step_record {
  int32_t ok, finite, accept, reserved;
  double model_change, sn, xn, cand_cost, gmax, x_cost;
} dvs_ba_step_record;
dvs_status dvs_ba_step_probe(dvs_ba* h, double radius, int32_t refresh, int32_t commit, double function_tolerance,
                             double parameter_tolerance, double* scale, double* diag, double* Vinv, double* S, double* rhs, double* step,
                             double* cand_q, double* cand_t, double* cand_X, dvs_ba_step_record* rec);

/* (needs a GPU) ONE trial step of dvs_ba_solve_global at `radius`, through the function that solver's loop itself calls for a trial
 * step (linear solve, the tail shared with dvs_ba_solve_device, one record read, the verdict, the accept).  The first call after
 * dvs_ba_set_problem, or after any solve or any other probe on the handle, first runs the loop's prologue at the problem's
 * parameters; later calls keep the scaling and the point, as later iterations of the loop do.
 *   refresh  the loop's "rebuild the LM diagonal" flag (0 after a rejected step: the stored diagonal is reused)
 *   commit   non-zero: the loop's own verdict is applied; if it accepts, the candidate becomes the point (full evaluation) and the
 *            next call is the loop's next iteration
 *   eta, max_pcg_iterations, function_tolerance, parameter_tolerance   as dvs_ba_solve_global takes them
 *   x_in     NULL, or camera rows [6 K] (scaled, not negated, as the PCG leaves them; rows of fixed cameras are not read) that take
 *            the place of the linear solve's: the system's launches run, the PCG does not (0 iterations, ok = 1), and the rest of
 *            the trial step runs on them.  Every iterate of a PCG started at zero satisfies x.(S x - b) = 0, which is all a
 *            formula for the model cost change needs in order to be right although it assumes S x = b; a step given here does not.
 * Outputs, each may be NULL.  N = 6 K + 3 L; the active set is dvs_ba_solve_global's (include/dvslam_hip.h, "Global BA"):
 *   scale, diag [N]   Jacobi scaling and LM diagonal (of the scaled system)
 *   Vinv [L][9]       per active landmark (zero rows otherwise)
 *   x [6 K]           the PCG's camera rows: scaled, as solved (not negated); zero rows for fixed cameras
 *   step [N]          the step as the candidate applies it: in parameter units (scaled back), camera rows negated
 *   cand_q [K][4], cand_t [K][3], cand_X [L][3]   the candidate point
 *   pcg_iterations, pcg_rel_residual, pcg_ok      as dvs_ba_pcg_probe returns them
 *   rec               the trial's status record; gmax and x_cost are those of the point the step was taken from
 * The handle's parameters (dvs_ba_get_parameters) stay those of dvs_ba_set_problem. */
dvs_status dvs_ba_global_step_probe(dvs_ba* h, double radius, int32_t refresh, int32_t commit, double eta, int32_t max_pcg_iterations,
                                    double function_tolerance, double parameter_tolerance, const double* x_in, double* scale,
                                    double* diag, double* Vinv, double* x, double* step, double* cand_q, double* cand_t, double* cand_X, int32_t* pcg_iterations,
                                    double* pcg_rel_residual, int32_t* pcg_ok, dvs_ba_step_record* rec);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_BA_H */
