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

/* (needs a GPU) ONE Levenberg-Marquardt trial step of dvs_pgo_solve at `radius`, through the functions that solver's loop itself calls:
 * the enqueue of a trial (LM diagonal, preconditioner, linear solve, candidate, candidate cost and model term, the record), the read of
 * the record, and the commit of an accepted step.  The first call after dvs_pgo_set_nodes / dvs_pgo_set_edges linearises at the handle's
 * poses, as the solver's prologue does; later calls work at the linearisation the handle holds, as later iterations of the loop do.
 *   max_pcg_iterations  0: max(100, 2 N), as dvs_pgo_params has it
 *   reuse_diagonal      non-zero: the LM diagonal of the call before is kept (the loop does so after a rejected step)
 *   commit              non-zero: the candidate becomes the point and is linearised (the loop's accept path); the verdict is the caller's
 *   x_in                NULL, or a step [6 N] to take in place of the linear solve's: the PCG kernel is not launched, and the record's
 *                       rnorm, gnorm, pcg_iterations and breakdown are zero
 * Outputs, each may be NULL: cur_q [N][4] (w, x, y, z), cur_t [N][3] the point the step was taken from; x [6 N] the step; D [6 N] the LM
 * diagonal; cand_q, cand_t the candidate; rec the status record (cur_cost and gmax are those of the point the step was taken from). */
typedef struct dvs_pgo_step_record {
  double cur_cost, gmax, cand_cost, model_cost_change, step2, x2, rnorm, gnorm;
  int32_t pcg_iterations, finite, breakdown, reserved;
} dvs_pgo_step_record;
dvs_status dvs_test_pgo_trial_step(dvs_pgo* h, double radius, double eta, int32_t max_pcg_iterations, int32_t reuse_diagonal, int32_t commit,
                                   const double* x_in, double* cur_q, double* cur_t, double* x, double* D, double* cand_q, double* cand_t,
                                   dvs_pgo_step_record* rec);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_PGO_H */
