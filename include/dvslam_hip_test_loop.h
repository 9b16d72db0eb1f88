/*
 * dvslam_hip_test_loop.h — the test hook of the loop verification (csrc/loop_verify.hip), part of dvslam_hip_test.h, which includes it:
 * exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.
 * Why a header of its own: tests/test_host_logic.py::test_exports_every_declared_symbol pins the list of dvs_test_* declarations in the
 * text of dvslam_hip_test.h itself, and existing tests stay as they are; a hook added there would fail it (dvslam_hip_test_tracker.h is
 * the precedent).
 */
#ifndef DVSLAM_HIP_TEST_LOOP_H
#define DVSLAM_HIP_TEST_LOOP_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* (needs a GPU) dvs_loopv_db_verify_device's own launch sequence — same kernels, same grids — for a batch of cap_cand candidate slots of
 * which the first n_cand are listed, on host inputs uploaded as they are: xyz_query [stride_rows][3] (rows past n are uploaded too: the
 * kernels must not look at them), train_idx [cap_cand][stride_rows].  Beside the product's outputs (results [cap_cand], inlier_mask
 * [cap_cand][stride_rows], both poisoned before the call) it returns what every stage left on the device, per slot c:
 *   gather      n_list[c] = rows of the list the later stages run on (0 where the candidate failed the gather), list_i[c][stride_rows] =
 *               the query row of list position k, list_pts[c][6][stride_rows] = planes ex ey ez qx qy qz by list position;
 *   hypotheses  sample[c][H][3] (list positions, draw order), valid[c][H], models[c][H][12] (R row-major, t), gap[c][H] = (lambda1 -
 *               lambda2) / |lambda1| of Horn's matrix (NaN where no fit ran);
 *   score       counts[c][H];      select  sel[c][4] = {best hypothesis or -1, iterations run, its count, 0};
 *   refine      rounds[c][9][16]: row 0 the selected hypothesis, row r the fit of round r: R (9), t (3), |S_r|, accepted (1 / 0), fit not
 *               degenerate (1 / 0), 0; rows of rounds that did not run are zeros. */
dvs_status dvs_test_loop_verify_stages(dvs_loop_db* db, const float* xyz_query, int32_t n, int32_t stride_rows, const int32_t* entry_ids, int32_t n_cand,
                                       int32_t cap_cand, const int32_t* train_idx, const dvs_loop_verify_params* params, dvs_loop_verify_result* results,
                                       uint8_t* inlier_mask, int32_t* n_list, int32_t* list_i, float* list_pts, int32_t* sample, int32_t* valid,
                                       double* models, double* gap, int32_t* counts, int32_t* sel, double* rounds);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_LOOP_H */
