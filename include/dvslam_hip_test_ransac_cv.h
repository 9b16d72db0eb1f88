/*
 * dvslam_hip_test_ransac_cv.h — the test hooks of the OpenCV-procedure robust estimators (csrc/ransac.hip, csrc/pnp_cv.h:
 * dvs_find_fundamental_cv*, dvs_solve_pnp_ransac_cv*), part of dvslam_hip_test.h, which includes it: exported by libdvslam_hip_test.so
 * (-DDVS_TEST_HOOKS) only, never by the product library.  A header of its own for the reason dvslam_hip_test_maptrack.h gives.
 * tests/test_gpu_ransac_cv_stages.py holds every stage to the float64 statements of tests/ransac_cv_stage_ref.py through them.
 */
#ifndef DVSLAM_HIP_TEST_RANSAC_CV_H
#define DVSLAM_HIP_TEST_RANSAC_CV_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* (need a GPU) Each runs the product call's own body — the same import, launches and grids — and returns, beside its results, what every
 * stage left on the device.  Problem b = correspondences [offsets[b], offsets[b + 1]) of the concatenated point arrays.
 *
 * dvs_test_fm_cv_stages: ONE pass of dvs_find_fundamental_cv_batch with the models of H iterations of a loop of up to max_iters (the
 * product runs H = min(max_iters, 96) first and H = max_iters where sel[3] asked for it; below 15 points H is LMedS' fixed count, 300 for
 * confidence 0.99).  The batch is of one kind: every problem >= 15 points (RANSAC) or every problem 8 .. 14 (LMedS).  Per problem:
 *   samples[b][H][7] and found[b] (iterations getSubset found a sample for; rows past it are zeros),
 *   F_all[b][3 H][9] and valid[b][3 H] (model 3 h + k = root k of sample h; invalid slots are zeros),
 *   counts[b][3 H] (RANSAC; LMedS has none: zeros),
 *   sel[b][4] = {best model or -1, iterations run, inliers, RANSAC: the loop wanted more than H / LMedS: success},
 *   mask[offsets[b] ..] and Fbest[b][9] as the pass left them on the device. */
dvs_status dvs_test_fm_cv_stages(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold,
                                 double confidence, int32_t max_iters, int32_t H, int32_t* samples, int32_t* found, double* F_all, int32_t* valid,
                                 int32_t* counts, int32_t* sel, uint8_t* mask, double* Fbest);
/* dvs_test_pnp_cv_stages: dvs_solve_pnp_ransac_cv_batch with iterations = H.  Per problem: samples[b][H][5] (zeros for a problem of fewer
 * than 6 points, which is refused), models[b][H][18] = {rvec, tvec, R row-major, 3 pad}, counts[b][H], sel[b][4] = {best, iterations run,
 * inliers, 0}, and the product's outputs: the inlier list at inliers + offsets[b], n_inliers[b], success[b], rvec3[b][3], tvec3[b][3]. */
dvs_status dvs_test_pnp_cv_stages(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                  double reproj_err, double confidence, int32_t H, int32_t* samples, double* models, int32_t* counts, int32_t* sel,
                                  int32_t* inliers, int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3);
/* k_ransac_select alone in the OpenCV-procedure form: counts of H models, `group` per iteration (H a multiple of it), of a loop of up to
 * max_iters_true iterations for `found` of which getSubset had a sample.  sel4[3] = 1: the loop wanted more than the H / group available. */
dvs_status dvs_test_ransac_select_cv(const int32_t* counts, int32_t H, int32_t n, int32_t model_points, double confidence, int32_t group, int32_t found,
                                     int32_t max_iters_true, int32_t* sel4);
/* k_pnpcv_refit alone on ONE problem with a model of the caller's as the selected one (model6 = rvec, tvec; NULL: nothing selected), grid
 * and block as the estimator's.  inliers: room for n indices, -1 where none was written.  dbg8 = {the initialisation handed to the
 * Levenberg-Marquardt loop: rvec, tvec; path: 0 no initialisation (the model is returned, success 0), 1 planar (homography), 2 DLT; the
 * loop's iteration count}. */
dvs_status dvs_test_pnpcv_refit(const float* pts3d, const float* pts2d, int32_t n, const double* K4, const double* model6, double reproj_err, int32_t* inliers,
                                int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3, double* dbg8);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_RANSAC_CV_H */
