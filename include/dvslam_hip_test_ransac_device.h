/*
 * dvslam_hip_test_ransac_device.h — the test hook of the robust estimators' DEVICE forms (csrc/ransac_device.h: fm_own_device,
 * fm_cv_device, pnp_own_device, pnp_cv_device, which the tracker and the relocalisation call on points that already live on the device),
 * part of dvslam_hip_test.h, which includes it: exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.
 * A header of its own for the reason dvslam_hip_test_maptrack.h gives.  tests/test_gpu_ransac_device_forms.py compares what a form leaves
 * on the device with the output of the host entry point of the same estimator, byte for byte.
 */
#ifndef DVSLAM_HIP_TEST_RANSAC_DEVICE_H
#define DVSLAM_HIP_TEST_RANSAC_DEVICE_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* (needs a GPU) Uploads ONE problem — pts_a, pts_b and, for the own forms, the count word — calls the device form `form` on ctx with it,
 * waits for ctx's stream and downloads what the form's contract (csrc/ransac_device.h) says it writes.  The device buffers hold `cap`
 * correspondences, cap >= max(n, 1), and every result buffer is filled with 0xff bytes first: what the form does not write stays so.
 *   form 0  fm_own_device   pts_a / pts_b = pts1 / pts2 (n x 2); iters = max_iters; *d_n = n, n_bound = cap; writes mask[0 .. n)
 *   form 1  fm_cv_device    as form 0 without seed (n >= 8 is the host's)
 *   form 2  pnp_own_device  pts_a = object points (n x 3), pts_b = image points (n x 2); *d_n = n; writes rec64 (the 64-byte result
 *                           record {int32 n_inliers, int32 success, 8 unused, double rvec[3], tvec[3]}) and inliers[0 .. n_inliers)
 *   form 3  pnp_cv_device   as form 2 without seed (n >= 6 is the host's); writes sel4 = {best model or -1, iterations run, inliers, 0} too
 * mask: cap bytes; inliers: cap ints; buffers a form does not write may be NULL. */
dvs_status dvs_test_ransac_device_form(dvs_matcher* ctx, int32_t form, const float* pts_a, const float* pts_b, int32_t n, int32_t cap, const double* K4,
                                       int32_t iters, double threshold, double confidence, uint64_t seed, uint8_t* mask, uint8_t* rec64, int32_t* inliers,
                                       int32_t* sel4);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_RANSAC_DEVICE_H */
