/*
 * dvslam_hip_test_tracker.h — the test hooks of the tracking front end (csrc/tracker.hip), part of dvslam_hip_test.h, which includes it:
 * exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.
 * Why a header of its own: tests/test_host_logic.py::test_exports_every_declared_symbol pins the list of dvs_test_* declarations in the
 * text of dvslam_hip_test.h itself (ten of them), and existing tests stay as they are; a hook added there would fail it.
 */
#ifndef DVSLAM_HIP_TEST_TRACKER_H
#define DVSLAM_HIP_TEST_TRACKER_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* (no GPU needed) the tracker's feature culling order (frontend.cpp:1193-1219) on the host, through the ordering code the culling kernel
 * runs (csrc/cull_order.h: the std::sort replica of csrc/lsort.h under the reference's comparator a.first > b.first): (response, index)
 * pairs of the entries with matched[i] == 0 in index order, sorted, cut at max_new or at the first response < min_response.
 * order[0 .. *n_out) = their indices (capacity n). */
void dvs_test_cull_order(const float* response, const uint8_t* matched, int32_t n, int32_t max_new, float min_response, int32_t* order,
                         int32_t* n_out);

/* (needs a GPU) the same order through the culling kernel itself: keypoints that carry the responses, the matched indices as its match
 * list; n <= 3072.  *heap_ranges (may be NULL) = ranges of the introsort that met the depth limit and took the heapsort branch. */
dvs_status dvs_test_cull_order_device(const float* response, const uint8_t* matched, int32_t n, int32_t max_new, float min_response,
                                      int32_t* order, int32_t* n_out, int32_t* heap_ranges);

/* (no GPU needed) the tracker's pose step (csrc/pose_host.h, frontend.cpp:925-948): the inverse of PnP's motion (rvec3, tvec3), the
 * motion-outlier test on it and — unless it is one — R9 <- R9 Ri, t3 <- t3 + R9 ti in place.  Returns 1 where the pose was updated, 0
 * for a motion outlier (R9, t3 untouched).  rodrigues9 (may be NULL) = cv::Rodrigues(rvec3) as the step computes it. */
int32_t dvs_test_tracker_pose_step(double* R9, double* t3, const double* rvec3, const double* tvec3, double max_translation, double max_rotation,
                                   double* rodrigues9);

/* (no GPU needed) the relative pose of the motion mask (csrc/pose_host.h): a12 = T(t-1), b12 = T(t-2) or NULL, ref12 = the reference
 * frame's pose, each {R row-major, t}; R9 / t3 = the result.  quat_xyzw4 (may be NULL) = publishKeyframe's quaternion of a12's rotation. */
void dvs_test_tracker_relative_pose(const double* a12, const double* b12, const double* ref12, double* R9, double* t3, double* quat_xyzw4);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_TRACKER_H */
