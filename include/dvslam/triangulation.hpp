// dvslam/triangulation.hpp — LandmarkInfo::triangulate (backend.cpp:439-613) on the device, and Backend::syncCallback's association
// loop for one category (backend.cpp:735-777) with the re-triangulation of every matched landmark folded in.
//
// Why one batched launch BEFORE the walk gives the one-by-one loop's result exactly: at backend.cpp:772 the new observation is not yet
// in all_observations_ (inserted at :809) and the new keyframe is not yet in keyframes_ (pushed at :806); triangulate skips ids it cannot
// find.  So within one keyframe, landmark L is triangulated from the views stored before this keyframe only.  Its current position enters
// the parallax gate alone — the SVD, the reprojection check and the depth check do not read it.  For a landmark matched twice: if the
// first call rejects, the position is unchanged and the second call rejects again; if it accepts P1, the second call either fails the
// gate at P1 or recomputes exactly P1.  The result per landmark is therefore a pure, idempotent function of its stored views and its
// position at the start of the keyframe: dvs_triangulate_landmarks over the landmarks once, then associateSequential applies it.
//
// Pose convention: x_cam = R X + t.  KeyframeInfo::R / t passed unchanged reproduce the reference; (R^T, -R^T t) is the geometrically
// consistent binding (the reference's reprojectPoint reads the same R, t as camera -> world, backend.cpp:1156).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "association.hpp"

namespace dvslam {

// views of landmark l: [view_offsets[l], view_offsets[l + 1]) of view_kf (index into kf_R (nkf x 9) / kf_t (nkf x 3), < 0 = skipped) and
// view_px (u, v).  lm_xyz (nlm x 3) is updated in place; returns the per-landmark dvs_tri_status.
inline std::vector<int32_t> triangulateLandmarks(dvs_matcher* ctx, int nkf, const double* kf_R, const double* kf_t, double fx, double fy, double cx,
                                                 double cy, int nlm, const int64_t* view_offsets, const int32_t* view_kf, const float* view_px,
                                                 float* lm_xyz) {
  std::vector<int32_t> status((size_t)nlm, DVS_TRI_FEW_VIEWS);
  const dvs_status st = dvs_triangulate_landmarks(ctx, nkf, kf_R, kf_t, fx, fy, cx, cy, nlm, view_offsets, view_kf, view_px, lm_xyz, lm_xyz, status.data());
  if (st != DVS_OK) throw std::runtime_error(std::string("dvs_triangulate_landmarks: ") + dvs_last_error());
  return status;
}

// backend.cpp:735-777 for the observations of one category against that category's landmarks (lm_* in the database's order, lm_xyz
// updated in place).  R, t: the new keyframe's pose as associateObservation uses it; the landmarks' stored views as triangulateLandmarks
// takes them (the views of keyframes stored before this one: the new observations are not in the database yet).  Returns best[i]
// (landmark index or -1); *tri_status (if given) receives every landmark's triangulation status, applied or not.
inline std::vector<int32_t> associateAndTriangulate(dvs_matcher* ctx, const uint8_t* obs_desc, const float* obs_px, int nobs, const uint8_t* lm_desc,
                                                    float* lm_xyz, int nlm, const double* R, const double* t, double fx, double fy, double cx,
                                                    double cy, double max_descriptor_distance, double max_reprojection_distance, int nkf,
                                                    const double* kf_R, const double* kf_t, const int64_t* view_offsets, const int32_t* view_kf,
                                                    const float* view_px, std::vector<int32_t>* tri_status = nullptr) {
  std::vector<float> tri(lm_xyz, lm_xyz + 3 * (size_t)nlm);
  const std::vector<int32_t> status = triangulateLandmarks(ctx, nkf, kf_R, kf_t, fx, fy, cx, cy, nlm, view_offsets, view_kf, view_px, tri.data());
  auto onMatch = [&](int, int j, float* xyz) {
    if (status[j] != DVS_TRI_UPDATED) return false;
    for (int k = 0; k < 3; k++) xyz[k] = tri[3 * (size_t)j + k];
    return true;
  };
  std::vector<int32_t> best = associateSequential(ctx, obs_desc, obs_px, nobs, lm_desc, lm_xyz, nlm, R, t, fx, fy, cx, cy, max_descriptor_distance,
                                                  max_reprojection_distance, onMatch);
  if (tri_status) *tri_status = status;
  return best;
}

}  // namespace dvslam
