// dvslam/map_tracking.hpp — a frame tracked against the map as an object (dvs_maptrack_* of dvslam_hip.h; INTEGRATION.md "Tracking against
// the map"): the landmarks projected into the frame, a descriptor search in a window around each projection, a one-to-one assignment and
// the refinement of the frame's pose on the kept pairs.  The reference has no counterpart (its front end is odometry only).  Header-only,
// plain C++; not thread-safe; not copyable.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"

namespace dvslam {

class MapTracker {
 public:
  struct Matches { std::vector<int32_t> lm_row; std::vector<int64_t> lm_id; std::vector<int32_t> dist; std::vector<uint8_t> inlier; };

  // the defaults for the given image size and intrinsics; change fields of the returned struct before constructing
  static dvs_maptrack_params defaultParams(int rows, int cols, double fx, double fy, double cx, double cy) {
    dvs_maptrack_params p;
    dvs_maptrack_default_params(&p);
    p.rows = rows; p.cols = cols; p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
    return p;
  }
  explicit MapTracker(const dvs_maptrack_params& params, int device = 0) : params_(params) {
    check(dvs_maptrack_create(&params, device, &h_), "dvs_maptrack_create");
  }
  ~MapTracker() { dvs_maptrack_destroy(h_); }
  MapTracker(const MapTracker&) = delete;
  MapTracker& operator=(const MapTracker&) = delete;

  void setStream(void* hip_stream) { check(dvs_maptrack_set_stream(h_, hip_stream), "dvs_maptrack_set_stream"); }

  // host arrays: lm_xyz 3 floats and lm_desc 32 bytes per landmark, lm_id ascending (empty: the rows), desc 32 bytes per keypoint; the prior
  // pose camera-to-world (R9 row-major, t3) -> the record; its pose is the refined one when status == DVS_MAPTRACK_OK
  dvs_maptrack_result track(const std::vector<float>& lm_xyz, const std::vector<uint8_t>& lm_desc, const std::vector<int64_t>& lm_id,
                            const std::vector<dvs_keypoint>& kps, const std::vector<uint8_t>& desc, const double* R9, const double* t3) {
    const size_t n_lm = lm_xyz.size() / 3, n_kp = kps.size();
    if (lm_desc.size() != n_lm * 32 || desc.size() != n_kp * 32 || (!lm_id.empty() && lm_id.size() != n_lm))
      throw std::invalid_argument("MapTracker::track: row counts differ");
    dvs_maptrack_result r;
    check(dvs_maptrack_track(h_, lm_xyz.data(), lm_desc.data(), lm_id.empty() ? nullptr : lm_id.data(), (int32_t)n_lm, kps.data(), desc.data(), (int32_t)n_kp,
                             R9, t3, &r),
          "dvs_maptrack_track");
    return r;
  }
  // the same on device arrays; synchronises
  dvs_maptrack_result trackDevice(const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm, const dvs_keypoint* d_kps,
                                  const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3) {
    dvs_maptrack_result r;
    check(dvs_maptrack_track_device(h_, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, R9, t3, &r), "dvs_maptrack_track_device");
    return r;
  }
  // stages 1-3 alone; result == nullptr: asynchronous on the handle's stream
  void searchDevice(const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm, const dvs_keypoint* d_kps, const uint8_t* d_desc,
                    int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result = nullptr) {
    check(dvs_maptrack_search_device(h_, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, R9, t3, result), "dvs_maptrack_search_device");
  }
  // the pose refinement alone on explicit correspondences (device: n x 3 doubles, n x 2 doubles, n int32)
  dvs_maptrack_result refineDevice(const double* d_X, const double* d_px, const int32_t* d_octave, int32_t n, const double* R9, const double* t3) {
    dvs_maptrack_result r;
    check(dvs_maptrack_refine_device(h_, d_X, d_px, d_octave, n, R9, t3, &r), "dvs_maptrack_refine_device");
    return r;
  }
  // a frame's device keypoints against the backend's landmark table as it stands; the map is not modified
  dvs_maptrack_result trackFrame(dvs_backend* backend, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3) {
    dvs_maptrack_result r;
    check(dvs_backend_track_frame(backend, h_, d_kps, d_desc, n_kp, R9, t3, &r), "dvs_backend_track_frame");
    return r;
  }
  // after a dvs_tracker_track: the tracker's last frame against the backend's map; apply: a refined pose replaces the tracker's
  dvs_maptrack_result trackMap(dvs_tracker* tracker, dvs_backend* backend, bool apply) {
    dvs_maptrack_result r;
    check(dvs_tracker_track_map(tracker, backend, h_, apply ? 1 : 0, &r), "dvs_tracker_track_map");
    return r;
  }
  // the last call's per-keypoint arrays
  Matches matches() {
    int32_t n = 0;
    check(dvs_maptrack_get_matches(h_, 0, nullptr, nullptr, nullptr, nullptr, &n), "dvs_maptrack_get_matches");
    Matches m;
    m.lm_row.resize((size_t)n); m.lm_id.resize((size_t)n); m.dist.resize((size_t)n); m.inlier.resize((size_t)n);
    check(dvs_maptrack_get_matches(h_, n, m.lm_row.data(), m.lm_id.data(), m.dist.data(), m.inlier.data(), &n), "dvs_maptrack_get_matches");
    return m;
  }
  dvs_maptrack* handle() const { return h_; }
  const dvs_maptrack_params& params() const { return params_; }

 private:
  static void check(dvs_status s, const char* what) {
    if (s != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
  }
  dvs_maptrack_params params_;
  dvs_maptrack* h_ = nullptr;
};

}  // namespace dvslam
