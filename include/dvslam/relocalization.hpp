// dvslam/relocalization.hpp — a frame's pose in the map without a prior, as an object (dvs_reloc_* of dvslam_hip.h; INTEGRATION.md
// "Relocalisation"): every landmark searches all keypoints, the keypoints keep one landmark each, P3P RANSAC finds a pose on the kept
// pairs and a dvslam::MapTracker's handle confirms it.  The reference has no counterpart (its front end is odometry only).  Header-only,
// plain C++; not thread-safe; not copyable.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"

namespace dvslam {

class Relocalizer {
 public:
  struct Pairs { std::vector<int32_t> lm_row, kp_index, dist; std::vector<uint8_t> pnp_inlier; };

  // the defaults for the given intrinsics; change fields of the returned struct before constructing
  static dvs_reloc_params defaultParams(double fx, double fy, double cx, double cy) {
    dvs_reloc_params p;
    dvs_reloc_default_params(&p);
    p.K4[0] = fx; p.K4[1] = fy; p.K4[2] = cx; p.K4[3] = cy;
    return p;
  }
  explicit Relocalizer(const dvs_reloc_params& params, int device = 0) : params_(params) {
    check(dvs_reloc_create(&params, device, &h_), "dvs_reloc_create");
  }
  ~Relocalizer() { dvs_reloc_destroy(h_); }
  Relocalizer(const Relocalizer&) = delete;
  Relocalizer& operator=(const Relocalizer&) = delete;

  void setStream(void* hip_stream) { check(dvs_reloc_set_stream(h_, hip_stream), "dvs_reloc_set_stream"); }

  // host arrays: lm_xyz 3 floats and lm_desc 32 bytes per landmark, lm_id ascending (empty: the rows), desc 32 bytes per keypoint; mt confirms
  // -> the record; R, t are the camera-to-world pose when status == DVS_RELOC_OK
  dvs_reloc_result locate(dvs_maptrack* mt, const std::vector<float>& lm_xyz, const std::vector<uint8_t>& lm_desc, const std::vector<int64_t>& lm_id,
                          const std::vector<dvs_keypoint>& kps, const std::vector<uint8_t>& desc) {
    const size_t n_lm = lm_xyz.size() / 3, n_kp = kps.size();
    if (lm_desc.size() != n_lm * 32 || desc.size() != n_kp * 32 || (!lm_id.empty() && lm_id.size() != n_lm))
      throw std::invalid_argument("Relocalizer::locate: row counts differ");
    dvs_reloc_result r;
    check(dvs_reloc_locate(h_, mt, lm_xyz.data(), lm_desc.data(), lm_id.empty() ? nullptr : lm_id.data(), (int32_t)n_lm, kps.data(), desc.data(), (int32_t)n_kp, &r),
          "dvs_reloc_locate");
    return r;
  }
  // the same on device arrays; synchronises
  dvs_reloc_result locateDevice(dvs_maptrack* mt, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm, const dvs_keypoint* d_kps,
                                const uint8_t* d_desc, int32_t n_kp) {
    dvs_reloc_result r;
    check(dvs_reloc_locate_device(h_, mt, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, &r), "dvs_reloc_locate_device");
    return r;
  }
  // a frame's device keypoints against the backend's landmark table as it stands; the map is not modified
  dvs_reloc_result relocalizeFrame(dvs_backend* backend, dvs_maptrack* mt, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp) {
    dvs_reloc_result r;
    check(dvs_backend_relocalize_frame(backend, h_, mt, d_kps, d_desc, n_kp, &r), "dvs_backend_relocalize_frame");
    return r;
  }
  // after a dvs_tracker_track: the tracker's last frame against the backend's map; apply: a confirmed pose replaces the tracker's
  dvs_reloc_result relocalize(dvs_tracker* tracker, dvs_backend* backend, dvs_maptrack* mt, bool apply) {
    dvs_reloc_result r;
    check(dvs_tracker_relocalize(tracker, backend, h_, mt, apply ? 1 : 0, &r), "dvs_tracker_relocalize");
    return r;
  }
  // the last call's stage-3 list
  Pairs pairs() {
    int32_t n = 0;
    check(dvs_reloc_get_pairs(h_, 0, nullptr, nullptr, nullptr, nullptr, &n), "dvs_reloc_get_pairs");
    Pairs p;
    p.lm_row.resize((size_t)n); p.kp_index.resize((size_t)n); p.dist.resize((size_t)n); p.pnp_inlier.resize((size_t)n);
    check(dvs_reloc_get_pairs(h_, n, p.lm_row.data(), p.kp_index.data(), p.dist.data(), p.pnp_inlier.data(), &n), "dvs_reloc_get_pairs");
    return p;
  }
  dvs_reloc* handle() const { return h_; }
  const dvs_reloc_params& params() const { return params_; }

 private:
  static void check(dvs_status s, const char* what) {
    if (s != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
  }
  dvs_reloc_params params_;
  dvs_reloc* h_ = nullptr;
};

}  // namespace dvslam
