// dvslam/covisibility.hpp — header-only C++ adapter over the "Covisibility" section of dvslam_hip.h (INTEGRATION.md "Covisibility"): the
// covisibility graph of the map a MappingBackend keeps on the device, the local BA window and the local map of one keyframe.
// covisibilityGraph() returns the weights and the neighbour lists, localWindow() the window as arrays, localBundleAdjust() refines it on a
// GlobalBA's solver handle (global_ba.hpp: keep one for the life of the map) and trackFrameLocal() tracks a frame against the local map
// only.  Errors throw std::runtime_error.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "global_ba.hpp"
#include "map_tracking.hpp"
#include "mapping_backend.hpp"

namespace dvslam {

struct CovisParams : dvs_covis_params {
  CovisParams() { dvs_covis_default_params(this); }
};

struct CovisGraph {
  int n = 0;                                   // keyframes
  std::vector<int32_t> weights;                // n x n, row-major (empty unless asked for)
  std::vector<int64_t> nb_offsets;             // n + 1
  std::vector<int32_t> nb_index, nb_weight;    // per keyframe by (weight descending, index ascending)
};

struct LocalWindow {
  std::vector<uint64_t> kf_frame_id;
  std::vector<double> kf_R, kf_t;              // 9 / 3 per keyframe
  std::vector<uint8_t> kf_fixed;
  std::vector<int32_t> kf_weight;
  std::vector<float> obs_px;                   // 2 per observation
  std::vector<uint64_t> obs_landmark_id, obs_frame_id;
  std::vector<int32_t> obs_class, obs_lm_index;
  std::vector<uint64_t> lm_id;
  std::vector<int32_t> lm_class;
  std::vector<float> lm_xyz;                   // 3 per landmark
  int n_left_out = 0;
};

namespace covis_detail {
inline void check(dvs_status s, const char* what) {
  if (s != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
}
}  // namespace covis_detail

inline CovisGraph covisibilityGraph(MappingBackend& map, int min_weight = 15, bool want_weights = true) {
  CovisGraph g;
  int32_t n = 0;
  int64_t m = 0;
  covis_detail::check(dvs_backend_covisibility(map.handle(), min_weight, 0, 0, nullptr, nullptr, nullptr, nullptr, &n, &m), "dvs_backend_covisibility");
  g.n = n;
  if (want_weights) g.weights.resize((size_t)n * (size_t)n);
  g.nb_offsets.resize((size_t)n + 1); g.nb_index.resize((size_t)m); g.nb_weight.resize((size_t)m);
  covis_detail::check(dvs_backend_covisibility(map.handle(), min_weight, n, m, want_weights ? g.weights.data() : nullptr, g.nb_offsets.data(), g.nb_index.data(),
                                               g.nb_weight.data(), &n, &m),
                      "dvs_backend_covisibility");
  return g;
}

inline LocalWindow localWindow(MappingBackend& map, uint64_t ref_frame_id, const CovisParams& params = CovisParams()) {
  LocalWindow w;
  int32_t nk = 0, no = 0, nl = 0, left = 0;
  covis_detail::check(dvs_backend_get_local_window(map.handle(), ref_frame_id, &params, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &nk, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, &no, nullptr, nullptr, nullptr, &nl, &left),
                      "dvs_backend_get_local_window");
  w.kf_frame_id.resize((size_t)nk); w.kf_R.resize(9 * (size_t)nk); w.kf_t.resize(3 * (size_t)nk); w.kf_fixed.resize((size_t)nk); w.kf_weight.resize((size_t)nk);
  w.obs_px.resize(2 * (size_t)no); w.obs_landmark_id.resize((size_t)no); w.obs_frame_id.resize((size_t)no); w.obs_class.resize((size_t)no);
  w.obs_lm_index.resize((size_t)no);
  w.lm_id.resize((size_t)nl); w.lm_class.resize((size_t)nl); w.lm_xyz.resize(3 * (size_t)nl);
  covis_detail::check(dvs_backend_get_local_window(map.handle(), ref_frame_id, &params, nk, no, nl, w.kf_frame_id.data(), w.kf_R.data(), w.kf_t.data(), w.kf_fixed.data(),
                                                   w.kf_weight.data(), &nk, w.obs_px.data(), w.obs_landmark_id.data(), w.obs_class.data(), w.obs_frame_id.data(),
                                                   w.obs_lm_index.data(), &no, w.lm_id.data(), w.lm_class.data(), w.lm_xyz.data(), &nl, &left),
                      "dvs_backend_get_local_window");
  w.n_left_out = left;
  return w;
}

// the map changes if and only if the returned summary.termination == 0 (CONVERGENCE)
inline dvs_backend_lba_result localBundleAdjust(MappingBackend& map, GlobalBA& solver, uint64_t ref_frame_id, const CovisParams& params = CovisParams()) {
  dvs_backend_lba_result out;
  covis_detail::check(dvs_backend_local_ba(map.handle(), solver.handle(), ref_frame_id, &params, &out), "dvs_backend_local_ba");
  return out;
}

// d_kps / d_desc: device pointers, as MapTracker's device forms take them; tracker.matches() then reports rows of the local map
inline dvs_maptrack_result trackFrameLocal(MappingBackend& map, MapTracker& tracker, uint64_t ref_frame_id, const dvs_keypoint* d_kps, const uint8_t* d_desc, int n_kp,
                                           const double* R9, const double* t3, const CovisParams& params = CovisParams()) {
  dvs_maptrack_result out;
  covis_detail::check(dvs_backend_track_frame_local(map.handle(), tracker.handle(), ref_frame_id, &params, d_kps, d_desc, n_kp, R9, t3, &out),
                      "dvs_backend_track_frame_local");
  return out;
}

}  // namespace dvslam
