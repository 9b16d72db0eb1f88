// dvslam/landmark_refresh.hpp — header-only C++ adapter over the "Landmark refresh" section of dvslam_hip.h (INTEGRATION.md "Landmark
// refresh"): refreshLandmarks(map, params) re-selects every landmark's descriptor from its views (the overload with a frame id: only the
// landmarks that keyframe observes — the per-keyframe use), landmarkGeometry(map) reads the viewing geometry and the selection without
// touching the map, trackFrameGated(map, tracker, ...) is MapTracker::trackFrame with the distance and viewing-angle gates.
// Errors throw std::runtime_error.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "map_tracking.hpp"
#include "mapping_backend.hpp"

namespace dvslam {

struct LandmarkRefreshParams : dvs_lm_refresh_params {
  LandmarkRefreshParams() { dvs_lm_refresh_default_params(this); }
};
struct MapTrackGates : dvs_maptrack_gates {
  MapTrackGates() { dvs_mapgate_default_gates(this); }
};

struct LandmarkGeometry {                      // one entry per landmark row, rows as dvs_backend_get_landmarks
  std::vector<std::array<double, 3>> normal;   // the mean viewing direction, not re-normalised
  std::vector<std::array<double, 2>> range;    // dmin, dmax
  std::vector<int32_t> n_counted;              // m
  std::vector<uint64_t> best_obs_id;           // the chosen view's observation id, UINT64_MAX without a view
  std::vector<int32_t> best_median;            // its median distance to the landmark's views, -1 without a view
};

inline dvs_lm_refresh_result refreshLandmarks(MappingBackend& map, const LandmarkRefreshParams& params = LandmarkRefreshParams()) {
  dvs_lm_refresh_params p = params;
  dvs_lm_refresh_result r{};
  if (dvs_backend_refresh_landmarks(map.handle(), &p, &r) != DVS_OK) throw std::runtime_error(std::string("dvs_backend_refresh_landmarks: ") + dvs_last_error());
  return r;
}

// only the landmarks keyframe scope_frame_id observes
inline dvs_lm_refresh_result refreshLandmarks(MappingBackend& map, uint64_t scope_frame_id, const LandmarkRefreshParams& params = LandmarkRefreshParams()) {
  LandmarkRefreshParams p = params;
  p.use_scope = 1; p.scope_frame_id = scope_frame_id;
  return refreshLandmarks(map, p);
}

inline LandmarkGeometry landmarkGeometry(MappingBackend& map) {
  LandmarkGeometry g;
  int32_t n = 0;
  if (dvs_backend_get_landmark_geometry(map.handle(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n) != DVS_OK)
    throw std::runtime_error(std::string("dvs_backend_get_landmark_geometry: ") + dvs_last_error());
  g.normal.resize((size_t)n); g.range.resize((size_t)n); g.n_counted.resize((size_t)n); g.best_obs_id.resize((size_t)n); g.best_median.resize((size_t)n);
  if (n == 0) return g;
  if (dvs_backend_get_landmark_geometry(map.handle(), n, g.normal[0].data(), g.range[0].data(), g.n_counted.data(), g.best_obs_id.data(), g.best_median.data(), &n) != DVS_OK)
    throw std::runtime_error(std::string("dvs_backend_get_landmark_geometry: ") + dvs_last_error());
  return g;
}

// a frame's device keypoints against the map's landmark table as it stands, landmarks outside the gates left out; the map is not modified.
// counts (nullable): what the near, far, back-facing and angle tests removed
inline dvs_maptrack_result trackFrameGated(MappingBackend& map, MapTracker& tracker, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9,
                                           const double* t3, const MapTrackGates& gates = MapTrackGates(), std::array<int32_t, 4>* counts = nullptr) {
  dvs_maptrack_gates g = gates;
  dvs_maptrack_result r;
  if (dvs_backend_track_frame_gated(map.handle(), tracker.handle(), &g, d_kps, d_desc, n_kp, R9, t3, &r) != DVS_OK)
    throw std::runtime_error(std::string("dvs_backend_track_frame_gated: ") + dvs_last_error());
  if (counts && dvs_mapgate_get_counts(tracker.handle(), counts->data()) != DVS_OK)
    throw std::runtime_error(std::string("dvs_mapgate_get_counts: ") + dvs_last_error());
  return r;
}

}  // namespace dvslam
