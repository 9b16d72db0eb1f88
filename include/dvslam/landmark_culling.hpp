// dvslam/landmark_culling.hpp — header-only C++ adapter over the "Landmark culling" section of dvslam_hip.h (INTEGRATION.md "Landmark
// culling"): the tracking statistics a MappingBackend records per landmark and the cull that reads them.  setTrackingStats(map, true)
// makes the backend's map-tracking calls record; landmarkStats / setLandmarkStats / clearLandmarkStats read, restore and clear the
// counters; cullLandmarks(map, params, apply) removes the landmarks that are predicted and never found, and the weak ones.
// Errors throw std::runtime_error.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "mapping_backend.hpp"

namespace dvslam {

struct LandmarkCullParams : dvs_lm_cull_params {
  LandmarkCullParams() { dvs_lm_cull_default_params(this); }
};

struct LandmarkCullReport {
  dvs_lm_cull_result result{};
  std::vector<uint64_t> culled_id;             // ascending
  std::vector<int32_t> culled_reason;          // 1: found ratio, 2: weak
};

struct LandmarkStats {                         // rows as the landmark table
  std::vector<uint64_t> id;
  std::vector<int32_t> visible, found, n_views, age_kf;
  int64_t n_frames_recorded = 0;
};

namespace lm_cull_detail {
inline void check(dvs_status s, const char* what) {
  if (s != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
}
}  // namespace lm_cull_detail

inline void setTrackingStats(MappingBackend& map, bool on) { lm_cull_detail::check(dvs_backend_set_tracking_stats(map.handle(), on ? 1 : 0), "dvs_backend_set_tracking_stats"); }

inline void clearLandmarkStats(MappingBackend& map) { lm_cull_detail::check(dvs_backend_clear_landmark_stats(map.handle()), "dvs_backend_clear_landmark_stats"); }

inline LandmarkStats landmarkStats(MappingBackend& map) {
  LandmarkStats r;
  int32_t n = 0;
  lm_cull_detail::check(dvs_backend_get_landmark_stats(map.handle(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n, &r.n_frames_recorded), "dvs_backend_get_landmark_stats");
  r.id.resize((size_t)n); r.visible.resize((size_t)n); r.found.resize((size_t)n); r.n_views.resize((size_t)n); r.age_kf.resize((size_t)n);
  if (n > 0)
    lm_cull_detail::check(dvs_backend_get_landmark_stats(map.handle(), n, r.id.data(), r.visible.data(), r.found.data(), r.n_views.data(), r.age_kf.data(), &n, nullptr),
                          "dvs_backend_get_landmark_stats");
  return r;
}

// ids strictly ascending; ids the map does not hold are skipped
inline void setLandmarkStats(MappingBackend& map, const std::vector<uint64_t>& id, const std::vector<int32_t>& visible, const std::vector<int32_t>& found) {
  if (id.size() != visible.size() || id.size() != found.size()) throw std::runtime_error("setLandmarkStats: one row per id");
  lm_cull_detail::check(dvs_backend_set_landmark_stats(map.handle(), (int32_t)id.size(), id.data(), visible.data(), found.data()), "dvs_backend_set_landmark_stats");
}

inline LandmarkCullReport cullLandmarks(MappingBackend& map, const LandmarkCullParams& params = LandmarkCullParams(), bool apply = true) {
  LandmarkCullReport r;
  const dvs_lm_cull_params p = params;
  int32_t n = 0;
  lm_cull_detail::check(dvs_backend_cull_landmarks(map.handle(), &p, 0, nullptr, 0, nullptr, nullptr, &n), "dvs_backend_cull_landmarks");   // a dry run for the count
  r.culled_id.resize((size_t)n); r.culled_reason.resize((size_t)n);
  lm_cull_detail::check(dvs_backend_cull_landmarks(map.handle(), &p, apply ? 1 : 0, &r.result, n, r.culled_id.data(), r.culled_reason.data(), &n), "dvs_backend_cull_landmarks");
  r.culled_id.resize((size_t)n); r.culled_reason.resize((size_t)n);
  return r;
}

}  // namespace dvslam
