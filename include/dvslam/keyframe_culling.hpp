// dvslam/keyframe_culling.hpp — header-only C++ adapter over the "Keyframe culling" section of dvslam_hip.h (INTEGRATION.md "Keyframe
// culling"): redundant keyframes leave the map a MappingBackend keeps on the device.  cullKeyframes(map, params, protectedIds, apply) walks
// every keyframe; the overload with ref_frame_id walks only the covisibility neighbours of that keyframe (local scope: params.local is set
// by the overload chosen, whatever the caller put there).  A caller who keeps a loop database removes report.culled_frame_id from it.
// Errors throw std::runtime_error.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "mapping_backend.hpp"

namespace dvslam {

struct CullParams : dvs_cull_params {
  CullParams() { dvs_cull_default_params(this); }
};

struct CullReport {
  dvs_cull_result result{};
  std::vector<uint64_t> culled_frame_id;       // ascending index in the table before the call
  std::vector<int32_t> kf_observed;            // per keyframe of the table before the call: n_k
  std::vector<int32_t> kf_redundant;           //   R_k under the initial counts
  std::vector<uint8_t> kf_state;               //   0 out of scope, 1 protected, 2 kept, 3 culled
};

namespace cull_detail {
inline CullReport run(MappingBackend& map, uint64_t ref_frame_id, dvs_cull_params p, const std::vector<uint64_t>& protectedIds, bool apply) {
  CullReport r;
  dvs_backend_count c;
  dvs_status s = dvs_backend_counts(map.handle(), &c);
  if (s != DVS_OK) throw std::runtime_error(std::string("dvs_backend_counts: ") + dvs_last_error());
  int32_t n = (int32_t)c.n_keyframes;
  r.culled_frame_id.resize((size_t)n); r.kf_observed.resize((size_t)n); r.kf_redundant.resize((size_t)n); r.kf_state.resize((size_t)n);
  s = dvs_backend_cull_keyframes(map.handle(), ref_frame_id, &p, protectedIds.empty() ? nullptr : protectedIds.data(), (int32_t)protectedIds.size(), apply ? 1 : 0, &r.result,
                                 n, r.culled_frame_id.data(), r.kf_observed.data(), r.kf_redundant.data(), r.kf_state.data(), &n);
  if (s != DVS_OK) throw std::runtime_error(std::string("dvs_backend_cull_keyframes: ") + dvs_last_error());
  r.culled_frame_id.resize((size_t)r.result.n_culled);
  return r;
}
}  // namespace cull_detail

// every keyframe is in scope
inline CullReport cullKeyframes(MappingBackend& map, const CullParams& params = CullParams(), const std::vector<uint64_t>& protectedIds = {}, bool apply = true) {
  dvs_cull_params p = params;
  p.local = 0;
  return cull_detail::run(map, 0, p, protectedIds, apply);
}

// local scope: only the keyframes of N(ref_frame_id; params.min_weight) are in scope, and ref_frame_id itself is protected
inline CullReport cullKeyframes(MappingBackend& map, uint64_t ref_frame_id, const CullParams& params = CullParams(), const std::vector<uint64_t>& protectedIds = {},
                                bool apply = true) {
  dvs_cull_params p = params;
  p.local = 1;
  return cull_detail::run(map, ref_frame_id, p, protectedIds, apply);
}

}  // namespace dvslam
