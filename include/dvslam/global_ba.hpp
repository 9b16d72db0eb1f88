// dvslam/global_ba.hpp — header-only C++ adapter over dvs_backend_global_ba of dvslam_hip.h ("Global BA of the map"; INTEGRATION.md "Loop
// closure"): every keyframe and landmark of the map a MappingBackend keeps on the device refined by dvs_ba_solve_global — the step that
// follows closeLoop() (loop_closing.hpp).  GlobalBA owns the solver handle (a stream, pinned blocks and grow-only arenas: keep one for the
// life of the map); globalBundleAdjust() assembles the problem, solves it and, if the solve converged, writes poses and positions back.
// Errors throw std::runtime_error.
#pragma once
#include <stdexcept>
#include <string>
#include "../dvslam_hip.h"
#include "mapping_backend.hpp"

namespace dvslam {

struct GlobalBaParams : dvs_ba_global_params {
  GlobalBaParams() { dvs_ba_default_global_params(this); }
};

class GlobalBA {
 public:
  explicit GlobalBA(int device = 0) {
    if (dvs_ba_create(device, &h_) != DVS_OK) throw std::runtime_error(std::string("dvs_ba_create: ") + dvs_last_error());
  }
  ~GlobalBA() { dvs_ba_destroy(h_); }
  GlobalBA(const GlobalBA&) = delete;
  GlobalBA& operator=(const GlobalBA&) = delete;
  dvs_ba* handle() const { return h_; }
  GlobalBaParams& params() { return params_; }
  const GlobalBaParams& params() const { return params_; }

 private:
  dvs_ba* h_ = nullptr;
  GlobalBaParams params_;
};

// the map changes if and only if the returned summary.ba.termination == 0 (CONVERGENCE)
inline dvs_backend_gba_result globalBundleAdjust(MappingBackend& map, GlobalBA& solver) {
  dvs_backend_gba_result out;
  if (dvs_backend_global_ba(map.handle(), solver.handle(), &solver.params(), &out) != DVS_OK)
    throw std::runtime_error(std::string("dvs_backend_global_ba: ") + dvs_last_error());
  return out;
}

}  // namespace dvslam
