// dvslam::SlidingWindowBA::setDeviceWindow on the 20-keyframe window of adapter_smoke.cpp: `default` leaves the object as constructed
// (19 free keyframes > 16: host solver, one line on stderr), `window` raises the device window to 63 first (device solver, silent).
// Prints "solver=<n> cost=<%.17g>".  Exit code 0 = ok, 3 = no GPU.  With -DDVSLAM_WITH_OPENCV (and the test stubs on the include path)
// the reference-named class must carry the same member.
#include <cmath>
#include <cstdio>
#include <cstring>
#ifdef DVSLAM_WITH_OPENCV
#include "dynamic_visual_slam/bundle_adjustment.hpp"
static void (SlidingWindowBA::*const kReferenceNamedMember)(int) = &SlidingWindowBA::setDeviceWindow;
#endif
#include "dvslam/sliding_window_ba.hpp"

int main(int argc, char** argv) {
#ifdef DVSLAM_WITH_OPENCV
  SlidingWindowBA named(900.0, 900.0, 640.0, 360.0);
  (named.*kReferenceNamedMember)(63);
#endif
  const bool wide = argc > 1 && std::strcmp(argv[1], "window") == 0;
  if (dvs_device_count() < 1) { std::printf("no device: adapter compiled, nothing run\n"); return 3; }
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::vector<dvslam::Landmark> lms;
  for (int i = 0; i < 30; i++) lms.emplace_back(100 + i, "unlabeled", -1.0 + 0.07 * i, 0.5 * std::sin(0.7 * i), 3.0 + 0.05 * i);
  std::vector<dvslam::KeyframeData> kf20;
  std::vector<dvslam::Observation> obs20;
  for (int c = 0; c < 20; c++) {
    const double tc[3] = {-0.05 * c, 0, 0};
    kf20.emplace_back(100 + c, I, tc);
    for (int i = 0; i < 30; i++) {
      const double X = -1.0 + 0.07 * i, Y = 0.5 * std::sin(0.7 * i), Z = 3.0 + 0.05 * i;
      obs20.emplace_back(900 * (X - 0.05 * c) / Z + 640 + 0.3 * std::sin(1.3 * i + c), 900 * Y / Z + 360 + 0.3 * std::cos(0.9 * i + 2 * c), 100 + i, "unlabeled", 100 + c);
    }
  }
  dvslam::SlidingWindowBA ba(900, 900, 640, 360);
  if (wide) ba.setDeviceWindow(63);
  dvslam::OptimizationResult r = ba.optimize(kf20, lms, obs20, 10);
  std::printf("solver=%d cost=%.17g success=%d poses=%d\n", ba.last_linear_solver(), r.final_cost, (int)r.success, (int)r.optimized_poses.size());
  if (r.optimized_poses.size() != 20 || ba.last_linear_solver() != (wide ? 1 : 2) || !(r.final_cost < 30.0)) return 1;
  return 0;
}
