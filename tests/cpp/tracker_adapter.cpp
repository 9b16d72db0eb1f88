// dvslam::TrackingFrontend (include/dvslam/tracking_frontend.hpp) over a sequence of gray frames read from a file:
//   tracker_adapter <frames.bin> <rows> <cols> <n> <focal> <depth_mm>
// One line per frame: index, keyframe flag / id / criterion, the counts, pose_updated, payload size and CRC-32, R_ and t_ as the hex of
// their bits.  tests/test_gpu_tracker.py holds the text against the Python mirror's.  Exit code 0 = ok, 3 = no GPU, 2 = usage.
// With -DDVSLAM_WITH_OPENCV (test stubs on the include path) the cv::Mat overload must compile as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dvslam/tracking_frontend.hpp"

static_assert(sizeof(dvs_tracker_params) == 200 && sizeof(dvs_track_result) == 248, "the ctypes mirror (dvslam_amd/tracker.py) assumes these sizes");

static uint32_t crc32_of(const std::vector<uint8_t>& v) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint8_t b : v) {
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

#ifdef DVSLAM_WITH_OPENCV
static dvslam::TrackResult (dvslam::TrackingFrontend::*const kMatOverload)(const cv::Mat&, const cv::Mat&, int32_t, uint32_t) = &dvslam::TrackingFrontend::track;
#endif

int main(int argc, char** argv) {
#ifdef DVSLAM_WITH_OPENCV
  (void)kMatOverload;
#endif
  dvs_tracker_params d = dvslam::TrackingFrontend::defaultParams(480, 640, 600, 600, 320, 240);
  if (d.orb.nfeatures != 1000 || d.kf_min_matches != 150 || d.cull_max_new != 200) return 1;
  if (dvs_device_count() < 1) { std::printf("no device: adapter compiled, nothing run\n"); return 3; }
  if (argc < 7) { std::fprintf(stderr, "usage: tracker_adapter frames.bin rows cols n focal depth_mm\n"); return 2; }
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n = std::atoi(argv[4]);
  const double f = std::atof(argv[5]);
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return 2;
  std::vector<uint8_t> img((size_t)rows * cols);
  std::vector<uint16_t> depth((size_t)rows * cols, (uint16_t)std::atoi(argv[6]));
  dvslam::TrackingFrontend fe(dvslam::TrackingFrontend::defaultParams(rows, cols, f, f, cols / 2.0, rows / 2.0));
  for (int t = 0; t < n; t++) {
    if (std::fread(img.data(), 1, img.size(), fh) != img.size()) return 2;
    const dvslam::TrackResult tr = fe.track(img.data(), 1, (size_t)cols, depth.data(), (size_t)cols * 2, t, 0);
    const dvs_track_result& r = tr.r;
    std::printf("%lld kf=%d id=%lld crit=%d n=%d,%d,%d,%d,%d,%d,%d upd=%d cdr=%zu,%u pose=", (long long)r.frame_index, r.is_keyframe, (long long)r.keyframe_id,
                r.kf_criterion, r.n_extracted, r.n_filtered, r.n_matches, r.n_geometric, r.n_pnp_points, r.n_pnp_inliers, r.n_backend, r.pose_updated,
                tr.payload.size(), tr.payload.empty() ? 0u : crc32_of(tr.payload));
    for (int k = 0; k < 12; k++) {
      const double v = k < 9 ? r.R[k] : r.t[k - 9];
      unsigned long long u;
      std::memcpy(&u, &v, 8);
      std::printf("%016llx%s", u, k == 11 ? "\n" : " ");
    }
  }
  std::fclose(fh);
  return 0;
}
