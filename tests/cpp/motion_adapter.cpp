// dvslam::MotionSegmenter (include/dvslam/motion_segmentation.hpp) and TrackingFrontend::setMotionMask / motionMask over a sequence read
// from a file of {gray frame rows * cols bytes, depth frame rows * cols uint16} records:
//   motion_adapter <sequence.bin> <rows> <cols> <n> <focal> <lag>
// Line "seg": the statistics and the CRC-32 of the mask of frame n - 1 against frame 0 under the identity pose.  Then one line per frame
// of the tracker with the mask on: index, counts, the reference's index, the mask statistics and CRC-32, the relative pose as the hex of
// its bits.  tests/test_cpp_motion.py holds the text against the Python mirror's.  Exit code 0 = ok, 3 = no GPU, 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dvslam/motion_segmentation.hpp"
#include "dvslam/tracking_frontend.hpp"

static_assert(sizeof(dvs_motion_params) == 72 && sizeof(dvs_motion_stats) == 24, "the ctypes mirror (dvslam_amd/motion.py) assumes these sizes");
static_assert(sizeof(dvs_tracker_params) == 200 && sizeof(dvs_track_result) == 248, "the tracker's structs do not change");

static uint32_t crc32_of(const std::vector<uint8_t>& v) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint8_t b : v) {
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

static void print_stats(const dvs_motion_stats& s) {
  std::printf("stats=%d,%d,%d,%d,%d,%d", s.n_valid, s.n_seed, s.n_components, s.n_components_kept, s.n_dynamic, s.n_masked);
}

int main(int argc, char** argv) {
  const dvs_motion_params d = dvslam::MotionSegmenter::defaultParams(480, 640, 600, 600, 320, 240);
  if (d.min_depth_mm != 300 || d.max_depth_mm != 3000 || d.min_area != 200 || d.dilate_radius != 8 || d.tau0_m != 0.03 || d.tau2_per_m != 0.005) return 1;
  if (dvs_device_count() < 1) { std::printf("no device: adapter compiled, nothing run\n"); return 3; }
  if (argc < 7) { std::fprintf(stderr, "usage: motion_adapter sequence.bin rows cols n focal lag\n"); return 2; }
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n = std::atoi(argv[4]), lag = std::atoi(argv[6]);
  const double f = std::atof(argv[5]);
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh || n < 2) return 2;
  const size_t px = (size_t)rows * cols;
  std::vector<std::vector<uint8_t>> img((size_t)n, std::vector<uint8_t>(px));
  std::vector<std::vector<uint16_t>> depth((size_t)n, std::vector<uint16_t>(px));
  for (int t = 0; t < n; t++)
    if (std::fread(img[t].data(), 1, px, fh) != px || std::fread(depth[t].data(), 2, px, fh) != px) return 2;
  std::fclose(fh);
  std::vector<uint8_t> mask;
  {
    dvslam::MotionSegmenter seg(dvslam::MotionSegmenter::defaultParams(rows, cols, f, f, cols / 2.0, rows / 2.0));
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
    const dvs_motion_stats s = seg.segment(depth[0].data(), (size_t)cols * 2, depth[n - 1].data(), (size_t)cols * 2, I, z, mask);
    std::printf("seg ");
    print_stats(s);
    std::printf(" crc=%u\n", crc32_of(mask));
  }
  dvslam::TrackingFrontend fe(dvslam::TrackingFrontend::defaultParams(rows, cols, f, f, cols / 2.0, rows / 2.0));
  dvs_motion_params mp;
  dvs_motion_default_params(&mp);
  fe.setMotionMask(&mp, lag);
  for (int t = 0; t < n; t++) {
    const dvslam::TrackResult tr = fe.track(img[t].data(), 1, (size_t)cols, depth[t].data(), (size_t)cols * 2, t, 0);
    double R[9], tt[3];
    dvs_motion_stats s;
    const long long ref = (long long)fe.motionMask(mask, R, tt, &s);
    std::printf("%lld n=%d,%d,%d upd=%d ref=%lld ", (long long)tr.r.frame_index, tr.r.n_extracted, tr.r.n_filtered, tr.r.n_backend, tr.r.pose_updated, ref);
    print_stats(s);
    std::printf(" crc=%u pose=", crc32_of(mask));
    for (int k = 0; k < 12; k++) {
      const double v = k < 9 ? R[k] : tt[k - 9];
      unsigned long long u;
      std::memcpy(&u, &v, 8);
      std::printf("%016llx%s", u, k == 11 ? "\n" : " ");
    }
  }
  fe.setMotionMask(nullptr);
  return 0;
}
