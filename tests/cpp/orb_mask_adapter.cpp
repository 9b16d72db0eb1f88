// The keep-mask surface of the C++ adapters (include/dvslam/orb_extractor.hpp): ORB_SLAM3::ORBextractor::honourMask and the masked
// dvslam::OrbExtractor overload, driven the way the reference's frontend calls operator() (frontend.cpp:1094), against the test-only
// stand-ins of tests/cpp/stubs.  Reads (int32 rows, int32 cols, rows x cols image bytes, rows x cols mask bytes) from argv[1] and writes
// every result to argv[2] as text for tests/test_gpu_orb_mask.py, which checks it against the Python mirror and the reference.
// Exit 0 = ok, 3 = no GPU (compiled, nothing run).
#define DVSLAM_WITH_OPENCV 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include <opencv2/core/core.hpp>
#include "dynamic_visual_slam/ORBextractor.hpp"

static void dump(FILE* f, const char* name, const std::vector<cv::KeyPoint>& k, const uint8_t* desc) {
  std::fprintf(f, "BEGIN %s %zu\n", name, k.size());
  for (size_t i = 0; i < k.size(); i++) {
    const float v[5] = {k[i].pt.x, k[i].pt.y, k[i].size, k[i].angle, k[i].response};
    uint32_t u[5];
    std::memcpy(u, v, sizeof(u));
    std::fprintf(f, "%08x %08x %08x %08x %08x %d %d ", u[0], u[1], u[2], u[3], u[4], k[i].octave, k[i].class_id);
    for (int b = 0; b < 32; b++) std::fprintf(f, "%02x", desc[i * 32 + b]);
    std::fprintf(f, "\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: orb_mask_adapter in.bin out.txt\n"); return 2; }
  if (dvs_device_count() < 1) { std::printf("no device: orb_mask_adapter compiled, nothing run\n"); return 3; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t rc[2];
  if (std::fread(rc, 4, 2, in) != 2) return 2;
  const int rows = rc[0], cols = rc[1];
  cv::Mat image(rows, cols, CV_8UC1), mask(rows, cols, CV_8UC1);
  if (std::fread(image.data, 1, image.total(), in) != image.total() || std::fread(mask.data, 1, mask.total(), in) != mask.total()) return 2;
  std::fclose(in);
  FILE* out = std::fopen(argv[2], "w");
  if (!out) return 2;

  ORB_SLAM3::ORBextractor ex(2000, 1.2f, 8, 20, 7);
  ex.keepImagePyramid(false);
  std::vector<int> lapping = {0, 0};
  std::vector<cv::KeyPoint> kps;
  cv::Mat desc;
  // default: the mask is ignored, as in the reference
  ex(image, mask, kps, desc, lapping);
  dump(out, "off", kps, desc.data);
  ex.honourMask(true);
  ex(image, mask, kps, desc, lapping);
  dump(out, "on", kps, desc.data);
  ex(image, cv::noArray(), kps, desc, lapping);   // honoured, but no mask given: the unmasked call
  dump(out, "on_nomask", kps, desc.data);
  int throws = 0;
  try { cv::Mat small(rows - 1, cols, CV_8UC1); ex(image, small, kps, desc, lapping); } catch (const std::exception&) { throws |= 1; }
  try { cv::Mat f32(rows, cols, CV_32F); ex(image, f32, kps, desc, lapping); } catch (const std::exception&) { throws |= 2; }
  ex.honourMask(false);
  try { cv::Mat small(rows - 1, cols, CV_8UC1); ex(image, small, kps, desc, lapping); } catch (const std::exception&) { throws |= 4; }
  std::fprintf(out, "THROWS %d\n", throws);

  // the plain-pointer overload with a padded mask (mask_step > cols)
  dvslam::OrbExtractor raw(2000, 1.2f, 8, 20, 7);
  const size_t mstep = (size_t)cols + 9;
  std::vector<uint8_t> padded((size_t)rows * mstep, 0);
  for (int y = 0; y < rows; y++) std::memcpy(&padded[(size_t)y * mstep], mask.data + (size_t)y * mask.step, (size_t)cols);
  std::vector<dvs_keypoint> rk;
  std::vector<uint8_t> rd;
  const int n = raw(image.data, rows, cols, image.step, padded.data(), mstep, rk, rd);
  std::vector<cv::KeyPoint> ck;
  for (int i = 0; i < n; i++) ck.emplace_back(rk[i].x, rk[i].y, rk[i].size, rk[i].angle, rk[i].response, rk[i].octave, rk[i].class_id);
  dump(out, "raw", ck, rd.data());
  bool bad_step = false;
  try { raw(image.data, rows, cols, image.step, padded.data(), (size_t)cols - 1, rk, rd); } catch (const std::exception&) { bad_step = true; }
  std::fprintf(out, "BADSTEP %d\n", bad_step ? 1 : 0);
  std::fclose(out);
  return 0;
}
