// The cv-typed knnMatch / radiusMatch / crossCheck match() of dvslam::HammingBFMatcher (include/dvslam/bf_matcher.hpp), driven the
// way a cv::BFMatcher(NORM_HAMMING[, true]) caller would, against the test-only stand-ins of tests/cpp/stubs.  Reads descriptors
// (int32 nq, int32 nt, nq x 32 bytes, nt x 32 bytes) from argv[1] and writes every result to argv[2] as text for
// tests/test_gpu_match_modes.py, which checks it against the numpy reference: the adapter's padding removal and compaction included.
// Exit 0 = ok, 3 = no GPU (compiled, nothing run).
#define DVSLAM_WITH_OPENCV 1
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
#include "dvslam/bf_matcher.hpp"

static void dump(FILE* f, const char* name, const std::vector<std::vector<cv::DMatch>>& m) {
  std::fprintf(f, "BEGIN %s %zu\n", name, m.size());
  for (const auto& row : m) {
    std::fprintf(f, "R %zu\n", row.size());
    for (const cv::DMatch& d : row) std::fprintf(f, "%d %d %d %.1f\n", d.queryIdx, d.trainIdx, d.imgIdx, (double)d.distance);
  }
}

static bool throws(void (*fn)(const cv::Mat&, const cv::Mat&), const cv::Mat& q, const cv::Mat& t) {
  try { fn(q, t); } catch (const std::exception&) { return true; }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: bf_matcher_modes in.bin out.txt\n"); return 2; }
  if (dvs_device_count() < 1) { std::printf("no device: bf_matcher_modes compiled, nothing run\n"); return 3; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t n[2];
  if (std::fread(n, 4, 2, in) != 2) return 2;
  cv::Mat query(n[0], 32, CV_8U), train(n[1], 32, CV_8U);
  if (std::fread(query.data, 32, (size_t)n[0], in) != (size_t)n[0] || std::fread(train.data, 32, (size_t)n[1], in) != (size_t)n[1]) return 2;
  std::fclose(in);
  FILE* out = std::fopen(argv[2], "w");
  if (!out) return 2;

  dvslam::HammingBFMatcher matcher(cv::NORM_HAMMING);
  std::vector<std::vector<cv::DMatch>> m;
  for (int k : {1, 2, 3, 5, n[1] + 3}) {
    matcher.knnMatch(query, train, m, k);
    dump(out, ("knn" + std::to_string(k)).c_str(), m);
  }
  matcher.knnMatch(query, train, m, 2, cv::Mat(), true);
  dump(out, "knn2c", m);
  for (float r : {-1.f, 0.f, 63.5f, 100.f, 256.f, NAN}) {
    matcher.radiusMatch(query, train, m, r);
    dump(out, ("radius" + std::to_string((int)std::floor(std::isnan(r) ? -7.f : r))).c_str(), m);
    matcher.radiusMatch(query, train, m, r, cv::noArray(), true);
    dump(out, ("radiusc" + std::to_string((int)std::floor(std::isnan(r) ? -7.f : r))).c_str(), m);
  }
  std::vector<cv::DMatch> one;
  matcher.match(query, train, one);
  dump(out, "match", {one});

  dvslam::HammingBFMatcher cross(cv::NORM_HAMMING, true);
  cross.match(query, train, one);   // DescriptorMatcher::match: only the mutual pairs, in query order
  dump(out, "cross", {one});
  cross.knnMatch(query, train, m, 1);
  dump(out, "crossknn", m);
  cross.knnMatch(query, train, m, 1, cv::noArray(), true);
  dump(out, "crossknnc", m);
  cross.radiusMatch(query, train, m, 100.f);   // radiusMatch never reads crossCheck
  dump(out, "crossradius100", m);

  // refused: k != 1 with crossCheck, a non-empty mask, k = 0
  static dvslam::HammingBFMatcher* xs = &cross;
  static dvslam::HammingBFMatcher* ps = &matcher;
  std::vector<std::vector<cv::DMatch>> sink;
  const bool t1 = throws([](const cv::Mat& q, const cv::Mat& t) { std::vector<std::vector<cv::DMatch>> s; xs->knnMatch(q, t, s, 2); }, query, train);
  const bool t2 = throws([](const cv::Mat& q, const cv::Mat& t) {
    std::vector<std::vector<cv::DMatch>> s;
    cv::Mat mask(q.rows, t.rows, CV_8U);
    ps->knnMatch(q, t, s, 2, mask);
  }, query, train);
  const bool t3 = throws([](const cv::Mat& q, const cv::Mat& t) { std::vector<std::vector<cv::DMatch>> s; ps->knnMatch(q, t, s, 0); }, query, train);
  std::fprintf(out, "THROWS %d %d %d\n", (int)t1, (int)t2, (int)t3);
  std::fclose(out);
  std::printf("bf_matcher_modes ok\n");
  return 0;
}
