// dvslam/bf_matcher.hpp — adapter with the call surface of cv::BFMatcher(cv::NORM_HAMMING, false).match as the
// reference uses it (src/frontend.cpp:220,614,1123; src/backend.cpp:222,1072) over the C-ABI.
//   dvslam::BFMatcher::match(q, nq, t, nt, matches)      plain pointers + dvslam::DMatch
//   (DVSLAM_WITH_OPENCV) match(const cv::Mat&, const cv::Mat&, std::vector<cv::DMatch>&)
// plus matchBelow() for the backend's association loop (backend.cpp:1068-1077): all (query, train) pairs with
// distance < max_dist in one launch instead of N_obs x N_landmarks 1x1 match() calls.
// The rest of the drop-in: crossCheck, knnMatch(k) and radiusMatch(maxDistance), plain-pointer and cv-typed.
// Masks, several train sets (add/train, imgIdx != 0) and other norms are refused.
#pragma once
#include <climits>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#ifdef DVSLAM_WITH_OPENCV
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
#endif

namespace dvslam {

struct DMatch {  // cv::DMatch layout
  int queryIdx, trainIdx, imgIdx;
  float distance;
};

class BFMatcher {
 public:
  explicit BFMatcher(int device = 0, bool crossCheck = false) : cross_(crossCheck) {
    if (dvs_matcher_create(device, &m_) != DVS_OK) throw std::runtime_error(std::string("dvs_matcher_create: ") + dvs_last_error());
  }
  ~BFMatcher() { dvs_matcher_destroy(m_); }
  BFMatcher(const BFMatcher&) = delete;
  BFMatcher& operator=(const BFMatcher&) = delete;

  // one DMatch per query row in query order; empty train set -> empty result (cv behaviour).  crossCheck: only the mutual pairs, in
  // query order (DescriptorMatcher::match is knnMatch(k = 1, compactResult = true))
  void match(const uint8_t* query, int nq, const uint8_t* train, int nt, std::vector<DMatch>& matches) const {
    matches.clear();
    if (nq <= 0 || nt <= 0) return;
    std::vector<int32_t> idx(nq), dist(nq);
    const dvs_status s = cross_ ? dvs_match_hamming_cross(m_, query, nq, train, nt, idx.data(), dist.data())
                                : dvs_match_hamming(m_, query, nq, train, nt, idx.data(), dist.data());
    if (s != DVS_OK) throw std::runtime_error(dvs_last_error());
    matches.reserve(nq);
    for (int i = 0; i < nq; i++)
      if (idx[i] >= 0) matches.push_back(DMatch{i, idx[i], 0, (float)dist[i]});
  }
  // knnMatch: per query the first min(k, nt) train rows by (distance, train index); compactResult drops queries without a match.
  // crossCheck: k must be 1, a query's list holds its mutual pair or nothing
  void knnMatch(const uint8_t* query, int nq, const uint8_t* train, int nt, std::vector<std::vector<DMatch>>& matches, int k,
                bool compactResult = false) const {
    matches.clear();
    if (cross_ && k != 1) throw std::invalid_argument("knnMatch: crossCheck needs k == 1");
    if (k < 1) throw std::invalid_argument("knnMatch: k must be >= 1");
    if (nq <= 0 || nt <= 0) return;
    std::vector<int32_t> idx((size_t)nq * k), dist((size_t)nq * k);
    const dvs_status s = cross_ ? dvs_match_hamming_cross(m_, query, nq, train, nt, idx.data(), dist.data())
                                : dvs_match_hamming_knn(m_, query, nq, train, nt, k, idx.data(), dist.data());
    if (s != DVS_OK) throw std::runtime_error(dvs_last_error());
    matches.reserve(nq);
    for (int i = 0; i < nq; i++) {
      std::vector<DMatch> row;
      for (int s2 = 0; s2 < k; s2++) {
        const size_t o = (size_t)i * k + s2;
        if (idx[o] < 0) break;   // the C-ABI's padding (k > nt, or no mutual pair)
        row.push_back(DMatch{i, idx[o], 0, (float)dist[o]});
      }
      if (!row.empty() || !compactResult) matches.push_back(std::move(row));
    }
  }
  // radiusMatch: every pair with (float)distance <= maxDistance, per query in std::sort-by-distance order (crossCheck is ignored,
  // as in OpenCV); compactResult drops queries without a match
  void radiusMatch(const uint8_t* query, int nq, const uint8_t* train, int nt, std::vector<std::vector<DMatch>>& matches, float maxDistance,
                   bool compactResult = false) const {
    matches.clear();
    if (nq <= 0 || nt <= 0) return;
    std::vector<int64_t> offs((size_t)nq + 1);
    std::vector<int32_t> pairs(2 * 4096);
    int64_t n = 0;
    if (dvs_match_hamming_radius(m_, query, nq, train, nt, maxDistance, offs.data(), pairs.data(), 4096, &n) != DVS_OK)
      throw std::runtime_error(dvs_last_error());
    if (n > 4096) {
      pairs.resize(2 * (size_t)n);
      if (dvs_match_hamming_radius(m_, query, nq, train, nt, maxDistance, offs.data(), pairs.data(), n, &n) != DVS_OK)
        throw std::runtime_error(dvs_last_error());
    }
    matches.reserve(nq);
    for (int i = 0; i < nq; i++) {
      std::vector<DMatch> row;
      row.reserve((size_t)(offs[i + 1] - offs[i]));
      for (int64_t p = offs[i]; p < offs[i + 1]; p++) row.push_back(DMatch{i, pairs[2 * p], 0, (float)pairs[2 * p + 1]});
      if (!row.empty() || !compactResult) matches.push_back(std::move(row));
    }
  }
  // (queryIdx, trainIdx, distance) for every pair with distance < max_dist, query-major order
  void matchBelow(const uint8_t* query, int nq, const uint8_t* train, int nt, int max_dist, std::vector<DMatch>& out) const {
    out.clear();
    if (nq <= 0 || nt <= 0) return;
    int32_t n = 0;
    std::vector<int32_t> pairs(3 * 1024);
    if (dvs_match_hamming_thresh(m_, query, nq, train, nt, max_dist, pairs.data(), 1024, &n) != DVS_OK) throw std::runtime_error(dvs_last_error());
    if (n > 1024) {
      pairs.resize(3 * (size_t)n);
      if (dvs_match_hamming_thresh(m_, query, nq, train, nt, max_dist, pairs.data(), n, &n) != DVS_OK) throw std::runtime_error(dvs_last_error());
    }
    out.resize(n);
    for (int i = 0; i < n; i++) out[i] = DMatch{pairs[3 * i], pairs[3 * i + 1], 0, (float)pairs[3 * i + 2]};
  }
#ifdef DVSLAM_WITH_OPENCV
  void match(const cv::Mat& query, const cv::Mat& train, std::vector<cv::DMatch>& matches) const {
    CV_Assert(query.empty() || (query.type() == CV_8U && query.cols == 32 && query.isContinuous()));
    CV_Assert(train.empty() || (train.type() == CV_8U && train.cols == 32 && train.isContinuous()));
    std::vector<DMatch> m;
    match(query.data, query.rows, train.data, train.rows, m);
    matches.resize(m.size());
    for (size_t i = 0; i < m.size(); i++) matches[i] = cv::DMatch(m[i].queryIdx, m[i].trainIdx, 0, m[i].distance);
  }
  void knnMatch(const cv::Mat& query, const cv::Mat& train, std::vector<std::vector<cv::DMatch>>& matches, int k,
                cv::InputArray mask = cv::noArray(), bool compactResult = false) const {
    CV_Assert(mask.empty());   // match masks are not supported
    std::vector<std::vector<DMatch>> m;
    knnMatch(rows_of(query), query.rows, rows_of(train), train.rows, m, k, compactResult);
    to_cv(m, matches);
  }
  void radiusMatch(const cv::Mat& query, const cv::Mat& train, std::vector<std::vector<cv::DMatch>>& matches, float maxDistance,
                   cv::InputArray mask = cv::noArray(), bool compactResult = false) const {
    CV_Assert(mask.empty());
    std::vector<std::vector<DMatch>> m;
    radiusMatch(rows_of(query), query.rows, rows_of(train), train.rows, m, maxDistance, compactResult);
    to_cv(m, matches);
  }
#endif
  bool isCrossCheck() const { return cross_; }
  dvs_matcher* handle() { return m_; }

 private:
#ifdef DVSLAM_WITH_OPENCV
  static const uint8_t* rows_of(const cv::Mat& d) {
    CV_Assert(d.empty() || (d.type() == CV_8U && d.cols == 32 && d.isContinuous()));
    return d.data;
  }
  static void to_cv(const std::vector<std::vector<DMatch>>& m, std::vector<std::vector<cv::DMatch>>& out) {
    out.assign(m.size(), std::vector<cv::DMatch>());
    for (size_t i = 0; i < m.size(); i++) {
      out[i].reserve(m[i].size());
      for (const DMatch& d : m[i]) out[i].push_back(cv::DMatch(d.queryIdx, d.trainIdx, 0, d.distance));
    }
  }
#endif
  dvs_matcher* m_ = nullptr;
  bool cross_ = false;
};

#ifdef DVSLAM_WITH_OPENCV
// cv::BFMatcher's own constructor signature for the reference's two member declarations (frontend.cpp:220
// `matcher_(cv::NORM_HAMMING)`, backend.cpp:222 `descriptor_matcher_(cv::NORM_HAMMING, false)`): changing the member's TYPE
// from cv::BFMatcher to dvslam::HammingBFMatcher is the whole matcher-side integration; every match() call compiles unchanged.
class HammingBFMatcher : public BFMatcher {
 public:
  explicit HammingBFMatcher(int normType = cv::NORM_HAMMING, bool crossCheck = false) : BFMatcher(0, crossCheck) {
    CV_Assert(normType == cv::NORM_HAMMING);
  }
};
#endif

}  // namespace dvslam
