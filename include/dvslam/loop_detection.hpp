// dvslam/loop_detection.hpp — header-only C++ adapter over dvs_loop_* of dvslam_hip.h: a keyframe database with a direct index
// (DBoW2's TemplatedDatabase(voc, use_di = true, di_levels), with DBoW2's names where they exist: add, query, size, clear,
// usingDirectIndex, getDirectIndexLevels, retrieveFeatures) and, beyond DBoW2, match / detect: node-guided, ratio-tested, one-to-one
// correspondences between a frame and candidate entries.  The matching rule is this library's own (dvslam_hip.h, "loop candidates";
// INTEGRATION.md "Loop candidates").  dvslam::OrbDatabase (place_recognition.hpp) stays the database without a direct index.
// Loop verification (dvslam_hip.h, "loop verification"): setPoints / getPoints keep an entry's 3D points (its camera frame) beside its
// descriptors; verify() and detectVerified() estimate, per candidate, the rigid motion x_query = R x_entry + t by a RANSAC over the
// matched 3D points on the device and fill LoopCandidate::verified, R, t, inliers, rms.
//   plain layer    features as `const uint8_t* rows, int n` (n x 32 bytes) or dvslam::DescriptorVector; needs only the C-ABI
//   OpenCV layer   std::vector<cv::Mat> features (one 1 x 32 CV_8U row each), compiled only when DVSLAM_WITH_OPENCV is defined
// Errors throw std::runtime_error.
#pragma once
#include <array>
#include <cmath>
#include "place_recognition.hpp"

namespace dvslam {

struct Match {
  int query, train, distance;     // row of the frame, row of the entry, Hamming distance
};
struct LoopCandidate {
  EntryId Id;
  double Score;                   // the query's L1 score; 0 from match(), which runs no query
  std::vector<Match> matches;     // ascending query row
  // filled by verify() / detectVerified(); as constructed by match() / detect()
  bool verified = false;          // at least VerifyParams::min_inliers inliers
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // row-major; x_query = R x_entry + t
  double t[3] = {0, 0, 0};
  std::vector<int> inliers;       // query rows of the inlier correspondences, ascending
  double rms = 0.0;               // square root of the mean inlier error, pixels
  int correspondences = 0;        // matches with a valid 3D point on both sides (-1: no such entry)
  int iterations = 0;             // RANSAC iterations run
};
typedef std::array<float, 3> Point3;
typedef std::vector<Point3> PointVector;   // one per descriptor row; a row without depth is any invalid point (NaN)
struct VerifyParams {
  int iterations = 256, min_correspondences = 12, min_inliers = 12, refine_rounds = 2;
  double reproj_err = 4.0, confidence = 0.99;
  uint64_t seed = 0;
  double fx = 0, fy = 0, cx = 0, cy = 0;   // no default: set them
};
struct MatchParams {
  int max_distance = 50, ratio_num = 3, ratio_den = 4;
};

// Borrows the vocabulary (DBoW2 copies it): the vocabulary must outlive the database.
class LoopDatabase {
 public:
  LoopDatabase() {}
  explicit LoopDatabase(const OrbVocabulary& voc, int di_levels = 0) { setVocabulary(voc, di_levels); }
  ~LoopDatabase() { dvs_loop_db_destroy(h_); }
  LoopDatabase(const LoopDatabase&) = delete;
  LoopDatabase& operator=(const LoopDatabase&) = delete;

  void setVocabulary(const OrbVocabulary& voc, int di_levels = 0) {
    if (!voc.handle()) throw std::runtime_error("LoopDatabase: the vocabulary is not loaded");
    dvs_loop_db* h = nullptr;
    detail::bow_check(dvs_loop_db_create(voc.handle(), di_levels, &h), "LoopDatabase::setVocabulary");
    dvs_loop_db_destroy(h_);
    h_ = h;
  }
  unsigned int size() const { return (unsigned int)dvs_loop_db_size(h_); }
  void clear() { if (h_) detail::bow_check(dvs_loop_db_clear(h_), "LoopDatabase::clear"); }
  bool usingDirectIndex() const { return h_ != nullptr; }
  int getDirectIndexLevels() const { return dvs_loop_db_di_levels(h_); }

  EntryId add(const uint8_t* rows, int n) {
    need();
    int32_t id = -1;
    detail::bow_check(dvs_loop_db_add(h_, rows, n, &id), "LoopDatabase::add");
    return (EntryId)id;
  }
  EntryId add(const DescriptorVector& features) { return add(data(features), (int)features.size()); }

  void query(const uint8_t* rows, int n, QueryResults& ret, int max_results = 1, int max_id = -1) const {
    need();
    ret.clear();
    const int cap = capacity(max_results);
    std::vector<int32_t> ids(cap > 0 ? cap : 1);
    std::vector<double> scores(cap > 0 ? cap : 1);
    int32_t nr = 0;
    detail::bow_check(dvs_loop_db_query(h_, rows, n, max_results, max_id < 0 ? -1 : max_id, ids.data(), scores.data(), cap, &nr), "LoopDatabase::query");
    for (int i = 0; i < nr; i++) ret.push_back(Result((EntryId)ids[i], scores[i]));
  }
  void query(const DescriptorVector& features, QueryResults& ret, int max_results = 1, int max_id = -1) const {
    query(data(features), (int)features.size(), ret, max_results, max_id);
  }

  // TemplatedDatabase::retrieveFeatures
  FeatureVector retrieveFeatures(EntryId id) const {
    need();
    int32_t nn = 0, m = 0;
    const dvs_status st = dvs_loop_db_get_features(h_, (int32_t)id, nullptr, nullptr, nullptr, 0, 0, &nn, &m);
    if (st != DVS_OK && st != DVS_ERR_CAPACITY) detail::bow_check(st, "LoopDatabase::retrieveFeatures");
    std::vector<int32_t> nodes(nn + 1), offsets(nn + 1), feats(m + 1);
    detail::bow_check(dvs_loop_db_get_features(h_, (int32_t)id, nodes.data(), offsets.data(), feats.data(), nn, m, &nn, &m), "LoopDatabase::retrieveFeatures");
    FeatureVector fv;
    for (int i = 0; i < nn; i++)
      fv.emplace_hint(fv.end(), (NodeId)nodes[i], std::vector<unsigned int>(feats.begin() + offsets[i], feats.begin() + offsets[i + 1]));
    return fv;
  }

  // guided match of a frame against the listed entries, in their order
  std::vector<LoopCandidate> match(const uint8_t* rows, int n, const std::vector<EntryId>& entries, const MatchParams& p = MatchParams()) const {
    need();
    const int c = (int)entries.size();
    std::vector<int32_t> ids(entries.begin(), entries.end()), nm(c + 1), train((size_t)c * n + 1), dist((size_t)c * n + 1);
    const dvs_loop_match_params P = {p.max_distance, p.ratio_num, p.ratio_den};
    detail::bow_check(dvs_loop_db_match(h_, rows, n, ids.data(), c, &P, train.data(), dist.data(), nm.data()), "LoopDatabase::match");
    std::vector<LoopCandidate> out(c);
    for (int x = 0; x < c; x++) { out[x].Id = entries[x]; out[x].Score = 0.0; collect(out[x], &train[(size_t)x * n], &dist[(size_t)x * n], n); }
    return out;
  }
  std::vector<LoopCandidate> match(const DescriptorVector& features, const std::vector<EntryId>& entries, const MatchParams& p = MatchParams()) const {
    return match(data(features), (int)features.size(), entries, p);
  }

  // one transform, the query and the guided match of its results in one enqueue and one read-back
  std::vector<LoopCandidate> detect(const uint8_t* rows, int n, int max_results = 4, int max_id = -1, const MatchParams& p = MatchParams()) const {
    need();
    const int cap = capacity(max_results);
    std::vector<int32_t> ids(cap + 1), nm(cap + 1), train((size_t)cap * n + 1), dist((size_t)cap * n + 1);
    std::vector<double> scores(cap + 1);
    const dvs_loop_match_params P = {p.max_distance, p.ratio_num, p.ratio_den};
    int32_t nr = 0;
    detail::bow_check(dvs_loop_db_detect(h_, rows, n, max_results, max_id < 0 ? -1 : max_id, &P, ids.data(), scores.data(), nm.data(), train.data(),
                                         dist.data(), cap, &nr), "LoopDatabase::detect");
    std::vector<LoopCandidate> out(nr);
    for (int x = 0; x < nr; x++) { out[x].Id = (EntryId)ids[x]; out[x].Score = scores[x]; collect(out[x], &train[(size_t)x * n], &dist[(size_t)x * n], n); }
    return out;
  }
  std::vector<LoopCandidate> detect(const DescriptorVector& features, int max_results = 4, int max_id = -1, const MatchParams& p = MatchParams()) const {
    return detect(data(features), (int)features.size(), max_results, max_id, p);
  }
  // ---- loop verification ----
  void setPoints(EntryId id, const float* xyz, int n) {
    need();
    detail::bow_check(dvs_loopv_db_set_points(h_, (int32_t)id, xyz, n), "LoopDatabase::setPoints");
  }
  void setPoints(EntryId id, const PointVector& points) { setPoints(id, points.empty() ? nullptr : points[0].data(), (int)points.size()); }
  PointVector getPoints(EntryId id) const {
    need();
    int32_t n = 0;
    const dvs_status st = dvs_loopv_db_get_points(h_, (int32_t)id, nullptr, 0, &n);
    if (st != DVS_OK && st != DVS_ERR_CAPACITY) detail::bow_check(st, "LoopDatabase::getPoints");
    PointVector out(n);
    detail::bow_check(dvs_loopv_db_get_points(h_, (int32_t)id, n ? out[0].data() : nullptr, n, &n), "LoopDatabase::getPoints");
    return out;
  }
  // the rigid 3D-3D verification of candidates that match() / detect() returned for the frame whose points these are (n rows)
  void verify(const float* xyz, int n, std::vector<LoopCandidate>& candidates, const VerifyParams& p) const {
    need();
    const int c = (int)candidates.size();
    std::vector<int32_t> ids(c + 1), train((size_t)c * n + 1, -1);
    for (int x = 0; x < c; x++) {
      ids[x] = (int32_t)candidates[x].Id;
      for (const Match& m : candidates[x].matches)
        if (m.query >= 0 && m.query < n) train[(size_t)x * n + m.query] = m.train;
    }
    std::vector<dvs_loop_verify_result> res(c + 1);
    std::vector<uint8_t> mask((size_t)c * n + 1);
    const dvs_loop_verify_params P = params(p);
    detail::bow_check(dvs_loopv_db_verify(h_, xyz, n, ids.data(), c, train.data(), &P, res.data(), mask.data()), "LoopDatabase::verify");
    for (int x = 0; x < c; x++) fill(candidates[x], res[x], &mask[(size_t)x * n], n);
  }
  void verify(const PointVector& points, std::vector<LoopCandidate>& candidates, const VerifyParams& p) const {
    verify(points.empty() ? nullptr : points[0].data(), (int)points.size(), candidates, p);
  }
  // transform, query, guided match and verification in one enqueue and one read-back
  std::vector<LoopCandidate> detectVerified(const uint8_t* rows, const float* xyz, int n, int max_results, int max_id, const VerifyParams& vp,
                                            const MatchParams& p = MatchParams()) const {
    need();
    const int cap = capacity(max_results);
    std::vector<int32_t> ids(cap + 1), nm(cap + 1), train((size_t)cap * n + 1), dist((size_t)cap * n + 1);
    std::vector<double> scores(cap + 1);
    std::vector<dvs_loop_verify_result> res(cap + 1);
    std::vector<uint8_t> mask((size_t)cap * n + 1);
    const dvs_loop_match_params P = {p.max_distance, p.ratio_num, p.ratio_den};
    const dvs_loop_verify_params V = params(vp);
    int32_t nr = 0;
    detail::bow_check(dvs_loopv_db_detect_verify(h_, rows, xyz, n, max_results, max_id < 0 ? -1 : max_id, &P, &V, ids.data(), scores.data(), nm.data(),
                                                train.data(), dist.data(), res.data(), mask.data(), cap, &nr), "LoopDatabase::detectVerified");
    std::vector<LoopCandidate> out(nr);
    for (int x = 0; x < nr; x++) {
      out[x].Id = (EntryId)ids[x]; out[x].Score = scores[x];
      collect(out[x], &train[(size_t)x * n], &dist[(size_t)x * n], n);
      fill(out[x], res[x], &mask[(size_t)x * n], n);
    }
    return out;
  }
  std::vector<LoopCandidate> detectVerified(const DescriptorVector& descriptors, const PointVector& points, int max_results, int max_id,
                                            const VerifyParams& vp, const MatchParams& p = MatchParams()) const {
    if (points.size() != descriptors.size()) throw std::runtime_error("LoopDatabase::detectVerified: one point per descriptor row");
    return detectVerified(data(descriptors), points.empty() ? nullptr : points[0].data(), (int)descriptors.size(), max_results, max_id, vp, p);
  }
#ifdef DVSLAM_WITH_OPENCV
  EntryId add(const std::vector<cv::Mat>& features) {
    const std::vector<uint8_t> rows = detail::pack_rows(features);
    return add(rows.data(), (int)features.size());
  }
  void query(const std::vector<cv::Mat>& features, QueryResults& ret, int max_results = 1, int max_id = -1) const {
    const std::vector<uint8_t> rows = detail::pack_rows(features);
    query(rows.data(), (int)features.size(), ret, max_results, max_id);
  }
  std::vector<LoopCandidate> match(const std::vector<cv::Mat>& features, const std::vector<EntryId>& entries, const MatchParams& p = MatchParams()) const {
    const std::vector<uint8_t> rows = detail::pack_rows(features);
    return match(rows.data(), (int)features.size(), entries, p);
  }
  std::vector<LoopCandidate> detect(const std::vector<cv::Mat>& features, int max_results = 4, int max_id = -1, const MatchParams& p = MatchParams()) const {
    const std::vector<uint8_t> rows = detail::pack_rows(features);
    return detect(rows.data(), (int)features.size(), max_results, max_id, p);
  }
#endif
  dvs_loop_db* handle() const { return h_; }

 private:
  static const uint8_t* data(const DescriptorVector& f) { return f.empty() ? nullptr : f[0].data(); }
  void need() const { if (!h_) throw std::runtime_error("LoopDatabase: no vocabulary set"); }
  int capacity(int max_results) const {
    const int size = dvs_loop_db_size(h_);
    return max_results > 0 && max_results < size ? max_results : size;
  }
  static void collect(LoopCandidate& c, const int32_t* train, const int32_t* dist, int n) {
    for (int i = 0; i < n; i++)
      if (train[i] >= 0) c.matches.push_back(Match{i, (int)train[i], (int)dist[i]});
  }
  static dvs_loop_verify_params params(const VerifyParams& p) {
    dvs_loop_verify_params P;
    P.iterations = p.iterations; P.min_correspondences = p.min_correspondences; P.min_inliers = p.min_inliers; P.refine_rounds = p.refine_rounds;
    P.reproj_err = p.reproj_err; P.confidence = p.confidence; P.seed = p.seed;
    P.K4[0] = p.fx; P.K4[1] = p.fy; P.K4[2] = p.cx; P.K4[3] = p.cy;
    return P;
  }
  // the record into the candidate: R from the Rodrigues vector (R = I + sin(a) K + (1 - cos(a)) K^2, K the unit axis' cross matrix)
  static void fill(LoopCandidate& c, const dvs_loop_verify_result& r, const uint8_t* mask, int n) {
    c.verified = r.success != 0; c.rms = r.rms_px; c.correspondences = r.n_corr; c.iterations = r.iterations;
    for (int k = 0; k < 3; k++) c.t[k] = r.tvec[k];
    const double a = std::sqrt(r.rvec[0] * r.rvec[0] + r.rvec[1] * r.rvec[1] + r.rvec[2] * r.rvec[2]);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; k++) c.R[k] = I[k];
    if (a > 0) {
      const double x = r.rvec[0] / a, y = r.rvec[1] / a, z = r.rvec[2] / a, K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          double kk = 0;
          for (int m = 0; m < 3; m++) kk += K[3 * i + m] * K[3 * m + j];
          c.R[3 * i + j] = I[3 * i + j] + std::sin(a) * K[3 * i + j] + (1.0 - std::cos(a)) * kk;
        }
    }
    c.inliers.clear();
    for (int i = 0; i < n; i++) if (mask[i]) c.inliers.push_back(i);
  }
  dvs_loop_db* h_ = nullptr;
};

}  // namespace dvslam
