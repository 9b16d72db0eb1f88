// dvslam/place_recognition.hpp — header-only C++ adapter with the call surface of DBoW2's OrbVocabulary / OrbDatabase as the reference's
// test/test_dbow2_integration.cpp:63-163 uses them, over dvs_bow_* and dvs_voc_* of dvslam_hip.h.  A call site swaps the two typedefs (:7-8)
//   typedef dvslam::OrbVocabulary OrbVocabulary;   typedef dvslam::OrbDatabase OrbDatabase;
// and DBoW2::EntryId / DBoW2::QueryResults for dvslam::EntryId / dvslam::QueryResults; the test body reads the same.
//   plain layer    features as `const uint8_t* rows, int n` (n x 32 bytes) or std::vector<std::array<uint8_t, 32>>; needs only the C-ABI
//   OpenCV layer   std::vector<cv::Mat> features (one 1 x 32 CV_8U row each), compiled only when DVSLAM_WITH_OPENCV is defined
// Semantics, the deviations (early-leaf node id, (raw, id) result order; training: iteration cap, emptied cluster, the stated sampler)
// and what is not built (scorings other than L1): INTEGRATION.md "Place recognition".  The direct index is dvslam::LoopDatabase
// (loop_detection.hpp); OrbDatabase stays the database without one.  Errors throw
// std::runtime_error, as DBoW2 throws on a file it cannot read.
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#ifdef DVSLAM_WITH_OPENCV
#include <cstring>
#include <opencv2/core/core.hpp>
#endif

namespace dvslam {

typedef unsigned int EntryId;
typedef unsigned int WordId;
typedef unsigned int NodeId;
typedef std::vector<std::array<uint8_t, 32>> DescriptorVector;
typedef std::map<WordId, double> BowVector;                       // DBoW2::BowVector is a std::map<WordId, WordValue>
typedef std::map<NodeId, std::vector<unsigned int>> FeatureVector;

enum WeightingType { TF_IDF = 0, TF = 1, IDF = 2, BINARY = 3 };                                  // DBoW2::WeightingType
enum ScoringType { L1_NORM = 0, L2_NORM = 1, CHI_SQUARE = 2, KL = 3, BHATTACHARYYA = 4, DOT_PRODUCT = 5 };   // DBoW2::ScoringType

struct Result {
  EntryId Id;
  double Score;
  Result() : Id(0), Score(0) {}
  Result(EntryId id, double score) : Id(id), Score(score) {}
};
typedef std::vector<Result> QueryResults;

namespace detail {
inline void bow_check(dvs_status st, const char* what) {
  if (st != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
}
#ifdef DVSLAM_WITH_OPENCV
inline std::vector<uint8_t> pack_rows(const std::vector<cv::Mat>& features) {
  std::vector<uint8_t> rows(features.size() * 32);
  for (size_t i = 0; i < features.size(); i++) {
    CV_Assert(features[i].type() == CV_8UC1 && features[i].total() == 32 && features[i].isContinuous());
    std::memcpy(&rows[i * 32], features[i].data, 32);
  }
  return rows;
}
#endif
}  // namespace detail

class OrbVocabulary {
 public:
  explicit OrbVocabulary(int device = 0, void* hip_stream = nullptr) : device_(device), stream_(hip_stream) {}
  explicit OrbVocabulary(const std::string& filename, int device = 0, void* hip_stream = nullptr) : device_(device), stream_(hip_stream) {
    loadFromTextFile(filename);
  }
  // TemplatedVocabulary(k, L, weighting, scoring): the parameters create(training_features) trains with (all four are required here:
  // the two-argument form is (device, stream))
  OrbVocabulary(int k, int L, WeightingType weighting, ScoringType scoring, int device = 0, void* hip_stream = nullptr)
      : device_(device), stream_(hip_stream), k_(k), L_(L), weighting_(weighting), scoring_(scoring) {}
  ~OrbVocabulary() { dvs_bow_vocab_destroy(h_); }
  OrbVocabulary(const OrbVocabulary&) = delete;
  OrbVocabulary& operator=(const OrbVocabulary&) = delete;

  bool loadFromTextFile(const std::string& filename) {
    dvs_bow_vocab* h = nullptr;
    detail::bow_check(dvs_bow_vocab_load_text(device_, stream_, filename.c_str(), &h), "OrbVocabulary::loadFromTextFile");
    dvs_bow_vocab_destroy(h_);
    h_ = h;
    return true;
  }
  // TemplatedVocabulary::create: hierarchical k-means over all images' features (test_dbow2_integration.cpp:158).  Replaces the handle:
  // a database that borrows the old one must be gone (DBoW2's database holds a copy instead).  Blocks until the vocabulary is trained.
  void create(const uint8_t* rows, const int32_t* image_counts, int nimages) {
    dvs_voc_train_params p;
    detail::bow_check(dvs_voc_train_default_params(&p), "OrbVocabulary::create");
    p.k = k_; p.L = L_; p.weighting = (int32_t)weighting_; p.scoring = (int32_t)scoring_; p.seed = seed_;
    dvs_bow_vocab* h = nullptr;
    detail::bow_check(dvs_voc_train(device_, stream_, &p, rows, image_counts, nimages, &h, &report_), "OrbVocabulary::create");
    dvs_bow_vocab_destroy(h_);
    h_ = h;
  }
  void create(const std::vector<DescriptorVector>& training_features) {
    std::vector<int32_t> counts;
    std::vector<uint8_t> rows;
    for (const DescriptorVector& image : training_features) {
      counts.push_back((int32_t)image.size());
      for (const std::array<uint8_t, 32>& d : image) rows.insert(rows.end(), d.begin(), d.end());
    }
    create(rows.empty() ? nullptr : rows.data(), counts.empty() ? nullptr : counts.data(), (int)counts.size());
  }
  void create(const std::vector<DescriptorVector>& training_features, int k, int L) {
    k_ = k; L_ = L;
    create(training_features);
  }
  void create(const std::vector<DescriptorVector>& training_features, int k, int L, WeightingType weighting, ScoringType scoring) {
    k_ = k; L_ = L; weighting_ = weighting; scoring_ = scoring;
    create(training_features);
  }
  // TemplatedVocabulary::saveToTextFile, the format loadFromTextFile reads
  void saveToTextFile(const std::string& filename) const {
    if (!h_) throw std::runtime_error("OrbVocabulary::saveToTextFile: no vocabulary");
    detail::bow_check(dvs_voc_save_text(h_, filename.c_str()), "OrbVocabulary::saveToTextFile");
  }
  void setSeed(uint64_t seed) { seed_ = seed; }              // the sampler's seed (DBoW2 seeds from the clock)
  const dvs_voc_train_report& lastTrainReport() const { return report_; }
  // number of words
  unsigned int size() const {
    int32_t n = 0;
    if (h_) detail::bow_check(dvs_bow_vocab_info(h_, nullptr, nullptr, nullptr, nullptr, nullptr, &n), "OrbVocabulary::size");
    return (unsigned int)n;
  }
  bool empty() const { return size() == 0; }

  void transform(const uint8_t* rows, int n, BowVector& v, FeatureVector& fv, int levelsup) const {
    v.clear(); fv.clear();
    if (!h_ || n <= 0) return;
    std::vector<int32_t> w(n), nodes(n), offsets(n + 1), feats(n);
    std::vector<double> val(n);
    int32_t nw = 0, nn = 0;
    detail::bow_check(dvs_bow_transform(h_, rows, n, levelsup, w.data(), val.data(), n, &nw, nodes.data(), offsets.data(), feats.data(), n, &nn, nullptr,
                                        nullptr, nullptr), "OrbVocabulary::transform");
    for (int i = 0; i < nw; i++) v.emplace_hint(v.end(), (WordId)w[i], val[i]);
    for (int i = 0; i < nn; i++)
      fv.emplace_hint(fv.end(), (NodeId)nodes[i], std::vector<unsigned int>(feats.begin() + offsets[i], feats.begin() + offsets[i + 1]));
  }
  void transform(const uint8_t* rows, int n, BowVector& v) const { FeatureVector fv; transform(rows, n, v, fv, 0); }
  void transform(const DescriptorVector& features, BowVector& v, FeatureVector& fv, int levelsup) const {
    transform(features.empty() ? nullptr : features[0].data(), (int)features.size(), v, fv, levelsup);
  }
  void transform(const DescriptorVector& features, BowVector& v) const { FeatureVector fv; transform(features, v, fv, 0); }
#ifdef DVSLAM_WITH_OPENCV
  void transform(const std::vector<cv::Mat>& features, BowVector& v, FeatureVector& fv, int levelsup) const {
    const std::vector<uint8_t> rows = detail::pack_rows(features);
    transform(rows.data(), (int)features.size(), v, fv, levelsup);
  }
  void transform(const std::vector<cv::Mat>& features, BowVector& v) const { FeatureVector fv; transform(features, v, fv, 0); }
  void create(const std::vector<std::vector<cv::Mat>>& training_features) {
    std::vector<int32_t> counts;
    std::vector<uint8_t> rows;
    for (const std::vector<cv::Mat>& image : training_features) {
      const std::vector<uint8_t> r = detail::pack_rows(image);
      counts.push_back((int32_t)image.size());
      rows.insert(rows.end(), r.begin(), r.end());
    }
    create(rows.empty() ? nullptr : rows.data(), counts.empty() ? nullptr : counts.data(), (int)counts.size());
  }
  void create(const std::vector<std::vector<cv::Mat>>& training_features, int k, int L) {
    k_ = k; L_ = L;
    create(training_features);
  }
  void create(const std::vector<std::vector<cv::Mat>>& training_features, int k, int L, WeightingType weighting, ScoringType scoring) {
    k_ = k; L_ = L; weighting_ = weighting; scoring_ = scoring;
    create(training_features);
  }
#endif
  dvs_bow_vocab* handle() const { return h_; }

 private:
  dvs_bow_vocab* h_ = nullptr;
  int device_;
  void* stream_;
  int k_ = 10, L_ = 5;
  WeightingType weighting_ = TF_IDF;
  ScoringType scoring_ = L1_NORM;
  uint64_t seed_ = 0;
  dvs_voc_train_report report_ = dvs_voc_train_report();
};

// Borrows the vocabulary (DBoW2 copies it): the vocabulary must outlive the database.
class OrbDatabase {
 public:
  OrbDatabase() {}
  explicit OrbDatabase(const OrbVocabulary& voc) { setVocabulary(voc); }
  ~OrbDatabase() { dvs_bow_db_destroy(h_); }
  OrbDatabase(const OrbDatabase&) = delete;
  OrbDatabase& operator=(const OrbDatabase&) = delete;

  void setVocabulary(const OrbVocabulary& voc) {
    if (!voc.handle()) throw std::runtime_error("OrbDatabase: the vocabulary is not loaded");
    dvs_bow_db* h = nullptr;
    detail::bow_check(dvs_bow_db_create(voc.handle(), &h), "OrbDatabase::setVocabulary");
    dvs_bow_db_destroy(h_);
    h_ = h;
  }
  unsigned int size() const { return (unsigned int)dvs_bow_db_size(h_); }
  void clear() { if (h_) detail::bow_check(dvs_bow_db_clear(h_), "OrbDatabase::clear"); }

  EntryId add(const uint8_t* rows, int n) {
    need();
    int32_t id = -1;
    detail::bow_check(dvs_bow_db_add(h_, rows, n, &id), "OrbDatabase::add");
    return (EntryId)id;
  }
  EntryId add(const DescriptorVector& features) { return add(features.empty() ? nullptr : features[0].data(), (int)features.size()); }

  void query(const uint8_t* rows, int n, QueryResults& ret, int max_results = 1, int max_id = -1) const {
    need();
    ret.clear();
    const int size = dvs_bow_db_size(h_);
    const int cap = max_results > 0 && max_results < size ? max_results : size;
    std::vector<int32_t> ids(cap > 0 ? cap : 1);
    std::vector<double> scores(cap > 0 ? cap : 1);
    int32_t nr = 0;
    detail::bow_check(dvs_bow_db_query(h_, rows, n, max_results, max_id < 0 ? -1 : max_id, ids.data(), scores.data(), cap, &nr), "OrbDatabase::query");
    for (int i = 0; i < nr; i++) ret.push_back(Result((EntryId)ids[i], scores[i]));
  }
  void query(const DescriptorVector& features, QueryResults& ret, int max_results = 1, int max_id = -1) const {
    query(features.empty() ? nullptr : features[0].data(), (int)features.size(), ret, max_results, max_id);
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
#endif
  dvs_bow_db* handle() const { return h_; }

 private:
  void need() const { if (!h_) throw std::runtime_error("OrbDatabase: no vocabulary set"); }
  dvs_bow_db* h_ = nullptr;
};

}  // namespace dvslam
