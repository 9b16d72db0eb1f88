// dvslam::LoopDatabase (include/dvslam/loop_detection.hpp) from a host program: a vocabulary text file and a rows file the Python side
// wrote (int32 frames, then per frame int32 n and n x 32 bytes; the LAST frame is the query, the others become entries in order).
// Prints the direct-index levels, entry 0's FeatureVector, the query results (ids and score bytes), then the match triplets of
// detect(top 2) and of match() against every entry; tests/test_cpp_loop.py compares them with tests/loop_ref.py.  With
// DVSLAM_WITH_OPENCV the frames go in as std::vector<cv::Mat>.  Exit codes: 0 ok, 1 a check failed, 2 usage, 3 no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "dvslam/loop_detection.hpp"

static void print_candidates(const char* tag, const std::vector<dvslam::LoopCandidate>& cands) {
  std::printf("%s %zu\n", tag, cands.size());
  for (const dvslam::LoopCandidate& c : cands) {
    uint64_t bits;
    std::memcpy(&bits, &c.Score, 8);
    std::printf("cand %u:%016llx %zu", c.Id, (unsigned long long)bits, c.matches.size());
    for (const dvslam::Match& m : c.matches) std::printf(" %d:%d:%d", m.query, m.train, m.distance);
    std::printf("\n");
  }
}

#ifdef DVSLAM_WITH_OPENCV
typedef std::vector<cv::Mat> Frame;
static Frame to_frame(const dvslam::DescriptorVector& d) {
  Frame f;
  for (const auto& r : d) { cv::Mat m(1, 32, CV_8UC1); std::memcpy(m.data, r.data(), 32); f.push_back(m); }
  return f;
}
#else
typedef dvslam::DescriptorVector Frame;
static Frame to_frame(const dvslam::DescriptorVector& d) { return d; }
#endif

int main(int argc, char** argv) {
  if (dvs_device_count() < 1) { std::fprintf(stderr, "no GPU: there is no CPU fallback\n"); return 3; }
  if (argc != 4) { std::fprintf(stderr, "usage: %s vocabulary.txt frames.bin di_levels\n", argv[0]); return 2; }
  std::vector<dvslam::DescriptorVector> frames;
  {
    FILE* fp = std::fopen(argv[2], "rb");
    int32_t nf = 0;
    if (!fp || std::fread(&nf, 4, 1, fp) != 1 || nf < 1) return 2;
    frames.resize(nf);
    for (int32_t f = 0; f < nf; f++) {
      int32_t n = 0;
      if (std::fread(&n, 4, 1, fp) != 1 || n < 0) return 2;
      frames[f].resize(n);
      if (n && std::fread(frames[f][0].data(), 32, n, fp) != (size_t)n) return 2;
    }
    std::fclose(fp);
  }
  const int di_levels = std::atoi(argv[3]);
  try {
    dvslam::OrbVocabulary vocabulary(argv[1]);
    dvslam::LoopDatabase database(vocabulary, di_levels);
    std::vector<dvslam::EntryId> all;
    for (size_t f = 0; f + 1 < frames.size(); f++) all.push_back(database.add(to_frame(frames[f])));
    const Frame query = to_frame(frames.back());
    std::printf("size %u di %d levels %d\n", database.size(), database.usingDirectIndex() ? 1 : 0, database.getDirectIndexLevels());
    if (database.size() > 0) {
      const dvslam::FeatureVector fv = database.retrieveFeatures(0);
      std::printf("fv %zu", fv.size());
      for (const auto& kv : fv) {
        std::printf(" %u:", kv.first);
        for (size_t i = 0; i < kv.second.size(); i++) std::printf(i ? ",%u" : "%u", kv.second[i]);
      }
      std::printf("\n");
    }
    dvslam::QueryResults results;
    database.query(query, results, 0);
    std::printf("query %zu", results.size());
    for (const dvslam::Result& r : results) {
      uint64_t bits;
      std::memcpy(&bits, &r.Score, 8);
      std::printf(" %u:%016llx", r.Id, (unsigned long long)bits);
    }
    std::printf("\n");
    print_candidates("detect", database.detect(query, 2));
    print_candidates("match", database.match(query, all));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
