// VocabularyCreation of the reference's test/test_dbow2_integration.cpp:138-163 over include/dvslam/place_recognition.hpp: the typedef
// (:7) swapped, the body in the reference's wording, then saveToTextFile / loadFromTextFile / transform on the result.  The training
// images come from a file the Python side wrote (int32 nimages, int32 counts[nimages], then the rows) instead of cv::ORB.  Prints the
// sizes, the training report and the BowVector bytes of the first image under the reloaded vocabulary; tests/test_cpp_bow_train.py
// compares them with tests/bow_train_ref.py.  Exit codes: 0 ok, 1 a check failed, 2 usage, 3 no GPU.
#include <cstdio>
#include <cstring>
#include <iostream>
#include "dvslam/place_recognition.hpp"

typedef dvslam::OrbVocabulary OrbVocabulary;

static int failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main(int argc, char** argv) {
  if (dvs_device_count() < 1) { std::fprintf(stderr, "no GPU: there is no CPU fallback\n"); return 3; }
  if (argc != 5) { std::fprintf(stderr, "usage: %s images.bin k L saved.txt\n", argv[0]); return 2; }
  std::vector<dvslam::DescriptorVector> training_features;
  {
    FILE* fp = std::fopen(argv[1], "rb");
    int32_t nimages = 0;
    if (!fp || std::fread(&nimages, 4, 1, fp) != 1 || nimages < 0) return 2;
    std::vector<int32_t> counts(nimages);
    if (nimages && std::fread(counts.data(), 4, nimages, fp) != (size_t)nimages) return 2;
    for (int32_t n : counts) {
      dvslam::DescriptorVector descriptor_vector(n);
      if (n && std::fread(descriptor_vector[0].data(), 32, n, fp) != (size_t)n) return 2;
      training_features.push_back(descriptor_vector);
    }
    std::fclose(fp);
  }
  const int k = std::atoi(argv[2]), L = std::atoi(argv[3]);

  // Test vocabulary creation from features
  OrbVocabulary vocabulary;
  bool created = false;
  try {
    vocabulary.setSeed(7);
    vocabulary.create(training_features, k, L);
    created = true;
  } catch (const std::exception& e) {
    std::cout << "Vocabulary creation failed: " << e.what() << std::endl;
  }
  EXPECT_TRUE(created);
  EXPECT_TRUE(vocabulary.size() > 0);
  if (!created) return 1;

  const dvs_voc_train_report& r = vocabulary.lastTrainReport();
  std::printf("words %u nodes %d\n", vocabulary.size(), r.n_nodes);
  std::printf("report %d %d %d %d %d %d %d\n", r.n_nodes, r.n_words, r.levels_run, r.max_passes, r.nodes_capped, r.clusters_emptied, r.nodes_short_seeded);

  vocabulary.saveToTextFile(argv[4]);
  OrbVocabulary loaded;
  loaded.loadFromTextFile(argv[4]);
  EXPECT_TRUE(loaded.size() == vocabulary.size());
  dvslam::BowVector v, again;
  dvslam::FeatureVector fv;
  loaded.transform(training_features[0], v, fv, 1);
  vocabulary.transform(training_features[0], again);
  EXPECT_TRUE(v == again);
  std::printf("bow %zu", v.size());
  for (const auto& kv : v) {
    uint64_t bits;
    std::memcpy(&bits, &kv.second, 8);
    std::printf(" %u:%016llx", kv.first, (unsigned long long)bits);
  }
  std::printf("\n");
  return failures ? 1 : 0;
}
