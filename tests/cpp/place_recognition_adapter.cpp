// BasicDatabaseOperations of the reference's test/test_dbow2_integration.cpp:63-126 over include/dvslam/place_recognition.hpp: the
// typedefs (:7-8) swapped, the body in the reference's wording.  The descriptors come from a file the Python side wrote (int32 n, then
// n x 32 bytes) instead of cv::ORB.  Prints the entry id and every result's id and score bytes; tests/test_cpp_bow.py compares them with
// tests/bow_ref.py.  Exit codes: 0 ok, 1 a check of the reference's test failed, 2 usage, 3 no GPU.
#include <cstdio>
#include <cstring>
#include <iostream>
#include "dvslam/place_recognition.hpp"

typedef dvslam::OrbVocabulary OrbVocabulary;
typedef dvslam::OrbDatabase OrbDatabase;

static int failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static void print_results(const char* tag, const dvslam::QueryResults& results) {
  std::printf("%s %zu", tag, results.size());
  for (const dvslam::Result& r : results) {
    uint64_t bits;
    std::memcpy(&bits, &r.Score, 8);
    std::printf(" %u:%016llx", r.Id, (unsigned long long)bits);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (dvs_device_count() < 1) { std::fprintf(stderr, "no GPU: there is no CPU fallback\n"); return 3; }
  if (argc != 3) { std::fprintf(stderr, "usage: %s vocabulary.txt descriptors.bin\n", argv[0]); return 2; }
  dvslam::DescriptorVector descriptor_vector;
  {
    FILE* fp = std::fopen(argv[2], "rb");
    int32_t n = 0;
    if (!fp || std::fread(&n, 4, 1, fp) != 1 || n < 0) return 2;
    descriptor_vector.resize(n);
    if (n && std::fread(descriptor_vector[0].data(), 32, n, fp) != (size_t)n) return 2;
    std::fclose(fp);
  }

  OrbVocabulary vocabulary;
  std::string vocab_path = argv[1];

  bool vocab_loaded = false;
  try {
    vocabulary.loadFromTextFile(vocab_path);
    vocab_loaded = true;
  } catch (const std::exception& e) {
    std::cout << "Failed to load vocabulary from: " << vocab_path << std::endl;
    std::cout << "Error: " << e.what() << std::endl;
  }

  EXPECT_TRUE(vocab_loaded);
  EXPECT_TRUE(vocabulary.size() > 0);
  if (!vocab_loaded) return 1;

  // Create database with the loaded vocabulary
  OrbDatabase database(vocabulary);
  dvslam::EntryId entry_id;

  entry_id = database.add(descriptor_vector);

  EXPECT_TRUE((int)entry_id >= 0);

  // Test querying
  dvslam::QueryResults results;
  database.query(descriptor_vector, results, 1);

  EXPECT_TRUE(results.size() > 0);

  if (!results.empty()) {
    EXPECT_TRUE(results[0].Id == entry_id);
    EXPECT_TRUE(results[0].Score > 0.0);
  }
  std::printf("words %u entry %u size %u\n", vocabulary.size(), entry_id, database.size());
  print_results("query1", results);

  // beyond the reference's test: a second entry (the first half of the rows), every result, and the BowVector itself
  dvslam::DescriptorVector half(descriptor_vector.begin(), descriptor_vector.begin() + descriptor_vector.size() / 2);
  const dvslam::EntryId second = database.add(half);
  database.query(descriptor_vector, results, 0);
  std::printf("second %u\n", second);
  print_results("queryall", results);
  dvslam::BowVector v;
  dvslam::FeatureVector fv;
  vocabulary.transform(descriptor_vector, v, fv, 1);
  std::printf("bow %zu", v.size());
  for (const auto& kv : v) {
    uint64_t bits;
    std::memcpy(&bits, &kv.second, 8);
    std::printf(" %u:%016llx", kv.first, (unsigned long long)bits);
  }
  std::printf("\nfv %zu", fv.size());
  for (const auto& kv : fv) {
    std::printf(" %u:", kv.first);
    for (size_t i = 0; i < kv.second.size(); i++) std::printf(i ? ",%u" : "%u", kv.second[i]);
  }
  std::printf("\n");
  return failures ? 1 : 0;
}
