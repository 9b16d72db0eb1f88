// The reference's feature-culling steps (frontend.cpp:1193-1219) with the REAL std::sort on std::pair<float, int>, for
// tests/test_tracker_cull_order.py: reads "n max_new min_response" and n lines "response matched" from stdin, prints the indices the
// loop adds, one per line.  With a second argument "stable" it sorts with std::stable_sort instead (the order the Python replay uses).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

int main(int argc, char** argv) {
  const bool stable = argc > 1 && std::strcmp(argv[1], "stable") == 0;
  int n = 0, max_new = 0;
  float min_response = 0.f;
  if (std::scanf("%d %d %f", &n, &max_new, &min_response) != 3) return 2;
  std::vector<std::pair<float, int>> unmatched_features;
  for (int i = 0; i < n; i++) {
    float response; int matched;
    if (std::scanf("%f %d", &response, &matched) != 2) return 2;
    if (!matched) unmatched_features.push_back({response, i});
  }
  auto cmp = [](const auto& a, const auto& b) { return a.first > b.first; };
  if (stable) std::stable_sort(unmatched_features.begin(), unmatched_features.end(), cmp);
  else std::sort(unmatched_features.begin(), unmatched_features.end(), cmp);
  int added_new = 0;
  for (const auto& [response, idx] : unmatched_features) {
    if (added_new >= max_new || response < min_response) break;
    std::printf("%d\n", idx);
    added_new++;
  }
  return 0;
}
