// cull_order.h — the ORDER of the tracker's feature culling (frontend.cpp:1193-1219), compiled for the device (k_cull in tracker.hip)
// and for the host (dvs_test_cull_order, which the CPU suite holds against the real std::sort).
// The reference sorts std::pair<float, int>(response, index) with std::sort under the comparator a.first > b.first: the index takes no
// part in the order, FAST scores are small integers with many ties, so which features survive the cut at 200 is decided by libstdc++'s
// introsort.  lsort::sort is its replica; an element here is a 64-bit word whose upper half orders like the comparator and whose lower
// half carries the index.
#pragma once
#include <stdint.h>
#include <string.h>
#include "lsort.h"

namespace dvs {

// upper half: a 32-bit key with key(a) < key(b)  <=>  a > b as floats (NaN excluded; -0 = +0)
LSORT_HD uint32_t cull_key32(float response) {
  if (response == 0.0f) response = 0.0f;
  uint32_t u;
  memcpy(&u, &response, 4);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending in the float's order
  return ~u;
}
LSORT_HD uint64_t cull_key(float response, int index) { return ((uint64_t)cull_key32(response) << 32) | (uint32_t)index; }

// how many of the sorted keys the loop at frontend.cpp:1209-1219 adds: it stops at max_new or at the first response < min_response
LSORT_HD int cull_cut(const uint32_t* key32_sorted, int n, int max_new, float min_response) {
  const uint32_t kmin = cull_key32(min_response);
  int m = 0;
  while (m < n && m < max_new && key32_sorted[m] <= kmin) m++;   // response >= min_response
  return m;
}

// Host statement of what k_cull runs: keys[0 .. n) = the unmatched features in index order, sorted as std::sort sorts them through
// lsort::sort_ranked — the rank-pairing form of the same introsort (lsort.h), which the kernel mirrors with one wavefront per partition
// (wave_partition<32>) and one lane per element for the leaves.  Lp / Rp: scratch of n ints each.  Returns the cut.
inline int cull_sort_and_cut(uint64_t* keys, int n, int max_new, float min_response, int* Lp, int* Rp, uint32_t* key32) {
  lsort::sort_ranked(keys, (long)n, lsort::Less<32>(), Lp, Rp);
  for (int i = 0; i < n; i++) key32[i] = (uint32_t)(keys[i] >> 32);
  return cull_cut(key32, n, max_new, min_response);
}

}  // namespace dvs
