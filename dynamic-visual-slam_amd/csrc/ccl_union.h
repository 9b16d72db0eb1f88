// ccl_union.h — find / union of the connected-component labelling (motion_seg.hip), written once over a memory policy so that the same
// text runs on LDS, on global memory under agent-scope atomics, and on the host (tests/cpp/ccl_union_host.cpp).
//
// The forest: parent[i] is an element index, parent[i] <= i always, a root has parent[i] == i.  Everything starts as its own root (or as
// any forest with parent[i] <= i).  A policy M gives
//   int load(int i)               the current parent[i]
//   int fetch_min(int i, int v)   parent[i] = min(parent[i], v) as ONE atomic step; returns the value it replaced
// and nothing else ever writes parent[].  So parent[i] only ever DECREASES, and never below 0.
//
// Why every loop ends, whatever the other threads do:
//   find(a)     each step replaces a by parent[a] < a (the loop ends at parent[a] == a): a strictly decreasing chain of non-negative integers.
//   unite(a, b) one round finds both roots, orders them a > b and tries fetch_min(a, b).  It decides on the RETURNED value `old`, never
//               on a separate read: old == a means a was still a root at that instant and now hangs under b — done.  Otherwise another
//               thread had already hung a under old < a; parent[a] is now min(old, b), and what is left to join is (old, b): the
//               next round starts from old < a.  b never grows (find only descends).  So a + b strictly decreases from round to round, and
//               the rounds end at a == b at the latest.
// Why the result does not depend on the schedule: a link always goes from a root to a smaller index, and a link that fetch_min
// replaces (a -> old by a -> b, b < old) is re-established by the (old, b) round of the same call, so connectivity is never lost and only
// requested pairs are ever joined.  When all calls have returned the trees are exactly the classes of the requested pairs; every
// parent is <= its child, so each tree's root is its smallest member: find(i) is the class minimum.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DVS_CCL_FN __host__ __device__ __forceinline__
#else
#define DVS_CCL_FN inline
#endif

namespace dvs {

template <class M>
DVS_CCL_FN int ccl_find(M& m, int a) {
  for (;;) {
    const int p = m.load(a);
    if (p == a) return a;
    a = p;   // p < a
  }
}

template <class M>
DVS_CCL_FN void ccl_unite(M& m, int a, int b) {
  for (;;) {
    a = ccl_find(m, a);
    b = ccl_find(m, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = m.fetch_min(a, b);   // a > b
    if (old == a) return;                // a was a root and is linked now
    a = old;                             // a had been linked meanwhile (old < a): join its former parent with b
  }
}

// the host's (sequential) policy: a plain array
struct CclPlain {
  int* parent;
  DVS_CCL_FN int load(int i) { return parent[i]; }
  DVS_CCL_FN int fetch_min(int i, int v) {
    const int old = parent[i];
    if (v < old) parent[i] = v;
    return old;
  }
};

// 8-connected labelling of a rows x cols binary image (nonzero = set) on the host, through the routines above: label[p] = smallest linear
// index of p's component, -1 off the set; area[r] = pixels of the component whose label is r, 0 elsewhere.  The statement the kernels
// are compared with, and the sanitizer's target.
inline void ccl_label_host(const unsigned char* img, int rows, int cols, int* label, int* area) {
  const long long n = (long long)rows * cols;
  for (long long p = 0; p < n; p++) { label[p] = img[p] ? (int)p : -1; area[p] = 0; }
  CclPlain m{label};
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const int p = y * cols + x;
      if (!img[p]) continue;
      if (x > 0 && img[p - 1]) ccl_unite(m, p, p - 1);
      if (y > 0) {   // as in the kernels: a set pixel above makes the diagonals redundant (its row neighbours hang on it by their west links)
        if (img[p - cols]) {
          ccl_unite(m, p, p - cols);
        } else {
          if (x > 0 && img[p - cols - 1]) ccl_unite(m, p, p - cols - 1);
          if (x + 1 < cols && img[p - cols + 1]) ccl_unite(m, p, p - cols + 1);
        }
      }
    }
  for (long long p = 0; p < n; p++)
    if (img[p]) { label[p] = ccl_find(m, (int)p); }   // roots come first in index order, so a flattened entry is still a valid parent
  for (long long p = 0; p < n; p++)
    if (label[p] >= 0) area[label[p]]++;
}

}  // namespace dvs
