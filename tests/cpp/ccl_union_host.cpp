// csrc/ccl_union.h on the host (tests/test_motion_cpu.py builds this with -fsanitize=address,undefined and runs it directly): reads binary
// images {int32 rows, int32 cols, rows * cols bytes} from argv[1] until the file ends, labels each with ccl_label_host — the same find /
// unite the kernels of csrc/motion_seg.hip run — and writes {labels int32[rows * cols], areas int32[rows * cols]} per image to argv[2].
// Beside that it hangs a descending chain under the routines (the longest find a forest can hold) and joins it from both ends.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../dynamic-visual-slam_amd/csrc/ccl_union.h"

static int chain_check() {
  const int n = 100000;
  std::vector<int> parent((size_t)n);
  for (int i = 0; i < n; i++) parent[(size_t)i] = i ? i - 1 : 0;   // one chain n-1 -> ... -> 0
  dvs::CclPlain m{parent.data()};
  if (dvs::ccl_find(m, n - 1) != 0) return 1;
  for (int i = 0; i < n; i++) parent[(size_t)i] = i;
  for (int i = n - 1; i > 0; i -= 2) dvs::ccl_unite(m, i, i - 1);   // pairs, then the pairs to each other from the top down
  for (int i = n - 1; i > 1; i--) dvs::ccl_unite(m, i - 2, i);
  for (int i = 0; i < n; i++) {
    if (parent[(size_t)i] > i) return 2;
    if (dvs::ccl_find(m, i) != 0) return 3;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ccl_union_host patterns.bin labels.bin\n"); return 2; }
  const int c = chain_check();
  if (c) { fprintf(stderr, "chain check failed: %d\n", c); return 1; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  int32_t hdr[2];
  int images = 0;
  while (fread(hdr, 4, 2, in) == 2) {
    const size_t n = (size_t)hdr[0] * (size_t)hdr[1];
    std::vector<unsigned char> img(n);
    std::vector<int> label(n), area(n);
    if (fread(img.data(), 1, n, in) != n) { fprintf(stderr, "short image\n"); return 1; }
    dvs::ccl_label_host(img.data(), hdr[0], hdr[1], label.data(), area.data());
    if (fwrite(label.data(), 4, n, out) != n || fwrite(area.data(), 4, n, out) != n) return 1;
    images++;
  }
  fclose(in);
  fclose(out);
  printf("%d images\n", images);
  return 0;
}
