// block_rank.h — ordered compaction inside one workgroup of four wavefronts (tracker.hip, backend.hip): wave64 ballot + prefix count.
#pragma once
#include <hip/hip_runtime.h>

namespace dvs {

// exclusive position of this thread's flag among the workgroup's 256 flags (thread order); total = how many are set.  s_w: 4 ints.
__device__ __forceinline__ int block_rank256(bool flag, int* s_w, int& total) {
  const unsigned long long b = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();                       // s_w may still be read from the trip before
  if (lane == 0) s_w[w] = __popcll(b);
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; k++) base += s_w[k];
  total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  return base + __popcll(b & ((1ull << lane) - 1ull));
}

}  // namespace dvs
