// splitmix64.h — the one mixing function behind the library's stated samplers (ransac.hip's hypothesis samples, bow_train.hip's
// k-means++ draws): host and device compute the same value.
#pragma once
#include <hip/hip_runtime.h>

namespace dvs {

__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace dvs
