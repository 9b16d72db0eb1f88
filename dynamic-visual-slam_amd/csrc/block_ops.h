// block_ops.h — what one workgroup computes together: ordered compaction over four wavefronts (wave64 ballot + prefix count) and the
// fixed-tree reduction that makes the solvers reproducible.  Device-only, no state of its own: every function works in LDS scratch
// the caller provides, and every thread of the workgroup must call it (uniform control flow).
//
// Barrier contract, the same for everything here: a barrier stands before the first write to the scratch and another after its last
// read.  Calls may therefore follow each other on the same scratch with nothing in between, the scratch may be reused for anything
// else right after a call, and the result (in registers) is usable at once.
#pragma once
#include <hip/hip_runtime.h>

namespace dvs {

// how many flags of the wavefront's ballot b belong to lanes below this one
__device__ __forceinline__ int lanes_below(unsigned long long b) { return __popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// exclusive position of this thread's flag among the workgroup's 256 flags (thread order); total = how many are set.  s_w: 4 ints.
__device__ __forceinline__ int block_rank256(bool flag, int* s_w, int& total) {
  const unsigned long long b = __ballot(flag);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[w] = __popcll(b);
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; k++) base += s_w[k];
  total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return base + lanes_below(b);
}

// number of threads of the 256-thread workgroup with pred.  s_w: 4 ints.
__device__ __forceinline__ int block_count256(bool pred, int* s_w) {
  int total;
  block_rank256(pred, s_w, total);
  return total;
}

// The fixed-tree reduction.  NT threads (a power of two, the whole workgroup) each bring NV values v[0 .. NV); afterwards v[k] holds,
// in every thread, the reduction of the NT values of index k.  sm: NV * NT elements, laid out [NV][NT].
// THE ASSOCIATION IS THE CONTRACT: thread t folds the value of thread t + s into its own, op(own, other), for s = NT/2, NT/4, .. 1,
// whatever the schedule — so a floating-point sum has the same bits on every run, and an NV-wide call gives each of its values the
// bits that NV one-wide calls would.
template <int NT, int NV, typename T, typename Op>
__device__ __forceinline__ void block_reduce(T* v, T* sm, Op op) {
  static_assert(NT > 1 && (NT & (NT - 1)) == 0, "the tree halves NT down to 1");
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; k++) sm[k * NT + tid] = v[k];
  __syncthreads();
  for (int s = NT / 2; s > 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < NV; k++) sm[k * NT + tid] = op(sm[k * NT + tid], sm[k * NT + tid + s]);
    }
    __syncthreads();
  }
  // the last fold (s = 1: 1 into 0) by every thread for itself — the same two operands in the same order, so the same bits, and one
  // barrier less than letting thread 0 store it for the others
#pragma unroll
  for (int k = 0; k < NV; k++) v[k] = op(sm[k * NT], sm[k * NT + 1]);
  __syncthreads();
}

struct OpSum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMin { template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct OpFmax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

template <int NT, int NV, typename T>
__device__ __forceinline__ void block_sums(T* v, T* sm) { block_reduce<NT, NV>(v, sm, OpSum()); }
template <int NT, typename T>
__device__ __forceinline__ T block_sum(T v, T* sm) { block_reduce<NT, 1>(&v, sm, OpSum()); return v; }
template <int NT, typename T>
__device__ __forceinline__ T block_min(T v, T* sm) { block_reduce<NT, 1>(&v, sm, OpMin()); return v; }
template <int NT>
__device__ __forceinline__ double block_max(double v, double* sm) { block_reduce<NT, 1>(&v, sm, OpFmax()); return v; }

}  // namespace dvs
