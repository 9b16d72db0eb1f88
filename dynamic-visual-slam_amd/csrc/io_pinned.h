// Pinned in / out for the small host entry points (match, RANSAC stages, the tracker's record): the two kernels and the operations of
// PinnedIo (io_host.h) that launch them.  A translation unit that only waits includes io_host.h and gains no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "io_host.h"

namespace dvs {
// in / out of the host entry points without copy commands: inputs sit in the matcher's pinned block and k_io_import brings them to
// the device; k_io_export (one workgroup) writes the contiguous result region back into the pinned block and publishes a sequence
// number behind a system-scope fence, which the host polls (bounded spin, then the stream wait).
static __global__ __launch_bounds__(256) void k_io_import(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int ndw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < ndw) dst[i] = src[i];
}
static __global__ __launch_bounds__(256) void k_io_export(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int ndw, int* __restrict__ hseq, int seq) {
  for (int i = threadIdx.x; i < ndw; i += 256) dst[i] = src[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) { *reinterpret_cast<volatile int*>(hseq) = seq; __threadfence_system(); }
}

// k_io_export of `bytes` from d_src to the pinned h_dst, publishing seq in *hseq, and the polled wait for it
inline dvs_status io_export_wait(hipStream_t st, const void* d_src, void* h_dst, size_t bytes, int* hseq, int seq) {
  hipLaunchKernelGGL(k_io_export, dim3(1), dim3(256), 0, st, (const uint32_t*)d_src, (uint32_t*)h_dst, (int)(bytes / 4), hseq, seq);
  DVS_HIP(hipGetLastError());
  return io_wait(hseq, seq, st);
}

inline void PinnedIo::import(hipStream_t st, void* d_dst, size_t bytes, size_t h_off) const {
  const int ndw = (int)(bytes / 4);
  hipLaunchKernelGGL(k_io_import, dim3((ndw + 255) / 256), dim3(256), 0, st, (const uint32_t*)(h() + h_off), (uint32_t*)d_dst, ndw);
}
inline dvs_status PinnedIo::fetch(hipStream_t st, const void* d_src, void* h_dst, size_t bytes, size_t export_max) {
  if (bytes <= export_max) return io_export_wait(st, d_src, h_dst, bytes, seq_word.get(), ++issued);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

}  // namespace dvs
