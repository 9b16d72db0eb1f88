// io_host.h — the host side of in / out without copy commands: the polled wait for a sequence number a kernel publishes in pinned
// memory, and the pinned block of the matcher context (matcher.h).  No kernel is defined here: io_pinned.h adds the import / export
// kernels and the two operations that launch them, for the translation units that use them.
#pragma once
#include <chrono>
#include "device_mem.h"

namespace dvs {

// Wait until the kernel enqueued on st has published `seq` in *hseq: a spin bounded by spin_ms, then the stream wait.
inline dvs_status io_wait(const volatile int* hseq, int seq, hipStream_t st, int spin_ms = 5) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int spin = 1; *hseq != seq; spin++) {
    __builtin_ia32_pause();
    if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(spin_ms)) break;
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (*hseq != seq) DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

// The pinned in / out block of the small host entry points (match, glue, RANSAC stages), the sequence word the device publishes and
// the host's count of the numbers issued.  A caller reserves the block, places its inputs in it, imports them, launches its work and
// fetches the result region; every call on the handle shares the one counter, so a number is never published twice.
struct PinnedIo {
  PinnedBuf<uint8_t> block;
  size_t cap = 0;
  PinnedBuf<int> seq_word;
  int issued = 0;

  uint8_t* h() const { return block.get(); }
  // At least `bytes`, never below 64 KB: the small calls never regrow it.  A call may have returned with its import kernel still
  // reading the block (fm_cv_device, pnp_cv_device), so st is synchronised before the block is released.
  dvs_status reserve(hipStream_t st, size_t bytes) {
    if (bytes > cap && block.get()) DVS_HIP(hipStreamSynchronize(st));
    DVS_TRY(grow(block, cap, std::max<size_t>(bytes, 65536)));
    if (!seq_word.get()) { DVS_TRY(seq_word.alloc(16)); *seq_word.get() = 0; issued = 0; }
    return DVS_OK;
  }
  // for a kernel that publishes the number itself (k_filter_depth): take the next one, launch, wait
  int next_seq() { return ++issued; }
  dvs_status wait(hipStream_t st, int seq) const { return io_wait(seq_word.get(), seq, st); }
  // (io_pinned.h) enqueue k_io_import of `bytes` (whole dwords) from h() + h_off to d_dst
  void import(hipStream_t st, void* d_dst, size_t bytes, size_t h_off = 0) const;
  // (io_pinned.h) `bytes` (whole dwords) from d_src into h_dst, a place in the block, complete on return: up to export_max bytes by
  // k_io_export and the polled wait (no copy command, no wake-up), above by a copy command and the stream wait
  dvs_status fetch(hipStream_t st, const void* d_src, void* h_dst, size_t bytes, size_t export_max);
};

}  // namespace dvs
