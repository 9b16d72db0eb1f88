// device_mem.h — owners of what a handle holds on the device: hipMalloc / hipHostMalloc blocks, streams, events, and the rings of buffer
// sets a pipelined caller's batches rotate through; and the Carver that lays sub-buffers out in one block.  Internal to the library;
// nothing here is exported.  Each resource is freed exactly once because its owner cannot be copied: a handle's "free everything" is the
// assignment of an empty struct of these.  A handle declares its own stream BEFORE its buffers, so that the stream outlives them.
#pragma once
#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>
#include "common.h"

namespace dvs {

// Move-only owner of `count` elements of device (Pinned: page-locked host) memory.  Kernels take get(), never the owner.
template <class T, bool Pinned>
class Buf {
 public:
  T* get() const { return p_.get(); }
  dvs_status alloc(size_t count) {   // frees what it held; never a zero-byte block
    p_.reset();
    T* p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    DVS_HIP(Pinned ? hipHostMalloc((void**)&p, bytes) : hipMalloc((void**)&p, bytes));
    p_.reset(p);
    return DVS_OK;
  }
  dvs_status upload(const std::vector<T>& v) {
    DVS_TRY(alloc(v.size()));
    if (!v.empty()) DVS_HIP(hipMemcpy(get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return DVS_OK;
  }
 private:
  struct Free { void operator()(T* p) const { (void)(Pinned ? hipHostFree(p) : hipFree(p)); } };
  std::unique_ptr<T, Free> p_;
};
template <class T> using DeviceBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// A device column of a table or of a row group: Per elements for every row, and Extra more behind the last row.  The type carries what
// an allocation and a copy of `rows` rows need, so no caller writes a byte count.
template <class T, int Per = 1, int Extra = 0>
struct Column : DeviceBuf<T> {
  dvs_status alloc_rows(size_t rows) { return this->alloc(rows * Per + Extra); }
  static constexpr size_t row_bytes = Per * sizeof(T);
};
template <class... C>
dvs_status alloc_rows(size_t rows, C&... cols) {   // in the order given; stops at the first failure
  dvs_status s = DVS_OK;
  (void)(... && ((s = cols.alloc_rows(rows)) == DVS_OK));
  return s;
}
// `n` rows of a column to the host, enqueued; nothing for a null destination (an output the caller did not ask for)
template <class D, class T, int Per, int Extra>
dvs_status copy_out(D* dst, const Column<T, Per, Extra>& src, size_t n, hipStream_t st) {
  static_assert(sizeof(D) == sizeof(T), "the destination's elements are the column's");
  if (dst) DVS_HIP(hipMemcpyAsync(dst, src.get(), n * src.row_bytes, hipMemcpyDeviceToHost, st));
  return DVS_OK;
}

// and `n` rows from the host into a column, enqueued
template <class S, class T, int Per, int Extra>
dvs_status copy_in(Column<T, Per, Extra>& dst, const S* src, size_t n, hipStream_t st) {
  static_assert(sizeof(S) == sizeof(T), "the source's elements are the column's");
  DVS_HIP(hipMemcpyAsync(dst.get(), src, n * dst.row_bytes, hipMemcpyHostToDevice, st));
  return DVS_OK;
}

// A row group: columns that share a row count and only grow.  Kept while `need` rows fit in `cap`, else every column is freed and
// allocated for `size` rows.  cap is zero from before the first allocation until the last one has succeeded: after a failure the group
// counts as empty, so the next call allocates all of it again and every owner still frees once.
template <class... C>
dvs_status grow_rows(size_t& cap, size_t need, size_t size, C&... cols) {
  if (need <= cap) return DVS_OK;
  cap = 0;
  DVS_TRY(alloc_rows(size, cols...));
  cap = size;
  return DVS_OK;
}
// The group of one block, with a quarter to spare.
template <class T, bool Pinned>
dvs_status grow(Buf<T, Pinned>& buf, size_t& cap, size_t need) {
  if (need <= cap) return DVS_OK;
  cap = 0;
  DVS_TRY(buf.alloc(need + need / 4));
  cap = need + need / 4;
  return DVS_OK;
}

// Move-only owner of another handle of the library (what a dvs_*_create returned), released by that handle's own destroy function.
template <class T, void (*Destroy)(T*)>
struct DestroyWith { void operator()(T* p) const { Destroy(p); } };
template <class T, void (*Destroy)(T*)>
using Owned = std::unique_ptr<T, DestroyWith<T, Destroy>>;

// Move-only owner of an event, without timing unless asked.  Empty until create(): a handle can be built (and destroyed) without a device.
class Event {
 public:
  hipError_t create(bool timing = false) {
    hipEvent_t e = nullptr;
    const hipError_t r = hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming);
    e_.reset(e);
    return r;
  }
  operator hipEvent_t() const { return e_.get(); }
 private:
  struct Destroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
  std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> e_;
};

// Move-only owner of a non-blocking stream.  Empty until create(); every HIP stream is a hardware queue, so a handle creates one only
// when it is used.  priority_class > 0 / < 0: the device's highest / lowest dispatch priority (as dvs_stream_create).
class Stream {
 public:
  hipError_t create(int priority_class = 0) {
    hipStream_t s = nullptr;
    int lo = 0, hi = 0;
    if (priority_class) (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    const hipError_t r = priority_class ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority_class > 0 ? hi : lo)
                                        : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    s_.reset(s);
    return r;
  }
  operator hipStream_t() const { return s_.get(); }
 private:
  struct Destroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
  std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroy> s_;
};

// Lays the buffers of a block out: run over a null base for the size, then over the block for the pointers.  Every buffer starts on a
// multiple of `align` bytes (a power of two) behind the base, and an empty one still takes one unit: no two buffers share an address.
struct Carver {
  uint8_t* base;
  size_t align = 256;
  size_t used = 0;
  template <class T> void take(T*& p, size_t count) {
    p = base ? (T*)(base + used) : nullptr;
    used += (std::max<size_t>(count * sizeof(T), 1) + align - 1) & ~(align - 1);
  }
};

// Four slots of which the first `depth` (3 or 4) are used in turn.  A slot is a small struct of owners; its user allocates a slot when
// the rotation first reaches it.
template <class Slot>
struct Ring {
  Slot slot[4];
  int idx = 0, depth = 3;
  Slot& cur() { return slot[idx]; }
  Slot& next() { return slot[(idx + 1) % depth]; }
  Slot& at(int k) { return slot[k]; }
  void advance() { idx = (idx + 1) % depth; }
  void rewind(int d) { idx = 0; depth = d; }   // everything idle: restart at the first slot, `d` slots from now on
};

}  // namespace dvs
