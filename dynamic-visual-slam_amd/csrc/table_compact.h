// table_compact.h — the ordered compaction of a whole table, stated once for the backend's files: the rows whose flag is 1, in table order,
// in three steps of 256 rows per workgroup (count, scan of the workgroups' counts, gather at block offset + block_rank256), and on top of
// it the one way rows leave the map: both tables (or the landmark table alone) written into the handle's spare pair without the rows that
// leave, the host's cascade over the keyframes' observation_ids, then the swap.  block_ops.h holds the workgroup's half; this is the
// table's.  Internal to the library; everything is enqueued on the handle's stream.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>
#include "backend_internal.h"
#include "block_ops.h"

namespace dvs {

// step 1: how many of each workgroup's 256 rows are flagged (step 2: match.hip's scan).  One copy per file that compacts.
static __global__ __launch_bounds__(256) void k_compact_count(const int* __restrict__ flag, int n, int* __restrict__ blk) {
  __shared__ int s_w[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  int total;
  block_rank256(i < n && flag[i] == 1, s_w, total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}
// step 3: emit(i, p) for every flagged row i, p its position among the flagged rows.  Emit: a plain struct of views and pointers.
template <class Emit>
__global__ __launch_bounds__(256) void k_compact_rows(const int* __restrict__ flag, int n, const i64* __restrict__ blk_offs, Emit emit) {
  __shared__ int s_w[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool f = i < n && flag[i] == 1;
  int total;
  const size_t p = (size_t)blk_offs[blockIdx.x] + block_rank256(f, s_w, total);
  if (f) emit((size_t)i, p);
}

// where the three steps over n >= 1 rows leave the number of flagged rows on the device, until the handle's next compaction
inline const i64* compact_total(const dvs_backend* h, int n) { return h->blk.offs.get() + (n + 255) / 256; }

// The three steps over flag[0 .. n) (a flag other than 1 is not flagged), and the copy of the total to *total where asked: enqueued, not
// synchronised.  n == 0 launches nothing and the total is 0.  The caller has grown h->blk for n rows.
template <class Emit>
dvs_status compact_rows(dvs_backend* h, const int* flag, int n, Emit emit, i64* total = nullptr) {
  if (total) *total = 0;
  if (n <= 0) return DVS_OK;
  hipStream_t st = h->ctx->stream;
  const int nblk = (n + 255) / 256;
  hipLaunchKernelGGL(k_compact_count, dim3(nblk), dim3(256), 0, st, flag, n, h->blk.cnt.get());
  launch_scan_counts(st, (const int*)h->blk.cnt.get(), nblk, h->blk.offs.get());
  hipLaunchKernelGGL(k_compact_rows<Emit>, dim3(nblk), dim3(256), 0, st, flag, n, (const i64*)h->blk.offs.get(), emit);
  DVS_HIP(hipGetLastError());
  if (total) DVS_HIP(hipMemcpyAsync(total, compact_total(h, n), sizeof(i64), hipMemcpyDeviceToHost, st));
  return DVS_OK;
}

// A table row that stays: the row copy, then what the caller changes in the copy.  Fix: fix(dst, p, src, i), a plain struct as an Emit is.
struct RowAsIs { template <class View> __device__ void operator()(const View&, size_t, const View&, size_t) const {} };
template <class Fix> struct LmRowEmit {
  LmView src, dst; Fix fix;
  __device__ void operator()(size_t i, size_t p) const { lm_row_copy(dst, p, src, i); fix(dst, p, src, i); }
};
template <class Fix> struct ObRowEmit {
  ObView src, dst; Fix fix;
  __device__ void operator()(size_t i, size_t p) const { ob_row_copy(dst, p, src, i); fix(dst, p, src, i); }
};
// an observation row that leaves: what the host's cascade reads
struct RemovedEmit {
  const i64* ob_id; const int* ob_kf; i64* rem_id; int* rem_kf;
  __device__ void operator()(size_t i, size_t p) const { rem_id[p] = ob_id[i]; rem_kf[p] = ob_kf[i]; }
};

// the compaction's flags for the tables as they stand (h->cmp_lm, h->cmp_ob) and the block scratch for them
inline dvs_status compact_grow(dvs_backend* h) {
  DVS_TRY(h->cmp_lm.grow((size_t)h->nlm)); DVS_TRY(h->cmp_ob.grow((size_t)h->nob));
  return h->blk.grow((size_t)std::max(h->nlm, h->nob) / 256 + 2);
}

struct TablesReplaced { int n_ob_gone = 0, n_kf_touched = 0; };

// The map's tables without the rows that leave.  lm_keep / ob_keep: the rows that stay (ob_keep null: the observation table is not
// touched); ob_gone (or null): the observation rows whose ids the keyframes' observation_ids lose.  want_lm, want_ob: the rows the
// caller expects to stay (want_ob < 0: whatever the gone rows leave).  In order: the spare pair as large as the live one, the
// compactions, one synchronisation, the counts checked (DVS_ERR_HIP in `who`'s name, the map untouched), the cascade, the swaps.
template <class LmFix, class ObFix>
dvs_status tables_replace(dvs_backend* h, const char* who, const int* lm_keep, LmFix lm_fix, i64 want_lm, const int* ob_keep, ObFix ob_fix, i64 want_ob,
                          const int* ob_gone, TablesReplaced* out) {
  const int nlm = h->nlm, nob = h->nob;
  hipStream_t st = h->ctx->stream;
  DVS_TRY(table_match_spare(h->lm_spare, h->lm));
  if (ob_keep) DVS_TRY(table_match_spare(h->ob_spare, h->ob));
  i64 kept_lm = 0, kept_ob = nob, gone_ob = 0;
  DVS_TRY(compact_rows(h, lm_keep, nlm, LmRowEmit<LmFix>{h->lm.view(), h->lm_spare.view(), lm_fix}, &kept_lm));
  if (ob_keep) DVS_TRY(compact_rows(h, ob_keep, nob, ObRowEmit<ObFix>{h->ob.view(), h->ob_spare.view(), ob_fix}, &kept_ob));
  if (ob_gone) DVS_TRY(compact_rows(h, ob_gone, nob, RemovedEmit{h->ob.id.get(), h->ob.kf.get(), h->cmp_ob.rem_id.get(), h->cmp_ob.rem_kf.get()}, &gone_ob));
  DVS_HIP(hipStreamSynchronize(st));
  if (kept_lm != want_lm || (want_ob >= 0 && kept_ob != want_ob) || kept_ob < 0 || gone_ob < 0 || (ob_gone && kept_ob + gone_ob != (i64)nob)) {
    set_error("%s: inconsistent counts %lld %lld %lld", who, (long long)kept_lm, (long long)kept_ob, (long long)gone_ob);
    return DVS_ERR_HIP;
  }
  if (ob_gone) {
    std::vector<i64> rid((size_t)gone_ob);
    std::vector<int> rkf((size_t)gone_ob);
    if (gone_ob) {
      DVS_TRY(copy_out(rid.data(), h->cmp_ob.rem_id, rid.size(), st)); DVS_TRY(copy_out(rkf.data(), h->cmp_ob.rem_kf, rkf.size(), st));
      DVS_HIP(hipStreamSynchronize(st));
    }
    out->n_kf_touched = backend_drop_observation_ids(h, rid, rkf);
  }
  out->n_ob_gone = (int)gone_ob;
  std::swap(h->lm, h->lm_spare);
  if (ob_keep) std::swap(h->ob, h->ob_spare);
  h->nlm = (int)kept_lm; h->nob = (int)kept_ob;
  return DVS_OK;
}

}  // namespace dvs
