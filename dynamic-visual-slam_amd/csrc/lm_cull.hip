// lm_cull.hip — landmark tracking statistics and landmark culling on the map the backend keeps on the device (include/dvslam_hip.h
// "Landmark culling"; the rule is stated there in full and restated in tests/landmark_culling_ref.py).
//
// The statistics are a side table of the handle (backend_internal.h, LmStatRows): id ascending, visible, found, joined to the landmark
// table by id and never a column of it.  Every call of the section aligns them first; the recording itself is map_track.hip's
// k_mt_record_stats, at the end of the dvs_backend_track_frame* calls.
//   k_ls_align      a landmark row per lane: lm_find of its id in the old statistics, a hit carries its counters over, a miss starts at 0 / 0
//   k_ls_set        a row of the caller's arrays per lane: lm_find of its id in the aligned statistics, ids the map does not hold are skipped
//   k_lc_views      a landmark row per lane over backend.hip's landmark -> views CSR: n, and the age in keyframes of its first valid view
//   k_lc_decide     a landmark row per lane: the first rule that holds (F, then W), the stay / leave flags, the two counts
//   CulledIdEmit    the culled ids and reasons in ascending id (table_compact.h's compact_rows)
//   k_lc_ob_flag    an observation row per lane: it leaves iff the landmark row it names leaves
//   StatRide        the apply is table_compact.h's tables_replace, dvs_backend_prune's cascade included; a landmark row that stays takes its
//                   statistics row along into the statistics' spare
// No atomics but the two counts, no order dependence: everything is integers and total orders.
#include <string.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "matcher.h"
#include "backend_internal.h"
#include "block_ops.h"
#include "table_compact.h"

namespace dvs {

__global__ __launch_bounds__(256) void k_ls_align(const i64* __restrict__ lm_id, int nlm, StatView old, int nold, StatView nw) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  const i64 key = lm_id[s];
  const int r = lm_find(old.id, nold, key);
  nw.id[s] = key; nw.visible[s] = r >= 0 ? old.visible[r] : 0; nw.found[s] = r >= 0 ? old.found[r] : 0;
}

__global__ __launch_bounds__(256) void k_ls_set(int n, const i64* __restrict__ id, const int* __restrict__ visible, const int* __restrict__ found, StatView st, int nstat) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int s = lm_find(st.id, nstat, id[r]);
  if (s >= 0) { st.visible[s] = visible[r]; st.found[s] = found[r]; }
}

// n[s] = the views of landmark row s; age[s] = (nkf - 1) - the keyframe of its first view in observation order that is a keyframe of the map
// (view_kf is -1 where it is none), -1 without such a view
__global__ __launch_bounds__(256) void k_lc_views(int nlm, int nkf, const i64* __restrict__ offs, const int* __restrict__ view_kf, int* __restrict__ n, int* __restrict__ age) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  const i64 b = offs[s], e = offs[s + 1];
  int first = -1;
  for (i64 p = b; p < e && first < 0; p++) first = view_kf[p];
  n[s] = (int)(e - b);
  age[s] = first >= 0 ? (nkf - 1) - first : -1;
}

__global__ __launch_bounds__(256) void k_lc_decide(int nlm, dvs_lm_cull_params P, const int* __restrict__ visible, const int* __restrict__ found, const int* __restrict__ n,
                                                   const int* __restrict__ age, int* __restrict__ reason, int* __restrict__ keep, int* __restrict__ mark,
                                                   LmCullCounts* __restrict__ counts) {
  __shared__ int s_w[4];
  const int s = blockIdx.x * 256 + threadIdx.x;
  int r = 0;
  if (s < nlm) {
    const int v = visible[s], f = found[s];
    if (P.found_ratio_pct > 0 && v >= P.min_visible && (i64)f * 100 < (i64)P.found_ratio_pct * (i64)v) r = 1;
    else if (P.weak_age_kf >= 0 && age[s] >= P.weak_age_kf && n[s] <= P.weak_max_views) r = 2;
    reason[s] = r; keep[s] = r == 0 ? 1 : 0; mark[s] = r != 0 ? 1 : 0;
  }
  const int t1 = block_count256(r == 1, s_w);
  const int t2 = block_count256(r == 2, s_w);
  if (threadIdx.x == 0) {
    if (t1) atomicAdd(&counts->n_by_ratio, t1);
    if (t2) atomicAdd(&counts->n_weak, t2);
  }
}

// the compaction over the marked rows: their ids and reasons in table order, which is ascending id
struct CulledIdEmit {
  const i64* lm_id; const int* reason; i64* cid; int* creason;
  __device__ void operator()(size_t s, size_t p) const { cid[p] = lm_id[s]; creason[p] = reason[s]; }
};

// ob_slot: the landmark row an observation row names, -1 if the table does not hold it (backend.hip, k_views_count)
__global__ __launch_bounds__(256) void k_lc_ob_flag(const int* __restrict__ ob_slot, int nob, const int* __restrict__ mark, int* __restrict__ keep, int* __restrict__ gone) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nob) return;
  const int s = ob_slot[i];
  const int g = (s >= 0 && mark[s] == 1) ? 1 : 0;
  keep[i] = 1 - g; gone[i] = g;
}

// a landmark row that stays, every column as it was: its statistics row stays with it
struct StatRide {
  StatView st, ns;
  __device__ void operator()(const LmView&, size_t p, const LmView&, size_t s) const { ns.id[p] = st.id[s]; ns.visible[p] = st.visible[s]; ns.found[p] = st.found[s]; }
};

}  // namespace dvs

using namespace dvs;

// Nothing is cached about "the map did not change": every call of the section aligns.
dvs_status dvs::lm_stats_align(dvs_backend* h) {
  const int nlm = h->nlm;
  if (nlm == 0) { h->nstat = 0; return DVS_OK; }
  DVS_HIP(hipSetDevice(h->device));
  DVS_TRY(h->stat_spare.grow((size_t)nlm));
  hipLaunchKernelGGL(k_ls_align, dim3((nlm + 255) / 256), dim3(256), 0, h->ctx->stream, (const i64*)h->lm.id.get(), nlm, stat_view(h->stat), h->nstat, stat_view(h->stat_spare));
  DVS_HIP(hipGetLastError());
  std::swap(h->stat, h->stat_spare);
  h->nstat = nlm;
  return DVS_OK;
}

namespace {

dvs_status lc_check(const dvs_lm_cull_params& P) {
  DVS_ARG(P.found_ratio_pct <= 100);
  DVS_ARG(P.min_visible >= 1);
  DVS_ARG(P.weak_max_views >= 0);
  return DVS_OK;
}

// n and age_kf of every landmark row into lc_lm.n / .age; needs at least one landmark
dvs_status lc_views(dvs_backend* h) {
  const int nlm = h->nlm;
  DVS_TRY(h->lc_lm.grow((size_t)nlm));
  DVS_TRY(backend_views_build(h));
  hipLaunchKernelGGL(k_lc_views, dim3((nlm + 255) / 256), dim3(256), 0, h->ctx->stream, nlm, (int)h->kfs.size(), (const i64*)h->v_lm.offs.get(), (const int*)h->v_ob.kf.get(),
                     h->lc_lm.n.get(), h->lc_lm.age.get());
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

}  // namespace

extern "C" {

void dvs_lm_cull_default_params(dvs_lm_cull_params* p) {
  if (!p) return;
  p->found_ratio_pct = 25; p->min_visible = 4; p->weak_age_kf = 2; p->weak_max_views = 1;
}

dvs_status dvs_backend_set_tracking_stats(dvs_backend* h, int32_t on) {
  DVS_ARG(h);
  h->stats_on = on != 0 ? 1 : 0;
  return DVS_OK;
}

dvs_status dvs_backend_clear_landmark_stats(dvs_backend* h) {
  DVS_ARG(h);
  h->nstat = 0; h->n_recorded = 0;                     // the next alignment finds no id: every counter starts at 0 / 0
  return DVS_OK;
}

dvs_status dvs_backend_get_landmark_stats(dvs_backend* h, int32_t cap, uint64_t* id, int32_t* visible, int32_t* found, int32_t* n_views, int32_t* age_kf, int32_t* n,
                                          int64_t* n_frames_recorded) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->nlm;
  if (n_frames_recorded) *n_frames_recorded = h->n_recorded;
  const bool want = id || visible || found || n_views || age_kf;
  if (want && h->nlm > cap) { set_error("dvs_backend_get_landmark_stats: %d landmarks, capacity %d", h->nlm, cap); return DVS_ERR_CAPACITY; }
  if (!want || h->nlm == 0) return DVS_OK;
  const size_t nlm = (size_t)h->nlm;
  hipStream_t st = h->ctx->stream;
  DVS_TRY(lm_stats_align(h));
  if (n_views || age_kf) DVS_TRY(lc_views(h));
  DVS_TRY(copy_out(id, h->stat.id, nlm, st)); DVS_TRY(copy_out(visible, h->stat.visible, nlm, st)); DVS_TRY(copy_out(found, h->stat.found, nlm, st));
  if (n_views) DVS_TRY(copy_out(n_views, h->lc_lm.n, nlm, st));
  if (age_kf) DVS_TRY(copy_out(age_kf, h->lc_lm.age, nlm, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_set_landmark_stats(dvs_backend* h, int32_t n_rows, const uint64_t* id, const int32_t* visible, const int32_t* found) {
  DVS_ARG(h && n_rows >= 0 && (n_rows == 0 || (id && visible && found)));
  for (int r = 0; r < n_rows; r++) {
    DVS_ARG(r == 0 || id[r - 1] < id[r]);
    DVS_ARG(found[r] >= 0 && found[r] <= visible[r]);
  }
  if (n_rows == 0 || h->nlm == 0) return DVS_OK;
  hipStream_t st = h->ctx->stream;
  DVS_TRY(lm_stats_align(h));
  if ((size_t)n_rows > h->c_ai64 || 2 * (size_t)n_rows > h->c_aint) DVS_HIP(hipStreamSynchronize(st));   // nothing in flight reads what is freed
  DVS_TRY(grow(h->a_i64, h->c_ai64, (size_t)n_rows)); DVS_TRY(grow(h->a_int, h->c_aint, 2 * (size_t)n_rows));
  DVS_HIP(hipMemcpyAsync(h->a_i64.get(), id, (size_t)n_rows * 8, hipMemcpyHostToDevice, st));
  DVS_HIP(hipMemcpyAsync(h->a_int.get(), visible, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
  DVS_HIP(hipMemcpyAsync(h->a_int.get() + n_rows, found, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ls_set, dim3((n_rows + 255) / 256), dim3(256), 0, st, n_rows, (const i64*)h->a_i64.get(), (const int*)h->a_int.get(), (const int*)h->a_int.get() + n_rows,
                     stat_view(h->stat), h->nstat);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipStreamSynchronize(st));                   // the caller's arrays are read until here
  return DVS_OK;
}

dvs_status dvs_backend_cull_landmarks(dvs_backend* h, const dvs_lm_cull_params* params, int32_t apply, dvs_lm_cull_result* out, int32_t cap, uint64_t* culled_id,
                                      int32_t* culled_reason, int32_t* n_culled) {
  DVS_ARG(h && n_culled && cap >= 0);
  dvs_lm_cull_params P;
  if (params) P = *params; else dvs_lm_cull_default_params(&P);
  dvs_lm_cull_result res;
  memset(&res, 0, sizeof(res));
  *n_culled = 0;
  if (out) *out = res;
  DVS_TRY(lc_check(P));
  const int nlm = h->nlm, nob = h->nob;
  if (nlm == 0) return DVS_OK;
  hipStream_t st = h->ctx->stream;
  BackendSmall* sm = h->s_small.get();
  DVS_TRY(lm_stats_align(h));
  DVS_TRY(lc_views(h));
  DVS_TRY(compact_grow(h));
  // decide
  LmCullLmRows& G = h->lc_lm;
  DVS_HIP(hipMemsetAsync(&sm->lmcull, 0, sizeof(LmCullCounts), st));
  hipLaunchKernelGGL(k_lc_decide, dim3((nlm + 255) / 256), dim3(256), 0, st, nlm, P, (const int*)h->stat.visible.get(), (const int*)h->stat.found.get(), (const int*)G.n.get(),
                     (const int*)G.age.get(), G.reason.get(), h->cmp_lm.keep.get(), G.mark.get(), &sm->lmcull);
  DVS_HIP(hipGetLastError());
  int cnt[2] = {0, 0};
  DVS_TRY(small_read(h, &sm->lmcull.n_by_ratio, cnt, 2));
  if (cnt[0] < 0 || cnt[1] < 0 || (i64)cnt[0] + cnt[1] > nlm) { set_error("dvs_backend_cull_landmarks: inconsistent counts %d %d", cnt[0], cnt[1]); return DVS_ERR_HIP; }
  const int nc = cnt[0] + cnt[1];
  *n_culled = nc;
  if ((culled_id || culled_reason) && nc > cap) {
    set_error("dvs_backend_cull_landmarks: %d culled landmarks, capacity %d", nc, cap);
    return DVS_ERR_CAPACITY;
  }
  res.n_landmarks = nlm; res.n_by_ratio = cnt[0]; res.n_weak = cnt[1];
  if (nc && (culled_id || culled_reason)) {            // the report, in ascending id
    DVS_TRY(compact_rows(h, G.mark.get(), nlm, CulledIdEmit{h->lm.id.get(), G.reason.get(), G.cid.get(), G.creason.get()}));
    DVS_TRY(copy_out(culled_id, G.cid, (size_t)nc, st)); DVS_TRY(copy_out(culled_reason, G.creason, (size_t)nc, st));
    DVS_HIP(hipStreamSynchronize(st));
  }
  if (apply && nc) {
    // dvs_backend_prune's cascade; the statistics go into their spare with the landmark rows, and change places as the tables do
    DVS_TRY(h->stat_spare.grow((size_t)nlm));
    if (nob) hipLaunchKernelGGL(k_lc_ob_flag, dim3((nob + 255) / 256), dim3(256), 0, st, (const int*)h->v_ob.slot.get(), nob, (const int*)G.mark.get(), h->cmp_ob.keep.get(),
                                h->cmp_ob.gone.get());
    TablesReplaced done;
    DVS_TRY(tables_replace(h, "dvs_backend_cull_landmarks", h->cmp_lm.keep.get(), StatRide{stat_view(h->stat), stat_view(h->stat_spare)}, (i64)nlm - nc, h->cmp_ob.keep.get(),
                           RowAsIs(), -1, h->cmp_ob.gone.get(), &done));
    std::swap(h->stat, h->stat_spare);
    h->nstat = h->nlm;
    res.n_keyframes_touched = done.n_kf_touched; res.n_landmarks_removed = nc; res.n_observations_removed = done.n_ob_gone;
  }
  if (out) *out = res;
  return DVS_OK;
}

}  // extern "C"
