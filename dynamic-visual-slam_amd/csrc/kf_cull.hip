// kf_cull.hip — redundant keyframes leave the map the backend keeps on the device (include/dvslam_hip.h "Keyframe culling"; the rule is
// stated there in full and restated in tests/keyframe_culling_ref.py).
//
// Everything is derived from covisibility.hip's covis_prepare: the landmark -> views CSR (v_lm.offs / v_ob.kf), the counting views
// (cv_ob.kf) and the keyframe -> landmarks CSR (cv_kf.offs / cv_ob.list, a keyframe's landmark rows distinct and ascending).
//   k_cull_observers   c(L): a wavefront per landmark, its lanes stride the segment and count the counting views
//   k_cull_initial     one workgroup per keyframe: n_k, R_k under the initial counts, and whether it is a candidate that is redundant now
//   WalkEmit           the initially redundant candidates in ascending index (table_compact.h's compact_rows).  c(.) only decreases
//                      during the walk and n_k is constant, so a keyframe that is not redundant under the initial counts never becomes
//                      redundant: the walk visits only this list.
//   k_cull_walk        THE SEQUENTIAL PART.  One workgroup takes the listed keyframes in turn: its threads stride the keyframe's landmark
//                      rows, one block_sum, a uniform decision, and each thread takes 1 off c of its own rows.  The rows of one list are
//                      distinct, so plain stores do; one workgroup reads and writes c, so the barrier between a keyframe's decrements and
//                      the next keyframe's loads is the whole protocol.  No kernel waits on another workgroup; every loop is bounded by a
//                      count read before it starts.
//   k_cull_ob_flag / k_cull_lm_flag   the apply's flags: an observation row leaves iff its keyframe is culled; per landmark the removed
//                      rows among ALL its views and whether it stays (it leaves only as an orphan, and only if asked)
//   k_cull_kf_keep     keep flags of the keyframes; their exclusive scan is the new-index table ob.kf goes through
//   CullLmFix / CullObFix   the apply is table_compact.h's tables_replace: a row that stays is copied, then observation_count loses the
//                      removed rows and kf goes through the new-index table
// Scope and protection are decided on the host (local scope reads one neighbour list through covis_rows) and arrive as a byte per keyframe.
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

enum { CULL_OUT = 0, CULL_PROTECTED = 1, CULL_KEPT = 2, CULL_CULLED = 3 };   // kf_state; a candidate is CULL_KEPT until the walk culls it

__global__ __launch_bounds__(256) void k_cull_observers(int nlm, const i64* __restrict__ offs, const int* __restrict__ cv_kf, int* __restrict__ c) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nlm) return;                                // the whole wavefront
  const i64 b = offs[s], e = offs[s + 1];
  int n = 0;
  for (i64 p0 = b; p0 < e; p0 += 64) {
    const i64 p = p0 + lane;
    n += __popcll(__ballot(p < e && cv_kf[p] >= 0));
  }
  if (lane == 0) c[s] = n;
}

__device__ __forceinline__ bool cull_redundant(int r, int n, int percent) { return n >= 1 && 100ll * (i64)r > (i64)percent * (i64)n; }

// workgroup k, before the walk touches c: n_obs[k] = n_k, r0[k] = R_k under the initial c, flag[k] = 1 iff k is a candidate and redundant under it
__global__ __launch_bounds__(256) void k_cull_initial(const i64* __restrict__ kl_offs, const int* __restrict__ list, const int* __restrict__ c, int min_obs, int percent,
                                                      const uint8_t* __restrict__ state, int* __restrict__ n_obs, int* __restrict__ r0, int* __restrict__ flag) {
  __shared__ int sm[256];
  const int k = blockIdx.x;
  const i64 b = kl_offs[k];
  const int n = (int)(kl_offs[k + 1] - b);
  int r = 0;
  for (int j = threadIdx.x; j < n; j += 256) r += c[list[b + j]] - 1 >= min_obs ? 1 : 0;
  r = block_sum<256>(r, sm);
  if (threadIdx.x == 0) { n_obs[k] = n; r0[k] = r; flag[k] = (state[k] == CULL_KEPT && cull_redundant(r, n, percent)) ? 1 : 0; }
}

// the compaction over the keyframes: the flagged ones in ascending index
struct WalkEmit {
  int* walk;
  __device__ void operator()(size_t k, size_t p) const { walk[p] = (int)k; }
};

// ONE workgroup.  culled[] and *n_culled start at zero.  c is read and written here and by nobody else while this runs.
__global__ __launch_bounds__(256) void k_cull_walk(const i64* __restrict__ n_walk, int nkf, const int* __restrict__ walk, const i64* __restrict__ kl_offs,
                                                   const int* __restrict__ list, int* c, int min_obs, int percent, int max_cull, int* __restrict__ culled,
                                                   int* __restrict__ n_culled) {
  __shared__ int sm[256];
  const int nw = (int)min((i64)nkf, max((i64)0, *n_walk));
  int done = 0;
  for (int i = 0; i < nw; i++) {
    const int k = walk[i];
    if (k < 0 || k >= nkf) break;                      // uniform: never with a list this file made
    const i64 b = kl_offs[k];
    const int n = (int)(kl_offs[k + 1] - b);
    int r = 0;
    for (int j = threadIdx.x; j < n; j += 256) r += c[list[b + j]] - 1 >= min_obs ? 1 : 0;
    r = block_sum<256>(r, sm);
    if (cull_redundant(r, n, percent)) {               // uniform: every thread holds the same sum
      for (int j = threadIdx.x; j < n; j += 256) c[list[b + j]] -= 1;
      if (threadIdx.x == 0) culled[k] = 1;
      done++;
      if (max_cull > 0 && done >= max_cull) break;
    }
    __syncthreads();                                   // the decrements are visible to the workgroup before the next keyframe's loads
  }
  if (threadIdx.x == 0) *n_culled = done;
}

// keep[i] = 0 iff row i's keyframe is culled (a kf outside [0, nkf) stays); *n_removed += the rows that leave
__global__ __launch_bounds__(256) void k_cull_ob_flag(const int* __restrict__ ob_kf, int nob, int nkf, const int* __restrict__ culled, int* __restrict__ keep,
                                                      int* __restrict__ n_removed) {
  __shared__ int s_w[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool gone = false;
  if (i < nob) {
    const int k = ob_kf[i];
    gone = k >= 0 && k < nkf && culled[k] != 0;
    keep[i] = gone ? 0 : 1;
  }
  const int t = block_count256(gone, s_w);
  if (threadIdx.x == 0 && t) atomicAdd(n_removed, t);
}
// a wavefront per landmark over ALL its views (view_kf is -1 where the row's kf is no keyframe): removed[s] = the views of culled keyframes,
// keep[s] = 0 iff orphans are dropped and every one of its rows leaves (it had at least one); *n_removed += the landmarks that leave
__global__ __launch_bounds__(256) void k_cull_lm_flag(int nlm, const i64* __restrict__ offs, const int* __restrict__ view_kf, const int* __restrict__ culled, int drop_orphans,
                                                      int* __restrict__ removed, int* __restrict__ keep, int* __restrict__ n_removed) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nlm) return;                                // the whole wavefront
  const i64 b = offs[s], e = offs[s + 1];
  i64 rem = 0;
  for (i64 p0 = b; p0 < e; p0 += 64) {
    const i64 p = p0 + lane;
    const int k = p < e ? view_kf[p] : -1;
    rem += __popcll(__ballot(k >= 0 && culled[k] != 0));
  }
  if (lane == 0) {
    const bool orphan = e > b && rem == e - b;
    removed[s] = (int)rem;
    keep[s] = (drop_orphans && orphan) ? 0 : 1;
    if (drop_orphans && orphan) atomicAdd(n_removed, 1);
  }
}
__global__ __launch_bounds__(256) void k_cull_kf_keep(const int* __restrict__ culled, int nkf, int* __restrict__ keep) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < nkf) keep[k] = culled[k] != 0 ? 0 : 1;
}

// a landmark row that stays: observation_count less the removed rows and never below 0
struct CullLmFix {
  const int* removed;
  __device__ void operator()(const LmView& nl, size_t p, const LmView& lm, size_t s) const { nl.cnt[p] = max(lm.cnt[s] - removed[s], 0); }
};
// an observation row that stays: kf through the new-index table (the exclusive scan of the keyframes' keep flags)
struct CullObFix {
  const i64* newidx; int nkf;
  __device__ void operator()(const ObView& no, size_t p, const ObView& ob, size_t i) const {
    const int kf = ob.kf[i];
    if (kf >= 0 && kf < nkf) no.kf[p] = (int)newidx[kf];
  }
};

}  // namespace dvs

using namespace dvs;

namespace {

dvs_status cull_check(const dvs_cull_params& P) {
  DVS_ARG(P.min_observers >= 1);
  DVS_ARG(P.redundancy_percent >= 0 && P.redundancy_percent <= 99);
  DVS_ARG(P.min_weight >= 1);
  DVS_ARG(P.keep_recent >= 0);
  DVS_ARG(P.max_cull >= 0);
  return DVS_OK;
}

}  // namespace

extern "C" {

void dvs_cull_default_params(dvs_cull_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_observers = 3; p->redundancy_percent = 90; p->min_weight = 15; p->local = 0; p->keep_recent = 2; p->max_cull = 0; p->drop_orphans = 1;
}

dvs_status dvs_backend_cull_keyframes(dvs_backend* h, uint64_t ref_frame_id, const dvs_cull_params* params, const uint64_t* protected_frame_ids, int32_t n_protected,
                                      int32_t apply, dvs_cull_result* out, int32_t cap_kf, uint64_t* culled_frame_id, int32_t* kf_observed, int32_t* kf_redundant,
                                      uint8_t* kf_state, int32_t* n_kf) {
  DVS_ARG(h && n_kf && cap_kf >= 0);
  dvs_cull_params P;
  if (params) P = *params; else dvs_cull_default_params(&P);
  dvs_cull_result res;
  memset(&res, 0, sizeof(res));
  if (out) *out = res;
  DVS_TRY(cull_check(P));
  DVS_ARG(n_protected >= 0);
  DVS_ARG(n_protected == 0 || protected_frame_ids);
  const int nkf = (int)h->kfs.size(), nlm = h->nlm, nob = h->nob;
  const bool local = P.local != 0;
  // scope and protection, as far as the host knows them: a candidate is CULL_KEPT
  std::vector<uint8_t> state((size_t)nkf, local ? CULL_OUT : CULL_KEPT);
  std::vector<uint8_t> prot((size_t)nkf, 0);
  for (int j = 0; j < n_protected; j++) {
    const auto it = h->kf_index.find(protected_frame_ids[j]);
    if (it == h->kf_index.end()) { set_error("dvs_backend_cull_keyframes: the map does not hold protected frame %llu", (unsigned long long)protected_frame_ids[j]); return DVS_ERR_ARG; }
    prot[(size_t)it->second] = 1;
  }
  int r = -1;
  if (local) {
    const auto it = h->kf_index.find(ref_frame_id);
    if (it == h->kf_index.end()) { set_error("dvs_backend_cull_keyframes: the map does not hold frame %llu", (unsigned long long)ref_frame_id); return DVS_ERR_ARG; }
    r = it->second;
    prot[(size_t)r] = 1;
    DVS_TRY(covis_limit(h, "dvs_backend_cull_keyframes"));
  }
  *n_kf = nkf;
  res.n_keyframes = nkf;
  if (out) *out = res;
  if ((culled_frame_id || kf_observed || kf_redundant || kf_state) && nkf > cap_kf) {
    set_error("dvs_backend_cull_keyframes: %d keyframes, capacity %d", nkf, cap_kf);
    return DVS_ERR_CAPACITY;
  }
  if (nkf == 0) return DVS_OK;
  prot[0] = 1;
  for (int k = (int)std::max<i64>(0, (i64)nkf - (i64)P.keep_recent); k < nkf; k++) prot[(size_t)k] = 1;

  std::vector<int> n_obs((size_t)nkf, 0), r0((size_t)nkf, 0), culled((size_t)nkf, 0);
  hipStream_t st = nullptr;
  BackendSmall* sm = h->s_small.get();
  if (nlm > 0) {
    DVS_HIP(hipSetDevice(h->device));
    st = h->ctx->stream;
    DVS_TRY(covis_grow(h, local ? 1 : 0));
    DVS_TRY(compact_grow(h)); DVS_TRY(h->blk.grow((size_t)nkf / 256 + 2));
    DVS_TRY(h->cull_kf.grow((size_t)nkf)); DVS_TRY(h->cull_lm.grow((size_t)nlm));
    DVS_TRY(covis_prepare(h));
    if (local) {                                       // N(ref; min_weight), the whole list
      DVS_TRY(covis_rows(h, r, 1, P.min_weight));
      int cnt = 0;
      DVS_TRY(copy_out(&cnt, h->cv_kf.nbc, 1, st));
      DVS_HIP(hipStreamSynchronize(st));
      if (cnt < 0 || cnt > nkf) { set_error("dvs_backend_cull_keyframes: inconsistent neighbour count %d", cnt); return DVS_ERR_HIP; }
      std::vector<int> nb((size_t)std::max(cnt, 1));
      if (cnt) { DVS_TRY(copy_out(nb.data(), h->cv_w.nbi, (size_t)cnt, st)); DVS_HIP(hipStreamSynchronize(st)); }
      for (int j = 0; j < cnt; j++) {
        if (nb[(size_t)j] < 0 || nb[(size_t)j] >= nkf) { set_error("dvs_backend_cull_keyframes: inconsistent neighbour index %d", nb[(size_t)j]); return DVS_ERR_HIP; }
        state[(size_t)nb[(size_t)j]] = CULL_KEPT;
      }
    }
  }
  for (int k = 0; k < nkf; k++) if (prot[(size_t)k]) state[(size_t)k] = CULL_PROTECTED;
  for (int k = 0; k < nkf; k++) res.n_candidates += state[(size_t)k] == CULL_KEPT ? 1 : 0;

  if (nlm > 0) {
    // decide
    const i64* voffs = h->v_lm.offs.get();
    const i64* kl_offs = h->cv_kf.offs.get();
    const int* list = h->cv_ob.list.get();
    DVS_TRY(copy_in(h->cull_kf.state, state.data(), (size_t)nkf, st));
    DVS_HIP(hipMemsetAsync(h->cull_kf.culled.get(), 0, (size_t)nkf * 4, st));
    DVS_HIP(hipMemsetAsync(&sm->cull, 0, sizeof(CullCounts), st));
    hipLaunchKernelGGL(k_cull_observers, dim3((nlm + 3) / 4), dim3(256), 0, st, nlm, voffs, (const int*)h->cv_ob.kf.get(), h->cull_lm.c.get());
    hipLaunchKernelGGL(k_cull_initial, dim3(nkf), dim3(256), 0, st, kl_offs, list, (const int*)h->cull_lm.c.get(), P.min_observers, P.redundancy_percent,
                       (const uint8_t*)h->cull_kf.state.get(), h->cull_kf.n_obs.get(), h->cull_kf.r0.get(), h->cull_kf.flag.get());
    DVS_TRY(compact_rows(h, h->cull_kf.flag.get(), nkf, WalkEmit{h->cull_kf.walk.get()}));
    hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(256), 0, st, compact_total(h, nkf), nkf, (const int*)h->cull_kf.walk.get(), kl_offs, list, h->cull_lm.c.get(),
                       P.min_observers, P.redundancy_percent, P.max_cull, h->cull_kf.culled.get(), &sm->cull.n_culled);
    DVS_HIP(hipGetLastError());
    DVS_TRY(copy_out(n_obs.data(), h->cull_kf.n_obs, (size_t)nkf, st)); DVS_TRY(copy_out(r0.data(), h->cull_kf.r0, (size_t)nkf, st));
    DVS_TRY(copy_out(culled.data(), h->cull_kf.culled, (size_t)nkf, st));
    int n_culled = 0;
    DVS_TRY(small_read(h, &sm->cull.n_culled, &n_culled));
    for (int k = 0; k < nkf; k++) {
      if (culled[(size_t)k] == 0) continue;
      if (state[(size_t)k] != CULL_KEPT) { set_error("dvs_backend_cull_keyframes: keyframe %d was culled without being a candidate", k); return DVS_ERR_HIP; }
      state[(size_t)k] = CULL_CULLED; res.n_culled++;
    }
    if (res.n_culled != n_culled) { set_error("dvs_backend_cull_keyframes: inconsistent counts %d %d", res.n_culled, n_culled); return DVS_ERR_HIP; }
  }
  for (int k = 0; k < nkf; k++) {
    const int n = n_obs[(size_t)k];
    res.n_redundant_initial += (n >= 1 && 100ll * (i64)r0[(size_t)k] > (i64)P.redundancy_percent * (i64)n) ? 1 : 0;
  }
  if (res.n_culled) {                                  // what the apply removes, also in a dry run
    if (nob) hipLaunchKernelGGL(k_cull_ob_flag, dim3((nob + 255) / 256), dim3(256), 0, st, (const int*)h->ob.kf.get(), nob, nkf, (const int*)h->cull_kf.culled.get(),
                                h->cmp_ob.keep.get(), &sm->cull.n_ob_removed);
    hipLaunchKernelGGL(k_cull_lm_flag, dim3((nlm + 3) / 4), dim3(256), 0, st, nlm, (const i64*)h->v_lm.offs.get(), (const int*)h->v_ob.kf.get(), (const int*)h->cull_kf.culled.get(),
                       P.drop_orphans != 0 ? 1 : 0, h->cull_lm.removed.get(), h->cmp_lm.keep.get(), &sm->cull.n_lm_removed);
    DVS_HIP(hipGetLastError());
    int cnt[2] = {0, 0};
    DVS_TRY(small_read(h, &sm->cull.n_ob_removed, cnt, 2));
    if (cnt[0] < 0 || cnt[0] > nob || cnt[1] < 0 || cnt[1] > nlm) { set_error("dvs_backend_cull_keyframes: inconsistent counts %d %d", cnt[0], cnt[1]); return DVS_ERR_HIP; }
    res.n_observations_removed = cnt[0]; res.n_landmarks_removed = cnt[1];
  }
  if (apply && res.n_culled) {
    // the keyframes' new indices, then both tables without the rows that leave
    hipLaunchKernelGGL(k_cull_kf_keep, dim3((nkf + 255) / 256), dim3(256), 0, st, (const int*)h->cull_kf.culled.get(), nkf, h->cull_kf.keep.get());
    launch_scan_counts(st, (const int*)h->cull_kf.keep.get(), nkf, h->cull_kf.newidx.get());
    TablesReplaced done;
    DVS_TRY(tables_replace(h, "dvs_backend_cull_keyframes", h->cmp_lm.keep.get(), CullLmFix{h->cull_lm.removed.get()}, (i64)nlm - res.n_landmarks_removed, h->cmp_ob.keep.get(),
                           CullObFix{h->cull_kf.newidx.get(), nkf}, (i64)nob - res.n_observations_removed, nullptr, &done));
  }
  // the report, in the order of the table before the call
  int nc = 0;
  for (int k = 0; k < nkf; k++) {
    if (kf_observed) kf_observed[k] = n_obs[(size_t)k];
    if (kf_redundant) kf_redundant[k] = r0[(size_t)k];
    if (kf_state) kf_state[k] = state[(size_t)k];
    if (state[(size_t)k] == CULL_CULLED) { if (culled_frame_id) culled_frame_id[nc] = h->kfs[(size_t)k].frame_id; nc++; }
  }
  if (out) *out = res;
  if (apply && res.n_culled) {
    // the keyframe list and the poses: the host records, then kf_R / kf_t rewritten from them
    size_t w = 0;
    for (size_t k = 0; k < (size_t)nkf; k++) {
      if (state[k] == CULL_CULLED) continue;
      if (w != k) h->kfs[w] = std::move(h->kfs[k]);
      w++;
    }
    h->kfs.resize(w);
    h->kf_index.clear();
    h->h_dbl.assign(12 * w, 0.0);
    for (size_t k = 0; k < w; k++) {
      h->kf_index[h->kfs[k].frame_id] = (int)k;
      memcpy(&h->h_dbl[9 * k], h->kfs[k].R, 72); memcpy(&h->h_dbl[9 * w + 3 * k], h->kfs[k].t, 24);
    }
    DVS_TRY(copy_in(h->kf_R, h->h_dbl.data(), w, st)); DVS_TRY(copy_in(h->kf_t, h->h_dbl.data() + 9 * w, w, st));
    DVS_HIP(hipStreamSynchronize(st));
  }
  return DVS_OK;
}

}  // extern "C"
