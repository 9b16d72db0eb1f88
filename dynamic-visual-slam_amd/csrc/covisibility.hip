// covisibility.hip — the covisibility graph of the map the backend keeps on the device, and its two consumers: the local BA window and the
// local map for tracking (include/dvslam_hip.h "Covisibility"; the rule is stated there in full and restated in tests/covisibility_ref.py).
//
// Everything is derived from backend_views_build's landmark -> views CSR (v_lm.offs / v_ob.kf / v_ob.rows, segments in observation order):
//   k_covis_first      per view: the keyframe where the view COUNTS (cv_kf) — its keyframe if no earlier view of the segment has the same
//                      one, else -1 — so a keyframe that names a landmark twice observes it once; histogram of the counting views by keyframe.
//                      The earlier views are searched, not assumed adjacent: nothing here rests on the order of the observation table
//                      beyond what k_views_finish states (a segment is in observation order).
//   k_covis_scatter / k_covis_order   keyframe -> landmarks CSR (cv_offs / cv_list), built as the views CSR is: histogram, match.hip's scan,
//                      scatter, then every segment put into ascending landmark row by rank (the rows of a segment are distinct)
//   k_covis_row        THE HOT PATH.  One workgroup per requested row a: a wavefront takes a landmark of S_a, its lanes take that landmark's
//                      views and add 1 to the view's keyframe in an LDS histogram of 4 bytes per keyframe; the counting views of one landmark
//                      have distinct keyframes, so the bins of one LDS add instruction are distinct (lanes that all hit the bin of a's
//                      nearest neighbour would serialise).  The row leaves with plain coalesced stores: no global atomics, so the matrix
//                      needs no zeroing and no address is shared by the workgroups of the newest keyframes.  Both consumers need ONE row.
//   k_covis_count      the same histogram over U's rows instead of S_a's: f_c = |S_c n U| for every keyframe
//   k_covis_neighbours per row: ordered compaction of the entries that pass theta, then placement by the rank of the 64-bit key
//                      (weight, ~index) — the keys are distinct, so the rank is the position.  The fixed ranking is the same kernel on f.
//   k_covis_lm_flag / CovisLmEmit   U: flags, then the ordered compaction over the whole table (table_compact.h's compact_rows) of the
//                      columns a window or a local map takes
//   k_covis_ob_flag / CovisObEmit   the window's observations: first rows of their (keyframe, landmark) pair, the same compaction
// Host decisions between the launches (who is free, who is fixed) read back one row of weights and one short list each.
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

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void k_covis_first(int nlm, int nkf, const i64* __restrict__ offs, const int* __restrict__ view_kf, int* __restrict__ cv_kf,
                                                     int* __restrict__ cnt) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nlm) return;
  const i64 b = offs[s], e = offs[s + 1];
  for (i64 p = b + lane; p < e; p += 64) {
    const int k = view_kf[p];
    bool first = k >= 0 && k < nkf;
    for (i64 q = b; first && q < p; q++) first = view_kf[q] != k;
    cv_kf[p] = first ? k : -1;
    if (first) atomicAdd(&cnt[k], 1);
  }
}
// any order inside a keyframe's segment (fill starts at zero); k_covis_order fixes it
__global__ __launch_bounds__(256) void k_covis_scatter(int nlm, const i64* __restrict__ offs, const int* __restrict__ cv_kf, const i64* __restrict__ kl_offs,
                                                       int* __restrict__ fill, int* __restrict__ tmp) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nlm) return;
  const i64 b = offs[s], e = offs[s + 1];
  for (i64 p = b + lane; p < e; p += 64) {
    const int k = cv_kf[p];
    if (k >= 0) tmp[kl_offs[k] + atomicAdd(&fill[k], 1)] = s;
  }
}
// one workgroup per keyframe: its landmark rows in ascending order; position = how many rows of the segment are smaller
__global__ __launch_bounds__(256) void k_covis_order(const i64* __restrict__ kl_offs, const int* __restrict__ tmp, int* __restrict__ list) {
  __shared__ int s_t[2048];
  const i64 b = kl_offs[blockIdx.x];
  const int n = (int)(kl_offs[blockIdx.x + 1] - b);
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const int v = i < n ? tmp[b + i] : 0;
    int r = 0;
    for (int j0 = 0; j0 < n; j0 += 2048) {
      const int m = min(2048, n - j0);
      __syncthreads();
      for (int j = threadIdx.x; j < m; j += 256) s_t[j] = tmp[b + j0 + j];
      __syncthreads();
      if (i < n) for (int j = 0; j < m; j++) r += s_t[j] < v ? 1 : 0;
    }
    if (i < n) list[b + r] = v;
  }
}

// histogram over keyframes of the counting views of the landmark rows list[lb, le), into out[0, nkf); hist: nkf ints of LDS
__device__ __forceinline__ void covis_hist(int* hist, int nkf, const int* __restrict__ list, i64 lb, i64 le, const i64* __restrict__ view_offs,
                                           const int* __restrict__ cv_kf, int* __restrict__ out) {
  for (int k = threadIdx.x; k < nkf; k += 256) hist[k] = 0;
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (i64 j = lb + w; j < le; j += 4) {
    const int s = list[j];
    const i64 vb = view_offs[s], ve = view_offs[s + 1];
    for (i64 p = vb + lane; p < ve; p += 64) {
      const int k = cv_kf[p];
      if (k >= 0) atomicAdd(&hist[k], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nkf; k += 256) out[k] = hist[k];
}
// workgroup b: row row0 + b of W into out + b * nkf
__global__ __launch_bounds__(256) void k_covis_row(int nkf, int row0, const i64* __restrict__ kl_offs, const int* __restrict__ list, const i64* __restrict__ view_offs,
                                                   const int* __restrict__ cv_kf, int* __restrict__ out) {
  extern __shared__ int hist[];
  const int a = row0 + blockIdx.x;
  covis_hist(hist, nkf, list, kl_offs[a], kl_offs[a + 1], view_offs, cv_kf, out + (size_t)blockIdx.x * nkf);
}
// one workgroup: f over the first *n_list rows of `list` (U's landmark rows)
__global__ __launch_bounds__(256) void k_covis_count(int nkf, const int* __restrict__ list, const i64* __restrict__ n_list, const i64* __restrict__ view_offs,
                                                     const int* __restrict__ cv_kf, int* __restrict__ out) {
  extern __shared__ int hist[];
  covis_hist(hist, nkf, list, 0, *n_list, view_offs, cv_kf, out);
}

__device__ __forceinline__ u64 covis_key(int w, int k) { return ((u64)(unsigned)w << 32) | (u64)(~(unsigned)k); }
// workgroup b: the entries k of row w + b * nkf with w[k] >= theta, k != self0 + b (self0 < 0: nobody is left out as self) and, if role is
// given, role[k] == 0, ordered by (weight descending, index ascending) into nb_idx / nb_w + b * nkf; nb_cnt[b] of them.  tmp: as large.
__global__ __launch_bounds__(256) void k_covis_neighbours(int nkf, int self0, const int* __restrict__ W, int theta, const int* __restrict__ role, int* __restrict__ tmp,
                                                          int* __restrict__ nb_idx, int* __restrict__ nb_w, int* __restrict__ nb_cnt) {
  __shared__ int s_w[4];
  __shared__ u64 s_key[1024];
  const int a = self0 < 0 ? -1 : self0 + (int)blockIdx.x;
  const size_t base = (size_t)blockIdx.x * nkf;
  const int* w = W + base;
  int* t = tmp + base;
  int n = 0;
  for (int k0 = 0; k0 < nkf; k0 += 256) {
    const int k = k0 + threadIdx.x;
    const bool keep = k < nkf && k != a && w[k] >= theta && (!role || role[k] == 0);
    int total;
    const int pos = n + block_rank256(keep, s_w, total);
    if (keep) t[pos] = k;
    n += total;
  }
  __threadfence_block();
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const int ki = i < n ? t[i] : 0;
    const u64 key = i < n ? covis_key(w[ki], ki) : 0;
    int r = 0;
    for (int j0 = 0; j0 < n; j0 += 1024) {
      const int m = min(1024, n - j0);
      __syncthreads();
      for (int j = threadIdx.x; j < m; j += 256) { const int kj = t[j0 + j]; s_key[j] = covis_key(w[kj], kj); }
      __syncthreads();
      if (i < n) for (int j = 0; j < m; j++) r += s_key[j] > key ? 1 : 0;
    }
    if (i < n) { nb_idx[base + r] = ki; nb_w[base + r] = w[ki]; }
  }
  if (threadIdx.x == 0) nb_cnt[blockIdx.x] = n;
}
__global__ __launch_bounds__(256) void k_covis_pack(int nkf, const i64* __restrict__ nb_offs, const int* __restrict__ nb_idx, const int* __restrict__ nb_w,
                                                    int* __restrict__ out_i, int* __restrict__ out_w) {
  const i64 o = nb_offs[blockIdx.x];
  const int n = (int)(nb_offs[blockIdx.x + 1] - o);
  const size_t base = (size_t)blockIdx.x * nkf;
  for (int i = threadIdx.x; i < n; i += 256) { out_i[o + i] = nb_idx[base + i]; out_w[o + i] = nb_w[base + i]; }
}

// U: the landmark rows a free keyframe (role 1) observes
__global__ __launch_bounds__(256) void k_covis_lm_flag(int nlm, const i64* __restrict__ view_offs, const int* __restrict__ cv_kf, const int* __restrict__ role,
                                                       int* __restrict__ flag) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  int f = 0;
  for (i64 p = view_offs[s]; p < view_offs[s + 1]; p++) {
    const int k = cv_kf[p];
    if (k >= 0 && role[k] == 1) f = 1;
  }
  flag[s] = f;
}
// the compaction for the landmarks: U's columns in ascending id (the table's order), every flagged row's position in U, U's rows
struct CovisLmEmit {
  LmView lm; int want_desc; int* pos; int* uslot; i64* uid; int* ucls; float* uxyz; uint8_t* udesc;
  __device__ void operator()(size_t s, size_t p) const {
    pos[s] = (int)p; uslot[p] = (int)s;
    uid[p] = lm.id[s]; ucls[p] = lm.cls[s];
    uxyz[3 * p] = lm.xyz[3 * s]; uxyz[3 * p + 1] = lm.xyz[3 * s + 1]; uxyz[3 * p + 2] = lm.xyz[3 * s + 2];
    if (want_desc) copy32(udesc + 32 * p, lm.desc + 32 * s);
  }
};
// the window's observation rows (oflag starts at zero): a view of a landmark of U from a keyframe of the window (role != 0) is in if it
// counts — it is the first row of its (keyframe, landmark) pair — and is a left-out row otherwise
__global__ __launch_bounds__(256) void k_covis_ob_flag(int nlm, const i64* __restrict__ view_offs, const int* __restrict__ view_kf, const int* __restrict__ cv_kf,
                                                       const int* __restrict__ v_obs, const int* __restrict__ role, const int* __restrict__ lflag,
                                                       int* __restrict__ oflag, int* __restrict__ n_left) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm || lflag[s] != 1) return;
  for (i64 p = view_offs[s]; p < view_offs[s + 1]; p++) {
    const int k = view_kf[p];
    if (k < 0 || role[k] == 0) continue;
    if (cv_kf[p] >= 0) oflag[v_obs[p]] = 1; else atomicAdd(n_left, 1);
  }
}
struct CovisObEmit {
  ObView ob; const int* ob_slot; const int* lpos; float* opx; i64* olm; int* ocls; i64* oframe; int* olmidx;
  __device__ void operator()(size_t i, size_t p) const {
    opx[2 * p] = ob.px[2 * i]; opx[2 * p + 1] = ob.px[2 * i + 1];
    olm[p] = ob.lm[i]; ocls[p] = ob.cls[i]; oframe[p] = ob.frame[i];
    olmidx[p] = lpos[ob_slot[i]];            // flagged rows have a landmark of U: ob_slot >= 0
  }
};

}  // namespace dvs

using namespace dvs;

namespace {

dvs_status covis_check(const dvs_covis_params& P) {
  DVS_ARG(P.min_weight >= 1);
  DVS_ARG(P.max_neighbours >= 0 && P.max_neighbours <= 62);
  DVS_ARG(P.max_fixed >= 0 && P.max_fixed <= 63);
  DVS_ARG(P.max_neighbours + 1 + P.max_fixed <= 64);
  DVS_ARG(P.ba_max_iterations >= 1);
  return DVS_OK;
}

}  // namespace

// covis_limit, covis_grow, covis_prepare and covis_rows are shared with kf_cull.hip (backend_internal.h)
dvs_status dvs::covis_limit(const dvs_backend* h, const char* who) {
  if (h->kfs.size() > (size_t)DVS_COVIS_MAX_KEYFRAMES) {
    set_error("%s: %zu keyframes, the row kernel's LDS histogram takes %d", who, h->kfs.size(), DVS_COVIS_MAX_KEYFRAMES);
    return DVS_ERR_CAPACITY;
  }
  return DVS_OK;
}

// scratch for nkf keyframes, the tables as they stand and `rows` rows of weights
dvs_status dvs::covis_grow(dvs_backend* h, size_t rows) {
  const size_t nkf = h->kfs.size(), nlm = (size_t)h->nlm, nob = (size_t)h->nob;
  DVS_TRY(h->cv_ob.grow(nob)); DVS_TRY(h->cv_kf.grow(nkf)); DVS_TRY(h->cv_lm.grow(nlm));
  DVS_TRY(h->blk.grow(std::max(nlm, nob) / 256 + 2));
  return h->cv_w.grow(std::max<size_t>(rows * nkf, 1));
}

// the views CSR, the counting views and the keyframe -> landmarks CSR, enqueued; needs at least one landmark and one keyframe
dvs_status dvs::covis_prepare(dvs_backend* h) {
  hipStream_t st = h->ctx->stream;
  const int nkf = (int)h->kfs.size(), nlm = h->nlm;
  DVS_TRY(backend_views_build(h));
  DVS_HIP(hipMemsetAsync(h->cv_kf.cnt.get(), 0, (size_t)nkf * 4, st));
  DVS_HIP(hipMemsetAsync(h->cv_kf.fill.get(), 0, (size_t)nkf * 4, st));
  const i64* voffs = h->v_lm.offs.get();
  hipLaunchKernelGGL(k_covis_first, dim3((nlm + 3) / 4), dim3(256), 0, st, nlm, nkf, voffs, (const int*)h->v_ob.kf.get(), h->cv_ob.kf.get(), h->cv_kf.cnt.get());
  launch_scan_counts(st, (const int*)h->cv_kf.cnt.get(), nkf, h->cv_kf.offs.get());
  hipLaunchKernelGGL(k_covis_scatter, dim3((nlm + 3) / 4), dim3(256), 0, st, nlm, voffs, (const int*)h->cv_ob.kf.get(), (const i64*)h->cv_kf.offs.get(), h->cv_kf.fill.get(),
                     h->cv_ob.tmp.get());
  hipLaunchKernelGGL(k_covis_order, dim3(nkf), dim3(256), 0, st, (const i64*)h->cv_kf.offs.get(), (const int*)h->cv_ob.tmp.get(), h->cv_ob.list.get());
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

// `rows` rows of W from keyframe row0 on into cv_w.w, and their neighbour lists at theta into cv_w.nbi / cv_w.nbw / cv_kf.nbc
dvs_status dvs::covis_rows(dvs_backend* h, int row0, int rows, int theta) {
  hipStream_t st = h->ctx->stream;
  const int nkf = (int)h->kfs.size();
  hipLaunchKernelGGL(k_covis_row, dim3(rows), dim3(256), (size_t)nkf * 4, st, nkf, row0, (const i64*)h->cv_kf.offs.get(), (const int*)h->cv_ob.list.get(),
                     (const i64*)h->v_lm.offs.get(), (const int*)h->cv_ob.kf.get(), h->cv_w.w.get());
  hipLaunchKernelGGL(k_covis_neighbours, dim3(rows), dim3(256), 0, st, nkf, row0, (const int*)h->cv_w.w.get(), theta, (const int*)nullptr, h->cv_w.nbt.get(), h->cv_w.nbi.get(),
                     h->cv_w.nbw.get(), h->cv_kf.nbc.get());
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

namespace {

struct LocalSet {
  std::vector<int> kf;            // the window's keyframes, ascending index (without want_window: the free keyframes)
  std::vector<uint8_t> fixed;
  std::vector<int> weight;        // W[r][k]
  int n_u = 0, n_obs = 0, n_left = 0;
};

// The local set of keyframe r on the device: U's columns in cv_lm.u and cv_lm.desc (descriptors if want_desc); with want_window the fixed keyframes and the
// window's observation columns in cv_ob.o.  Returns synchronised.
dvs_status covis_local(dvs_backend* h, int r, const dvs_covis_params& P, bool want_window, bool want_desc, LocalSet* out) {
  const int nkf = (int)h->kfs.size(), nlm = h->nlm, nob = h->nob;
  *out = LocalSet();
  if (nlm == 0) {                                      // nobody observes anything: r alone, the gauge
    out->kf.push_back(r); out->fixed.push_back(want_window ? 1 : 0); out->weight.push_back(0);
    return DVS_OK;
  }
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_TRY(covis_grow(h, 1));
  DVS_TRY(covis_prepare(h));
  DVS_TRY(covis_rows(h, r, 1, P.min_weight));
  std::vector<int> w((size_t)nkf), nb((size_t)std::max(P.max_neighbours, 1)), role((size_t)nkf, 0);
  int cnt = 0;
  const int take = std::min(P.max_neighbours, nkf);
  DVS_TRY(copy_out(w.data(), h->cv_w.w, (size_t)nkf, st));
  if (take) DVS_TRY(copy_out(nb.data(), h->cv_w.nbi, (size_t)take, st));
  DVS_TRY(copy_out(&cnt, h->cv_kf.nbc, 1, st));
  DVS_HIP(hipStreamSynchronize(st));
  if (cnt < 0 || cnt > nkf) { set_error("covisibility: inconsistent neighbour count %d", cnt); return DVS_ERR_HIP; }
  role[(size_t)r] = 1;
  for (int j = 0; j < std::min(cnt, take); j++) {
    if (nb[(size_t)j] < 0 || nb[(size_t)j] >= nkf) { set_error("covisibility: inconsistent neighbour index %d", nb[(size_t)j]); return DVS_ERR_HIP; }
    role[(size_t)nb[(size_t)j]] = 1;
  }
  // U
  DVS_HIP(hipMemcpyAsync(h->cv_kf.role.get(), role.data(), (size_t)nkf * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_covis_lm_flag, dim3((nlm + 255) / 256), dim3(256), 0, st, nlm, (const i64*)h->v_lm.offs.get(), (const int*)h->cv_ob.kf.get(), (const int*)h->cv_kf.role.get(),
                     h->cv_lm.flag.get());
  i64 nu = 0;
  DVS_TRY(compact_rows(h, h->cv_lm.flag.get(), nlm, CovisLmEmit{h->lm.view(), want_desc ? 1 : 0, h->cv_lm.pos.get(), h->cv_lm.slot.get(), h->cv_lm.u.id.get(), h->cv_lm.u.cls.get(),
                                                                 h->cv_lm.u.xyz.get(), h->cv_lm.desc.get()}, &nu));
  int nfix = 0;
  std::vector<int> fx((size_t)std::max(P.max_fixed, 1));
  const int take_f = want_window ? std::min(P.max_fixed, nkf) : 0;
  if (want_window) {                                   // f over U, ranked among the keyframes that are not free
    hipLaunchKernelGGL(k_covis_count, dim3(1), dim3(256), (size_t)nkf * 4, st, nkf, (const int*)h->cv_lm.slot.get(), compact_total(h, nlm),
                       (const i64*)h->v_lm.offs.get(), (const int*)h->cv_ob.kf.get(), h->cv_kf.f.get());
    hipLaunchKernelGGL(k_covis_neighbours, dim3(1), dim3(256), 0, st, nkf, -1, (const int*)h->cv_kf.f.get(), 1, (const int*)h->cv_kf.role.get(), h->cv_w.nbt.get(), h->cv_w.nbi.get(),
                       h->cv_w.nbw.get(), h->cv_kf.nbc.get());
    DVS_HIP(hipGetLastError());
    if (take_f) DVS_TRY(copy_out(fx.data(), h->cv_w.nbi, (size_t)take_f, st));
    DVS_TRY(copy_out(&nfix, h->cv_kf.nbc, 1, st));
  }
  DVS_HIP(hipStreamSynchronize(st));
  if (nu < 0 || nu > nlm || nfix < 0 || nfix > nkf) { set_error("covisibility: inconsistent counts %lld %d", (long long)nu, nfix); return DVS_ERR_HIP; }
  out->n_u = (int)nu;
  if (want_window) {
    int marked = 0;
    for (int j = 0; j < std::min(nfix, take_f); j++) {
      if (fx[(size_t)j] < 0 || fx[(size_t)j] >= nkf || role[(size_t)fx[(size_t)j]] != 0) { set_error("covisibility: inconsistent fixed keyframe %d", fx[(size_t)j]); return DVS_ERR_HIP; }
      role[(size_t)fx[(size_t)j]] = 2; marked++;
    }
    if (marked == 0)                                   // the gauge: the free keyframe of lowest index
      for (int k = 0; k < nkf; k++) if (role[(size_t)k] == 1) { role[(size_t)k] = 2; break; }
  }
  for (int k = 0; k < nkf; k++)
    if (role[(size_t)k]) { out->kf.push_back(k); out->fixed.push_back(role[(size_t)k] == 2 ? 1 : 0); out->weight.push_back(w[(size_t)k]); }
  if (!want_window || nob == 0) return DVS_OK;
  // the window's observations
  int* d_left = &h->s_small.get()->left_out;
  DVS_HIP(hipMemcpyAsync(h->cv_kf.role.get(), role.data(), (size_t)nkf * sizeof(int), hipMemcpyHostToDevice, st));
  DVS_HIP(hipMemsetAsync(h->cv_ob.flag.get(), 0, (size_t)nob * 4, st));
  DVS_HIP(hipMemsetAsync(d_left, 0, 4, st));
  hipLaunchKernelGGL(k_covis_ob_flag, dim3((nlm + 255) / 256), dim3(256), 0, st, nlm, (const i64*)h->v_lm.offs.get(), (const int*)h->v_ob.kf.get(), (const int*)h->cv_ob.kf.get(),
                     (const int*)h->v_ob.rows.get(), (const int*)h->cv_kf.role.get(), (const int*)h->cv_lm.flag.get(), h->cv_ob.flag.get(), d_left);
  i64 no = 0;
  int left = 0;
  DVS_TRY(compact_rows(h, h->cv_ob.flag.get(), nob, CovisObEmit{h->ob.view(), h->v_ob.slot.get(), h->cv_lm.pos.get(), h->cv_ob.o.px.get(), h->cv_ob.o.lm.get(), h->cv_ob.o.cls.get(),
                                                                 h->cv_ob.o.frame.get(), h->cv_ob.o.lmidx.get()}, &no));
  DVS_TRY(small_read(h, d_left, &left));
  if (no < 0 || no > nob || left < 0 || left > nob) { set_error("covisibility: inconsistent counts %lld %d", (long long)no, left); return DVS_ERR_HIP; }
  out->n_obs = (int)no; out->n_left = left;
  return DVS_OK;
}

struct WindowHost {
  LocalSet S;
  std::vector<float> o_px, l_xyz;
  std::vector<uint64_t> o_lm, o_frame, l_id;
  std::vector<int32_t> o_cls, o_lmidx, l_cls;
};

// the local window's columns on the host
dvs_status covis_window_host(dvs_backend* h, int r, const dvs_covis_params& P, WindowHost* W) {
  DVS_TRY(covis_local(h, r, P, true, false, &W->S));
  const size_t no = (size_t)W->S.n_obs, nl = (size_t)W->S.n_u;
  W->o_px.resize(2 * no); W->o_lm.resize(no); W->o_frame.resize(no); W->o_cls.resize(no); W->o_lmidx.resize(no);
  W->l_xyz.resize(3 * nl); W->l_id.resize(nl); W->l_cls.resize(nl);
  if (no == 0 && nl == 0) return DVS_OK;
  hipStream_t st = h->ctx->stream;
  DVS_TRY(window_copy_out(h->cv_ob.o, no, h->cv_lm.u, nl, W->o_px.data(), W->o_lm.data(), W->o_cls.data(), W->o_frame.data(), W->o_lmidx.data(), W->l_id.data(), W->l_cls.data(),
                          W->l_xyz.data(), st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status covis_ref_index(dvs_backend* h, uint64_t ref_frame_id, const char* who, int* r) {
  const auto it = h->kf_index.find(ref_frame_id);
  if (it == h->kf_index.end()) { set_error("%s: the map does not hold frame %llu", who, (unsigned long long)ref_frame_id); return DVS_ERR_ARG; }
  *r = it->second;
  return DVS_OK;
}

}  // namespace

dvs_status dvs::backend_local_map(dvs_backend* h, uint64_t ref_frame_id, const dvs_covis_params* params, const float** d_xyz, const uint8_t** d_desc,
                                  const i64** d_id, int* n) {
  dvs_covis_params P;
  if (params) P = *params; else dvs_covis_default_params(&P);
  DVS_TRY(covis_check(P));
  int r = 0;
  DVS_TRY(covis_ref_index(h, ref_frame_id, "dvs_backend_track_frame_local", &r));
  DVS_TRY(covis_limit(h, "dvs_backend_track_frame_local"));
  LocalSet S;
  DVS_TRY(covis_local(h, r, P, false, true, &S));
  *d_xyz = h->cv_lm.u.xyz.get(); *d_desc = h->cv_lm.desc.get(); *d_id = h->cv_lm.u.id.get(); *n = S.n_u;
  return DVS_OK;
}

extern "C" {

void dvs_covis_default_params(dvs_covis_params* p) {
  if (!p) return;
  p->min_weight = 15; p->max_neighbours = 10; p->max_fixed = 32; p->ba_max_iterations = 20;
}

dvs_status dvs_backend_covisibility(dvs_backend* h, int32_t min_weight, int32_t cap_kf, int64_t cap_nb, int32_t* weights, int64_t* nb_offsets, int32_t* nb_index,
                                    int32_t* nb_weight, int32_t* n_kf, int64_t* n_nb) {
  DVS_ARG(h && n_kf && n_nb && cap_kf >= 0 && cap_nb >= 0);
  DVS_ARG(min_weight >= 1);
  DVS_TRY(covis_limit(h, "dvs_backend_covisibility"));
  const int nkf = (int)h->kfs.size();
  *n_kf = nkf; *n_nb = 0;
  const bool per_kf = weights || nb_offsets;
  if (nkf == 0 || h->nlm == 0) {                       // no keyframe observes anything
    if (per_kf && nkf > cap_kf) { set_error("dvs_backend_covisibility: %d keyframes, capacity %d", nkf, cap_kf); return DVS_ERR_CAPACITY; }
    if (weights) memset(weights, 0, (size_t)nkf * (size_t)nkf * 4);
    if (nb_offsets) memset(nb_offsets, 0, ((size_t)nkf + 1) * 8);
    return DVS_OK;
  }
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_TRY(covis_grow(h, (size_t)nkf));
  DVS_TRY(covis_prepare(h));
  DVS_TRY(covis_rows(h, 0, nkf, min_weight));
  launch_scan_counts(st, (const int*)h->cv_kf.nbc.get(), nkf, h->cv_kf.nboffs.get());
  hipLaunchKernelGGL(k_covis_pack, dim3(nkf), dim3(256), 0, st, nkf, (const i64*)h->cv_kf.nboffs.get(), (const int*)h->cv_w.nbi.get(), (const int*)h->cv_w.nbw.get(), h->cv_w.pki.get(),
                     h->cv_w.pkw.get());
  DVS_HIP(hipGetLastError());
  i64 total = 0;
  DVS_HIP(hipMemcpyAsync(&total, h->cv_kf.nboffs.get() + nkf, sizeof(i64), hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  if (total < 0 || total > (i64)nkf * nkf) { set_error("dvs_backend_covisibility: inconsistent count %lld", (long long)total); return DVS_ERR_HIP; }
  *n_nb = total;
  if ((per_kf && nkf > cap_kf) || ((nb_index || nb_weight) && total > cap_nb)) {
    set_error("dvs_backend_covisibility: %d keyframes / %lld neighbours, capacities %d / %lld", nkf, (long long)total, cap_kf, (long long)cap_nb);
    return DVS_ERR_CAPACITY;
  }
  DVS_TRY(copy_out(weights, h->cv_w.w, (size_t)nkf * (size_t)nkf, st)); DVS_TRY(copy_out(nb_offsets, h->cv_kf.nboffs, (size_t)nkf + 1, st));
  if (total) { DVS_TRY(copy_out(nb_index, h->cv_w.pki, (size_t)total, st)); DVS_TRY(copy_out(nb_weight, h->cv_w.pkw, (size_t)total, st)); }
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_get_local_window(dvs_backend* h, uint64_t ref_frame_id, const dvs_covis_params* params, int32_t cap_kf, int32_t cap_obs, int32_t cap_lm,
                                        uint64_t* kf_frame_id, double* kf_R, double* kf_t, uint8_t* kf_fixed, int32_t* kf_weight, int32_t* n_kf, float* obs_px,
                                        uint64_t* obs_lm_id, int32_t* obs_class, uint64_t* obs_frame_id, int32_t* obs_lm_index, int32_t* n_obs, uint64_t* lm_id,
                                        int32_t* lm_class, float* lm_xyz, int32_t* n_lm, int32_t* n_left_out) {
  DVS_ARG(h && n_kf && n_obs && n_lm && cap_kf >= 0 && cap_obs >= 0 && cap_lm >= 0);
  dvs_covis_params P;
  if (params) P = *params; else dvs_covis_default_params(&P);
  DVS_TRY(covis_check(P));
  int r = 0;
  DVS_TRY(covis_ref_index(h, ref_frame_id, "dvs_backend_get_local_window", &r));
  DVS_TRY(covis_limit(h, "dvs_backend_get_local_window"));
  *n_kf = *n_obs = *n_lm = 0;
  if (n_left_out) *n_left_out = 0;
  WindowHost W;
  DVS_TRY(covis_window_host(h, r, P, &W));
  const int nk = (int)W.S.kf.size(), no = W.S.n_obs, nl = W.S.n_u;
  *n_kf = nk; *n_obs = no; *n_lm = nl;
  if (n_left_out) *n_left_out = W.S.n_left;
  const bool wk = kf_frame_id || kf_R || kf_t || kf_fixed || kf_weight, wo = obs_px || obs_lm_id || obs_class || obs_frame_id || obs_lm_index,
             wl = lm_id || lm_class || lm_xyz;
  if ((wk && nk > cap_kf) || (wo && no > cap_obs) || (wl && nl > cap_lm)) {
    set_error("dvs_backend_get_local_window: %d keyframes / %d observations / %d landmarks, capacities %d / %d / %d", nk, no, nl, cap_kf, cap_obs, cap_lm);
    return DVS_ERR_CAPACITY;
  }
  for (int k = 0; k < nk; k++) {
    const KeyframeRec& K = h->kfs[(size_t)W.S.kf[(size_t)k]];
    if (kf_frame_id) kf_frame_id[k] = K.frame_id;
    if (kf_R) memcpy(kf_R + 9 * (size_t)k, K.R, 72);
    if (kf_t) memcpy(kf_t + 3 * (size_t)k, K.t, 24);
    if (kf_fixed) kf_fixed[k] = W.S.fixed[(size_t)k];
    if (kf_weight) kf_weight[k] = W.S.weight[(size_t)k];
  }
  if (no) {
    if (obs_px) memcpy(obs_px, W.o_px.data(), (size_t)no * 8);
    if (obs_lm_id) memcpy(obs_lm_id, W.o_lm.data(), (size_t)no * 8);
    if (obs_class) memcpy(obs_class, W.o_cls.data(), (size_t)no * 4);
    if (obs_frame_id) memcpy(obs_frame_id, W.o_frame.data(), (size_t)no * 8);
    if (obs_lm_index) memcpy(obs_lm_index, W.o_lmidx.data(), (size_t)no * 4);
  }
  if (nl) {
    if (lm_id) memcpy(lm_id, W.l_id.data(), (size_t)nl * 8);
    if (lm_class) memcpy(lm_class, W.l_cls.data(), (size_t)nl * 4);
    if (lm_xyz) memcpy(lm_xyz, W.l_xyz.data(), (size_t)nl * 12);
  }
  return DVS_OK;
}

// Local BA ("Covisibility" in the header).  The problem is assembled on the host from the local window's columns, as dvs_backend_global_ba
// assembles its own from the tables; the solve is the caller's dvs_ba handle's.
dvs_status dvs_backend_local_ba(dvs_backend* h, dvs_ba* ba, uint64_t ref_frame_id, const dvs_covis_params* params, dvs_backend_lba_result* out) {
  DVS_ARG(h && ba && out);
  memset(out, 0, sizeof(*out));
  dvs_covis_params P;
  if (params) P = *params; else dvs_covis_default_params(&P);
  DVS_TRY(covis_check(P));
  int r = 0;
  DVS_TRY(covis_ref_index(h, ref_frame_id, "dvs_backend_local_ba", &r));
  DVS_TRY(covis_limit(h, "dvs_backend_local_ba"));
  WindowHost W;
  DVS_TRY(covis_window_host(h, r, P, &W));
  const int K = (int)W.S.kf.size(), no = W.S.n_obs, nu = W.S.n_u;
  // the window's keyframe of every observation, the landmarks that keep two rows, their rows in the problem
  std::vector<int> cam_of_frame_row((size_t)no, -1), cnt((size_t)nu, 0), lrow((size_t)nu, -1);
  for (int i = 0; i < no; i++) {
    const auto it = h->kf_index.find(W.o_frame[(size_t)i]);
    const int k = it == h->kf_index.end() ? -1 : it->second;
    const auto w = std::lower_bound(W.S.kf.begin(), W.S.kf.end(), k);
    const int l = W.o_lmidx[(size_t)i];
    if (k < 0 || w == W.S.kf.end() || *w != k || l < 0 || l >= nu) { set_error("dvs_backend_local_ba: inconsistent window row %d", i); return DVS_ERR_HIP; }
    cam_of_frame_row[(size_t)i] = (int)(w - W.S.kf.begin());
    cnt[(size_t)l]++;
  }
  int L = 0;
  for (int l = 0; l < nu; l++) if (cnt[(size_t)l] >= 2) lrow[(size_t)l] = L++;
  std::vector<int32_t> cam, lmi;
  std::vector<double> uv;
  for (int i = 0; i < no; i++) {
    const int l = W.o_lmidx[(size_t)i];
    if (lrow[(size_t)l] < 0) continue;
    cam.push_back(cam_of_frame_row[(size_t)i]); lmi.push_back(lrow[(size_t)l]);
    uv.push_back((double)W.o_px[2 * (size_t)i]); uv.push_back((double)W.o_px[2 * (size_t)i + 1]);
  }
  const int R = (int)cam.size();
  int nfixed = 0;
  for (uint8_t f : W.S.fixed) nfixed += f ? 1 : 0;
  out->n_cameras = K; out->n_fixed = nfixed; out->n_landmarks = L; out->n_observations = R; out->n_left_out = W.S.n_left; out->n_dropped = no - R;
  if (nfixed == K) { set_error("dvs_backend_local_ba: the window of frame %llu has no keyframe that is not fixed", (unsigned long long)ref_frame_id); return DVS_ERR_ARG; }
  if (R == 0) { set_error("dvs_backend_local_ba: no landmark of the window has two observations"); return DVS_ERR_ARG; }
  std::vector<double> q(4 * (size_t)K), t(3 * (size_t)K), X(3 * (size_t)L);
  for (int k = 0; k < K; k++) {
    const KeyframeRec& F = h->kfs[(size_t)W.S.kf[(size_t)k]];
    DVS_TRY(dvs_ba_pose_from_rt(F.R, F.t, &q[4 * (size_t)k], &t[3 * (size_t)k]));
  }
  for (int l = 0; l < nu; l++)
    if (lrow[(size_t)l] >= 0) for (int c = 0; c < 3; c++) X[3 * (size_t)lrow[(size_t)l] + c] = (double)W.l_xyz[3 * (size_t)l + c];
  DVS_TRY(dvs_ba_set_problem(ba, K, q.data(), t.data(), L, X.data(), R, cam.data(), lmi.data(), uv.data(), W.S.fixed.data(), nullptr, h->P.fx, h->P.fy, h->P.cx, h->P.cy,
                             1.0, 1.345));
  DVS_TRY(dvs_ba_solve_device(ba, P.ba_max_iterations, 1e-6, 1e-10, 1e-8, &out->summary));
  if (out->summary.termination != 0) return DVS_OK;    // the map stays as it was
  DVS_TRY(dvs_ba_get_parameters(ba, q.data(), t.data(), X.data()));
  std::vector<uint64_t> frames; std::vector<double> Rs, ts;
  for (int k = 0; k < K; k++) {
    if (W.S.fixed[(size_t)k]) continue;
    double Rk[9], tk[3];
    DVS_TRY(dvs_ba_pose_to_rt(&q[4 * (size_t)k], &t[3 * (size_t)k], Rk, tk));
    frames.push_back(h->kfs[(size_t)W.S.kf[(size_t)k]].frame_id); Rs.insert(Rs.end(), Rk, Rk + 9); ts.insert(ts.end(), tk, tk + 3);
  }
  std::vector<uint64_t> ids; std::vector<int32_t> cls;
  for (int l = 0; l < nu; l++)
    if (lrow[(size_t)l] >= 0) { ids.push_back(W.l_id[(size_t)l]); cls.push_back(W.l_cls[(size_t)l]); }
  return dvs_backend_apply_optimized(h, (int32_t)frames.size(), frames.data(), Rs.data(), ts.data(), (int32_t)ids.size(), ids.data(), cls.data(), X.data());
}

}  // extern "C"
