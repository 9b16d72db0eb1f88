// landmark_refresh.hip — a landmark's descriptor re-selected from all its views, and its viewing geometry (include/dvslam_hip.h "Landmark
// refresh"; the rule is stated there in full and restated in tests/landmark_refresh_ref.py).  The gates that read the geometry are in
// map_track.hip's k_mt_search.
//
// Everything is derived from backend.hip's landmark -> views CSR (v_lm.offs, v_ob.rows / .kf / .oid, segments in observation order).
//   k_lr_count         a wavefront per landmark: n, whether the scope keyframe is among its views, the chosen view cleared
//   k_lr_bin           ONE workgroup: the landmarks in scope with n >= 1 into three lists by n (block_ops.h's ordered compaction, so the
//                      lists are in row order), and the counts of the result.  The work per landmark is n * n popcounts of 256 bits with n
//                      2..10 for almost every landmark and several hundred for a few, so each list gets the shape that fits it:
//   k_lr_select_small  n <= 8: eight landmarks per wavefront in segments of eight lanes; lane i holds view i and the eight distances of its row
//   k_lr_select_wave   n <= 64: a wavefront per landmark; lane i holds view i in registers, view j is read from LDS at a wave-uniform address
//   k_lr_select_block  n > 64: a workgroup per landmark; the views go through LDS in tiles of 256 and the lanes stride the rows
//                      The n x n matrix is never stored: med_i, the (n - 1) / 2-th smallest of row i, is found by nine bisection steps over
//                      0..256, each recounting the row's distances <= mid.  The arg-min over (med_i, i) is an integer minimum over a packed
//                      key — shuffles in a segment or wavefront, block_min in a workgroup.  No atomics, no order dependence.
//   k_lr_geometry      a lane per landmark walks its segment sequentially in FP64: the fixed order the rule states; memory-bound
//   k_lr_apply         a lane per landmark: the chosen view's observation id; where the landmark is in scope and has min_views views, the
//                      chosen descriptor compared with the landmark's and (update) written in place; the changed rows counted
#include <string.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "matcher.h"
#include "backend_internal.h"
#include "block_ops.h"

namespace dvs {

struct D256 { unsigned long long w[4]; };
__device__ __forceinline__ D256 lr_load(const uint8_t* __restrict__ p) {   // one descriptor row, 16-byte aligned
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  D256 d;
  d.w[0] = (unsigned long long)a.x | ((unsigned long long)a.y << 32); d.w[1] = (unsigned long long)a.z | ((unsigned long long)a.w << 32);
  d.w[2] = (unsigned long long)b.x | ((unsigned long long)b.y << 32); d.w[3] = (unsigned long long)b.z | ((unsigned long long)b.w << 32);
  return d;
}
__device__ __forceinline__ int lr_ham(const D256& a, const D256& b) {
  return (__popcll(a.w[0] ^ b.w[0]) + __popcll(a.w[1] ^ b.w[1])) + (__popcll(a.w[2] ^ b.w[2]) + __popcll(a.w[3] ^ b.w[3]));
}
constexpr int kLrSteps = 9;   // 257 values halve to one in nine steps: 257, 129, 65, 33, 17, 9, 5, 3, 2, 1
// one bisection step for the smallest v with #(distances <= v) >= k + 1: c is that count at mid = (lo + hi) >> 1
__device__ __forceinline__ void lr_bisect(int& lo, int& hi, int c, int k) {
  if (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c >= k + 1) hi = mid; else lo = mid + 1;
  }
}

__global__ __launch_bounds__(256) void k_lr_count(int nlm, const i64* __restrict__ offs, const int* __restrict__ view_kf, int scope_kf, int* __restrict__ n_views,
                                                  int* __restrict__ scope, int* __restrict__ best, int* __restrict__ med) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nlm) return;                                // the whole wavefront
  const i64 b = offs[s], e = offs[s + 1];
  bool in = scope_kf < 0;
  if (!in) {
    for (i64 p0 = b; p0 < e; p0 += 64) {
      const i64 p = p0 + lane;
      in = in || __ballot(p < e && view_kf[p] == scope_kf) != 0ull;
    }
  }
  if (lane == 0) { n_views[s] = (int)(e - b); scope[s] = in ? 1 : 0; best[s] = -1; med[s] = -1; }
}

struct OpMaxInt { __device__ int operator()(int a, int b) const { return b > a ? b : a; } };

__global__ __launch_bounds__(256) void k_lr_bin(int nlm, const int* __restrict__ n_views, const int* __restrict__ scope, int* __restrict__ list0, int* __restrict__ list1,
                                                int* __restrict__ list2, RefreshCounts* __restrict__ out) {
  __shared__ int s_w[4];
  __shared__ int s_red[256];
  int done[3] = {0, 0, 0}, in_scope = 0, without = 0, mx = 0;
  int* const list[3] = {list0, list1, list2};
  for (int s0 = 0; s0 < nlm; s0 += 256) {
    const int s = s0 + threadIdx.x;
    const bool in = s < nlm && scope[s] != 0;
    const int n = in ? n_views[s] : 0;
    const int bin = !in || n < 1 ? -1 : (n <= 8 ? 0 : (n <= 64 ? 1 : 2));
#pragma unroll
    for (int b = 0; b < 3; b++) {
      int total;
      const int pos = done[b] + block_rank256(bin == b, s_w, total);
      if (bin == b) list[b][pos] = s;
      done[b] += total;
    }
    in_scope += block_count256(in, s_w);
    without += block_count256(in && n == 0, s_w);
    mx = max(mx, n);
  }
  block_reduce<256, 1>(&mx, s_red, OpMaxInt());
  if (threadIdx.x == 0) {
    out->n_bin[0] = done[0]; out->n_bin[1] = done[1]; out->n_bin[2] = done[2];
    out->n_in_scope = in_scope; out->n_without_views = without; out->max_views = mx; out->n_changed = 0; out->pad = 0;
  }
}

// n <= 8.  Segment g of the wavefront takes entry (wavefront * 8 + g) of the list; every lane stays to the end (the shuffles want them all).
__global__ __launch_bounds__(256) void k_lr_select_small(const int* __restrict__ n_list, const int* __restrict__ list, const i64* __restrict__ offs,
                                                         const int* __restrict__ rows, const uint8_t* __restrict__ ob_desc, int* __restrict__ best, int* __restrict__ med) {
  const int lane = threadIdx.x & 63, i = lane & 7, seg0 = lane & ~7;
  const int e = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + (lane >> 3);
  const bool have = e < *n_list;
  const int s = have ? list[e] : 0;
  const i64 b = have ? offs[s] : 0;
  const int n = have ? min((int)(offs[s + 1] - b), 8) : 0;
  D256 mine = {{0ull, 0ull, 0ull, 0ull}};
  if (i < n) mine = lr_load(ob_desc + 32 * (size_t)rows[b + i]);
  int dist[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    D256 o;
#pragma unroll
    for (int k = 0; k < 4; k++) o.w[k] = __shfl(mine.w[k], seg0 + j);
    dist[j] = j < n ? lr_ham(mine, o) : 1 << 20;
  }
  const int kth = (n - 1) / 2;
  int lo = 0, hi = 256;
  for (int it = 0; it < kLrSteps; it++) {
    const int mid = (lo + hi) >> 1;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) c += dist[j] <= mid ? 1 : 0;
    lr_bisect(lo, hi, c, kth);
  }
  int key = i < n ? (lo << 8) | i : 0x7fffffff;
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) key = min(key, __shfl_xor(key, m));
  if (have && i == 0 && n >= 1) { best[s] = (int)b + (key & 255); med[s] = key >> 8; }
}

// 9 <= n <= 64.  Wavefront w of the workgroup takes entry (workgroup * 4 + w); no early return: the barrier wants every thread.
__global__ __launch_bounds__(256) void k_lr_select_wave(const int* __restrict__ n_list, const int* __restrict__ list, const i64* __restrict__ offs,
                                                        const int* __restrict__ rows, const uint8_t* __restrict__ ob_desc, int* __restrict__ best, int* __restrict__ med) {
  __shared__ D256 s_d[4][64];
  const int w = threadIdx.x >> 6, i = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + w;
  const bool have = e < *n_list;
  const int s = have ? list[e] : 0;
  const i64 b = have ? offs[s] : 0;
  const int n = have ? min((int)(offs[s + 1] - b), 64) : 0;   // wave-uniform
  D256 mine = {{0ull, 0ull, 0ull, 0ull}};
  if (i < n) mine = lr_load(ob_desc + 32 * (size_t)rows[b + i]);
  s_d[w][i] = mine;
  __syncthreads();
  const int kth = (n - 1) / 2;
  int lo = 0, hi = 256;
  for (int it = 0; it < kLrSteps; it++) {
    const int mid = (lo + hi) >> 1;
    int c = 0;
#pragma unroll 8                                      // several LDS reads in flight: one wavefront per SIMD has nothing else to hide their latency
    for (int j = 0; j < n; j++) c += lr_ham(mine, s_d[w][j]) <= mid ? 1 : 0;
    lr_bisect(lo, hi, c, kth);
  }
  int key = i < n ? (lo << 8) | i : 0x7fffffff;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) key = min(key, __shfl_xor(key, m));
  if (have && i == 0 && n >= 1) { best[s] = (int)b + (key & 255); med[s] = key >> 8; }
}

// n > 64, no upper limit.  Workgroup e takes entry e.  Rows in chunks of 256 (thread t: row chunk + t), views in tiles of 256 through LDS; with
// one tile (n <= 256) it is loaded once, otherwise once per step and tile.  Every loop bound is workgroup-uniform, so every barrier is reached
// by every thread.
__global__ __launch_bounds__(256) void k_lr_select_block(const int* __restrict__ n_list, const int* __restrict__ list, const i64* __restrict__ offs,
                                                         const int* __restrict__ rows, const uint8_t* __restrict__ ob_desc, int* __restrict__ best, int* __restrict__ med) {
  __shared__ D256 s_t[256];
  __shared__ unsigned long long s_red[256];
  if ((int)blockIdx.x >= *n_list) return;              // the whole workgroup
  const int tid = threadIdx.x;
  const int s = list[blockIdx.x];
  const i64 b = offs[s];
  const int n = (int)(offs[s + 1] - b);
  const bool one_tile = n <= 256;
  const int kth = (n - 1) / 2;
  if (one_tile) {
    if (tid < n) s_t[tid] = lr_load(ob_desc + 32 * (size_t)rows[b + tid]);
    __syncthreads();
  }
  unsigned long long key = ~0ull;
  for (int rc = 0; rc < n; rc += 256) {
    const int i = rc + tid;
    D256 mine = {{0ull, 0ull, 0ull, 0ull}};
    if (i < n) mine = lr_load(ob_desc + 32 * (size_t)rows[b + i]);
    int lo = 0, hi = 256;
    for (int it = 0; it < kLrSteps; it++) {
      const int mid = (lo + hi) >> 1;
      int c = 0;
      for (int tc = 0; tc < n; tc += 256) {
        const int m = min(256, n - tc);
        if (!one_tile) {
          __syncthreads();
          if (tid < m) s_t[tid] = lr_load(ob_desc + 32 * (size_t)rows[b + tc + tid]);
          __syncthreads();
        }
#pragma unroll 8
        for (int j = 0; j < m; j++) c += lr_ham(mine, s_t[j]) <= mid ? 1 : 0;
      }
      lr_bisect(lo, hi, c, kth);
    }
    if (i < n) key = min(key, ((unsigned long long)lo << 32) | (unsigned)i);
  }
  key = block_min<256>(key, s_red);
  if (tid == 0) { best[s] = (int)(b + (i64)(unsigned)key); med[s] = (int)(key >> 32); }
}

__global__ __launch_bounds__(256) void k_lr_geometry(int nlm, const i64* __restrict__ offs, const int* __restrict__ view_kf, const double* __restrict__ kf_t,
                                                     const float* __restrict__ xyz, double* __restrict__ normal, double* __restrict__ range, int* __restrict__ ncnt) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  const double X0 = (double)xyz[3 * (size_t)s], X1 = (double)xyz[3 * (size_t)s + 1], X2 = (double)xyz[3 * (size_t)s + 2];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, dmin = 0.0, dmax = 0.0;
  int m = 0;
  const i64 e = offs[s + 1];
  for (i64 p = offs[s]; p < e; p++) {
    const int k = view_kf[p];
    if (k < 0) continue;
    const double d0 = X0 - kf_t[3 * (size_t)k], d1 = X1 - kf_t[3 * (size_t)k + 1], d2 = X2 - kf_t[3 * (size_t)k + 2];
    const double r = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    if (!(r > 0.0 && r < (double)INFINITY)) continue;
    a0 += d0 / r; a1 += d1 / r; a2 += d2 / r;
    dmin = m == 0 ? r : (r < dmin ? r : dmin);
    dmax = m == 0 ? r : (r > dmax ? r : dmax);
    m++;
  }
  if (m > 0) { a0 = a0 / (double)m; a1 = a1 / (double)m; a2 = a2 / (double)m; }
  normal[3 * (size_t)s] = a0; normal[3 * (size_t)s + 1] = a1; normal[3 * (size_t)s + 2] = a2;
  range[2 * (size_t)s] = dmin; range[2 * (size_t)s + 1] = dmax;
  ncnt[s] = m;
}

__global__ __launch_bounds__(256) void k_lr_apply(int nlm, const int* __restrict__ n_views, const int* __restrict__ scope, const int* __restrict__ best,
                                                  const int* __restrict__ rows, const i64* __restrict__ view_oid, const uint8_t* __restrict__ ob_desc, int min_views,
                                                  int update, uint8_t* lm_desc, i64* __restrict__ oid, int* __restrict__ n_changed) {
  __shared__ int s_w[4];
  const int s = blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (s < nlm) {
    const int p = best[s];
    oid[s] = p >= 0 ? view_oid[p] : -1ll;
    if (p >= 0 && scope[s] != 0 && n_views[s] >= min_views) {
      const D256 a = lr_load(ob_desc + 32 * (size_t)rows[p]), l = lr_load(lm_desc + 32 * (size_t)s);
      changed = a.w[0] != l.w[0] || a.w[1] != l.w[1] || a.w[2] != l.w[2] || a.w[3] != l.w[3];
      if (changed && update) copy32(lm_desc + 32 * (size_t)s, ob_desc + 32 * (size_t)rows[p]);
    }
  }
  const int t = block_count256(changed, s_w);
  if (threadIdx.x == 0 && t) atomicAdd(n_changed, t);
}

}  // namespace dvs

using namespace dvs;

namespace {

// the row group and the views for the tables as they stand; needs at least one landmark
dvs_status lr_prepare(dvs_backend* h) {
  DVS_HIP(hipSetDevice(h->device));
  DVS_TRY(h->lr_lm.grow((size_t)h->nlm));
  return backend_views_build(h);
}

// the chosen view of every landmark in scope (scope_kf < 0: all) into lr_lm.best / .med, the counts into the counter block; enqueued
dvs_status lr_select(dvs_backend* h, int scope_kf) {
  hipStream_t st = h->ctx->stream;
  const int nlm = h->nlm, nob = h->nob;
  RefreshLmRows& G = h->lr_lm;
  RefreshCounts* rc = &h->s_small.get()->refresh;
  const i64* offs = h->v_lm.offs.get();
  const int* rows = h->v_ob.rows.get();
  const uint8_t* od = h->ob.desc.get();
  hipLaunchKernelGGL(k_lr_count, dim3((nlm + 3) / 4), dim3(256), 0, st, nlm, offs, (const int*)h->v_ob.kf.get(), scope_kf, G.n.get(), G.scope.get(), G.best.get(), G.med.get());
  hipLaunchKernelGGL(k_lr_bin, dim3(1), dim3(256), 0, st, nlm, (const int*)G.n.get(), (const int*)G.scope.get(), G.list0.get(), G.list1.get(), G.list2.get(), rc);
  // the lists' lengths stay on the device: each grid covers the most its list can hold (a landmark of the second list has 9 views at least,
  // one of the third 65), and what lies behind the list's end does nothing
  const int cap0 = nlm, cap1 = std::min(nlm, nob / 9), cap2 = std::min(nlm, nob / 65);
  hipLaunchKernelGGL(k_lr_select_small, dim3((cap0 + 31) / 32), dim3(256), 0, st, (const int*)&rc->n_bin[0], (const int*)G.list0.get(), offs, rows, od, G.best.get(), G.med.get());
  if (cap1) hipLaunchKernelGGL(k_lr_select_wave, dim3((cap1 + 3) / 4), dim3(256), 0, st, (const int*)&rc->n_bin[1], (const int*)G.list1.get(), offs, rows, od, G.best.get(), G.med.get());
  if (cap2) hipLaunchKernelGGL(k_lr_select_block, dim3(cap2), dim3(256), 0, st, (const int*)&rc->n_bin[2], (const int*)G.list2.get(), offs, rows, od, G.best.get(), G.med.get());
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status lr_apply(dvs_backend* h, int min_views, int update) {
  RefreshLmRows& G = h->lr_lm;
  hipLaunchKernelGGL(k_lr_apply, dim3((h->nlm + 255) / 256), dim3(256), 0, h->ctx->stream, h->nlm, (const int*)G.n.get(), (const int*)G.scope.get(), (const int*)G.best.get(),
                     (const int*)h->v_ob.rows.get(), (const i64*)h->v_ob.oid.get(), (const uint8_t*)h->ob.desc.get(), min_views, update, h->lm.desc.get(), G.oid.get(),
                     &h->s_small.get()->refresh.n_changed);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

void lr_geometry(dvs_backend* h) {
  RefreshLmRows& G = h->lr_lm;
  hipLaunchKernelGGL(k_lr_geometry, dim3((h->nlm + 255) / 256), dim3(256), 0, h->ctx->stream, h->nlm, (const i64*)h->v_lm.offs.get(), (const int*)h->v_ob.kf.get(),
                     (const double*)h->kf_t.get(), (const float*)h->lm.xyz.get(), G.normal.get(), G.range.get(), G.ncnt.get());
}

}  // namespace

dvs_status dvs::refresh_geometry(dvs_backend* h) {
  DVS_TRY(lr_prepare(h));
  lr_geometry(h);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

extern "C" {

void dvs_lm_refresh_default_params(dvs_lm_refresh_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->update_descriptors = 1; p->min_views = 1;
}

dvs_status dvs_backend_refresh_landmarks(dvs_backend* h, const dvs_lm_refresh_params* params, dvs_lm_refresh_result* result) {
  DVS_ARG(h);
  dvs_lm_refresh_params P;
  if (params) P = *params; else dvs_lm_refresh_default_params(&P);
  dvs_lm_refresh_result res;
  memset(&res, 0, sizeof(res));
  if (result) *result = res;
  DVS_ARG(P.min_views >= 1);
  int scope_kf = -1;
  if (P.use_scope) {
    const auto it = h->kf_index.find(P.scope_frame_id);
    if (it == h->kf_index.end()) { set_error("dvs_backend_refresh_landmarks: the map does not hold frame %llu", (unsigned long long)P.scope_frame_id); return DVS_ERR_ARG; }
    scope_kf = it->second;
  }
  if (h->nlm == 0) return DVS_OK;
  DVS_TRY(lr_prepare(h));
  DVS_TRY(lr_select(h, scope_kf));
  DVS_TRY(lr_apply(h, P.min_views, P.update_descriptors != 0 ? 1 : 0));
  RefreshCounts c;
  DVS_TRY(small_read(h, (const int*)&h->s_small.get()->refresh, (int*)&c, (int)(sizeof(c) / sizeof(int))));
  if (c.n_in_scope < 0 || c.n_in_scope > h->nlm || c.n_changed < 0 || c.n_changed > c.n_in_scope || c.n_bin[0] + c.n_bin[1] + c.n_bin[2] + c.n_without_views != c.n_in_scope) {
    set_error("dvs_backend_refresh_landmarks: inconsistent counts %d %d %d", c.n_in_scope, c.n_changed, c.n_without_views);
    return DVS_ERR_HIP;
  }
  res.n_in_scope = c.n_in_scope; res.n_changed = c.n_changed; res.n_without_views = c.n_without_views; res.max_views = c.max_views;
  if (result) *result = res;
  return DVS_OK;
}

dvs_status dvs_backend_get_landmark_geometry(dvs_backend* h, int32_t cap, double* normal, double* range, int32_t* n_counted, uint64_t* best_obs_id,
                                             int32_t* best_median, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->nlm;
  const bool want = normal || range || n_counted || best_obs_id || best_median;
  if (want && h->nlm > cap) { set_error("dvs_backend_get_landmark_geometry: %d landmarks, capacity %d", h->nlm, cap); return DVS_ERR_CAPACITY; }
  if (!want || h->nlm == 0) return DVS_OK;
  const size_t nlm = (size_t)h->nlm;
  hipStream_t st = h->ctx->stream;
  DVS_TRY(lr_prepare(h));
  if (best_obs_id || best_median) {
    DVS_TRY(lr_select(h, -1));
    DVS_TRY(lr_apply(h, 1, 0));
  }
  if (normal || range || n_counted) lr_geometry(h);
  DVS_HIP(hipGetLastError());
  DVS_TRY(copy_out(normal, h->lr_lm.normal, nlm, st)); DVS_TRY(copy_out(range, h->lr_lm.range, nlm, st)); DVS_TRY(copy_out(n_counted, h->lr_lm.ncnt, nlm, st));
  DVS_TRY(copy_out(best_obs_id, h->lr_lm.oid, nlm, st)); DVS_TRY(copy_out(best_median, h->lr_lm.med, nlm, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

}  // extern "C"
