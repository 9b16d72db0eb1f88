// match_modes.hip — the rest of cv::BFMatcher(NORM_HAMMING[, crossCheck]) beside match() (boundary B2, include/dvslam_hip.h):
// knnMatch, crossCheck and radiusMatch.  Semantics (OpenCV 4.x batchDistance / radiusMatchImpl, restated, parity unpinned) are
// written out in INTEGRATION.md §B2; in short:
//   knn(k):   per query the first min(k, nt) train rows in ascending (distance, train index); unused slots -1 / INT32_MAX
//   cross:    query i keeps j = argmin_j d(i, .) only if i = argmin_i d(., j) (lowest index on ties on both sides)
//   radius:   every pair with (float)d <= maxDistance, per query in train order, then ordered as std::sort by distance alone orders it
// Kernels:
//   k_match_fp4<NQ, K>  2 <= k <= 4 on the matrix cores (match.hip): the arg-min's operand build and MFMA loop, a top-K epilogue
//   k_knn_hist          any k (and every k under DVS_MATCH_MFMA=0): one wavefront per query, distance histogram + ordered emit
//   k_cross_keep        the mutual-pair filter over two runs of the existing arg-min (q -> t and t -> q)
//   k_radius_sort       per-query std::sort replica (lsort.h) of the pairs k_thresh_count / k_thresh_write found
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "matcher.h"
#include "lsort.h"

namespace dvs {

// =============================================================================================================================
// Any k: one wavefront per query, two passes over the job's train rows (64 consecutive rows per trip, coalesced).
//   pass 1: a 257-bin histogram of the distances in LDS; its prefix sum gives the k-th distance D (kk = min(k, nt)), the count
//           `below` of rows closer than D, and turns each bin d <= D into the first output slot of distance d.
//   pass 2: rows in train order; a row with d <= D goes to slot base[d] + (its rank among the equal-distance rows of the trip) while the
//           slot is < kk, and base[d] advances.  That is exactly the (distance, train index) order of batchDistance's insertion, with no
//           sort; the pass stops as soon as kk slots are written.
// =============================================================================================================================
constexpr int kHistBins = 257;
__global__ __launch_bounds__(256) void k_knn_hist(const u64* __restrict__ q, const int* __restrict__ nqArr, int qStrideRows,
                                                  const u64* __restrict__ t, const int* __restrict__ ntArr, int tStrideRows, int k,
                                                  int* __restrict__ outIdx, int* __restrict__ outDist) {
  __shared__ int hist[4][kHistBins + 7];
  const int pair = blockIdx.y;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int qi = blockIdx.x * 4 + w;
  const int nq = min(max(nqArr[pair], 0), qStrideRows);
  const int nt = min(max(ntArr[pair], 0), tStrideRows);
  if (qi >= nq) return;   // the waves of a workgroup share no data: no workgroup barrier below
  int* hb = hist[w];
  const u64* qp = q + ((size_t)pair * qStrideRows + qi) * 4;
  const u64 a[4] = {qp[0], qp[1], qp[2], qp[3]};
  const u64* tp = t + (size_t)pair * tStrideRows * 4;
  int* oI = outIdx + ((size_t)pair * qStrideRows + qi) * (size_t)k;
  int* oD = outDist + ((size_t)pair * qStrideRows + qi) * (size_t)k;
  const int kk = min(k, nt);
  for (int s = kk + lane; s < k; s += 64) { oI[s] = -1; oD[s] = INT_MAX; }
  if (kk == 0) return;
  auto dist = [&](int j) -> int { return hamming256(a, tp + (size_t)j * 4); };
  for (int i = lane; i < kHistBins; i += 64) hb[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int j = lane; j < nt; j += 64) atomicAdd(&hb[dist(j)], 1);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // lane l owns bins [4l, 4l + 4), lane 63 also bin 256
  const int nb = lane == 63 ? 5 : 4;
  int c[5], own = 0;
#pragma unroll
  for (int b = 0; b < 5; b++) { c[b] = b < nb ? hb[4 * lane + b] : 0; own += c[b]; }
  int incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  int run = incl - own, myD = -1;
#pragma unroll
  for (int b = 0; b < 5; b++) {
    if (b < nb) {
      if (myD < 0 && run < kk && run + c[b] >= kk) myD = 4 * lane + b;
      hb[4 * lane + b] = run;   // first slot of distance 4 lane + b
      run += c[b];
    }
  }
  const u64 found = __ballot(myD >= 0);
  const int src = __ffsll((long long)found) - 1;
  const int D = __shfl(myD, src);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  int written = 0;
  for (int j0 = 0; j0 < nt && written < kk; j0 += 64) {
    const int j = j0 + lane;
    const int d = j < nt ? dist(j) : INT_MAX;
    bool pending = d <= D;
    u64 pb = __ballot(pending);
    while (pb) {   // one round per distinct distance <= D among this trip's rows
      const int leader = __ffsll((long long)pb) - 1;
      const int dl = __shfl(d, leader);
      const bool mine = pending && d == dl;
      const u64 same = __ballot(mine);
      const int base = hb[dl];
      if (mine) {
        const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        if (slot < kk) { oI[slot] = j; oD[slot] = d; }
        pending = false;
      }
      const int n = __popcll(same);
      written += min(n, max(kk - base, 0));
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) hb[dl] = base + n;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      pb &= ~same;
    }
  }
}

// crossCheck: keep query i's arg-min j only if the reverse arg-min of j is i; otherwise -1 / INT_MAX
__global__ __launch_bounds__(256) void k_cross_keep(const int* __restrict__ nqArr, int qStrideRows, const int* __restrict__ rIdx, int tStrideRows,
                                                    int* __restrict__ idx, int* __restrict__ dist) {
  const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int nq = min(max(nqArr[pair], 0), qStrideRows);
  if (i >= nq) return;
  const size_t o = (size_t)pair * qStrideRows + i;
  const int j = idx[o];
  if (j < 0 || j >= tStrideRows || rIdx[(size_t)pair * tStrideRows + j] != i) { idx[o] = -1; dist[o] = INT_MAX; }
}

// radiusMatch order: the (q, t, d) triplets of query i (offs[i] .. offs[i + 1], train ascending, k_thresh_write) as keys d << 32 | t,
// sorted the way std::sort(DMatch::operator<) sorts them (lsort::sort with Less<32>: only the distance is compared, and the exact
// permutation of equal distances is std::sort's), written out as (train, dist) pairs.  One lane per query.
__global__ __launch_bounds__(256) void k_radius_sort(const long long* __restrict__ offs, const int* __restrict__ trip, int nq,
                                                     u64* __restrict__ keys, int* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  const long long b = offs[i], n = offs[i + 1] - b;
  u64* kp = keys + b;
  for (long long p = 0; p < n; p++) kp[p] = ((u64)(uint32_t)trip[3 * (b + p) + 2] << 32) | (uint32_t)trip[3 * (b + p) + 1];
  lsort::sort(kp, (long)n, lsort::Less<32>());
  for (long long p = 0; p < n; p++) { out[2 * (b + p)] = (int)(uint32_t)kp[p]; out[2 * (b + p) + 1] = (int)(kp[p] >> 32); }
}

}  // namespace dvs

using namespace dvs;

extern "C" {

dvs_status dvs_match_hamming_knn_batch_device(dvs_matcher* m, const uint8_t* d_q, const int32_t* d_nq, int32_t q_stride_rows,
                                              const uint8_t* d_t, const int32_t* d_nt, int32_t t_stride_rows, int32_t npairs, int32_t k,
                                              int32_t* d_idx, int32_t* d_dist) {
  DVS_ARG(m && k >= 1);
  DVS_ARG(d_q && d_t && d_nq && d_nt && d_idx && d_dist && npairs >= 0 && q_stride_rows > 0 && t_stride_rows >= 0);
  DVS_ARG(t_stride_rows < (1 << 23));
  if (npairs == 0) return DVS_OK;
  if (k == 1) return dvs_match_hamming_batch_device(m, d_q, d_nq, q_stride_rows, d_t, d_nt, t_stride_rows, npairs, d_idx, d_dist);
  DVS_HIP(hipSetDevice(m->device));
  if (m->use_mfma && k <= 4 && t_stride_rows > 0 && (((uintptr_t)d_q | (uintptr_t)d_t) & 15) == 0)
    launch_match_fp4(m->stream, k, npairs, d_q, d_nq, q_stride_rows, d_t, d_nt, t_stride_rows, nullptr, nullptr, d_idx, d_dist);
  else
    hipLaunchKernelGGL(k_knn_hist, dim3((q_stride_rows + 3) / 4, npairs), dim3(256), 0, m->stream, (const u64*)d_q, d_nq, q_stride_rows, (const u64*)d_t,
                       d_nt, t_stride_rows, k, d_idx, d_dist);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status dvs_match_hamming_cross_batch_device(dvs_matcher* m, const uint8_t* d_q, const int32_t* d_nq, int32_t q_stride_rows,
                                                const uint8_t* d_t, const int32_t* d_nt, int32_t t_stride_rows, int32_t npairs,
                                                int32_t* d_idx, int32_t* d_dist) {
  DVS_ARG(m && d_q && d_t && d_nq && d_nt && d_idx && d_dist && npairs >= 0 && q_stride_rows > 0 && t_stride_rows >= 0);
  DVS_ARG(t_stride_rows < (1 << 23) && q_stride_rows < (1 << 23));   // both directions pack the train index into 23 bits
  if (npairs == 0) return DVS_OK;
  DVS_TRY(dvs_match_hamming_batch_device(m, d_q, d_nq, q_stride_rows, d_t, d_nt, t_stride_rows, npairs, d_idx, d_dist));
  if (t_stride_rows == 0) return DVS_OK;   // no train rows anywhere: every query already has -1 / INT32_MAX
  int* r = nullptr;   // the reverse arg-min (train -> query), idx then dist
  DVS_TRY(matcher_scratch(m, 3, (size_t)npairs * t_stride_rows * 8, (void**)&r));
  DVS_TRY(dvs_match_hamming_batch_device(m, d_t, d_nt, t_stride_rows, d_q, d_nq, q_stride_rows, npairs, r, r + (size_t)npairs * t_stride_rows));
  hipLaunchKernelGGL(k_cross_keep, dim3((q_stride_rows + 255) / 256, npairs), dim3(256), 0, m->stream, d_nq, q_stride_rows, (const int*)r,
                     t_stride_rows, d_idx, d_dist);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

}  // extern "C"

namespace {
// host entry points: q / t staged in scratch slots 0 / 1, the two counts and the outputs in slot 2, one job on the device entry point
template <class F>
dvs_status run_host_job(dvs_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, int width, int32_t* idx, int32_t* dist, F&& device_call) {
  DVS_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  uint8_t *dq = nullptr, *dt = nullptr, *dio = nullptr;
  const size_t nout = (size_t)nq * width;
  DVS_TRY(matcher_scratch(m, 0, (size_t)nq * 32, (void**)&dq));
  DVS_TRY(matcher_scratch(m, 1, (size_t)std::max(nt, 1) * 32, (void**)&dt));
  DVS_TRY(matcher_scratch(m, 2, 64 + nout * 8, (void**)&dio));
  const int32_t counts[2] = {nq, nt};
  int32_t* dn = (int32_t*)dio;
  int32_t* didx = (int32_t*)(dio + 64);
  int32_t* ddist = didx + nout;
  DVS_HIP(hipMemcpyAsync(dq, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
  if (nt) DVS_HIP(hipMemcpyAsync(dt, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
  DVS_HIP(hipMemcpyAsync(dn, counts, 8, hipMemcpyHostToDevice, st));
  DVS_TRY(device_call(dq, dn, dt, dn + 1, didx, ddist));
  DVS_HIP(hipMemcpyAsync(idx, didx, nout * 4, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipMemcpyAsync(dist, ddist, nout * 4, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));   // (also keeps `counts` alive until its copy has run)
  return DVS_OK;
}
}  // namespace

extern "C" {

dvs_status dvs_match_hamming_knn(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k, int32_t* train_idx,
                                 int32_t* dist) {
  DVS_ARG(m && k >= 1 && nq >= 0 && nt >= 0);
  if (nq == 0) return DVS_OK;
  DVS_ARG(q && train_idx && dist && (t || nt == 0));
  DVS_ARG(nt < (1 << 23));
  if (k == 1) return dvs_match_hamming(m, q, nq, t, nt, train_idx, dist);   // the same kernels as match(): bit for bit
  if (nt == 0) {
    for (size_t i = 0; i < (size_t)nq * k; i++) { train_idx[i] = -1; dist[i] = INT_MAX; }
    return DVS_OK;
  }
  return run_host_job(m, q, nq, t, nt, k, train_idx, dist, [&](const uint8_t* dq, const int32_t* dnq, const uint8_t* dt, const int32_t* dnt, int32_t* di, int32_t* dd) {
    return dvs_match_hamming_knn_batch_device(m, dq, dnq, nq, dt, dnt, nt, 1, k, di, dd);
  });
}

dvs_status dvs_match_hamming_cross(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t* train_idx, int32_t* dist) {
  DVS_ARG(m && nq >= 0 && nt >= 0);
  if (nq == 0) return DVS_OK;
  DVS_ARG(q && train_idx && dist && (t || nt == 0));
  DVS_ARG(nt < (1 << 23) && nq < (1 << 23));
  if (nt == 0) {
    for (int i = 0; i < nq; i++) { train_idx[i] = -1; dist[i] = INT_MAX; }
    return DVS_OK;
  }
  return run_host_job(m, q, nq, t, nt, 1, train_idx, dist, [&](const uint8_t* dq, const int32_t* dnq, const uint8_t* dt, const int32_t* dnt, int32_t* di, int32_t* dd) {
    return dvs_match_hamming_cross_batch_device(m, dq, dnq, nq, dt, dnt, nt, 1, di, dd);
  });
}

dvs_status dvs_match_hamming_radius(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, float max_distance,
                                    int64_t* offsets, int32_t* pairs, int64_t cap, int64_t* n_total) {
  DVS_ARG(m && n_total && offsets && nq >= 0 && nt >= 0 && cap >= 0);
  *n_total = 0;
  for (int i = 0; i <= nq; i++) offsets[i] = 0;
  // (float)d <= max_distance for an integer d in [0, 256]  <=>  d < floor(max_distance) + 1; negative / NaN: nothing
  if (nq == 0 || nt == 0 || !(max_distance >= 0.f)) return DVS_OK;
  DVS_ARG(q && t && (pairs || cap == 0));
  const int bound = max_distance >= 256.f ? 257 : (int)floorf(max_distance) + 1;
  const long long* d_offs; const int* d_trip; long long total = 0;
  DVS_TRY(matcher_thresh_device(m, q, nq, t, nt, bound, &d_offs, &d_trip, &total));
  hipStream_t st = m->stream;
  DVS_HIP(hipMemcpyAsync(offsets, d_offs, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, st));
  if (total) {
    uint8_t* buf = nullptr;   // keys, then (train, dist) pairs
    DVS_TRY(matcher_scratch(m, 3, (size_t)total * 16, (void**)&buf));
    u64* keys = (u64*)buf;
    int* out = (int*)(buf + (size_t)total * 8);
    hipLaunchKernelGGL(k_radius_sort, dim3((nq + 255) / 256), dim3(256), 0, st, d_offs, d_trip, nq, keys, out);
    DVS_HIP(hipGetLastError());
    const long long nw = std::min<long long>(total, cap);
    if (nw) DVS_HIP(hipMemcpyAsync(pairs, out, (size_t)nw * 8, hipMemcpyDeviceToHost, st));
  }
  DVS_HIP(hipStreamSynchronize(st));
  *n_total = total;
  return DVS_OK;
}

}  // extern "C"
