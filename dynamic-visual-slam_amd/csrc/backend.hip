// backend.hip — the mapping backend as one handle and one call per keyframe (include/dvslam_hip.h, dvs_backend_*): Backend::syncCallback
// (backend.cpp:709-832), the BA window of bundleAdjustmentCallback (:892-945), updateOptimizedResults (:1356-1392) and pruneLandmarks
// (:1249-1322), with the landmark table, the observation table (all_observations_) and the keyframe poses resident in HBM.
//
// Both tables are kept in ascending id: ids are handed out in increasing order, rows are appended, and pruning compacts in order.  So a
// class's landmarks "in ascending id" are an ordered compaction of the table, a landmark's observation_ids are the observations that name
// it in table order, and id -> row is a binary search.  The kernels this file adds:
//   k_categorize       class id and filtered flag per observation (:746-751, :1011-1029) + the kept observations grouped by class, in order
//   k_class_gather     one class's landmarks in ascending id: row, descriptor, position                                      (:1068)
//   k_views_count / _scatter / _finish   landmark -> views CSR from the observation table (histogram, match.hip's scan, scatter; _finish puts
//                      every landmark's segment back into observation order and fills view_kf / view_px / the observation ids)  (:451-481)
//   k_pair_gather      per association candidate: the landmark's id, row, position, triangulated position and status — what the host walk reads
//   k_match_apply      observation_count, last_seen and the triangulated position of the matched landmarks                  (:766-772)
//   k_append_obs / k_append_lm   the keyframe's observations and new landmarks join the tables                              (:803-820)
//   k_window_gather    the window's observations, the distinct landmarks in id order, indices into that list                (:916-945)
//   k_apply            optimised positions and poses                                                                        (:1356-1392)
//   k_prune_mark / k_prune_ob_flag   the landmarks that leave and the observations that name one; table_compact.h's tables_replace
//                      then writes both tables without them, in order, and lists the removed observations                      (:1249-1322)
// The list builders are one workgroup of four wavefronts walking the table in trips of 256 (block_ops.h), as tracker.hip does it; what
// removes rows from the tables is the three-step compaction of table_compact.h.
//
// Triangulation: LandmarkInfo::triangulate at :772 reads the views stored BEFORE this keyframe and the landmark's position at the start of
// the keyframe only (include/dvslam/triangulation.hpp states why), so it runs once per keyframe over the whole table, before the classes.
// Association is the launch sequence of dvs_associate_candidates on device pointers (associate_device.h), once per class present; the host
// walks each class's observations in order with associateSequential's logic on the candidate read-back, then one pass over all
// observations in message order hands out observation ids and new landmark ids as the interleaved loop would.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "matcher.h"
#include "backend_internal.h"
#include "associate_device.h"
#include "block_ops.h"
#include "table_compact.h"
#include "../../include/dvslam/association.hpp"   // reprojection_error: the device kernel's arithmetic on the host

namespace dvs {

// LmView / ObView, lm_find, copy32, the tables and the handle: backend_internal.h

// categorizeObservation (:1011-1029): the first detection whose box holds the pixel — the float pixel promoted to double against
// c -/+ size / 2 in double, inclusive on all four sides — else class 0.  code[i] = class, or -1 - class when the class is filtered (:749).
// Then, class by class of `classes` (nc distinct unfiltered ids), the kept observations in order: order / q_px / q_desc hold class 0's
// rows, then class 1's, ...; class_cnt[k] rows each.
__global__ __launch_bounds__(256) void k_categorize(const float* __restrict__ px, const uint8_t* __restrict__ desc, int n, const DetRec* __restrict__ det, int ndet,
                                                    const int* __restrict__ filt, int nfilt, const int* __restrict__ classes, int nc, int* __restrict__ code,
                                                    int* __restrict__ order, float* __restrict__ q_px, uint8_t* __restrict__ q_desc, int* __restrict__ class_cnt) {
  __shared__ int s_w[4];
  for (int i = threadIdx.x; i < n; i += 256) {
    const double x = (double)px[2 * i], y = (double)px[2 * i + 1];
    int c = 0;
    for (int d = 0; d < ndet; d++) {
      const DetRec b = det[d];
      if (x >= b.cx - b.w / 2 && x <= b.cx + b.w / 2 && y >= b.cy - b.h / 2 && y <= b.cy + b.h / 2) { c = b.cls; break; }
    }
    bool f = false;
    for (int k = 0; k < nfilt; k++) f = f || filt[k] == c;
    code[i] = f ? -1 - c : c;
  }
  __threadfence_block();
  __syncthreads();
  int done = 0;
  for (int k = 0; k < nc; k++) {
    const int c = classes[k];
    const int first = done;
    for (int i0 = 0; i0 < n; i0 += 256) {
      const int i = i0 + threadIdx.x;
      const bool keep = i < n && code[i] == c;
      int total;
      const int pos = done + block_rank256(keep, s_w, total);
      if (keep) {
        order[pos] = i;
        q_px[2 * pos] = px[2 * i]; q_px[2 * pos + 1] = px[2 * i + 1];
        copy32(q_desc + 32 * (size_t)pos, desc + 32 * (size_t)i);
      }
      done += total;
    }
    if (threadIdx.x == 0) class_cnt[k] = done - first;
  }
}

// landmark_database_[category] in ascending id (:1068): rows of class c, with descriptor and position
__global__ __launch_bounds__(256) void k_class_gather(LmView lm, int nlm, int c, int* __restrict__ g_slot, uint8_t* __restrict__ g_desc, float* __restrict__ g_xyz,
                                                      int* __restrict__ n_out) {
  __shared__ int s_w[4];
  int done = 0;
  for (int s0 = 0; s0 < nlm; s0 += 256) {
    const int s = s0 + threadIdx.x;
    const bool keep = s < nlm && lm.cls[s] == c;
    int total;
    const int pos = done + block_rank256(keep, s_w, total);
    if (keep) {
      g_slot[pos] = s;
      copy32(g_desc + 32 * (size_t)pos, lm.desc + 32 * (size_t)s);
      g_xyz[3 * pos] = lm.xyz[3 * s]; g_xyz[3 * pos + 1] = lm.xyz[3 * s + 1]; g_xyz[3 * pos + 2] = lm.xyz[3 * s + 2];
    }
    done += total;
  }
  if (threadIdx.x == 0) *n_out = done;
}

// views CSR, step 1: every observation's landmark row (ob_slot, -1 if the landmark is gone) and the histogram by landmark
__global__ __launch_bounds__(256) void k_views_count(ObView ob, int nob, const i64* __restrict__ lm_id, int nlm, int* __restrict__ ob_slot, int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nob) return;
  const int s = lm_find(lm_id, nlm, ob.lm[i]);
  ob_slot[i] = s;
  if (s >= 0) atomicAdd(&cnt[s], 1);
}
// step 2: exclusive scan of the histogram into 64-bit offsets: match.hip's k_scan_counts (launch_scan_counts)
// step 3: scatter the observation rows into their landmark's segment (any order inside it; fill starts at zero)
__global__ __launch_bounds__(256) void k_views_scatter(const int* __restrict__ ob_slot, int nob, const i64* __restrict__ offs, int* __restrict__ fill,
                                                       int* __restrict__ v_obs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nob) return;
  const int s = ob_slot[i];
  if (s >= 0) v_obs[offs[s] + atomicAdd(&fill[s], 1)] = i;
}
// step 4: one thread per landmark puts its segment into observation order (= observation_ids order, :451) and writes the views: the
// keyframe's index (-1 where the reference's find_if over keyframes_ would fail), the pixel, the observation id
__global__ __launch_bounds__(256) void k_views_finish(ObView ob, int nkf, int nlm, const i64* __restrict__ offs, int* __restrict__ v_obs, int* __restrict__ view_kf,
                                                      float* __restrict__ view_px, i64* __restrict__ view_oid) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  const i64 b = offs[s], e = offs[s + 1];
  for (i64 p = b + 1; p < e; p++) {
    const int v = v_obs[p];
    i64 q = p;
    while (q > b && v_obs[q - 1] > v) { v_obs[q] = v_obs[q - 1]; q--; }
    v_obs[q] = v;
  }
  for (i64 p = b; p < e; p++) {
    const int i = v_obs[p];
    const int k = ob.kf[i];
    view_kf[p] = (k >= 0 && k < nkf) ? k : -1;
    view_px[2 * p] = ob.px[2 * i]; view_px[2 * p + 1] = ob.px[2 * i + 1];
    view_oid[p] = ob.id[i];
  }
}

// what the host walk reads per candidate pair (class-local landmark j = pairs3[3 p + 1])
__global__ __launch_bounds__(256) void k_pair_gather(const int* __restrict__ pairs3, i64 npairs, const int* __restrict__ g_slot, const i64* __restrict__ lm_id,
                                                     const float* __restrict__ lm_xyz, const float* __restrict__ tri_xyz, const int* __restrict__ tri_status,
                                                     PairRec* __restrict__ rec) {
  const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
  if (p >= npairs) return;
  const int j = pairs3[3 * p + 1], s = g_slot[j];
  PairRec r;
  r.id = lm_id[s]; r.j = j; r.slot = s; r.status = tri_status[s]; r.pad = 0;
  for (int k = 0; k < 3; k++) { r.xyz[k] = lm_xyz[3 * (size_t)s + k]; r.tri[k] = tri_xyz[3 * (size_t)s + k]; }
  rec[p] = r;
}

// :766-772 for the m distinct matched landmarks: observation_count += matches, last_seen = the keyframe's stamp, position = the
// triangulated one where triangulate() accepted it
__global__ __launch_bounds__(256) void k_match_apply(int m, const int* __restrict__ slot, const int* __restrict__ inc, const int* __restrict__ moved, i64 stamp,
                                                     const float* __restrict__ tri_xyz, LmView lm, int nlm) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  const int s = slot[e];
  if (s < 0 || s >= nlm) return;
  lm.cnt[s] += inc[e];
  lm.seen[s] = stamp;
  if (moved[e]) for (int k = 0; k < 3; k++) lm.xyz[3 * (size_t)s + k] = tri_xyz[3 * (size_t)s + k];
}

// :809: the kept observations, in message order, at rows base ..; ids first_id ..
__global__ __launch_bounds__(256) void k_append_obs(int m, const int* __restrict__ src, const i64* __restrict__ lm_of, i64 first_id, i64 frame, int kf,
                                                    const float* __restrict__ px, const uint8_t* __restrict__ desc, const int* __restrict__ code, int n_src, ObView ob,
                                                    int base) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  const int i = src[e];
  if (i < 0 || i >= n_src) return;
  const size_t r = (size_t)base + e;
  ob.id[r] = first_id + e; ob.frame[r] = frame; ob.lm[r] = lm_of[e]; ob.kf[r] = kf; ob.cls[r] = code[i];
  ob.px[2 * r] = px[2 * i]; ob.px[2 * r + 1] = px[2 * i + 1];
  copy32(ob.desc + 32 * r, desc + 32 * (size_t)i);
}
// :786-791, :812-815: new landmarks with observation_count 1 and last_seen = the stamp (:397)
__global__ __launch_bounds__(256) void k_append_lm(int m, const int* __restrict__ src, i64 first_id, i64 stamp, const float* __restrict__ xyz,
                                                   const uint8_t* __restrict__ desc, const int* __restrict__ code, int n_src, LmView lm, int base) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  const int i = src[e];
  if (i < 0 || i >= n_src) return;
  const size_t r = (size_t)base + e;
  lm.id[r] = first_id + e; lm.seen[r] = stamp; lm.cls[r] = code[i]; lm.cnt[r] = 1;
  for (int k = 0; k < 3; k++) lm.xyz[3 * r + k] = xyz[3 * (size_t)i + k];
  copy32(lm.desc + 32 * r, desc + 32 * (size_t)i);
}

// :916-945.  The observations of keyframes kf_start .. (all_observations_ order), the distinct landmarks they name in ascending id, and
// each observation's row in that list.  flag / pos: nlm ints of scratch; w_oi / w_slot: nob ints of scratch.  counts: {observations, landmarks}.
__global__ __launch_bounds__(256) void k_window_gather(ObView ob, int nob, LmView lm, int nlm, int kf_start, int* __restrict__ flag, int* __restrict__ pos,
                                                       int* __restrict__ w_oi, int* __restrict__ w_slot, float* __restrict__ o_px, i64* __restrict__ o_lm,
                                                       int* __restrict__ o_cls, i64* __restrict__ o_frame, int* __restrict__ o_lmidx, i64* __restrict__ l_id,
                                                       int* __restrict__ l_cls, float* __restrict__ l_xyz, int* __restrict__ counts) {
  __shared__ int s_w[4];
  for (int s = threadIdx.x; s < nlm; s += 256) flag[s] = 0;
  __threadfence_block();
  __syncthreads();
  int nw = 0;
  for (int i0 = 0; i0 < nob; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool keep = i < nob && ob.kf[i] >= kf_start;
    int total;
    const int p = nw + block_rank256(keep, s_w, total);
    if (keep) {
      const int s = lm_find(lm.id, nlm, ob.lm[i]);
      w_oi[p] = i; w_slot[p] = s;
      if (s >= 0) flag[s] = 1;
    }
    nw += total;
  }
  __threadfence_block();
  __syncthreads();
  int nl = 0;
  for (int s0 = 0; s0 < nlm; s0 += 256) {
    const int s = s0 + threadIdx.x;
    const bool keep = s < nlm && flag[s] != 0;
    int total;
    const int p = nl + block_rank256(keep, s_w, total);
    if (keep) {
      pos[s] = p;
      l_id[p] = lm.id[s]; l_cls[p] = lm.cls[s];
      l_xyz[3 * p] = lm.xyz[3 * s]; l_xyz[3 * p + 1] = lm.xyz[3 * s + 1]; l_xyz[3 * p + 2] = lm.xyz[3 * s + 2];
    }
    nl += total;
  }
  __threadfence_block();
  __syncthreads();
  for (int e = threadIdx.x; e < nw; e += 256) {
    const int i = w_oi[e], s = w_slot[e];
    o_px[2 * e] = ob.px[2 * i]; o_px[2 * e + 1] = ob.px[2 * i + 1];
    o_lm[e] = ob.lm[i]; o_cls[e] = ob.cls[i]; o_frame[e] = ob.frame[i];
    o_lmidx[e] = s >= 0 ? pos[s] : -1;
  }
  if (threadIdx.x == 0) { counts[0] = nw; counts[1] = nl; }
}

// updateOptimizedResults: landmark positions by (id, class), stored as float (:1382-1384); poses by keyframe index (12 doubles: R, t)
__global__ __launch_bounds__(256) void k_apply(int nl, const i64* __restrict__ ids, const int* __restrict__ cls, const double* __restrict__ xyz, LmView lm, int nlm,
                                               int np, const int* __restrict__ kf_idx, const double* __restrict__ Rt, double* __restrict__ kf_R, double* __restrict__ kf_t,
                                               int nkf) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < nl) {
    const int s = lm_find(lm.id, nlm, ids[e]);
    if (s >= 0 && lm.cls[s] == cls[e])
      for (int k = 0; k < 3; k++) lm.xyz[3 * (size_t)s + k] = (float)xyz[3 * (size_t)e + k];
  }
  if (e < np) {
    const int k = kf_idx[e];
    if (k >= 0 && k < nkf) {
      for (int c = 0; c < 9; c++) kf_R[9 * (size_t)k + c] = Rt[12 * (size_t)e + c];
      for (int c = 0; c < 3; c++) kf_t[3 * (size_t)k + c] = Rt[12 * (size_t)e + 9 + c];
    }
  }
}

// :1258-1273: observation_count < min_obs AND (double)(now - last_seen) / 1e9 > max_age
__global__ __launch_bounds__(256) void k_prune_mark(LmView lm, int nlm, i64 now, int min_obs, double max_age, int* __restrict__ keep, int* __restrict__ gone,
                                                    int* __restrict__ n_marked) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  const double age = (double)(now - lm.seen[s]) / 1e9;
  const int f = (lm.cnt[s] < min_obs && age > max_age) ? 1 : 0;
  keep[s] = 1 - f; gone[s] = f;
  if (f) atomicAdd(n_marked, 1);
}
// :1279-1312: an observation leaves iff it names a marked landmark
__global__ __launch_bounds__(256) void k_prune_ob_flag(const i64* __restrict__ lm_id, int nlm, const int* __restrict__ lm_gone, const i64* __restrict__ ob_lm, int nob,
                                                       int* __restrict__ keep, int* __restrict__ gone) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nob) return;
  const int s = lm_find(lm_id, nlm, ob_lm[i]);
  const int g = (s >= 0 && lm_gone[s] != 0) ? 1 : 0;
  keep[i] = 1 - g; gone[i] = g;
}

#ifdef DVS_TEST_HOOKS
struct IndexEmit {   // dvs_test_compact_rows: the flagged rows' indices
  int* out;
  __device__ void operator()(size_t i, size_t p) const { out[p] = (int)i; }
};
#endif

}  // namespace dvs

using namespace dvs;

namespace {

dvs_status backend_grow_tables(dvs_backend* h, size_t need_lm, size_t need_ob, size_t need_kf) {
  hipStream_t st = h->ctx->stream;
  DVS_TRY(table_regrow(h->lm, need_lm, (size_t)h->nlm, st));
  DVS_TRY(table_regrow(h->ob, need_ob, (size_t)h->nob, st));
  if (need_kf > h->cap_kf) {
    size_t c = std::max<size_t>(h->cap_kf, 1);
    while (c < need_kf) c *= 2;
    Column<double, 9> r; Column<double, 3> t;
    DVS_TRY(alloc_rows(c, r, t));
    const size_t n = h->kfs.size();
    if (n) {
      DVS_HIP(hipMemcpyAsync(r.get(), h->kf_R.get(), n * r.row_bytes, hipMemcpyDeviceToDevice, st)); DVS_HIP(hipMemcpyAsync(t.get(), h->kf_t.get(), n * t.row_bytes, hipMemcpyDeviceToDevice, st));
    }
    DVS_HIP(hipStreamSynchronize(st));
    h->kf_R = std::move(r); h->kf_t = std::move(t); h->cap_kf = c;
  }
  return DVS_OK;
}

void quat_to_R(const double* q_xyzw, double* R) {   // extractPoseFromTransform (:1194-1215)
  double qx = q_xyzw[0], qy = q_xyzw[1], qz = q_xyzw[2], qw = q_xyzw[3];
  const double norm = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= norm; qx /= norm; qy /= norm; qz /= norm;
  R[0] = 1 - 2 * (qy * qy + qz * qz); R[1] = 2 * (qx * qy - qw * qz); R[2] = 2 * (qx * qz + qw * qy);
  R[3] = 2 * (qx * qy + qw * qz); R[4] = 1 - 2 * (qx * qx + qz * qz); R[5] = 2 * (qy * qz - qw * qx);
  R[6] = 2 * (qx * qz - qw * qy); R[7] = 2 * (qy * qz + qw * qx); R[8] = 1 - 2 * (qx * qx + qy * qy);
}

}  // namespace

// landmark -> views CSR over the whole table into v_lm.offs and v_ob.kf / .px / .oid (nothing to do for an empty landmark table)
dvs_status dvs::backend_views_build(dvs_backend* h) {
  hipStream_t st = h->ctx->stream;
  const int nlm = h->nlm, nob = h->nob;
  if (nlm == 0) return DVS_OK;
  DVS_TRY(h->v_lm.grow((size_t)nlm)); DVS_TRY(h->v_ob.grow((size_t)nob));
  DVS_HIP(hipMemsetAsync(h->v_lm.cnt.get(), 0, (size_t)nlm * 4, st));
  DVS_HIP(hipMemsetAsync(h->v_lm.fill.get(), 0, (size_t)nlm * 4, st));
  const ObView ob = h->ob.view();
  if (nob) hipLaunchKernelGGL(k_views_count, dim3((nob + 255) / 256), dim3(256), 0, st, ob, nob, (const i64*)h->lm.id.get(), nlm, h->v_ob.slot.get(), h->v_lm.cnt.get());
  launch_scan_counts(st, (const int*)h->v_lm.cnt.get(), nlm, h->v_lm.offs.get());
  if (nob) hipLaunchKernelGGL(k_views_scatter, dim3((nob + 255) / 256), dim3(256), 0, st, (const int*)h->v_ob.slot.get(), nob, (const i64*)h->v_lm.offs.get(), h->v_lm.fill.get(), h->v_ob.rows.get());
  hipLaunchKernelGGL(k_views_finish, dim3((nlm + 255) / 256), dim3(256), 0, st, ob, (int)h->kfs.size(), nlm, (const i64*)h->v_lm.offs.get(), h->v_ob.rows.get(), h->v_ob.kf.get(),
                     h->v_ob.px.get(), h->v_ob.oid.get());
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

// :1303-1312 keyframes' observation_ids lose the removed ids
int dvs::backend_drop_observation_ids(dvs_backend* h, const std::vector<i64>& rid, const std::vector<int>& rkf) {
  std::unordered_set<uint64_t> gone(rid.begin(), rid.end());
  std::unordered_set<int> touched(rkf.begin(), rkf.end());
  int n = 0;
  for (int k : touched) {
    if (k < 0 || k >= (int)h->kfs.size()) continue;
    std::vector<uint64_t>& ids = h->kfs[(size_t)k].obs_ids;
    const size_t before = ids.size();
    ids.erase(std::remove_if(ids.begin(), ids.end(), [&](uint64_t id) { return gone.count(id) != 0; }), ids.end());
    n += ids.size() != before ? 1 : 0;
  }
  return n;
}

extern "C" {

void dvs_backend_default_params(dvs_backend_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_descriptor_distance = 50.0; p->max_reprojection_distance = 5.0;
  p->window = 5; p->prune_min_observations = 2; p->prune_max_age_sec = 20.0;
  p->initial_capacity = 4096;
}

dvs_status dvs_backend_create(const dvs_backend_params* params, int32_t device, dvs_backend** out) {
  DVS_ARG(params && out);
  *out = nullptr;
  const dvs_backend_params& P = *params;
  DVS_ARG(P.fx > 0 && P.fy > 0 && P.window >= 1 && P.initial_capacity >= 1 && P.n_filtered >= 0 && P.n_filtered <= DVS_BACKEND_MAX_FILTERED);
  DVS_ARG(P.max_descriptor_distance >= 0 && P.max_reprojection_distance >= 0);
  for (int k = 0; k < P.n_filtered; k++) DVS_ARG(P.filtered_class_ids[k] >= 0);
  DVS_TRY(check_device(device));
  dvs_backend* h = new (std::nothrow) dvs_backend();
  if (!h) { set_error("dvs_backend_create: out of memory"); return DVS_ERR_HIP; }
  h->P = P; h->device = device;
  dvs_status s = dvs_matcher_create(device, &h->ctx);
  auto alloc_all = [&]() -> dvs_status {
    DVS_TRY(backend_grow_tables(h, (size_t)P.initial_capacity, (size_t)P.initial_capacity, 16));
    DVS_TRY(h->s_small.alloc(1)); DVS_TRY(h->d_Rt.alloc(12));
    return DVS_OK;
  };
  if (s == DVS_OK) s = alloc_all();
  if (s != DVS_OK) { dvs_backend_destroy(h); return s; }
  *out = h;
  return DVS_OK;
}

void dvs_backend_destroy(dvs_backend* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->ctx) { (void)hipStreamSynchronize(h->ctx->stream); dvs_matcher_destroy(h->ctx); }
  delete h;
}

dvs_status dvs_backend_reset(dvs_backend* h) {
  DVS_ARG(h);
  DVS_TRY(dvs_matcher_synchronize(h->ctx));
  h->nlm = h->nob = 0; h->kfs.clear(); h->kf_index.clear(); h->next_obs = h->next_lm = 0;
  h->nstat = 0; h->n_recorded = 0;                   // "Landmark culling": the statistics are emptied, the recording switch stays as set
  return DVS_OK;
}

dvs_status dvs_backend_counts(dvs_backend* h, dvs_backend_count* out) {
  DVS_ARG(h && out);
  out->n_keyframes = (int64_t)h->kfs.size(); out->n_observations = h->nob; out->n_landmarks = h->nlm;
  out->next_observation_id = h->next_obs; out->next_landmark_id = h->next_lm;
  return DVS_OK;
}

dvs_status dvs_backend_add_keyframe(dvs_backend* h, const dvs_keyframe_header* hdr, int32_t n, const double* landmark_xyz, const double* obs_pixels,
                                    const uint8_t* obs_desc, const dvs_detection* detections, int32_t ndet, dvs_backend_result* result) {
  DVS_ARG(h && hdr && result && n >= 0 && ndet >= 0);
  DVS_ARG(n == 0 || (landmark_xyz && obs_pixels && obs_desc));
  DVS_ARG(ndet == 0 || detections);
  memset(result, 0, sizeof(*result));
  const dvs_backend_params& P = h->P;
  if (h->kf_index.count(hdr->keyframe_id)) { set_error("dvs_backend_add_keyframe: frame_id %llu is in the map already", (unsigned long long)hdr->keyframe_id); return DVS_ERR_ARG; }
  // the distinct unfiltered classes a detection can give, class 0 first
  std::vector<int> classes(1, 0);
  auto filtered = [&](int c) { for (int k = 0; k < P.n_filtered; k++) if (P.filtered_class_ids[k] == c) return true; return false; };
  for (int d = 0; d < ndet; d++) {
    DVS_ARG(detections[d].class_id >= 0);
    const int c = detections[d].class_id;
    if (std::find(classes.begin(), classes.end(), c) == classes.end()) classes.push_back(c);
  }
  classes.erase(std::remove_if(classes.begin(), classes.end(), filtered), classes.end());
  if (classes.size() > 64) { set_error("dvs_backend_add_keyframe: %zu classes in one keyframe, 64 are held", classes.size()); return DVS_ERR_UNSUPPORTED; }
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const i64 stamp = (i64)hdr->stamp_sec * 1000000000ll + (i64)hdr->stamp_nanosec;
  const int kf = (int)h->kfs.size();
  KeyframeRec K;
  K.frame_id = hdr->keyframe_id; K.stamp = stamp;
  quat_to_R(hdr->rotation_xyzw, K.R);
  for (int k = 0; k < 3; k++) K.t[k] = hdr->translation[k];
  result->first_observation_id = h->next_obs; result->first_landmark_id = h->next_lm;
  const int nlm = h->nlm;
  std::vector<int> code((size_t)n, 0);
  std::vector<i64> match_id((size_t)n, -1);
  struct Hit { int inc, moved; };
  std::map<int, Hit> hits;                            // landmark row -> matches in this keyframe
  if (n > 0) {
    // ---- :735-751: pixels as cv::Point2f, positions as cv::Point3f, categories
    DVS_TRY(h->kf_ob.grow((size_t)n));
    DVS_TRY(grow(h->s_det, h->c_det, (size_t)ndet));
    h->h_px.resize((size_t)n * 2); h->h_xyz.resize((size_t)n * 3); h->h_det.resize((size_t)ndet);
    for (size_t k = 0; k < (size_t)n * 2; k++) h->h_px[k] = (float)obs_pixels[k];
    for (size_t k = 0; k < (size_t)n * 3; k++) h->h_xyz[k] = (float)landmark_xyz[k];
    for (int d = 0; d < ndet; d++) h->h_det[d] = DetRec{detections[d].cx, detections[d].cy, detections[d].w, detections[d].h, detections[d].class_id, 0};
    h->h_small = BackendSmall();
    for (int k = 0; k < P.n_filtered; k++) h->h_small.filtered[k] = P.filtered_class_ids[k];
    for (size_t k = 0; k < classes.size(); k++) h->h_small.classes[k] = classes[k];
    DVS_TRY(copy_in(h->kf_ob.s_px, h->h_px.data(), (size_t)n, st)); DVS_TRY(copy_in(h->kf_ob.s_xyz, h->h_xyz.data(), (size_t)n, st)); DVS_TRY(copy_in(h->kf_ob.s_desc, obs_desc, (size_t)n, st));
    if (ndet) DVS_HIP(hipMemcpyAsync(h->s_det.get(), h->h_det.data(), (size_t)ndet * sizeof(DetRec), hipMemcpyHostToDevice, st));
    DVS_HIP(hipMemcpyAsync(h->s_small.get(), &h->h_small, sizeof(BackendSmall), hipMemcpyHostToDevice, st));
    double Rt[12];
    memcpy(Rt, K.R, 72); memcpy(Rt + 9, K.t, 24);
    DVS_HIP(hipMemcpyAsync(h->d_Rt.get(), Rt, 96, hipMemcpyHostToDevice, st));
    BackendSmall* sm = h->s_small.get();
    hipLaunchKernelGGL(k_categorize, dim3(1), dim3(256), 0, st, (const float*)h->kf_ob.s_px.get(), (const uint8_t*)h->kf_ob.s_desc.get(), n, (const DetRec*)h->s_det.get(), ndet,
                       (const int*)sm->filtered, P.n_filtered, (const int*)sm->classes, (int)classes.size(), h->kf_ob.s_code.get(), h->kf_ob.s_order.get(), h->kf_ob.q_px.get(), h->kf_ob.q_desc.get(),
                       sm->class_cnt);
    DVS_HIP(hipGetLastError());
    // ---- :772 for every landmark at once, from the views stored before this keyframe
    if (nlm > 0) {
      DVS_TRY(backend_views_build(h));
      DVS_TRY(dvs_triangulate_landmarks_device(h->ctx, kf, h->kf_R.get(), h->kf_t.get(), P.fx, P.fy, P.cx, P.cy, nlm, (const int64_t*)h->v_lm.offs.get(), h->v_ob.kf.get(),
                                               h->v_ob.px.get(), h->lm.xyz.get(), h->v_lm.tri_xyz.get(), h->v_lm.tri_status.get()));
    }
    int class_cnt[64] = {0};
    DVS_TRY(copy_out(code.data(), h->kf_ob.s_code, (size_t)n, st));
    DVS_TRY(small_read(h, sm->class_cnt, class_cnt, 64));
    // ---- :758 per class present: gather, associate, walk
    std::vector<std::vector<int>> by_class(classes.size());
    for (int i = 0; i < n; i++) {
      if (code[i] < 0) continue;
      const size_t k = std::find(classes.begin(), classes.end(), code[i]) - classes.begin();
      if (k == classes.size()) { set_error("dvs_backend_add_keyframe: observation %d came back with class %d", i, code[i]); return DVS_ERR_HIP; }
      by_class[k].push_back(i);
    }
    for (size_t k = 0; k < classes.size(); k++)     // the device's grouped lists (q_px / q_desc) must be the lists the walk indexes
      if (class_cnt[k] != (int)by_class[k].size()) { set_error("dvs_backend_add_keyframe: class %d holds %d observations on the device, %zu on the host", classes[k], class_cnt[k], by_class[k].size()); return DVS_ERR_HIP; }
    size_t off = 0;
    for (size_t k = 0; k < classes.size(); off += by_class[k].size(), k++) {
      const std::vector<int>& mine = by_class[k];
      const int no = (int)mine.size();
      if (no == 0 || nlm == 0) continue;
      DVS_TRY(h->cls_lm.grow((size_t)nlm));
      hipLaunchKernelGGL(k_class_gather, dim3(1), dim3(256), 0, st, h->lm.view(), nlm, classes[k], h->cls_lm.slot.get(), h->cls_lm.desc.get(), h->cls_lm.xyz.get(), sm->counts);
      DVS_HIP(hipGetLastError());
      int nl = 0;
      DVS_TRY(small_read(h, sm->counts, &nl));
      if (nl <= 0) continue;                          // a class seen for the first time
      const long long* d_offs; const int* d_pairs; long long total = 0;
      DVS_TRY(associate_rows_device(h->ctx, h->kf_ob.q_desc.get() + 32 * off, h->kf_ob.q_px.get() + 2 * off, no, h->cls_lm.desc.get(), h->cls_lm.xyz.get(), nl, h->d_Rt.get(), P.fx, P.fy, P.cx,
                                    P.cy, P.max_descriptor_distance, P.max_reprojection_distance, h->kf_ob.d_best.get(), &d_offs, &d_pairs, &total));
      if (total == 0) continue;
      DVS_TRY(grow(h->p_rec, h->c_pair, (size_t)total));
      hipLaunchKernelGGL(k_pair_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_pairs, (i64)total, (const int*)h->cls_lm.slot.get(), (const i64*)h->lm.id.get(),
                         (const float*)h->lm.xyz.get(), (const float*)h->v_lm.tri_xyz.get(), (const int*)h->v_lm.tri_status.get(), h->p_rec.get());
      DVS_HIP(hipGetLastError());
      std::vector<int> best((size_t)no);
      std::vector<i64> offs((size_t)no + 1);
      std::vector<PairRec> rec((size_t)total);
      DVS_TRY(copy_out(best.data(), h->kf_ob.d_best, (size_t)no, st));
      DVS_HIP(hipMemcpyAsync(offs.data(), d_offs, ((size_t)no + 1) * 8, hipMemcpyDeviceToHost, st));
      DVS_HIP(hipMemcpyAsync(rec.data(), h->p_rec.get(), (size_t)total * sizeof(PairRec), hipMemcpyDeviceToHost, st));
      DVS_HIP(hipStreamSynchronize(st));
      // associateSequential's walk (include/dvslam/association.hpp): an observation whose candidates moved is evaluated again
      std::unordered_set<int> moved;
      for (int e = 0; e < no; e++) {
        const int i = mine[e];
        int bj = best[e];
        if (!moved.empty()) {
          bool stale = false;
          for (i64 p = offs[e]; p < offs[e + 1] && !stale; p++) stale = moved.count(rec[p].j) != 0;
          if (stale) {
            bj = -1;
            double be = DBL_MAX;
            for (i64 p = offs[e]; p < offs[e + 1]; p++) {
              const PairRec& r = rec[p];
              const double err = dvslam::reprojection_error(&h->h_px[2 * (size_t)i], moved.count(r.j) ? r.tri : r.xyz, K.R, K.t, P.fx, P.fy, P.cx, P.cy);
              if (err < P.max_reprojection_distance && err < be) { bj = r.j; be = err; }
            }
          }
        }
        if (bj < 0) continue;
        const PairRec* hit = nullptr;
        for (i64 p = offs[e]; p < offs[e + 1] && !hit; p++) if (rec[p].j == bj) hit = &rec[p];
        if (!hit) { set_error("dvs_backend_add_keyframe: best landmark %d is not among observation %d's candidates", bj, i); return DVS_ERR_HIP; }
        match_id[i] = hit->id;
        Hit& H = hits[hit->slot];
        H.inc++;
        if (hit->status == DVS_TRI_UPDATED) { H.moved = 1; moved.insert(bj); }
      }
    }
  }
  // ---- one pass in message order: observation ids, new landmark ids (:744-797)
  std::vector<int> app_src, new_src;
  std::vector<i64> app_lm;
  for (int i = 0; i < n; i++) {
    if (code[i] < 0) { result->n_filtered++; continue; }
    K.obs_ids.push_back((uint64_t)h->next_obs++);
    app_src.push_back(i);
    if (match_id[i] >= 0) { app_lm.push_back(match_id[i]); result->n_associated++; }
    else { app_lm.push_back(h->next_lm++); new_src.push_back(i); }
  }
  const int m = (int)app_src.size(), mn = (int)new_src.size(), mh = (int)hits.size();
  result->n_kept = m; result->n_created = mn;
  // ---- :766-772 on the matched landmarks, then :803-820
  DVS_TRY(backend_grow_tables(h, (size_t)nlm + mn, (size_t)h->nob + m, (size_t)kf + 1));
  h->h_int.clear(); h->h_i64 = app_lm;
  h->h_int.insert(h->h_int.end(), app_src.begin(), app_src.end());
  h->h_int.insert(h->h_int.end(), new_src.begin(), new_src.end());
  for (const auto& kv : hits) h->h_int.push_back(kv.first);
  for (const auto& kv : hits) h->h_int.push_back(kv.second.inc);
  for (const auto& kv : hits) { h->h_int.push_back(kv.second.moved); result->n_moved += kv.second.moved; }
  DVS_TRY(grow(h->a_int, h->c_aint, h->h_int.size())); DVS_TRY(grow(h->a_i64, h->c_ai64, h->h_i64.size()));
  if (!h->h_int.empty()) DVS_HIP(hipMemcpyAsync(h->a_int.get(), h->h_int.data(), h->h_int.size() * 4, hipMemcpyHostToDevice, st));
  if (m) DVS_HIP(hipMemcpyAsync(h->a_i64.get(), h->h_i64.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
  const int* a = h->a_int.get();
  if (mh) hipLaunchKernelGGL(k_match_apply, dim3((mh + 255) / 256), dim3(256), 0, st, mh, a + m + mn, a + m + mn + mh, a + m + mn + 2 * mh, stamp, (const float*)h->v_lm.tri_xyz.get(),
                             h->lm.view(), nlm);
  if (m) hipLaunchKernelGGL(k_append_obs, dim3((m + 255) / 256), dim3(256), 0, st, m, a, (const i64*)h->a_i64.get(), result->first_observation_id, (i64)K.frame_id, kf,
                            (const float*)h->kf_ob.s_px.get(), (const uint8_t*)h->kf_ob.s_desc.get(), (const int*)h->kf_ob.s_code.get(), n, h->ob.view(), h->nob);
  if (mn) hipLaunchKernelGGL(k_append_lm, dim3((mn + 255) / 256), dim3(256), 0, st, mn, a + m, result->first_landmark_id, stamp, (const float*)h->kf_ob.s_xyz.get(),
                             (const uint8_t*)h->kf_ob.s_desc.get(), (const int*)h->kf_ob.s_code.get(), n, h->lm.view(), nlm);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipMemcpyAsync(h->kf_R.get() + 9 * (size_t)kf, K.R, h->kf_R.row_bytes, hipMemcpyHostToDevice, st));
  DVS_HIP(hipMemcpyAsync(h->kf_t.get() + 3 * (size_t)kf, K.t, h->kf_t.row_bytes, hipMemcpyHostToDevice, st));
  DVS_HIP(hipStreamSynchronize(st));
  h->nob += m; h->nlm += mn;
  h->kf_index[K.frame_id] = kf;
  h->kfs.push_back(std::move(K));
  return DVS_OK;
}

dvs_status dvs_backend_add_keyframe_cdr(dvs_backend* h, const uint8_t* payload, size_t len, const dvs_detection* detections, int32_t ndet,
                                        dvs_backend_result* result) {
  DVS_ARG(h && payload && result);
  const int32_t cap = (int32_t)std::min<size_t>(len / 28 + 1, 1u << 30);
  std::vector<double> xyz((size_t)cap * 3), px((size_t)cap * 2);
  std::vector<uint8_t> desc((size_t)cap * 32);
  dvs_keyframe_header hdr;
  char fid[256];
  int32_t nl = 0, no = 0;
  DVS_TRY(dvs_keyframe_unpack_cdr(payload, len, &hdr, fid, sizeof(fid), nullptr, xyz.data(), nullptr, px.data(), desc.data(), cap, &nl, &no));
  if (nl != no) { set_error("dvs_backend_add_keyframe_cdr: %d landmarks, %d observations", nl, no); return DVS_ERR_ARG; }   // :735-737 pairs them by index
  return dvs_backend_add_keyframe(h, &hdr, no, xyz.data(), px.data(), desc.data(), detections, ndet, result);
}

dvs_status dvs_backend_get_window(dvs_backend* h, int32_t cap_kf, int32_t cap_obs, int32_t cap_lm, uint64_t* kf_frame_id, double* kf_R, double* kf_t,
                                  int32_t* n_kf, float* obs_px, uint64_t* obs_lm_id, int32_t* obs_class, uint64_t* obs_frame_id, int32_t* obs_lm_index,
                                  int32_t* n_obs, uint64_t* lm_id, int32_t* lm_class, float* lm_xyz, int32_t* n_lm) {
  DVS_ARG(h && n_kf && n_obs && n_lm && cap_kf >= 0 && cap_obs >= 0 && cap_lm >= 0);
  const int nkf = (int)h->kfs.size(), w = std::min(h->P.window, nkf), start = nkf - w;   // :895-896
  *n_kf = w; *n_obs = 0; *n_lm = 0;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const int nob = h->nob, nlm = h->nlm;
  int counts[2] = {0, 0};
  if (w > 0 && nob > 0) {
    DVS_TRY(h->win_ob.grow((size_t)nob)); DVS_TRY(h->win_lm.grow((size_t)nlm));
    int* d_counts = h->s_small.get()->counts;
    hipLaunchKernelGGL(k_window_gather, dim3(1), dim3(256), 0, st, h->ob.view(), nob, h->lm.view(), nlm, start, h->win_lm.flag.get(), h->win_lm.pos.get(), h->win_ob.oi.get(),
                       h->win_ob.slot.get(), h->win_ob.o.px.get(), h->win_ob.o.lm.get(), h->win_ob.o.cls.get(), h->win_ob.o.frame.get(), h->win_ob.o.lmidx.get(), h->win_lm.l.id.get(), h->win_lm.l.cls.get(), h->win_lm.l.xyz.get(),
                       d_counts);
    DVS_HIP(hipGetLastError());
    DVS_TRY(small_read(h, d_counts, counts, 2));
  }
  *n_obs = counts[0]; *n_lm = counts[1];
  if (w > cap_kf || counts[0] > cap_obs || counts[1] > cap_lm) {
    set_error("dvs_backend_get_window: %d keyframes / %d observations / %d landmarks, capacities %d / %d / %d", w, counts[0], counts[1], cap_kf, cap_obs, cap_lm);
    return DVS_ERR_CAPACITY;
  }
  for (int k = 0; k < w; k++) {
    const KeyframeRec& K = h->kfs[(size_t)start + k];
    if (kf_frame_id) kf_frame_id[k] = K.frame_id;
    if (kf_R) memcpy(kf_R + 9 * (size_t)k, K.R, 72);
    if (kf_t) memcpy(kf_t + 3 * (size_t)k, K.t, 24);
  }
  DVS_TRY(window_copy_out(h->win_ob.o, (size_t)counts[0], h->win_lm.l, (size_t)counts[1], obs_px, obs_lm_id, obs_class, obs_frame_id, obs_lm_index, lm_id, lm_class, lm_xyz, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_apply_optimized(dvs_backend* h, int32_t nposes, const uint64_t* frame_ids, const double* R, const double* t, int32_t nlm,
                                       const uint64_t* lm_ids, const int32_t* lm_class, const double* lm_xyz) {
  DVS_ARG(h && nposes >= 0 && nlm >= 0);
  DVS_ARG(nposes == 0 || (frame_ids && R && t));
  DVS_ARG(nlm == 0 || (lm_ids && lm_class && lm_xyz));
  if (nposes == 0 && nlm == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  h->h_int.clear(); h->h_dbl.clear(); h->h_i64.clear();
  for (int k = 0; k < nlm; k++) { h->h_i64.push_back((i64)lm_ids[k]); h->h_int.push_back(lm_class[k]); }
  h->h_dbl.insert(h->h_dbl.end(), lm_xyz, lm_xyz + 3 * (size_t)nlm);
  int np = 0;
  for (int k = 0; k < nposes; k++) {                  // :1358-1370: the keyframe with that frame_id, if any
    const auto it = h->kf_index.find(frame_ids[k]);
    if (it == h->kf_index.end()) continue;
    KeyframeRec& K = h->kfs[(size_t)it->second];
    memcpy(K.R, R + 9 * (size_t)k, 72); memcpy(K.t, t + 3 * (size_t)k, 24);
    h->h_int.push_back(it->second);
    h->h_dbl.insert(h->h_dbl.end(), K.R, K.R + 9); h->h_dbl.insert(h->h_dbl.end(), K.t, K.t + 3);
    np++;
  }
  DVS_TRY(grow(h->a_int, h->c_aint, h->h_int.size())); DVS_TRY(grow(h->a_i64, h->c_ai64, h->h_i64.size())); DVS_TRY(grow(h->a_dbl, h->c_adbl, h->h_dbl.size()));
  if (!h->h_int.empty()) DVS_HIP(hipMemcpyAsync(h->a_int.get(), h->h_int.data(), h->h_int.size() * 4, hipMemcpyHostToDevice, st));
  if (!h->h_i64.empty()) DVS_HIP(hipMemcpyAsync(h->a_i64.get(), h->h_i64.data(), h->h_i64.size() * 8, hipMemcpyHostToDevice, st));
  if (!h->h_dbl.empty()) DVS_HIP(hipMemcpyAsync(h->a_dbl.get(), h->h_dbl.data(), h->h_dbl.size() * 8, hipMemcpyHostToDevice, st));
  const int g = (std::max(nlm, np) + 255) / 256;
  if (g) hipLaunchKernelGGL(k_apply, dim3(g), dim3(256), 0, st, (int)nlm, (const i64*)h->a_i64.get(), (const int*)h->a_int.get(), (const double*)h->a_dbl.get(), h->lm.view(),
                            h->nlm, np, (const int*)h->a_int.get() + nlm, (const double*)h->a_dbl.get() + 3 * (size_t)nlm, h->kf_R.get(), h->kf_t.get(), (int)h->kfs.size());
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_prune(dvs_backend* h, int32_t now_sec, uint32_t now_nanosec, int32_t* removed_landmarks, int32_t* removed_observations) {
  DVS_ARG(h && removed_landmarks && removed_observations);
  *removed_landmarks = *removed_observations = 0;
  const int nlm = h->nlm, nob = h->nob;
  if (nlm == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const i64 now = (i64)now_sec * 1000000000ll + (i64)now_nanosec;
  BackendSmall* sm = h->s_small.get();
  DVS_TRY(compact_grow(h));
  DVS_HIP(hipMemsetAsync(&sm->marked, 0, 4, st));
  hipLaunchKernelGGL(k_prune_mark, dim3((nlm + 255) / 256), dim3(256), 0, st, h->lm.view(), nlm, now, h->P.prune_min_observations, h->P.prune_max_age_sec, h->cmp_lm.keep.get(),
                     h->cmp_lm.gone.get(), &sm->marked);
  DVS_HIP(hipGetLastError());
  int marked = 0;
  DVS_TRY(small_read(h, &sm->marked, &marked));
  if (marked == 0) return DVS_OK;                    // the common BA cycle: nothing to compact
  if (nob) hipLaunchKernelGGL(k_prune_ob_flag, dim3((nob + 255) / 256), dim3(256), 0, st, (const i64*)h->lm.id.get(), nlm, (const int*)h->cmp_lm.gone.get(), (const i64*)h->ob.lm.get(),
                              nob, h->cmp_ob.keep.get(), h->cmp_ob.gone.get());
  TablesReplaced done;
  DVS_TRY(tables_replace(h, "dvs_backend_prune", h->cmp_lm.keep.get(), RowAsIs(), (i64)nlm - marked, h->cmp_ob.keep.get(), RowAsIs(), -1, h->cmp_ob.gone.get(), &done));
  *removed_landmarks = marked; *removed_observations = done.n_ob_gone;
  return DVS_OK;
}

dvs_status dvs_backend_get_landmarks(dvs_backend* h, int32_t cap, int64_t cap_obs_ids, uint64_t* id, int32_t* class_id, float* xyz, uint8_t* desc,
                                     int32_t* observation_count, int64_t* last_seen_ns, int64_t* obs_offsets, uint64_t* obs_ids, int32_t* n,
                                     int64_t* n_obs_ids) {
  DVS_ARG(h && n && cap >= 0 && cap_obs_ids >= 0);
  const size_t nlm = (size_t)h->nlm;
  *n = h->nlm;
  if (n_obs_ids) *n_obs_ids = 0;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  i64 nv = 0;
  const bool want_csr = obs_offsets || obs_ids || n_obs_ids;
  if (want_csr && nlm) {
    DVS_TRY(backend_views_build(h));
    DVS_HIP(hipMemcpyAsync(&nv, h->v_lm.offs.get() + nlm, sizeof(i64), hipMemcpyDeviceToHost, st));
    DVS_HIP(hipStreamSynchronize(st));
    if (n_obs_ids) *n_obs_ids = nv;
  }
  if (h->nlm > cap || (obs_ids && nv > cap_obs_ids)) {
    set_error("dvs_backend_get_landmarks: %d landmarks / %lld observation ids, capacities %d / %lld", h->nlm, (long long)nv, cap, (long long)cap_obs_ids);
    return DVS_ERR_CAPACITY;
  }
  if (obs_offsets && nlm == 0) obs_offsets[0] = 0;
  if (nlm == 0) return DVS_OK;
  DVS_TRY(copy_out(id, h->lm.id, nlm, st)); DVS_TRY(copy_out(class_id, h->lm.cls, nlm, st)); DVS_TRY(copy_out(xyz, h->lm.xyz, nlm, st));
  DVS_TRY(copy_out(desc, h->lm.desc, nlm, st)); DVS_TRY(copy_out(observation_count, h->lm.cnt, nlm, st)); DVS_TRY(copy_out(last_seen_ns, h->lm.seen, nlm, st));
  DVS_TRY(copy_out(obs_offsets, h->v_lm.offs, nlm + 1, st));
  if (nv) DVS_TRY(copy_out(obs_ids, h->v_ob.oid, (size_t)nv, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_get_observations(dvs_backend* h, int32_t cap, uint64_t* id, uint64_t* frame_id, float* px, uint8_t* desc, int32_t* class_id,
                                        uint64_t* landmark_id, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  const size_t nob = (size_t)h->nob;
  *n = h->nob;
  if (h->nob > cap) { set_error("dvs_backend_get_observations: %d rows, capacity %d", h->nob, cap); return DVS_ERR_CAPACITY; }
  if (nob == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_TRY(copy_out(id, h->ob.id, nob, st)); DVS_TRY(copy_out(frame_id, h->ob.frame, nob, st)); DVS_TRY(copy_out(px, h->ob.px, nob, st));
  DVS_TRY(copy_out(desc, h->ob.desc, nob, st)); DVS_TRY(copy_out(class_id, h->ob.cls, nob, st)); DVS_TRY(copy_out(landmark_id, h->ob.lm, nob, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_get_keyframes(dvs_backend* h, int32_t cap, int64_t cap_obs_ids, uint64_t* frame_id, int64_t* stamp_ns, double* R, double* t,
                                     int64_t* obs_offsets, uint64_t* obs_ids, int32_t* n, int64_t* n_obs_ids) {
  DVS_ARG(h && n && cap >= 0 && cap_obs_ids >= 0);
  const size_t nkf = h->kfs.size();
  int64_t total = 0;
  for (const KeyframeRec& K : h->kfs) total += (int64_t)K.obs_ids.size();
  *n = (int32_t)nkf;
  if (n_obs_ids) *n_obs_ids = total;
  if ((int64_t)nkf > cap || (obs_ids && total > cap_obs_ids)) {
    set_error("dvs_backend_get_keyframes: %zu keyframes / %lld observation ids, capacities %d / %lld", nkf, (long long)total, cap, (long long)cap_obs_ids);
    return DVS_ERR_CAPACITY;
  }
  // the poses come from the device: they are part of the resident map (the host copies serve the window and the walk)
  if (nkf && (R || t)) {
    DVS_HIP(hipSetDevice(h->device));
    hipStream_t st = h->ctx->stream;
    DVS_TRY(copy_out(R, h->kf_R, nkf, st)); DVS_TRY(copy_out(t, h->kf_t, nkf, st));
    DVS_HIP(hipStreamSynchronize(st));
  }
  int64_t o = 0;
  for (size_t k = 0; k < nkf; k++) {
    const KeyframeRec& K = h->kfs[k];
    if (frame_id) frame_id[k] = K.frame_id;
    if (stamp_ns) stamp_ns[k] = K.stamp;
    if (obs_offsets) obs_offsets[k] = o;
    if (obs_ids) for (size_t e = 0; e < K.obs_ids.size(); e++) obs_ids[o + (int64_t)e] = K.obs_ids[e];
    o += (int64_t)K.obs_ids.size();
  }
  if (obs_offsets) obs_offsets[nkf] = o;
  return DVS_OK;
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test.h)
dvs_status dvs_test_compact_rows(dvs_backend* h, int32_t n, const int32_t* flags, int32_t* out_pos, int64_t* out_total) {
  DVS_ARG(h && n >= 0 && out_total && (n == 0 || (flags && out_pos)));
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_TRY(h->blk.grow((size_t)n / 256 + 2));
  DVS_TRY(grow(h->a_int, h->c_aint, 2 * (size_t)n));
  int* d_flag = h->a_int.get();
  int* d_out = d_flag + n;
  if (n) {
    DVS_HIP(hipMemcpyAsync(d_flag, flags, (size_t)n * 4, hipMemcpyHostToDevice, st));
    DVS_HIP(hipMemsetAsync(d_out, 0xFF, (size_t)n * 4, st));
  }
  i64 total = -1;
  DVS_TRY(compact_rows(h, d_flag, n, IndexEmit{d_out}, &total));
  if (n) DVS_HIP(hipMemcpyAsync(out_pos, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  *out_total = total;
  return DVS_OK;
}
#endif  // DVS_TEST_HOOKS

}  // extern "C"
