// loop_close.hip — loop closing on the map the mapping backend keeps on the device (include/dvslam_hip.h "Loop closing on the map"):
// the anchors of the landmarks, the pose graph the keyframes imply, dvs_backend_close_loop (pose-graph solve through the public dvs_pgo_*
// entry points, poses written back, landmarks moved in place with their anchor keyframes) and landmark fusion — ORB-SLAM's CorrectLoop and
// SearchAndFuse as published ideas; the rule is the library's own, stated in the header and restated in tests/loop_closing_ref.py.
//
// The kernels this file adds (tables in ascending id, so "ascending id" is "ascending row"):
//   k_anchors        per landmark the keyframe of the first view of its segment in the views CSR (backend_views_build), -1 without one
//   k_fuse_mark      per observation: its landmark's row, and the landmark flagged target (named by the query keyframe q) or entry-side
//                    (named by a keyframe of E) with an integer atomic OR; the observation that sets a target's flag first counts it
//   k_fuse_lists     one workgroup, trips of 256 (block_ops.h): q's observations — one run of the table, found by binary search — packed
//                    in table order (pixel, class, id, target row, descriptor), and the source rows (entry-side and not target) in ascending id
//   k_fuse_propose   one lane per source, 256 per workgroup: camera point and float pixel once, the descriptor in eight registers; q's
//                    packed observations stream through LDS in tiles of 256 (14 KB; every lane reads the same row, a broadcast), eight
//                    rows per step: class compare and per-axis float gate for all eight, then for the rare rows that pass the exact
//                    double error and only then the popcount; the lane keeps its smallest (e, observation id) and lowers the target's
//                    best error with a 64-bit integer atomicMin on e's bits
//   k_fuse_resolve   among the proposals whose e equals the target's minimum the lowest source row wins (integer atomicMin)
//   k_fuse_pairs     per target with a winner: redirect[removed row] = survivor row, partner[survivor row] = removed row
//   k_fuse_pairlist  one workgroup: the kept pairs in ascending removed id (survivor id, removed id, e) and their count
//   k_fuse_repoint   observations naming a removed landmark name its survivor
//   k_fuse_keep / FuseLmFix   the landmark table without the removed rows (table_compact.h's tables_replace, the observation table
//                    untouched): a row stays iff nothing redirects it, the survivors with the summed observation_count and the later
//                    last_seen
// No floating-point atomics anywhere: (e, id) is a total order and every minimum is an integer minimum, so two identical calls on
// identical maps give identical bytes.
#include <limits.h>
#include <math.h>
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

struct FuseCam { double R[9], t[3], fx, fy, cx, cy, max_reproj, max_desc; float gate; };   // gate: the least float >= max_reproj

const int kFuseTile = 256;
const int kRoleQuery = 1, kRoleEntry = 2;
const int kNoSource = 0x7F7F7F7F;            // f_bsrc after its memset: above every row
const int kNoRow = INT_MIN, kNoLane = INT_MIN + 1;   // class ids are >= 0: neither equals one, nor the other

__global__ __launch_bounds__(256) void k_anchors(int nlm, const i64* __restrict__ offs, const int* __restrict__ view_kf, int* __restrict__ anchor,
                                                 int* __restrict__ n_anchored) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nlm) return;
  const int a = offs[s + 1] > offs[s] ? view_kf[offs[s]] : -1;
  anchor[s] = a;
  if (a >= 0) atomicAdd(n_anchored, 1);
}

__global__ __launch_bounds__(256) void k_fuse_mark(ObView ob, int nob, const i64* __restrict__ lm_id, int nlm, const int* __restrict__ role, int nkf,
                                                   int* __restrict__ ob_row, int* __restrict__ flag, int* __restrict__ n_targets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nob) return;
  const int s = lm_find(lm_id, nlm, ob.lm[i]);
  ob_row[i] = s;
  const int k = ob.kf[i];
  if (s < 0 || k < 0 || k >= nkf || role[k] == 0) return;
  const int before = atomicOr(&flag[s], role[k]);
  if (role[k] == kRoleQuery && (before & kRoleQuery) == 0) atomicAdd(n_targets, 1);   // the first of q's observations to name it
}

// first row of the ascending keyframe column that holds `key` or more (n if none)
__device__ __forceinline__ int kf_lower_bound(const int* __restrict__ kf, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kf[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// counts: {q observations kept, sources}; at most cap_q observations are written (the host holds the count against cap_q).  The
// observations of one keyframe are ONE RUN of the table — rows are appended keyframe by keyframe and every compaction keeps the order —
// so the walk covers that run only, found by two binary searches on the keyframe column.
__global__ __launch_bounds__(256) void k_fuse_lists(ObView ob, int nob, int nlm, int q, const int* __restrict__ ob_row, const int* __restrict__ flag, int cap_q,
                                                    float* __restrict__ q_px, int* __restrict__ q_cls, i64* __restrict__ q_oid, int* __restrict__ q_brow,
                                                    uint8_t* __restrict__ q_desc, int* __restrict__ src, int* __restrict__ counts) {
  __shared__ int s_w[4];
  const int first = kf_lower_bound(ob.kf, nob, q), end = kf_lower_bound(ob.kf, nob, q + 1);
  int nq = 0;
  for (int i0 = first; i0 < end; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool keep = i < end && ob.kf[i] == q && ob_row[i] >= 0;
    int total;
    const int p = nq + block_rank256(keep, s_w, total);
    if (keep && p < cap_q) {
      q_px[2 * p] = ob.px[2 * i]; q_px[2 * p + 1] = ob.px[2 * i + 1];
      q_cls[p] = ob.cls[i]; q_oid[p] = ob.id[i]; q_brow[p] = ob_row[i];
      copy32(q_desc + 32 * (size_t)p, ob.desc + 32 * (size_t)i);
    }
    nq += total;
  }
  int ns = 0;
  for (int s0 = 0; s0 < nlm; s0 += 256) {
    const int s = s0 + threadIdx.x;
    const bool source = s < nlm && flag[s] == kRoleEntry;
    int total;
    const int p = ns + block_rank256(source, s_w, total);
    if (source) src[p] = s;
    ns += total;
  }
  if (threadIdx.x == 0) { counts[0] = nq; counts[1] = ns; }
}

// counts: as k_fuse_lists wrote them; n_prop: proposals made
__global__ __launch_bounds__(256) void k_fuse_propose(LmView lm, const int* __restrict__ src, const int* __restrict__ counts, int cap_q, FuseCam cam,
                                                      const float* __restrict__ q_px, const int* __restrict__ q_cls, const i64* __restrict__ q_oid,
                                                      const int* __restrict__ q_brow, const uint8_t* __restrict__ q_desc, u64* __restrict__ prop_e,
                                                      int* __restrict__ prop_b, u64* __restrict__ best_e, int* __restrict__ n_prop) {
  __shared__ __attribute__((aligned(16))) float s_px[2 * kFuseTile];
  __shared__ __attribute__((aligned(16))) int s_cls[kFuseTile];
  __shared__ int s_brow[kFuseTile];
  __shared__ i64 s_oid[kFuseTile];
  __shared__ uint32_t s_desc[8 * kFuseTile];
  const int ns = counts[1], nq = min(counts[0], cap_q);
  if ((int)blockIdx.x * 256 >= ns) return;          // the grid is sized by the landmark table: whole workgroups past the sources leave
  const int g = blockIdx.x * 256 + threadIdx.x;
  const bool live = g < ns;
  const int a = live ? src[g] : 0;
  float u = -1.f, v = -1.f;
  int cls = kNoLane;                                // a lane without a source, or with one behind the camera, matches no row's class
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const float* X = lm.xyz + 3 * (size_t)a;
    const double d0 = (double)X[0] - cam.t[0], d1 = (double)X[1] - cam.t[1], d2 = (double)X[2] - cam.t[2];
    const double c0 = cam.R[0] * d0 + cam.R[3] * d1 + cam.R[6] * d2;
    const double c1 = cam.R[1] * d0 + cam.R[4] * d1 + cam.R[7] * d2;
    const double c2 = cam.R[2] * d0 + cam.R[5] * d1 + cam.R[8] * d2;
    if (c2 > 0) {
      u = (float)(cam.fx * c0 / c2 + cam.cx); v = (float)(cam.fy * c1 / c2 + cam.cy);
      cls = lm.cls[a];
    }
    const uint4 lo = reinterpret_cast<const uint4*>(lm.desc + 32 * (size_t)a)[0], hi = reinterpret_cast<const uint4*>(lm.desc + 32 * (size_t)a)[1];
    d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w; d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
  }
  double be = 0;
  i64 bo = -1;
  int bb = -1;
  for (int r0 = 0; r0 < nq; r0 += kFuseTile) {
    const int r = r0 + threadIdx.x;
    __syncthreads();                                // the tile before may still be read
    if (r < nq) {
      s_px[2 * threadIdx.x] = q_px[2 * r]; s_px[2 * threadIdx.x + 1] = q_px[2 * r + 1];
      s_cls[threadIdx.x] = q_cls[r]; s_brow[threadIdx.x] = q_brow[r]; s_oid[threadIdx.x] = q_oid[r];
      const uint4 lo = reinterpret_cast<const uint4*>(q_desc + 32 * (size_t)r)[0], hi = reinterpret_cast<const uint4*>(q_desc + 32 * (size_t)r)[1];
      uint32_t* w = s_desc + 8 * threadIdx.x;
      w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
    } else {
      s_cls[threadIdx.x] = kNoRow;                  // the tile's tail matches no class
      s_px[2 * threadIdx.x] = 0.f; s_px[2 * threadIdx.x + 1] = 0.f;
    }
    __syncthreads();
    const int m = (min(kFuseTile, nq - r0) + 7) & ~7;
    // eight rows at a time: their sixteen LDS reads are independent and issue back to back; the rare rows that pass the class
    // compare and the per-axis gate (e >= |dx| and e >= |dy|, so the gate never rejects a candidate) are then looked at one by one
    for (int k0 = 0; k0 < m; k0 += 8) {
      // six 16-byte LDS reads, no branch between them: with `&&` the compiler reads the eight rows one after the other
      const int4 ca = *reinterpret_cast<const int4*>(s_cls + k0), cb = *reinterpret_cast<const int4*>(s_cls + k0 + 4);
      const float4 p0 = *reinterpret_cast<const float4*>(s_px + 2 * k0), p1 = *reinterpret_cast<const float4*>(s_px + 2 * k0 + 4);
      const float4 p2 = *reinterpret_cast<const float4*>(s_px + 2 * k0 + 8), p3 = *reinterpret_cast<const float4*>(s_px + 2 * k0 + 12);
      const int rc[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
      const float rx[8] = {p0.x, p0.z, p1.x, p1.z, p2.x, p2.z, p3.x, p3.z}, ry[8] = {p0.y, p0.w, p1.y, p1.w, p2.y, p2.w, p3.y, p3.w};
      unsigned hit = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float dx = __fsub_rn(rx[j], u), dy = __fsub_rn(ry[j], v);
        hit |= ((unsigned)(rc[j] == cls) & (unsigned)(fabsf(dx) < cam.gate) & (unsigned)(fabsf(dy) < cam.gate)) << j;
      }
      while (hit) {
        const int k = k0 + __ffs(hit) - 1;
        hit &= hit - 1;
        const float dx = __fsub_rn(s_px[2 * k], u), dy = __fsub_rn(s_px[2 * k + 1], v);
        const double e = sqrt((double)dx * dx + (double)dy * dy);
        if (!(e < cam.max_reproj)) continue;
        const uint32_t* w = s_desc + 8 * k;
        int h = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) h += __popc(d[c] ^ w[c]);
        if (!((double)h < cam.max_desc)) continue;
        const i64 o = s_oid[k];
        if (bb < 0 || e < be || (e == be && o < bo)) { be = e; bo = o; bb = s_brow[k]; }
      }
    }
  }
  if (!live) return;
  prop_b[g] = bb;
  if (bb >= 0) {
    const u64 bits = (u64)__double_as_longlong(be);   // e >= 0: the bit pattern orders as the value does
    prop_e[g] = bits;
    atomicMin(&best_e[bb], bits);
    atomicAdd(n_prop, 1);
  }
}

__global__ __launch_bounds__(256) void k_fuse_resolve(const int* __restrict__ src, const int* __restrict__ counts, const u64* __restrict__ prop_e,
                                                      const int* __restrict__ prop_b, const u64* __restrict__ best_e, int* __restrict__ best_src) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= counts[1]) return;
  const int b = prop_b[g];
  if (b >= 0 && prop_e[g] == best_e[b]) atomicMin(&best_src[b], src[g]);
}

__global__ __launch_bounds__(256) void k_fuse_pairs(int nlm, const int* __restrict__ flag, const int* __restrict__ best_src, int* __restrict__ redirect,
                                                    int* __restrict__ partner) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nlm || (flag[b] & kRoleQuery) == 0) return;
  const int a = best_src[b];
  if (a == kNoSource || a < 0 || a >= nlm) return;   // nobody proposed
  const int keep = min(a, b), gone = max(a, b);
  redirect[gone] = keep; partner[keep] = gone;
}

__global__ __launch_bounds__(256) void k_fuse_pairlist(int nlm, const i64* __restrict__ lm_id, const int* __restrict__ flag, const int* __restrict__ redirect,
                                                       const u64* __restrict__ best_e, i64* __restrict__ p_surv, i64* __restrict__ p_rem, double* __restrict__ p_e,
                                                       int* __restrict__ n_fused) {
  __shared__ int s_w[4];
  int n = 0;
  for (int s0 = 0; s0 < nlm; s0 += 256) {
    const int s = s0 + threadIdx.x;
    const bool gone = s < nlm && redirect[s] >= 0;
    int total;
    const int p = n + block_rank256(gone, s_w, total);
    if (gone) {
      const int k = redirect[s];
      const int target = (flag[s] & kRoleQuery) ? s : k;
      p_surv[p] = lm_id[k]; p_rem[p] = lm_id[s]; p_e[p] = __longlong_as_double((long long)best_e[target]);
    }
    n += total;
  }
  if (threadIdx.x == 0) *n_fused = n;
}

__global__ __launch_bounds__(256) void k_fuse_repoint(i64* __restrict__ ob_lm, int nob, const int* __restrict__ ob_row, const int* __restrict__ redirect,
                                                      const i64* __restrict__ lm_id) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nob) return;
  const int s = ob_row[i];
  if (s >= 0 && redirect[s] >= 0) ob_lm[i] = lm_id[redirect[s]];
}

__global__ __launch_bounds__(256) void k_fuse_keep(const int* __restrict__ redirect, int nlm, int* __restrict__ keep) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < nlm) keep[s] = redirect[s] < 0 ? 1 : 0;
}
// a landmark row that stays: a survivor takes its partner's observations and the later of the two last_seen
struct FuseLmFix {
  const int* partner; int nlm;
  __device__ void operator()(const LmView& nl, size_t p, const LmView& lm, size_t s) const {
    const int o = partner[s];
    if (o >= 0 && o < nlm) { nl.cnt[p] = lm.cnt[s] + lm.cnt[o]; nl.seen[p] = max(lm.seen[s], lm.seen[o]); }
  }
};

}  // namespace dvs

using namespace dvs;

namespace {

bool finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

struct Graph {
  std::vector<double> R, t, rvec, tvec, w_rot, w_trans;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> ei, ej;
};

// the header's Log on Q = R_a^T R_b, every product a left-to-right sum
void relative_pose(const double* Ra, const double* ta, const double* Rb, const double* tb, double* rvec, double* tvec) {
  double Q[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Q[3 * r + c] = Ra[r] * Rb[c] + Ra[3 + r] * Rb[3 + c] + Ra[6 + r] * Rb[6 + c];
  const double d[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
  for (int r = 0; r < 3; r++) tvec[r] = Ra[r] * d[0] + Ra[3 + r] * d[1] + Ra[6 + r] * d[2];
  const double v[3] = {(Q[7] - Q[5]) / 2, (Q[2] - Q[6]) / 2, (Q[3] - Q[1]) / 2};
  const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), c = (Q[0] + Q[4] + Q[8] - 1) / 2;
  const double theta = atan2(s, c);
  const double k = s > 1e-12 ? theta / s : 1.0;
  for (int a = 0; a < 3; a++) rvec[a] = s > 1e-12 ? v[a] * k : v[a];
}

// the checks and the graph of dvs_backend_build_pose_graph; nothing but `g` is written
dvs_status build_graph(dvs_backend* h, int32_t n_loops, const uint64_t* lq, const uint64_t* le, const double* l_rvec, const double* l_tvec, const double* l_wr,
                       const double* l_wt, double odo_wr, double odo_wt, Graph& g) {
  DVS_ARG(n_loops >= 0);
  DVS_ARG(n_loops == 0 || (lq && le && l_rvec && l_tvec && l_wr && l_wt));
  DVS_ARG(isfinite(odo_wr) && isfinite(odo_wt) && odo_wr > 0 && odo_wt > 0);
  const int nkf = (int)h->kfs.size();
  if (nkf < 2) { set_error("loop closing needs at least two keyframes, the map holds %d", nkf); return DVS_ERR_ARG; }
  const size_t ne = (size_t)nkf - 1 + (size_t)n_loops;
  g.R.resize((size_t)nkf * 9); g.t.resize((size_t)nkf * 3); g.fixed.assign((size_t)nkf, 0);
  g.ei.resize(ne); g.ej.resize(ne); g.rvec.resize(ne * 3); g.tvec.resize(ne * 3); g.w_rot.resize(ne); g.w_trans.resize(ne);
  g.fixed[0] = 1;
  for (int k = 0; k < nkf; k++) { memcpy(&g.R[9 * (size_t)k], h->kfs[(size_t)k].R, 72); memcpy(&g.t[3 * (size_t)k], h->kfs[(size_t)k].t, 24); }
  for (size_t k = 0; k < g.R.size(); k++) DVS_ARG(isfinite(g.R[k]));
  for (size_t k = 0; k < g.t.size(); k++) DVS_ARG(isfinite(g.t[k]));
  for (int k = 0; k + 1 < nkf; k++) {
    g.ei[(size_t)k] = k; g.ej[(size_t)k] = k + 1; g.w_rot[(size_t)k] = odo_wr; g.w_trans[(size_t)k] = odo_wt;
    relative_pose(&g.R[9 * (size_t)k], &g.t[3 * (size_t)k], &g.R[9 * (size_t)k + 9], &g.t[3 * (size_t)k + 3], &g.rvec[3 * (size_t)k], &g.tvec[3 * (size_t)k]);
  }
  for (int l = 0; l < n_loops; l++) {
    const size_t e = (size_t)nkf - 1 + (size_t)l;
    const auto iq = h->kf_index.find(lq[l]), ie = h->kf_index.find(le[l]);
    if (iq == h->kf_index.end() || ie == h->kf_index.end()) {
      set_error("loop %d names frame %llu / %llu, which the map does not hold", l, (unsigned long long)lq[l], (unsigned long long)le[l]);
      return DVS_ERR_ARG;
    }
    DVS_ARG(iq->second != ie->second);
    DVS_ARG(finite3(l_rvec + 3 * (size_t)l) && finite3(l_tvec + 3 * (size_t)l) && isfinite(l_wr[l]) && isfinite(l_wt[l]) && l_wr[l] > 0 && l_wt[l] > 0);
    g.ei[e] = iq->second; g.ej[e] = ie->second; g.w_rot[e] = l_wr[l]; g.w_trans[e] = l_wt[l];
    memcpy(&g.rvec[3 * e], l_rvec + 3 * (size_t)l, 24); memcpy(&g.tvec[3 * e], l_tvec + 3 * (size_t)l, 24);
  }
  return DVS_OK;
}

bool fuse_params_ok(const dvs_fuse_params& p) {
  return isfinite(p.max_descriptor_distance) && isfinite(p.max_reprojection_distance) && p.max_descriptor_distance > 0 && p.max_reprojection_distance > 0 &&
         p.fuse_neighbours >= 0 && p.fuse_neighbours <= 31;   // at most 63 entry keyframes
}

// anchors of all landmarks into f_anchor, the number of anchored ones into s_small's fuse.n_anchored; asynchronous on the handle's stream
dvs_status anchors_build(dvs_backend* h) {
  hipStream_t st = h->ctx->stream;
  const int nlm = h->nlm;
  if (nlm == 0) return DVS_OK;
  DVS_TRY(backend_views_build(h));
  DVS_TRY(grow(h->f_anchor, h->c_flm, (size_t)nlm));
  int* n_anchored = &h->s_small.get()->fuse.n_anchored;
  DVS_HIP(hipMemsetAsync(n_anchored, 0, 4, st));
  hipLaunchKernelGGL(k_anchors, dim3((nlm + 255) / 256), dim3(256), 0, st, nlm, (const i64*)h->v_lm.offs.get(), (const int*)h->v_ob.kf.get(), h->f_anchor.get(), n_anchored);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

// fusion over the keyframe indices q and E (checked by the caller); the pair list stays on the device in fuse_lm.psurv / .prem / .pe
dvs_status fuse_run(dvs_backend* h, int q, const std::vector<int>& E, const dvs_fuse_params& P, bool apply, dvs_fuse_result* out, int32_t cap_pairs,
                    uint64_t* survivor_id, uint64_t* removed_id, double* err, int32_t* n_pairs) {
  memset(out, 0, sizeof(*out));
  if (n_pairs) *n_pairs = 0;
  const int nlm = h->nlm, nob = h->nob, nkf = (int)h->kfs.size();
  if (nlm == 0 || nob == 0) return DVS_OK;           // nobody names anybody: no launch
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const KeyframeRec& K = h->kfs[(size_t)q];
  const int cap_q = (int)std::max<size_t>(K.obs_ids.size(), 1);
  DVS_TRY(h->fuse_lm.grow((size_t)nlm));
  DVS_TRY(grow(h->f_obrow, h->c_fob, (size_t)nob));
  DVS_TRY(h->fuse_q.grow((size_t)cap_q));
  // keyframe roles ride in a_int
  h->h_int.assign((size_t)nkf, 0);
  for (int k : E) h->h_int[(size_t)k] = kRoleEntry;
  h->h_int[(size_t)q] = kRoleQuery;
  DVS_TRY(grow(h->a_int, h->c_aint, (size_t)nkf));
  DVS_HIP(hipMemcpyAsync(h->a_int.get(), h->h_int.data(), (size_t)nkf * 4, hipMemcpyHostToDevice, st));
  FuseCounts* fc = &h->s_small.get()->fuse;              // kernels take the record as ints from n_query on
  DVS_HIP(hipMemsetAsync(fc, 0, offsetof(FuseCounts, n_anchored), st));
  DVS_HIP(hipMemsetAsync(h->fuse_lm.flag.get(), 0, (size_t)nlm * 4, st));
  DVS_HIP(hipMemsetAsync(h->fuse_lm.beste.get(), 0xFF, (size_t)nlm * 8, st));
  DVS_HIP(hipMemsetAsync(h->fuse_lm.bsrc.get(), 0x7F, (size_t)nlm * 4, st));
  DVS_HIP(hipMemsetAsync(h->fuse_lm.redirect.get(), 0xFF, (size_t)nlm * 4, st));
  DVS_HIP(hipMemsetAsync(h->fuse_lm.partner.get(), 0xFF, (size_t)nlm * 4, st));
  FuseCam cam;
  memcpy(cam.R, K.R, 72); memcpy(cam.t, K.t, 24);
  cam.fx = h->P.fx; cam.fy = h->P.fy; cam.cx = h->P.cx; cam.cy = h->P.cy;
  cam.max_reproj = P.max_reprojection_distance; cam.max_desc = P.max_descriptor_distance;
  cam.gate = (float)cam.max_reproj;
  if ((double)cam.gate < cam.max_reproj) cam.gate = nextafterf(cam.gate, INFINITY);
  const dim3 g_ob((nob + 255) / 256), g_lm((nlm + 255) / 256), b(256);
  const LmView lm = h->lm.view();
  const ObView ob = h->ob.view();
  hipLaunchKernelGGL(k_fuse_mark, g_ob, b, 0, st, ob, nob, (const i64*)lm.id, nlm, (const int*)h->a_int.get(), nkf, h->f_obrow.get(), h->fuse_lm.flag.get(), &fc->n_targets);
  hipLaunchKernelGGL(k_fuse_lists, dim3(1), b, 0, st, ob, nob, nlm, q, (const int*)h->f_obrow.get(), (const int*)h->fuse_lm.flag.get(), cap_q, h->fuse_q.px.get(), h->fuse_q.cls.get(),
                     h->fuse_q.oid.get(), h->fuse_q.brow.get(), h->fuse_q.desc.get(), h->fuse_lm.src.get(), &fc->n_query);
  hipLaunchKernelGGL(k_fuse_propose, g_lm, b, 0, st, lm, (const int*)h->fuse_lm.src.get(), (const int*)&fc->n_query, cap_q, cam, (const float*)h->fuse_q.px.get(), (const int*)h->fuse_q.cls.get(),
                     (const i64*)h->fuse_q.oid.get(), (const int*)h->fuse_q.brow.get(), (const uint8_t*)h->fuse_q.desc.get(), h->fuse_lm.prope.get(), h->fuse_lm.propb.get(), h->fuse_lm.beste.get(), &fc->n_proposals);
  hipLaunchKernelGGL(k_fuse_resolve, g_lm, b, 0, st, (const int*)h->fuse_lm.src.get(), (const int*)&fc->n_query, (const u64*)h->fuse_lm.prope.get(), (const int*)h->fuse_lm.propb.get(),
                     (const u64*)h->fuse_lm.beste.get(), h->fuse_lm.bsrc.get());
  hipLaunchKernelGGL(k_fuse_pairs, g_lm, b, 0, st, nlm, (const int*)h->fuse_lm.flag.get(), (const int*)h->fuse_lm.bsrc.get(), h->fuse_lm.redirect.get(), h->fuse_lm.partner.get());
  hipLaunchKernelGGL(k_fuse_pairlist, dim3(1), b, 0, st, nlm, (const i64*)lm.id, (const int*)h->fuse_lm.flag.get(), (const int*)h->fuse_lm.redirect.get(), (const u64*)h->fuse_lm.beste.get(),
                     h->fuse_lm.psurv.get(), h->fuse_lm.prem.get(), h->fuse_lm.pe.get(), &fc->n_fused);
  DVS_HIP(hipGetLastError());
  int c[5] = {0, 0, 0, 0, 0};                          // n_query .. n_fused
  DVS_TRY(small_read(h, &fc->n_query, c, 5));
  if (c[0] < 0 || c[0] > cap_q || c[1] < 0 || c[1] > nlm || c[4] < 0 || c[4] > c[3] || c[4] > c[2]) {
    set_error("dvs_backend_fuse: inconsistent counts %d %d %d %d %d (keyframe %d lists %d observations)", c[0], c[1], c[2], c[3], c[4], q, cap_q);
    return DVS_ERR_HIP;
  }
  out->n_sources = c[1]; out->n_targets = c[2]; out->n_proposals = c[3]; out->n_fused = c[4];
  const int nf = c[4];
  if (n_pairs) *n_pairs = nf;
  const bool want = survivor_id || removed_id || err;
  if (want && nf > cap_pairs) { set_error("dvs_backend_fuse: %d pairs, capacity %d", nf, cap_pairs); return DVS_ERR_CAPACITY; }
  if (want && nf) {
    DVS_TRY(copy_out(survivor_id, h->fuse_lm.psurv, (size_t)nf, st)); DVS_TRY(copy_out(removed_id, h->fuse_lm.prem, (size_t)nf, st)); DVS_TRY(copy_out(err, h->fuse_lm.pe, (size_t)nf, st));
  }
  if (apply && nf) {
    DVS_TRY(compact_grow(h));
    hipLaunchKernelGGL(k_fuse_repoint, g_ob, b, 0, st, ob.lm, nob, (const int*)h->f_obrow.get(), (const int*)h->fuse_lm.redirect.get(), (const i64*)lm.id);
    hipLaunchKernelGGL(k_fuse_keep, g_lm, b, 0, st, (const int*)h->fuse_lm.redirect.get(), nlm, h->cmp_lm.keep.get());
    DVS_HIP(hipGetLastError());
    TablesReplaced done;
    DVS_TRY(tables_replace(h, "dvs_backend_fuse", h->cmp_lm.keep.get(), FuseLmFix{h->fuse_lm.partner.get(), nlm}, (i64)nlm - nf, nullptr, RowAsIs(), -1, nullptr, &done));
  } else if (want && nf) {
    DVS_HIP(hipStreamSynchronize(st));
  }
  return DVS_OK;
}

dvs_status fuse_resolve_frames(dvs_backend* h, uint64_t query, const uint64_t* entries, int32_t n_entry, int* q, std::vector<int>& E) {
  DVS_ARG(entries && n_entry >= 1 && n_entry <= 64);
  const auto iq = h->kf_index.find(query);
  if (iq == h->kf_index.end()) { set_error("dvs_backend_fuse: the map does not hold frame %llu", (unsigned long long)query); return DVS_ERR_ARG; }
  *q = iq->second;
  E.clear();
  for (int k = 0; k < n_entry; k++) {
    const auto it = h->kf_index.find(entries[k]);
    if (it == h->kf_index.end()) { set_error("dvs_backend_fuse: the map does not hold frame %llu", (unsigned long long)entries[k]); return DVS_ERR_ARG; }
    DVS_ARG(it->second != *q);
    DVS_ARG(std::find(E.begin(), E.end(), it->second) == E.end());
    E.push_back(it->second);
  }
  return DVS_OK;
}

}  // namespace

extern "C" {

dvs_status dvs_fuse_default_params(dvs_fuse_params* p) {
  DVS_ARG(p);
  memset(p, 0, sizeof(*p));
  p->max_descriptor_distance = 50.0; p->max_reprojection_distance = 5.0; p->fuse_neighbours = 2;
  return DVS_OK;
}

dvs_status dvs_backend_get_anchors(dvs_backend* h, int32_t cap, uint64_t* lm_id, int32_t* anchor_kf, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->nlm;
  if (h->nlm > cap) { set_error("dvs_backend_get_anchors: %d landmarks, capacity %d", h->nlm, cap); return DVS_ERR_CAPACITY; }
  if (h->nlm == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_TRY(anchors_build(h));
  DVS_TRY(copy_out(lm_id, h->lm.id, (size_t)h->nlm, st)); DVS_TRY(copy_out(anchor_kf, h->f_anchor, (size_t)h->nlm, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_build_pose_graph(dvs_backend* h, int32_t n_loops, const uint64_t* loop_query_frame_id, const uint64_t* loop_entry_frame_id,
                                        const double* loop_rvec, const double* loop_tvec, const double* loop_w_rot, const double* loop_w_trans, double odo_w_rot,
                                        double odo_w_trans, int32_t cap_nodes, int32_t cap_edges, double* R, double* t, uint8_t* fixed, int32_t* ei, int32_t* ej,
                                        double* rvec, double* tvec, double* w_rot, double* w_trans, int32_t* n_nodes, int32_t* n_edges) {
  DVS_ARG(h && n_nodes && n_edges && cap_nodes >= 0 && cap_edges >= 0);
  *n_nodes = *n_edges = 0;
  Graph g;
  DVS_TRY(build_graph(h, n_loops, loop_query_frame_id, loop_entry_frame_id, loop_rvec, loop_tvec, loop_w_rot, loop_w_trans, odo_w_rot, odo_w_trans, g));
  const size_t nn = g.fixed.size(), ne = g.ei.size();
  *n_nodes = (int32_t)nn; *n_edges = (int32_t)ne;
  if (nn > (size_t)cap_nodes || ne > (size_t)cap_edges) {
    set_error("dvs_backend_build_pose_graph: %zu nodes / %zu edges, capacities %d / %d", nn, ne, cap_nodes, cap_edges);
    return DVS_ERR_CAPACITY;
  }
  if (R) memcpy(R, g.R.data(), nn * 72);
  if (t) memcpy(t, g.t.data(), nn * 24);
  if (fixed) memcpy(fixed, g.fixed.data(), nn);
  if (ei) memcpy(ei, g.ei.data(), ne * 4);
  if (ej) memcpy(ej, g.ej.data(), ne * 4);
  if (rvec) memcpy(rvec, g.rvec.data(), ne * 24);
  if (tvec) memcpy(tvec, g.tvec.data(), ne * 24);
  if (w_rot) memcpy(w_rot, g.w_rot.data(), ne * 8);
  if (w_trans) memcpy(w_trans, g.w_trans.data(), ne * 8);
  return DVS_OK;
}

dvs_status dvs_backend_fuse(dvs_backend* h, uint64_t query_frame_id, const uint64_t* entry_frame_ids, int32_t n_entry, const dvs_fuse_params* params, int32_t apply,
                            dvs_fuse_result* out, int32_t cap_pairs, uint64_t* survivor_id, uint64_t* removed_id, double* err, int32_t* n_pairs) {
  DVS_ARG(h && out && cap_pairs >= 0);
  dvs_fuse_params P;
  dvs_fuse_default_params(&P);
  if (params) P = *params;
  DVS_ARG(fuse_params_ok(P));
  int q = -1;
  std::vector<int> E;
  DVS_TRY(fuse_resolve_frames(h, query_frame_id, entry_frame_ids, n_entry, &q, E));
  return fuse_run(h, q, E, P, apply != 0, out, cap_pairs, survivor_id, removed_id, err, n_pairs);
}

dvs_status dvs_backend_close_loop(dvs_backend* h, dvs_pgo* pgo, int32_t n_loops, const uint64_t* loop_query_frame_id, const uint64_t* loop_entry_frame_id,
                                  const double* loop_rvec, const double* loop_tvec, const double* loop_w_rot, const double* loop_w_trans, double odo_w_rot,
                                  double odo_w_trans, const dvs_pgo_params* pgo_params, const dvs_fuse_params* fuse_params, dvs_close_loop_result* out) {
  DVS_ARG(h && pgo && out);
  memset(out, 0, sizeof(*out));
  if (fuse_params) DVS_ARG(fuse_params_ok(*fuse_params));
  Graph g;
  DVS_TRY(build_graph(h, n_loops, loop_query_frame_id, loop_entry_frame_id, loop_rvec, loop_tvec, loop_w_rot, loop_w_trans, odo_w_rot, odo_w_trans, g));
  const int nkf = (int)g.fixed.size(), ne = (int)g.ei.size();
  out->n_nodes = nkf; out->n_edges = ne;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_HIP(hipStreamSynchronize(st));                 // the pose graph works on its own stream
  DVS_TRY(dvs_pgo_set_nodes(pgo, nkf, g.R.data(), g.t.data(), g.fixed.data()));
  DVS_TRY(dvs_pgo_set_edges(pgo, ne, g.ei.data(), g.ej.data(), g.rvec.data(), g.tvec.data(), g.w_rot.data(), g.w_trans.data()));
  DVS_TRY(dvs_pgo_solve(pgo, pgo_params, &out->summary));
  if (out->summary.termination == 2) return DVS_OK;  // the map stays as it was
  // poses: the bytes dvs_pgo_get_nodes returns, on the host copy and in kf_R / kf_t
  DVS_TRY(dvs_pgo_get_nodes(pgo, g.R.data(), g.t.data()));
  for (int k = 0; k < nkf; k++) { memcpy(h->kfs[(size_t)k].R, &g.R[9 * (size_t)k], 72); memcpy(h->kfs[(size_t)k].t, &g.t[3 * (size_t)k], 24); }
  DVS_HIP(hipSetDevice(h->device));
  DVS_TRY(copy_in(h->kf_R, g.R.data(), (size_t)nkf, st)); DVS_TRY(copy_in(h->kf_t, g.t.data(), (size_t)nkf, st));
  // landmarks: in place on the table's xyz column with the device anchors
  if (h->nlm) {
    DVS_TRY(anchors_build(h));
    int moved = 0;
    DVS_TRY(small_read(h, &h->s_small.get()->fuse.n_anchored, &moved));
    out->n_landmarks_moved = moved;
    DVS_TRY(dvs_pgo_correct_points_device(pgo, h->nlm, h->lm.xyz.get(), h->f_anchor.get()));
    DVS_TRY(dvs_pgo_synchronize(pgo));
  } else {
    DVS_HIP(hipStreamSynchronize(st));
  }
  if (!fuse_params) return DVS_OK;
  for (int l = 0; l < n_loops; l++) {
    const int q = g.ei[(size_t)nkf - 1 + (size_t)l], entry = g.ej[(size_t)nkf - 1 + (size_t)l];
    std::vector<int> E;
    for (int k = std::max(0, entry - fuse_params->fuse_neighbours); k <= std::min(nkf - 1, entry + fuse_params->fuse_neighbours) && E.size() < 64; k++)
      if (k != q) E.push_back(k);
    if (E.empty()) continue;
    dvs_fuse_result r;
    DVS_TRY(fuse_run(h, q, E, *fuse_params, true, &r, 0, nullptr, nullptr, nullptr, nullptr));
    out->fuse.n_sources += r.n_sources; out->fuse.n_targets += r.n_targets; out->fuse.n_proposals += r.n_proposals; out->fuse.n_fused += r.n_fused;
  }
  return DVS_OK;
}

// Global BA over the whole map ("Global BA of the map" in the header).  The problem is assembled on the host from the tables' columns
// (one read-back per column, as the per-keyframe BA cycle's dvs_backend_get_window does); the solve is the caller's dvs_ba handle's.
dvs_status dvs_backend_global_ba(dvs_backend* h, dvs_ba* ba, const dvs_ba_global_params* params, dvs_backend_gba_result* out) {
  DVS_ARG(h && ba && out);
  memset(out, 0, sizeof(*out));
  const int nkf = (int)h->kfs.size(), nlm = h->nlm, nob = h->nob;
  if (nkf < 2) { set_error("dvs_backend_global_ba: %d keyframes, at least 2 are needed", nkf); return DVS_ERR_ARG; }
  std::vector<uint64_t> lm_id((size_t)std::max(nlm, 1)), ob_frame((size_t)std::max(nob, 1)), ob_lm((size_t)std::max(nob, 1));
  std::vector<int32_t> lm_cls((size_t)std::max(nlm, 1));
  std::vector<float> lm_xyz(3 * (size_t)std::max(nlm, 1)), ob_px(2 * (size_t)std::max(nob, 1));
  int32_t n = 0;
  DVS_TRY(dvs_backend_get_landmarks(h, nlm, 0, lm_id.data(), lm_cls.data(), lm_xyz.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &n, nullptr));
  DVS_TRY(dvs_backend_get_observations(h, nob, nullptr, ob_frame.data(), ob_px.data(), nullptr, nullptr, ob_lm.data(), &n));
  // observations whose landmark the table holds, then only those of landmarks with at least two of them
  std::vector<int> row((size_t)nob, -1), cnt((size_t)nlm, 0), camOf((size_t)nob, -1);
  for (int i = 0; i < nob; i++) {
    const auto it = std::lower_bound(lm_id.begin(), lm_id.begin() + nlm, ob_lm[(size_t)i]);
    const auto kf = h->kf_index.find(ob_frame[(size_t)i]);
    if (it == lm_id.begin() + nlm || *it != ob_lm[(size_t)i] || kf == h->kf_index.end()) continue;
    row[(size_t)i] = (int)(it - lm_id.begin()); camOf[(size_t)i] = kf->second;
    cnt[(size_t)row[(size_t)i]]++;
  }
  std::vector<int32_t> cam, lmi;
  std::vector<double> uv;
  for (int i = 0; i < nob; i++) {
    const int l = row[(size_t)i];
    if (l < 0 || cnt[(size_t)l] < 2) continue;
    cam.push_back(camOf[(size_t)i]); lmi.push_back(l);
    uv.push_back((double)ob_px[2 * (size_t)i]); uv.push_back((double)ob_px[2 * (size_t)i + 1]);
  }
  const int R = (int)cam.size();
  out->n_cameras = nkf; out->n_landmarks = nlm; out->n_observations = R; out->n_left_out = nob - R;
  if (R == 0) { set_error("dvs_backend_global_ba: no landmark of the map has two observations"); return DVS_ERR_ARG; }
  std::vector<double> q(4 * (size_t)nkf), t(3 * (size_t)nkf), X(3 * (size_t)nlm);
  for (int k = 0; k < nkf; k++) DVS_TRY(dvs_ba_pose_from_rt(h->kfs[(size_t)k].R, h->kfs[(size_t)k].t, &q[4 * (size_t)k], &t[3 * (size_t)k]));
  for (size_t i = 0; i < X.size(); i++) X[i] = (double)lm_xyz[i];
  std::vector<uint8_t> pose_fixed((size_t)nkf, 0);
  pose_fixed[0] = 1;                                   // the gauge, as SlidingWindowBA fixes its first keyframe
  DVS_TRY(dvs_ba_set_problem(ba, nkf, q.data(), t.data(), nlm, X.data(), R, cam.data(), lmi.data(), uv.data(), pose_fixed.data(), nullptr, h->P.fx, h->P.fy,
                             h->P.cx, h->P.cy, 1.0, 1.345));
  DVS_TRY(dvs_ba_solve_global(ba, params, &out->summary));
  if (out->summary.ba.termination != 0) return DVS_OK;   // the map stays as it was
  DVS_TRY(dvs_ba_get_parameters(ba, q.data(), t.data(), X.data()));
  std::vector<uint64_t> frames; std::vector<double> Rs, ts;
  for (int k = 1; k < nkf; k++) {
    double Rk[9], tk[3];
    DVS_TRY(dvs_ba_pose_to_rt(&q[4 * (size_t)k], &t[3 * (size_t)k], Rk, tk));
    frames.push_back(h->kfs[(size_t)k].frame_id); Rs.insert(Rs.end(), Rk, Rk + 9); ts.insert(ts.end(), tk, tk + 3);
  }
  std::vector<uint64_t> ids; std::vector<int32_t> cls; std::vector<double> xyz;
  for (int l = 0; l < nlm; l++) {
    if (cnt[(size_t)l] < 2) continue;                    // left without observations: keeps its position bytes
    ids.push_back(lm_id[(size_t)l]); cls.push_back(lm_cls[(size_t)l]); xyz.insert(xyz.end(), &X[3 * (size_t)l], &X[3 * (size_t)l] + 3);
  }
  return dvs_backend_apply_optimized(h, (int32_t)frames.size(), frames.data(), Rs.data(), ts.data(), (int32_t)ids.size(), ids.data(), cls.data(), xyz.data());
}

}  // extern "C"
