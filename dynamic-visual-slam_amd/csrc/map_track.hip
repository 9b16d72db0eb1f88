// map_track.hip — tracking a frame against the map (include/dvslam_hip.h "Tracking against the map", dvs_maptrack_*): the landmarks
// projected into the frame, a descriptor search in a window around each projection, a one-to-one assignment and the refinement of the
// frame's pose on the kept 3D-2D pairs.  The rule is stated in the header and restated in numpy in tests/map_track_ref.py; this file is
// its device form:
//   k_mt_cells     a keypoint per lane: its cell (or none), the cell histogram, the per-keypoint proposal key cleared
//   k_mt_scan      one workgroup: the exclusive scan of the histogram -> the CSR row starts
//   k_mt_scatter   a keypoint per lane into its cell's segment, in arrival order ...
//   k_mt_order     ... and each segment put in ascending keypoint index by rank (the counting sort's stable order)
//   k_mt_search    a landmark per lane: stage 1 in FP64, the walk over the window's cells with the descriptor as four 64-bit words,
//                  the proposal as ONE 64-bit atomicMin on (d << 40 | landmark row) at the best keypoint
//   k_mt_finalize  a keypoint per lane: the kept row, id and distance out of the key; the landmark's kept flag
//   k_mt_refine    ONE workgroup: gathers the kept pairs in keypoint order, then runs the four rounds of ten Gauss-Newton steps itself —
//                  per-lane strided partial sums, added through LDS in one fixed order, the 6 x 6 Cholesky on lane 0 — and writes the 128-byte record.  No host decision between iterations.
//                  The schedule (first round, rounds, steps per round) is an argument, 0, 4, 10 in every product launch; the product's
//                  instantiation has it as constants, the test hook's (dvs_test_maptrack_refine_steps: single steps compared) reads it.
//   k_mt_record_stats  (only from the dvs_backend_track_frame* calls, and only while the backend's recording is on; "Landmark culling" in the
//                  header) a row of the call per lane: visible and found of the row's id in the backend's statistics
// Every launch is on the handle's stream but that last one, which runs on the backend's; nothing is read back but the record.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "block_ops.h"
#include "backend_internal.h"
#include "maptrack_internal.h"

namespace dvs {

struct MtPose { double Rcw[9], tcw[3], R[9], t[3]; };   // the prior both ways: the kernels compute with the first, return the bytes of the second
struct MtRec { double u, v; int visible, best_k, d_best, d_second, proposed, kept; };   // dvs_maptrack_lm_record
static_assert(sizeof(MtRec) == sizeof(dvs_maptrack_lm_record), "record layout");
enum { MC_VISIBLE = 0, MC_PROPOSED = 1, MC_MATCHES = 2, MC_UNBINNED = 3, MC_GATE = 4, MC_INTS = 8 };   // MC_GATE .. + 3: near, far, back-facing, angle
// "Landmark refresh" in the header: the per-landmark viewing geometry and the gates' constants; read by k_mt_search<true> only
struct MtGateArgs { const double* normal; const double* range; const int* ncnt; double range_factor, cc; };
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kRefThreads = 256, kSums = 28;   // 21 of H's upper triangle, 6 of b, the cost

__global__ __launch_bounds__(256) void k_mt_cells(const dvs_keypoint* __restrict__ kps, int n_kp, int rows, int cols, int cell, int gw, int n_levels,
                                                  int* __restrict__ cellid, int* __restrict__ cnt, unsigned long long* __restrict__ key, int* __restrict__ counters) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_kp) return;
  const float x = kps[k].x, y = kps[k].y;
  const int oct = kps[k].octave;
  int c = -1;
  if (x >= 0.f && x < (float)cols && y >= 0.f && y < (float)rows && oct >= 0 && oct < n_levels) c = ((int)y / cell) * gw + (int)x / cell;
  cellid[k] = c;
  key[k] = kNoKey;
  if (c >= 0) atomicAdd(&cnt[c], 1);
  else atomicAdd(&counters[MC_UNBINNED], 1);
}

// start[c] = sum of cnt[0 .. c), start[ncell] = the number of binned keypoints
__global__ __launch_bounds__(256) void k_mt_scan(const int* __restrict__ cnt, int ncell, int* __restrict__ start) {
  __shared__ int s_v[256];
  __shared__ int s_base;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < ncell; c0 += 256) {
    const int c = c0 + threadIdx.x;
    const int v = c < ncell ? cnt[c] : 0;
    s_v[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // Hillis-Steele, inclusive
      const int add = threadIdx.x >= off ? s_v[threadIdx.x - off] : 0;
      __syncthreads();
      s_v[threadIdx.x] += add;
      __syncthreads();
    }
    const int base = s_base;
    if (c < ncell) start[c] = base + s_v[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 255) s_base = base + s_v[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) start[ncell] = s_base;
}

__global__ __launch_bounds__(256) void k_mt_scatter(const int* __restrict__ cellid, int n_kp, const int* __restrict__ start, int* __restrict__ fill,
                                                    int* __restrict__ arrival) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_kp) return;
  const int c = cellid[k];
  if (c >= 0) arrival[start[c] + atomicAdd(&fill[c], 1)] = k;
}

// slot s of a segment holds keypoint arrival[s]; its place in ascending index is its rank among the segment's (distinct) indices
__global__ __launch_bounds__(256) void k_mt_order(const int* __restrict__ cellid, const int* __restrict__ arrival, const int* __restrict__ start, int ncell,
                                                  int* __restrict__ order) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= start[ncell]) return;
  const int k = arrival[s], c = cellid[k];
  const int b = start[c], e = start[c + 1];
  int r = 0;
  for (int j = b; j < e; j++) r += arrival[j] < k ? 1 : 0;
  order[b + r] = k;
}

__device__ __forceinline__ void mt_camera_point(const MtPose& T, double X0, double X1, double X2, double* c) {
#pragma unroll
  for (int i = 0; i < 3; i++) c[i] = ((T.Rcw[3 * i] * X0 + T.Rcw[3 * i + 1] * X1) + T.Rcw[3 * i + 2] * X2) + T.tcw[i];
}

// kGated is a template argument, so the ungated instantiation holds none of the gates' code
template <bool kGated>
__global__ __launch_bounds__(256) void k_mt_search(dvs_maptrack_params P, MtPose T, MtGateArgs g, const float* __restrict__ xyz, const uint8_t* __restrict__ ldesc, int n_lm,
                                                   const dvs_keypoint* __restrict__ kps, const uint8_t* __restrict__ kdesc, const int* __restrict__ start,
                                                   const int* __restrict__ order, int gw, int gh, MtRec* __restrict__ rec,
                                                   unsigned long long* __restrict__ key, int* __restrict__ counters) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_lm) return;
  double c[3];
  mt_camera_point(T, (double)xyz[3 * (size_t)j], (double)xyz[3 * (size_t)j + 1], (double)xyz[3 * (size_t)j + 2], c);
  MtRec r;
  r.u = 0.0; r.v = 0.0; r.visible = 0; r.best_k = -1; r.d_best = -1; r.d_second = -1; r.proposed = 0; r.kept = 0;
  bool vis = P.min_z < c[2] && c[2] < P.max_z;
  if (kGated) {
    if (g.ncnt[j] > 0) {
      const double p0 = (double)xyz[3 * (size_t)j] - T.t[0], p1 = (double)xyz[3 * (size_t)j + 1] - T.t[1], p2 = (double)xyz[3 * (size_t)j + 2] - T.t[2];
      const double q = (p0 * p0 + p1 * p1) + p2 * p2;
      const double s = (p0 * g.normal[3 * (size_t)j] + p1 * g.normal[3 * (size_t)j + 1]) + p2 * g.normal[3 * (size_t)j + 2];
      const double a = g.range[2 * (size_t)j] / g.range_factor, b = g.range[2 * (size_t)j + 1] * g.range_factor;
      const int gate = q < a * a ? 0 : (q > b * b ? 1 : (s < 0.0 ? 2 : (s * s < g.cc * q ? 3 : -1)));
      if (gate >= 0) { vis = false; atomicAdd(&counters[MC_GATE + gate], 1); }
    }
  }
  double u = 0.0, v = 0.0;
  if (vis) {
    u = P.fx * c[0] / c[2] + P.cx;
    v = P.fy * c[1] / c[2] + P.cy;
    vis = 0.0 <= u && u < (double)P.cols && 0.0 <= v && v < (double)P.rows;
  }
  if (vis) {
    r.u = u; r.v = v; r.visible = 1;
    // the cells a candidate can lie in: a candidate has lo <= x, so (int)x >= floor(lo), and x <= hi, x < cols
    const double xlo = u - P.radius, xhi = u + P.radius, ylo = v - P.radius, yhi = v + P.radius;
    const int cx0 = xlo <= 0.0 ? 0 : (int)xlo / P.cell, cx1 = xhi >= (double)P.cols ? gw - 1 : (int)xhi / P.cell;
    const int cy0 = ylo <= 0.0 ? 0 : (int)ylo / P.cell, cy1 = yhi >= (double)P.rows ? gh - 1 : (int)yhi / P.cell;
    const unsigned long long* ld = reinterpret_cast<const unsigned long long*>(ldesc + 32 * (size_t)j);
    const unsigned long long l0 = ld[0], l1 = ld[1], l2 = ld[2], l3 = ld[3];
    unsigned long long best = kNoKey;   // d << 32 | k
    int second = -1;
    for (int cy = cy0; cy <= cy1; cy++) {
      const int b = start[cy * gw + cx0], e = start[cy * gw + cx1 + 1];   // the row's cells are one run of the CSR
      for (int s = b; s < e; s++) {
        const int k = order[s];
        const double dx = (double)kps[k].x - u, dy = (double)kps[k].y - v;
        if (!(fabs(dx) <= P.radius && fabs(dy) <= P.radius)) continue;
        const unsigned long long* kd = reinterpret_cast<const unsigned long long*>(kdesc + 32 * (size_t)k);
        const int d = (__popcll(l0 ^ kd[0]) + __popcll(l1 ^ kd[1])) + (__popcll(l2 ^ kd[2]) + __popcll(l3 ^ kd[3]));
        const unsigned long long cand = ((unsigned long long)d << 32) | (unsigned)k;
        if (cand < best) {
          if (best != kNoKey) second = (int)(best >> 32);   // the old best is the nearest of the others seen so far: it was <= second
          best = cand;
        } else if (second < 0 || d < second) {
          second = d;
        }
      }
    }
    if (best != kNoKey) {
      r.best_k = (int)(unsigned)best; r.d_best = (int)(best >> 32); r.d_second = second;
      const bool ratio_ok = second < 0 || P.ratio_pct <= 0 || (long long)r.d_best * 100 < (long long)P.ratio_pct * second;
      if (r.d_best < P.max_hamming && ratio_ok) {
        r.proposed = 1;
        atomicMin(&key[r.best_k], ((unsigned long long)r.d_best << 40) | (unsigned long long)j);
      }
    }
  }
  rec[j] = r;
  if (vis) atomicAdd(&counters[MC_VISIBLE], 1);   // (the compiler makes these one add per wavefront)
  if (r.proposed) atomicAdd(&counters[MC_PROPOSED], 1);
}

__global__ __launch_bounds__(256) void k_mt_finalize(const unsigned long long* __restrict__ key, int n_kp, const long long* __restrict__ lm_id,
                                                     MtRec* __restrict__ rec, int* __restrict__ kp_lm, long long* __restrict__ kp_id,
                                                     int* __restrict__ kp_dist, uint8_t* __restrict__ kp_inl, int* __restrict__ counters) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_kp) return;
  {
    const unsigned long long q = key[k];
    const bool have = q != kNoKey;
    const int row = have ? (int)(q & ((1ull << 40) - 1ull)) : -1;
    kp_lm[k] = row;
    kp_id[k] = have ? (lm_id ? lm_id[row] : (long long)row) : -1ll;
    kp_dist[k] = have ? (int)(q >> 40) : -1;
    kp_inl[k] = 0;
    if (have) { rec[row].kept = 1; atomicAdd(&counters[MC_MATCHES], 1); }
  }
}

// ---------------------------------------------------------------------------------------------------- stage 4
struct MtCorr {   // the correspondences the refinement reads; in gather mode it fills them itself from the search's outputs
  double* X; double* px; int* oct; int* kp;   // kp: the keypoint of pair i (NULL in explicit mode)
  uint8_t* inl;                                // one flag per pair
};
struct MtGather {   // gather = 0: explicit mode
  const int* kp_lm; const float* xyz; const dvs_keypoint* kps; int n_kp, gather;
};

// chi and residual of pair i at (R, t); false (chi = +inf) where the point is not in front of the camera or its octave has no sigma.
// A position that is not finite gives no finite c2 (a row of R times it is never finite), so c2 < inf keeps such a pair out as well.
__device__ __forceinline__ bool mt_residual(const dvs_maptrack_params& P, const double* R, const double* t, const double* X, const double* px, int oct,
                                            double* c, double& ex, double& ey, double& s2, double& chi) {
  if (oct < 0 || oct >= P.n_levels) return false;
#pragma unroll
  for (int i = 0; i < 3; i++) c[i] = ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i];
  if (!(c[2] > 0.0 && c[2] < (double)INFINITY)) return false;
  ex = px[0] - (P.fx * c[0] / c[2] + P.cx);
  ey = px[1] - (P.fy * c[1] / c[2] + P.cy);
  s2 = P.level_sigma2[oct];
  chi = (ex * ex + ey * ey) / s2;
  return true;
}

// the sums over the workgroup into s_tot, in one fixed order: every lane's partial into LDS (a row of kRedStride doubles per sum), then
// lane (a, c) adds lanes c, c + 8, c + 16, ... of sum a in that order, then the eight of a sum are added in order.  The row padding of 8
// doubles keeps the 64 lanes of the second step on distinct banks.
constexpr int kRedStride = kRefThreads + 8;
template <int nacc>
__device__ __forceinline__ void mt_reduce(const double* acc, double* s_red, double (*s_red8)[8], double* s_tot) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int a = 0; a < nacc; a++) s_red[a * kRedStride + tid] = acc[a];
  __syncthreads();
  if (tid < nacc * 8) {
    const int a = tid >> 3, c = tid & 7;
    double v = 0.0;
    for (int i = 0; i < kRefThreads / 8; i++) v += s_red[a * kRedStride + i * 8 + c];
    s_red8[a][c] = v;
  }
  __syncthreads();
  if (tid < nacc) {
    double v = s_red8[tid][0];
    for (int c = 1; c < 8; c++) v += s_red8[tid][c];
    s_tot[tid] = v;
  }
  __syncthreads();
}

// lane 0: H delta = b by Cholesky (s = the 27 sums), the pose update in place; false: a pivot too small or something not finite
__device__ bool mt_solve_update(const double* s, double* R, double* t) {
  double H[36], L[36], b[6], y[6], d[6];
  int q = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) { H[6 * i + j] = s[q]; H[6 * j + i] = s[q]; q++; }
  for (int i = 0; i < 6; i++) b[i] = s[21 + i];
  double maxd = 0.0;
  for (int i = 0; i < 6; i++) { if (!isfinite(H[7 * i])) return false; maxd = fmax(maxd, H[7 * i]); }
  for (int j = 0; j < 6; j++) {
    double p = H[7 * j];
    for (int k = 0; k < j; k++) p -= L[6 * j + k] * L[6 * j + k];
    if (!isfinite(p) || p <= 1e-10 * maxd) return false;
    const double lj = sqrt(p);
    L[7 * j] = lj;
    for (int i = j + 1; i < 6; i++) {
      double v = H[6 * i + j];
      for (int k = 0; k < j; k++) v -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / lj;
    }
  }
  for (int i = 0; i < 6; i++) { double v = b[i]; for (int k = 0; k < i; k++) v -= L[6 * i + k] * y[k]; y[i] = v / L[7 * i]; }
  for (int i = 5; i >= 0; i--) { double v = y[i]; for (int k = i + 1; k < 6; k++) v -= L[6 * k + i] * d[k]; d[i] = v / L[7 * i]; }
  for (int i = 0; i < 6; i++) if (!isfinite(d[i])) return false;
  // Exp(omega)
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double E[9];
  if (th < 1e-12) {
    for (int k = 0; k < 9; k++) E[k] = (k % 4 == 0 ? 1.0 : 0.0) + K[k];
  } else {
    const double A = sin(th) / th, B = (1.0 - cos(th)) / th2;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
        E[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * k2;
      }
  }
  double Rn[9], tn[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) Rn[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
    tn[i] = ((E[3 * i] * t[0] + E[3 * i + 1] * t[1]) + E[3 * i + 2] * t[2]) + d[3 + i];
  }
  for (int k = 0; k < 9; k++) { if (!isfinite(Rn[k])) return false; R[k] = Rn[k]; }
  for (int k = 0; k < 3; k++) { if (!isfinite(tn[k])) return false; t[k] = tn[k]; }
  return true;
}

// rounds first_round .. first_round + n_rounds - 1 of n_iters steps each; round r is robust iff r < 2.  The product's schedule is 0, 4, 10:
// kAnySchedule = false compiles those in (reading them cost a track call 3 - 5 %: EXPERIMENTS.md "Map tracking"), true takes the arguments
template <bool kAnySchedule>
__global__ __launch_bounds__(kRefThreads) void k_mt_refine(dvs_maptrack_params P, MtPose T, MtGather G, MtCorr C, int n_explicit, uint8_t* kp_inl,
                                                           int* kp_lm_out, long long* kp_id_out, int* kp_dist_out, const int* counters,
                                                           int first_round_arg, int n_rounds_arg, int n_iters_arg, dvs_maptrack_result* out) {
  const int first_round = kAnySchedule ? first_round_arg : 0, n_rounds = kAnySchedule ? n_rounds_arg : 4, n_iters = kAnySchedule ? n_iters_arg : 10;
  __shared__ double s_red[27 * kRedStride];
  __shared__ double s_red8[kSums][8];
  __shared__ double s_tot[kSums];
  __shared__ double s_R[9], s_t[3];
  __shared__ int s_w[4];
  __shared__ int s_ok, s_nin;
  const int tid = threadIdx.x;
  int n = 0;
  if (G.gather) {   // the kept pairs in keypoint order
    for (int k0 = 0; k0 < G.n_kp; k0 += kRefThreads) {
      const int k = k0 + tid;
      const int row = k < G.n_kp ? G.kp_lm[k] : -1;
      int total;
      const int pos = n + block_rank256(row >= 0, s_w, total);
      if (row >= 0) {
        for (int a = 0; a < 3; a++) C.X[3 * (size_t)pos + a] = (double)G.xyz[3 * (size_t)row + a];
        C.px[2 * (size_t)pos] = (double)G.kps[k].x; C.px[2 * (size_t)pos + 1] = (double)G.kps[k].y;
        C.oct[pos] = G.kps[k].octave;
        C.kp[pos] = k;
      }
      n += total;
    }
    __threadfence_block();
  } else {
    n = n_explicit;
    for (int i = tid; i < n; i += kRefThreads) { kp_lm_out[i] = i; kp_id_out[i] = i; kp_dist_out[i] = 0; }
  }
  if (tid < 9) s_R[tid] = T.Rcw[tid];
  if (tid < 3) s_t[tid] = T.tcw[tid];
  if (tid == 0) { s_ok = 1; s_nin = 0; }
  for (int i = tid; i < n; i += kRefThreads) C.inl[i] = 1;
  __syncthreads();
  int status = DVS_MAPTRACK_OK;
  double cost = 0.0;
  if (n < P.min_matches) {
    status = DVS_MAPTRACK_FEW_MATCHES;
  } else {
    for (int round = first_round; round < first_round + n_rounds && status == DVS_MAPTRACK_OK; round++) {
      const bool robust = round < 2;
      for (int it = 0; it < n_iters; it++) {
        double R[9], t[3], acc[kSums];
        for (int k = 0; k < 9; k++) R[k] = s_R[k];
        for (int k = 0; k < 3; k++) t[k] = s_t[k];
        for (int a = 0; a < kSums; a++) acc[a] = 0.0;
        for (int i = tid; i < n; i += kRefThreads) {
          if (!C.inl[i]) continue;
          double c[3], ex, ey, s2, chi;
          if (!mt_residual(P, R, t, C.X + 3 * (size_t)i, C.px + 2 * (size_t)i, C.oct[i], c, ex, ey, s2, chi)) continue;
          const double w = (robust && chi > P.chi2_gate) ? sqrt(P.chi2_gate / chi) : 1.0;
          const double ws = w / s2, iz = 1.0 / c[2];
          const double a = P.fx * iz, b = P.fy * iz, a2 = -(a * c[0]) * iz, b2 = -(b * c[1]) * iz;   // d(u, v) / dc = [a 0 a2; 0 b b2]
          const double Ju[6] = {a2 * c[1], a * c[2] - a2 * c[0], -(a * c[1]), a, 0.0, a2};
          const double Jv[6] = {b2 * c[1] - b * c[2], -(b2 * c[0]), b * c[0], 0.0, b, b2};
          int q = 0;
#pragma unroll
          for (int r = 0; r < 6; r++)
#pragma unroll
            for (int s = r; s < 6; s++) acc[q++] += ws * (Ju[r] * Ju[s] + Jv[r] * Jv[s]);
#pragma unroll
          for (int r = 0; r < 6; r++) acc[21 + r] += ws * (Ju[r] * ex + Jv[r] * ey);
        }
        mt_reduce<27>(acc, s_red, s_red8, s_tot);
        if (tid == 0 && !mt_solve_update(s_tot, s_R, s_t)) s_ok = 0;
        __syncthreads();
        if (!s_ok) { status = DVS_MAPTRACK_DEGENERATE; break; }
      }
      if (status != DVS_MAPTRACK_OK) break;
      // reclassify every pair at the round's last pose; the cost over the new inliers
      double R[9], t[3], acc[1] = {0.0};
      for (int k = 0; k < 9; k++) R[k] = s_R[k];
      for (int k = 0; k < 3; k++) t[k] = s_t[k];
      if (tid == 0) s_nin = 0;
      __syncthreads();
      int mine = 0;
      for (int i = tid; i < n; i += kRefThreads) {
        double c[3], ex, ey, s2, chi;
        const bool in = mt_residual(P, R, t, C.X + 3 * (size_t)i, C.px + 2 * (size_t)i, C.oct[i], c, ex, ey, s2, chi) && chi <= P.chi2_gate;
        C.inl[i] = in ? 1 : 0;
        if (in) { acc[0] += chi; mine++; }
      }
      if (mine) atomicAdd(&s_nin, mine);
      mt_reduce<1>(acc, s_red, s_red8, s_tot);   // its barriers also publish s_nin and the flags
      cost = s_tot[0];
      if (!isfinite(cost)) status = DVS_MAPTRACK_DEGENERATE;
    }
    if (status == DVS_MAPTRACK_OK && s_nin < P.min_inliers) status = DVS_MAPTRACK_FEW_INLIERS;
  }
  __syncthreads();
  const bool flags = status == DVS_MAPTRACK_OK || status == DVS_MAPTRACK_FEW_INLIERS;
  for (int i = tid; i < n; i += kRefThreads) {
    const uint8_t f = flags ? C.inl[i] : 0;
    C.inl[i] = f;
    if (G.gather) kp_inl[C.kp[i]] = f; else kp_inl[i] = f;
  }
  if (tid == 0) {
    dvs_maptrack_result r;
    if (status == DVS_MAPTRACK_OK) {
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r.R[3 * i + j] = s_R[3 * j + i];
        r.t[i] = -((s_R[i] * s_t[0] + s_R[3 + i] * s_t[1]) + s_R[6 + i] * s_t[2]);
      }
    } else {
      for (int k = 0; k < 9; k++) r.R[k] = T.R[k];
      for (int k = 0; k < 3; k++) r.t[k] = T.t[k];
    }
    r.cost = flags ? cost : 0.0;
    r.status = status;
    r.n_visible = counters ? counters[MC_VISIBLE] : 0; r.n_proposed = counters ? counters[MC_PROPOSED] : 0;
    r.n_unbinned = counters ? counters[MC_UNBINNED] : 0;
    r.n_matches = n;
    r.n_inliers = flags ? s_nin : 0;
    *out = r;
  }
}

// the record of a search on its own: the prior and the counts
__global__ void k_mt_search_record(MtPose T, const int* counters, dvs_maptrack_result* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  dvs_maptrack_result r;
  for (int k = 0; k < 9; k++) r.R[k] = T.R[k];
  for (int k = 0; k < 3; k++) r.t[k] = T.t[k];
  r.cost = 0.0; r.status = DVS_MAPTRACK_OK;
  r.n_visible = counters[MC_VISIBLE]; r.n_proposed = counters[MC_PROPOSED]; r.n_matches = counters[MC_MATCHES]; r.n_inliers = 0;
  r.n_unbinned = counters[MC_UNBINNED];
  *out = r;
}

// "Landmark culling" in the header, the recording: thread j owns row j of the arrays the call handed to the tracker and the statistics row
// of that row's id, which no other thread writes (the ids of a call are distinct).  Nothing changes unless the device record says OK.
__global__ __launch_bounds__(256) void k_mt_record_stats(const MtRec* __restrict__ rec, const i64* __restrict__ id, int n, const uint8_t* __restrict__ kp_inl, int n_kp,
                                                         const dvs_maptrack_result* __restrict__ res, StatView st, int nstat) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n || res->status != DVS_MAPTRACK_OK) return;
  if (rec[j].visible == 0) return;
  const int s = lm_find(st.id, nstat, id[j]);
  if (s < 0) return;
  const int v = st.visible[s];
  if (v == 0x7fffffff) return;
  st.visible[s] = v + 1;
  const int k = rec[j].best_k;
  if (rec[j].kept != 0 && k >= 0 && k < n_kp && kp_inl[k] != 0) st.found[s] += 1;
}

static dvs_status maptrack_check_params(const dvs_maptrack_params& P) {
  DVS_ARG(P.rows >= 1 && P.rows <= 16384 && P.cols >= 1 && P.cols <= 16384);
  DVS_ARG(__builtin_isfinite(P.fx) && __builtin_isfinite(P.fy) && __builtin_isfinite(P.cx) && __builtin_isfinite(P.cy) && P.fx > 0 && P.fy > 0);
  DVS_ARG(__builtin_isfinite(P.min_z) && __builtin_isfinite(P.max_z) && P.min_z >= 0 && P.min_z < P.max_z);
  DVS_ARG(__builtin_isfinite(P.radius) && P.radius >= 0);
  DVS_ARG(P.cell >= 1 && P.cell <= 16384);
  DVS_ARG((long long)((P.cols + P.cell - 1) / P.cell) * ((P.rows + P.cell - 1) / P.cell) <= (1ll << 20));
  DVS_ARG(P.max_hamming >= 0 && P.max_hamming <= 257 && P.ratio_pct <= 100000);
  DVS_ARG(__builtin_isfinite(P.chi2_gate) && P.chi2_gate > 0);
  DVS_ARG(P.min_matches >= 3 && P.min_inliers >= 0);
  DVS_ARG(P.n_levels >= 1 && P.n_levels <= DVS_MAPTRACK_MAX_LEVELS);
  for (int k = 0; k < P.n_levels; k++) DVS_ARG(__builtin_isfinite(P.level_sigma2[k]) && P.level_sigma2[k] > 0);
  return DVS_OK;
}

static dvs_status maptrack_pose(const double* R9, const double* t3, MtPose* T) {
  DVS_ARG(R9 && t3);
  for (int k = 0; k < 9; k++) DVS_ARG(__builtin_isfinite(R9[k]));
  for (int k = 0; k < 3; k++) DVS_ARG(__builtin_isfinite(t3[k]));
  memcpy(T->R, R9, sizeof(T->R)); memcpy(T->t, t3, sizeof(T->t));
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T->Rcw[3 * i + j] = R9[3 * j + i];
    T->tcw[i] = -((R9[i] * t3[0] + R9[3 + i] * t3[1]) + R9[6 + i] * t3[2]);
  }
  return DVS_OK;
}

}  // namespace dvs

using namespace dvs;

struct dvs_maptrack {
  dvs_maptrack_params P;
  int device = 0;
  hipStream_t stream = nullptr;
  int gw = 0, gh = 0, ncell = 0;
  // per cell: [cnt ncell | fill ncell | counters MC_INTS] cleared by one memset per call, and the CSR row starts
  DeviceBuf<int> cells, start;
  // per keypoint (grow-only)
  Column<int> cellid, arrival, order, kp_lm, kp_dist; Column<long long> kp_id; Column<unsigned long long> key; Column<uint8_t> kp_inl;
  size_t c_kp = 0;
  // per landmark (grow-only)
  DeviceBuf<MtRec> rec;
  size_t c_lm = 0;
  // the correspondences of the refinement (grow-only)
  Column<double, 3> cX; Column<double, 2> cpx; Column<int> coct, ckp; Column<uint8_t> cinl;
  size_t c_corr = 0;
  DeviceBuf<dvs_maptrack_result> d_res;
  FrameStaging stage;   // of the host form
  // the last call
  int last_n_kp = 0, last_n_lm = 0;
  bool last_search = false;
};

namespace dvs {   // maptrack_internal.h
const dvs_maptrack_params& maptrack_params(const dvs_maptrack* h) { return h->P; }
int maptrack_device(const dvs_maptrack* h) { return h->device; }
}  // namespace dvs

static int* mt_cnt(dvs_maptrack* h) { return h->cells.get(); }
static int* mt_fill(dvs_maptrack* h) { return h->cells.get() + h->ncell; }
static int* mt_counters(dvs_maptrack* h) { return h->cells.get() + 2 * (size_t)h->ncell; }

static dvs_status mt_grow_kp(dvs_maptrack* h, size_t n) {
  return grow_rows(h->c_kp, n, n + n / 4, h->cellid, h->arrival, h->order, h->kp_lm, h->kp_dist, h->kp_id, h->key, h->kp_inl);
}
static dvs_status mt_grow_corr(dvs_maptrack* h, size_t n) { return grow_rows(h->c_corr, n, n + n / 4, h->cX, h->cpx, h->coct, h->ckp, h->cinl); }

static dvs_status mt_check_search_args(const dvs_maptrack* h, const void* xyz, const void* ldesc, int n_lm, const void* kps, const void* kdesc, int n_kp) {
  DVS_ARG(h && n_lm >= 0 && n_kp >= 0 && n_lm <= (1 << 30) && n_kp <= (1 << 30));
  DVS_ARG(n_lm == 0 || (xyz && ldesc));
  DVS_ARG(n_kp == 0 || (kps && kdesc));
  DVS_ARG(((uintptr_t)ldesc & 7) == 0 && ((uintptr_t)kdesc & 7) == 0 && ((uintptr_t)xyz & 3) == 0 && ((uintptr_t)kps & 3) == 0);
  return DVS_OK;
}

// stages 1-3, enqueued; arguments checked by the caller
static dvs_status mt_search(dvs_maptrack* h, const MtPose& T, const MtGateArgs* gate, const float* d_xyz, const uint8_t* d_ldesc, const int64_t* d_id, int n_lm, const dvs_keypoint* d_kps,
                            const uint8_t* d_kdesc, int n_kp) {
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  h->last_n_kp = 0; h->last_n_lm = 0; h->last_search = false;
  if ((size_t)n_kp > h->c_kp || (size_t)n_lm > h->c_lm) DVS_HIP(hipStreamSynchronize(st));   // nothing in flight reads what is freed
  DVS_TRY(mt_grow_kp(h, (size_t)n_kp));
  DVS_TRY(grow(h->rec, h->c_lm, (size_t)n_lm));
  const dvs_maptrack_params& P = h->P;
  DVS_HIP(hipMemsetAsync(h->cells.get(), 0, (2 * (size_t)h->ncell + MC_INTS) * sizeof(int), st));
  const unsigned gk = (unsigned)((n_kp + 255) / 256), gl = (unsigned)((n_lm + 255) / 256);
  if (n_kp > 0)
    hipLaunchKernelGGL(k_mt_cells, dim3(gk), dim3(256), 0, st, d_kps, n_kp, P.rows, P.cols, P.cell, h->gw, P.n_levels, h->cellid.get(), mt_cnt(h), h->key.get(),
                       mt_counters(h));
  hipLaunchKernelGGL(k_mt_scan, dim3(1), dim3(256), 0, st, (const int*)mt_cnt(h), h->ncell, h->start.get());
  if (n_kp > 0) {
    hipLaunchKernelGGL(k_mt_scatter, dim3(gk), dim3(256), 0, st, (const int*)h->cellid.get(), n_kp, (const int*)h->start.get(), mt_fill(h), h->arrival.get());
    hipLaunchKernelGGL(k_mt_order, dim3(gk), dim3(256), 0, st, (const int*)h->cellid.get(), (const int*)h->arrival.get(), (const int*)h->start.get(), h->ncell,
                       h->order.get());
  }
  if (n_lm > 0 && gate)
    hipLaunchKernelGGL(k_mt_search<true>, dim3(gl), dim3(256), 0, st, P, T, *gate, d_xyz, d_ldesc, n_lm, d_kps, d_kdesc, (const int*)h->start.get(),
                       (const int*)h->order.get(), h->gw, h->gh, h->rec.get(), h->key.get(), mt_counters(h));
  else if (n_lm > 0)
    hipLaunchKernelGGL(k_mt_search<false>, dim3(gl), dim3(256), 0, st, P, T, MtGateArgs{nullptr, nullptr, nullptr, 0.0, 0.0}, d_xyz, d_ldesc, n_lm, d_kps, d_kdesc,
                       (const int*)h->start.get(), (const int*)h->order.get(), h->gw, h->gh, h->rec.get(), h->key.get(), mt_counters(h));
  if (n_kp > 0)
    hipLaunchKernelGGL(k_mt_finalize, dim3(gk), dim3(256), 0, st, (const unsigned long long*)h->key.get(), n_kp, (const long long*)d_id, h->rec.get(),
                       h->kp_lm.get(), h->kp_id.get(), h->kp_dist.get(), h->kp_inl.get(), mt_counters(h));
  DVS_HIP(hipGetLastError());
  h->last_n_kp = n_kp; h->last_n_lm = n_lm; h->last_search = true;
  return DVS_OK;
}

static dvs_status mt_read_result(dvs_maptrack* h, dvs_maptrack_result* result) {
  DVS_HIP(hipMemcpyAsync(result, h->d_res.get(), sizeof(*result), hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  return DVS_OK;
}

// stage 4 on explicit correspondences with a schedule: dvs_maptrack_refine_device's launch (0, 4, 10) and the test hook's
static dvs_status mt_refine_explicit(dvs_maptrack* h, const double* d_X, const double* d_px, const int32_t* d_octave, int32_t n, const double* R9,
                                     const double* t3, bool any_schedule, int first_round, int n_rounds, int n_iters, dvs_maptrack_result* result) {
  DVS_ARG(h && result && n >= 0 && n <= (1 << 30) && (n == 0 || (d_X && d_px && d_octave)));
  DVS_ARG(((uintptr_t)d_X & 7) == 0 && ((uintptr_t)d_px & 7) == 0 && ((uintptr_t)d_octave & 3) == 0);
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  h->last_n_kp = 0; h->last_n_lm = 0; h->last_search = false;
  if ((size_t)n > h->c_kp || (size_t)n > h->c_corr) DVS_HIP(hipStreamSynchronize(st));
  DVS_TRY(mt_grow_kp(h, (size_t)n));
  DVS_TRY(mt_grow_corr(h, (size_t)n));
  MtGather G; G.kp_lm = nullptr; G.xyz = nullptr; G.kps = nullptr; G.n_kp = 0; G.gather = 0;
  MtCorr C; C.X = const_cast<double*>(d_X); C.px = const_cast<double*>(d_px); C.oct = const_cast<int*>(d_octave); C.kp = nullptr; C.inl = h->cinl.get();
#ifdef DVS_TEST_HOOKS
  if (any_schedule)
    hipLaunchKernelGGL(k_mt_refine<true>, dim3(1), dim3(kRefThreads), 0, st, h->P, T, G, C, n, h->kp_inl.get(), h->kp_lm.get(), h->kp_id.get(), h->kp_dist.get(),
                       (const int*)nullptr, first_round, n_rounds, n_iters, h->d_res.get());
  else
#endif
    hipLaunchKernelGGL(k_mt_refine<false>, dim3(1), dim3(kRefThreads), 0, st, h->P, T, G, C, n, h->kp_inl.get(), h->kp_lm.get(), h->kp_id.get(), h->kp_dist.get(),
                       (const int*)nullptr, 0, 4, 10, h->d_res.get());
  (void)any_schedule; (void)first_round; (void)n_rounds; (void)n_iters;
  DVS_HIP(hipGetLastError());
  h->last_n_kp = n;
  return mt_read_result(h, result);
}

// the gated calls' extra arguments ("Landmark refresh" in the header): ranges checked, the constants formed once
static dvs_status mt_gate_args(const dvs_maptrack_gates* gates, const double* d_normal, const double* d_range, const int32_t* d_ncnt, int n_lm, MtGateArgs* g) {
  dvs_maptrack_gates G;
  if (gates) G = *gates; else dvs_mapgate_default_gates(&G);
  DVS_ARG(G.cos_min >= 0.0 && G.cos_min <= 1.0 && __builtin_isfinite(G.range_factor) && G.range_factor >= 1.0);
  DVS_ARG(n_lm <= 0 || (d_normal && d_range && d_ncnt));
  DVS_ARG(((uintptr_t)d_normal & 7) == 0 && ((uintptr_t)d_range & 7) == 0 && ((uintptr_t)d_ncnt & 3) == 0);
  g->normal = d_normal; g->range = d_range; g->ncnt = d_ncnt; g->range_factor = G.range_factor; g->cc = G.cos_min * G.cos_min;
  return DVS_OK;
}
// the bodies the ungated and the gated entry points share (gate NULL: ungated)
static dvs_status mt_search_call(dvs_maptrack* h, const MtGateArgs* gate, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                 const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result);
static dvs_status mt_track_call(dvs_maptrack* h, const MtGateArgs* gate, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result);

// the end of the three dvs_backend_track_frame* calls ("Landmark culling" in the header): with the switch off nothing is launched or waited
// for.  d_id / n: the rows the call handed to the tracker, whose records, flags and device record mt still holds; mt's stream has been
// synchronised by the read of the result, so the backend's stream may read them.
static dvs_status mt_record_stats(dvs_backend* h, dvs_maptrack* mt, const i64* d_id, int n, const dvs_maptrack_result* result) {
  if (!h->stats_on) return DVS_OK;
  DVS_TRY(dvs::lm_stats_align(h));
  hipStream_t st = h->ctx->stream;
  if (n > 0 && h->nstat > 0 && mt->last_search && mt->last_n_lm == n)
    hipLaunchKernelGGL(k_mt_record_stats, dim3((n + 255) / 256), dim3(256), 0, st, (const MtRec*)mt->rec.get(), d_id, n, (const uint8_t*)mt->kp_inl.get(), mt->last_n_kp,
                       (const dvs_maptrack_result*)mt->d_res.get(), stat_view(h->stat), h->nstat);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipStreamSynchronize(st));
  if (result->status == DVS_MAPTRACK_OK) h->n_recorded++;
  return DVS_OK;
}

extern "C" {

void dvs_mapgate_default_gates(dvs_maptrack_gates* g) {
  if (!g) return;
  g->cos_min = 0.5; g->range_factor = 2.0;
}

void dvs_maptrack_default_params(dvs_maptrack_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_z = 0.05; p->max_z = 20.0;
  p->radius = 15.0; p->cell = 32; p->max_hamming = 50; p->ratio_pct = 90;
  p->chi2_gate = 5.991; p->min_matches = 15; p->min_inliers = 10;
  p->n_levels = 8;
  float scale = 1.0f;                                  // the extractor's table (orb.hip): scale in float, the factor widened
  for (int i = 0; i < 8; i++) {
    if (i > 0) scale = (float)(scale * (double)1.2f);
    p->level_sigma2[i] = (double)(scale * scale);
  }
}

dvs_status dvs_maptrack_create(const dvs_maptrack_params* params, int32_t device, dvs_maptrack** out) {
  DVS_ARG(params && out);
  *out = nullptr;
  DVS_TRY(maptrack_check_params(*params));
  DVS_TRY(check_device(device));
  dvs_maptrack* h = new (std::nothrow) dvs_maptrack();
  if (!h) { set_error("dvs_maptrack_create: out of memory"); return DVS_ERR_HIP; }
  h->P = *params; h->device = device;
  h->gw = (h->P.cols + h->P.cell - 1) / h->P.cell; h->gh = (h->P.rows + h->P.cell - 1) / h->P.cell; h->ncell = h->gw * h->gh;
  auto alloc_all = [&]() -> dvs_status {
    DVS_TRY(h->cells.alloc(2 * (size_t)h->ncell + MC_INTS)); DVS_TRY(h->start.alloc((size_t)h->ncell + 1)); DVS_TRY(h->d_res.alloc(1));
    DVS_HIP(hipMemset(h->start.get(), 0, ((size_t)h->ncell + 1) * sizeof(int)));
    DVS_HIP(hipMemset(h->d_res.get(), 0, sizeof(dvs_maptrack_result)));
    return DVS_OK;
  };
  const dvs_status s = alloc_all();
  if (s != DVS_OK) { dvs_maptrack_destroy(h); return s; }
  *out = h;
  return DVS_OK;
}

void dvs_maptrack_destroy(dvs_maptrack* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;
}

dvs_status dvs_maptrack_set_stream(dvs_maptrack* h, void* hip_stream) {
  DVS_ARG(h);
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->stream));
  h->stream = (hipStream_t)hip_stream;
  return DVS_OK;
}

dvs_status dvs_maptrack_search_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                      const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3,
                                      dvs_maptrack_result* result) {
  return mt_search_call(h, nullptr, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, R9, t3, result);
}

dvs_status dvs_mapgate_search_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                     const double* d_lm_normal, const double* d_lm_range, const int32_t* d_lm_ncounted,
                                     const dvs_maptrack_gates* gates, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp,
                                     const double* R9, const double* t3, dvs_maptrack_result* result) {
  MtGateArgs g;
  DVS_TRY(mt_gate_args(gates, d_lm_normal, d_lm_range, d_lm_ncounted, n_lm, &g));
  return mt_search_call(h, &g, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, R9, t3, result);
}

static dvs_status mt_search_call(dvs_maptrack* h, const MtGateArgs* gate, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                 const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result) {
  DVS_TRY(mt_check_search_args(h, d_lm_xyz, d_lm_desc, n_lm, d_kps, d_desc, n_kp));
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  DVS_TRY(mt_search(h, T, gate, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp));
  if (!result) return DVS_OK;
  hipLaunchKernelGGL(k_mt_search_record, dim3(1), dim3(64), 0, h->stream, T, (const int*)mt_counters(h), h->d_res.get());
  DVS_HIP(hipGetLastError());
  return mt_read_result(h, result);
}

dvs_status dvs_maptrack_refine_device(dvs_maptrack* h, const double* d_X, const double* d_px, const int32_t* d_octave, int32_t n, const double* R9,
                                      const double* t3, dvs_maptrack_result* result) {
  return mt_refine_explicit(h, d_X, d_px, d_octave, n, R9, t3, false, 0, 4, 10, result);
}

dvs_status dvs_maptrack_track_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                     const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3,
                                     dvs_maptrack_result* result) {
  return mt_track_call(h, nullptr, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, R9, t3, result);
}

dvs_status dvs_mapgate_track_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                    const double* d_lm_normal, const double* d_lm_range, const int32_t* d_lm_ncounted,
                                    const dvs_maptrack_gates* gates, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp,
                                    const double* R9, const double* t3, dvs_maptrack_result* result) {
  MtGateArgs g;
  DVS_TRY(mt_gate_args(gates, d_lm_normal, d_lm_range, d_lm_ncounted, n_lm, &g));
  return mt_track_call(h, &g, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, R9, t3, result);
}

dvs_status dvs_mapgate_get_counts(dvs_maptrack* h, int32_t out[4]) {
  DVS_ARG(h && out);
  memset(out, 0, 4 * sizeof(int32_t));
  if (!h->last_search) return DVS_OK;                  // the counters are those of a search
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipMemcpyAsync(out, mt_counters(h) + MC_GATE, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  return DVS_OK;
}

static dvs_status mt_track_call(dvs_maptrack* h, const MtGateArgs* gate, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result) {
  DVS_TRY(mt_check_search_args(h, d_lm_xyz, d_lm_desc, n_lm, d_kps, d_desc, n_kp));
  DVS_ARG(result);
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  DVS_HIP(hipSetDevice(h->device));
  if ((size_t)n_kp > h->c_corr) DVS_HIP(hipStreamSynchronize(h->stream));
  DVS_TRY(mt_grow_corr(h, (size_t)n_kp));   // a keypoint keeps at most one landmark
  DVS_TRY(mt_search(h, T, gate, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp));
  MtGather G; G.kp_lm = h->kp_lm.get(); G.xyz = d_lm_xyz; G.kps = d_kps; G.n_kp = n_kp; G.gather = 1;
  MtCorr C; C.X = h->cX.get(); C.px = h->cpx.get(); C.oct = h->coct.get(); C.kp = h->ckp.get(); C.inl = h->cinl.get();
  hipLaunchKernelGGL(k_mt_refine<false>, dim3(1), dim3(kRefThreads), 0, h->stream, h->P, T, G, C, 0, h->kp_inl.get(), h->kp_lm.get(), h->kp_id.get(), h->kp_dist.get(),
                     (const int*)mt_counters(h), 0, 4, 10, h->d_res.get());
  DVS_HIP(hipGetLastError());
  return mt_read_result(h, result);
}

dvs_status dvs_maptrack_track(dvs_maptrack* h, const float* lm_xyz, const uint8_t* lm_desc, const int64_t* lm_id, int32_t n_lm, const dvs_keypoint* kps,
                              const uint8_t* desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result) {
  DVS_ARG(h && result && n_lm >= 0 && n_kp >= 0 && n_lm <= (1 << 30) && n_kp <= (1 << 30));
  DVS_ARG((n_lm == 0 || (lm_xyz && lm_desc)) && (n_kp == 0 || (kps && desc)));
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  DVS_TRY(stage_frame(h->stage, h->P, h->device, h->stream, lm_xyz, lm_desc, lm_id, n_lm, kps, desc, n_kp));
  const FrameStaging& S = h->stage;
  return dvs_maptrack_track_device(h, S.xyz.get(), S.ldesc.get(), S.ids(lm_id, n_lm), n_lm, S.kps.get(), S.kdesc.get(), n_kp, R9, t3, result);
}

dvs_status dvs_maptrack_get_matches(dvs_maptrack* h, int32_t cap, int32_t* lm_row, int64_t* lm_id, int32_t* dist, uint8_t* inlier, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->last_n_kp;
  if (h->last_n_kp > cap && (lm_row || lm_id || dist || inlier)) {
    set_error("dvs_maptrack_get_matches: %d rows, capacity %d", h->last_n_kp, cap);
    return DVS_ERR_CAPACITY;
  }
  if (h->last_n_kp == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t m = (size_t)h->last_n_kp;
  DVS_TRY(copy_out(lm_row, h->kp_lm, m, st)); DVS_TRY(copy_out(lm_id, h->kp_id, m, st));
  DVS_TRY(copy_out(dist, h->kp_dist, m, st)); DVS_TRY(copy_out(inlier, h->kp_inl, m, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_backend_track_frame(dvs_backend* h, dvs_maptrack* mt, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9,
                                   const double* t3, dvs_maptrack_result* result) {
  DVS_ARG(h && mt && result && h->device == mt->device);
  DVS_TRY(mt_check_search_args(mt, h->lm.xyz.get(), h->lm.desc.get(), h->nlm, d_kps, d_desc, n_kp));
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));   // the table as the backend's last call left it
  DVS_TRY(dvs_maptrack_track_device(mt, h->lm.xyz.get(), h->lm.desc.get(), (const int64_t*)h->lm.id.get(), h->nlm, d_kps, d_desc, n_kp, R9, t3, result));
  return mt_record_stats(h, mt, h->lm.id.get(), h->nlm, result);
}

// the same with the gates of "Landmark refresh": landmark_refresh.hip computes the geometry of the table as it stands into the backend's scratch
dvs_status dvs_backend_track_frame_gated(dvs_backend* h, dvs_maptrack* mt, const dvs_maptrack_gates* gates, const dvs_keypoint* d_kps, const uint8_t* d_desc,
                                         int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result) {
  DVS_ARG(h && mt && result && h->device == mt->device);
  DVS_TRY(mt_check_search_args(mt, h->lm.xyz.get(), h->lm.desc.get(), h->nlm, d_kps, d_desc, n_kp));
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  MtGateArgs g;
  DVS_TRY(mt_gate_args(gates, nullptr, nullptr, nullptr, 0, &g));
  DVS_HIP(hipSetDevice(h->device));
  if (h->nlm > 0) DVS_TRY(dvs::refresh_geometry(h));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));   // the table as the backend's last call left it, and its geometry
  g.normal = h->lr_lm.normal.get(); g.range = h->lr_lm.range.get(); g.ncnt = h->lr_lm.ncnt.get();
  DVS_TRY(mt_track_call(mt, &g, h->lm.xyz.get(), h->lm.desc.get(), (const int64_t*)h->lm.id.get(), h->nlm, d_kps, d_desc, n_kp, R9, t3, result));
  return mt_record_stats(h, mt, h->lm.id.get(), h->nlm, result);
}

// the same against the local map of one keyframe ("Covisibility" in the header): covisibility.hip compacts U's columns on the device
dvs_status dvs_backend_track_frame_local(dvs_backend* h, dvs_maptrack* mt, uint64_t ref_frame_id, const dvs_covis_params* params, const dvs_keypoint* d_kps,
                                         const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result) {
  DVS_ARG(h && mt && result && h->device == mt->device);
  DVS_TRY(mt_check_search_args(mt, h->lm.xyz.get(), h->lm.desc.get(), h->nlm, d_kps, d_desc, n_kp));
  MtPose T;
  DVS_TRY(maptrack_pose(R9, t3, &T));
  const float* xyz = nullptr; const uint8_t* desc = nullptr; const dvs::i64* id = nullptr;
  int n = 0;
  DVS_TRY(dvs::backend_local_map(h, ref_frame_id, params, &xyz, &desc, &id, &n));   // returns with the backend's stream synchronised
  DVS_TRY(dvs_maptrack_track_device(mt, xyz, desc, (const int64_t*)id, n, d_kps, d_desc, n_kp, R9, t3, result));
  return mt_record_stats(h, mt, id, n, result);   // U's ids are scratch of the backend, valid until its next call: the alignment leaves them alone
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test_maptrack.h)
dvs_status dvs_test_maptrack_landmarks(dvs_maptrack* h, int32_t cap, dvs_maptrack_lm_record* rec, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->last_search ? h->last_n_lm : 0;
  if (!rec || *n == 0) return DVS_OK;
  if (*n > cap) { set_error("dvs_test_maptrack_landmarks: %d rows, capacity %d", *n, cap); return DVS_ERR_CAPACITY; }
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipMemcpyAsync(rec, h->rec.get(), (size_t)*n * sizeof(MtRec), hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  return DVS_OK;
}

dvs_status dvs_test_maptrack_cells(dvs_maptrack* h, int32_t cap_cells, int32_t cap_kp, int32_t* cell_start, int32_t* order, int32_t* n_cells,
                                   int32_t* n_binned) {
  DVS_ARG(h && n_cells && n_binned && cap_cells >= 0 && cap_kp >= 0);
  *n_cells = h->ncell; *n_binned = 0;
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->stream));
  int nb = 0;
  if (h->last_search) DVS_HIP(hipMemcpy(&nb, h->start.get() + h->ncell, 4, hipMemcpyDeviceToHost));
  *n_binned = nb;
  if ((cell_start && h->ncell > cap_cells) || (order && nb > cap_kp)) { set_error("dvs_test_maptrack_cells: %d cells, %d keypoints", h->ncell, nb); return DVS_ERR_CAPACITY; }
  if (cell_start) {
    if (h->last_search) DVS_HIP(hipMemcpy(cell_start, h->start.get(), ((size_t)h->ncell + 1) * sizeof(int), hipMemcpyDeviceToHost));
    else memset(cell_start, 0, ((size_t)h->ncell + 1) * sizeof(int));
  }
  if (order && nb > 0) DVS_HIP(hipMemcpy(order, h->order.get(), (size_t)nb * h->order.row_bytes, hipMemcpyDeviceToHost));
  return DVS_OK;
}

dvs_status dvs_test_maptrack_refine_steps(dvs_maptrack* h, const double* d_X, const double* d_px, const int32_t* d_octave, int32_t n, const double* R9,
                                          const double* t3, int32_t first_round, int32_t n_rounds, int32_t n_iters, dvs_maptrack_result* result) {
  DVS_ARG(first_round >= 0 && n_rounds >= 1 && first_round <= 4 && n_rounds <= 4 && first_round + n_rounds <= 4 && n_iters >= 1 && n_iters <= 10);
  return mt_refine_explicit(h, d_X, d_px, d_octave, n, R9, t3, true, first_round, n_rounds, n_iters, result);
}
#endif

}  // extern "C"
