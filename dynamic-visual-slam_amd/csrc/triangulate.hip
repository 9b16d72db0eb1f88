// triangulate.hip — LandmarkInfo::triangulate (backend.cpp:439-613) for a batch of landmarks, one thread per landmark, FP64.
//
// What one thread computes (the reference's steps, in its own operation order; tests/triangulate_ref.py restates them in numpy and
// the GPU tests compare bit for bit):
//   views      the landmark's views in observation order, skipping view_kf < 0 (the reference's failed find_if); V = their number
//   P, C       P = K [R | t] as OpenCV's small GEMM sums it (K's zeros add exact zeros), C = -(R^T t)
//   gate       max over view pairs of atan2(|Ci - Cj|, (|X - Ci| + |X - Cj|) / 2) against 0.0175 * 5 (X: the float position)
//   A, SVD     A = 2V x 4 rows u P2 - P0, v P2 - P1; OpenCV 4.x JacobiSVDImpl_<double> on At = A^T (one-sided Jacobi, row-major
//              pair sweeps, eps = 10 DBL_EPSILON, max(m, 30) sweeps, selection sort of the singular values); the null vector is the
//              sorted Vt's row 3
//   dehom.     V == 2: cv::triangulatePoints' CV_32F output, divided in float; V >= 3: divided in double, then rounded to float
//   checks     mean reprojection error over the views in front of the camera > 2 px rejects (none in front: accepted — the
//              reference's quirk); 0.1 < z < 10 replaces the position
// Two departures, both documented in include/dvslam_hip.h: gamma = sqrt(p p + beta beta) in place of hypot, and the device atan2.
//
// Where At lives: each Jacobi rotation reads and rewrites two rows of At (4 x 2V doubles) and two of Vt (4 x 4), and every sum runs
// in ascending k, so a landmark is one sequential chain of dependent FP64 operations — one thread each, parallel over landmarks.
// Up to kRegViews = 8 views (m = 16) At stays in registers: 64 doubles = 128 VGPRs, Vt 32 more, under the 512-VGPR file of a SIMD
// lane at two waves per SIMD; views past V are zero, which leaves every sum and rotation of the real entries bit for bit unchanged
// (x + 0 = x; a zero column stays zero).  Four views (m = 8) get their own instantiation, since the zero padding is not free.
// Larger V (the reference's observation_ids only grows) runs the same code on a per-landmark slice of global scratch, 64 B per view
// slot, addressed by the landmark's view offset: a few landmarks, through L1/L2.  The FP64 work is a few thousand flops per landmark;
// the kernel is latency bound, so 64-thread workgroups spread a small batch over as many CUs as possible.
#pragma clang fp contract(off)
#include <float.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "matcher.h"

namespace dvs {

constexpr int kRegViews = 8;

// P = K [R | t] (backend.cpp:469-477) and C = -(R^T t) (:481) of keyframe kf
struct Cam {
  double P[3][4];
};
__device__ __forceinline__ void load_cam(const double* __restrict__ R, const double* __restrict__ t, int kf, double fx, double fy, double cx,
                                         double cy, Cam& c) {
  const double* r = R + 9 * (size_t)kf;
  const double* tt = t + 3 * (size_t)kf;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c.P[0][k] = fx * r[k] + cx * r[6 + k];
    c.P[1][k] = fy * r[3 + k] + cy * r[6 + k];
    c.P[2][k] = r[6 + k];
  }
  c.P[0][3] = fx * tt[0] + cx * tt[2];
  c.P[1][3] = fy * tt[1] + cy * tt[2];
  c.P[2][3] = tt[2];
}
__device__ __forceinline__ void load_centre(const double* __restrict__ R, const double* __restrict__ t, int kf, double C[3]) {
  const double* r = R + 9 * (size_t)kf;
  const double* tt = t + 3 * (size_t)kf;
#pragma unroll
  for (int k = 0; k < 3; k++) C[k] = -(r[k] * tt[0] + r[3 + k] * tt[1] + r[6 + k] * tt[2]);
}

// At storage: registers (NV views, zero padded) or a global slice (NV == 0, m = 2V entries per row)
template <int NV>
struct AtRegs {
  static constexpr int M = 2 * NV;
  double a[4][M];
  __device__ __forceinline__ double& at(int r, int k) { return a[r][k]; }
};
struct AtGlobal {
  static constexpr int M = 0;
  double* base;
  int m;
  __device__ __forceinline__ double& at(int r, int k) { return base[(size_t)r * m + k]; }
};

// JacobiSVDImpl_<double> (OpenCV 4.x modules/core/src/lapack.cpp) on At (n = 4 rows of length m); returns the sorted Vt's row 3
template <class S>
__device__ __forceinline__ void jacobi_null_vector(S& A, int m, double x[4]) {
  const int mm = S::M ? S::M : m;
  const double eps = 10.0 * DBL_EPSILON;
  const int max_iter = m > 30 ? m : 30;
  double W[4], Vt[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll 16
    for (int k = 0; k < mm; k++) { const double t = A.at(i, k); sd += t * t; }
    W[i] = sd;
#pragma unroll
    for (int k = 0; k < 4; k++) Vt[i][k] = i == k ? 1.0 : 0.0;
  }
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = i + 1; j < 4; j++) {
        double a = W[i], p = 0, b = W[j];
#pragma unroll 16
        for (int k = 0; k < mm; k++) p += A.at(i, k) * A.at(j, k);
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = sqrt(p * p + beta * beta);
        double c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = sqrt(delta / gamma);
          c = p / (gamma * s * 2);
        } else {
          c = sqrt((gamma + beta) / (gamma * 2));
          s = p / (gamma * c * 2);
        }
        a = b = 0;
#pragma unroll 16
        for (int k = 0; k < mm; k++) {
          const double ai = A.at(i, k), aj = A.at(j, k);
          const double t0 = c * ai + s * aj;
          const double t1 = -s * ai + c * aj;
          A.at(i, k) = t0; A.at(j, k) = t1;
          a += t0 * t0; b += t1 * t1;
        }
        W[i] = a; W[j] = b;
        changed = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const double t0 = c * Vt[i][k] + s * Vt[j][k];
          const double t1 = -s * Vt[i][k] + c * Vt[j][k];
          Vt[i][k] = t0; Vt[j][k] = t1;
        }
      }
    if (!changed) break;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll 16
    for (int k = 0; k < mm; k++) { const double t = A.at(i, k); sd += t * t; }
    W[i] = sqrt(sd);
  }
  // selection sort, descending (`if (W[j] < W[k]) j = k`): only the row that ends in place 3 is needed, so the swaps move indices
  int idx[4] = {0, 1, 2, 3};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int j = i; double wj = W[i];
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (wj < W[k]) { j = k; wj = W[k]; }
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (k == j) {
        const double tw = W[i]; W[i] = W[k]; W[k] = tw;
        const int ti = idx[i]; idx[i] = idx[k]; idx[k] = ti;
      }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (idx[3] == r) {
#pragma unroll
      for (int k = 0; k < 4; k++) x[k] = Vt[r][k];
    }
}

struct TriArgs {
  const double* R; const double* t; int nkf;
  double fx, fy, cx, cy;
  int nlm; long long nviews;
  const long long* offs; const int* vkf; const float* vpx;
  const float* xyz_in; float* xyz_out; int* status;
  double* scratch;   // 8 doubles per view slot (landmarks with more than kRegViews views)
};

__device__ __forceinline__ long long next_view(const int* __restrict__ vkf, long long v, long long end) {
  while (v < end && vkf[v] < 0) v++;
  return v;
}

// A rows of the views into At (registers: every slot s < NV, zero past V)
template <class S>
__device__ __forceinline__ void fill_A(S& A, const TriArgs& g, long long o0, long long o1, int V) {
  const int slots = S::M ? S::M / 2 : V;
  long long v = next_view(g.vkf, o0, o1);
#pragma unroll 8
  for (int s = 0; s < slots; s++) {
    if (s < V) {
      Cam cam;
      load_cam(g.R, g.t, g.vkf[v], g.fx, g.fy, g.cx, g.cy, cam);
      const double u = (double)g.vpx[2 * v], w = (double)g.vpx[2 * v + 1];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        A.at(k, 2 * s) = u * cam.P[2][k] - cam.P[0][k];
        A.at(k, 2 * s + 1) = w * cam.P[2][k] - cam.P[1][k];
      }
      v = next_view(g.vkf, v + 1, o1);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) { A.at(k, 2 * s) = 0.0; A.at(k, 2 * s + 1) = 0.0; }
    }
  }
}

template <class S>
__device__ __forceinline__ void null_vector(S& A, const TriArgs& g, long long o0, long long o1, int V, double x[4]) {
  fill_A(A, g, o0, o1, V);
  jacobi_null_vector(A, 2 * V, x);
}

__global__ __launch_bounds__(64) void k_triangulate(TriArgs g) {
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= g.nlm) return;
  const float X0 = g.xyz_in[3 * (size_t)l], X1 = g.xyz_in[3 * (size_t)l + 1], X2 = g.xyz_in[3 * (size_t)l + 2];
  float o[3] = {X0, X1, X2};
  int status = DVS_TRI_UPDATED;
  const long long o0 = g.offs[l], o1 = g.offs[l + 1];
  int V = 0;
  if (o0 < 0 || o1 < o0 || o1 > g.nviews) {
    status = DVS_ERR_ARG;   // the host entry point refuses these; the device one marks the landmark and leaves it
  } else {
    for (long long v = o0; v < o1; v++) {
      const int kf = g.vkf[v];
      if (kf >= g.nkf) status = DVS_ERR_ARG;
      V += kf >= 0;
    }
  }
  if (status == DVS_TRI_UPDATED && V < 2) status = DVS_TRI_FEW_VIEWS;
  if (status == DVS_TRI_UPDATED) {
    // parallax gate (backend.cpp:489-521): the maximum is >= the bound iff one pair reaches it, so the walk stops there
    const double Xd[3] = {(double)X0, (double)X1, (double)X2};
    const double min_angle = 0.0175 * 5;
    bool pass = false;
    for (long long vi = next_view(g.vkf, o0, o1); vi < o1 && !pass; vi = next_view(g.vkf, vi + 1, o1)) {
      double Ci[3];
      load_centre(g.R, g.t, g.vkf[vi], Ci);
      const double e0 = Xd[0] - Ci[0], e1 = Xd[1] - Ci[1], e2 = Xd[2] - Ci[2];
      const double d1 = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
      for (long long vj = next_view(g.vkf, vi + 1, o1); vj < o1; vj = next_view(g.vkf, vj + 1, o1)) {
        double Cj[3];
        load_centre(g.R, g.t, g.vkf[vj], Cj);
        const double b0 = Ci[0] - Cj[0], b1 = Ci[1] - Cj[1], b2 = Ci[2] - Cj[2];
        const double bl = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
        const double f0 = Xd[0] - Cj[0], f1 = Xd[1] - Cj[1], f2 = Xd[2] - Cj[2];
        const double d2 = sqrt(f0 * f0 + f1 * f1 + f2 * f2);
        if (atan2(bl, (d1 + d2) / 2.0) >= min_angle) { pass = true; break; }
      }
    }
    if (!pass) status = DVS_TRI_LOW_PARALLAX;
  }
  float n[3] = {0.f, 0.f, 0.f};
  if (status == DVS_TRI_UPDATED) {
    double x[4];
    if (V <= 4) {
      AtRegs<4> A;
      null_vector(A, g, o0, o1, V, x);
    } else if (V <= kRegViews) {
      AtRegs<kRegViews> A;
      null_vector(A, g, o0, o1, V, x);
    } else {
      AtGlobal A{g.scratch + 8 * (size_t)o0, 2 * V};
      null_vector(A, g, o0, o1, V, x);
    }
    if (V == 2) {   // cv::triangulatePoints writes CV_32F (backend.cpp:533-545)
      const float w = (float)x[3];
      if (w != 0) { n[0] = (float)x[0] / w; n[1] = (float)x[1] / w; n[2] = (float)x[2] / w; }
      else status = DVS_TRI_DEGENERATE;
    } else {        // backend.cpp:566-574
      if (x[3] != 0) { n[0] = (float)(x[0] / x[3]); n[1] = (float)(x[1] / x[3]); n[2] = (float)(x[2] / x[3]); }
      else status = DVS_TRI_DEGENERATE;
    }
  }
  if (status == DVS_TRI_UPDATED) {   // reprojection check (backend.cpp:580-603)
    const double Y[4] = {(double)n[0], (double)n[1], (double)n[2], 1.0};
    double total = 0.0;
    int count = 0;
    for (long long v = next_view(g.vkf, o0, o1); v < o1; v = next_view(g.vkf, v + 1, o1)) {
      Cam cam;
      load_cam(g.R, g.t, g.vkf[v], g.fx, g.fy, g.cx, g.cy, cam);
      double pr[3];
#pragma unroll
      for (int r = 0; r < 3; r++) pr[r] = cam.P[r][0] * Y[0] + cam.P[r][1] * Y[1] + cam.P[r][2] * Y[2] + cam.P[r][3] * Y[3];
      if (pr[2] > 0) {
        const float ru = (float)(pr[0] / pr[2]), rv = (float)(pr[1] / pr[2]);
        const float dx = g.vpx[2 * v] - ru, dy = g.vpx[2 * v + 1] - rv;
        total += sqrt((double)dx * dx + (double)dy * dy);
        count++;
      }
    }
    if (count > 0 && total / count > 2.0) status = DVS_TRI_REPROJECTION;
  }
  if (status == DVS_TRI_UPDATED) {   // depth range (backend.cpp:607-610)
    if (n[2] > 0.1 && n[2] < 10.0) { o[0] = n[0]; o[1] = n[1]; o[2] = n[2]; }
    else status = DVS_TRI_DEPTH;
  }
  g.xyz_out[3 * (size_t)l] = o[0]; g.xyz_out[3 * (size_t)l + 1] = o[1]; g.xyz_out[3 * (size_t)l + 2] = o[2];
  g.status[l] = status;
}

// the device launch; nviews = view_offsets[nlm] (read by the caller)
static dvs_status tri_launch(dvs_matcher* ctx, int32_t nkf, const double* d_R, const double* d_t, double fx, double fy, double cx, double cy,
                             int32_t nlm, long long nviews, const int64_t* d_offs, const int32_t* d_vkf, const float* d_vpx, const float* d_in,
                             float* d_out, int32_t* d_status) {
  double* scratch = nullptr;
  if (nviews > 0) DVS_TRY(matcher_scratch(ctx, 3, (size_t)nviews * 64, (void**)&scratch));
  static_assert(sizeof(long long) == sizeof(int64_t), "offset width");
  TriArgs g{d_R, d_t, nkf, fx, fy, cx, cy, nlm, nviews, (const long long*)d_offs, d_vkf, d_vpx, d_in, d_out, d_status, scratch};
  hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((nlm + 63) / 64)), dim3(64), 0, ctx->stream, g);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

}  // namespace dvs

using namespace dvs;

extern "C" {

dvs_status dvs_triangulate_landmarks_device(dvs_matcher* ctx, int32_t nkf, const double* d_R, const double* d_t, double fx, double fy, double cx,
                                            double cy, int32_t nlm, const int64_t* d_view_offsets, const int32_t* d_view_kf, const float* d_view_px,
                                            const float* d_lm_xyz_in, float* d_lm_xyz_out, int32_t* d_status) {
  DVS_ARG(ctx && nkf >= 0 && nlm >= 0);
  if (nlm == 0) return DVS_OK;
  DVS_ARG(d_view_offsets && d_lm_xyz_in && d_lm_xyz_out && d_status);
  DVS_HIP(hipSetDevice(ctx->device));
  // the view count sizes the scratch of landmarks with more than kRegViews views: the one value read back
  int64_t nviews = 0;
  DVS_HIP(hipMemcpyAsync(&nviews, d_view_offsets + nlm, 8, hipMemcpyDeviceToHost, ctx->stream));
  DVS_HIP(hipStreamSynchronize(ctx->stream));
  DVS_ARG(nviews >= 0);
  DVS_ARG(nviews == 0 || (d_view_kf && d_view_px));
  DVS_ARG(nkf == 0 || (d_R && d_t));
  return tri_launch(ctx, nkf, d_R, d_t, fx, fy, cx, cy, nlm, nviews, d_view_offsets, d_view_kf, d_view_px, d_lm_xyz_in, d_lm_xyz_out, d_status);
}

dvs_status dvs_triangulate_landmarks(dvs_matcher* ctx, int32_t nkf, const double* R, const double* t, double fx, double fy, double cx, double cy,
                                     int32_t nlm, const int64_t* view_offsets, const int32_t* view_kf, const float* view_px, const float* lm_xyz_in,
                                     float* lm_xyz_out, int32_t* status) {
  DVS_ARG(ctx && nkf >= 0 && nlm >= 0);
  if (nlm == 0) return DVS_OK;
  DVS_ARG(view_offsets && lm_xyz_in && lm_xyz_out && status);
  DVS_ARG(view_offsets[0] >= 0);
  for (int32_t l = 0; l < nlm; l++)
    if (view_offsets[l + 1] < view_offsets[l]) { set_error("view_offsets decrease at landmark %d", l); return DVS_ERR_ARG; }
  const int64_t nviews = view_offsets[nlm];
  DVS_ARG(nviews == 0 || (view_kf && view_px));
  for (int64_t v = view_offsets[0]; v < nviews; v++)
    if (view_kf[v] >= nkf) { set_error("view %lld names keyframe %d of %d", (long long)v, view_kf[v], nkf); return DVS_ERR_ARG; }
  DVS_ARG(nkf == 0 || (R && t));
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const auto al = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t bR = al((size_t)nkf * 72 + 8), bt = al((size_t)nkf * 24 + 8), bo = al(((size_t)nlm + 1) * 8), bk = al((size_t)nviews * 4 + 4),
               bp = al((size_t)nviews * 8 + 8), bx = al((size_t)nlm * 12), bs = al((size_t)nlm * 4);
  uint8_t* base;
  DVS_TRY(matcher_scratch(ctx, 0, bR + bt + bo + bk + bp + 2 * bx + bs, (void**)&base));
  double* d_R = (double*)base; double* d_t = (double*)(base + bR);
  int64_t* d_o = (int64_t*)(base + bR + bt); int32_t* d_k = (int32_t*)(base + bR + bt + bo);
  float* d_p = (float*)(base + bR + bt + bo + bk); float* d_in = (float*)(base + bR + bt + bo + bk + bp);
  float* d_out = (float*)(base + bR + bt + bo + bk + bp + bx); int32_t* d_s = (int32_t*)(base + bR + bt + bo + bk + bp + 2 * bx);
  if (nkf) {
    DVS_HIP(hipMemcpyAsync(d_R, R, (size_t)nkf * 72, hipMemcpyHostToDevice, st));
    DVS_HIP(hipMemcpyAsync(d_t, t, (size_t)nkf * 24, hipMemcpyHostToDevice, st));
  }
  DVS_HIP(hipMemcpyAsync(d_o, view_offsets, ((size_t)nlm + 1) * 8, hipMemcpyHostToDevice, st));
  if (nviews) {
    DVS_HIP(hipMemcpyAsync(d_k, view_kf, (size_t)nviews * 4, hipMemcpyHostToDevice, st));
    DVS_HIP(hipMemcpyAsync(d_p, view_px, (size_t)nviews * 8, hipMemcpyHostToDevice, st));
  }
  DVS_HIP(hipMemcpyAsync(d_in, lm_xyz_in, (size_t)nlm * 12, hipMemcpyHostToDevice, st));
  DVS_TRY(tri_launch(ctx, nkf, d_R, d_t, fx, fy, cx, cy, nlm, nviews, d_o, d_k, d_p, d_in, d_out, d_s));
  DVS_HIP(hipMemcpyAsync(lm_xyz_out, d_out, (size_t)nlm * 12, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipMemcpyAsync(status, d_s, (size_t)nlm * 4, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

}  // extern "C"
