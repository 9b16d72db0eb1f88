// ransac.hip — the frontend's two robust-estimation stages as BATCHED HYPOTHESIS kernels:
//   dvs_find_fundamental_ransac   cv::findFundamentalMat(p1, p2, mask, FM_RANSAC, 2.0, 0.99)     frontend.cpp:635, 1146-1147
//   dvs_solve_pnp_ransac          cv::solvePnPRansac(obj, img, K, dist, rvec, tvec, false, 100, 4.0, 0.99, inliers)
//                                                                                                frontend.cpp:911-921
// OpenCV runs these as sequential sample -> fit -> count loops on one CPU thread.  Here ALL hypotheses of a call are fitted
// at once (one thread each), scored at once (one workgroup per hypothesis over all correspondences), and a single thread then
// replays the sequential loop over the counts — RANSACUpdateNumIters's adaptive stopping rule included — so the result is what
// the sequential loop with the same samples would return.
//
// Two forms of the fundamental-matrix stage: dvs_find_fundamental_cv follows OpenCV's own procedure (cv::RNG sample sequence, 7-point
// solver: see k_f7_hypotheses below); dvs_find_fundamental_ransac and the PnP stage are the library's own estimators — the reference
// only consumes the inlier SET (frontend.cpp:640-644, 1149-1153) and the refined pose — over a sampler stated here and in DESIGN.md: sample j of hypothesis h draws r = splitmix64(seed + 0x9E3779B97F4A7C15
// * (h * 16 + j + 1)) mod (n - j) and takes the r-th index not drawn before (ascending), i.e. a uniform draw without
// replacement; parity of the whole estimator is a tolerance on the inlier set and the pose (tests/test_ransac.py), not bit equality;
// each stage on its own (hypotheses, score, select, mask / inlier list, refinement) is held to a float64 reference in
// tests/test_gpu_ransac_stages.py through the dvs_test_*_stages hooks at the end of this file.
// The OpenCV-procedure forms (dvs_find_fundamental_cv*, dvs_solve_pnp_ransac_cv*) likewise: tests/test_gpu_ransac_cv_stages.py through the
// hooks of include/dvslam_hip_test_ransac_cv.h.
// The file is kernels first, then the host side: one pass per estimator over a layout of ransac_layout.h, called by the host batch body
// and by the device form of ransac_device.h (tests/test_gpu_ransac_device_forms.py: the same bytes from both), the entry points, the hooks.
// Minimal solvers: normalised 8-point (null vector by complete-pivoting elimination, rank 2 enforced through the smallest
// right singular vector) where OpenCV's kernel is the 7-point one; P3P (Grunert's quartic, all <= 4 poses scored) where
// OpenCV's kernel is 5-point EPnP.  The final pose is refined on the inliers by Levenberg-Marquardt on the reprojection error,
// which is what SOLVEPNP_ITERATIVE does, so it does not depend on the minimal solver.
// All arithmetic is FP64 (a few hundred hypotheses of a few dozen flops: latency-bound, not a throughput kernel).
#include <float.h>
#include <math.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "block_ops.h"
#include "common.h"
#ifdef DVS_TEST_HOOKS
#include "../../include/dvslam_hip_test.h"
#endif
#include "io_pinned.h"
#include "matcher.h"
#include "pnp_cv.h"   // cv::solvePnPRansac by OpenCV's procedure: EPnP hypotheses, float scoring, solvePnP(ITERATIVE) refit
#include "ransac_device.h"
#include "ransac_layout.h"
#include "ransac_shared.h"
#include "splitmix64.h"

namespace dvs {

// RansacProb (ransac_layout.h): one problem of a batch, blockIdx.y of every kernel below.

// eigenvector of the smallest eigenvalue of a symmetric 3x3 (cyclic Jacobi)
__device__ __forceinline__ void smallest_eigvec3(const double* S, double* v) {
  double a[3][3] = {{S[0], S[1], S[2]}, {S[1], S[4], S[5]}, {S[2], S[5], S[8]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; sweep++) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (off < 1e-300) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq; }
        for (int k = 0; k < 3; k++) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk; }
        for (int k = 0; k < 3; k++) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
      }
  }
  int m = 0;
  if (a[1][1] < a[m][m]) m = 1;
  if (a[2][2] < a[m][m]) m = 2;
  for (int k = 0; k < 3; k++) v[k] = V[k][m];
}

// ---------------------------------------------------------------------------------------------------------------------------
// fundamental matrix: one thread = one hypothesis from 8 correspondences (x2^T F x1 = 0)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_f_hypotheses(const float* __restrict__ p1, const float* __restrict__ p2, const RansacProb* __restrict__ probs, int H,
                                                     double* __restrict__ Fout, int* __restrict__ valid) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  const RansacProb pb = probs[blockIdx.y];
  const int n = pb.n;
  p1 += 2 * (size_t)pb.off; p2 += 2 * (size_t)pb.off;
  Fout += 9 * (size_t)H * blockIdx.y; valid += (size_t)H * blockIdx.y;
  if (n < 8) { valid[h] = 0; return; }
  int idx[8];
  sample_distinct<8>(pb.seed, h, n, idx);
  double x1[8], y1[8], x2[8], y2[8];
  double c1x = 0, c1y = 0, c2x = 0, c2y = 0;
  for (int i = 0; i < 8; i++) {
    x1[i] = p1[2 * idx[i]]; y1[i] = p1[2 * idx[i] + 1]; x2[i] = p2[2 * idx[i]]; y2[i] = p2[2 * idx[i] + 1];
    c1x += x1[i]; c1y += y1[i]; c2x += x2[i]; c2y += y2[i];
  }
  c1x /= 8; c1y /= 8; c2x /= 8; c2y /= 8;
  double d1 = 0, d2 = 0;
  for (int i = 0; i < 8; i++) {
    d1 += sqrt((x1[i] - c1x) * (x1[i] - c1x) + (y1[i] - c1y) * (y1[i] - c1y));
    d2 += sqrt((x2[i] - c2x) * (x2[i] - c2x) + (y2[i] - c2y) * (y2[i] - c2y));
  }
  bool ok = d1 > 1e-9 && d2 > 1e-9;
  const double s1 = ok ? sqrt(2.0) * 8 / d1 : 1.0, s2 = ok ? sqrt(2.0) * 8 / d2 : 1.0;   // Hartley: mean distance sqrt(2)
  double A[8][9];
  for (int i = 0; i < 8; i++) {
    const double u1 = (x1[i] - c1x) * s1, v1 = (y1[i] - c1y) * s1, u2 = (x2[i] - c2x) * s2, v2 = (y2[i] - c2y) * s2;
    A[i][0] = u2 * u1; A[i][1] = u2 * v1; A[i][2] = u2; A[i][3] = v2 * u1; A[i][4] = v2 * v1; A[i][5] = v2; A[i][6] = u1; A[i][7] = v1; A[i][8] = 1.0;
  }
  // null vector of the 8 x 9 system by Gauss-Jordan elimination with complete pivoting; the column never chosen is the free one.
  // Every loop is unrolled and the run-time row / column (pivot position) is applied by selects, so that the 72 matrix entries stay
  // in registers: indexed with run-time subscripts the array lived in scratch memory and this kernel took 102 us.  Same operations
  // in the same order on the same values.
  int colOf[8];
  unsigned usedMask = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (ok) {
      int pr = k, pc = -1;
      double best = 0;
#pragma unroll
      for (int i = k; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 9; j++) {
          const double a = fabs(A[i][j]);
          const bool take = !((usedMask >> j) & 1u) && a > best;
          best = take ? a : best; pr = take ? i : pr; pc = take ? j : pc;
        }
      if (pc < 0 || best < 1e-12) {
        ok = false;
      } else {
        // rows k and pr change places
#pragma unroll
        for (int j = 0; j < 9; j++) {
          const double tmp = A[k][j];
          double apr = tmp;
#pragma unroll
          for (int i = k + 1; i < 8; i++) apr = i == pr ? A[i][j] : apr;
          A[k][j] = apr;
#pragma unroll
          for (int i = k + 1; i < 8; i++) A[i][j] = i == pr ? tmp : A[i][j];
        }
        usedMask |= 1u << pc; colOf[k] = pc;
        double piv = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) piv = j == pc ? A[k][j] : piv;
        const double inv = 1.0 / piv;
#pragma unroll
        for (int j = 0; j < 9; j++) A[k][j] *= inv;
#pragma unroll
        for (int i = 0; i < 8; i++)
          if (i != k) {
            double fcoef = 0;
#pragma unroll
            for (int j = 0; j < 9; j++) fcoef = j == pc ? A[i][j] : fcoef;
            const bool nz = fcoef != 0.0;
#pragma unroll
            for (int j = 0; j < 9; j++) A[i][j] = nz ? A[i][j] - fcoef * A[k][j] : A[i][j];
          }
      }
    }
  }
  double f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) {
    int fc = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) if (!((usedMask >> j) & 1u)) fc = j;
#pragma unroll
    for (int j = 0; j < 9; j++) f[j] = j == fc ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      double afc = 0;
#pragma unroll
      for (int j = 0; j < 9; j++) afc = j == fc ? A[k][j] : afc;
#pragma unroll
      for (int j = 0; j < 9; j++) f[j] = j == colOf[k] ? -afc : f[j];
    }
    // rank 2: F <- F - (F v) v^T with v the right singular vector of the smallest singular value
    double S[9];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) S[3 * a + b] = f[a] * f[b] + f[3 + a] * f[3 + b] + f[6 + a] * f[6 + b];
    double v[3];
    smallest_eigvec3(S, v);
    for (int r = 0; r < 3; r++) {
      const double fv = f[3 * r] * v[0] + f[3 * r + 1] * v[1] + f[3 * r + 2] * v[2];
      for (int cidx = 0; cidx < 3; cidx++) f[3 * r + cidx] -= fv * v[cidx];
    }
    // denormalise: F = T2^T Fn T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1]
    double G[9];
    // Fn T1
    for (int r = 0; r < 3; r++) {
      G[3 * r] = f[3 * r] * s1; G[3 * r + 1] = f[3 * r + 1] * s1;
      G[3 * r + 2] = f[3 * r + 2] - s1 * (f[3 * r] * c1x + f[3 * r + 1] * c1y);
    }
    // T2^T (.)
    for (int cidx = 0; cidx < 3; cidx++) {
      f[cidx] = s2 * G[cidx]; f[3 + cidx] = s2 * G[3 + cidx];
      f[6 + cidx] = G[6 + cidx] - s2 * (c2x * G[cidx] + c2y * G[3 + cidx]);
    }
    double nrm = 0;
    for (int k = 0; k < 9; k++) nrm += f[k] * f[k];
    ok = nrm > 0 && isfinite(nrm);
    if (ok) { nrm = 1.0 / sqrt(nrm); for (int k = 0; k < 9; k++) f[k] *= nrm; }
  }
  for (int k = 0; k < 9; k++) Fout[9 * (size_t)h + k] = ok ? f[k] : 0.0;
  valid[h] = ok ? 1 : 0;
}

// OpenCV's FMEstimatorCallback::computeError: max of the two squared point-to-epipolar-line distances
__device__ __forceinline__ double epi_err(const double* F, double x1, double y1, double x2, double y2) {
  const double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
  const double d2 = x2 * a + y2 * b + c, s2 = 1.0 / (a * a + b * b);
  const double a1 = F[0] * x2 + F[3] * y2 + F[6], b1 = F[1] * x2 + F[4] * y2 + F[7], c1 = F[2] * x2 + F[5] * y2 + F[8];
  const double d1 = x1 * a1 + y1 * b1 + c1, s1 = 1.0 / (a1 * a1 + b1 * b1);
  return fmax(d1 * d1 * s1, d2 * d2 * s2);
}

// one workgroup per hypothesis: inlier count over all correspondences
__global__ __launch_bounds__(256) void k_f_score(const float* __restrict__ p1, const float* __restrict__ p2, const RansacProb* __restrict__ probs, int H,
                                                 const double* __restrict__ Fall, const int* __restrict__ valid, double thr2, int* __restrict__ counts, int fcmp) {
  const int h = blockIdx.x;
  const RansacProb pb = probs[blockIdx.y];
  const int n = pb.n;
  p1 += 2 * (size_t)pb.off; p2 += 2 * (size_t)pb.off;
  Fall += 9 * (size_t)H * blockIdx.y; valid += (size_t)H * blockIdx.y; counts += (size_t)H * blockIdx.y;
  if (!valid[h]) { if (threadIdx.x == 0) counts[h] = 0; return; }
  double F[9];
  for (int k = 0; k < 9; k++) F[k] = Fall[9 * (size_t)h + k];
  __shared__ int s_w[4];
  int total = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    bool in = false;
    if (i < n) {
      const double e = epi_err(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
      in = fcmp ? (float)e <= (float)thr2 : e <= thr2;   // OpenCV stores the error and the squared threshold as floats (findInliers)
    }
    total += block_count256(in, s_w);
  }
  if (threadIdx.x == 0) counts[h] = total;
}

__global__ __launch_bounds__(256) void k_f_mask(const float* __restrict__ p1, const float* __restrict__ p2, const RansacProb* __restrict__ probs, int H,
                                                const double* __restrict__ Fall, const int* __restrict__ sel, double thr2, unsigned char* __restrict__ mask,
                                                double* __restrict__ Fbest, int fcmp) {
  const RansacProb pb = probs[blockIdx.y];
  const int n = pb.n;
  p1 += 2 * (size_t)pb.off; p2 += 2 * (size_t)pb.off; mask += pb.off;
  Fall += 9 * (size_t)H * blockIdx.y; sel += 4 * (size_t)blockIdx.y; Fbest += 9 * (size_t)blockIdx.y;
  const int best = sel[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (best < 0) { if (i < n) mask[i] = 0; if (i < 9) Fbest[i] = 0.0; return; }
  double F[9];
  for (int k = 0; k < 9; k++) F[k] = Fall[9 * (size_t)best + k];
  if (i < 9) Fbest[i] = F[i];
  if (i < n) {
    const double e = epi_err(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
    mask[i] = (fcmp ? (float)e <= (float)thr2 : e <= thr2) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// cv::findFundamentalMat(FM_RANSAC) as OpenCV 4.x runs it for >= 15 points (calib3d fundam.cpp / ptsetreg.cpp, restated from the
// published algorithm — the library is not in this image, PARITY UNPINNED):
//   * RANSACPointSetRegistrator(modelPoints = 7): one cv::RNG, seeded with (uint64)-1, threaded through all iterations; getSubset
//     draws index i as rng.uniform(0, n) = next() % n, drawn again while it repeats an earlier index of the sample; a complete
//     sample whose LAST point is collinear with two earlier ones in either image (FMEstimatorCallback::checkSubset ->
//     haveCollinearPoints) is drawn again as a whole, up to 10000 attempts;
//   * cv::RNG::next(): multiply-with-carry, state = (uint32)state * 4164903690 + (state >> 32), value = (uint32)state;
//   * run7Point: the two null vectors f1, f2 of the 7 x 9 system of RAW pixel coordinates, det(lambda f1 + (1 - lambda) f2) = 0 by
//     cv::solveCubic (closed form), one model per real root, scaled to F(3,3) = 1; every model of a sample is scored in order;
//   * findInliers: error and squared threshold compared as floats; a strictly better count replaces the best model and shortens the
//     loop (RANSACUpdateNumIters with modelPoints = 7).  No refit on the inliers.
// The sample sequence is sequential by nature (a repeated index or a rejected sample shifts everything behind it): it is made on
// the HOST (cv_subsets: microseconds) and uploaded with the points; the models of all samples are fitted and scored at once as in
// the library's own estimator above, and the sequential loop is replayed over the counts.  OpenCV takes the null space from an SVD
// (this kernel: complete-pivoting elimination): the same models to rounding, but the order of a sample's models follows the basis,
// so a tie in inlier count between two models of ONE sample may resolve differently.
// ---------------------------------------------------------------------------------------------------------------------------
struct CvRng {
  unsigned long long state;
  explicit CvRng(unsigned long long s = 0xffffffffull) : state(s ? s : 0xffffffffull) {}
  unsigned next() { state = (unsigned long long)(unsigned)state * 4164903690ull + (unsigned)(state >> 32); return (unsigned)state; }
  int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

static bool cv_have_collinear(const float* pts, const int* idx, int count) {   // the LAST point against every earlier pair
  const int i = count - 1;
  for (int j = 0; j < i; j++) {
    const double dx1 = pts[2 * idx[j]] - pts[2 * idx[i]], dy1 = pts[2 * idx[j] + 1] - pts[2 * idx[i] + 1];
    for (int k = 0; k < j; k++) {
      const double dx2 = pts[2 * idx[k]] - pts[2 * idx[i]], dy2 = pts[2 * idx[k] + 1] - pts[2 * idx[i] + 1];
      if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
  }
  return false;
}

// the samples of iterations 0 .. iters - 1 (modelPoints <= 16 indices each); returns how many iterations found one.  p1 = p2 = NULL: getSubset
// without a checkSubset, the 5-point samples of cv::solvePnPRansac's RANSAC stage — every iteration finds one at its first attempt
static int cv_subsets(const float* p1, const float* p2, int n, int modelPoints, int iters, int32_t* idx_out, int maxAttempts = 10000) {
  CvRng rng(~0ull);
  int idx[16];
  for (int it = 0; it < iters; it++) {
    bool found = false;
    for (int attempt = 0; attempt < maxAttempts && !found; attempt++) {
      for (int i = 0; i < modelPoints; i++) {
        int v;
        bool dup;
        do {
          v = rng.uniform(0, n);
          dup = false;
          for (int j = 0; j < i; j++) dup = dup || idx[j] == v;
        } while (dup);
        idx[i] = v;
      }
      found = !p1 || !(cv_have_collinear(p1, idx, modelPoints) || cv_have_collinear(p2, idx, modelPoints));
    }
    if (!found) return it;
    for (int i = 0; i < modelPoints; i++) idx_out[(size_t)it * modelPoints + i] = idx[i];
  }
  return iters;
}

// cv::solveCubic for c[0] x^3 + c[1] x^2 + c[2] x + c[3] (closed form, roots in the order OpenCV returns them)
__device__ __forceinline__ int cv_solve_cubic(const double* c, double* x) {
  double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3];
  int n = 0;
  x[0] = x[1] = x[2] = 0;
  if (a0 == 0) {
    if (a1 == 0) {
      if (a2 == 0) return 0;
      x[0] = -a3 / a2; return 1;
    }
    double d = a2 * a2 - 4 * a1 * a3;
    if (d >= 0) {
      d = sqrt(d);
      const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
      if (fabs(q1) > fabs(q2)) { x[0] = q1 / a1; x[1] = a3 / q1; } else { x[0] = q2 / a1; x[1] = a3 / q2; }
      n = d > 0 ? 2 : 1;
    }
    return n;
  }
  a0 = 1. / a0; a1 *= a0; a2 *= a0; a3 *= a0;
  const double Q = (a1 * a1 - 3 * a2) * (1. / 9), R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1. / 54);
  const double Qcubed = Q * Q * Q;
  double d = Qcubed - R * R;
  if (d > 0) {
    const double theta = acos(R / sqrt(Qcubed)), sqrtQ = sqrt(Q);
    const double t0 = -2 * sqrtQ, t1 = theta * (1. / 3), t2 = a1 * (1. / 3);
    x[0] = t0 * cos(t1) - t2;
    x[1] = t0 * cos(t1 + (2. * 3.1415926535897932384626433832795 / 3)) - t2;
    x[2] = t0 * cos(t1 + (4. * 3.1415926535897932384626433832795 / 3)) - t2;
    n = 3;
  } else if (d == 0) {
    if (R >= 0) { x[0] = -2 * pow(R, 1. / 3) - a1 / 3; x[1] = pow(R, 1. / 3) - a1 / 3; }
    else { x[0] = 2 * pow(-R, 1. / 3) - a1 / 3; x[1] = -pow(-R, 1. / 3) - a1 / 3; }
    n = x[0] == x[1] ? 1 : 2;
    if (n == 1) x[1] = 0;
  } else {
    d = sqrt(-d);
    double e = pow(d + fabs(R), 1. / 3);
    if (R > 0) e = -e;
    x[0] = (e + Q / e) - a1 * (1. / 3);
    n = 1;
  }
  return n;
}

__device__ __forceinline__ double det3rows(const double* a, const double* b, const double* c) {   // rows a, b, c
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// one thread = one sample: up to three models at Fout[3 h .. 3 h + 2]
__global__ __launch_bounds__(64) void k_f7_hypotheses(const float* __restrict__ p1, const float* __restrict__ p2, const RansacProb* __restrict__ probs,
                                                      const int32_t* __restrict__ samples, int H, double* __restrict__ Fout, int* __restrict__ valid) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  const RansacProb pb = probs[blockIdx.y];
  p1 += 2 * (size_t)pb.off; p2 += 2 * (size_t)pb.off;
  Fout += 27 * (size_t)H * blockIdx.y; valid += 3 * (size_t)H * blockIdx.y; samples += 7 * (size_t)H * blockIdx.y;
  valid[3 * h] = valid[3 * h + 1] = valid[3 * h + 2] = 0;
  if (h >= pb.sampled_iterations()) return;   // iterations getSubset found no sample for
  double A[7][9];
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const int id = samples[7 * (size_t)h + i];
    const double x0 = p1[2 * id], y0 = p1[2 * id + 1], x1 = p2[2 * id], y1 = p2[2 * id + 1];
    A[i][0] = x1 * x0; A[i][1] = x1 * y0; A[i][2] = x1; A[i][3] = y1 * x0; A[i][4] = y1 * y0; A[i][5] = y1; A[i][6] = x0; A[i][7] = y0; A[i][8] = 1.0;
  }
  // reduced row echelon form by Gauss-Jordan elimination with complete pivoting, everything unrolled and the run-time pivot position
  // applied by selects (as in k_f_hypotheses: the matrix stays in registers); the two columns never chosen are the free ones
  int colOf[7];
  unsigned usedMask = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    if (ok) {
      int pr = k, pc = -1;
      double best = 0;
#pragma unroll
      for (int i = k; i < 7; i++)
#pragma unroll
        for (int j = 0; j < 9; j++) {
          const double a = fabs(A[i][j]);
          const bool take = !((usedMask >> j) & 1u) && a > best;
          best = take ? a : best; pr = take ? i : pr; pc = take ? j : pc;
        }
      if (pc < 0 || !(best > 0)) {
        ok = false;
      } else {
#pragma unroll
        for (int j = 0; j < 9; j++) {
          const double tmp = A[k][j];
          double apr = tmp;
#pragma unroll
          for (int i = k + 1; i < 7; i++) apr = i == pr ? A[i][j] : apr;
          A[k][j] = apr;
#pragma unroll
          for (int i = k + 1; i < 7; i++) A[i][j] = i == pr ? tmp : A[i][j];
        }
        usedMask |= 1u << pc; colOf[k] = pc;
        double piv = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) piv = j == pc ? A[k][j] : piv;
        const double inv = 1.0 / piv;
#pragma unroll
        for (int j = 0; j < 9; j++) A[k][j] *= inv;
#pragma unroll
        for (int i = 0; i < 7; i++)
          if (i != k) {
            double fcoef = 0;
#pragma unroll
            for (int j = 0; j < 9; j++) fcoef = j == pc ? A[i][j] : fcoef;
            const bool nz = fcoef != 0.0;
#pragma unroll
            for (int j = 0; j < 9; j++) A[i][j] = nz ? A[i][j] - fcoef * A[k][j] : A[i][j];
          }
      }
    }
  }
  if (!ok) return;
  int fa = -1, fb = -1;
#pragma unroll
  for (int j = 0; j < 9; j++) if (!((usedMask >> j) & 1u)) { if (fa < 0) fa = j; else fb = j; }
  double f1[9], f2[9];
#pragma unroll
  for (int j = 0; j < 9; j++) { f1[j] = j == fa ? 1.0 : 0.0; f2[j] = j == fb ? 1.0 : 0.0; }
#pragma unroll
  for (int k = 0; k < 7; k++) {
    double aa = 0, ab = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) { aa = j == fa ? A[k][j] : aa; ab = j == fb ? A[k][j] : ab; }
#pragma unroll
    for (int j = 0; j < 9; j++) { f1[j] = j == colOf[k] ? -aa : f1[j]; f2[j] = j == colOf[k] ? -ab : f2[j]; }
  }
  // unit length (the elimination's basis has entries of very different size; OpenCV's comes from an SVD), then run7Point
  double n1 = 0, n2 = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) { n1 += f1[j] * f1[j]; n2 += f2[j] * f2[j]; }
  n1 = 1.0 / sqrt(n1); n2 = 1.0 / sqrt(n2);
#pragma unroll
  for (int j = 0; j < 9; j++) { f1[j] *= n1; f2[j] *= n2; }
#pragma unroll
  for (int j = 0; j < 9; j++) f1[j] -= f2[j];
  // det(lambda f1 + f2) = c0 lambda^3 + c1 lambda^2 + c2 lambda + c3
  double c[4];
  c[0] = det3rows(f1, f1 + 3, f1 + 6);
  c[1] = det3rows(f2, f1 + 3, f1 + 6) + det3rows(f1, f2 + 3, f1 + 6) + det3rows(f1, f1 + 3, f2 + 6);
  c[2] = det3rows(f1, f2 + 3, f2 + 6) + det3rows(f2, f1 + 3, f2 + 6) + det3rows(f2, f2 + 3, f1 + 6);
  c[3] = det3rows(f2, f2 + 3, f2 + 6);
  double r[3];
  const int nr = cv_solve_cubic(c, r);
  for (int k = 0; k < nr; k++) {
    double lambda = r[k], mu = 1.0;
    const double sden = f1[8] * r[k] + f2[8];
    double F[9];
    if (fabs(sden) > DBL_EPSILON) { mu = 1.0 / sden; lambda *= mu; F[8] = 1.0; } else F[8] = 0.0;
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 8; j++) { F[j] = f1[j] * lambda + f2[j] * mu; fin = fin && isfinite(F[j]); }
    if (!fin) continue;
#pragma unroll
    for (int j = 0; j < 9; j++) Fout[9 * (size_t)(3 * h + k) + j] = F[j];
    valid[3 * h + k] = 1;
  }
}

// cv::LMeDSPointSetRegistrator::run over the models of k_f7_hypotheses — what cv::findFundamentalMat(FM_RANSAC) runs BELOW 15 points
// (calib3d ptsetreg.cpp, restated from the published algorithm): a fixed number of iterations (RANSACUpdateNumIters(confidence, 0.45, 7,
// maxIters), at least 3: 300 for 0.99), the same sample procedure (getSubset with 1000 attempts), every model of a sample in order;
// a model's score is the MEDIAN of its float errors (std::nth_element at count / 2: the upper median), a strictly smaller median
// replaces the best; then sigma = 2.5 * 1.4826 * (1 + 5 / (count - 7)) * sqrt(minMedian), at least 0.001, the inliers are the errors
// <= (float)(sigma^2), and the call succeeds when at least 7 of them remain (the mask is written either way).  One workgroup per
// problem (n <= 14 here): the threads take the models in turn, the lowest (median, index) wins, thread 0 writes the mask.
// sel[0] = best model (-1: none), sel[1] = iterations run, sel[2] = inliers, sel[3] = success.
__global__ __launch_bounds__(256) void k_lmeds_select(const float* __restrict__ p1, const float* __restrict__ p2, const RansacProb* __restrict__ probs, int H,
                                                      int niters, const double* __restrict__ Fall, const int* __restrict__ valid, int* __restrict__ sel,
                                                      unsigned char* __restrict__ mask, double* __restrict__ Fbest) {
  const RansacProb pb = probs[blockIdx.x];
  const int n = pb.n, tid = threadIdx.x;
  p1 += 2 * (size_t)pb.off; p2 += 2 * (size_t)pb.off; mask += pb.off;
  Fall += 27 * (size_t)H * blockIdx.x; valid += 3 * (size_t)H * blockIdx.x; sel += 4 * (size_t)blockIdx.x; Fbest += 9 * (size_t)blockIdx.x;
  const int iters = min(min(niters, H), pb.sampled_iterations());
  __shared__ unsigned long long s_best[256];
  unsigned long long best = ~0ull;   // (median's float bits << 32) | model index: non-negative floats order as their bit patterns
  for (int m = tid; m < 3 * iters; m += 256) {
    if (!valid[m]) continue;
    double F[9];
    for (int k = 0; k < 9; k++) F[k] = Fall[9 * (size_t)m + k];
    float e[16];
    for (int i = 0; i < 16; i++) e[i] = 3.0e38f;
    for (int i = 0; i < n && i < 16; i++) e[i] = (float)epi_err(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
    for (int i = 1; i < 16; i++) {   // insertion sort (n <= 14; NaN errors of a degenerate model sort as they fall: the model cannot win)
      const float v = e[i];
      int j = i - 1;
      while (j >= 0 && e[j] > v) { e[j + 1] = e[j]; j--; }
      e[j + 1] = v;
    }
    const float med = e[n / 2];
    if (!(med >= 0.0f)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(med) << 32) | (unsigned)m;
    best = key < best ? key : best;
  }
  best = block_min<256>(best, s_best);
  if (tid != 0) return;
  sel[1] = iters;
  if (best == ~0ull) { sel[0] = -1; sel[2] = 0; sel[3] = 0; for (int i = 0; i < n; i++) mask[i] = 0; for (int k = 0; k < 9; k++) Fbest[k] = 0.0; return; }
  const int bm = (int)(unsigned)best;
  const double minMedian = (double)__uint_as_float((unsigned)(best >> 32));
  double sigma = 2.5 * 1.4826 * (1 + 5. / (n - 7)) * sqrt(minMedian);
  sigma = fmax(sigma, 0.001);
  const float t = (float)(sigma * sigma);
  double F[9];
  for (int k = 0; k < 9; k++) { F[k] = Fall[9 * (size_t)bm + k]; Fbest[k] = F[k]; }
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    const int in = (float)epi_err(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) <= t ? 1 : 0;
    mask[i] = (unsigned char)in; cnt += in;
  }
  sel[0] = bm; sel[2] = cnt; sel[3] = cnt >= 7 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// PnP: P3P hypotheses (Grunert 1841 as in Haralick et al., "Review and analysis of solutions of the three point perspective
// pose estimation problem", IJCV 1994): quartic in v = s3 / s1, then u = s2 / s1, the three depths, and the rigid motion that
// takes the object triangle onto the camera-frame triangle.
// ---------------------------------------------------------------------------------------------------------------------------
// real roots of a4 x^4 + a3 x^3 + a2 x^2 + a1 x + a0 (Ferrari through the resolvent cubic), each polished by Newton steps
__host__ __device__ __forceinline__ int quartic_real_roots(double a4, double a3, double a2, double a1, double a0, double* roots) {
  if (!(fabs(a4) > 1e-14 * (fabs(a3) + fabs(a2) + fabs(a1) + fabs(a0)))) return 0;
  const double b = a3 / a4, c = a2 / a4, d = a1 / a4, e = a0 / a4;
  // depressed quartic y^4 + p y^2 + q y + r, x = y - b / 4
  const double p = c - 3.0 * b * b / 8.0, q = d - b * c / 2.0 + b * b * b / 8.0, r = e - b * d / 4.0 + b * b * c / 16.0 - 3.0 * b * b * b * b / 256.0;
  int nr = 0;
  double ys[4];
  if (fabs(q) < 1e-14 * (1.0 + fabs(p) + fabs(r))) {  // biquadratic
    const double disc = p * p - 4.0 * r;
    if (disc >= -1e-9 * (p * p + fabs(4.0 * r))) {
      const double sd = sqrt(fmax(disc, 0.0));
      const double z[2] = {(-p + sd) / 2.0, (-p - sd) / 2.0};
      for (int k = 0; k < 2; k++) if (z[k] >= 0) { ys[nr++] = sqrt(z[k]); ys[nr++] = -sqrt(z[k]); }
    }
  } else {
    // resolvent cubic 8 m^3 + 8 p m^2 + (2 p^2 - 8 r) m - q^2 = 0: its largest real root is positive when q != 0
    const double B = p, C = (p * p - 4.0 * r) / 4.0, D = -q * q / 8.0;   // m^3 + B m^2 + C m + D
    const double Q3 = (3.0 * C - B * B) / 9.0, R3 = (9.0 * B * C - 27.0 * D - 2.0 * B * B * B) / 54.0;
    const double disc = Q3 * Q3 * Q3 + R3 * R3;
    double m;
    if (disc >= 0) {
      const double sd = sqrt(disc);
      m = cbrt(R3 + sd) + cbrt(R3 - sd) - B / 3.0;
    } else {
      const double th = acos(fmax(-1.0, fmin(1.0, R3 / sqrt(-Q3 * Q3 * Q3))));
      m = 2.0 * sqrt(-Q3) * cos(th / 3.0) - B / 3.0;
    }
    for (int k = 0; k < 3; k++) {  // polish the resolvent root
      const double fm = ((m + B) * m + C) * m + D, dfm = (3.0 * m + 2.0 * B) * m + C;
      if (dfm != 0.0) m -= fm / dfm;
    }
    if (m > 0) {
      const double s2m = sqrt(2.0 * m);
      // (y^2 + p/2 + m)^2 = 2 m (y - q / (4 m))^2  ->  y^2 + s y + (p/2 + m - q / (2 s)) = 0  and  y^2 - s y + (p/2 + m + q / (2 s)) = 0
      const double t2 = p / 2.0 + m - q / (2.0 * s2m), t1 = p / 2.0 + m + q / (2.0 * s2m);   // t2 pairs with the (-s) roots, t1 with (+s)
      // a double root shows up as a discriminant of either sign at rounding level: keep it (Newton below settles it), or a
      // fronto-parallel triangle — the planar scenes of an RGB-D camera facing a wall — loses its true pose
      const double dA = 2.0 * m - 4.0 * t2, dB = 2.0 * m - 4.0 * t1, tol = 1e-9 * (fabs(2.0 * m) + fabs(4.0 * t1) + fabs(4.0 * t2));
      if (dA >= -tol) { const double sd = sqrt(fmax(dA, 0.0)); ys[nr++] = (-s2m + sd) / 2.0; ys[nr++] = (-s2m - sd) / 2.0; }
      if (dB >= -tol) { const double sd = sqrt(fmax(dB, 0.0)); ys[nr++] = (s2m + sd) / 2.0; ys[nr++] = (s2m - sd) / 2.0; }
    }
  }
  for (int k = 0; k < nr; k++) {
    double x = ys[k] - b / 4.0;
    for (int itn = 0; itn < 3; itn++) {
      const double fx = (((a4 * x + a3) * x + a2) * x + a1) * x + a0, dfx = ((4.0 * a4 * x + 3.0 * a3) * x + 2.0 * a2) * x + a1;
      if (dfx == 0.0) break;
      x -= fx / dfx;
    }
    roots[k] = x;
  }
  return nr;
}

__host__ __device__ __forceinline__ void triad(const double* A0, const double* A1, const double* A2, double E[3][3], bool& ok) {
  double d1[3], d2[3], e3[3];
  for (int k = 0; k < 3; k++) { d1[k] = A1[k] - A0[k]; d2[k] = A2[k] - A0[k]; }
  const double n1 = sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]);
  e3[0] = d1[1] * d2[2] - d1[2] * d2[1]; e3[1] = d1[2] * d2[0] - d1[0] * d2[2]; e3[2] = d1[0] * d2[1] - d1[1] * d2[0];
  const double n3 = sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
  ok = ok && n1 > 1e-12 && n3 > 1e-12;
  for (int k = 0; k < 3; k++) { E[k][0] = d1[k] / n1; E[k][2] = e3[k] / n3; }
  E[0][1] = E[1][2] * E[2][0] - E[2][2] * E[1][0];
  E[1][1] = E[2][2] * E[0][0] - E[0][2] * E[2][0];
  E[2][1] = E[0][2] * E[1][0] - E[1][2] * E[0][0];
}

// Grunert's P3P for one triangle: object points P (rows), unit bearings j (rows) -> up to 4 poses (R row-major 9, t 3 each) with
// x_cam = R X + t, in ascending order of the quartic's root
__host__ __device__ __forceinline__ int p3p_solve(const double P[3][3], const double j[3][3], double* poses /* 4 x 12 */) {
  auto dist2 = [&](int a, int b) { double s = 0; for (int k = 0; k < 3; k++) s += (P[a][k] - P[b][k]) * (P[a][k] - P[b][k]); return s; };
  auto dot = [&](int a, int b) { return j[a][0] * j[b][0] + j[a][1] * j[b][1] + j[a][2] * j[b][2]; };
  const double a2 = dist2(1, 2), b2 = dist2(0, 2), c2 = dist2(0, 1);
  const double ca = dot(1, 2), cb = dot(0, 2), cg = dot(0, 1);
  int nsol = 0;
  if (!(a2 > 1e-18 && b2 > 1e-18 && c2 > 1e-18)) return 0;
  const double q = (a2 - c2) / b2, w = (a2 + c2) / b2;
  const double A4 = (q - 1) * (q - 1) - 4 * c2 / b2 * ca * ca;
  const double A3 = 4 * (q * (1 - q) * cb - (1 - w) * ca * cg + 2 * c2 / b2 * ca * ca * cb);
  const double A2 = 2 * (q * q - 1 + 2 * q * q * cb * cb + 2 * (b2 - c2) / b2 * ca * ca - 4 * w * ca * cb * cg + 2 * (b2 - a2) / b2 * cg * cg);
  const double A1 = 4 * (-q * (1 + q) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - w) * ca * cg);
  const double A0 = (1 + q) * (1 + q) - 4 * a2 / b2 * cg * cg;
  double roots[4];
  const int nr = quartic_real_roots(A4, A3, A2, A1, A0, roots);
  for (int a = 1; a < nr; a++) {   // canonical solution order (ascending v): ties between equally good poses resolve the same way
    const double key = roots[a];
    int b = a - 1;
    while (b >= 0 && roots[b] > key) { roots[b + 1] = roots[b]; b--; }
    roots[b + 1] = key;
  }
  for (int rI = 0; rI < nr && nsol < 4; rI++) {
    double v = roots[rI];
    if (!(v > 0) || !isfinite(v)) continue;
    if (rI > 0 && fabs(v - roots[rI - 1]) <= 1e-9 * fabs(v)) continue;   // a double root gives one pose
    const double den = 2 * (cg - v * ca);
    if (fabs(den) < 1e-12) continue;
    double u = ((-1 + q) * v * v - 2 * q * cb * v + 1 + q) / den;
    if (!(u > 0) || !isfinite(u)) continue;
    // (u, v) is a common root of the cosine laws of sides c and a, each divided by the one of side b:
    //   f1 = 1 + u^2 - 2 u cg - (c2 / b2) m,   f2 = u^2 + v^2 - 2 u v ca - (a2 / b2) m,   m = 1 + v^2 - 2 v cb.
    // The quartic's root carries the cancellations of its coefficients divided by the distance to the next root (roots 3e-4 apart
    // left v 5e-10 off and the pose 4e-6 px off its own sample), and u the root's last digits divided by `den` (den = 1e-4 left u 5e-7
    // off, the pose 2e-4 px).  The pair itself has no such cancellation: where it is not met to rounding, Newton steps on it, each
    // kept only if it lowers the residual.  A pair that meets it is left as it is, bit for bit.
    for (int k = 0; k < 3; k++) {
      const double m = 1 + v * v - 2 * v * cb;
      const double f1 = 1 + u * u - 2 * u * cg - c2 / b2 * m, f2 = u * u + v * v - 2 * u * v * ca - a2 / b2 * m;
      const double res = fmax(fabs(f1), fabs(f2));
      if (!(res > 1e-12 * (1 + u * u + v * v))) break;
      const double f1u = 2 * (u - cg), f1v = -2 * c2 / b2 * (v - cb), f2u = 2 * (u - v * ca), f2v = 2 * (v - u * ca) - 2 * a2 / b2 * (v - cb);
      const double det = f1u * f2v - f1v * f2u;
      if (det == 0.0) break;
      const double un = u - (f1 * f2v - f1v * f2) / det, vn = v - (f1u * f2 - f2u * f1) / det;
      const double mn = 1 + vn * vn - 2 * vn * cb;
      const double g1 = 1 + un * un - 2 * un * cg - c2 / b2 * mn, g2 = un * un + vn * vn - 2 * un * vn * ca - a2 / b2 * mn;
      if (!(fmax(fabs(g1), fabs(g2)) < res)) break;
      u = un; v = vn;
    }
    if (!(u > 0) || !(v > 0)) continue;
    const double dd = 1 + u * u - 2 * u * cg;
    if (!(dd > 1e-18)) continue;
    const double s1 = sqrt(c2 / dd), s2 = u * s1, s3 = v * s1;
    double Q[3][3];
    for (int k = 0; k < 3; k++) { Q[0][k] = s1 * j[0][k]; Q[1][k] = s2 * j[1][k]; Q[2][k] = s3 * j[2][k]; }
    double EQ[3][3], EP[3][3];
    bool ok = true;
    triad(Q[0], Q[1], Q[2], EQ, ok);
    triad(P[0], P[1], P[2], EP, ok);
    if (!ok) continue;
    double* o = poses + 12 * nsol;
    double R[9];
    for (int a = 0; a < 3; a++) for (int bq = 0; bq < 3; bq++) R[3 * a + bq] = EQ[a][0] * EP[bq][0] + EQ[a][1] * EP[bq][1] + EQ[a][2] * EP[bq][2];
    bool fin = true;
    for (int k = 0; k < 9; k++) { o[k] = R[k]; fin = fin && isfinite(R[k]); }
    for (int a = 0; a < 3; a++) { o[9 + a] = Q[0][a] - (R[3 * a] * P[0][0] + R[3 * a + 1] * P[0][1] + R[3 * a + 2] * P[0][2]); fin = fin && isfinite(o[9 + a]); }
    if (!fin) continue;
    nsol++;
  }
  return nsol;
}

// one thread = one sample of 3 correspondences -> up to 4 poses; unused slots are marked invalid
__global__ __launch_bounds__(64) void k_p3p_hypotheses(const float* __restrict__ obj, const float* __restrict__ img, const RansacProb* __restrict__ probs, int H,
                                                       double fx, double fy, double cx, double cy, double* __restrict__ poses, int* __restrict__ valid) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  const RansacProb pb = probs[blockIdx.y];
  const int n = pb.n;
  obj += 3 * (size_t)pb.off; img += 2 * (size_t)pb.off;
  poses += 12 * (size_t)4 * H * blockIdx.y; valid += (size_t)4 * H * blockIdx.y;
  if (n < 4) { for (int s = 0; s < 4; s++) valid[4 * h + s] = 0; return; }
  int idx[3];
  sample_distinct<3>(pb.seed, h, n, idx);
  double P[3][3], j[3][3];
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) P[i][k] = obj[3 * idx[i] + k];
    const double bx = (img[2 * idx[i]] - cx) / fx, by = (img[2 * idx[i] + 1] - cy) / fy;
    const double nn = 1.0 / sqrt(bx * bx + by * by + 1.0);
    j[i][0] = bx * nn; j[i][1] = by * nn; j[i][2] = nn;
  }
  // the solutions go straight to their slots (a local array indexed by the running solution count lived in scratch memory)
  const int nsol = p3p_solve(P, j, poses + 12 * ((size_t)4 * h));
  for (int s = 0; s < 4; s++) valid[4 * h + s] = s < nsol ? 1 : 0;
}

__device__ __forceinline__ double reproj_err2(const double* R, const double* t, double fx, double fy, double cx, double cy, const float* X, const float* uv) {
  const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
  if (!(z > 1e-9)) return 1e300;
  const double du = fx * x / z + cx - uv[0], dv = fy * y / z + cy - uv[1];
  return du * du + dv * dv;
}

__global__ __launch_bounds__(256) void k_pnp_score(const float* __restrict__ obj, const float* __restrict__ img, const RansacProb* __restrict__ probs, int H4,
                                                   const double* __restrict__ poses, const int* __restrict__ valid, double fx, double fy, double cx, double cy,
                                                   double thr2, int* __restrict__ counts) {
  const int h = blockIdx.x;
  const RansacProb pb = probs[blockIdx.y];
  const int n = pb.n;
  obj += 3 * (size_t)pb.off; img += 2 * (size_t)pb.off;
  poses += 12 * (size_t)H4 * blockIdx.y; valid += (size_t)H4 * blockIdx.y; counts += (size_t)H4 * blockIdx.y;
  if (!valid[h]) { if (threadIdx.x == 0) counts[h] = 0; return; }
  double Rt[12];
  for (int k = 0; k < 12; k++) Rt[k] = poses[12 * (size_t)h + k];
  __shared__ int s_w[4];
  int total = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    bool in = false;
    if (i < n) in = reproj_err2(Rt, Rt + 9, fx, fy, cx, cy, obj + 3 * i, img + 2 * i) <= thr2;
    total += block_count256(in, s_w);
  }
  if (threadIdx.x == 0) counts[h] = total;
}

__device__ __forceinline__ void exp_so3(const double* w, double* E) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  const double A = th < 1e-8 ? 1.0 - th2 / 6.0 : sin(th) / th, B = th < 1e-8 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double kk = 0;
      for (int c = 0; c < 3; c++) kk += K[3 * a + c] * K[3 * c + b];
      E[3 * a + b] = (a == b ? 1.0 : 0.0) + A * K[3 * a + b] + B * kk;
    }
}

// inlier mask of the selected pose, then Levenberg-Marquardt on the reprojection error over the inliers (what
// SOLVEPNP_ITERATIVE does), one workgroup.  out: rvec (Rodrigues) + tvec; inliers as ascending indices.
// Per problem (blockIdx.x): results record `res` = {nin, success, pad, pad (16 B) | rvec, tvec (48 B)}, inlier list at inliers + off.
__global__ __launch_bounds__(256) void k_pnp_refine(const float* __restrict__ obj, const float* __restrict__ img, const RansacProb* __restrict__ probs, int H4,
                                                    const double* __restrict__ poses, const int* __restrict__ sel, double fx, double fy, double cx, double cy,
                                                    double thr2, int* __restrict__ inliers, PnpRecord* __restrict__ resAll) {
  const RansacProb pb = probs[blockIdx.x];
  const int n = pb.n;
  obj += 3 * (size_t)pb.off; img += 2 * (size_t)pb.off; inliers += pb.off;
  poses += 12 * (size_t)H4 * blockIdx.x; sel += 4 * (size_t)blockIdx.x;
  PnpRecord& res = resAll[blockIdx.x];
  __shared__ double sm[256];
  __shared__ double sm27[27][256];   // 54 KB: all normal-equation sums of an iteration in one reduction tree
  __shared__ double sR[9], st[3], sRn[9], stn[3], sH[36], sg[6], sd[6];
  __shared__ int s_w[4];
  __shared__ double s_lambda;
  __shared__ int s_stop;
  const int tid = threadIdx.x;
  const int best = sel[0];
  if (best < 0) { if (tid == 0) { res.n_inliers = 0; res.success = 0; for (int k = 0; k < 3; k++) res.rvec[k] = 0; for (int k = 0; k < 3; k++) res.tvec[k] = 0; } return; }
  if (tid < 9) sR[tid] = poses[12 * (size_t)best + tid];
  if (tid < 3) st[tid] = poses[12 * (size_t)best + 9 + tid];
  if (tid == 0) { s_lambda = 1e-3; s_stop = 0; }
  __syncthreads();
  // ordered inlier list (ascending index): trips of 256
  int m = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    const bool in = i < n && reproj_err2(sR, st, fx, fy, cx, cy, obj + 3 * i, img + 2 * i) <= thr2;
    int total;
    const int pos = m + block_rank256(in, s_w, total);
    if (in) inliers[pos] = i;
    m += total;
  }
  if (tid == 0) res.n_inliers = m;
  auto cost_of = [&](const double* R, const double* t) -> double {
    double c = 0;
    for (int e = tid; e < m; e += 256) { const int i = inliers[e]; c += fmin(reproj_err2(R, t, fx, fy, cx, cy, obj + 3 * i, img + 2 * i), 1e12); }
    return block_sum<256>(c, sm);
  };
  __threadfence_block();
  __syncthreads();
  double cost = cost_of(sR, st);
  for (int iter = 0; iter < 20 && m >= 3; iter++) {
    // normal equations of the current pose: left perturbation R <- exp(w) R, t <- t + dt
    double Hg[27];   // the upper triangle of H, then g
    double *H = Hg, *g = Hg + 21;
    for (int k = 0; k < 27; k++) Hg[k] = 0;
    for (int e = tid; e < m; e += 256) {
      const int i = inliers[e];
      const float* X = obj + 3 * i;
      const double rx = sR[0] * X[0] + sR[1] * X[1] + sR[2] * X[2], ry = sR[3] * X[0] + sR[4] * X[1] + sR[5] * X[2], rz = sR[6] * X[0] + sR[7] * X[1] + sR[8] * X[2];
      const double x = rx + st[0], y = ry + st[1], z = rz + st[2];
      if (!(z > 1e-9)) continue;
      const double iz = 1.0 / z, du = fx * x * iz + cx - img[2 * i], dv = fy * y * iz + cy - img[2 * i + 1];
      // d(u,v)/d p_c
      const double a00 = fx * iz, a02 = -fx * x * iz * iz, a11 = fy * iz, a12 = -fy * y * iz * iz;
      // d p_c / d w = -[R X]_x ; d p_c / d t = I
      double Ju[6], Jv[6];
      // -[r]_x = [[0, rz, -ry], [-rz, 0, rx], [ry, -rx, 0]]
      Ju[0] = a02 * ry;            Ju[1] = a00 * rz - a02 * rx;   Ju[2] = -a00 * ry;
      Jv[0] = -a11 * rz + a12 * ry; Jv[1] = -a12 * rx;             Jv[2] = a11 * rx;
      Ju[3] = a00; Ju[4] = 0; Ju[5] = a02;
      Jv[3] = 0; Jv[4] = a11; Jv[5] = a12;
      int k = 0;
      for (int a = 0; a < 6; a++) {
        for (int b = a; b < 6; b++) H[k++] += Ju[a] * Ju[b] + Jv[a] * Jv[b];
        g[a] += Ju[a] * du + Jv[a] * dv;
      }
    }
    // the 27 sums through ONE tree (27 one-wide passes were ~250 barriers per iteration and most of this kernel's 165 us)
    block_sums<256, 27>(Hg, &sm27[0][0]);
    if (tid == 0) {
      int k = 0;
      for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) { const double v = H[k++]; sH[6 * a + b] = v; sH[6 * b + a] = v; }
      for (int a = 0; a < 6; a++) sg[a] = g[a];
    }
    __syncthreads();
    bool accepted = false;
    for (int tries = 0; tries < 8 && !accepted; tries++) {
      if (tid == 0) {  // (H + lambda diag(H)) d = -g by Cholesky
        // every loop unrolled: with run-time subscripts the 6 x 6 system lived in scratch memory (one thread, ~100 dependent
        // scratch round trips per solve)
        double A[36], b6[6];
#pragma unroll
        for (int k = 0; k < 36; k++) A[k] = sH[k];
#pragma unroll
        for (int a = 0; a < 6; a++) { A[7 * a] += s_lambda * fmax(sH[7 * a], 1e-12); b6[a] = -sg[a]; }
        bool ok = true;
#pragma unroll
        for (int jx = 0; jx < 6; jx++) {
          if (ok) {
            double d = A[7 * jx];
#pragma unroll
            for (int k = 0; k < jx; k++) d -= A[6 * jx + k] * A[6 * jx + k];
            if (!(d > 0)) {
              ok = false;
            } else {
              d = sqrt(d);
              A[7 * jx] = d;
#pragma unroll
              for (int i = jx + 1; i < 6; i++) {
                double sacc = A[6 * i + jx];
#pragma unroll
                for (int k = 0; k < jx; k++) sacc -= A[6 * i + k] * A[6 * jx + k];
                A[6 * i + jx] = sacc / d;
              }
            }
          }
        }
        if (ok) {
#pragma unroll
          for (int i = 0; i < 6; i++) {
            double sacc = b6[i];
#pragma unroll
            for (int k = 0; k < i; k++) sacc -= A[6 * i + k] * b6[k];
            b6[i] = sacc / A[7 * i];
          }
#pragma unroll
          for (int i = 5; i >= 0; i--) {
            double sacc = b6[i];
#pragma unroll
            for (int k = i + 1; k < 6; k++) sacc -= A[6 * k + i] * b6[k];
            b6[i] = sacc / A[7 * i];
          }
          double E[9];
          exp_so3(b6, E);
          for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) sRn[3 * a + b] = E[3 * a] * sR[b] + E[3 * a + 1] * sR[3 + b] + E[3 * a + 2] * sR[6 + b];
          for (int a = 0; a < 3; a++) stn[a] = st[a] + b6[3 + a];
          for (int a = 0; a < 6; a++) sd[a] = b6[a];
        } else {
          for (int k = 0; k < 9; k++) sRn[k] = sR[k];
          for (int k = 0; k < 3; k++) stn[k] = st[k];
          for (int a = 0; a < 6; a++) sd[a] = 0;
        }
      }
      __syncthreads();
      const double ncost = cost_of(sRn, stn);
      if (ncost < cost) {
        accepted = true;
        const double stepn = fabs(sd[0]) + fabs(sd[1]) + fabs(sd[2]) + fabs(sd[3]) + fabs(sd[4]) + fabs(sd[5]);
        __syncthreads();
        if (tid == 0) {
          for (int k = 0; k < 9; k++) sR[k] = sRn[k];
          for (int k = 0; k < 3; k++) st[k] = stn[k];
          s_lambda = fmax(s_lambda * 0.1, 1e-12);
          if (stepn < 1e-12 || cost - ncost <= 1e-14 * cost) s_stop = 1;
        }
        cost = ncost;
      } else {
        __syncthreads();
        if (tid == 0) s_lambda *= 10.0;
      }
      __syncthreads();
    }
    if (!accepted || s_stop) break;
  }
  __syncthreads();
  if (tid == 0) {
    double w[3];
    rotation_to_rodrigues(sR, w);
    for (int k = 0; k < 3; k++) { res.rvec[k] = w[k]; res.tvec[k] = st[k]; }
    res.success = m > 0 ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The host side.  Each estimator has ONE pass — what runs on the stream once its device layout (ransac_layout.h) is carved — and two
// callers of it: the host batch body (check, zero the outputs, lay out, place the points, run the pass, fetch, unpack) and the device
// form of ransac_device.h (lay out, run the pass on the caller's pointers).  The points, the mask, the result records and the inlier
// lists are the layout's own arrays in the first and the caller's in the second; n_bound >= every problem's n sizes the
// per-correspondence grid.
// ---------------------------------------------------------------------------------------------------------------------------
static void fm_own_pass(hipStream_t st, const FmLayout& d, int nprob, int n_bound, const float* d_p1, const float* d_p2, unsigned char* d_mask, int H,
                        double threshold, double confidence) {
  hipLaunchKernelGGL(k_f_hypotheses, dim3((H + 63) / 64, nprob), dim3(64), 0, st, d_p1, d_p2, d.probs, H, d.models, d.valid);
  hipLaunchKernelGGL(k_f_score, dim3(H, nprob), dim3(256), 0, st, d_p1, d_p2, d.probs, H, d.models, d.valid, threshold * threshold, d.counts, 0);
  hipLaunchKernelGGL(k_ransac_select, dim3(nprob), dim3(1), 0, st, d.counts, H, d.probs, 8, confidence, 1, d.sel);
  hipLaunchKernelGGL(k_f_mask, dim3((std::max(n_bound, 9) + 255) / 256, nprob), dim3(256), 0, st, d_p1, d_p2, d.probs, H, d.models, d.sel, threshold * threshold, d_mask, d.F, 0);
}
static void pnp_own_pass(hipStream_t st, const PnpLayout& d, int nprob, const float* d_obj, const float* d_img, int* d_inl, PnpRecord* d_rec, int H,
                         const double* K4, double reproj_err, double confidence) {
  const int H4 = kP3pPoses * H;
  const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3], thr2 = reproj_err * reproj_err;
  hipLaunchKernelGGL(k_p3p_hypotheses, dim3((H + 63) / 64, nprob), dim3(64), 0, st, d_obj, d_img, d.probs, H, fx, fy, cx, cy, d.models, d.valid);
  hipLaunchKernelGGL(k_pnp_score, dim3(H4, nprob), dim3(256), 0, st, d_obj, d_img, d.probs, H4, d.models, d.valid, fx, fy, cx, cy, thr2, d.counts);
  hipLaunchKernelGGL(k_ransac_select, dim3(nprob), dim3(1), 0, st, d.counts, H4, d.probs, 3, confidence, kP3pPoses, d.sel);
  hipLaunchKernelGGL(k_pnp_refine, dim3(nprob), dim3(256), 0, st, d_obj, d_img, d.probs, H4, d.models, d.sel, fx, fy, cx, cy, thr2, d_inl, d_rec);
}
// the problem record of a device-resident single problem of the own estimators: the count comes from the device
__global__ void k_ransac_prob(RansacProb* __restrict__ prob, const int* __restrict__ d_n, unsigned long long seed) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *prob = RansacProb::seeded(0, *d_n, seed);
}

// cv::findFundamentalMat(FM_RANSAC)'s host policy, which dvs_find_fundamental_cv_batch and fm_cv_device both consult: the defaults, RANSAC
// or LMedS, and how many iterations get their models fitted.  The adaptive rule ends most RANSAC loops after a few dozen iterations (10 %
// outliers: ~10), and the sample sequence is the same whatever the number of samples drawn: first the models of first_pass() iterations,
// then — only where the loop wanted more (sel[3]) — all max_iters: the same result a full run gives, a prefix of the same sequence.
struct FmCvPolicy {
  double threshold, confidence;
  int max_iters;
  static bool lmeds(int n) { return n < kFmCvRansacPoints; }
  int lmeds_iters() const { return std::max(ransac_update_iters(confidence, 0.45, 7, max_iters), 3); }   // outlierRatio = 0.45; 300 for 0.99
  int first_pass() const { return std::min(max_iters, kFmCvFirstPass); }
  bool wants_full(const int* sel, int H) const { return sel[3] != 0 && H < max_iters; }
};
static FmCvPolicy fm_cv_policy(double threshold, double confidence, int max_iters) {
  if (threshold <= 0) threshold = 3;                                                 // as cv::findFundamentalMat
  if (confidence < DBL_EPSILON || confidence > 1 - DBL_EPSILON) confidence = 0.99;
  return FmCvPolicy{threshold, confidence, max_iters};
}

// OpenCV's procedure with the models of H iterations: the host draws every problem's 7-point samples from its points (pts1 / pts2: where the
// HOST reads them) into `h`, the pinned mirror of `d`, with the problem records; [records | ... | samples] go up; 3 H models per problem are
// fitted and the loop is replayed.  lmeds: the 8..14-point form (H = its fixed count, k_lmeds_select instead of score / select / mask).
static void fm_cv_pass(hipStream_t st, const PinnedIo* io, const FmLayout& d, const FmLayout& h, int nprob, const int32_t* offsets, const float* pts1,
                       const float* pts2, int n_bound, const float* d_p1, const float* d_p2, unsigned char* d_mask, int H, bool lmeds, const FmCvPolicy& P) {
  memset(h.samples, 0, h.sampb);
  for (int b = 0; b < nprob; b++) {
    const int n = offsets[b + 1] - offsets[b];
    const int found = cv_subsets(pts1 + 2 * (size_t)offsets[b], pts2 + 2 * (size_t)offsets[b], n, 7, H, h.samples + (size_t)b * H * 7, lmeds ? 1000 : 10000);
    h.probs[b] = RansacProb::sampled(offsets[b], n, found);
  }
  io->import(st, d.probs, d.inb, (size_t)((const uint8_t*)h.probs - io->h()));
  const int H3 = kF7Roots * H;
  hipLaunchKernelGGL(k_f7_hypotheses, dim3((H + 63) / 64, nprob), dim3(64), 0, st, d_p1, d_p2, d.probs, d.samples, H, d.models, d.valid);
  if (lmeds) {
    hipLaunchKernelGGL(k_lmeds_select, dim3(nprob), dim3(256), 0, st, d_p1, d_p2, d.probs, H, H, d.models, d.valid, d.sel, d_mask, d.F);
  } else {
    hipLaunchKernelGGL(k_f_score, dim3(H3, nprob), dim3(256), 0, st, d_p1, d_p2, d.probs, H3, d.models, d.valid, P.threshold * P.threshold, d.counts, 1);
    hipLaunchKernelGGL(k_ransac_select, dim3(nprob), dim3(1), 0, st, d.counts, H3, d.probs, 7, P.confidence, kF7Roots, d.sel, 1, P.max_iters);
    hipLaunchKernelGGL(k_f_mask, dim3((std::max(n_bound, 9) + 255) / 256, nprob), dim3(256), 0, st, d_p1, d_p2, d.probs, H3, d.models, d.sel, P.threshold * P.threshold, d_mask, d.F, 1);
  }
}
// cv::solvePnPRansac's procedure likewise: the 5-point samples depend on the counts alone; a problem below kPnpCvMinPoints gets none and runs
// no iteration (n == 5 would be solvePnP on all points, n == 4 the P3P kernel: not what the reference can reach)
static void pnp_cv_pass(hipStream_t st, const PinnedIo* io, const PnpLayout& d, const PnpLayout& h, int nprob, const int32_t* offsets, const float* d_obj,
                        const float* d_img, int* d_inl, PnpRecord* d_rec, int* d_sel, int H, const double* K4, double reproj_err, double confidence) {
  memset(h.samples, 0, h.sampb);
  for (int b = 0; b < nprob; b++) {
    const int n = offsets[b + 1] - offsets[b];
    const bool run = n >= kPnpCvMinPoints;
    if (run) cv_subsets(nullptr, nullptr, n, 5, H, h.samples + (size_t)b * H * 5);
    h.probs[b] = RansacProb::sampled(offsets[b], n, run ? H : 0);
  }
  io->import(st, d.probs, d.inb);
  const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
  const float thr = (float)(reproj_err * reproj_err);
  hipLaunchKernelGGL(k_epnp_hypotheses, dim3((H + kEpnpGroups - 1) / kEpnpGroups, nprob), dim3(64), 0, st, d_obj, d_img, d.probs, d.samples, H, fx, fy, cx, cy, d.models);
  hipLaunchKernelGGL(k_pnpcv_score, dim3(H, nprob), dim3(256), 0, st, d_obj, d_img, d.probs, H, d.models, fx, fy, cx, cy, thr, d.counts);
  hipLaunchKernelGGL(k_ransac_select, dim3(nprob), dim3(1), 0, st, d.counts, H, d.probs, 5, confidence, 1, d_sel, 1, H);
  hipLaunchKernelGGL(k_pnpcv_refit, dim3(nprob), dim3(64), 0, st, d_obj, d_img, d.probs, H, d.models, d_sel, fx, fy, cx, cy, thr, d_inl, d_rec DVS_REFIT_DBG_NONE);
}

// Results up to this size leave through the export kernel and a polled sequence number (no copy command, no wake-up), larger ones
// by a copy command and the stream wait.
constexpr size_t kExportMax = 65536;

// lay out: scratch slot 0 carved as `r` says; for a host batch also the pinned block as the mirror of its [in | out]
template <class Layout>
static dvs_status lay_out(dvs_matcher* ctx, RansacRegions r, bool cv, int nprob, int total, int H, Layout* d) {
  uint8_t* base;
  DVS_TRY(matcher_scratch(ctx, 0, Layout(nullptr, r, cv, nprob, total, H).bytes + kScratchSlack, (void**)&base));
  *d = Layout(base, r, cv, nprob, total, H);
  return DVS_OK;
}
template <class Layout>
static dvs_status lay_out_batch(dvs_matcher* ctx, bool cv, int nprob, int total, int H, Layout* d, Layout* h, PinnedIo** io) {
  DVS_TRY(lay_out(ctx, kBatchDevice, cv, nprob, total, H, d));
  DVS_TRY(matcher_pinned(ctx, d->inb + d->outb, io));
  *h = Layout((*io)->h(), kBatchPinned, cv, nprob, total, H);
  return DVS_OK;
}

// check: the offsets of a batch rise from 0; its longest problem and its correspondences in all
static dvs_status batch_extent(int32_t nprob, const int32_t* offsets, int* maxn, int* total) {
  DVS_ARG(offsets && offsets[0] == 0);
  *maxn = 0;
  for (int b = 0; b < nprob; b++) { DVS_ARG(offsets[b + 1] >= offsets[b]); *maxn = std::max(*maxn, offsets[b + 1] - offsets[b]); }
  *total = offsets[nprob];
  return DVS_OK;
}
static void pnp_zero_outputs(int32_t nprob, double* rvec3, double* tvec3, int32_t* n_inliers, int32_t* success, int32_t* iterations_run) {
  memset(success, 0, (size_t)nprob * 4);
  if (n_inliers) memset(n_inliers, 0, (size_t)nprob * 4);
  if (iterations_run) memset(iterations_run, 0, (size_t)nprob * 4);
  memset(rvec3, 0, (size_t)nprob * 24); memset(tvec3, 0, (size_t)nprob * 24);
}

// ---- the batch bodies.  `dev` (may be NULL) receives the call's device layout — default, all NULL, where the call returned before any
// launch — for the dvs_test_*_stages hooks at the end of this file.

// the body of dvs_find_fundamental_ransac_batch: problem b = correspondences [offsets[b], offsets[b + 1]) of the concatenated point
// arrays, sampler seed seeds[b]
static dvs_status fm_own_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold,
                               double confidence, int32_t max_iters, const uint64_t* seeds, double* F9, uint8_t* inlier_mask, int32_t* n_inliers,
                               FmLayout* dev = nullptr) {
  if (dev) *dev = FmLayout();
  DVS_ARG(ctx && nprob >= 0 && max_iters >= 1 && max_iters <= kFmMaxIters && threshold > 0);
  if (nprob == 0) return DVS_OK;
  int maxn, total;
  DVS_TRY(batch_extent(nprob, offsets, &maxn, &total));
  DVS_ARG(seeds && (total == 0 || (pts1 && pts2 && inlier_mask)));
  if (n_inliers) memset(n_inliers, 0, (size_t)nprob * 4);
  if (F9) memset(F9, 0, (size_t)nprob * kFmModelBytes);
  if (total) memset(inlier_mask, 0, (size_t)total);
  if (maxn < kFmOwnMinPoints) return DVS_OK;   // cv::findFundamentalMat needs >= 7 points for FM_RANSAC (8 for our kernel): empty F, masks of zeros
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  FmLayout d, h;
  PinnedIo* io;
  DVS_TRY(lay_out_batch(ctx, false, nprob, total, max_iters, &d, &h, &io));
  for (int b = 0; b < nprob; b++) h.probs[b] = RansacProb::seeded(offsets[b], offsets[b + 1] - offsets[b], seeds[b]);
  memcpy(h.p1, pts1, (size_t)total * 8); memcpy(h.p2, pts2, (size_t)total * 8);
  io->import(st, d.probs, d.inb);
  fm_own_pass(st, d, nprob, maxn, d.p1, d.p2, d.mask, max_iters, threshold, confidence);
  if (dev) *dev = d;
  DVS_TRY(io->fetch(st, d.sel, h.sel, d.outb, kExportMax));
  h.unpack(nprob, total, F9, inlier_mask, n_inliers);
  return DVS_OK;
}

// one pass of the OpenCV procedure over a batch of ONE kind (all RANSAC or all LMedS) with the models of the first H iterations;
// unfinished[b] = 1 where the loop wanted more than H (lmeds: where the call FAILED, i.e. fewer than 7 inliers: OpenCV returns an empty
// matrix then, the mask stays as written)
static dvs_status fm_cv_batch_pass(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, const FmCvPolicy& P, int32_t H,
                                   bool lmeds, double* F9, uint8_t* inlier_mask, int32_t* n_inliers, int32_t* iterations, uint8_t* unfinished,
                                   FmLayout* dev = nullptr) {
  int maxn, total;
  DVS_TRY(batch_extent(nprob, offsets, &maxn, &total));
  hipStream_t st = ctx->stream;
  FmLayout d, h;
  PinnedIo* io;
  DVS_TRY(lay_out_batch(ctx, true, nprob, total, H, &d, &h, &io));
  memcpy(h.p1, pts1, (size_t)total * 8); memcpy(h.p2, pts2, (size_t)total * 8);
  fm_cv_pass(st, io, d, h, nprob, offsets, pts1, pts2, maxn, d.p1, d.p2, d.mask, H, lmeds, P);
  if (dev) *dev = d;
  DVS_TRY(io->fetch(st, d.sel, h.sel, d.outb, kExportMax));
  h.unpack(nprob, total, F9, inlier_mask, n_inliers);
  for (int b = 0; b < nprob; b++) {
    const int* sel = h.sel + kSel * b;
    if (iterations) iterations[b] = sel[1];
    unfinished[b] = lmeds ? (uint8_t)(sel[3] ? 0 : 1) : (uint8_t)sel[3];
    if (F9 && lmeds && !sel[3]) memset(F9 + 9 * (size_t)b, 0, kFmModelBytes);   // the call failed: OpenCV returns an empty matrix
  }
  return DVS_OK;
}

// the problems `which` of a batch as a batch of their own (concatenated copies) through one pass, their results written back; `again`
// (may be NULL) collects those the pass left unfinished
static dvs_status fm_cv_subset_pass(dvs_matcher* ctx, const std::vector<int>& which, const int32_t* offsets, const float* pts1, const float* pts2, const FmCvPolicy& P,
                                    int32_t H, bool lmeds, double* F9, uint8_t* inlier_mask, int32_t* n_inliers, int32_t* iterations, std::vector<int>* again) {
  const size_t m = which.size();
  std::vector<int32_t> off(m + 1, 0);
  for (size_t i = 0; i < m; i++) off[i + 1] = off[i] + (offsets[which[i] + 1] - offsets[which[i]]);
  std::vector<float> q1((size_t)off[m] * 2 + 2), q2((size_t)off[m] * 2 + 2);
  for (size_t i = 0; i < m; i++) {
    memcpy(q1.data() + 2 * (size_t)off[i], pts1 + 2 * (size_t)offsets[which[i]], (size_t)(off[i + 1] - off[i]) * 8);
    memcpy(q2.data() + 2 * (size_t)off[i], pts2 + 2 * (size_t)offsets[which[i]], (size_t)(off[i + 1] - off[i]) * 8);
  }
  std::vector<double> F(m * 9, 0.0);
  std::vector<uint8_t> mask((size_t)off[m] + 1, 0), flag(m, 0);
  std::vector<int32_t> nin(m, 0), its(m, 0);
  DVS_TRY(fm_cv_batch_pass(ctx, (int)m, off.data(), q1.data(), q2.data(), P, H, lmeds, F.data(), mask.data(), nin.data(), its.data(), flag.data()));
  for (size_t i = 0; i < m; i++) {
    const int b = which[i];
    memcpy(inlier_mask + offsets[b], mask.data() + off[i], (size_t)(off[i + 1] - off[i]));
    if (n_inliers) n_inliers[b] = nin[i];
    if (iterations) iterations[b] = its[i];
    if (F9) memcpy(F9 + 9 * (size_t)b, F.data() + 9 * i, kFmModelBytes);
    if (again && flag[i]) again->push_back(b);
  }
  return DVS_OK;
}

// the body of dvs_solve_pnp_ransac_batch; inliers: concatenated like the points (problem b's ascending inlier indices at inliers +
// offsets[b], n_inliers[b] of them)
static dvs_status pnp_own_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                int32_t iterations, double reproj_err, double confidence, const uint64_t* seeds, double* rvec3, double* tvec3,
                                int32_t* inliers, int32_t* n_inliers, int32_t* success, PnpLayout* dev = nullptr) {
  if (dev) *dev = PnpLayout();
  DVS_ARG(ctx && nprob >= 0 && iterations >= 1 && iterations <= kPnpMaxIters && K4 && reproj_err > 0);
  if (nprob == 0) return DVS_OK;
  int maxn, total;
  DVS_TRY(batch_extent(nprob, offsets, &maxn, &total));
  DVS_ARG(seeds && rvec3 && tvec3 && success && (total == 0 || (pts3d && pts2d)));
  pnp_zero_outputs(nprob, rvec3, tvec3, n_inliers, success, nullptr);
  if (maxn < kPnpOwnMinPoints) return DVS_OK;   // cv::solvePnPRansac: "npoints >= 4"
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PnpLayout d, h;
  PinnedIo* io;
  DVS_TRY(lay_out_batch(ctx, false, nprob, total, iterations, &d, &h, &io));
  for (int b = 0; b < nprob; b++) h.probs[b] = RansacProb::seeded(offsets[b], offsets[b + 1] - offsets[b], seeds[b]);
  memcpy(h.obj, pts3d, (size_t)total * 12); memcpy(h.img, pts2d, (size_t)total * 8);
  io->import(st, d.probs, d.inb);
  pnp_own_pass(st, d, nprob, d.obj, d.img, d.inl, d.rec, iterations, K4, reproj_err, confidence);
  if (dev) *dev = d;
  DVS_TRY(io->fetch(st, d.rec, h.rec, d.outb, kExportMax));
  h.unpack(nprob, offsets, false, rvec3, tvec3, inliers, n_inliers, success);
  return DVS_OK;
}

// the body of dvs_solve_pnp_ransac_cv_batch: cv::solvePnPRansac(obj, img, K, no distortion, rvec, tvec, false, iterations, reproj_err,
// confidence, inliers) as OpenCV 4.x runs it with its default flags (csrc/pnp_cv.h).  Problems with fewer than 6 points are refused per
// problem (success 0; the reference returns before the call, frontend.cpp:900).  iterations_run[b] = iterations the adaptive loop used
// (may be NULL).
static dvs_status pnp_cv_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                               int32_t iterations, double reproj_err, double confidence, double* rvec3, double* tvec3, int32_t* inliers,
                               int32_t* n_inliers, int32_t* success, int32_t* iterations_run, PnpLayout* dev = nullptr) {
  if (dev) *dev = PnpLayout();
  DVS_ARG(ctx && nprob >= 0 && iterations >= 1 && iterations <= kPnpMaxIters && K4 && reproj_err > 0 && confidence > 0 && confidence < 1);
  if (nprob == 0) return DVS_OK;
  int maxn, total;
  DVS_TRY(batch_extent(nprob, offsets, &maxn, &total));
  DVS_ARG(rvec3 && tvec3 && success && (total == 0 || (pts3d && pts2d)));
  pnp_zero_outputs(nprob, rvec3, tvec3, n_inliers, success, iterations_run);
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PnpLayout d, h;
  PinnedIo* io;
  DVS_TRY(lay_out_batch(ctx, true, nprob, total, iterations, &d, &h, &io));
  memcpy(h.obj, pts3d, (size_t)total * 12); memcpy(h.img, pts2d, (size_t)total * 8);
  pnp_cv_pass(st, io, d, h, nprob, offsets, d.obj, d.img, d.inl, d.rec, d.sel, iterations, K4, reproj_err, confidence);
  if (dev) *dev = d;
  DVS_TRY(io->fetch(st, d.rec, h.rec, d.outb, kExportMax));
  h.unpack(nprob, offsets, true, rvec3, tvec3, inliers, n_inliers, success);
  if (iterations_run) for (int b = 0; b < nprob; b++) iterations_run[b] = h.sel[kSel * b + 1];
  return DVS_OK;
}

// ---- the device forms (ransac_device.h): one problem whose points already live on the device; argument rules as the host entry points'
dvs_status fm_own_device(dvs_matcher* ctx, const float* d_p1, const float* d_p2, const int* d_n, int n_bound, unsigned long long seed, double threshold,
                         double confidence, int max_iters, unsigned char* d_mask) {
  DVS_ARG(ctx && d_p1 && d_p2 && d_n && d_mask && n_bound >= 0 && max_iters >= 1 && max_iters <= kFmMaxIters && threshold > 0);
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  FmLayout d;
  DVS_TRY(lay_out(ctx, kFormDevice, false, 1, 0, max_iters, &d));
  hipLaunchKernelGGL(k_ransac_prob, dim3(1), dim3(1), 0, st, d.probs, d_n, seed);
  fm_own_pass(st, d, 1, n_bound, d_p1, d_p2, d_mask, max_iters, threshold, confidence);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status pnp_own_device(dvs_matcher* ctx, const float* d_obj, const float* d_img, const int* d_n, unsigned long long seed, const double* K4,
                          int iterations, double reproj_err, double confidence, int* d_inl, PnpRecord* d_out) {
  DVS_ARG(ctx && d_obj && d_img && d_n && K4 && d_inl && d_out && iterations >= 1 && iterations <= kPnpMaxIters && reproj_err > 0);
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PnpLayout d;
  DVS_TRY(lay_out(ctx, kFormDevice, false, 1, 0, iterations, &d));
  hipLaunchKernelGGL(k_ransac_prob, dim3(1), dim3(1), 0, st, d.probs, d_n, seed);
  pnp_own_pass(st, d, 1, d_obj, d_img, d_inl, d_out, iterations, K4, reproj_err, confidence);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status fm_cv_device(dvs_matcher* ctx, const float* d_p1, const float* d_p2, int n, double threshold, double confidence, int max_iters,
                        unsigned char* d_mask) {
  DVS_ARG(ctx && d_p1 && d_p2 && d_mask && n >= kFmCvMinPoints && max_iters >= 1 && max_iters <= kFmMaxIters);
  const FmCvPolicy P = fm_cv_policy(threshold, confidence, max_iters);
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool lmeds = P.lmeds(n);
  const int Hfull = lmeds ? P.lmeds_iters() : max_iters;
  // pinned: [pts1 | pts2 | the mirror of a pass's layout, with room for the longest pass]
  float *hp1, *hp2;
  uint8_t* hpass;
  const auto carve = [&](Carver c) {
    c.take(hp1, 2 * (size_t)n); c.take(hp2, 2 * (size_t)n); c.take(hpass, FmLayout(nullptr, kFormPinned, true, 1, 0, Hfull).bytes);
    return c.used;
  };
  PinnedIo* io;
  DVS_TRY(matcher_pinned(ctx, carve(Carver{nullptr, 16}), &io));
  carve(Carver{io->h(), 16});
  DVS_HIP(hipMemcpyAsync(hp1, d_p1, (size_t)n * 8, hipMemcpyDeviceToHost, st));   // what the sampler's collinearity test reads
  DVS_HIP(hipMemcpyAsync(hp2, d_p2, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  const int32_t offsets[2] = {0, n};
  for (int H = lmeds ? Hfull : P.first_pass();; H = max_iters) {
    FmLayout d;
    DVS_TRY(lay_out(ctx, kFormDevice, true, 1, 0, H, &d));
    const FmLayout h(hpass, kFormPinned, true, 1, 0, H);
    fm_cv_pass(st, io, d, h, 1, offsets, hp1, hp2, n, d_p1, d_p2, d_mask, H, lmeds, P);
    DVS_TRY(io->fetch(st, d.sel, h.sel, 16, 16));   // the select record alone: the mask stays on the device
    if (lmeds || !P.wants_full(h.sel, H)) break;
  }
  return DVS_OK;
}

dvs_status pnp_cv_device(dvs_matcher* ctx, const float* d_obj, const float* d_img, int n, const double* K4, int iterations, double reproj_err,
                         double confidence, int* d_inl, PnpRecord* d_out, SelRecord* d_sel) {
  DVS_ARG(ctx && d_obj && d_img && K4 && d_inl && d_out && d_sel && n >= kPnpCvMinPoints && iterations >= 1 && iterations <= kPnpMaxIters && reproj_err > 0 &&
          confidence > 0 && confidence < 1);
  DVS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PnpLayout d;
  DVS_TRY(lay_out(ctx, kFormDevice, true, 1, 0, iterations, &d));
  PinnedIo* io;
  DVS_TRY(matcher_pinned(ctx, d.inb, &io));
  const PnpLayout h(io->h(), kFormPinned, true, 1, 0, iterations);
  const int32_t offsets[2] = {0, n};
  // (returns with the import still reading the block: PinnedIo::reserve waits before it releases one)
  pnp_cv_pass(st, io, d, h, 1, offsets, d_obj, d_img, d_inl, d_out, &d_sel->best, iterations, K4, reproj_err, confidence);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

}  // namespace dvs

using namespace dvs;

extern "C" {

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test.h)
// host-logic test hooks (no GPU): the product's quartic and P3P routines, compiled for the host
int32_t dvs_test_quartic_roots(double a4, double a3, double a2, double a1, double a0, double* roots4) {
  return quartic_real_roots(a4, a3, a2, a1, a0, roots4);
}
int32_t dvs_test_p3p(const double* P9, const double* j9, double* poses48) {
  double P[3][3], j[3][3];
  memcpy(P, P9, sizeof(P)); memcpy(j, j9, sizeof(j));
  return p3p_solve(P, j, poses48);
}
#endif  // DVS_TEST_HOOKS

// ---- batches of independent RANSAC problems (one launch sequence for all of them; the single-problem entry points are batches of one) ----
dvs_status dvs_find_fundamental_ransac_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold,
                                             double confidence, int32_t max_iters, const uint64_t* seeds, double* F9, uint8_t* inlier_mask,
                                             int32_t* n_inliers) {
  return fm_own_batch(ctx, nprob, offsets, pts1, pts2, threshold, confidence, max_iters, seeds, F9, inlier_mask, n_inliers);
}

// cv::findFundamentalMat(FM_RANSAC) the way OpenCV 4.x runs it (see k_f7_hypotheses): RANSAC from 15 correspondences on, LMedS for 8..14
// (OpenCV switches there: k_lmeds_select); fewer than 8 are DVS_ERR_UNSUPPORTED (the reference calls with >= 8, frontend.cpp:627)
dvs_status dvs_find_fundamental_cv_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold,
                                         double confidence, int32_t max_iters, double* F9, uint8_t* inlier_mask, int32_t* n_inliers, int32_t* iterations) {
  DVS_ARG(ctx && nprob >= 0 && max_iters >= 1 && max_iters <= kFmMaxIters);
  if (nprob == 0) return DVS_OK;
  DVS_ARG(offsets && offsets[0] == 0 && pts1 && pts2 && inlier_mask);
  const FmCvPolicy P = fm_cv_policy(threshold, confidence, max_iters);
  std::vector<int> big, small, again;
  for (int b = 0; b < nprob; b++) {
    DVS_ARG(offsets[b + 1] >= offsets[b]);
    const int n = offsets[b + 1] - offsets[b];
    if (n < kFmCvMinPoints) { set_error("dvs_find_fundamental_cv: problem %d has %d correspondences (the reference calls with >= 8, frontend.cpp:627)", b, n); return DVS_ERR_UNSUPPORTED; }
    (P.lmeds(n) ? small : big).push_back(b);
  }
  DVS_HIP(hipSetDevice(ctx->device));
  if (!big.empty()) DVS_TRY(fm_cv_subset_pass(ctx, big, offsets, pts1, pts2, P, P.first_pass(), false, F9, inlier_mask, n_inliers, iterations, &again));
  if (!again.empty() && P.first_pass() < max_iters)
    DVS_TRY(fm_cv_subset_pass(ctx, again, offsets, pts1, pts2, P, max_iters, false, F9, inlier_mask, n_inliers, iterations, nullptr));
  if (!small.empty()) DVS_TRY(fm_cv_subset_pass(ctx, small, offsets, pts1, pts2, P, P.lmeds_iters(), true, F9, inlier_mask, n_inliers, iterations, nullptr));
  return DVS_OK;
}

dvs_status dvs_find_fundamental_cv(dvs_matcher* ctx, const float* pts1, const float* pts2, int32_t n, double threshold, double confidence,
                                   int32_t max_iters, double* F9, uint8_t* inlier_mask, int32_t* n_inliers, int32_t* iterations) {
  DVS_ARG(ctx && n >= 0);
  const int32_t offsets[2] = {0, n};
  return dvs_find_fundamental_cv_batch(ctx, 1, offsets, pts1, pts2, threshold, confidence, max_iters, F9, inlier_mask, n_inliers, iterations);
}

// host only (no GPU): the sample sequence of the call above — iteration it draws idx[7 it .. 7 it + 6]; *found = iterations that have one
// (pts1 = pts2 = NULL: a callback without checkSubset, as cv::solvePnPRansac's)
dvs_status dvs_cv_ransac_subsets(const float* pts1, const float* pts2, int32_t n, int32_t model_points, int32_t iterations, int32_t* idx, int32_t* found) {
  DVS_ARG(idx && found && n >= model_points && model_points >= 1 && model_points <= 16 && iterations >= 0 && (pts1 == nullptr) == (pts2 == nullptr));
  *found = cv_subsets(pts1, pts2, n, model_points, iterations, idx);
  return DVS_OK;
}

dvs_status dvs_solve_pnp_ransac_cv_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                         int32_t iterations, double reproj_err, double confidence, double* rvec3, double* tvec3, int32_t* inliers,
                                         int32_t* n_inliers, int32_t* success, int32_t* iterations_run) {
  return pnp_cv_batch(ctx, nprob, offsets, pts3d, pts2d, K4, iterations, reproj_err, confidence, rvec3, tvec3, inliers, n_inliers, success, iterations_run);
}

dvs_status dvs_solve_pnp_ransac_cv(dvs_matcher* ctx, const float* pts3d, const float* pts2d, int32_t n, const double* K4, int32_t iterations,
                                   double reproj_err, double confidence, double* rvec3, double* tvec3, int32_t* inliers, int32_t* n_inliers,
                                   int32_t* success, int32_t* iterations_run) {
  DVS_ARG(ctx && n >= 0 && rvec3 && tvec3 && success);
  const int32_t offsets[2] = {0, n};
  return dvs_solve_pnp_ransac_cv_batch(ctx, 1, offsets, pts3d, pts2d, K4, iterations, reproj_err, confidence, rvec3, tvec3, inliers, n_inliers, success,
                                       iterations_run);
}

dvs_status dvs_find_fundamental_ransac(dvs_matcher* ctx, const float* pts1, const float* pts2, int32_t n, double threshold, double confidence,
                                       int32_t max_iters, uint64_t seed, double* F9, uint8_t* inlier_mask, int32_t* n_inliers) {
  DVS_ARG(ctx && n >= 0 && (inlier_mask || n == 0));
  const int32_t offsets[2] = {0, n};
  return dvs_find_fundamental_ransac_batch(ctx, 1, offsets, pts1, pts2, threshold, confidence, max_iters, &seed, F9, inlier_mask, n_inliers);
}

dvs_status dvs_solve_pnp_ransac_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                      int32_t iterations, double reproj_err, double confidence, const uint64_t* seeds, double* rvec3, double* tvec3,
                                      int32_t* inliers, int32_t* n_inliers, int32_t* success) {
  return pnp_own_batch(ctx, nprob, offsets, pts3d, pts2d, K4, iterations, reproj_err, confidence, seeds, rvec3, tvec3, inliers, n_inliers, success);
}

dvs_status dvs_solve_pnp_ransac(dvs_matcher* ctx, const float* pts3d, const float* pts2d, int32_t n, const double* K4, int32_t iterations,
                                double reproj_err, double confidence, uint64_t seed, double* rvec3, double* tvec3, int32_t* inliers,
                                int32_t* n_inliers, int32_t* success) {
  DVS_ARG(ctx && n >= 0 && rvec3 && tvec3 && success);
  const int32_t offsets[2] = {0, n};
  return dvs_solve_pnp_ransac_batch(ctx, 1, offsets, pts3d, pts2d, K4, iterations, reproj_err, confidence, &seed, rvec3, tvec3, inliers, n_inliers, success);
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test.h): the stages of the two own estimators, one by one
// the product call (fm_own_batch: same import, same launches, same grids) and, beside its results, what each stage left on the device,
// read through the layout the call hands back
dvs_status dvs_test_fm_stages(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold, double confidence,
                              int32_t H, const uint64_t* seeds, double* F_all, int32_t* valid, int32_t* counts, int32_t* sel, uint8_t* mask, double* Fbest) {
  DVS_ARG(ctx && nprob >= 1 && H >= 1 && offsets && F_all && valid && counts && sel && Fbest);
  FmLayout dev;
  DVS_TRY(fm_own_batch(ctx, nprob, offsets, pts1, pts2, threshold, confidence, H, seeds, Fbest, mask, nullptr, &dev));
  const size_t nh = (size_t)nprob * H;
  if (!dev.models) {   // no problem had 8 points: nothing ran
    memset(F_all, 0, nh * kFmModelBytes); memset(valid, 0, nh * 4); memset(counts, 0, nh * 4);
    for (int b = 0; b < nprob; b++) { sel[4 * b] = -1; sel[4 * b + 1] = sel[4 * b + 2] = sel[4 * b + 3] = 0; }
    return DVS_OK;
  }
  DVS_HIP(hipMemcpy(F_all, dev.models, nh * kFmModelBytes, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(valid, dev.valid, nh * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(counts, dev.counts, nh * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel, dev.sel, (size_t)nprob * 16, hipMemcpyDeviceToHost));
  // k_f_hypotheses writes no model for a problem of fewer than 8 points (its `valid` says so): zeros, not what the scratch block held
  for (int b = 0; b < nprob; b++) if (offsets[b + 1] - offsets[b] < 8) memset(F_all + 9 * (size_t)H * b, 0, (size_t)H * kFmModelBytes);
  return DVS_OK;
}

dvs_status dvs_test_pnp_stages(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4, double reproj_err,
                               double confidence, int32_t H, const uint64_t* seeds, double* poses, int32_t* valid, int32_t* counts, int32_t* sel,
                               int32_t* inliers, int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3) {
  DVS_ARG(ctx && nprob >= 1 && H >= 1 && offsets && poses && valid && counts && sel && n_inliers && success && rvec3 && tvec3);
  PnpLayout dev;
  DVS_TRY(pnp_own_batch(ctx, nprob, offsets, pts3d, pts2d, K4, H, reproj_err, confidence, seeds, rvec3, tvec3, inliers, n_inliers, success, &dev));
  const size_t nh = (size_t)nprob * 4 * H;
  if (!dev.models) {   // no problem had 4 points: nothing ran
    memset(poses, 0, nh * kPosePnpBytes); memset(valid, 0, nh * 4); memset(counts, 0, nh * 4);
    for (int b = 0; b < nprob; b++) { sel[4 * b] = -1; sel[4 * b + 1] = sel[4 * b + 2] = sel[4 * b + 3] = 0; }
    return DVS_OK;
  }
  DVS_HIP(hipMemcpy(poses, dev.models, nh * kPosePnpBytes, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(valid, dev.valid, nh * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(counts, dev.counts, nh * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel, dev.sel, (size_t)nprob * 16, hipMemcpyDeviceToHost));
  return DVS_OK;
}

// k_ransac_select alone on counts of the caller's (H of them, H a multiple of `group`), in the own estimators' form
dvs_status dvs_test_ransac_select(const int32_t* counts, int32_t H, int32_t n, int32_t model_points, double confidence, int32_t group, int32_t* sel4) {
  DVS_ARG(counts && sel4 && H >= 1 && n >= 1 && model_points >= 1 && group >= 1 && H % group == 0);
  DeviceBuf<int> dc, ds; DeviceBuf<RansacProb> dp;
  DVS_TRY(dc.upload(std::vector<int>(counts, counts + H)));
  DVS_TRY(dp.upload(std::vector<RansacProb>(1, RansacProb::seeded(0, n, 0ull))));
  DVS_TRY(ds.alloc(4));
  hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(1), 0, 0, dc.get(), H, dp.get(), model_points, confidence, group, ds.get(), 0, 0);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipMemcpy(sel4, ds.get(), 16, hipMemcpyDeviceToHost));
  return DVS_OK;
}

// k_pnp_refine alone on ONE problem with a pose of the caller's as the selected one (pose12 = R row-major, t; NULL: nothing selected,
// sel[0] = -1), grid and block as pnp_own_pass's for one problem.  What pnp_own_pass cannot reach: select takes no pose with fewer
// than 3 inliers, so the kernel's "fewer than 3 inliers: no LM step" path never runs through it.  inliers: room for n indices.
dvs_status dvs_test_pnp_refine(const float* pts3d, const float* pts2d, int32_t n, const double* K4, const double* pose12, double reproj_err,
                               int32_t* inliers, int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3) {
  DVS_ARG(pts3d && pts2d && n >= 1 && K4 && reproj_err > 0 && inliers && n_inliers && success && rvec3 && tvec3);
  DeviceBuf<float> dobj, dimg; DeviceBuf<RansacProb> dp; DeviceBuf<double> dpose; DeviceBuf<int> dsel, dinl; DeviceBuf<PnpRecord> dres;
  DVS_TRY(dobj.upload(std::vector<float>(pts3d, pts3d + 3 * (size_t)n)));
  DVS_TRY(dimg.upload(std::vector<float>(pts2d, pts2d + 2 * (size_t)n)));
  DVS_TRY(dp.upload(std::vector<RansacProb>(1, RansacProb::seeded(0, n, 0ull))));
  DVS_TRY(dpose.upload(pose12 ? std::vector<double>(pose12, pose12 + 12) : std::vector<double>(12, 0.0)));
  DVS_TRY(dsel.upload(std::vector<int>{pose12 ? 0 : -1, 1, 0, 0}));
  DVS_TRY(dinl.upload(std::vector<int>((size_t)n, -1)));
  DVS_TRY(dres.alloc(1));
  hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(256), 0, 0, dobj.get(), dimg.get(), dp.get(), 1, dpose.get(), dsel.get(), K4[0], K4[1], K4[2], K4[3],
                     reproj_err * reproj_err, dinl.get(), dres.get());
  DVS_HIP(hipGetLastError());
  PnpRecord res;
  DVS_HIP(hipMemcpy(&res, dres.get(), sizeof(res), hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(inliers, dinl.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  *n_inliers = res.n_inliers; *success = res.success; memcpy(rvec3, res.rvec, sizeof(res.rvec)); memcpy(tvec3, res.tvec, sizeof(res.tvec));
  return DVS_OK;
}

// host only (no GPU): the conversion that ends k_pnp_refine
void dvs_test_rotation_to_rodrigues(const double* R9, double* w3) { rotation_to_rodrigues(R9, w3); }

// ---- the OpenCV-procedure forms (include/dvslam_hip_test_ransac_cv.h; tests/test_gpu_ransac_cv_stages.py)
// ONE fm_cv_batch_pass with the models of H iterations (the product's passes: H = min(max_iters, 96), then max_iters where the loop asked; LMedS:
// the fixed count) and, beside its results, what every stage left on the device.  A batch is of one kind — all problems >= 15 points
// (RANSAC) or all 8 .. 14 (LMedS: no counts, zeros) — as the product's passes are.
dvs_status dvs_test_fm_cv_stages(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold,
                                 double confidence, int32_t max_iters, int32_t H, int32_t* samples, int32_t* found, double* F_all, int32_t* valid,
                                 int32_t* counts, int32_t* sel, uint8_t* mask, double* Fbest) {
  DVS_ARG(ctx && nprob >= 1 && H >= 1 && max_iters >= 1 && offsets && offsets[0] == 0 && pts1 && pts2 && threshold > 0 && samples && found && F_all && valid &&
          counts && sel && mask && Fbest);
  int nsmall = 0;
  for (int b = 0; b < nprob; b++) {
    const int n = offsets[b + 1] - offsets[b];
    DVS_ARG(n >= 8);
    nsmall += FmCvPolicy::lmeds(n) ? 1 : 0;
  }
  DVS_ARG(nsmall == 0 || nsmall == nprob);
  const bool lmeds = nsmall != 0;
  DVS_HIP(hipSetDevice(ctx->device));
  std::vector<uint8_t> flag(nprob);
  FmLayout dev;
  DVS_TRY(fm_cv_batch_pass(ctx, nprob, offsets, pts1, pts2, FmCvPolicy{threshold, confidence, max_iters}, H, lmeds, nullptr, mask, nullptr, nullptr, flag.data(), &dev));
  const size_t nh = (size_t)nprob * H;
  std::vector<RansacProb> probs(nprob);
  DVS_HIP(hipMemcpy(probs.data(), dev.probs, (size_t)nprob * sizeof(RansacProb), hipMemcpyDeviceToHost));
  for (int b = 0; b < nprob; b++) found[b] = probs[b].sampled_iterations();
  DVS_HIP(hipMemcpy(samples, dev.samples, nh * 28, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(F_all, dev.models, nh * kF7Roots * kFmModelBytes, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(valid, dev.valid, nh * 12, hipMemcpyDeviceToHost));
  if (lmeds) memset(counts, 0, nh * 12);
  else DVS_HIP(hipMemcpy(counts, dev.counts, nh * 12, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel, dev.sel, (size_t)nprob * 16, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(Fbest, dev.F, (size_t)nprob * kFmModelBytes, hipMemcpyDeviceToHost));
  // k_f7_hypotheses writes no model into a slot it marks invalid (its `valid` says so): zeros, not what the scratch block held
  for (size_t m = 0; m < 3 * nh; m++) if (!valid[m]) memset(F_all + 9 * m, 0, kFmModelBytes);
  return DVS_OK;
}

// the body of dvs_solve_pnp_ransac_cv_batch with iterations = H and what every stage left on the device: models[b][H][18] (rvec, tvec, R,
// pad), counts[b][H], sel[b][4], the samples the host drew (zeros for a refused problem)
dvs_status dvs_test_pnp_cv_stages(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                  double reproj_err, double confidence, int32_t H, int32_t* samples, double* models, int32_t* counts, int32_t* sel,
                                  int32_t* inliers, int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3) {
  DVS_ARG(ctx && nprob >= 1 && H >= 1 && offsets && samples && models && counts && sel && n_inliers && success && rvec3 && tvec3);
  PnpLayout dev;
  DVS_TRY(pnp_cv_batch(ctx, nprob, offsets, pts3d, pts2d, K4, H, reproj_err, confidence, rvec3, tvec3, inliers, n_inliers, success, nullptr, &dev));
  DVS_ARG(dev.models != nullptr);
  const size_t nh = (size_t)nprob * H;
  DVS_HIP(hipMemcpy(samples, dev.samples, nh * 20, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(models, dev.models, nh * kModelPnpCvBytes, hipMemcpyDeviceToHost));
  for (size_t m = 0; m < nh; m++) models[18 * m + 15] = models[18 * m + 16] = models[18 * m + 17] = 0.0;   // the pad: no kernel writes it
  DVS_HIP(hipMemcpy(counts, dev.counts, nh * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel, dev.sel, (size_t)nprob * 16, hipMemcpyDeviceToHost));
  return DVS_OK;
}

// k_ransac_select alone in the OpenCV-procedure form (capInSeed = 1): counts of H models, `group` per iteration (H a multiple of it), of a
// loop of up to max_iters_true iterations of which getSubset found a sample for `found`
dvs_status dvs_test_ransac_select_cv(const int32_t* counts, int32_t H, int32_t n, int32_t model_points, double confidence, int32_t group, int32_t found,
                                     int32_t max_iters_true, int32_t* sel4) {
  DVS_ARG(counts && sel4 && H >= 1 && n >= 1 && model_points >= 1 && group >= 1 && H % group == 0 && found >= 0 && max_iters_true >= 1);
  DeviceBuf<int> dc, ds; DeviceBuf<RansacProb> dp;
  DVS_TRY(dc.upload(std::vector<int>(counts, counts + H)));
  DVS_TRY(dp.upload(std::vector<RansacProb>(1, RansacProb::sampled(0, n, found))));
  DVS_TRY(ds.alloc(4));
  hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(1), 0, 0, dc.get(), H, dp.get(), model_points, confidence, group, ds.get(), 1, max_iters_true);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipMemcpy(sel4, ds.get(), 16, hipMemcpyDeviceToHost));
  return DVS_OK;
}

// k_pnpcv_refit alone on ONE problem with a model of the caller's as the selected one (model6 = rvec, tvec — the rotation matrix the
// hypothesis kernel stores beside it is made here, by the same routine; NULL: nothing selected, sel[0] = -1), grid and block as
// pnp_cv_pass's for one problem.  inliers: room for n indices (-1 where none was written).  dbg8: see k_pnpcv_refit.
static __global__ void k_test_pnpcv_model(const double* __restrict__ model6, double* __restrict__ m18) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double R[9];
  const double rv[3] = {model6[0], model6[1], model6[2]};
  pnpcv::rodrigues_vec(rv, R, nullptr);
  for (int k = 0; k < 6; k++) m18[k] = model6[k];
  for (int k = 0; k < 9; k++) m18[6 + k] = R[k];
  for (int k = 15; k < 18; k++) m18[k] = 0.0;
}
dvs_status dvs_test_pnpcv_refit(const float* pts3d, const float* pts2d, int32_t n, const double* K4, const double* model6, double reproj_err, int32_t* inliers,
                                int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3, double* dbg8) {
  DVS_ARG(pts3d && pts2d && n >= 1 && K4 && reproj_err > 0 && inliers && n_inliers && success && rvec3 && tvec3 && dbg8);
  DeviceBuf<float> dobj, dimg; DeviceBuf<RansacProb> dp; DeviceBuf<double> dm6, dm18, ddbg; DeviceBuf<int> dsel, dinl; DeviceBuf<PnpRecord> dres;
  DVS_TRY(dobj.upload(std::vector<float>(pts3d, pts3d + 3 * (size_t)n)));
  DVS_TRY(dimg.upload(std::vector<float>(pts2d, pts2d + 2 * (size_t)n)));
  DVS_TRY(dp.upload(std::vector<RansacProb>(1, RansacProb::sampled(0, n, 1))));
  DVS_TRY(dm6.upload(model6 ? std::vector<double>(model6, model6 + 6) : std::vector<double>(6, 0.0)));
  DVS_TRY(dm18.upload(std::vector<double>(18, 0.0)));
  DVS_TRY(ddbg.upload(std::vector<double>(8, -1.0)));
  DVS_TRY(dsel.upload(std::vector<int>{model6 ? 0 : -1, 1, 0, 0}));
  DVS_TRY(dinl.upload(std::vector<int>((size_t)n, -1)));
  DVS_TRY(dres.alloc(1));
  DVS_HIP(hipMemset(dres.get(), 0xff, sizeof(PnpRecord)));
  if (model6) hipLaunchKernelGGL(k_test_pnpcv_model, dim3(1), dim3(1), 0, 0, dm6.get(), dm18.get());
  hipLaunchKernelGGL(k_pnpcv_refit, dim3(1), dim3(64), 0, 0, dobj.get(), dimg.get(), dp.get(), 1, dm18.get(), dsel.get(), K4[0], K4[1], K4[2], K4[3],
                     (float)(reproj_err * reproj_err), dinl.get(), dres.get(), ddbg.get());
  DVS_HIP(hipGetLastError());
  PnpRecord res;
  DVS_HIP(hipMemcpy(&res, dres.get(), sizeof(res), hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(inliers, dinl.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(dbg8, ddbg.get(), 64, hipMemcpyDeviceToHost));
  *n_inliers = res.n_inliers; *success = res.success; memcpy(rvec3, res.rvec, sizeof(res.rvec)); memcpy(tvec3, res.tvec, sizeof(res.tvec));
  return DVS_OK;
}

// ---- the device forms (include/dvslam_hip_test_ransac_device.h; tests/test_gpu_ransac_device_forms.py): one problem uploaded, the chosen
// form of ransac_device.h run on it, what that form writes downloaded (0xff bytes where it wrote nothing)
dvs_status dvs_test_ransac_device_form(dvs_matcher* ctx, int32_t form, const float* pts_a, const float* pts_b, int32_t n, int32_t cap, const double* K4,
                                       int32_t iters, double threshold, double confidence, uint64_t seed, uint8_t* mask, uint8_t* rec64, int32_t* inliers,
                                       int32_t* sel4) {
  const bool fm = form == 0 || form == 1;
  DVS_ARG(ctx && form >= 0 && form <= 3 && n >= 0 && cap >= std::max(n, 1) && (n == 0 || (pts_a && pts_b)));
  DVS_ARG(fm ? mask != nullptr : K4 && rec64 && inliers && (form == 2 || sel4));
  const size_t wa = fm ? 2 : 3;
  std::vector<float> a((size_t)cap * wa, 0.f), b((size_t)cap * 2, 0.f);
  if (n) { memcpy(a.data(), pts_a, (size_t)n * wa * 4); memcpy(b.data(), pts_b, (size_t)n * 8); }
  DeviceBuf<float> da, db; DeviceBuf<int> dn, dinl; DeviceBuf<SelRecord> dsel; DeviceBuf<unsigned char> dmask; DeviceBuf<PnpRecord> drec;
  DVS_TRY(da.upload(a)); DVS_TRY(db.upload(b));
  DVS_TRY(dn.upload(std::vector<int>(1, n)));
  DVS_TRY(dmask.upload(std::vector<unsigned char>((size_t)cap, 0xff)));
  DVS_TRY(drec.alloc(1));
  DVS_HIP(hipMemset(drec.get(), 0xff, sizeof(PnpRecord)));
  DVS_TRY(dinl.upload(std::vector<int>((size_t)cap, -1)));
  DVS_TRY(dsel.upload(std::vector<SelRecord>(1, SelRecord{-1, -1, -1, -1})));
  if (form == 0) DVS_TRY(fm_own_device(ctx, da.get(), db.get(), dn.get(), cap, seed, threshold, confidence, iters, dmask.get()));
  if (form == 1) DVS_TRY(fm_cv_device(ctx, da.get(), db.get(), n, threshold, confidence, iters, dmask.get()));
  if (form == 2) DVS_TRY(pnp_own_device(ctx, da.get(), db.get(), dn.get(), seed, K4, iters, threshold, confidence, dinl.get(), drec.get()));
  if (form == 3) DVS_TRY(pnp_cv_device(ctx, da.get(), db.get(), n, K4, iters, threshold, confidence, dinl.get(), drec.get(), dsel.get()));
  DVS_HIP(hipStreamSynchronize(ctx->stream));
  if (fm) DVS_HIP(hipMemcpy(mask, dmask.get(), (size_t)cap, hipMemcpyDeviceToHost));
  else {
    DVS_HIP(hipMemcpy(rec64, drec.get(), kPnpRecord, hipMemcpyDeviceToHost));
    DVS_HIP(hipMemcpy(inliers, dinl.get(), (size_t)cap * 4, hipMemcpyDeviceToHost));
    if (form == 3) DVS_HIP(hipMemcpy(sel4, dsel.get(), sizeof(SelRecord), hipMemcpyDeviceToHost));
  }
  return DVS_OK;
}
#endif  // DVS_TEST_HOOKS

}  // extern "C"
