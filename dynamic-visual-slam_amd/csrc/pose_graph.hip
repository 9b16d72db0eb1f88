// pose_graph.hip — pose-graph optimisation over all keyframes and the map correction that follows a verified loop (dvs_pgo_*; the rule is
// stated in include/dvslam_hip.h "Pose-graph optimisation").  FP64 throughout.  Launches of one Levenberg-Marquardt trial step, all on
// the handle's stream with no host read-back between them:
//   k_pgo_lm_diag      D = clamp(diag(H), 1e-6, 1e32) per free node (skipped after a rejected step: the diagonal is kept)
//   k_pgo_precond      the 6 x 6 diagonal blocks of H + D / radius, inverted by Cholesky, one thread per node
//   k_pgo_pcg          the whole preconditioned CG solve in ONE workgroup: vectors in global memory, workgroup barriers between the
//                      phases of an iteration, the stopping test on the device.  Any N and E run (a thread strides over nodes / edges);
//                      there is no grid-wide barrier and nothing that needs more than one resident workgroup.
//   k_pgo_candidate    q <- q * exp(omega), t <- t + R v per node, the candidate's R, and the step / parameter norms' per-node terms
//   k_pgo_trial_edges  the candidate's residuals (cost only) and the model term |A x_i + B x_j|^2 per edge
//   k_pgo_trial_reduce the sums, folded in a fixed order, into the ONE status record the host reads per trial step
// and after an accepted step k_pgo_linearize (one thread per edge), k_pgo_nodes (gradient and diagonal blocks: a node's incident edges
// in ascending edge index) and k_pgo_state_reduce (cost, max |g|), whose record the NEXT trial's read brings along.
// The trust-region policy and the verdict on a trial step are trust_region.h's, shared with the bundle adjustment's solvers.
#include <math.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "block_ops.h"
#include "common.h"
#include "device_mem.h"
#include "trust_region.h"
#ifdef DVS_TEST_HOOKS
#include "../../include/dvslam_hip_test.h"
#endif

namespace {
using namespace dvs;

constexpr int kPcgThreads = 512;
constexpr int kMaxNodes = 1 << 20, kMaxEdges = 1 << 22;

struct PgoStatus {          // device -> host, once per trial step
  double cur_cost, gmax;    // of the current linearisation (k_pgo_state_reduce)
  double cand_cost, model_cost_change, step2, x2;   // of the trial (k_pgo_trial_reduce)
  double rnorm, gnorm;      // of the linear solve (k_pgo_pcg)
  int32_t pcg_iterations, finite, breakdown, pad;
};

struct PgoDev {             // what the kernels see
  int N, E;
  const int32_t *ei, *ej, *nodeStart, *inc;
  const uint8_t* fixed;
  const double* meas;       // [E][14]: R_z (9, row-major), t_z (3), w_rot, w_trans
  double *res, *A, *B, *ecost, *emodel;   // [E][6], [E][36], [E][36], [E], [E]
  double *g, *Hd, *D, *Minv;              // [N][6], [N][36], [N][6], [N][36]
  double *x, *r, *z, *p, *y, *u;          // PCG vectors [6N] and the per-edge product [E][6]
  double* nodePart;                       // [N][2]
  PgoStatus* status;
};

// ------------------------------------------------------------------------------------------------ small dense pieces
__host__ __device__ inline void quat_to_R(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// residual of one edge and what the Jacobian blocks are made of: M = R_i^T R_j, Q = R_z^T M, omega = Log(Q), p = R_i^T (t_j - t_i)
__device__ inline void edge_residual(const double* Ri, const double* ti, const double* Rj, const double* tj, const double* m, double* r,
                                     double* M, double* Q, double* om, double* theta, double* p) {
  const double* Rz = m; const double* tz = m + 9;
  const double wr = m[12], wt = m[13];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) M[3 * a + b] = Ri[a] * Rj[b] + Ri[3 + a] * Rj[3 + b] + Ri[6 + a] * Rj[6 + b];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Q[3 * a + b] = Rz[a] * M[b] + Rz[3 + a] * M[3 + b] + Rz[6 + a] * M[6 + b];
  const double v0 = (Q[7] - Q[5]) / 2, v1 = (Q[2] - Q[6]) / 2, v2 = (Q[3] - Q[1]) / 2;
  const double s = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  const double c = (Q[0] + Q[4] + Q[8] - 1) / 2;
  const double th = atan2(s, c);
  const double k = s > 1e-12 ? th / s : 1.0;
  om[0] = v0 * k; om[1] = v1 * k; om[2] = v2 * k;
  *theta = th;
  const double d0 = tj[0] - ti[0], d1 = tj[1] - ti[1], d2 = tj[2] - ti[2];
#pragma unroll
  for (int a = 0; a < 3; a++) p[a] = Ri[a] * d0 + Ri[3 + a] * d1 + Ri[6 + a] * d2;
  const double e0 = p[0] - tz[0], e1 = p[1] - tz[1], e2 = p[2] - tz[2];
#pragma unroll
  for (int a = 0; a < 3; a++) { r[a] = wr * om[a]; r[3 + a] = wt * (Rz[a] * e0 + Rz[3 + a] * e1 + Rz[6 + a] * e2); }
}

// u_e = A_e p_i + B_e p_j
__device__ inline void edge_product(const PgoDev& P, int e, const double* vec) {
  const double* A = P.A + 36 * (size_t)e; const double* B = P.B + 36 * (size_t)e;
  const double* pi = vec + 6 * (size_t)P.ei[e]; const double* pj = vec + 6 * (size_t)P.ej[e];
  double a[6], b[6];
#pragma unroll
  for (int c = 0; c < 6; c++) { a[c] = pi[c]; b[c] = pj[c]; }
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) s += A[6 * r + c] * a[c];
#pragma unroll
    for (int c = 0; c < 6; c++) s += B[6 * r + c] * b[c];
    P.u[6 * (size_t)e + r] = s;
  }
}
// y_n = sum over n's incident edges, ascending edge index, of (A_e or B_e)^T u_e, plus (D_n / radius) p_n; zero on a fixed node
__device__ inline void node_gather(const PgoDev& P, int n, double radius, const double* vec, double* out) {
  double acc[6] = {0, 0, 0, 0, 0, 0};
  if (!P.fixed[n]) {
    for (int k = P.nodeStart[n]; k < P.nodeStart[n + 1]; k++) {
      const int code = P.inc[k], e = code >> 1;
      const double* blk = ((code & 1) ? P.B : P.A) + 36 * (size_t)e;
      const double* u = P.u + 6 * (size_t)e;
#pragma unroll
      for (int r = 0; r < 6; r++) {
        const double ur = u[r];
#pragma unroll
        for (int c = 0; c < 6; c++) acc[c] += blk[6 * r + c] * ur;
      }
    }
#pragma unroll
    for (int c = 0; c < 6; c++) acc[c] += (P.D[6 * (size_t)n + c] / radius) * vec[6 * (size_t)n + c];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) out[c] = acc[c];
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ void k_pgo_R_from_q(int N, const double* q, double* R) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) quat_to_R(q + 4 * (size_t)n, R + 9 * (size_t)n);
}

__global__ __launch_bounds__(256) void k_pgo_linearize(PgoDev P, const double* R, const double* t) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.E) return;
  const int i = P.ei[e], j = P.ej[e];
  const double* m = P.meas + 14 * (size_t)e;
  double r[6], M[9], Q[9], om[3], th, p[3];
  edge_residual(R + 9 * (size_t)i, t + 3 * (size_t)i, R + 9 * (size_t)j, t + 3 * (size_t)j, m, r, M, Q, om, &th, p);
  double c2 = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) { P.res[6 * (size_t)e + a] = r[a]; c2 += r[a] * r[a]; }
  P.ecost[e] = c2;
  // Jr^-1(omega) = I + [omega]x / 2 + c [omega]x^2
  double c;
  if (th < 1e-2) { const double t2 = th * th; c = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0; }
  else c = 1.0 / (th * th) - (1.0 + cos(th)) / (2.0 * th * sin(th));
  const double W[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
  double Ji[9];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++)
      Ji[3 * a + b] = (a == b ? 1.0 : 0.0) + W[3 * a + b] / 2 + c * (W[3 * a] * W[b] + W[3 * a + 1] * W[3 + b] + W[3 * a + 2] * W[6 + b]);
  const double wr = m[12], wt = m[13];
  double A[36], B[36];
#pragma unroll
  for (int k = 0; k < 36; k++) { A[k] = 0; B[k] = 0; }
  if (!P.fixed[i]) {
    const double px[9] = {0, -p[2], p[1], p[2], 0, -p[0], -p[1], p[0], 0};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) {
        A[6 * a + b] = -wr * (Ji[3 * a] * M[3 * b] + Ji[3 * a + 1] * M[3 * b + 1] + Ji[3 * a + 2] * M[3 * b + 2]);     // -w_rot Jr^-1 M^T
        A[6 * (3 + a) + b] = wt * (m[a] * px[b] + m[3 + a] * px[3 + b] + m[6 + a] * px[6 + b]);                          // w_trans R_z^T [p]x
        A[6 * (3 + a) + 3 + b] = -wt * m[3 * b + a];                                                                      // -w_trans R_z^T
      }
  }
  if (!P.fixed[j]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) { B[6 * a + b] = wr * Ji[3 * a + b]; B[6 * (3 + a) + 3 + b] = wt * Q[3 * a + b]; }
  }
#pragma unroll
  for (int k = 0; k < 36; k++) { P.A[36 * (size_t)e + k] = A[k]; P.B[36 * (size_t)e + k] = B[k]; }
}

// gradient and 6 x 6 diagonal block of H per node
__global__ __launch_bounds__(256) void k_pgo_nodes(PgoDev P) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= P.N) return;
  double g[6] = {0, 0, 0, 0, 0, 0}, H[36];
#pragma unroll
  for (int k = 0; k < 36; k++) H[k] = 0;
  if (!P.fixed[n]) {
    for (int k = P.nodeStart[n]; k < P.nodeStart[n + 1]; k++) {
      const int code = P.inc[k], e = code >> 1;
      const double* blk = ((code & 1) ? P.B : P.A) + 36 * (size_t)e;
      const double* r = P.res + 6 * (size_t)e;
#pragma unroll
      for (int row = 0; row < 6; row++) {
        double b[6];
#pragma unroll
        for (int c = 0; c < 6; c++) b[c] = blk[6 * row + c];
        const double rr = r[row];
#pragma unroll
        for (int c = 0; c < 6; c++) {
          g[c] += b[c] * rr;
#pragma unroll
          for (int d = 0; d < 6; d++) H[6 * c + d] += b[c] * b[d];
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 6; c++) P.g[6 * (size_t)n + c] = g[c];
#pragma unroll
  for (int k = 0; k < 36; k++) P.Hd[36 * (size_t)n + k] = H[k];
}

__global__ __launch_bounds__(kPcgThreads) void k_pgo_state_reduce(PgoDev P) {
  __shared__ double sh[kPcgThreads];
  double c = 0, m = 0;
  for (int e = threadIdx.x; e < P.E; e += kPcgThreads) c += P.ecost[e];
  for (int n = threadIdx.x; n < P.N; n += kPcgThreads)
    if (!P.fixed[n])
      for (int a = 0; a < 6; a++) m = fmax(m, fabs(P.g[6 * (size_t)n + a]));
  c = block_sum<kPcgThreads>(c, sh);
  m = block_max<kPcgThreads>(m, sh);
  if (threadIdx.x == 0) { P.status->cur_cost = 0.5 * c; P.status->gmax = m; }
}

__global__ void k_pgo_lm_diag(PgoDev P) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= 6 * P.N) return;
  const int n = k / 6, a = k % 6;
  P.D[k] = P.fixed[n] ? 0.0 : fmin(fmax(P.Hd[36 * (size_t)n + 7 * a], 1e-6), 1e32);
}

// Minv_n = (H_nn + D_n / radius)^-1 by Cholesky (L, L^-1, L^-T L^-1); zero on a fixed node; the inverse of the diagonal alone if the
// factorisation meets a pivot that is not positive
__global__ __launch_bounds__(256) void k_pgo_precond(PgoDev P, double radius) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= P.N) return;
  double* out = P.Minv + 36 * (size_t)n;
  if (P.fixed[n]) { for (int k = 0; k < 36; k++) out[k] = 0; return; }
  double L[36], Li[36], dg[6];
#pragma unroll
  for (int k = 0; k < 36; k++) { L[k] = P.Hd[36 * (size_t)n + k]; Li[k] = 0; }
#pragma unroll
  for (int a = 0; a < 6; a++) { L[7 * a] += P.D[6 * (size_t)n + a] / radius; dg[a] = L[7 * a]; }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = L[7 * j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= L[6 * j + k] * L[6 * j + k];
    if (!(d > 0)) ok = false;
    d = sqrt(d);
    L[7 * j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = L[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s / d;
    }
  }
  // L^-1, column by column
#pragma unroll
  for (int c = 0; c < 6; c++) {
#pragma unroll
    for (int i = c; i < 6; i++) {
      double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = c; k < i; k++) s -= L[6 * i + k] * Li[6 * k + c];
      Li[6 * i + c] = s / L[7 * i];
    }
  }
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) if (k >= a && k >= b) s += Li[6 * k + a] * Li[6 * k + b];
      out[6 * a + b] = ok ? s : (a == b ? 1.0 / dg[a] : 0.0);
    }
}

__device__ inline double precond_row_dot(const PgoDev& P, int n, const double* rv, double* zv) {   // z_n = Minv_n r_n; returns r_n . z_n
  const double* Mi = P.Minv + 36 * (size_t)n;
  double r[6], s = 0;
#pragma unroll
  for (int c = 0; c < 6; c++) r[c] = rv[6 * (size_t)n + c];
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double z = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) z += Mi[6 * a + c] * r[c];
    zv[6 * (size_t)n + a] = z;
    s += r[a] * z;
  }
  return s;
}

// (H + D / radius) x = -g by block-Jacobi preconditioned conjugate gradients from x = 0, one workgroup.  Stops at the first iteration k
// with |r_k| <= eta |g| (k = 0 included: a zero gradient gives x = 0 in 0 iterations) or at max_it.
__global__ __launch_bounds__(kPcgThreads) void k_pgo_pcg(PgoDev P, double radius, double eta, int max_it) {
  __shared__ double sh[kPcgThreads];
  const int tid = threadIdx.x;
  double part = 0;
  for (int n = tid; n < P.N; n += kPcgThreads)
    for (int c = 0; c < 6; c++) {
      const size_t k = 6 * (size_t)n + c;
      const double v = P.fixed[n] ? 0.0 : -P.g[k];
      P.r[k] = v; P.x[k] = 0; P.p[k] = 0;
      part += v * v;
    }
  const double gnorm = sqrt(block_sum<kPcgThreads>(part, sh));
  double rnorm = gnorm;
  int it = 0, breakdown = 0;
  if (!(rnorm <= eta * gnorm) && max_it > 0) {
    part = 0;
    for (int n = tid; n < P.N; n += kPcgThreads) {
      part += precond_row_dot(P, n, P.r, P.z);
      for (int c = 0; c < 6; c++) P.p[6 * (size_t)n + c] = P.z[6 * (size_t)n + c];
    }
    double rz = block_sum<kPcgThreads>(part, sh);
    for (;;) {
      __syncthreads();   // p of every node is written
      for (int e = tid; e < P.E; e += kPcgThreads) edge_product(P, e, P.p);
      __syncthreads();
      part = 0;
      for (int n = tid; n < P.N; n += kPcgThreads) {
        double y[6];
        node_gather(P, n, radius, P.p, y);
        for (int c = 0; c < 6; c++) { P.y[6 * (size_t)n + c] = y[c]; part += P.p[6 * (size_t)n + c] * y[c]; }
      }
      const double pAp = block_sum<kPcgThreads>(part, sh);
      if (!(pAp > 0) || !isfinite(pAp)) { breakdown = 1; break; }
      const double alpha = rz / pAp;
      part = 0;
      for (int n = tid; n < P.N; n += kPcgThreads)
        for (int c = 0; c < 6; c++) {
          const size_t k = 6 * (size_t)n + c;
          P.x[k] = P.x[k] + alpha * P.p[k];
          const double rv = P.r[k] - alpha * P.y[k];
          P.r[k] = rv;
          part += rv * rv;
        }
      rnorm = sqrt(block_sum<kPcgThreads>(part, sh));
      it++;
      if (rnorm <= eta * gnorm || it >= max_it) break;
      part = 0;
      for (int n = tid; n < P.N; n += kPcgThreads) part += precond_row_dot(P, n, P.r, P.z);
      const double rz2 = block_sum<kPcgThreads>(part, sh);
      const double beta = rz2 / rz;
      rz = rz2;
      for (int n = tid; n < P.N; n += kPcgThreads)
        for (int c = 0; c < 6; c++) { const size_t k = 6 * (size_t)n + c; P.p[k] = P.z[k] + beta * P.p[k]; }
    }
  }
  if (tid == 0) { P.status->pcg_iterations = it; P.status->rnorm = rnorm; P.status->gnorm = gnorm; P.status->breakdown = breakdown; }
}

// the operator alone on P.p -> P.y (dvs_test_pgo_apply), through the same two device functions the solve uses
__global__ __launch_bounds__(kPcgThreads) void k_pgo_apply(PgoDev P, double radius) {
  for (int e = threadIdx.x; e < P.E; e += kPcgThreads) edge_product(P, e, P.p);
  __syncthreads();
  for (int n = threadIdx.x; n < P.N; n += kPcgThreads) {
    double y[6];
    node_gather(P, n, radius, P.p, y);
    for (int c = 0; c < 6; c++) P.y[6 * (size_t)n + c] = y[c];
  }
}

// candidate pose per node: q' = normalised q * exp(omega), t' = t + R v with the R before the step, R' from q'
__global__ __launch_bounds__(256) void k_pgo_candidate(PgoDev P, const double* q, const double* t, const double* R, double* qc, double* tc, double* Rc) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= P.N) return;
  const double* qn = q + 4 * (size_t)n; const double* tn = t + 3 * (size_t)n; const double* Rn = R + 9 * (size_t)n;
  double qo[4] = {qn[0], qn[1], qn[2], qn[3]}, to[3] = {tn[0], tn[1], tn[2]};
  double step2 = 0, x2 = 0;
  if (!P.fixed[n]) {
    const double* d = P.x + 6 * (size_t)n;
    const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    double e[4] = {1, 0, 0, 0};
    if (th != 0) { const double s = sin(th / 2) / th; e[0] = cos(th / 2); e[1] = s * d[0]; e[2] = s * d[1]; e[3] = s * d[2]; }
    double m[4];
    m[0] = qn[0] * e[0] - qn[1] * e[1] - qn[2] * e[2] - qn[3] * e[3];
    m[1] = qn[0] * e[1] + qn[1] * e[0] + qn[2] * e[3] - qn[3] * e[2];
    m[2] = qn[0] * e[2] - qn[1] * e[3] + qn[2] * e[0] + qn[3] * e[1];
    m[3] = qn[0] * e[3] + qn[1] * e[2] - qn[2] * e[1] + qn[3] * e[0];
    const double nm = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3]);
    for (int a = 0; a < 4; a++) qo[a] = m[a] / nm;
    for (int a = 0; a < 3; a++) to[a] = tn[a] + (Rn[3 * a] * d[3] + Rn[3 * a + 1] * d[4] + Rn[3 * a + 2] * d[5]);
    for (int a = 0; a < 4; a++) { step2 += (qo[a] - qn[a]) * (qo[a] - qn[a]); x2 += qn[a] * qn[a]; }
    for (int a = 0; a < 3; a++) { step2 += (to[a] - tn[a]) * (to[a] - tn[a]); x2 += tn[a] * tn[a]; }
  }
  for (int a = 0; a < 4; a++) qc[4 * (size_t)n + a] = qo[a];
  for (int a = 0; a < 3; a++) tc[3 * (size_t)n + a] = to[a];
  quat_to_R(qo, Rc + 9 * (size_t)n);
  P.nodePart[2 * (size_t)n] = step2; P.nodePart[2 * (size_t)n + 1] = x2;
}

// per edge: the candidate's |r|^2, and |A x_i + B x_j|^2 at the current linearisation
__global__ __launch_bounds__(256) void k_pgo_trial_edges(PgoDev P, const double* Rc, const double* tc) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.E) return;
  const int i = P.ei[e], j = P.ej[e];
  double r[6], M[9], Q[9], om[3], th, p[3];
  edge_residual(Rc + 9 * (size_t)i, tc + 3 * (size_t)i, Rc + 9 * (size_t)j, tc + 3 * (size_t)j, P.meas + 14 * (size_t)e, r, M, Q, om, &th, p);
  double c2 = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) c2 += r[a] * r[a];
  P.ecost[e] = c2;
  edge_product(P, e, P.x);
  double m2 = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) { const double u = P.u[6 * (size_t)e + a]; m2 += u * u; }
  P.emodel[e] = m2;
}

__global__ __launch_bounds__(kPcgThreads) void k_pgo_trial_reduce(PgoDev P) {
  __shared__ double sh[6 * kPcgThreads];   // 24 KB: the six sums through one tree
  double c = 0, m = 0, xg = 0, s2 = 0, x2 = 0;
  int finite = 1;
  for (int e = threadIdx.x; e < P.E; e += kPcgThreads) { c += P.ecost[e]; m += P.emodel[e]; }
  for (int n = threadIdx.x; n < P.N; n += kPcgThreads) {
    for (int a = 0; a < 6; a++) { const double xv = P.x[6 * (size_t)n + a]; xg += xv * P.g[6 * (size_t)n + a]; if (!isfinite(xv)) finite = 0; }
    s2 += P.nodePart[2 * (size_t)n]; x2 += P.nodePart[2 * (size_t)n + 1];
  }
  double v[6] = {c, m, xg, s2, x2, finite ? 0.0 : 1.0};
  block_sums<kPcgThreads, 6>(v, sh);
  if (threadIdx.x == 0) {
    P.status->cand_cost = 0.5 * v[0]; P.status->model_cost_change = -(v[2] + 0.5 * v[1]); P.status->step2 = v[3]; P.status->x2 = v[4];
    P.status->finite = v[5] == 0.0 ? 1 : 0;
  }
}

// x' = R'_a (R_a^T (x - t_a)) + t'_a, FP64 in that order, one rounding to float; anchors outside [0, N) leave the point as it is
__global__ __launch_bounds__(256) void k_pgo_correct_points(int N, int n, const double* R0, const double* t0, const double* R1, const double* t1,
                                                            float* xyz, const int32_t* anchor) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int a = anchor[k];
  if (a < 0 || a >= N) return;
  const double* Ra = R0 + 9 * (size_t)a; const double* ta = t0 + 3 * (size_t)a;
  const double* Rb = R1 + 9 * (size_t)a; const double* tb = t1 + 3 * (size_t)a;
  float* x = xyz + 3 * (size_t)k;
  const double d0 = (double)x[0] - ta[0], d1 = (double)x[1] - ta[1], d2 = (double)x[2] - ta[2];
  double y[3];
#pragma unroll
  for (int c = 0; c < 3; c++) y[c] = Ra[c] * d0 + Ra[3 + c] * d1 + Ra[6 + c] * d2;
#pragma unroll
  for (int c = 0; c < 3; c++) x[c] = (float)(Rb[3 * c] * y[0] + Rb[3 * c + 1] * y[1] + Rb[3 * c + 2] * y[2] + tb[c]);
}

// ------------------------------------------------------------------------------------------------ host side
void rodrigues_to_R(const double* w, double* R) {   // cos I + (1 - cos) k k^T + sin [k]x; the identity for the zero vector
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (th == 0) { for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0; return; }
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const double c = cos(th), s = sin(th);
  const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) R[3 * a + b] = c * (a == b ? 1.0 : 0.0) + (1 - c) * (k[a] * k[b]) + s * K[3 * a + b];
}

void quat_from_R(const double* R, double* q) {      // by the largest of the four (Shepperd), normalised
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) {
    const double s = sqrt(tr + 1.0) * 2;
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int a = 0; a < 4; a++) q[a] /= n;
}

bool all_finite(const double* v, size_t n) {
  for (size_t k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
  return true;
}

dvs_status check_nodes(int32_t N, const double* R, const double* t, const uint8_t* fixed) {
  if (N < 1 || N > kMaxNodes) { set_error("pose graph: %d nodes (1 .. %d)", N, kMaxNodes); return DVS_ERR_ARG; }
  DVS_ARG(R && t && fixed);
  if (!all_finite(R, 9 * (size_t)N) || !all_finite(t, 3 * (size_t)N)) { set_error("pose graph: a node pose is not finite"); return DVS_ERR_ARG; }
  bool any = false;
  for (int n = 0; n < N; n++) any = any || fixed[n];
  if (!any) { set_error("pose graph: no fixed node (the gauge is free)"); return DVS_ERR_ARG; }
  return DVS_OK;
}
dvs_status check_edges(int32_t N, int32_t E, const int32_t* i, const int32_t* j, const double* rvec, const double* tvec, const double* w_rot,
                       const double* w_trans) {
  if (E < 1 || E > kMaxEdges) { set_error("pose graph: %d edges (1 .. %d)", E, kMaxEdges); return DVS_ERR_ARG; }
  DVS_ARG(i && j && rvec && tvec && w_rot && w_trans);
  for (int e = 0; e < E; e++) {
    if (i[e] < 0 || i[e] >= N || j[e] < 0 || j[e] >= N || i[e] == j[e]) { set_error("pose graph: edge %d joins %d and %d of %d nodes", e, i[e], j[e], N); return DVS_ERR_ARG; }
    if (!(w_rot[e] > 0) || !(w_trans[e] > 0) || !std::isfinite(w_rot[e]) || !std::isfinite(w_trans[e])) { set_error("pose graph: edge %d has a weight that is not > 0 and finite", e); return DVS_ERR_ARG; }
  }
  if (!all_finite(rvec, 3 * (size_t)E) || !all_finite(tvec, 3 * (size_t)E)) { set_error("pose graph: an edge measurement is not finite"); return DVS_ERR_ARG; }
  return DVS_OK;
}

}  // namespace

struct dvs_pgo {
  int device = 0;
  Stream stream;   // declared before the blocks: it outlives them
  int N = 0, E = 0;
  // host copies
  std::vector<double> R0, t0, q, t;          // "before" as given; the current quaternion and translation
  std::vector<uint8_t> fixed;
  std::vector<int32_t> ei, ej, nodeStart, inc;
  std::vector<double> meas;
  bool nodes_dirty = false, edges_dirty = false, lin_valid = false;
  // device
  DeviceBuf<double> dR0, dt0, dq, dt, dR, dqc, dtc, dRc, dmeas, dres, dA, dB, decost, demodel, dg, dHd, dD, dMinv, dx, dr, dz, dp, dy, du, dnodePart;
  DeviceBuf<uint8_t> dfixed;
  DeviceBuf<int32_t> dei, dej, dnodeStart, dinc;
  DeviceBuf<PgoStatus> dstatus;
  PinnedBuf<PgoStatus> hstatus;
  DeviceBuf<float> pts; DeviceBuf<int32_t> anchors; size_t pts_cap = 0, anchors_cap = 0;
  double *q_cur = nullptr, *t_cur = nullptr, *R_cur = nullptr, *q_cand = nullptr, *t_cand = nullptr, *R_cand = nullptr;
  std::vector<double> trace;   // 7 per row
  void log(double radius, const StepVerdict& v, const TrialRecord& r, int pcg) {
    const double row[7] = {radius, (double)v.kind, v.cost_change, r.model_change, v.rel, v.kind == kStepInvalid ? 0.0 : r.cand_cost, (double)pcg};
    trace.insert(trace.end(), row, row + 7);
  }
};

namespace {

inline dim3 grid_for(int n) { return dim3((unsigned)((n + 255) / 256)); }

PgoDev dev_view(dvs_pgo* h) {
  PgoDev P;
  P.N = h->N; P.E = h->E;
  P.ei = h->dei.get(); P.ej = h->dej.get(); P.nodeStart = h->dnodeStart.get(); P.inc = h->dinc.get();
  P.fixed = h->dfixed.get(); P.meas = h->dmeas.get();
  P.res = h->dres.get(); P.A = h->dA.get(); P.B = h->dB.get(); P.ecost = h->decost.get(); P.emodel = h->demodel.get();
  P.g = h->dg.get(); P.Hd = h->dHd.get(); P.D = h->dD.get(); P.Minv = h->dMinv.get();
  P.x = h->dx.get(); P.r = h->dr.get(); P.z = h->dz.get(); P.p = h->dp.get(); P.y = h->dy.get(); P.u = h->du.get();
  P.nodePart = h->dnodePart.get(); P.status = h->dstatus.get();
  return P;
}

// uploads what set_nodes / set_edges left on the host; allocates what the kernels need
dvs_status prepare(dvs_pgo* h, bool need_edges) {
  DVS_HIP(hipSetDevice(h->device));
  if (h->N == 0) { set_error("pose graph: dvs_pgo_set_nodes has not been called"); return DVS_ERR_ARG; }
  if (need_edges && h->E == 0) { set_error("pose graph: dvs_pgo_set_edges has not been called"); return DVS_ERR_ARG; }
  const size_t N = h->N, E = h->E;
  if (h->nodes_dirty) {
    DVS_HIP(hipStreamSynchronize(h->stream));
    DVS_TRY(h->dR0.upload(h->R0)); DVS_TRY(h->dt0.upload(h->t0)); DVS_TRY(h->dq.upload(h->q)); DVS_TRY(h->dt.upload(h->t));
    DVS_TRY(h->dfixed.upload(h->fixed));
    DVS_TRY(h->dR.alloc(9 * N)); DVS_TRY(h->dqc.alloc(4 * N)); DVS_TRY(h->dtc.alloc(3 * N)); DVS_TRY(h->dRc.alloc(9 * N));
    DVS_TRY(h->dg.alloc(6 * N)); DVS_TRY(h->dHd.alloc(36 * N)); DVS_TRY(h->dD.alloc(6 * N)); DVS_TRY(h->dMinv.alloc(36 * N));
    DVS_TRY(h->dx.alloc(6 * N)); DVS_TRY(h->dr.alloc(6 * N)); DVS_TRY(h->dz.alloc(6 * N)); DVS_TRY(h->dp.alloc(6 * N)); DVS_TRY(h->dy.alloc(6 * N));
    DVS_TRY(h->dnodePart.alloc(2 * N));
    if (!h->dstatus.get()) { DVS_TRY(h->dstatus.alloc(1)); DVS_TRY(h->hstatus.alloc(1)); }
    DVS_HIP(hipMemsetAsync(h->dstatus.get(), 0, sizeof(PgoStatus), h->stream));
    h->q_cur = h->dq.get(); h->t_cur = h->dt.get(); h->R_cur = h->dR.get();
    h->q_cand = h->dqc.get(); h->t_cand = h->dtc.get(); h->R_cand = h->dRc.get();
    hipLaunchKernelGGL(k_pgo_R_from_q, grid_for(h->N), dim3(256), 0, h->stream, h->N, h->q_cur, h->R_cur);
    DVS_HIP(hipGetLastError());
    h->nodes_dirty = false; h->lin_valid = false;
  }
  if (h->edges_dirty && E) {
    DVS_HIP(hipStreamSynchronize(h->stream));
    DVS_TRY(h->dei.upload(h->ei)); DVS_TRY(h->dej.upload(h->ej)); DVS_TRY(h->dnodeStart.upload(h->nodeStart)); DVS_TRY(h->dinc.upload(h->inc));
    DVS_TRY(h->dmeas.upload(h->meas));
    DVS_TRY(h->dres.alloc(6 * E)); DVS_TRY(h->dA.alloc(36 * E)); DVS_TRY(h->dB.alloc(36 * E)); DVS_TRY(h->decost.alloc(E)); DVS_TRY(h->demodel.alloc(E));
    DVS_TRY(h->du.alloc(6 * E));
    h->edges_dirty = false; h->lin_valid = false;
  }
  return DVS_OK;
}

// residuals, blocks, gradient, diagonal blocks, cost and max |g| of the current poses
void enqueue_linearize(dvs_pgo* h) {
  const PgoDev P = dev_view(h);
  hipLaunchKernelGGL(k_pgo_linearize, grid_for(h->E), dim3(256), 0, h->stream, P, h->R_cur, h->t_cur);
  hipLaunchKernelGGL(k_pgo_nodes, grid_for(h->N), dim3(256), 0, h->stream, P);
  hipLaunchKernelGGL(k_pgo_state_reduce, dim3(1), dim3(kPcgThreads), 0, h->stream, P);
  h->lin_valid = true;
}

// the launches of ONE trial step at `radius`, from the current linearisation: the LM diagonal (kept when the step before was rejected),
// the preconditioner, the linear solve, the candidate and its record.  dvs_pgo_solve's loop and dvs_test_pgo_trial_step both enqueue a
// trial through this function; given_x (the hook only) leaves the linear solve out and takes the step that is already in P.x.
void enqueue_trial(dvs_pgo* h, double radius, double eta, int max_pcg, bool reuse_diagonal, bool given_x = false) {
  const PgoDev P = dev_view(h);
  const int N = h->N, E = h->E;
  hipStream_t st = h->stream;
  if (!reuse_diagonal) hipLaunchKernelGGL(k_pgo_lm_diag, grid_for(6 * N), dim3(256), 0, st, P);
  hipLaunchKernelGGL(k_pgo_precond, grid_for(N), dim3(256), 0, st, P, radius);
  if (!given_x) hipLaunchKernelGGL(k_pgo_pcg, dim3(1), dim3(kPcgThreads), 0, st, P, radius, eta, max_pcg);
  hipLaunchKernelGGL(k_pgo_candidate, grid_for(N), dim3(256), 0, st, P, h->q_cur, h->t_cur, h->R_cur, h->q_cand, h->t_cand, h->R_cand);
  hipLaunchKernelGGL(k_pgo_trial_edges, grid_for(E), dim3(256), 0, st, P, h->R_cand, h->t_cand);
  hipLaunchKernelGGL(k_pgo_trial_reduce, dim3(1), dim3(kPcgThreads), 0, st, P);
}

// an accepted step: the candidate becomes the point (the two sets of buffers change roles) and is linearised
void commit_candidate(dvs_pgo* h) {
  std::swap(h->q_cur, h->q_cand); std::swap(h->t_cur, h->t_cand); std::swap(h->R_cur, h->R_cand);
  enqueue_linearize(h);
}

dvs_status read_status(dvs_pgo* h, PgoStatus* out) {
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipMemcpyAsync(h->hstatus.get(), h->dstatus.get(), sizeof(PgoStatus), hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  *out = *h->hstatus.get();
  return DVS_OK;
}

dvs_status download_poses(dvs_pgo* h) {
  DVS_HIP(hipMemcpy(h->q.data(), h->q_cur, h->q.size() * 8, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(h->t.data(), h->t_cur, h->t.size() * 8, hipMemcpyDeviceToHost));
  return DVS_OK;
}

bool params_ok(const dvs_pgo_params* p) {
  return p->max_iterations >= 0 && p->max_pcg_iterations >= 0 && std::isfinite(p->function_tolerance) && p->function_tolerance >= 0 &&
         std::isfinite(p->gradient_tolerance) && p->gradient_tolerance >= 0 && std::isfinite(p->parameter_tolerance) && p->parameter_tolerance >= 0 &&
         std::isfinite(p->eta) && p->eta > 0 && p->eta < 1;
}

}  // namespace

extern "C" {

dvs_status dvs_pgo_default_params(dvs_pgo_params* p) {
  DVS_ARG(p);
  p->max_iterations = 50; p->max_pcg_iterations = 0;
  p->function_tolerance = 1e-6; p->gradient_tolerance = 1e-10; p->parameter_tolerance = 1e-8; p->eta = 0.1;
  return DVS_OK;
}

dvs_status dvs_pgo_check_graph(int32_t N, const double* R, const double* t, const uint8_t* fixed, int32_t E, const int32_t* i, const int32_t* j,
                               const double* rvec, const double* tvec, const double* w_rot, const double* w_trans) {
  DVS_TRY(check_nodes(N, R, t, fixed));
  return check_edges(N, E, i, j, rvec, tvec, w_rot, w_trans);
}

dvs_status dvs_pgo_create(int32_t device, dvs_pgo** out) {
  DVS_ARG(out);
  *out = nullptr;
  DVS_TRY(check_device(device));
  dvs_pgo* h = new (std::nothrow) dvs_pgo();
  if (!h) { set_error("out of host memory"); return DVS_ERR_HIP; }
  h->device = device;
  const hipError_t e = h->stream.create();
  if (e != hipSuccess) { delete h; set_error("hipStreamCreate: %s", hipGetErrorString(e)); return DVS_ERR_HIP; }
  *out = h;
  return DVS_OK;
}

void dvs_pgo_destroy(dvs_pgo* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;
}

dvs_status dvs_pgo_synchronize(dvs_pgo* h) {
  DVS_ARG(h);
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->stream));
  return DVS_OK;
}

dvs_status dvs_pgo_set_nodes(dvs_pgo* h, int32_t N, const double* R, const double* t, const uint8_t* fixed) {
  DVS_ARG(h);
  DVS_TRY(check_nodes(N, R, t, fixed));
  if (N != h->N) { h->E = 0; h->ei.clear(); h->ej.clear(); }   // edges of another node count no longer apply
  h->N = N;
  h->R0.assign(R, R + 9 * (size_t)N); h->t0.assign(t, t + 3 * (size_t)N); h->t = h->t0;
  h->fixed.resize(N);
  for (int n = 0; n < N; n++) h->fixed[n] = fixed[n] ? 1 : 0;
  h->q.resize(4 * (size_t)N);
  for (int n = 0; n < N; n++) quat_from_R(R + 9 * (size_t)n, &h->q[4 * (size_t)n]);
  h->nodes_dirty = true; h->lin_valid = false;
  h->trace.clear();
  return DVS_OK;
}

dvs_status dvs_pgo_set_edges(dvs_pgo* h, int32_t E, const int32_t* i, const int32_t* j, const double* rvec, const double* tvec, const double* w_rot,
                             const double* w_trans) {
  DVS_ARG(h);
  if (h->N == 0) { set_error("pose graph: dvs_pgo_set_nodes comes first"); return DVS_ERR_ARG; }
  DVS_TRY(check_edges(h->N, E, i, j, rvec, tvec, w_rot, w_trans));
  const int N = h->N;
  h->E = E;
  h->ei.assign(i, i + E); h->ej.assign(j, j + E);
  h->meas.resize(14 * (size_t)E);
  for (int e = 0; e < E; e++) {
    double* m = &h->meas[14 * (size_t)e];
    rodrigues_to_R(rvec + 3 * (size_t)e, m);
    for (int a = 0; a < 3; a++) m[9 + a] = tvec[3 * (size_t)e + a];
    m[12] = w_rot[e]; m[13] = w_trans[e];
  }
  // node -> incident (edge, side) lists, ascending edge index: the order every per-node sum folds in
  h->nodeStart.assign(N + 1, 0);
  for (int e = 0; e < E; e++) { h->nodeStart[i[e] + 1]++; h->nodeStart[j[e] + 1]++; }
  for (int n = 0; n < N; n++) h->nodeStart[n + 1] += h->nodeStart[n];
  h->inc.assign(2 * (size_t)E, 0);
  std::vector<int32_t> cur(h->nodeStart.begin(), h->nodeStart.end() - 1);
  for (int e = 0; e < E; e++) { h->inc[cur[i[e]]++] = 2 * e; h->inc[cur[j[e]]++] = 2 * e + 1; }
  h->edges_dirty = true; h->lin_valid = false;
  return DVS_OK;
}

dvs_status dvs_pgo_evaluate(dvs_pgo* h, double* cost, double* residuals, double* Ji, double* Jj, double* grad) {
  DVS_ARG(h);
  DVS_TRY(prepare(h, true));
  enqueue_linearize(h);
  PgoStatus st;
  DVS_TRY(read_status(h, &st));
  const size_t N = h->N, E = h->E;
  if (cost) *cost = st.cur_cost;
  if (residuals) DVS_HIP(hipMemcpy(residuals, h->dres.get(), 6 * E * 8, hipMemcpyDeviceToHost));
  if (Ji) DVS_HIP(hipMemcpy(Ji, h->dA.get(), 36 * E * 8, hipMemcpyDeviceToHost));
  if (Jj) DVS_HIP(hipMemcpy(Jj, h->dB.get(), 36 * E * 8, hipMemcpyDeviceToHost));
  if (grad) DVS_HIP(hipMemcpy(grad, h->dg.get(), 6 * N * 8, hipMemcpyDeviceToHost));
  return DVS_OK;
}

dvs_status dvs_pgo_solve(dvs_pgo* h, const dvs_pgo_params* params, dvs_pgo_summary* summary) {
  DVS_ARG(h && summary);
  dvs_pgo_params prm;
  dvs_pgo_default_params(&prm);
  if (params) prm = *params;
  DVS_ARG(params_ok(&prm));
  memset(summary, 0, sizeof(*summary));
  summary->termination = 2;
  DVS_TRY(prepare(h, true));
  const int max_pcg = prm.max_pcg_iterations > 0 ? prm.max_pcg_iterations : std::max(100, 2 * h->N);
  hipStream_t st = h->stream;
  h->trace.clear();
  enqueue_linearize(h);
  PgoStatus s;
  DVS_TRY(read_status(h, &s));
  double x_cost = s.cur_cost;
  summary->initial_cost = x_cost;
  TrustRegion tr;
  while (go_on(tr.before_trial(prm.max_iterations), &summary->termination)) {
    const double radius = tr.radius;
    enqueue_trial(h, radius, prm.eta, max_pcg, tr.reuse_diagonal);
    DVS_TRY(read_status(h, &s));
    // the gradient test of the loop head, on the record this read brought along: the trial enqueued above is dropped, uncounted
    if (!go_on(tr.count_trial(s.gmax, prm.gradient_tolerance), &summary->termination)) break;
    summary->pcg_iterations += s.pcg_iterations;
    const TrialRecord rec = {s.finite, s.model_cost_change, s.cand_cost, s.step2, s.x2};
    const StepVerdict v = verdict_host_decides(rec, x_cost, prm.parameter_tolerance, prm.function_tolerance);
    h->log(radius, v, rec, s.pcg_iterations);
    if (!go_on(tr.update(v), &summary->termination)) break;
    if (v.kind == kStepAccepted) {
      commit_candidate(h);    // its cost and max |g| arrive with the next trial's record
      x_cost = rec.cand_cost;
      summary->num_successful_steps++;
    }
  }
  summary->num_iterations = tr.iteration;
  summary->final_cost = x_cost;
  DVS_HIP(hipStreamSynchronize(st));
  DVS_HIP(hipGetLastError());
  return download_poses(h);
}

dvs_status dvs_pgo_get_nodes(dvs_pgo* h, double* R, double* t) {
  DVS_ARG(h);
  DVS_TRY(prepare(h, false));
  DVS_HIP(hipStreamSynchronize(h->stream));
  if (R) DVS_HIP(hipMemcpy(R, h->R_cur, 9 * (size_t)h->N * 8, hipMemcpyDeviceToHost));
  if (t) DVS_HIP(hipMemcpy(t, h->t_cur, 3 * (size_t)h->N * 8, hipMemcpyDeviceToHost));
  return DVS_OK;
}

dvs_status dvs_pgo_get_trace(const dvs_pgo* h, double* rows, int32_t cap_rows, int32_t* n_rows) {
  DVS_ARG(h && n_rows && cap_rows >= 0);
  const int n = (int)(h->trace.size() / 7);
  *n_rows = n;
  if (rows) memcpy(rows, h->trace.data(), (size_t)std::min(n, cap_rows) * 7 * sizeof(double));
  return DVS_OK;
}

dvs_status dvs_pgo_correct_points_device(dvs_pgo* h, int32_t n, float* d_xyz, const int32_t* d_anchor) {
  DVS_ARG(h && n >= 0 && (n == 0 || (d_xyz && d_anchor)));
  DVS_TRY(prepare(h, false));
  if (n == 0) return DVS_OK;
  hipLaunchKernelGGL(k_pgo_correct_points, grid_for(n), dim3(256), 0, h->stream, h->N, n, h->dR0.get(), h->dt0.get(), h->R_cur, h->t_cur, d_xyz, d_anchor);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status dvs_pgo_correct_points(dvs_pgo* h, int32_t n, float* xyz, const int32_t* anchor) {
  DVS_ARG(h && n >= 0 && (n == 0 || (xyz && anchor)));
  DVS_TRY(prepare(h, false));
  if (n == 0) return DVS_OK;
  DVS_HIP(hipStreamSynchronize(h->stream));
  DVS_TRY(grow(h->pts, h->pts_cap, 3 * (size_t)n)); DVS_TRY(grow(h->anchors, h->anchors_cap, (size_t)n));
  DVS_HIP(hipMemcpyAsync(h->pts.get(), xyz, 3 * (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  DVS_HIP(hipMemcpyAsync(h->anchors.get(), anchor, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  DVS_TRY(dvs_pgo_correct_points_device(h, n, h->pts.get(), h->anchors.get()));
  DVS_HIP(hipMemcpyAsync(xyz, h->pts.get(), 3 * (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  return DVS_OK;
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test_pgo.h)
DVS_HOOK dvs_status dvs_test_pgo_apply(dvs_pgo* h, double radius, const double* p, double* y) {
  DVS_ARG(h && p && y && radius > 0);
  DVS_TRY(prepare(h, true));
  if (!h->lin_valid) enqueue_linearize(h);
  const PgoDev P = dev_view(h);
  const size_t bytes = 6 * (size_t)h->N * 8;
  hipLaunchKernelGGL(k_pgo_lm_diag, grid_for(6 * h->N), dim3(256), 0, h->stream, P);
  DVS_HIP(hipMemcpyAsync(P.p, p, bytes, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_pgo_apply, dim3(1), dim3(kPcgThreads), 0, h->stream, P, radius);
  DVS_HIP(hipGetLastError());
  DVS_HIP(hipMemcpyAsync(y, P.y, bytes, hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  return DVS_OK;
}

DVS_HOOK dvs_status dvs_test_pgo_pcg(dvs_pgo* h, double radius, double eta, int32_t max_it, double* x, int32_t* iterations, double* rnorm, double* gnorm) {
  DVS_ARG(h && x && radius > 0 && eta > 0 && max_it >= 0);
  DVS_TRY(prepare(h, true));
  if (!h->lin_valid) enqueue_linearize(h);
  const PgoDev P = dev_view(h);
  hipLaunchKernelGGL(k_pgo_lm_diag, grid_for(6 * h->N), dim3(256), 0, h->stream, P);
  hipLaunchKernelGGL(k_pgo_precond, grid_for(h->N), dim3(256), 0, h->stream, P, radius);
  hipLaunchKernelGGL(k_pgo_pcg, dim3(1), dim3(kPcgThreads), 0, h->stream, P, radius, eta, (int)max_it);
  PgoStatus s;
  DVS_TRY(read_status(h, &s));
  DVS_HIP(hipMemcpy(x, P.x, 6 * (size_t)h->N * 8, hipMemcpyDeviceToHost));
  if (iterations) *iterations = s.pcg_iterations;
  if (rnorm) *rnorm = s.rnorm;
  if (gnorm) *gnorm = s.gnorm;
  return DVS_OK;
}

// ONE trial step through enqueue_trial / read_status / commit_candidate, the three functions dvs_pgo_solve's loop is made of
DVS_HOOK dvs_status dvs_test_pgo_trial_step(dvs_pgo* h, double radius, double eta, int32_t max_pcg_iterations, int32_t reuse_diagonal, int32_t commit,
                                            const double* x_in, double* cur_q, double* cur_t, double* x, double* D, double* cand_q, double* cand_t,
                                            dvs_pgo_step_record* rec) {
  static_assert(sizeof(dvs_pgo_step_record) == sizeof(PgoStatus), "the hook's record is the status record");
  DVS_ARG(h && radius > 0 && eta > 0 && eta < 1 && max_pcg_iterations >= 0);
  DVS_TRY(prepare(h, true));
  if (!h->lin_valid) enqueue_linearize(h);
  const PgoDev P = dev_view(h);
  const size_t N = h->N;
  const int max_pcg = max_pcg_iterations > 0 ? max_pcg_iterations : std::max(100, 2 * h->N);
  if (x_in) {   // the linear solve's part of the record is not written by this trial: zero, not what an earlier call left
    DVS_HIP(hipMemcpyAsync(P.x, x_in, 6 * N * 8, hipMemcpyHostToDevice, h->stream));
    DVS_HIP(hipMemsetAsync(&P.status->rnorm, 0, sizeof(PgoStatus) - offsetof(PgoStatus, rnorm), h->stream));
  }
  enqueue_trial(h, radius, eta, max_pcg, reuse_diagonal != 0, x_in != nullptr);
  PgoStatus s;
  DVS_TRY(read_status(h, &s));
  if (cur_q) DVS_HIP(hipMemcpy(cur_q, h->q_cur, 4 * N * 8, hipMemcpyDeviceToHost));
  if (cur_t) DVS_HIP(hipMemcpy(cur_t, h->t_cur, 3 * N * 8, hipMemcpyDeviceToHost));
  if (x) DVS_HIP(hipMemcpy(x, P.x, 6 * N * 8, hipMemcpyDeviceToHost));
  if (D) DVS_HIP(hipMemcpy(D, P.D, 6 * N * 8, hipMemcpyDeviceToHost));
  if (cand_q) DVS_HIP(hipMemcpy(cand_q, h->q_cand, 4 * N * 8, hipMemcpyDeviceToHost));
  if (cand_t) DVS_HIP(hipMemcpy(cand_t, h->t_cand, 3 * N * 8, hipMemcpyDeviceToHost));
  if (rec) memcpy(rec, &s, sizeof(s));
  if (commit) {
    commit_candidate(h);
    DVS_HIP(hipStreamSynchronize(h->stream));
    DVS_HIP(hipGetLastError());
  }
  return DVS_OK;
}
#endif  // DVS_TEST_HOOKS

}  // extern "C"
