// jacobi_eig.h — the cyclic Jacobi eigen-decomposition of a small symmetric matrix, per thread, arrays in private memory.  Moved out
// of pnp_cv.h when loop_verify.hip became its second user (Horn's 4 x 4 matrix).  The stopping threshold is a parameter: jacobi_eig is the
// routine pnp_cv.h always ran (1e-28: the off-diagonal norm below 1e-14 of the diagonal's), constant for constant.
#pragma once
#include <math.h>

namespace dvs {
namespace pnpcv {

// cyclic Jacobi on the symmetric N x N matrix A (row-major, destroyed); eigenvectors in the COLUMNS of V
template <int N>
__device__ inline void jacobi_eig_tol(double* A, double* V, double tol2) {
  for (int i = 0; i < N * N; i++) V[i] = 0.0;
  for (int i = 0; i < N; i++) V[i * N + i] = 1.0;
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0.0, dg = 0.0;
    for (int p = 0; p < N; p++) { dg += A[p * N + p] * A[p * N + p]; for (int q = p + 1; q < N; q++) off += A[p * N + q] * A[p * N + q]; }
    if (!(off > tol2 * dg)) break;   // sums of squares: off-diagonal norm below sqrt(tol2) of the diagonal's; Jacobi converges quadratically
    for (int p = 0; p < N - 1; p++)
      for (int q = p + 1; q < N; q++) {
        const double apq = A[p * N + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; k++) { const double a = A[k * N + p], b = A[k * N + q]; A[k * N + p] = c * a - s * b; A[k * N + q] = s * a + c * b; }
        for (int k = 0; k < N; k++) { const double a = A[p * N + k], b = A[q * N + k]; A[p * N + k] = c * a - s * b; A[q * N + k] = s * a + c * b; }
        for (int k = 0; k < N; k++) { const double a = V[k * N + p], b = V[k * N + q]; V[k * N + p] = c * a - s * b; V[k * N + q] = s * a + c * b; }
      }
  }
}
template <int N>
__device__ inline void jacobi_eig(double* A, double* V) { jacobi_eig_tol<N>(A, V, 1e-28); }

}  // namespace pnpcv
}  // namespace dvs
