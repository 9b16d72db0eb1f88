// ransac_shared.h — what the library's batched-hypothesis estimators share: ransac.hip (fundamental matrix, PnP) and loop_verify.hip
// (rigid 3D-3D loop verification) draw their samples with the same rule, replay the same sequential loop over their counts and end in
// the same rotation -> Rodrigues conversion.  One copy of each, stated once; k_ransac_select has internal linkage because
// two translation units launch it.
#pragma once
#include <float.h>
#include <math.h>
#include "ransac_device.h"
#include "splitmix64.h"

namespace dvs {

// k distinct indices out of n (k <= 8), uniform without replacement, in draw order
template <int KS>
__device__ __forceinline__ void sample_distinct(unsigned long long seed, int h, int n, int* idx) {
  int sorted[KS];
#pragma unroll
  for (int j = 0; j < KS; j++) {
    int r = (int)(splitmix64(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(h * 16 + j + 1)) % (unsigned long long)(n - j));
    for (int i = 0; i < j; i++) if (r >= sorted[i]) r++;   // skip the indices drawn before (ascending)
    idx[j] = r;
    int p = j;
    while (p > 0 && sorted[p - 1] > r) { sorted[p] = sorted[p - 1]; p--; }
    sorted[p] = r;
  }
}

// cv::RANSACUpdateNumIters (on the host: LMedS' fixed iteration count)
__host__ __device__ __forceinline__ int ransac_update_iters(double p, double ep, int modelPoints, int maxIters) {
  p = fmax(p, 0.0); p = fmin(p, 1.0);
  ep = fmax(ep, 0.0); ep = fmin(ep, 1.0);
  double num = fmax(1.0 - p, DBL_MIN);
  double denom = 1.0 - pow(1.0 - ep, (double)modelPoints);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= maxIters * (-denom) ? maxIters : (int)rint(num / denom);
}

// the sequential RANSAC loop replayed over the hypothesis counts (RANSACPointSetRegistrator::run): hypothesis h is iteration h,
// a strictly better count replaces the best and shortens the loop.  sel[0] = best hypothesis (-1: none), sel[1] = iterations used.
static __global__ void k_ransac_select(const int* __restrict__ counts, int H, const RansacProb* __restrict__ probs, int modelPoints, double confidence, int group,
                                int* __restrict__ sel, int capInSeed = 0, int maxItersTrue = 0) {
  if (threadIdx.x != 0) return;
  const int n = probs[blockIdx.x].n;
  counts += (size_t)H * blockIdx.x; sel += 4 * (size_t)blockIdx.x;
  // cv mode: only the first H / group iterations of a loop of up to maxItersTrue have their models here (the loop usually stops long
  // before), and the problem record says how many iterations getSubset found a sample for.  sel[3] = 1: the loop wanted to go on past them
  const int avail = H / group;
  int niters = maxItersTrue > 0 ? maxItersTrue : avail, best = -1, bestCount = 0, it = 0;
  const int maxIters = niters;
  const int found = capInSeed ? (int)probs[blockIdx.x].seed : avail;   // = sampled_iterations(), spelled out: through the member the compiler schedules this kernel differently
  for (; it < niters && it < avail && it < found; it++) {
    for (int s = 0; s < group; s++) {   // `group` candidate models per iteration (P3P: up to 4 poses per sample), in order
      const int h = it * group + s;
      const int good = counts[h];
      if (good > max(bestCount, modelPoints - 1)) {
        bestCount = good; best = h;
        niters = ransac_update_iters(confidence, (double)(n - good) / n, modelPoints, maxIters);
      }
    }
  }
  sel[0] = best; sel[1] = it; sel[2] = bestCount;
  sel[3] = it < niters && it >= avail && found >= avail ? 1 : 0;
}

// rotation matrix -> Rodrigues vector, the principal one (|w| <= pi).  The antisymmetric part of R is 2 sin(theta) a and gives the axis a,
// acos of the trace gives the angle — except where sin(theta) < 1e-4, next to 0 and next to pi.  There acos loses half the digits
// (a rotation by 1e-9 has a trace of exactly 3 and came out as no rotation at all): the angle is atan2(sin, cos).  And next to pi the
// antisymmetric part is too small to carry the axis (at pi - 1e-7 its rounding errors are 1e-9 of its length; at pi it is zero): the
// axis comes from the symmetric part, (R + R^T) / 2 = cos I + (1 - cos) a a^T, whose row of the largest axis component k gives
// every component WITH its sign relative to a_k; what is left of the antisymmetric part decides between a and -a.  Everywhere else
// the operations are the ones k_pnp_refine always ran, bit for bit.
__host__ __device__ __forceinline__ void rotation_to_rodrigues(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  const double cth = fmax(-1.0, fmin(1.0, (tr - 1.0) / 2.0)), th = acos(cth);
  w[0] = R[7] - R[5]; w[1] = R[2] - R[6]; w[2] = R[3] - R[1];
  const double sn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) / 2.0;   // sin(theta)
  const bool flat = sn < 1e-4;
  if (flat && cth < 0) {
    const double d[3] = {R[0] - cth, R[4] - cth, R[8] - cth};               // (1 - cos) a_i^2
    int k = 0;
    if (d[1] > d[k]) k = 1;
    if (d[2] > d[k]) k = 2;
    const double omc = 1.0 - cth, ak = sqrt(fmax(d[k], 0.0) / omc);
    double a[3];
    for (int i = 0; i < 3; i++) a[i] = i == k ? ak : (R[3 * k + i] + R[3 * i + k]) / 2.0 / (omc * ak);
    const double sgn = w[0] * a[0] + w[1] * a[1] + w[2] * a[2] < 0 ? -1.0 : 1.0;
    const double ang = atan2(sn, cth);
    for (int i = 0; i < 3; i++) w[i] = sgn * ang * a[i];
  } else if (sn > 1e-12) {
    const double f = (flat ? atan2(sn, cth) : th) / (2.0 * sn);
    for (int k = 0; k < 3; k++) w[k] *= f;
  } else {   // theta = 0 to rounding
    for (int k = 0; k < 3; k++) w[k] *= 0.5;
  }
}

}  // namespace dvs
