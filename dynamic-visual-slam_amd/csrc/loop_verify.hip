// loop_verify.hip — loop verification: the rigid motion x_q = R x_e + t between a query keyframe and each loop candidate, by a
// batched-hypothesis RANSAC over the 3D points both keyframes carry, in the style of ransac.hip: all hypotheses of all candidates are
// fitted at once (one thread each), scored at once (one workgroup per hypothesis, blockIdx.y = candidate), the sequential loop is
// replayed over the counts (k_ransac_select, ransac_shared.h), and one workgroup per candidate refines on the inliers.  The rule is the
// header's (include/dvslam_hip.h, "loop verification"); tests/loop_verify_ref.py is its sequential restatement.  All arithmetic is FP64
// on the float inputs; no floating atomics anywhere: every sum is folded in a fixed order, so a call's bytes do not depend on the schedule.
//   k_lv_gather      one workgroup per candidate slot: the ordered compaction of the valid correspondences (ballot ranks inside a
//                    wavefront, the four wavefront totals through LDS, a running base per 256-row chunk) into six coordinate planes, so
//                    that consecutive list positions are consecutive floats for the scoring reads; the mask cleared; the slot's RansacProb
//   k_lv_hypotheses  one thread per (hypothesis, candidate): sample_distinct<3>, Horn's closed form (jacobi_eig_tol<4>)
//   k_lv_score       one workgroup per (hypothesis, candidate): the inlier count
//   k_ransac_select  ransac_shared.h
//   k_lv_refine      one workgroup per candidate: the refinement rounds, the mask, the record
#include <math.h>
#include <string.h>
#include <vector>
#include "block_ops.h"
#include "common.h"
#include "device_mem.h"
#include "loop_internal.h"
#include "ransac_shared.h"
#include "jacobi_eig.h"
#ifdef DVS_TEST_HOOKS
#include "../../include/dvslam_hip_test.h"
#endif

namespace {
using namespace dvs;

constexpr int kBlock = 256;
constexpr int kRoundRec = 16;     // doubles per refinement-round record of the test hook
constexpr int kRoundRows = 9;     // the selected hypothesis and up to 8 rounds

struct Cam { double fx, fy, cx, cy; };

__device__ __forceinline__ int clamp_count(const int* p, int cap) { return min(max(*p, 0), cap); }

__device__ __forceinline__ bool point_valid(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z) && z > 0.0f; }

// the error of one correspondence under (R, t): the larger of the squared reprojection distances in the two images; +inf where a
// transformed depth is <= 0 (or anything is not a number: such a correspondence is never an inlier)
__device__ __forceinline__ double lv_error(const double* R, const double* t, const Cam& K, double ex, double ey, double ez, double qx, double qy, double qz) {
  const double px = R[0] * ex + R[1] * ey + R[2] * ez + t[0], py = R[3] * ex + R[4] * ey + R[5] * ez + t[1], pz = R[6] * ex + R[7] * ey + R[8] * ez + t[2];
  const double dx = qx - t[0], dy = qy - t[1], dz = qz - t[2];
  const double rx = R[0] * dx + R[3] * dy + R[6] * dz, ry = R[1] * dx + R[4] * dy + R[7] * dz, rz = R[2] * dx + R[5] * dy + R[8] * dz;
  if (!(pz > 0.0) || !(rz > 0.0)) return INFINITY;
  const double du1 = (K.fx * px / pz + K.cx) - (K.fx * qx / qz + K.cx), dv1 = (K.fy * py / pz + K.cy) - (K.fy * qy / qz + K.cy);
  const double du2 = (K.fx * rx / rz + K.cx) - (K.fx * ex / ez + K.cx), dv2 = (K.fy * ry / rz + K.cy) - (K.fy * ey / ez + K.cy);
  const double e = fmax(du1 * du1 + dv1 * dv1, du2 * du2 + dv2 * dv2);
  return e == e ? e : INFINITY;
}

// Horn's closed form from the centroids and the cross-covariance S[3 a + b] = sum (e_a - me_a)(q_b - mq_b): R (row-major), t and the
// relative gap (lambda1 - lambda2) / |lambda1| of the 4 x 4 matrix.  false: degenerate (not finite, or the gap <= 1e-9).
// The Jacobi sweeps stop at an off-diagonal norm of 1e-16 of the diagonal's: the eigenvector's error is that norm divided by the gap.
__device__ inline bool horn_fit(const double* me, const double* mq, const double* S, double* R, double* t, double* gap) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double A[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                  Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                  Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                  Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
  double V[16];
  pnpcv::jacobi_eig_tol<4>(A, V, 1e-32);
  const double l[4] = {A[0], A[5], A[10], A[15]};
  int i1 = 0;
  for (int k = 1; k < 4; k++) if (l[k] > l[i1]) i1 = k;
  double l2 = -INFINITY;
  for (int k = 0; k < 4; k++) if (k != i1 && l[k] > l2) l2 = l[k];
  const double l1 = l[i1];
  *gap = (l1 - l2) / fabs(l1);
  bool ok = isfinite(l1) && isfinite(l2) && !((l1 - l2) <= 1e-9 * fabs(l1));
  double q0 = V[i1], qx = V[4 + i1], qy = V[8 + i1], qz = V[12 + i1];
  const double nrm = sqrt(q0 * q0 + qx * qx + qy * qy + qz * qz);
  ok = ok && nrm > 0.0 && isfinite(nrm);
  const double sg = (q0 >= 0.0 ? 1.0 : -1.0) / (ok ? nrm : 1.0);
  q0 *= sg; qx *= sg; qy *= sg; qz *= sg;
  R[0] = q0 * q0 + qx * qx - qy * qy - qz * qz; R[1] = 2.0 * (qx * qy - q0 * qz);             R[2] = 2.0 * (qx * qz + q0 * qy);
  R[3] = 2.0 * (qx * qy + q0 * qz);             R[4] = q0 * q0 - qx * qx + qy * qy - qz * qz; R[5] = 2.0 * (qy * qz - q0 * qx);
  R[6] = 2.0 * (qx * qz - q0 * qy);             R[7] = 2.0 * (qy * qz + q0 * qx);             R[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
  for (int a = 0; a < 3; a++) t[a] = mq[a] - (R[3 * a] * me[0] + R[3 * a + 1] * me[1] + R[3 * a + 2] * me[2]);
  for (int k = 0; k < 9; k++) ok = ok && isfinite(R[k]);
  for (int k = 0; k < 3; k++) ok = ok && isfinite(t[k]);
  return ok;
}

__device__ __forceinline__ void write_failed(dvs_loop_verify_result* r, int n_corr) {
  r->n_corr = n_corr; r->n_inliers = 0; r->success = 0; r->iterations = 0;
  for (int k = 0; k < 3; k++) { r->rvec[k] = 0.0; r->tvec[k] = 0.0; }
  r->rms_px = 0.0;
}

// grid (cap_cand), 256 threads.  Slot c's list: positions [0, m) of list_i + c * stride and of the six planes at pts + 6 * c * stride.
__global__ __launch_bounds__(kBlock) void k_lv_gather(const long long* __restrict__ row_off, const float* __restrict__ e_xyz, int n_entries,
                                                      const float* __restrict__ q_xyz, const int* __restrict__ d_n, int stride_rows,
                                                      const int* __restrict__ d_entry_ids, const int* __restrict__ d_n_cand, int cap_cand,
                                                      const int* __restrict__ train_idx, int min_corr, unsigned long long seed,
                                                      RansacProb* __restrict__ probs, int* __restrict__ list_i, float* __restrict__ pts,
                                                      dvs_loop_verify_result* __restrict__ results, unsigned char* __restrict__ mask) {
  __shared__ int s_wave[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)c * stride_rows;
  for (int i = tid; i < stride_rows; i += kBlock) mask[base + i] = 0;
  const bool listed = c < clamp_count(d_n_cand, cap_cand);
  const int e = listed ? d_entry_ids[c] : -1;
  if (!listed || e < 0 || e >= n_entries) {
    if (tid == 0) { probs[c] = RansacProb::seeded(0, 0, 0ull); write_failed(&results[c], listed ? -1 : 0); }
    return;
  }
  const int n = clamp_count(d_n, stride_rows);
  const long long eo = row_off[e], rows = row_off[e + 1] - eo;
  const float* ep = e_xyz + 3 * eo;
  float* plane = pts + 6 * base;
  int m = 0;                                          // the same in every thread
  for (int i0 = 0; i0 < n; i0 += kBlock) {
    const int i = i0 + tid;
    bool take = false;
    float ex = 0, ey = 0, ez = 0, qx = 0, qy = 0, qz = 0;
    if (i < n) {
      const int j = train_idx[base + i];
      if (j >= 0 && j < rows) {
        qx = q_xyz[3 * (size_t)i]; qy = q_xyz[3 * (size_t)i + 1]; qz = q_xyz[3 * (size_t)i + 2];
        ex = ep[3 * (size_t)j]; ey = ep[3 * (size_t)j + 1]; ez = ep[3 * (size_t)j + 2];
        take = point_valid(qx, qy, qz) && point_valid(ex, ey, ez);
      }
    }
    int total;
    const int pos = m + block_rank256(take, s_wave, total);   // pos <= i < stride_rows
    if (take) {
      list_i[base + pos] = i;
      plane[pos] = ex; plane[(size_t)stride_rows + pos] = ey; plane[2 * (size_t)stride_rows + pos] = ez;
      plane[3 * (size_t)stride_rows + pos] = qx; plane[4 * (size_t)stride_rows + pos] = qy; plane[5 * (size_t)stride_rows + pos] = qz;
    }
    m += total;
  }
  if (tid == 0) {
    // a list shorter than min_correspondences runs no later stage: its RansacProb is empty
    probs[c] = RansacProb::seeded(0, m >= min_corr ? m : 0, splitmix64(seed ^ (unsigned long long)e));
    write_failed(&results[c], m);                     // the refinement completes the record where the candidate gets that far
  }
}

// grid (ceil(H / 64), cap_cand), 64 threads
__global__ __launch_bounds__(64) void k_lv_hypotheses(const RansacProb* __restrict__ probs, const float* __restrict__ pts, int stride_rows, int H,
                                                      double* __restrict__ models, int* __restrict__ valid, int* __restrict__ dbg_sample,
                                                      double* __restrict__ dbg_gap) {
  const int h = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
  if (h >= H) return;
  const RansacProb pb = probs[c];
  const size_t o = (size_t)c * H + h;
  double* M = models + 12 * o;
  if (pb.n < 3) {
    valid[o] = 0;
    for (int k = 0; k < 12; k++) M[k] = 0.0;
    if (dbg_sample) { dbg_sample[3 * o] = dbg_sample[3 * o + 1] = dbg_sample[3 * o + 2] = -1; }
    if (dbg_gap) dbg_gap[o] = NAN;
    return;
  }
  const float* plane = pts + 6 * (size_t)c * stride_rows;
  int idx[3];
  sample_distinct<3>(pb.seed, h, pb.n, idx);
  double E[3][3], Q[3][3], me[3] = {0, 0, 0}, mq[3] = {0, 0, 0};
  for (int s = 0; s < 3; s++)
    for (int a = 0; a < 3; a++) {
      E[s][a] = plane[(size_t)a * stride_rows + idx[s]]; Q[s][a] = plane[(size_t)(3 + a) * stride_rows + idx[s]];
      me[a] += E[s][a]; mq[a] += Q[s][a];
    }
  for (int a = 0; a < 3; a++) { me[a] /= 3.0; mq[a] /= 3.0; }
  double S[9];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double v = 0;
      for (int s = 0; s < 3; s++) v += (E[s][a] - me[a]) * (Q[s][b] - mq[b]);
      S[3 * a + b] = v;
    }
  double R[9], t[3], gap;
  const bool ok = horn_fit(me, mq, S, R, t, &gap);
  for (int k = 0; k < 9; k++) M[k] = ok ? R[k] : 0.0;
  for (int k = 0; k < 3; k++) M[9 + k] = ok ? t[k] : 0.0;
  valid[o] = ok ? 1 : 0;
  if (dbg_sample) { dbg_sample[3 * o] = idx[0]; dbg_sample[3 * o + 1] = idx[1]; dbg_sample[3 * o + 2] = idx[2]; }
  if (dbg_gap) dbg_gap[o] = gap;
}

// grid (H, cap_cand), 256 threads: thread k of a chunk reads position k of each plane — consecutive floats
__global__ __launch_bounds__(kBlock) void k_lv_score(const RansacProb* __restrict__ probs, const float* __restrict__ pts, int stride_rows, int H,
                                                     const double* __restrict__ models, const int* __restrict__ valid, Cam K, double thr2,
                                                     int* __restrict__ counts) {
  __shared__ int s_cnt[4];
  const int h = blockIdx.x, c = blockIdx.y;
  const size_t o = (size_t)c * H + h;
  if (!valid[o]) { if (threadIdx.x == 0) counts[o] = 0; return; }
  const int n = probs[c].n;
  const float* plane = pts + 6 * (size_t)c * stride_rows;
  double R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = models[12 * o + k];
  for (int k = 0; k < 3; k++) t[k] = models[12 * o + 9 + k];
  int total = 0;
  for (int k0 = 0; k0 < n; k0 += kBlock) {
    const int k = k0 + threadIdx.x;
    bool in = false;
    if (k < n)
      in = lv_error(R, t, K, plane[k], plane[(size_t)stride_rows + k], plane[2 * (size_t)stride_rows + k], plane[3 * (size_t)stride_rows + k],
                    plane[4 * (size_t)stride_rows + k], plane[5 * (size_t)stride_rows + k]) <= thr2;
    total += block_count256(in, s_cnt);
  }
  if (threadIdx.x == 0) counts[o] = total;
}

// the sums of k_lv_refine: thread t's partial sums (its positions t, t + 256, ... in ascending order) folded by block_ops.h's fixed tree
// grid (cap_cand), 256 threads
__global__ __launch_bounds__(kBlock) void k_lv_refine(const RansacProb* __restrict__ probs, const float* __restrict__ pts, const int* __restrict__ list_i,
                                                      int stride_rows, int H, const double* __restrict__ models, const int* __restrict__ sel, Cam K,
                                                      double thr2, int rounds, int min_inliers, dvs_loop_verify_result* __restrict__ results,
                                                      unsigned char* __restrict__ mask, double* __restrict__ dbg_rounds) {
  __shared__ double s_red[9 * kBlock];
  __shared__ int s_cnt[4];
  __shared__ double s_fit[14];                        // R, t, gap, ok of the round's fit (thread 0 fits, everybody reads)
  const int c = blockIdx.x, tid = threadIdx.x;
  double* dbg = dbg_rounds ? dbg_rounds + (size_t)c * kRoundRows * kRoundRec : nullptr;
  if (dbg) for (int k = tid; k < kRoundRows * kRoundRec; k += kBlock) dbg[k] = 0.0;
  const int n = probs[c].n, best = sel[4 * c];
  if (n < 3 || best < 0) return;                      // the record k_lv_gather wrote stands: failed
  const float* plane = pts + 6 * (size_t)c * stride_rows;
  const float *pex = plane, *pey = plane + stride_rows, *pez = plane + 2 * (size_t)stride_rows, *pqx = plane + 3 * (size_t)stride_rows,
              *pqy = plane + 4 * (size_t)stride_rows, *pqz = plane + 5 * (size_t)stride_rows;
  double R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = models[12 * ((size_t)c * H + best) + k];
  for (int k = 0; k < 3; k++) t[k] = models[12 * ((size_t)c * H + best) + 9 + k];
  auto count_set = [&](const double* Rm, const double* tm) {
    int total = 0;
    for (int k0 = 0; k0 < n; k0 += kBlock) {
      const int k = k0 + tid;
      const bool in = k < n && lv_error(Rm, tm, K, pex[k], pey[k], pez[k], pqx[k], pqy[k], pqz[k]) <= thr2;
      total += block_count256(in, s_cnt);
    }
    return total;
  };
  int size = count_set(R, t);                         // |S_0|: the selected hypothesis' count again
  __syncthreads();
  if (dbg && tid == 0) { for (int k = 0; k < 9; k++) dbg[k] = R[k]; for (int k = 0; k < 3; k++) dbg[9 + k] = t[k]; dbg[12] = size; dbg[13] = 1.0; dbg[14] = 1.0; }
  for (int r = 1; r <= rounds; r++) {
    // pass 1: the centroids of S_(r-1), the inliers of the model in hand
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += kBlock)
      if (lv_error(R, t, K, pex[k], pey[k], pez[k], pqx[k], pqy[k], pqz[k]) <= thr2) {
        v[0] += pex[k]; v[1] += pey[k]; v[2] += pez[k]; v[3] += pqx[k]; v[4] += pqy[k]; v[5] += pqz[k];
      }
    block_sums<kBlock, 6>(v, s_red);
    const double me[3] = {v[0] / size, v[1] / size, v[2] / size}, mq[3] = {v[3] / size, v[4] / size, v[5] / size};
    // pass 2: the centred cross-covariance
    for (int k = 0; k < 9; k++) v[k] = 0.0;
    for (int k = tid; k < n; k += kBlock)
      if (lv_error(R, t, K, pex[k], pey[k], pez[k], pqx[k], pqy[k], pqz[k]) <= thr2) {
        const double e[3] = {pex[k] - me[0], pey[k] - me[1], pez[k] - me[2]}, q[3] = {pqx[k] - mq[0], pqy[k] - mq[1], pqz[k] - mq[2]};
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) v[3 * a + b] += e[a] * q[b];
      }
    block_sums<kBlock, 9>(v, s_red);
    if (tid == 0) {
      double Rn[9], tn[3], gap;
      const bool ok = horn_fit(me, mq, v, Rn, tn, &gap);
      for (int k = 0; k < 9; k++) s_fit[k] = Rn[k];
      for (int k = 0; k < 3; k++) s_fit[9 + k] = tn[k];
      s_fit[12] = gap; s_fit[13] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    double Rn[9], tn[3];
    for (int k = 0; k < 9; k++) Rn[k] = s_fit[k];
    for (int k = 0; k < 3; k++) tn[k] = s_fit[9 + k];
    const bool ok = s_fit[13] != 0.0;
    const int nsize = ok ? count_set(Rn, tn) : 0;
    const bool accept = ok && nsize >= size;
    __syncthreads();                                  // s_fit has been read by everybody
    if (dbg && tid == 0) {
      double* d = dbg + r * kRoundRec;
      for (int k = 0; k < 9; k++) d[k] = Rn[k];
      for (int k = 0; k < 3; k++) d[9 + k] = tn[k];
      d[12] = nsize; d[13] = accept ? 1.0 : 0.0; d[14] = ok ? 1.0 : 0.0;
    }
    if (!accept) break;
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
    for (int k = 0; k < 3; k++) t[k] = tn[k];
    size = nsize;
  }
  // the mask over query rows and the mean inlier error
  double es = 0.0;
  for (int k = tid; k < n; k += kBlock) {
    const double e = lv_error(R, t, K, pex[k], pey[k], pez[k], pqx[k], pqy[k], pqz[k]);
    if (e <= thr2) { es += e; mask[(size_t)c * stride_rows + list_i[(size_t)c * stride_rows + k]] = 1; }
  }
  es = block_sum<kBlock>(es, s_red);
  if (tid == 0) {
    dvs_loop_verify_result* res = &results[c];
    res->n_inliers = size; res->success = size >= min_inliers ? 1 : 0; res->iterations = sel[4 * c + 1];
    double w[3];
    rotation_to_rodrigues(R, w);
    for (int k = 0; k < 3; k++) { res->rvec[k] = w[k]; res->tvec[k] = t[k]; }
    res->rms_px = sqrt(es / size);
  }
}

}  // namespace

namespace dvs {

dvs_status loop_verify_check_params(const dvs_loop_verify_params* p, const char* what) {
  if (!p) { set_error("%s: the verification parameters are NULL (K4 has no default)", what); return DVS_ERR_ARG; }
  const bool ok = p->iterations >= 1 && p->iterations <= 4096 && p->min_correspondences >= 3 && p->min_inliers >= 3 && p->refine_rounds >= 0 &&
                  p->refine_rounds <= 8 && isfinite(p->reproj_err) && p->reproj_err > 0 && p->confidence > 0 && p->confidence < 1 && isfinite(p->K4[0]) &&
                  isfinite(p->K4[1]) && isfinite(p->K4[2]) && isfinite(p->K4[3]) && p->K4[0] > 0 && p->K4[1] > 0;
  if (!ok) {
    set_error("%s: verification parameters iterations=%d min_correspondences=%d min_inliers=%d refine_rounds=%d reproj_err=%g confidence=%g K4=(%g, %g, "
              "%g, %g): iterations in 1..4096, the two minima >= 3, refine_rounds in 0..8, reproj_err and the focal lengths > 0, confidence in (0, 1)",
              what, p->iterations, p->min_correspondences, p->min_inliers, p->refine_rounds, p->reproj_err, p->confidence, p->K4[0], p->K4[1], p->K4[2],
              p->K4[3]);
    return DVS_ERR_ARG;
  }
  return DVS_OK;
}

dvs_status loop_verify_reserve(dvs_loop_db* db, int cap_cand, int stride_rows, int H) {
  DVS_ARG(cap_cand >= 0 && cap_cand <= 65535 && stride_rows >= 0 && H >= 1);
  DVS_ARG((size_t)cap_cand * std::max((size_t)stride_rows, (size_t)db->max_stride) < 0x7fffffffu && (size_t)cap_cand * (size_t)H < 0x7fffffffu);
  const size_t cand = (size_t)cap_cand, list = cand * (size_t)stride_rows, hyp = cand * (size_t)H;
  DVS_HIP(hipSetDevice(db->inv.voc->device));         // the scratch belongs on the handle's device, whichever one the thread had current
  if (cand > db->cap_v_cand || list > db->cap_v_list || hyp > db->cap_v_hyp) {
    DVS_HIP(hipStreamSynchronize(db->inv.voc->stream));   // an earlier verification may still use the blocks this frees
    // blocks that share a capacity: the capacity counts only once all of them have grown
    if (cand > db->cap_v_cand) {
      size_t a = 0, b = 0;
      db->cap_v_cand = 0;
      DVS_TRY(grow(db->v_probs, a, cand));
      DVS_TRY(grow(db->v_sel, b, 4 * cand));
      db->cap_v_cand = a;
    }
    if (list > db->cap_v_list) {
      size_t a = 0, b = 0;
      db->cap_v_list = 0;
      DVS_TRY(grow(db->v_list_i, a, list));
      DVS_TRY(grow(db->v_pts, b, 6 * list));
      db->cap_v_list = a;
    }
    if (hyp > db->cap_v_hyp) {
      size_t a = 0, b = 0, m = 0;
      db->cap_v_hyp = 0;
      DVS_TRY(grow(db->v_counts, a, hyp));
      DVS_TRY(grow(db->v_valid, b, hyp));
      DVS_TRY(grow(db->v_models, m, 12 * hyp));
      db->cap_v_hyp = a;
    }
  }
  return DVS_OK;
}

dvs_status loop_verify_host_blocks(dvs_loop_db* db, size_t cand, size_t n, bool train) {
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  if (3 * n > db->cap_v_in_xyz || (train && cand * n > db->cap_v_in_train) || cand > db->cap_v_res || cand * n > db->cap_v_mask) {
    DVS_HIP(hipStreamSynchronize(db->inv.voc->stream));
    DVS_TRY(grow(db->v_in_xyz, db->cap_v_in_xyz, 3 * n));
    if (train) DVS_TRY(grow(db->v_in_train, db->cap_v_in_train, cand * n));
    DVS_TRY(grow(db->v_res, db->cap_v_res, cand));
    DVS_TRY(grow(db->v_mask, db->cap_v_mask, cand * n));
  }
  return DVS_OK;
}

dvs_status loop_verify_enqueue(dvs_loop_db* db, const float* d_xyz_query, const int* d_n, int stride_rows, const int* d_entry_ids, const int* d_n_cand,
                               int cap_cand, const int* d_train_idx, const dvs_loop_verify_params& P, dvs_loop_verify_result* d_results,
                               uint8_t* d_inlier_mask, const LoopVerifyDebug* debug) {
  if (cap_cand <= 0) return DVS_OK;
  const LoopVerifyDebug none, &dbg = debug ? *debug : none;
  hipStream_t s = db->inv.voc->stream;
  const int H = P.iterations;
  const Cam K{P.K4[0], P.K4[1], P.K4[2], P.K4[3]};
  const double thr2 = P.reproj_err * P.reproj_err;
  hipLaunchKernelGGL(k_lv_gather, dim3(cap_cand), dim3(kBlock), 0, s, db->row_off.get(), db->xyz.get(), db->inv.n_entries, d_xyz_query, d_n, stride_rows,
                     d_entry_ids, d_n_cand, cap_cand, d_train_idx, P.min_correspondences, (unsigned long long)P.seed, db->v_probs.get(), db->v_list_i.get(),
                     db->v_pts.get(), d_results, d_inlier_mask);
  hipLaunchKernelGGL(k_lv_hypotheses, dim3((H + 63) / 64, cap_cand), dim3(64), 0, s, db->v_probs.get(), db->v_pts.get(), stride_rows, H, db->v_models.get(),
                     db->v_valid.get(), dbg.sample, dbg.gap);
  hipLaunchKernelGGL(k_lv_score, dim3(H, cap_cand), dim3(kBlock), 0, s, db->v_probs.get(), db->v_pts.get(), stride_rows, H, db->v_models.get(),
                     db->v_valid.get(), K, thr2, db->v_counts.get());
  hipLaunchKernelGGL(k_ransac_select, dim3(cap_cand), dim3(1), 0, s, db->v_counts.get(), H, db->v_probs.get(), 3, P.confidence, 1, db->v_sel.get(), 0, 0);
  hipLaunchKernelGGL(k_lv_refine, dim3(cap_cand), dim3(kBlock), 0, s, db->v_probs.get(), db->v_pts.get(), db->v_list_i.get(), stride_rows, H,
                     db->v_models.get(), db->v_sel.get(), K, thr2, P.refine_rounds, P.min_inliers, d_results, d_inlier_mask, dbg.rounds);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

}  // namespace dvs

extern "C" {

dvs_status dvs_loopv_default_params(dvs_loop_verify_params* p) {
  DVS_ARG(p);
  p->iterations = 256; p->min_correspondences = 12; p->min_inliers = 12; p->refine_rounds = 2;
  p->reproj_err = 4.0; p->confidence = 0.99; p->seed = 0;
  p->K4[0] = p->K4[1] = p->K4[2] = p->K4[3] = 0.0;
  return DVS_OK;
}

dvs_status dvs_loopv_db_verify_device(dvs_loop_db* db, const float* d_xyz_query, const int32_t* d_n, int32_t stride_rows, const int32_t* d_entry_ids,
                                     const int32_t* d_n_cand, int32_t cap_cand, const int32_t* d_train_idx, const dvs_loop_verify_params* params,
                                     dvs_loop_verify_result* d_results, uint8_t* d_inlier_mask) {
  DVS_ARG(db && d_n && stride_rows >= 0 && cap_cand >= 0 && d_n_cand && (cap_cand == 0 || (d_entry_ids && d_results)));
  DVS_ARG(cap_cand == 0 || stride_rows == 0 || (d_xyz_query && d_train_idx && d_inlier_mask));
  DVS_TRY(loop_verify_check_params(params, "dvs_loopv_db_verify_device"));
  DVS_TRY(loop_verify_reserve(db, cap_cand, stride_rows, params->iterations));
  if (cap_cand == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  return loop_verify_enqueue(db, d_xyz_query, d_n, stride_rows, d_entry_ids, d_n_cand, cap_cand, d_train_idx, *params, d_results, d_inlier_mask);
}

dvs_status dvs_loopv_db_verify(dvs_loop_db* db, const float* xyz, int32_t n, const int32_t* entry_ids, int32_t n_cand, const int32_t* train_idx,
                              const dvs_loop_verify_params* params, dvs_loop_verify_result* results, uint8_t* inlier_mask) {
  DVS_ARG(db && n >= 0 && n_cand >= 0 && n_cand <= 65535 && (n_cand == 0 || (entry_ids && results)));
  DVS_ARG(n_cand == 0 || n == 0 || (xyz && train_idx && inlier_mask));
  DVS_TRY(loop_verify_check_params(params, "dvs_loopv_db_verify"));
  for (int c = 0; c < n_cand; c++)
    if (entry_ids[c] < 0 || entry_ids[c] >= db->inv.n_entries) {
      set_error("dvs_loopv_db_verify: candidate %d is entry id %d, the database holds %d entries", c, entry_ids[c], db->inv.n_entries);
      return DVS_ERR_ARG;
    }
  DVS_TRY(loop_verify_reserve(db, n_cand, n, params->iterations));
  if (n_cand == 0) return DVS_OK;
  hipStream_t s = db->inv.voc->stream;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  DVS_TRY(loop_verify_host_blocks(db, (size_t)n_cand, (size_t)n, true));
  if ((size_t)n_cand + 2 > db->cap_cand_ids) { DVS_HIP(hipStreamSynchronize(s)); DVS_TRY(grow(db->cand_ids, db->cap_cand_ids, (size_t)n_cand + 2)); }
  db->h_cand.assign(1, n_cand);                       // [0] the count, the ids, then the frame's row count
  db->h_cand.insert(db->h_cand.end(), entry_ids, entry_ids + n_cand);
  db->h_cand.push_back(n);
  DVS_HIP(hipMemcpyAsync(db->cand_ids.get(), db->h_cand.data(), sizeof(int) * (n_cand + 2), hipMemcpyHostToDevice, s));
  if (n > 0) {
    DVS_HIP(hipMemcpyAsync(db->v_in_xyz.get(), xyz, (size_t)n * 12, hipMemcpyHostToDevice, s));
    DVS_HIP(hipMemcpyAsync(db->v_in_train.get(), train_idx, sizeof(int) * (size_t)n_cand * n, hipMemcpyHostToDevice, s));
  }
  DVS_TRY(loop_verify_enqueue(db, db->v_in_xyz.get(), db->cand_ids.get() + n_cand + 1, n, db->cand_ids.get() + 1, db->cand_ids.get(), n_cand,
                              db->v_in_train.get(), *params, db->v_res.get(), db->v_mask.get()));
  DVS_HIP(hipMemcpyAsync(results, db->v_res.get(), sizeof(dvs_loop_verify_result) * n_cand, hipMemcpyDeviceToHost, s));
  if (n > 0) DVS_HIP(hipMemcpyAsync(inlier_mask, db->v_mask.get(), (size_t)n_cand * n, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  return DVS_OK;
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test_loop.h)
// the product's enqueue on uploaded inputs, and what each stage left in the handle's scratch
dvs_status dvs_test_loop_verify_stages(dvs_loop_db* db, const float* xyz_query, int32_t n, int32_t stride_rows, const int32_t* entry_ids, int32_t n_cand,
                                       int32_t cap_cand, const int32_t* train_idx, const dvs_loop_verify_params* params, dvs_loop_verify_result* results,
                                       uint8_t* inlier_mask, int32_t* n_list, int32_t* list_i, float* list_pts, int32_t* sample, int32_t* valid,
                                       double* models, double* gap, int32_t* counts, int32_t* sel, double* rounds) {
  DVS_ARG(db && xyz_query && stride_rows >= 1 && n >= 0 && cap_cand >= 1 && n_cand >= 0 && entry_ids && train_idx && results && inlier_mask && n_list &&
          list_i && list_pts && sample && valid && models && gap && counts && sel && rounds);
  DVS_TRY(loop_verify_check_params(params, "dvs_test_loop_verify_stages"));
  DVS_TRY(loop_verify_reserve(db, cap_cand, stride_rows, params->iterations));
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  hipStream_t s = db->inv.voc->stream;
  const size_t C = (size_t)cap_cand, S = (size_t)stride_rows, H = (size_t)params->iterations;
  DeviceBuf<float> dq; DeviceBuf<int> dn, dids, dnc, dtr, dsample; DeviceBuf<dvs_loop_verify_result> dres; DeviceBuf<uint8_t> dmask;
  DeviceBuf<double> dgap, drounds;
  DVS_TRY(dq.upload(std::vector<float>(xyz_query, xyz_query + 3 * S)));
  DVS_TRY(dn.upload(std::vector<int>(1, n)));
  DVS_TRY(dnc.upload(std::vector<int>(1, n_cand)));
  std::vector<int> ids(C, 0);
  for (int c = 0; c < n_cand && c < cap_cand; c++) ids[c] = entry_ids[c];
  DVS_TRY(dids.upload(ids));
  DVS_TRY(dtr.upload(std::vector<int>(train_idx, train_idx + C * S)));
  DVS_TRY(dres.alloc(C)); DVS_TRY(dmask.alloc(C * S)); DVS_TRY(dsample.alloc(3 * C * H)); DVS_TRY(dgap.alloc(C * H)); DVS_TRY(drounds.alloc(C * kRoundRows * kRoundRec));
  DVS_HIP(hipMemsetAsync(dres.get(), 0x5a, sizeof(dvs_loop_verify_result) * C, s));   // poison: every slot must be written
  DVS_HIP(hipMemsetAsync(dmask.get(), 0x5a, C * S, s));
  LoopVerifyDebug dbg;
  dbg.sample = dsample.get(); dbg.gap = dgap.get(); dbg.rounds = drounds.get();
  const dvs_status st = loop_verify_enqueue(db, dq.get(), dn.get(), stride_rows, dids.get(), dnc.get(), cap_cand, dtr.get(), *params, dres.get(), dmask.get(),
                                            &dbg);
  DVS_HIP(hipStreamSynchronize(s));
  DVS_TRY(st);
  std::vector<RansacProb> probs(C);
  DVS_HIP(hipMemcpy(probs.data(), db->v_probs.get(), sizeof(RansacProb) * C, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < C; c++) n_list[c] = probs[c].n;
  DVS_HIP(hipMemcpy(results, dres.get(), sizeof(dvs_loop_verify_result) * C, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(inlier_mask, dmask.get(), C * S, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(list_i, db->v_list_i.get(), sizeof(int) * C * S, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(list_pts, db->v_pts.get(), sizeof(float) * 6 * C * S, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sample, dsample.get(), sizeof(int) * 3 * C * H, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(valid, db->v_valid.get(), sizeof(int) * C * H, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(models, db->v_models.get(), sizeof(double) * 12 * C * H, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(gap, dgap.get(), sizeof(double) * C * H, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(counts, db->v_counts.get(), sizeof(int) * C * H, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel, db->v_sel.get(), sizeof(int) * 4 * C, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(rounds, drounds.get(), sizeof(double) * C * kRoundRows * kRoundRec, hipMemcpyDeviceToHost));
  return DVS_OK;
}
#endif  // DVS_TEST_HOOKS

}  // extern "C"
