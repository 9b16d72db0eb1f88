// pose_host.h — the FP64 pose arithmetic the tracking handles do on the host between two waits: plain C++, no handle, no device.
// tracker.hip (Frontend::syncCallback's pose step, publishKeyframe's quaternion, the motion mask's relative pose), reloc.hip and
// map_track.hip include it.  Every expression is written with the parenthesisation and the order of operations it has had since
// tests/tracker_ref.py restated it operation for operation, and nothing here may be fused: the tests compare R_ / t_ bit for bit.
#pragma once
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>
#include "../../include/dvslam_hip.h"   // dvs_tracker_params, DVS_KF_*

namespace dvs {

// cv::Rodrigues(rvec) in double, explicit order of operations
inline void rodrigues(const double* w, double* R) {
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  if (th < 1e-15) { for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0; return; }
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const double c = cos(th), s = sin(th), c1 = 1.0 - c;
  const double K[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = ((i == j ? c : 0.0) + c1 * (k[i] * k[j])) + s * K[3 * i + j];
}

// frontend.cpp:925-948: the inverse of PnP's motion (rvec, tvec), isMotionOutlier (:549-570) on it, and — unless it is one — the pose
// products R <- R Ri, t <- t + R ti in place.  Returns true where the pose was updated, false for a motion outlier (R, t untouched).
inline bool pose_step(double* R, double* t, const double* rvec, const double* tvec, double max_translation, double max_rotation) {
  double Rr[9], Ri[9], ti[3];
  rodrigues(rvec, Rr);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ri[3 * i + j] = Rr[3 * j + i];                             // :937
  for (int i = 0; i < 3; i++) ti[i] = -((Ri[3 * i] * tvec[0] + Ri[3 * i + 1] * tvec[1]) + Ri[3 * i + 2] * tvec[2]);   // :938
  const double tn = sqrt((ti[0] * ti[0] + ti[1] * ti[1]) + ti[2] * ti[2]);
  const double ca = (((Ri[0] + Ri[4]) + Ri[8]) - 1.0) / 2.0, ang = acos(ca < -1.0 ? -1.0 : (ca > 1.0 ? 1.0 : ca));
  if (tn > max_translation || ang > max_rotation) return false;
  double Rn[9], tn3[3];
  for (int i = 0; i < 3; i++) tn3[i] = t[i] + ((R[3 * i] * ti[0] + R[3 * i + 1] * ti[1]) + R[3 * i + 2] * ti[2]);   // :947
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rn[3 * i + j] = (R[3 * i] * Ri[j] + R[3 * i + 1] * Ri[3 + j]) + R[3 * i + 2] * Ri[6 + j];   // :948
  memcpy(R, Rn, sizeof(Rn)); memcpy(t, tn3, sizeof(tn3));
  return true;
}

// frontend.cpp:699-790 publishKeyframe's rotation as a quaternion (x, y, z, w)
inline void rotation_to_quat_xyzw(const double* R, double* q) {
  const double tr1 = ((1.0 + R[0]) + R[4]) + R[8];
  const double w = sqrt(tr1 > 0.0 ? tr1 : 0.0) / 2.0;
  q[0] = (R[7] - R[5]) / (4 * w); q[1] = (R[2] - R[6]) / (4 * w); q[2] = (R[3] - R[1]) / (4 * w);
  q[3] = w;
}

// A camera-to-world pose (R row-major, t).
struct PoseRt { double R[9], t[3]; };

// the relative pose of dvs_tracker_set_motion_mask: `a` = T(t-1), `b` = T(t-2) or NULL, against `ref`.  With b the prediction is the
// constant-velocity one, T(t-1) o (T(t-2)^-1 o T(t-1)); without, T(t-1) itself.  Every product is a plain row-by-column sum in index order.
inline void relative_pose(const PoseRt& a, const PoseRt* b, const PoseRt& ref, double* R, double* tr) {
  double Rp[9], tp[3];
  memcpy(Rp, a.R, sizeof(Rp)); memcpy(tp, a.t, sizeof(tp));
  if (b) {
    double Rrel[9], trel[3];   // T(t-2)^-1 o T(t-1)
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Rrel[3 * i + j] = b->R[i] * a.R[j] + b->R[3 + i] * a.R[3 + j] + b->R[6 + i] * a.R[6 + j];
      trel[i] = b->R[i] * (a.t[0] - b->t[0]) + b->R[3 + i] * (a.t[1] - b->t[1]) + b->R[6 + i] * (a.t[2] - b->t[2]);
    }
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Rp[3 * i + j] = a.R[3 * i] * Rrel[j] + a.R[3 * i + 1] * Rrel[3 + j] + a.R[3 * i + 2] * Rrel[6 + j];
      tp[i] = a.R[3 * i] * trel[0] + a.R[3 * i + 1] * trel[1] + a.R[3 * i + 2] * trel[2] + a.t[i];
    }
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[3 * i + j] = ref.R[i] * Rp[j] + ref.R[3 + i] * Rp[3 + j] + ref.R[6 + i] * Rp[6 + j];
    tr[i] = ref.R[i] * (tp[0] - ref.t[0]) + ref.R[3 + i] * (tp[1] - ref.t[1]) + ref.R[6 + i] * (tp[2] - ref.t[2]);
  }
}

// relocalisation: camera-to-world from a PnP record (x_cam = R_cw X + tvec): R_cw by Rodrigues' formula in FP64, every expression as
// written.  NOT rodrigues() above: the two are different expressions and give different bits.
inline void reloc_pose(const double* rvec, const double* tvec, double* R9, double* t3) {
  const double wx = rvec[0], wy = rvec[1], wz = rvec[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double Rcw[9];
  if (th < 1e-12) {
    for (int k = 0; k < 9; k++) Rcw[k] = (k % 4 == 0 ? 1.0 : 0.0) + K[k];
  } else {
    const double A = sin(th) / th, B = (1.0 - cos(th)) / th2;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
        Rcw[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * k2;
      }
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R9[3 * i + j] = Rcw[3 * j + i];
    t3[i] = -((Rcw[i] * tvec[0] + Rcw[3 + i] * tvec[1]) + Rcw[6 + i] * tvec[2]);
  }
}

// frontend.cpp:601-662 isKeyframe as the tracker asks it after every tracked frame.  kf_run: this frame's culled set was matched against the
// last keyframe's (n_kfm matches below the Hamming bound, n_kfg of them after the fundamental-matrix gate).
struct KeyframeDecision { bool publish; int criterion; int since_kf; };
inline KeyframeDecision keyframe_decision(bool has_last_kf, bool kf_run, int n_kfg, int since_kf, const dvs_tracker_params& P) {
  if (!has_last_kf) return {true, DVS_KF_NO_REFERENCE, since_kf};   // :603-606 (the first frame publishes without asking isKeyframe)
  const bool few = kf_run && n_kfg < P.kf_min_matches;              // :651
  const bool late = since_kf > P.kf_max_frames;
  if (few || late) return {true, (few ? DVS_KF_FEW_MATCHES : 0) | (late ? DVS_KF_MAX_FRAMES : 0), 0};   // :655-657
  return {false, 0, since_kf + 1};                                  // :660
}

}  // namespace dvs
