// ransac_device.h — the RANSAC stages of ransac.hip on inputs that already live on the device (used by tracker.hip and reloc.hip).  The
// host-pointer entry points of include/dvslam_hip.h place their points in a layout of ransac_layout.h, import it and run one pass of the
// estimator; these forms carve the same layout without its point and result arrays, run the SAME pass on the caller's pointers and leave
// their results on the device (tests/test_gpu_ransac_device_forms.py compares the two byte for byte).  `ctx` gives the stream and scratch
// slot 0 (hypotheses, counts, selection: gone with the next call).
#pragma once
#include "matcher.h"
#include "ransac_layout.h"   // RansacProb, PnpRecord, SelRecord

namespace dvs {

// dvs_find_fundamental_ransac on d_p1 / d_p2 (n x 2 float) with the count read from *d_n on the device (n_bound >= *d_n sizes the
// grids): d_mask[0 .. *d_n) = the inlier mask.  Fewer than 8 correspondences give a mask of zeros.  Asynchronous.
dvs_status fm_own_device(dvs_matcher* ctx, const float* d_p1, const float* d_p2, const int* d_n, int n_bound, unsigned long long seed, double threshold,
                         double confidence, int max_iters, unsigned char* d_mask);
// dvs_solve_pnp_ransac on d_obj (n x 3) / d_img (n x 2), count *d_n: d_out = the stage's result record (ransac_layout.h), d_inl = ascending
// inlier indices.  Asynchronous.
dvs_status pnp_own_device(dvs_matcher* ctx, const float* d_obj, const float* d_img, const int* d_n, unsigned long long seed, const double* K4,
                          int iterations, double reproj_err, double confidence, int* d_inl, PnpRecord* d_out);
// dvs_find_fundamental_cv: OpenCV's sample sequence is drawn on the host from the count AND the points (collinear samples are drawn again),
// so the n (>= 8) correspondences are read back first; samples go up, the 16-byte selection record comes back (the 96-iteration pass may
// ask for the full one).  The mask stays on the device.  Synchronises.
dvs_status fm_cv_device(dvs_matcher* ctx, const float* d_p1, const float* d_p2, int n, double threshold, double confidence, int max_iters,
                        unsigned char* d_mask);
// dvs_solve_pnp_ransac_cv: its 5-point samples depend on the count alone (host `n` >= 6); samples go up, nothing comes back.  d_out as
// above (rvec / tvec are meaningful when d_sel->best >= 0), d_sel = {best model or -1, iterations run, its inlier count, 0}.  Asynchronous.
dvs_status pnp_cv_device(dvs_matcher* ctx, const float* d_obj, const float* d_img, int n, const double* K4, int iterations, double reproj_err,
                         double confidence, int* d_inl, PnpRecord* d_out, SelRecord* d_sel);

}  // namespace dvs
