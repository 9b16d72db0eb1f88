// associate_device.h — the launch sequence of dvs_associate / dvs_associate_candidates (frontend.hip) on device pointers, for callers that
// keep descriptors, pixels and landmark positions in HBM (backend.hip), as ransac_device.h does for the RANSAC stages.
#pragma once
#include "matcher.h"

namespace dvs {

int associate_hamming_bound(double max_descriptor_distance);   // the integer bound d < ... that (float)d < max_descriptor_distance means
// k_reproject_errors + k_assoc_argmin over the candidate triplets of matcher_thresh_*: d_err (total doubles) is scratch, d_best nobs ints
dvs_status associate_errors_device(dvs_matcher* ctx, const long long* d_offs, const int* d_pairs, long long total, const float* d_obs_px,
                                   const float* d_lm_xyz, int nobs, const double* d_Rt, double fx, double fy, double cx, double cy,
                                   double max_reprojection_distance, double* d_err, int* d_best);
// the whole of dvs_associate_candidates: candidates by Hamming bound, reprojection errors, arg-min.  d_best[i] = landmark row or -1;
// *d_offs (nobs + 1) / *d_pairs ((obs, landmark, distance) triplets in (obs, landmark) order) / *total stay valid until the context's
// next threshold match (NULL / 0 when nobs or nlm is 0).  Uses scratch slot 2.  d_Rt: R (9, row-major) then t (3), on the device.
dvs_status associate_rows_device(dvs_matcher* ctx, const uint8_t* d_obs_desc, const float* d_obs_px, int nobs, const uint8_t* d_lm_desc,
                                 const float* d_lm_xyz, int nlm, const double* d_Rt, double fx, double fy, double cx, double cy,
                                 double max_descriptor_distance, double max_reprojection_distance, int* d_best, const long long** d_offs,
                                 const int** d_pairs, long long* total);

}  // namespace dvs
