// loop_internal.h — what loop.hip (direct index, guided matching) and loop_verify.hip (rigid 3D-3D verification of the candidates) share:
// the handle and the one enqueue of the verification that the device form, the host form, detect_verify and the test hook all run.
// Internal to the library; nothing here is exported.
#pragma once
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "bow_internal.h"
#include "ransac_device.h"

struct dvs_loop_db {
  dvs_bow_db inv;              // the inverted part: bow.hip's, through bow_internal.h
  int di_levels = 0;
  long long rows_bound = 0;    // no fewer than the rows stored (device frames count as stride_rows until the count is read back)
  int max_stride = 0;          // the longest frame ever reserved: the width of a candidate's winner column
  size_t cap_e_off = 0, cap_e_nn = 0, cap_e_m = 0, cap_desc = 0, cap_nodes = 0, cap_start = 0, cap_feat = 0, cap_xyz = 0;
  size_t cap_keys = 0, cap_cand_ids = 0, cap_out_t = 0, cap_out_d = 0, cap_out_n = 0;
  dvs::DeviceBuf<long long> row_off;
  dvs::DeviceBuf<int> e_nn, e_m, fv_nodes, fv_start, fv_feat;
  dvs::DeviceBuf<uint4> desc;  // two per row
  // three floats per row, the entry keyframe's camera frame.  Every row at or past row_off[size] holds NaN (all bytes 0xff): a block is
  // filled that way when it grows and when the database is cleared, so an entry that was never given points has no valid point.
  dvs::DeviceBuf<float> xyz;
  dvs::DeviceBuf<unsigned long long> keys;   // [candidates][max_stride]: the smallest (d1 << 32 | i) that proposed entry feature j
  dvs::DeviceBuf<int> cand_ids;     // the host forms' candidate list: [0] the count, then the ids
  dvs::DeviceBuf<int> out_train, out_dist, out_n;   // the host forms' outputs
  std::vector<int> h_cand;
  // verification scratch (loop_verify.hip), grown on demand: per candidate slot its RansacProb (rows of the gathered list, the
  // candidate's seed), the gathered list (the query row of every correspondence and six planes of coordinates), H hypotheses with their
  // validity and counts, and the selection
  size_t cap_v_cand = 0, cap_v_list = 0, cap_v_hyp = 0, cap_v_in_xyz = 0, cap_v_in_train = 0, cap_v_res = 0, cap_v_mask = 0;
  dvs::DeviceBuf<dvs::RansacProb> v_probs;
  dvs::DeviceBuf<int> v_list_i, v_valid, v_counts, v_sel;
  dvs::DeviceBuf<float> v_pts;               // [candidates][6][stride_rows]: ex ey ez qx qy qz, plane by plane
  dvs::DeviceBuf<double> v_models;           // [candidates][H][12]: R row-major, t
  dvs::DeviceBuf<float> v_in_xyz;            // the host forms' staging and outputs
  dvs::DeviceBuf<int> v_in_train;
  dvs::DeviceBuf<dvs_loop_verify_result> v_res;
  dvs::DeviceBuf<uint8_t> v_mask;
};

namespace dvs {

// what the test hook additionally asks the kernels to leave behind (device pointers).  The product's calls pass no such struct.
struct LoopVerifyDebug {
  int* sample = nullptr;                     // [candidates][H][3]
  double* gap = nullptr;                     // [candidates][H]: (lambda1 - lambda2) / |lambda1|
  double* rounds = nullptr;                  // [candidates][9][16]: per refinement round R, t, |S_r|, accepted, fit not degenerate
};

// range checks of dvs_loop_verify_params (NULL: DVS_ERR_ARG, K4 has no default)
dvs_status loop_verify_check_params(const dvs_loop_verify_params* p, const char* what);
// the limits of one call, then (on the handle's device, which it makes current) the scratch for it; before any device work of the call
dvs_status loop_verify_reserve(dvs_loop_db* db, int cap_cand, int stride_rows, int H);
// gather, hypotheses, score, select, refine for cap_cand candidate slots, enqueued on the handle's stream (after loop_verify_reserve)
dvs_status loop_verify_enqueue(dvs_loop_db* db, const float* d_xyz_query, const int* d_n, int stride_rows, const int* d_entry_ids, const int* d_n_cand,
                               int cap_cand, const int* d_train_idx, const dvs_loop_verify_params& P, dvs_loop_verify_result* d_results,
                               uint8_t* d_inlier_mask, const LoopVerifyDebug* debug = nullptr);
// the host forms' staging (query points, train_idx) and output blocks (results, masks); makes the handle's device current
dvs_status loop_verify_host_blocks(dvs_loop_db* db, size_t cand, size_t n, bool train);

}  // namespace dvs
