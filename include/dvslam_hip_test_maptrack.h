/*
 * dvslam_hip_test_maptrack.h — the test hooks of the tracking against the map (csrc/map_track.hip), part of dvslam_hip_test.h, which
 * includes it: exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.
 * Why a header of its own: tests/test_host_logic.py::test_exports_every_declared_symbol pins the list of dvs_test_* declarations in the
 * text of dvslam_hip_test.h itself, and existing tests stay as they are (dvslam_hip_test_loop.h is the precedent).
 */
#ifndef DVSLAM_HIP_TEST_MAPTRACK_H
#define DVSLAM_HIP_TEST_MAPTRACK_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* what stages 1-3 leave per landmark (40 bytes): u = v = 0 unless visible; best_k = d_best = -1 without a candidate, d_second = -1
 * without another one */
typedef struct dvs_maptrack_lm_record {
  double u, v;
  int32_t visible, best_k, d_best, d_second, proposed, kept;
} dvs_maptrack_lm_record;

/* (needs a GPU) the per-landmark records of the handle's LAST search / track call; count-then-capacity, *n = that call's n_lm */
dvs_status dvs_test_maptrack_landmarks(dvs_maptrack* h, int32_t cap, dvs_maptrack_lm_record* rec, int32_t* n);
/* (needs a GPU) the cell CSR of that call: cell_start[*n_cells + 1] over the cells in row-major order and the binned keypoints' indices
 * in CSR order (order[*n_binned]); count-then-capacity on both, either output nullable */
dvs_status dvs_test_maptrack_cells(dvs_maptrack* h, int32_t cap_cells, int32_t cap_kp, int32_t* cell_start, int32_t* order, int32_t* n_cells,
                                   int32_t* n_binned);
/* (needs a GPU) dvs_maptrack_refine_device's launch with a part of its schedule, so that single Gauss-Newton steps can be compared: rounds
 * first_round .. first_round + n_rounds - 1 of n_iters steps each (the product runs 0, 4, 10).  Round r is robust iff r < 2, r counted
 * from first_round; every pair counts as an inlier before the first round that runs; all pairs are reclassified after every round that
 * runs, and cost, flags, FEW_MATCHES, FEW_INLIERS and DEGENERATE are as in the product after the last of them.  DVS_ERR_ARG outside
 * 0 <= first_round, 1 <= n_rounds, first_round + n_rounds <= 4, 1 <= n_iters <= 10. */
dvs_status dvs_test_maptrack_refine_steps(dvs_maptrack* h, const double* d_X, const double* d_px, const int32_t* d_octave, int32_t n, const double* R9,
                                          const double* t3, int32_t first_round, int32_t n_rounds, int32_t n_iters, dvs_maptrack_result* result);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_MAPTRACK_H */
