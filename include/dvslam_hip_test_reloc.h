/*
 * dvslam_hip_test_reloc.h — the test hooks of the relocalisation (csrc/reloc.hip), part of dvslam_hip_test.h, which includes it: exported
 * by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.  A header of its own for the reason
 * dvslam_hip_test_maptrack.h gives.
 */
#ifndef DVSLAM_HIP_TEST_RELOC_H
#define DVSLAM_HIP_TEST_RELOC_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* what stages 1-2 leave per landmark (20 bytes): best_k = d_best = -1 where nothing was compared (a position that is not finite, or no
 * keypoint), d_second = -1 without another keypoint; kept: the landmark's proposal is the one its keypoint keeps */
typedef struct dvs_reloc_lm_record {
  int32_t best_k, d_best, d_second, proposed, kept;
} dvs_reloc_lm_record;

/* (needs a GPU) the per-landmark records of the handle's LAST locate call; count-then-capacity, *n = that call's n_lm */
dvs_status dvs_test_reloc_landmarks(dvs_reloc* h, int32_t cap, dvs_reloc_lm_record* rec, int32_t* n);
/* (no device work) stage 4's record of that call as it came back from the device, in dvs_solve_pnp_ransac's terms: the result struct holds
 * only its host conversion.  Zeros when nothing was solved (status FEW_PAIRS). */
dvs_status dvs_test_reloc_pnp_record(dvs_reloc* h, int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_RELOC_H */
