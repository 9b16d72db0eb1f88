/*
 * dvslam_hip_test_motion.h — the test hooks of the motion segmentation (csrc/motion_seg.hip), part of dvslam_hip_test.h, which includes
 * it: exported by libdvslam_hip_test.so (-DDVS_TEST_HOOKS) only, never by the product library.
 * Why a header of its own: tests/test_host_logic.py::test_exports_every_declared_symbol pins the list of dvs_test_* declarations in the
 * text of dvslam_hip_test.h itself, and existing tests stay as they are (dvslam_hip_test_loop.h is the precedent).
 */
#ifndef DVSLAM_HIP_TEST_MOTION_H
#define DVSLAM_HIP_TEST_MOTION_H
#include <stdint.h>
#include "dvslam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the labelling's tile: a tile-local union-find per DVS_MOTION_TILE x DVS_MOTION_TILE block, then the merge across tile borders */
#define DVS_MOTION_TILE 32

/* (needs a GPU) the three labelling launches of dvs_motion_segment_device on an arbitrary binary image (host, rows x cols packed, nonzero =
 * set; 1..4096 each): labels[rows * cols] (smallest linear index of the component, -1 off the set) and areas[rows * cols] (the pixel
 * count at each component's root, 0 elsewhere) */
dvs_status dvs_test_motion_label(int32_t device, const uint8_t* img, int32_t rows, int32_t cols, int32_t* labels, int32_t* areas);
/* (needs a GPU) what the stages of the handle's LAST call left on the device, each rows x cols packed and nullable: the seed image
 * (0 / 1), the labels, the dynamic image (0 / 1) */
dvs_status dvs_test_motion_stages(dvs_motion* h, uint8_t* seed, int32_t* labels, uint8_t* dynamic);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_TEST_MOTION_H */
