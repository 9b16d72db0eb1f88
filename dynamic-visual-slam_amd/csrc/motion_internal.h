// motion_internal.h — what tracker.hip uses of motion_seg.hip beside the C-ABI entry points of include/dvslam_hip.h
#pragma once
#include "common.h"

namespace dvs {

// the ranges of dvs_motion_params (include/dvslam_hip.h); DVS_ERR_ARG with the failed condition as the message
dvs_status motion_check_params(const dvs_motion_params& P);
// the statistics record of the handle's last call; waits for the handle's stream
dvs_status motion_last_stats(dvs_motion* h, dvs_motion_stats* out);

}  // namespace dvs
