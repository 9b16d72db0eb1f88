// maptrack_internal.h — what reloc.hip reads of a map-tracking handle (dvs_maptrack, map_track.hip): its parameters and its device.
#pragma once
#include "common.h"

namespace dvs {
const dvs_maptrack_params& maptrack_params(const dvs_maptrack* h);
int maptrack_device(const dvs_maptrack* h);
}  // namespace dvs
