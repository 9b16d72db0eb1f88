// maptrack_internal.h — what map_track.hip and reloc.hip share: what reloc.hip reads of a map-tracking handle (dvs_maptrack: its
// parameters and its device), and the staging of their host forms, which upload the same five arrays and call their device forms.
#pragma once
#include "common.h"
#include "device_mem.h"

namespace dvs {
const dvs_maptrack_params& maptrack_params(const dvs_maptrack* h);
int maptrack_device(const dvs_maptrack* h);

// A landmark table and a frame's keypoints on the device, for a call that got them as host arrays: two row groups that only grow.
struct FrameStaging {
  Column<float, 3> xyz; Column<uint8_t, 32> ldesc; Column<long long> id;   // per landmark
  size_t cap_lm = 0;
  Column<dvs_keypoint> kps; Column<uint8_t, 32> kdesc;                     // per keypoint
  size_t cap_kp = 0;
  // the ids as the device forms take them: NULL where the caller gave none
  const int64_t* ids(const int64_t* lm_id, int n_lm) const { return (lm_id && n_lm > 0) ? (const int64_t*)id.get() : nullptr; }
};

// Checks what the device forms cannot (every keypoint inside M's image and octave table, ids ascending), then enqueues the uploads on
// `st`; a group that must grow is freed after the stream has drained, so nothing in flight reads what is freed.  The counts are the
// caller's to bound.
inline dvs_status stage_frame(FrameStaging& s, const dvs_maptrack_params& M, int device, hipStream_t st, const float* lm_xyz, const uint8_t* lm_desc,
                              const int64_t* lm_id, int n_lm, const dvs_keypoint* kps, const uint8_t* desc, int n_kp) {
  for (int k = 0; k < n_kp; k++)
    DVS_ARG(kps[k].x >= 0.f && kps[k].x < (float)M.cols && kps[k].y >= 0.f && kps[k].y < (float)M.rows && kps[k].octave >= 0 && kps[k].octave < M.n_levels);
  if (lm_id) for (int j = 1; j < n_lm; j++) DVS_ARG(lm_id[j - 1] < lm_id[j]);
  DVS_HIP(hipSetDevice(device));
  const size_t nl = (size_t)n_lm, nk = (size_t)n_kp;
  if (nl > s.cap_lm || nk > s.cap_kp) DVS_HIP(hipStreamSynchronize(st));
  DVS_TRY(grow_rows(s.cap_lm, nl, nl + nl / 4, s.xyz, s.ldesc, s.id));
  DVS_TRY(grow_rows(s.cap_kp, nk, nk + nk / 4, s.kps, s.kdesc));
  if (n_lm > 0) {
    DVS_TRY(copy_in(s.xyz, lm_xyz, nl, st)); DVS_TRY(copy_in(s.ldesc, lm_desc, nl, st));
    if (lm_id) DVS_TRY(copy_in(s.id, lm_id, nl, st));
  }
  if (n_kp > 0) { DVS_TRY(copy_in(s.kps, kps, nk, st)); DVS_TRY(copy_in(s.kdesc, desc, nk, st)); }
  return DVS_OK;
}
}  // namespace dvs
