// matcher.h — the matcher handle (dvs_matcher, include/dvslam_hip.h) and the internal entry points of match.hip that the other
// translation units use.  The handle is also the context of the glue (frontend.hip) and RANSAC (ransac.hip) entry points: its stream,
// its grow-only device scratch and its pinned in / out block.
#pragma once
#include "common.h"
#include "device_mem.h"
#include "io_host.h"

struct dvs_matcher {
  int device = 0;
  dvs::Stream own_stream;          // declared before the blocks: it outlives them
  hipStream_t stream = nullptr;    // own_stream or the caller's (dvs_matcher_create_on_stream, dvs_matcher_set_stream)
  // grow-only staging for the host entry points (dvs::grow): rows of 32 descriptor bytes, (idx | dist), the threshold match's passes
  dvs::DeviceBuf<uint8_t> d_q, d_t;
  dvs::DeviceBuf<int> d_idx, d_counts, d_pairs;
  dvs::DeviceBuf<long long> d_offs;
  size_t cq = 0, ct = 0, cidx = 0, ccounts = 0, cpairs = 0, coffs = 0;   // capacities in elements
  dvs::DeviceBuf<uint8_t> scratch[4];  // grow-only buffers of matcher_scratch
  size_t cscratch[4] = {0, 0, 0, 0};
  dvs::DeviceBuf<int> d_zero;      // 64 zero bytes: the empty predecessor of dvs_match_hamming_sequence_device
  int use_mfma = 1;                // DVS_MATCH_MFMA=0 keeps every job on the popcount kernels
  // pinned in / out block of the small host entry points: inputs are placed here and imported by a kernel, results are exported by a
  // kernel that publishes a sequence number the host polls — no copy commands, no stream wait
  dvs::PinnedIo io;
};

namespace dvs {

typedef unsigned long long u64;

// popcount(a XOR b) of two 256-bit descriptors (four 64-bit words each)
__device__ __forceinline__ int hamming256(const u64* a, const u64* b) {
  return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}

// Slot `slot` (0..3) of the handle's grow-only device scratch, at least `bytes` long.  A slot's contents live until the next call that
// takes the same slot, so entry points that nest must take different ones:
//   0  host staging of frontend.hip (dvs_bgr_to_gray input, dvs_filter_matches, dvs_backproject, dvs_publish_keyframe,
//      dvs_harris_responses) and of dvs_triangulate_landmarks and of every ransac.hip stage; the query rows of match_modes.hip's host entry points
//   1  dvs_bgr_to_gray output; the train rows of match_modes.hip's host entry points
//   2  dvs_associate*; the counts and outputs of match_modes.hip's host entry points
//   3  dvs_publish_keyframe_device's pose; the reverse arg-min of dvs_match_hamming_cross_batch_device; dvs_match_hamming_radius's sort;
//      the At rows of dvs_triangulate_landmarks* for landmarks with more than eight views
dvs_status matcher_scratch(dvs_matcher* m, int slot, size_t bytes, void** out);
// the pinned in / out block, at least `bytes` long (PinnedIo::reserve on the handle's stream)
inline dvs_status matcher_pinned(dvs_matcher* m, size_t bytes, PinnedIo** out) {
  DVS_TRY(m->io.reserve(m->stream, bytes));
  *out = &m->io;
  return DVS_OK;
}
// candidate pairs (Hamming < max_dist) as (q, t, dist) triplets in (q, t) order + per-query offsets, left on the device (own staging,
// no scratch slot); synchronises once for the total
dvs_status matcher_thresh_device(dvs_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, int max_dist, const long long** d_offs,
                                 const int** d_pairs, long long* total);
// enqueue k_scan_counts on st: single-workgroup exclusive scan of n int counts into 64-bit offsets, total at offs[n]
void launch_scan_counts(hipStream_t st, const int* counts, int n, long long* offs);
// the same on rows that already are on the device (16-byte aligned): nothing is copied
dvs_status matcher_thresh_rows_device(dvs_matcher* m, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int max_dist, const long long** d_offs,
                                      const int** d_pairs, long long* total);
// enqueue k_match_fp4<NQ, k> (1 <= k <= 4) for npairs jobs on st: outputs k (idx, dist) slots per query; q / t / t0 16-byte aligned,
// tStrideRows > 0; job 0 matches against t0 / nt0 when t0 is given
void launch_match_fp4(hipStream_t st, int k, int npairs, const uint8_t* q, const int* nq, int qStrideRows, const uint8_t* t, const int* nt,
                      int tStrideRows, const uint8_t* t0, const int* nt0, int* idx, int* dist);

}  // namespace dvs
