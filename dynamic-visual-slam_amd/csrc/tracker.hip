// tracker.hip — the tracking front end as one handle and one call per RGB-D frame (include/dvslam_hip.h, dvs_tracker_*):
// Frontend::syncCallback (frontend.cpp:1068-1324) with keypoints, descriptors, matches, point lists and masks resident in HBM between the
// stages.  The image is copied up; the depth images stay in pinned host memory and are read at the keypoints (see dvs_tracker below).
//
// The stages are the library's own entry points in their device forms (extractor, filterDepth, Hamming match, the RANSAC launch
// sequences of ransac_device.h, Keyframe.msg CDR); what this file adds is the glue between them that used to run on the host:
//   k_compact_matches  match result + both keypoint blocks + Hamming bound -> (query, train) index lists and both float point lists, in
//                      query order, count on the device                                                  (frontend.cpp:1126-1142, 617-632)
//   k_compact_mask     the same lists under an inlier mask                                               (frontend.cpp:1150-1154)
//   k_cull             matched features first, then the unmatched ones in std::sort's order, cut, gathered (frontend.cpp:1171-1219)
//   k_pnp_points       3D-2D correspondences from the PREVIOUS depth image                               (frontend.cpp:859-892)
// All are one workgroup of four wavefronts per frame (n <= nfeatures + 3 nlevels rows): ordered compaction by wave64 ballot + prefix.
// The host sees fixed-size records only: one 256-byte block of counts and the PnP result, exported through a pinned block that the
// host polls (io_pinned.h), three times per frame — the branches of syncCallback (reset, >= 8, >= 5, >= 6, keyframe) are host decisions.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "backend_internal.h"
#include "common.h"
#include "cull_order.h"
#include "device_mem.h"
#include "io_pinned.h"
#include "matcher.h"
#include "motion_internal.h"
#include "orb_device_common.h"
#include "pose_host.h"
#include "ransac_device.h"
#include "block_ops.h"

namespace dvs {

constexpr int kTrkMaxCap = 3072;   // k_cull sorts in LDS: 20 bytes per unmatched feature (keys, two rank scratches, sorted keys)

// frontend.cpp:1126-1142 (and :617-632 against the last keyframe): matches with distance < max_dist, in query order; p_train / p_query
// are the .pt of the train (previous frame / last keyframe) and query (current frame) keypoints
__global__ __launch_bounds__(256) void k_compact_matches(const int* __restrict__ idx, const int* __restrict__ dist, const int* __restrict__ d_nq,
                                                         const int* __restrict__ d_nt, const dvs_keypoint* __restrict__ kq,
                                                         const dvs_keypoint* __restrict__ kt, int cap, int max_dist, int* __restrict__ q_out,
                                                         int* __restrict__ t_out, float* __restrict__ p_train, float* __restrict__ p_query,
                                                         int* __restrict__ n_out) {
  __shared__ int s_w[4];
  const int nq = min(max(*d_nq, 0), cap), nt = min(max(*d_nt, 0), cap);
  int done = 0;
  for (int i0 = 0; i0 < nq; i0 += 256) {
    const int i = i0 + threadIdx.x;
    int j = -1;
    bool keep = false;
    if (i < nq) { j = idx[i]; keep = j >= 0 && j < nt && dist[i] < max_dist; }
    int total;
    const int pos = done + block_rank256(keep, s_w, total);
    if (keep) {
      q_out[pos] = i; t_out[pos] = j;
      p_train[2 * pos] = kt[j].x; p_train[2 * pos + 1] = kt[j].y;
      p_query[2 * pos] = kq[i].x; p_query[2 * pos + 1] = kq[i].y;
    }
    done += total;
  }
  if (threadIdx.x == 0) *n_out = done;
}

// frontend.cpp:1150-1154: the lists under the inlier mask (any output list may be NULL: the keyframe gate only wants the count)
__global__ __launch_bounds__(256) void k_compact_mask(const unsigned char* __restrict__ mask, const int* __restrict__ d_n, int cap, const int* __restrict__ q_in,
                                                      const int* __restrict__ t_in, const float* __restrict__ p1_in, const float* __restrict__ p2_in,
                                                      int* __restrict__ q_out, int* __restrict__ t_out, float* __restrict__ p1_out,
                                                      float* __restrict__ p2_out, int* __restrict__ n_out) {
  __shared__ int s_w[4];
  const int n = min(max(*d_n, 0), cap);
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool keep = i < n && mask[i] != 0;
    int total;
    const int pos = done + block_rank256(keep, s_w, total);
    if (keep && q_out) {
      q_out[pos] = q_in[i]; t_out[pos] = t_in[i];
      p1_out[2 * pos] = p1_in[2 * i]; p1_out[2 * pos + 1] = p1_in[2 * i + 1];
      p2_out[2 * pos] = p2_in[2 * i]; p2_out[2 * pos + 1] = p2_in[2 * i + 1];
    }
    done += total;
  }
  if (threadIdx.x == 0) *n_out = done;
}

// frontend.cpp:1171-1219: backend set = the matched features in match order, then the unmatched ones as (response, index) pairs built in
// index order, sorted by std::sort under a.first > b.first (cull_order.h), cut at max_new or the first response < min_response.
// Gathers the 28-byte keypoints and 32-byte descriptor rows and writes the selection index.
__global__ __launch_bounds__(256) void k_cull(const dvs_keypoint* __restrict__ fk, const uint8_t* __restrict__ fd, const int* __restrict__ d_n,
                                              const int* __restrict__ q_list, const int* __restrict__ d_nq, int cap, int max_new, float min_response,
                                              dvs_keypoint* __restrict__ bk, uint8_t* __restrict__ bd, int* __restrict__ sel, int* __restrict__ n_out,
                                              int* __restrict__ heap_ranges /* test hook: ranges that met the depth limit; NULL otherwise */) {
  __shared__ unsigned long long s_keys[kTrkMaxCap];
  __shared__ int s_Lp[kTrkMaxCap], s_Rp[kTrkMaxCap];
  __shared__ uint32_t s_k32[kTrkMaxCap];
  __shared__ uint32_t s_matched[kTrkMaxCap / 32];
  __shared__ int s_stack[3 * 64];
  __shared__ int s_w[4];
  __shared__ int s_m;
  const int n = min(max(*d_n, 0), cap), nq = min(max(*d_nq, 0), cap);
  for (int w = threadIdx.x; w < kTrkMaxCap / 32; w += 256) s_matched[w] = 0u;
  __syncthreads();
  for (int e = threadIdx.x; e < nq; e += 256) {          // :1175-1190
    const int i = q_list[e];
    sel[e] = i;
    if (i >= 0 && i < n) atomicOr(&s_matched[i >> 5], 1u << (i & 31));
  }
  __syncthreads();
  int nun = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {                  // :1193-1198, index order
    const int i = i0 + threadIdx.x;
    const bool un = i < n && !((s_matched[i >> 5] >> (i & 31)) & 1u);
    int total;
    const int pos = nun + block_rank256(un, s_w, total);
    if (un) s_keys[pos] = cull_key(fk[i].response, i);
    nun += total;
  }
  __syncthreads();
  // :1201-1202 std::sort, in lsort.h's rank-pairing form (cull_order.h states it for the host): wavefront 0 walks the introsort's ranges
  // with an explicit stack — each partition is wave_partition<32>, ranges are disjoint so their order is free — and marks every range of
  // <= 16 elements as a leaf (first | end << 16 in s_Lp, which a finished range no longer needs as scratch)
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64 && nun > 0) {
    int lg = 0;
    for (int v = nun; v > 1; v >>= 1) lg++;
    int sp = 0;
    if (lane == 0) { s_stack[0] = 0; s_stack[1] = nun; s_stack[2] = 2 * lg; }
    sp = 1;
    wave_lds_fence();
    while (sp > 0) {
      sp--;
      const int f = s_stack[3 * sp], l = s_stack[3 * sp + 1], d = s_stack[3 * sp + 2];
      wave_lds_fence();
      if (l - f <= 16) {
        if (lane < l - f) s_Lp[f + lane] = f | (l << 16);
      } else if (d == 0) {                               // depth limit: std::__partial_sort, every element its own leaf
        if (lane == 0) { lsort::heap_sort_all(s_keys + f, s_keys + l, lsort::Less<32>()); if (heap_ranges) atomicAdd(heap_ranges, 1); }
        for (int i = f + lane; i < l; i += 64) s_Lp[i] = i | ((i + 1) << 16);
      } else {
        const int cut = wave_partition<32>(s_keys, s_Lp, s_Rp, f, l, lane);
        if (lane == 0) {
          s_stack[3 * sp] = cut; s_stack[3 * sp + 1] = l; s_stack[3 * sp + 2] = d - 1;
          s_stack[3 * sp + 3] = f; s_stack[3 * sp + 4] = cut; s_stack[3 * sp + 5] = d - 1;
        }
        sp += 2;
      }
      wave_lds_fence();
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nun; i += 256) {         // leaves (__final_insertion_sort): stable placement by rank within the leaf
    const int fl = s_Lp[i];
    const int f = fl & 0xFFFF, l = fl >> 16;
    const unsigned long long ke = s_keys[i] >> 32;
    int rnk = f;
    for (int j = f; j < l; j++) {
      const unsigned long long kj = s_keys[j] >> 32;
      rnk += (kj < ke || (kj == ke && j < i)) ? 1 : 0;
    }
    s_Rp[i] = rnk;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nun; i += 256) { s_Lp[s_Rp[i]] = (int)(uint32_t)s_keys[i]; s_k32[s_Rp[i]] = (uint32_t)(s_keys[i] >> 32); }
  __syncthreads();
  if (threadIdx.x == 0) s_m = cull_cut(s_k32, nun, max_new, min_response);   // :1205-1210
  __syncthreads();
  const int m = min(s_m, cap - nq), nb = nq + m;
  for (int e = threadIdx.x; e < m; e += 256) sel[nq + e] = s_Lp[e];
  if (threadIdx.x == 0) *n_out = nb;
  __threadfence_block();
  __syncthreads();
  const uint32_t* fk32 = reinterpret_cast<const uint32_t*>(fk); uint32_t* bk32 = reinterpret_cast<uint32_t*>(bk);
  const uint32_t* fd32 = reinterpret_cast<const uint32_t*>(fd); uint32_t* bd32 = reinterpret_cast<uint32_t*>(bd);
  for (int w = threadIdx.x; w < nb * 7; w += 256) {      // keypoints: 7 dwords each
    const int e = w / 7, c = w - 7 * e, i = sel[e];
    if (i >= 0 && i < n) bk32[w] = fk32[7 * (size_t)i + c];
  }
  for (int w = threadIdx.x; w < nb * 8; w += 256) {      // descriptor rows: 8 dwords each
    const int e = w >> 3, c = w & 7, i = sel[e];
    if (i >= 0 && i < n) bd32[w] = fd32[8 * (size_t)i + c];
  }
}

// frontend.cpp:859-892: float arithmetic, std::round, bounds check, d <= min || d > max rejected; the depth image is the PREVIOUS frame's
__global__ __launch_bounds__(256) void k_pnp_points(const float* __restrict__ p_prev, const float* __restrict__ p_cur, const int* __restrict__ d_n, int cap,
                                                    const uint16_t* __restrict__ depth, int rows, int cols, float fx, float fy, float cx, float cy,
                                                    float min_depth, float max_depth, float* __restrict__ obj, float* __restrict__ img,
                                                    int* __restrict__ n_out) {
  __shared__ int s_w[4];
  const int n = min(max(*d_n, 0), cap);
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    bool keep = false;
    float px = 0.f, py = 0.f, d = 0.f;
    if (i < n) {
      px = p_prev[2 * i]; py = p_prev[2 * i + 1];
      const int x = (int)roundf(px), y = (int)roundf(py);
      if (x >= 0 && y >= 0 && x < cols && y < rows) {
        d = (float)depth[(size_t)y * cols + x] * 0.001f;
        keep = !(d <= min_depth || d > max_depth);
      }
    }
    int total;
    const int pos = done + block_rank256(keep, s_w, total);
    if (keep) {
      obj[3 * pos] = (px - cx) * d / fx; obj[3 * pos + 1] = (py - cy) * d / fy; obj[3 * pos + 2] = d;
      img[2 * pos] = p_cur[2 * i]; img[2 * pos + 1] = p_cur[2 * i + 1];
    }
    done += total;
  }
  if (threadIdx.x == 0) *n_out = done;
}

__global__ __launch_bounds__(256) void k_iota(int* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = i;
}

}  // namespace dvs

using namespace dvs;

// The record block: what the kernels count and what the estimators leave, exported whole to a pinned copy after each group of launches.
// A kernel takes an int* to ONE counter.  f[p] / b[bw]: the depth-filtered and the backend set of the frame in slot p / bw.
struct TrackRec {
  int ext, f[2], match, geo, pnp, b[2], kfmatch, kfgeo, cdrn;
  int pad0[5];
  PnpRecord pnp_rec;
  SelRecord sel;         // pnp_mode 1 alone
  uint64_t cdr_size;
  uint8_t pad1[104];
};
static_assert(sizeof(TrackRec) == 256 && offsetof(TrackRec, pnp_rec) == 64 && offsetof(TrackRec, sel) == 128 && offsetof(TrackRec, cdr_size) == 144, "record layout");

// the motion-mask opt-in (dvs_tracker_set_motion_mask): empty while it is off, and torn down by assigning an empty one
struct MotionSlot { int64_t frame = -1; bool pose_updated = false; PoseRt T; };
struct Motion {
  Owned<dvs_motion, dvs_motion_destroy> seg;
  int lag = 0;
  DeviceBuf<uint16_t> ring;                        // lag + 1 depth images: frame f lives in slot f % (lag + 1)
  DeviceBuf<uint8_t> mask;
  MotionSlot slot[17];
  int seq = 0;                                     // frames of the current sequence in the ring (it begins at a first frame / a tracking reset)
  bool after_reset = false;                        // the previous frame reset the tracking
  int64_t ref = -1;                                // the last frame's reference (-1: its extraction was unmasked)
  double R[9], t[3];                               // ... and the relative pose its mask was made with
  void reset_state() { seq = 0; after_reset = false; ref = -1; for (auto& s : slot) s.frame = -1; }
};

struct dvs_tracker {
  dvs_tracker_params P;
  int device = 0, cap = 0;
  Owned<dvs_orb, dvs_orb_destroy> orb;             // owns the stream: the first member, destroyed last
  Owned<dvs_matcher, dvs_matcher_destroy> ctx;
  // frame buffers
  DeviceBuf<uint8_t> d_img, d_gray, d_cdr;
  Column<uint8_t, 1, 16> d_mask;
  DeviceBuf<TrackRec> d_rec;
  // current / prev_frame_depth_, in PINNED host memory: the kernels read the few thousand pixels under the keypoints over PCIe (as
  // dvs_filter_depth does), the image itself is staged here and copied: the extractor reads all of it many times
  PinnedBuf<uint16_t> d_depth[2];
  PinnedBuf<uint8_t> h_img;
  // one row per feature: extracted, depth-filtered (current / prev_kps_), backend sets (this frame's / last keyframe's)
  Column<dvs_keypoint> d_kraw, f_k[2], b_k[2];
  Column<uint8_t, 32> d_draw, f_d[2], b_d[2];
  Column<int> d_idx, d_dist, c_q, c_t, g_q, g_t, k_q, k_t, b_sel, d_inl;
  Column<float, 2> c_p1, c_p2, g_p1, g_p2, k_p1, k_p2, o_img;
  Column<float, 3> o_obj;
  PinnedBuf<TrackRec> h_rec;                       // the exported record block + the sequence number the host polls
  PinnedBuf<int> h_seq;
  int seq = 0;
  size_t cdr_cap_dev = 0;
  // Frontend's members
  bool prev_valid = false, has_last_kf = false;    // prev_frame_valid_, has_last_keyframe_
  int p = 0;                                       // f_*[p] / d_depth[p] receive the current frame; [1 - p] hold prev_kps_ / prev_descriptors_ / prev_frame_depth_
  int prev_n = 0;                                  // prev_kps_.size()
  int bkf = 0, kf_n = 0;                           // b_*[bkf] = last_keyframe_keypoints_ / _descriptors_
  int blast = 0, last_n = 0;                       // the last frame's culled set (dvs_tracker_get_backend_features)
  int since_kf = 0;                                // frames_since_last_keyframe_
  int64_t keyframe_id = 0, t = 0;                  // keyframe_id_; frames since create / reset
  double R[9], tt[3];                              // R_, t_
  Motion mo;                                       // the last member: destroyed before ctx and orb
};

// what the stages of one dvs_tracker_track call share
struct TrackCall {
  const int p, q, bw;                              // this frame's / the previous frame's slot; where this frame's backend set goes (the last keyframe's stays)
  const int64_t t;
  int n_f = 0, n_match = 0, n_backend = 0, n_kfm = 0;   // counts read so far
  const int* d_ng = nullptr;                       // the device count of the geometrically consistent matches (geo, or match when the gate was skipped)
  bool kf_match = false, kf_run = false, do_pnp = false, kf_gate = false, publish = false;
};

static void tracker_reset_state(dvs_tracker* h) {
  h->prev_valid = false; h->has_last_kf = false; h->p = 0; h->prev_n = 0; h->bkf = 0; h->kf_n = 0; h->blast = 0; h->last_n = 0;
  h->since_kf = 0; h->keyframe_id = 0; h->t = 0;
  for (int k = 0; k < 9; k++) h->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  h->tt[0] = h->tt[1] = h->tt[2] = 0.0;
  h->mo.reset_state();
}

// the record block to the host: export kernel + polled sequence number (no copy command, no stream wait)
static dvs_status tracker_export(dvs_tracker* h) {
  return io_export_wait(h->ctx->stream, h->d_rec.get(), h->h_rec.get(), sizeof(TrackRec), h->h_seq.get(), ++h->seq);
}

static dvs_status tracker_fm(dvs_tracker* h, const float* p1, const float* p2, const int* d_n, int n, unsigned long long seed) {
  const dvs_tracker_params& P = h->P;
  if (P.fm_mode == 1) return fm_cv_device(h->ctx.get(), p1, p2, n, P.fm_threshold, P.fm_confidence, P.fm_max_iters, h->d_mask.get());
  return fm_own_device(h->ctx.get(), p1, p2, d_n, n, seed, P.fm_threshold, P.fm_confidence, P.fm_max_iters, h->d_mask.get());
}

static unsigned long long frame_seed(const dvs_tracker* h, int64_t t, unsigned long long stage) { return h->P.seed_base + 2ull * (unsigned long long)t + stage; }

static void copy_pose(const dvs_tracker* h, dvs_track_result* out) {
  for (int k = 0; k < 9; k++) out->R[k] = h->R[k];
  for (int k = 0; k < 3; k++) out->t[k] = h->tt[k];
}

// ---- the stages of dvs_tracker_track, in the order it runs them ----

// frontend.cpp:1084: the image and the depth image to their pinned blocks (row by row where the caller's rows are padded), the image up,
// BGR -> gray.  *d_gray: what the extractor reads
static dvs_status upload_frame(dvs_tracker* h, const TrackCall& C, const uint8_t* image, int channels, size_t step, const uint16_t* depth_u16, size_t depth_step,
                               const uint8_t** d_gray) {
  const dvs_tracker_params& P = h->P;
  const int rows = P.rows, cols = P.cols;
  const size_t irow = (size_t)cols * channels, drow = (size_t)cols * sizeof(uint16_t);
  if (step == irow) memcpy(h->h_img.get(), image, irow * rows);
  else for (int r = 0; r < rows; r++) memcpy(h->h_img.get() + r * irow, image + r * step, irow);
  if (depth_step == drow) memcpy(h->d_depth[C.p].get(), depth_u16, drow * rows);
  else for (int r = 0; r < rows; r++) memcpy((uint8_t*)h->d_depth[C.p].get() + r * drow, (const uint8_t*)depth_u16 + r * depth_step, drow);
  DVS_HIP(hipMemcpyAsync(h->d_img.get(), h->h_img.get(), irow * rows, hipMemcpyHostToDevice, h->ctx->stream));
  *d_gray = h->d_img.get();
  if (channels == 3) {
    DVS_TRY(dvs_bgr_to_gray_device(h->ctx.get(), h->d_img.get(), 1, rows, cols, irow, 0, h->d_gray.get(), cols, 0, P.gray_variant));
    *d_gray = h->d_gray.get();
  }
  return DVS_OK;
}

// the motion mask of this frame (opt-in): its depth image into the ring, and — when the reference slot holds the frame the lag asks
// for — the segmentation against it under the predicted relative pose.  *d_keep = NULL: the unmasked extraction, as ever
static dvs_status choose_motion_mask(dvs_tracker* h, const TrackCall& C, const uint8_t** d_keep) {
  *d_keep = nullptr;
  Motion& M = h->mo;
  if (!M.seg) return DVS_OK;
  const int ns = M.lag + 1;
  const size_t px = (size_t)h->P.rows * h->P.cols, drow = (size_t)h->P.cols * sizeof(uint16_t);
  uint16_t* d_cur = M.ring.get() + (size_t)(C.t % ns) * px;
  DVS_HIP(hipMemcpyAsync(d_cur, h->d_depth[C.p].get(), px * sizeof(uint16_t), hipMemcpyHostToDevice, h->ctx->stream));
  M.ref = -1;
  if (!h->prev_valid || M.after_reset || M.seq < 1) return DVS_OK;
  const int64_t ref = C.t - std::min(M.lag, M.seq);
  const MotionSlot& rs = M.slot[ref % ns];
  if (rs.frame != ref) return DVS_OK;
  const MotionSlot& a = M.slot[(C.t - 1) % ns];   // T(t-1); T(t-2) where there is one: constant-velocity prediction
  relative_pose(a.T, (a.pose_updated && M.seq >= 2) ? &M.slot[(C.t - 2) % ns].T : nullptr, rs.T, M.R, M.t);
  DVS_TRY(dvs_motion_segment_device(M.seg.get(), M.ring.get() + (size_t)(ref % ns) * px, drow, d_cur, drow, M.R, M.t, M.mask.get(), h->P.cols, nullptr));
  M.ref = ref;
  *d_keep = M.mask.get();
  return DVS_OK;
}

// :1094 / :1285 extract; :1100 / :1291 filterDepth
static dvs_status extract_and_filter(dvs_tracker* h, const TrackCall& C, const uint8_t* d_gray, const uint8_t* d_keep) {
  const dvs_tracker_params& P = h->P;
  const int rows = P.rows, cols = P.cols, cap = h->cap;
  TrackRec* d = h->d_rec.get();
  if (d_keep) DVS_TRY(dvs_orb_extract_batch_device_masked(h->orb.get(), d_gray, 1, rows, cols, cols, (size_t)rows * cols, d_keep, cols, 0, h->d_kraw.get(),
                                                          h->d_draw.get(), cap, &d->ext));
  else DVS_TRY(dvs_orb_extract_batch_device(h->orb.get(), d_gray, 1, rows, cols, cols, (size_t)rows * cols, h->d_kraw.get(), h->d_draw.get(), cap, &d->ext));
  return dvs_filter_depth_batch_device(h->ctx.get(), h->d_kraw.get(), h->d_draw.get(), &d->ext, cap, 1, h->d_depth[C.p].get(), rows, cols,
                                       (size_t)cols * sizeof(uint16_t), 0, P.min_depth, P.max_depth, h->f_k[C.p].get(), h->f_d[C.p].get(), nullptr, &d->f[C.p]);
}

// :1123 match, :1126-1132 distance filter (enqueued before the counts are known: an empty frame gives no matches)
static dvs_status match_previous(dvs_tracker* h, const TrackCall& C) {
  const int p = C.p, q = C.q, cap = h->cap;
  TrackRec* d = h->d_rec.get();
  DVS_TRY(dvs_match_hamming_batch_device(h->ctx.get(), h->f_d[p].get(), &d->f[p], cap, h->f_d[q].get(), &d->f[q], cap, 1, h->d_idx.get(), h->d_dist.get()));
  hipLaunchKernelGGL(k_compact_matches, dim3(1), dim3(256), 0, h->ctx->stream, h->d_idx.get(), h->d_dist.get(), &d->f[p], &d->f[q], h->f_k[p].get(), h->f_k[q].get(),
                     cap, h->P.max_hamming, h->c_q.get(), h->c_t.get(), h->c_p1.get(), h->c_p2.get(), &d->match);
  return DVS_OK;
}

// :1278-1312 first frame: all depth-filtered features are the initial keyframe
static dvs_status first_frame(dvs_tracker* h, TrackCall& C, dvs_track_result* out) {
  const int p = C.p, bw = C.bw, n_f = C.n_f;
  hipStream_t st = h->ctx->stream;
  TrackRec* d = h->d_rec.get();
  out->first_frame = 1;
  if (n_f > 0) {
    DVS_HIP(hipMemcpyAsync(h->b_k[bw].get(), h->f_k[p].get(), (size_t)n_f * h->f_k[p].row_bytes, hipMemcpyDeviceToDevice, st));
    DVS_HIP(hipMemcpyAsync(h->b_d[bw].get(), h->f_d[p].get(), (size_t)n_f * h->f_d[p].row_bytes, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_iota, dim3((n_f + 255) / 256), dim3(256), 0, st, h->b_sel.get(), n_f);
  }
  DVS_HIP(hipMemcpyAsync(&d->b[bw], &d->f[p], sizeof(int), hipMemcpyDeviceToDevice, st));
  C.n_backend = n_f;
  C.publish = true; out->kf_criterion = DVS_KF_FIRST_FRAME;
  return DVS_OK;
}

// :1136-1166 the fundamental-matrix gate from 8 matches on, else the distance-filtered set; :1171-1219 feature culling; :859-892 the 3D-2D
// correspondences of estimateCameraPose, from prev_frame_depth_; :611-623 isKeyframe's match against the last keyframe (it depends on the
// culled set alone)
static dvs_status gate_cull_and_points(dvs_tracker* h, TrackCall& C, dvs_track_result* out) {
  const dvs_tracker_params& P = h->P;
  const int p = C.p, q = C.q, bw = C.bw, cap = h->cap;
  hipStream_t st = h->ctx->stream;
  TrackRec* d = h->d_rec.get();
  const int* gq = h->c_q.get();
  const float *gp1 = h->c_p1.get(), *gp2 = h->c_p2.get();
  C.d_ng = &d->match;
  if (C.n_match >= 8) {
    DVS_TRY(tracker_fm(h, h->c_p1.get(), h->c_p2.get(), &d->match, C.n_match, frame_seed(h, C.t, 0ull)));
    hipLaunchKernelGGL(k_compact_mask, dim3(1), dim3(256), 0, st, h->d_mask.get(), &d->match, cap, h->c_q.get(), h->c_t.get(), h->c_p1.get(), h->c_p2.get(),
                       h->g_q.get(), h->g_t.get(), h->g_p1.get(), h->g_p2.get(), &d->geo);
    gq = h->g_q.get(); gp1 = h->g_p1.get(); gp2 = h->g_p2.get(); C.d_ng = &d->geo;
  } else {
    out->fm_skipped = 1;
  }
  hipLaunchKernelGGL(k_cull, dim3(1), dim3(256), 0, st, h->f_k[p].get(), h->f_d[p].get(), &d->f[p], gq, C.d_ng, cap, P.cull_max_new, P.cull_min_response,
                     h->b_k[bw].get(), h->b_d[bw].get(), h->b_sel.get(), &d->b[bw], (int*)nullptr);
  hipLaunchKernelGGL(k_pnp_points, dim3(1), dim3(256), 0, st, gp1, gp2, C.d_ng, cap, h->d_depth[q].get(), P.rows, P.cols, (float)P.fx, (float)P.fy, (float)P.cx,
                     (float)P.cy, P.min_depth, P.max_depth, h->o_obj.get(), h->o_img.get(), &d->pnp);
  C.kf_match = h->has_last_kf && h->kf_n > 0;
  if (C.kf_match) {
    const int bkf = h->bkf;
    DVS_TRY(dvs_match_hamming_batch_device(h->ctx.get(), h->b_d[bw].get(), &d->b[bw], cap, h->b_d[bkf].get(), &d->b[bkf], cap, 1, h->d_idx.get(), h->d_dist.get()));
    hipLaunchKernelGGL(k_compact_matches, dim3(1), dim3(256), 0, st, h->d_idx.get(), h->d_dist.get(), &d->b[bw], &d->b[bkf], h->b_k[bw].get(), h->b_k[bkf].get(),
                       cap, P.max_hamming, h->k_q.get(), h->k_t.get(), h->k_p1.get(), h->k_p2.get(), &d->kfmatch);
  }
  return DVS_OK;
}

// :1237 / :899 PnP wants >= 5 matches and >= 6 points; :627 the keyframe gate >= 8 matches.  Reads the second export's counts
static dvs_status pnp_and_keyframe_gate(dvs_tracker* h, TrackCall& C, dvs_track_result* out) {
  const dvs_tracker_params& P = h->P;
  const TrackRec& rec = *h->h_rec.get();
  TrackRec* d = h->d_rec.get();
  const int n_geo = C.n_match >= 8 ? rec.geo : C.n_match, n_pnp = rec.pnp;
  C.n_backend = rec.b[C.bw];
  out->n_geometric = n_geo;
  C.kf_run = C.kf_match && C.n_backend > 0;          // :611
  C.n_kfm = C.kf_run ? rec.kfmatch : 0;
  C.do_pnp = n_geo >= 5 && n_pnp >= 6;
  if (n_geo >= 5) out->n_pnp_points = n_pnp;
  if (!C.do_pnp) out->pnp_skipped = 1;
  const double K4[4] = {P.fx, P.fy, P.cx, P.cy};
  if (C.do_pnp) {
    if (P.pnp_mode == 1) DVS_TRY(pnp_cv_device(h->ctx.get(), h->o_obj.get(), h->o_img.get(), n_pnp, K4, P.pnp_iterations, P.pnp_reproj_err, P.pnp_confidence, h->d_inl.get(), &d->pnp_rec, &d->sel));
    else DVS_TRY(pnp_own_device(h->ctx.get(), h->o_obj.get(), h->o_img.get(), &d->pnp, frame_seed(h, C.t, 1ull), K4, P.pnp_iterations, P.pnp_reproj_err, P.pnp_confidence,
                                h->d_inl.get(), &d->pnp_rec));
  }
  C.kf_gate = C.kf_run && C.n_kfm >= 8;
  if (C.kf_gate) {
    DVS_TRY(tracker_fm(h, h->k_p1.get(), h->k_p2.get(), &d->kfmatch, C.n_kfm, frame_seed(h, C.t, 1000003ull)));
    hipLaunchKernelGGL(k_compact_mask, dim3(1), dim3(256), 0, h->ctx->stream, h->d_mask.get(), &d->kfmatch, h->cap, (const int*)nullptr, (const int*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (int*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr, &d->kfgeo);
  }
  return DVS_OK;
}

// :925-948 the PnP result into R_, t_ (pose_host.h), unless PnP failed or the motion is an outlier.  Reads the third export's record
static void pose_update(dvs_tracker* h, dvs_track_result* out) {
  const TrackRec& rec = *h->h_rec.get();
  const PnpRecord& r = rec.pnp_rec;
  const bool have = h->P.pnp_mode == 1 ? rec.sel.best >= 0 : r.success != 0;
  if (have) { memcpy(out->rvec, r.rvec, sizeof(r.rvec)); memcpy(out->tvec, r.tvec, sizeof(r.tvec)); }
  if (!r.success) { out->pnp_failed = 1; return; }
  out->n_pnp_inliers = r.n_inliers;
  if (pose_step(h->R, h->tt, out->rvec, out->tvec, h->P.max_translation, h->P.max_rotation)) out->pose_updated = 1;
  else out->motion_outlier = 1;
}

// :601-662 isKeyframe
static void decide_keyframe(dvs_tracker* h, TrackCall& C, dvs_track_result* out) {
  const int n_kfg = C.kf_gate ? h->h_rec.get()->kfgeo : C.n_kfm;
  if (C.kf_run) { out->n_kf_matches = C.n_kfm; out->n_kf_geometric = n_kfg; }   // (kf_run: there is a last keyframe)
  const KeyframeDecision k = keyframe_decision(h->has_last_kf, C.kf_run, n_kfg, h->since_kf, h->P);
  h->has_last_kf = true;
  h->since_kf = k.since_kf;
  C.publish = k.publish;
  if (k.publish) out->kf_criterion = k.criterion;
}

// :699-790 publishKeyframe: pose -> quaternion, CDR payload on the device (and the call's last wait) when the caller wants one, last
// keyframe := this frame's backend set.  *ret = DVS_ERR_CAPACITY where cdr_out is too small: the frame still counts
static dvs_status publish_keyframe(dvs_tracker* h, const TrackCall& C, int32_t stamp_sec, uint32_t stamp_nanosec, dvs_track_result* out, uint8_t* cdr_out,
                                   size_t cdr_cap, dvs_status* ret) {
  const dvs_tracker_params& P = h->P;
  const int bw = C.bw;
  hipStream_t st = h->ctx->stream;
  out->is_keyframe = 1;
  out->keyframe_id = h->keyframe_id;
  if (cdr_out) {
    TrackRec* d = h->d_rec.get();
    dvs_keyframe_header hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.stamp_sec = stamp_sec; hdr.stamp_nanosec = stamp_nanosec; hdr.frame_id = "camera_link"; hdr.keyframe_id = (uint64_t)h->keyframe_id;
    rotation_to_quat_xyzw(h->R, hdr.rotation_xyzw);
    for (int k = 0; k < 3; k++) hdr.translation[k] = h->tt[k];
    DVS_TRY(dvs_publish_keyframe_device(h->ctx.get(), &hdr, h->b_k[bw].get(), h->b_d[bw].get(), C.n_backend, h->d_depth[C.p].get(), P.rows, P.cols,
                                        (size_t)P.cols * sizeof(uint16_t), (float)P.fx, (float)P.fy, (float)P.cx, (float)P.cy, h->R, h->tt, h->d_cdr.get(), h->cdr_cap_dev,
                                        &d->cdr_size, &d->cdrn));
    DVS_TRY(tracker_export(h));
    const TrackRec& rec = *h->h_rec.get();
    const uint64_t sz = rec.cdr_size;
    out->cdr_bytes = sz; out->cdr_landmarks = rec.cdrn;
    if (sz > cdr_cap) {
      set_error("keyframe payload needs %llu bytes, cdr_out has %zu", (unsigned long long)sz, cdr_cap);
      *ret = DVS_ERR_CAPACITY;
    } else {
      DVS_HIP(hipMemcpyAsync(cdr_out, h->d_cdr.get(), (size_t)sz, hipMemcpyDeviceToHost, st));
      DVS_HIP(hipStreamSynchronize(st));
    }
  }
  h->keyframe_id++;                                   // :729
  h->bkf = bw; h->kf_n = C.n_backend;                 // :779-780
  return DVS_OK;
}

// :1258-1259, 1274-1275 / :1299-1312: this frame becomes the previous one
static void advance(dvs_tracker* h, const TrackCall& C, const dvs_track_result* out) {
  Motion& M = h->mo;
  if (M.seg) {   // this frame's pose beside its depth image in the ring; a first frame and a tracking reset begin a sequence
    MotionSlot& s = M.slot[C.t % (M.lag + 1)];
    s.frame = C.t; s.pose_updated = out->pose_updated != 0;
    memcpy(s.T.R, h->R, sizeof(s.T.R)); memcpy(s.T.t, h->tt, sizeof(s.T.t));
    const bool begins = out->first_frame || out->tracking_reset;
    M.seq = begins ? 1 : std::min(M.seq + 1, M.lag + 1);
    M.after_reset = out->tracking_reset != 0;
  }
  h->p = C.q; h->prev_n = C.n_f; h->prev_valid = true; h->t = C.t + 1;
}

// the prologue of the three calls against a map: the device, an idle stream, and the last frame's depth-filtered set — advance() made
// it the "previous" one, f_*[1 - p] with prev_n rows.  After a frame with tracking_reset the set may be empty
static dvs_status last_filtered_set(dvs_tracker* h, const dvs_backend* backend, bool others, const char* who, const dvs_keypoint** d_kps, const uint8_t** d_desc) {
  DVS_ARG(h && backend && others && backend->device == h->device);
  if (!h->prev_valid) { set_error("%s: no frame has been tracked", who); return DVS_ERR_EMPTY; }
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  *d_kps = h->f_k[1 - h->p].get(); *d_desc = h->f_d[1 - h->p].get();
  return DVS_OK;
}
static void apply_pose(dvs_tracker* h, bool apply, const double* R9, const double* t3) {
  if (apply) { memcpy(h->R, R9, sizeof(h->R)); memcpy(h->tt, t3, sizeof(h->tt)); }
}

extern "C" {

void dvs_tracker_default_params(dvs_tracker_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->orb.nfeatures = 1000; p->orb.scale_factor = 1.2f; p->orb.nlevels = 8; p->orb.ini_th_fast = 20; p->orb.min_th_fast = 7;   // frontend.cpp:206
  p->min_depth = 0.3f; p->max_depth = 3.0f;
  p->max_hamming = 50;
  p->fm_threshold = 2.0; p->fm_confidence = 0.99; p->fm_max_iters = 1000;
  p->cull_max_new = 200; p->cull_min_response = 50.0f;
  p->pnp_iterations = 100; p->pnp_reproj_err = 4.0; p->pnp_confidence = 0.99;
  p->kf_min_matches = 150; p->kf_max_frames = 30;
  p->max_translation = 0.5; p->max_rotation = 0.2;
}

dvs_status dvs_tracker_create(const dvs_tracker_params* params, int32_t device, dvs_tracker** out) {
  DVS_ARG(params && out);
  *out = nullptr;
  const dvs_tracker_params& P = *params;
  DVS_ARG(P.rows > 0 && P.cols > 0 && P.fx > 0 && P.fy > 0);
  DVS_ARG((P.fm_mode == 0 || P.fm_mode == 1) && (P.pnp_mode == 0 || P.pnp_mode == 1) && (P.gray_variant == 0 || P.gray_variant == 1));
  DVS_ARG(P.fm_max_iters >= 1 && P.fm_max_iters <= 4096 && P.fm_threshold > 0 && P.pnp_iterations >= 1 && P.pnp_iterations <= 1024 && P.pnp_reproj_err > 0);
  DVS_ARG(P.pnp_confidence > 0 && P.pnp_confidence < 1 && P.cull_max_new >= 0 && P.max_hamming >= 0);
  DVS_TRY(check_device(device));
  dvs_tracker* h = new (std::nothrow) dvs_tracker();
  if (!h) { set_error("dvs_tracker_create: out of memory"); return DVS_ERR_HIP; }
  h->P = P; h->device = device;
  tracker_reset_state(h);
  auto create_all = [&]() -> dvs_status {
    dvs_orb_params op = P.orb;
    op.max_batch = 1;
    dvs_orb* orb = nullptr;
    DVS_TRY(dvs_orb_create(&op, device, &orb));
    h->orb.reset(orb);
    dvs_matcher* ctx = nullptr;
    DVS_TRY(dvs_matcher_create_on_stream(device, dvs_orb_get_stream(orb), &ctx));   // one stream: every stage depends on the one before
    h->ctx.reset(ctx);
    h->cap = dvs_orb_max_keypoints(orb);
    if (h->cap > kTrkMaxCap) { set_error("dvs_tracker_create: %d keypoints per frame, the culling kernel holds %d", h->cap, kTrkMaxCap); return DVS_ERR_UNSUPPORTED; }
    const size_t px = (size_t)P.rows * P.cols;
    DVS_TRY(h->d_img.alloc(px * 3)); DVS_TRY(h->d_gray.alloc(px)); DVS_TRY(h->h_img.alloc(px * 3));
    DVS_TRY(h->d_depth[0].alloc(px)); DVS_TRY(h->d_depth[1].alloc(px));
    DVS_TRY(alloc_rows((size_t)h->cap, h->d_kraw, h->f_k[0], h->f_k[1], h->b_k[0], h->b_k[1], h->d_draw, h->f_d[0], h->f_d[1], h->b_d[0], h->b_d[1], h->d_mask,
                       h->d_idx, h->d_dist, h->c_q, h->c_t, h->g_q, h->g_t, h->k_q, h->k_t, h->b_sel, h->d_inl,
                       h->c_p1, h->c_p2, h->g_p1, h->g_p2, h->k_p1, h->k_p2, h->o_img, h->o_obj));
    h->cdr_cap_dev = dvs_keyframe_cdr_capacity("camera_link", h->cap);
    DVS_TRY(h->d_cdr.alloc(h->cdr_cap_dev + 64));
    DVS_TRY(h->d_rec.alloc(1)); DVS_TRY(h->h_rec.alloc(1)); DVS_TRY(h->h_seq.alloc(16));
    *h->h_seq.get() = 0;
    DVS_HIP(hipMemset(h->d_rec.get(), 0, sizeof(TrackRec)));
    // scratch slot 0 of the context at its largest (the own estimators' hypotheses), so that no frame allocates
    void* dummy;
    const size_t fm_b = (size_t)P.fm_max_iters * 3 * 80 + (size_t)P.fm_max_iters * 28 + 4096, pnp_b = (size_t)P.pnp_iterations * 4 * 104 + (size_t)P.pnp_iterations * 164 + 4096;
    return matcher_scratch(ctx, 0, std::max(fm_b, pnp_b), &dummy);
  };
  const dvs_status s = create_all();
  if (s != DVS_OK) { dvs_tracker_destroy(h); return s; }
  *out = h;
  return DVS_OK;
}

void dvs_tracker_destroy(dvs_tracker* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->ctx) (void)hipStreamSynchronize(h->ctx->stream);
  delete h;   // the motion handle, the context, the extractor (and its stream), in that order
}

dvs_status dvs_tracker_synchronize(dvs_tracker* h) {
  DVS_ARG(h);
  DVS_TRY(dvs_orb_synchronize(h->orb.get()));
  return dvs_matcher_synchronize(h->ctx.get());
}

dvs_status dvs_tracker_reset(dvs_tracker* h) {
  DVS_ARG(h);
  DVS_TRY(dvs_tracker_synchronize(h));
  tracker_reset_state(h);
  return DVS_OK;
}

dvs_status dvs_tracker_set_stream(dvs_tracker* h, void* hip_stream) {
  DVS_ARG(h);
  DVS_TRY(dvs_tracker_synchronize(h));
  DVS_TRY(dvs_orb_set_stream(h->orb.get(), hip_stream));
  if (h->mo.seg) DVS_TRY(dvs_motion_set_stream(h->mo.seg.get(), hip_stream));
  return dvs_matcher_set_stream(h->ctx.get(), hip_stream);
}

// Frontend::syncCallback (frontend.cpp:1068-1324).  The host waits for the record block three times on the tracking path (and once more
// for a payload): every branch below is a host decision on counts of the export before it.
dvs_status dvs_tracker_track(dvs_tracker* h, const uint8_t* image, int32_t channels, size_t step, const uint16_t* depth_u16, size_t depth_step,
                             int32_t stamp_sec, uint32_t stamp_nanosec, dvs_track_result* out, uint8_t* cdr_out, size_t cdr_cap) {
  DVS_ARG(h && out);
  memset(out, 0, sizeof(*out));
  out->keyframe_id = -1; out->n_kf_matches = -1; out->n_kf_geometric = -1;
  DVS_ARG(image && depth_u16 && (channels == 1 || channels == 3) && step >= (size_t)h->P.cols * channels && depth_step >= (size_t)h->P.cols * sizeof(uint16_t));
  DVS_HIP(hipSetDevice(h->device));
  TrackCall C{h->p, 1 - h->p, 1 - h->bkf, h->t};
  out->frame_index = C.t;
  h->last_n = 0;   // until this frame's culled set is complete: a call that fails half-way leaves no set to read back (reset the handle after an error)
  const uint8_t *d_gray, *d_keep;
  DVS_TRY(upload_frame(h, C, image, channels, step, depth_u16, depth_step, &d_gray));
  DVS_TRY(choose_motion_mask(h, C, &d_keep));
  DVS_TRY(extract_and_filter(h, C, d_gray, d_keep));
  if (h->prev_valid && h->prev_n > 0) DVS_TRY(match_previous(h, C));
  DVS_TRY(tracker_export(h));                                   // ---- the first wait: extracted, filtered, matched
  const TrackRec& rec = *h->h_rec.get();
  C.n_f = rec.f[C.p];
  out->n_extracted = rec.ext; out->n_filtered = C.n_f;
  copy_pose(h, out);
  if (!h->prev_valid) {
    DVS_TRY(first_frame(h, C, out));
  } else if (C.n_f == 0 || h->prev_n == 0) {                    // :1107-1117 reset: the state is replaced, no pose change, no keyframe
    out->tracking_reset = 1;
    advance(h, C, out);
    return DVS_OK;
  } else {
    out->n_matches = C.n_match = rec.match;
    DVS_TRY(gate_cull_and_points(h, C, out));
    DVS_TRY(tracker_export(h));                                 // ---- the second: consistent matches, PnP points, backend set, keyframe matches
    DVS_TRY(pnp_and_keyframe_gate(h, C, out));
    if (C.do_pnp || C.kf_gate) DVS_TRY(tracker_export(h));      // ---- the third: the PnP record, the keyframe gate's count
    if (C.do_pnp) pose_update(h, out);
    copy_pose(h, out);
    decide_keyframe(h, C, out);
  }
  out->n_backend = C.n_backend;
  h->blast = C.bw; h->last_n = C.n_backend;
  dvs_status ret = DVS_OK;
  if (C.publish) DVS_TRY(publish_keyframe(h, C, stamp_sec, stamp_nanosec, out, cdr_out, cdr_cap, &ret));
  advance(h, C, out);
  return ret;
}

dvs_status dvs_tracker_get_backend_features(dvs_tracker* h, dvs_keypoint* kps, uint8_t* desc, int32_t* sel_index, int32_t cap, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->last_n;
  if (h->last_n > cap) { set_error("dvs_tracker_get_backend_features: %d rows, capacity %d", h->last_n, cap); return DVS_ERR_CAPACITY; }
  if (h->last_n == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const size_t m = (size_t)h->last_n;
  DVS_TRY(copy_out(kps, h->b_k[h->blast], m, st)); DVS_TRY(copy_out(desc, h->b_d[h->blast], m, st)); DVS_TRY(copy_out(sel_index, h->b_sel, m, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

dvs_status dvs_tracker_set_motion_mask(dvs_tracker* h, const dvs_motion_params* p, int32_t lag) {
  DVS_ARG(h);
  dvs_motion_params mp;
  if (p) {
    DVS_ARG(lag >= 1 && lag <= 16);
    mp = *p;
    mp.rows = h->P.rows; mp.cols = h->P.cols; mp.fx = h->P.fx; mp.fy = h->P.fy; mp.cx = h->P.cx; mp.cy = h->P.cy;
    DVS_TRY(motion_check_params(mp));
  }
  DVS_TRY(dvs_tracker_synchronize(h));
  DVS_HIP(hipSetDevice(h->device));
  h->mo = Motion();   // off: the segmentation handle, then the ring and the mask
  if (!p) return DVS_OK;
  const size_t px = (size_t)h->P.rows * h->P.cols;
  Motion M;           // complete, or gone with this scope
  dvs_motion* seg = nullptr;
  DVS_TRY(dvs_motion_create(&mp, h->device, &seg));
  M.seg.reset(seg);
  DVS_TRY(dvs_motion_set_stream(seg, h->ctx->stream));
  DVS_TRY(M.ring.alloc(px * (size_t)(lag + 1))); DVS_TRY(M.mask.alloc(px));
  M.lag = lag;
  h->mo = std::move(M);
  return DVS_OK;
}

dvs_status dvs_tracker_get_motion_mask(dvs_tracker* h, uint8_t* mask, size_t step, double* R9, double* t3, int64_t* ref_frame_index, dvs_motion_stats* stats) {
  DVS_ARG(h && (!mask || step >= (size_t)h->P.cols));
  const Motion& M = h->mo;
  const bool used = M.seg && M.ref >= 0;
  if (ref_frame_index) *ref_frame_index = used ? M.ref : -1;
  for (int k = 0; k < 9; k++) if (R9) R9[k] = used ? M.R[k] : (k % 4 == 0 ? 1.0 : 0.0);
  for (int k = 0; k < 3; k++) if (t3) t3[k] = used ? M.t[k] : 0.0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!used) {
    if (mask) for (int r = 0; r < h->P.rows; r++) memset(mask + (size_t)r * step, 255, (size_t)h->P.cols);
    return DVS_OK;
  }
  DVS_HIP(hipSetDevice(h->device));
  if (stats) DVS_TRY(motion_last_stats(M.seg.get(), stats));
  if (mask) {
    DVS_HIP(hipMemcpy2DAsync(mask, step, M.mask.get(), (size_t)h->P.cols, (size_t)h->P.cols, (size_t)h->P.rows, hipMemcpyDeviceToHost, h->ctx->stream));
    DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  }
  return DVS_OK;
}

// the last frame's depth-filtered set: dvs_tracker_track's advance() made it the "previous" one, f_*[1 - p] with prev_n rows
dvs_status dvs_tracker_get_filtered_features(dvs_tracker* h, dvs_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  const int m = h->prev_valid ? h->prev_n : 0;
  *n = m;
  if (m > cap) { set_error("dvs_tracker_get_filtered_features: %d rows, capacity %d", m, cap); return DVS_ERR_CAPACITY; }
  if (m == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const int q = 1 - h->p;
  DVS_TRY(copy_out(kps, h->f_k[q], (size_t)m, st)); DVS_TRY(copy_out(desc, h->f_d[q], (size_t)m, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

// include/dvslam_hip.h "Tracking against the map": the last filtered set against the backend's landmark table, prior R_, t_; the tracker
// itself launches nothing here
dvs_status dvs_tracker_track_map(dvs_tracker* h, dvs_backend* backend, dvs_maptrack* mt, int32_t apply, dvs_maptrack_result* result) {
  const dvs_keypoint* d_kps; const uint8_t* d_desc;
  DVS_TRY(last_filtered_set(h, backend, mt && result, "dvs_tracker_track_map", &d_kps, &d_desc));
  DVS_TRY(dvs_backend_track_frame(backend, mt, d_kps, d_desc, h->prev_n, h->R, h->tt, result));
  apply_pose(h, apply && result->status == DVS_MAPTRACK_OK, result->R, result->t);
  return DVS_OK;
}

// include/dvslam_hip.h "Landmark refresh": the same through the gated call
dvs_status dvs_tracker_track_map_gated(dvs_tracker* h, dvs_backend* backend, dvs_maptrack* mt, const dvs_maptrack_gates* gates, int32_t apply,
                                       dvs_maptrack_result* result) {
  const dvs_keypoint* d_kps; const uint8_t* d_desc;
  DVS_TRY(last_filtered_set(h, backend, mt && result, "dvs_tracker_track_map_gated", &d_kps, &d_desc));
  DVS_TRY(dvs_backend_track_frame_gated(backend, mt, gates, d_kps, d_desc, h->prev_n, h->R, h->tt, result));
  apply_pose(h, apply && result->status == DVS_MAPTRACK_OK, result->R, result->t);
  return DVS_OK;
}

// include/dvslam_hip.h "Relocalisation": that set against the table with no prior.  An empty set: FEW_PAIRS, not an error
dvs_status dvs_tracker_relocalize(dvs_tracker* h, dvs_backend* backend, dvs_reloc* reloc, dvs_maptrack* mt, int32_t apply, dvs_reloc_result* result) {
  const dvs_keypoint* d_kps; const uint8_t* d_desc;
  DVS_TRY(last_filtered_set(h, backend, reloc && mt && result, "dvs_tracker_relocalize", &d_kps, &d_desc));
  DVS_TRY(dvs_backend_relocalize_frame(backend, reloc, mt, d_kps, d_desc, h->prev_n, result));
  apply_pose(h, apply && result->status == DVS_RELOC_OK, result->R, result->t);
  return DVS_OK;
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test.h)
// pose_host.h as the tracker calls it (no GPU)
int32_t dvs_test_tracker_pose_step(double* R9, double* t3, const double* rvec3, const double* tvec3, double max_translation, double max_rotation,
                                   double* rodrigues9) {
  if (rodrigues9) rodrigues(rvec3, rodrigues9);
  return pose_step(R9, t3, rvec3, tvec3, max_translation, max_rotation) ? 1 : 0;
}
void dvs_test_tracker_relative_pose(const double* a12, const double* b12, const double* ref12, double* R9, double* t3, double* quat_xyzw4) {
  PoseRt a, b, ref;
  memcpy(&a, a12, sizeof(a)); memcpy(&ref, ref12, sizeof(ref));
  if (b12) memcpy(&b, b12, sizeof(b));
  relative_pose(a, b12 ? &b : nullptr, ref, R9, t3);
  if (quat_xyzw4) rotation_to_quat_xyzw(a.R, quat_xyzw4);
}
// the same order through k_cull itself (needs a GPU): keypoints that carry the responses, the matched indices as the match list
dvs_status dvs_test_cull_order_device(const float* response, const uint8_t* matched, int32_t n, int32_t max_new, float min_response, int32_t* order,
                                      int32_t* n_out, int32_t* heap_ranges) {
  DVS_ARG(n >= 0 && n <= kTrkMaxCap && n_out && (n == 0 || (response && matched && order)));
  *n_out = 0;
  if (heap_ranges) *heap_ranges = 0;
  if (n == 0) return DVS_OK;
  DVS_TRY(check_device(0));
  std::vector<dvs_keypoint> k((size_t)n);
  std::vector<int> q, head(4, 0);
  for (int i = 0; i < n; i++) { memset(&k[i], 0, sizeof(dvs_keypoint)); k[i].response = response[i]; if (matched[i]) q.push_back(i); }
  head[0] = n; head[1] = (int)q.size();
  q.resize((size_t)n);
  DeviceBuf<dvs_keypoint> d_k; DeviceBuf<int> d_q, d_head;
  Column<dvs_keypoint> d_bk; Column<uint8_t, 32> d_d, d_bd; Column<int> d_sel;
  DVS_TRY(d_k.upload(k)); DVS_TRY(d_q.upload(q)); DVS_TRY(d_head.upload(head));
  DVS_TRY(alloc_rows((size_t)n, d_bk, d_d, d_bd, d_sel));
  DVS_HIP(hipMemset(d_d.get(), 0, (size_t)n * d_d.row_bytes));
  hipLaunchKernelGGL(k_cull, dim3(1), dim3(256), 0, (hipStream_t) nullptr, d_k.get(), d_d.get(), d_head.get(), d_q.get(), d_head.get() + 1, n, max_new, min_response,
                     d_bk.get(), d_bd.get(), d_sel.get(), d_head.get() + 2, d_head.get() + 3);
  DVS_HIP(hipGetLastError());
  std::vector<int> sel((size_t)n);
  DVS_HIP(hipMemcpy(head.data(), d_head.get(), head.size() * sizeof(int), hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel.data(), d_sel.get(), (size_t)n * d_sel.row_bytes, hipMemcpyDeviceToHost));
  const int m = head[2] - head[1];
  for (int e = 0; e < m; e++) order[e] = sel[(size_t)head[1] + e];
  *n_out = m;
  if (heap_ranges) *heap_ranges = head[3];
  return DVS_OK;
}
void dvs_test_cull_order(const float* response, const uint8_t* matched, int32_t n, int32_t max_new, float min_response, int32_t* order, int32_t* n_out) {
  std::vector<uint64_t> keys;
  for (int i = 0; i < n; i++) if (!matched[i]) keys.push_back(cull_key(response[i], i));
  std::vector<int> lp(keys.size() + 1), rp(keys.size() + 1);
  std::vector<uint32_t> k32(keys.size() + 1);
  const int m = cull_sort_and_cut(keys.data(), (int)keys.size(), max_new, min_response, lp.data(), rp.data(), k32.data());
  for (int e = 0; e < m; e++) order[e] = (int)(uint32_t)keys[e];
  *n_out = m;
}
#endif

}  // extern "C"
