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

// cv::Rodrigues(rvec) in double, explicit order of operations (tests/tracker_ref.py restates it operation for operation)
static void rodrigues(const double* w, double* R) {
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  if (th < 1e-15) { for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0; return; }
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const double c = cos(th), s = sin(th), c1 = 1.0 - c;
  const double K[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = ((i == j ? c : 0.0) + c1 * (k[i] * k[j])) + s * K[3 * i + j];
}

}  // namespace dvs

using namespace dvs;

// slots of the device count block (int32 each); the block is exported whole
enum { C_EXT = 0, C_F0 = 1, C_F1 = 2, C_MATCH = 3, C_GEO = 4, C_PNP = 5, C_B0 = 6, C_B1 = 7, C_KFMATCH = 8, C_KFGEO = 9, C_CDRN = 10, C_INTS = 16 };
// record block: [C_INTS ints | PnP record 64 B | PnP selection 16 B | CDR size 8 B | pad] = 256 bytes
static const size_t kRecPnp = 64, kRecSel = 128, kRecCdr = 144, kRecBytes = 256;

struct dvs_tracker {
  dvs_tracker_params P;
  int device = 0, cap = 0;
  dvs_orb* orb = nullptr;
  dvs_matcher* ctx = nullptr;
  // frame buffers
  DeviceBuf<uint8_t> d_img, d_gray, d_kraw, d_draw, d_cdr, d_mask, d_rec;
  // current / prev_frame_depth_, in PINNED host memory: the kernels read the few thousand pixels under the keypoints over PCIe (as
  // dvs_filter_depth does), the image itself is staged here and copied: the extractor reads all of it many times
  PinnedBuf<uint16_t> d_depth[2];
  PinnedBuf<uint8_t> h_img;
  DeviceBuf<dvs_keypoint> f_k[2], b_k[2];          // depth-filtered (current / prev_kps_), backend sets (this frame's / last keyframe's)
  DeviceBuf<uint8_t> f_d[2], b_d[2];
  DeviceBuf<int> d_idx, d_dist, c_q, c_t, g_q, g_t, k_q, k_t, b_sel, d_inl;
  DeviceBuf<float> c_p1, c_p2, g_p1, g_p2, k_p1, k_p2, o_obj, o_img;
  PinnedBuf<uint8_t> h_rec;                        // the exported record block + the sequence number the host polls
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
  // the motion-mask opt-in (dvs_tracker_set_motion_mask); everything below is empty while it is off
  struct MotionSlot { int64_t frame = -1; bool pose_updated = false; double R[9], t[3]; };
  dvs_motion* mo = nullptr;
  int mo_lag = 0;
  DeviceBuf<uint16_t> mo_ring;                     // mo_lag + 1 depth images: frame f lives in slot f % (mo_lag + 1)
  DeviceBuf<uint8_t> mo_mask;
  MotionSlot mo_slot[17];
  int mo_seq = 0;                                  // frames of the current sequence in the ring (it begins at a first frame / a tracking reset)
  bool mo_after_reset = false;                     // the previous frame reset the tracking
  int64_t mo_ref = -1;                             // the last frame's reference (-1: its extraction was unmasked)
  double mo_R[9], mo_t[3];                         // ... and the relative pose its mask was made with
};

// the relative pose of dvs_tracker_set_motion_mask for frame t: constant-velocity prediction against slot `ref`.  Every product is a plain
// row-by-column sum in index order (tests recompute it from the returned poses to 1e-12, not bit for bit).
static void motion_relative_pose(const dvs_tracker* h, int64_t t, const dvs_tracker::MotionSlot& ref, double* R, double* tr) {
  const int ns = h->mo_lag + 1;
  const dvs_tracker::MotionSlot& a = h->mo_slot[(t - 1) % ns];   // T(t-1)
  double Rp[9], tp[3];
  memcpy(Rp, a.R, sizeof(Rp)); memcpy(tp, a.t, sizeof(tp));
  if (a.pose_updated && h->mo_seq >= 2) {
    const dvs_tracker::MotionSlot& b = h->mo_slot[(t - 2) % ns];   // T(t-2)
    double Rrel[9], trel[3];                                      // T(t-2)^-1 o T(t-1)
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Rrel[3 * i + j] = b.R[i] * a.R[j] + b.R[3 + i] * a.R[3 + j] + b.R[6 + i] * a.R[6 + j];
      trel[i] = b.R[i] * (a.t[0] - b.t[0]) + b.R[3 + i] * (a.t[1] - b.t[1]) + b.R[6 + i] * (a.t[2] - b.t[2]);
    }
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Rp[3 * i + j] = a.R[3 * i] * Rrel[j] + a.R[3 * i + 1] * Rrel[3 + j] + a.R[3 * i + 2] * Rrel[6 + j];
      tp[i] = a.R[3 * i] * trel[0] + a.R[3 * i + 1] * trel[1] + a.R[3 * i + 2] * trel[2] + a.t[i];
    }
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[3 * i + j] = ref.R[i] * Rp[j] + ref.R[3 + i] * Rp[3 + j] + ref.R[6 + i] * Rp[6 + j];
    tr[i] = ref.R[i] * (tp[0] - ref.t[0]) + ref.R[3 + i] * (tp[1] - ref.t[1]) + ref.R[6 + i] * (tp[2] - ref.t[2]);
  }
}

static void motion_reset_state(dvs_tracker* h) {
  h->mo_seq = 0; h->mo_after_reset = false; h->mo_ref = -1;
  for (auto& s : h->mo_slot) s.frame = -1;
}

static void tracker_reset_state(dvs_tracker* h) {
  h->prev_valid = false; h->has_last_kf = false; h->p = 0; h->prev_n = 0; h->bkf = 0; h->kf_n = 0; h->blast = 0; h->last_n = 0;
  h->since_kf = 0; h->keyframe_id = 0; h->t = 0;
  for (int k = 0; k < 9; k++) h->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  h->tt[0] = h->tt[1] = h->tt[2] = 0.0;
  motion_reset_state(h);
}

// the record block to the host: export kernel + polled sequence number (no copy command, no stream wait)
static dvs_status tracker_export(dvs_tracker* h) {
  return io_export_wait(h->ctx->stream, h->d_rec.get(), h->h_rec.get(), kRecBytes, h->h_seq.get(), ++h->seq);
}

static dvs_status tracker_fm(dvs_tracker* h, const float* p1, const float* p2, const int* d_n, int n, unsigned long long seed, unsigned char* mask) {
  const dvs_tracker_params& P = h->P;
  if (P.fm_mode == 1) return fm_cv_device(h->ctx, p1, p2, n, P.fm_threshold, P.fm_confidence, P.fm_max_iters, mask);
  return fm_own_device(h->ctx, p1, p2, d_n, n, seed, P.fm_threshold, P.fm_confidence, P.fm_max_iters, mask);
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
  dvs_orb_params op = P.orb;
  op.max_batch = 1;
  dvs_status s = dvs_orb_create(&op, device, &h->orb);
  if (s == DVS_OK) s = dvs_matcher_create_on_stream(device, dvs_orb_get_stream(h->orb), &h->ctx);   // one stream: every stage depends on the one before
  if (s == DVS_OK) {
    h->cap = dvs_orb_max_keypoints(h->orb);
    if (h->cap > kTrkMaxCap) { set_error("dvs_tracker_create: %d keypoints per frame, the culling kernel holds %d", h->cap, kTrkMaxCap); s = DVS_ERR_UNSUPPORTED; }
  }
  auto alloc_all = [&]() -> dvs_status {
    const size_t cap = (size_t)h->cap, px = (size_t)P.rows * P.cols;
    DVS_TRY(h->d_img.alloc(px * 3)); DVS_TRY(h->d_gray.alloc(px)); DVS_TRY(h->h_img.alloc(px * 3));
    for (int k = 0; k < 2; k++) {
      DVS_TRY(h->d_depth[k].alloc(px));
      DVS_TRY(h->f_k[k].alloc(cap)); DVS_TRY(h->f_d[k].alloc(cap * 32)); DVS_TRY(h->b_k[k].alloc(cap)); DVS_TRY(h->b_d[k].alloc(cap * 32));
    }
    DVS_TRY(h->d_kraw.alloc(cap * sizeof(dvs_keypoint))); DVS_TRY(h->d_draw.alloc(cap * 32));
    DVS_TRY(h->d_mask.alloc(cap + 16)); DVS_TRY(h->d_rec.alloc(kRecBytes));
    DeviceBuf<int>* ib[] = {&h->d_idx, &h->d_dist, &h->c_q, &h->c_t, &h->g_q, &h->g_t, &h->k_q, &h->k_t, &h->b_sel, &h->d_inl};
    for (auto* b : ib) DVS_TRY(b->alloc(cap));
    DeviceBuf<float>* fb[] = {&h->c_p1, &h->c_p2, &h->g_p1, &h->g_p2, &h->k_p1, &h->k_p2, &h->o_img};
    for (auto* b : fb) DVS_TRY(b->alloc(cap * 2));
    DVS_TRY(h->o_obj.alloc(cap * 3));
    h->cdr_cap_dev = dvs_keyframe_cdr_capacity("camera_link", h->cap);
    DVS_TRY(h->d_cdr.alloc(h->cdr_cap_dev + 64));
    DVS_TRY(h->h_rec.alloc(kRecBytes)); DVS_TRY(h->h_seq.alloc(16));
    *h->h_seq.get() = 0;
    DVS_HIP(hipMemset(h->d_rec.get(), 0, kRecBytes));
    // scratch slot 0 of the context at its largest (the own estimators' hypotheses), so that no frame allocates
    void* dummy;
    const size_t fm_b = (size_t)P.fm_max_iters * 3 * 80 + (size_t)P.fm_max_iters * 28 + 4096, pnp_b = (size_t)P.pnp_iterations * 4 * 104 + (size_t)P.pnp_iterations * 164 + 4096;
    DVS_TRY(matcher_scratch(h->ctx, 0, std::max(fm_b, pnp_b), &dummy));
    return DVS_OK;
  };
  if (s == DVS_OK) s = alloc_all();
  if (s != DVS_OK) { dvs_tracker_destroy(h); return s; }
  *out = h;
  return DVS_OK;
}

void dvs_tracker_destroy(dvs_tracker* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->ctx) (void)hipStreamSynchronize(h->ctx->stream);
  if (h->mo) dvs_motion_destroy(h->mo);
  if (h->ctx) dvs_matcher_destroy(h->ctx);
  if (h->orb) dvs_orb_destroy(h->orb);
  delete h;
}

dvs_status dvs_tracker_synchronize(dvs_tracker* h) {
  DVS_ARG(h);
  DVS_TRY(dvs_orb_synchronize(h->orb));
  return dvs_matcher_synchronize(h->ctx);
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
  DVS_TRY(dvs_orb_set_stream(h->orb, hip_stream));
  if (h->mo) DVS_TRY(dvs_motion_set_stream(h->mo, hip_stream));
  return dvs_matcher_set_stream(h->ctx, hip_stream);
}

dvs_status dvs_tracker_track(dvs_tracker* h, const uint8_t* image, int32_t channels, size_t step, const uint16_t* depth_u16, size_t depth_step,
                             int32_t stamp_sec, uint32_t stamp_nanosec, dvs_track_result* out, uint8_t* cdr_out, size_t cdr_cap) {
  DVS_ARG(h && out);
  memset(out, 0, sizeof(*out));
  out->keyframe_id = -1; out->n_kf_matches = -1; out->n_kf_geometric = -1;
  const dvs_tracker_params& P = h->P;
  const int rows = P.rows, cols = P.cols, cap = h->cap;
  DVS_ARG(image && depth_u16 && (channels == 1 || channels == 3) && step >= (size_t)cols * channels && depth_step >= (size_t)cols * 2);
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  int* cnt = (int*)h->d_rec.get();
  const int* rec = (const int*)h->h_rec.get();
  const int p = h->p, q = 1 - p;
  const int64_t t = h->t;
  out->frame_index = t;
  h->last_n = 0;   // until this frame's culled set is complete: a call that fails half-way leaves no set to read back (reset the handle after an error)
  // ---- frontend.cpp:1084: BGR -> gray; :1094 / :1285 extract; :1100 / :1291 filterDepth
  const uint8_t* d_gray = h->d_img.get();
  const size_t irow = (size_t)cols * channels, drow = (size_t)cols * 2;
  if (step == irow) memcpy(h->h_img.get(), image, irow * rows);
  else for (int r = 0; r < rows; r++) memcpy(h->h_img.get() + r * irow, image + r * step, irow);
  if (depth_step == drow) memcpy(h->d_depth[p].get(), depth_u16, drow * rows);
  else for (int r = 0; r < rows; r++) memcpy((uint8_t*)h->d_depth[p].get() + r * drow, (const uint8_t*)depth_u16 + r * depth_step, drow);
  DVS_HIP(hipMemcpyAsync(h->d_img.get(), h->h_img.get(), irow * rows, hipMemcpyHostToDevice, st));
  if (channels == 3) {
    DVS_TRY(dvs_bgr_to_gray_device(h->ctx, h->d_img.get(), 1, rows, cols, (size_t)cols * 3, 0, h->d_gray.get(), cols, 0, P.gray_variant));
    d_gray = h->d_gray.get();
  }
  const uint8_t* d_keep = nullptr;   // the motion mask of this frame (opt-in; NULL: the unmasked extraction, as ever)
  if (h->mo) {
    const int ns = h->mo_lag + 1;
    const size_t px = (size_t)rows * cols;
    uint16_t* d_cur = h->mo_ring.get() + (size_t)(t % ns) * px;
    DVS_HIP(hipMemcpyAsync(d_cur, h->d_depth[p].get(), px * 2, hipMemcpyHostToDevice, st));
    h->mo_ref = -1;
    if (h->prev_valid && !h->mo_after_reset && h->mo_seq >= 1) {
      const int64_t ref = t - std::min(h->mo_lag, h->mo_seq);
      const dvs_tracker::MotionSlot& rs = h->mo_slot[ref % ns];
      if (rs.frame == ref) {
        motion_relative_pose(h, t, rs, h->mo_R, h->mo_t);
        DVS_TRY(dvs_motion_segment_device(h->mo, h->mo_ring.get() + (size_t)(ref % ns) * px, (size_t)cols * 2, d_cur, (size_t)cols * 2, h->mo_R, h->mo_t,
                                          h->mo_mask.get(), cols, nullptr));
        h->mo_ref = ref;
        d_keep = h->mo_mask.get();
      }
    }
  }
  if (d_keep) DVS_TRY(dvs_orb_extract_batch_device_masked(h->orb, d_gray, 1, rows, cols, cols, (size_t)rows * cols, d_keep, cols, 0, (dvs_keypoint*)h->d_kraw.get(),
                                                          h->d_draw.get(), cap, cnt + C_EXT));
  else DVS_TRY(dvs_orb_extract_batch_device(h->orb, d_gray, 1, rows, cols, cols, (size_t)rows * cols, (dvs_keypoint*)h->d_kraw.get(), h->d_draw.get(), cap, cnt + C_EXT));
  DVS_TRY(dvs_filter_depth_batch_device(h->ctx, (const dvs_keypoint*)h->d_kraw.get(), h->d_draw.get(), cnt + C_EXT, cap, 1, h->d_depth[p].get(), rows, cols,
                                        (size_t)cols * 2, 0, P.min_depth, P.max_depth, h->f_k[p].get(), h->f_d[p].get(), nullptr, cnt + C_F0 + p));
  const bool tracking = h->prev_valid && h->prev_n > 0;
  if (tracking) {   // :1123 match, :1126-1132 distance filter (enqueued before the counts are known: an empty frame gives no matches)
    DVS_TRY(dvs_match_hamming_batch_device(h->ctx, h->f_d[p].get(), cnt + C_F0 + p, cap, h->f_d[q].get(), cnt + C_F0 + q, cap, 1, h->d_idx.get(), h->d_dist.get()));
    hipLaunchKernelGGL(k_compact_matches, dim3(1), dim3(256), 0, st, h->d_idx.get(), h->d_dist.get(), cnt + C_F0 + p, cnt + C_F0 + q, h->f_k[p].get(),
                       h->f_k[q].get(), cap, P.max_hamming, h->c_q.get(), h->c_t.get(), h->c_p1.get(), h->c_p2.get(), cnt + C_MATCH);
  }
  DVS_TRY(tracker_export(h));
  const int n_ext = rec[C_EXT], n_f = rec[C_F0 + p];
  out->n_extracted = n_ext; out->n_filtered = n_f;
  for (int k = 0; k < 9; k++) out->R[k] = h->R[k];
  for (int k = 0; k < 3; k++) out->t[k] = h->tt[k];
  auto advance = [&]() {   // :1258-1259, 1274-1275 / :1299-1312
    if (h->mo) {           // this frame's pose beside its depth image in the ring; a first frame and a tracking reset begin a sequence
      dvs_tracker::MotionSlot& s = h->mo_slot[t % (h->mo_lag + 1)];
      s.frame = t; s.pose_updated = out->pose_updated != 0;
      memcpy(s.R, h->R, sizeof(s.R)); memcpy(s.t, h->tt, sizeof(s.t));
      const bool begins = out->first_frame || out->tracking_reset;
      h->mo_seq = begins ? 1 : std::min(h->mo_seq + 1, h->mo_lag + 1);
      h->mo_after_reset = out->tracking_reset != 0;
    }
    h->p = q; h->prev_n = n_f; h->prev_valid = true; h->t = t + 1;
  };
  const int bw = 1 - h->bkf;                       // where this frame's backend set goes (the last keyframe's stays)
  int n_backend = 0;
  bool publish = false;
  if (!h->prev_valid) {
    // ---- :1278-1312 first frame: all depth-filtered features are the initial keyframe
    out->first_frame = 1;
    if (n_f > 0) {
      DVS_HIP(hipMemcpyAsync(h->b_k[bw].get(), h->f_k[p].get(), (size_t)n_f * sizeof(dvs_keypoint), hipMemcpyDeviceToDevice, st));
      DVS_HIP(hipMemcpyAsync(h->b_d[bw].get(), h->f_d[p].get(), (size_t)n_f * 32, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_iota, dim3((n_f + 255) / 256), dim3(256), 0, st, h->b_sel.get(), n_f);
    }
    DVS_HIP(hipMemcpyAsync(cnt + C_B0 + bw, cnt + C_F0 + p, 4, hipMemcpyDeviceToDevice, st));
    n_backend = n_f;
    publish = true; out->kf_criterion = DVS_KF_FIRST_FRAME;
  } else if (n_f == 0 || h->prev_n == 0) {
    // ---- :1107-1117 reset: the state is replaced, no pose change, no keyframe
    out->tracking_reset = 1;
    h->last_n = 0;
    advance();
    return DVS_OK;
  } else {
    const int n_match = rec[C_MATCH];
    out->n_matches = n_match;
    // ---- :1136-1166 fundamental-matrix gate from 8 matches on, else the distance-filtered set
    const int *gq = h->c_q.get(), *gt = h->c_t.get(), *d_ng = cnt + C_MATCH;
    const float *gp1 = h->c_p1.get(), *gp2 = h->c_p2.get();
    if (n_match >= 8) {
      DVS_TRY(tracker_fm(h, h->c_p1.get(), h->c_p2.get(), cnt + C_MATCH, n_match, P.seed_base + 2ull * (unsigned long long)t, h->d_mask.get()));
      hipLaunchKernelGGL(k_compact_mask, dim3(1), dim3(256), 0, st, h->d_mask.get(), cnt + C_MATCH, cap, h->c_q.get(), h->c_t.get(), h->c_p1.get(), h->c_p2.get(),
                         h->g_q.get(), h->g_t.get(), h->g_p1.get(), h->g_p2.get(), cnt + C_GEO);
      gq = h->g_q.get(); gt = h->g_t.get(); gp1 = h->g_p1.get(); gp2 = h->g_p2.get(); d_ng = cnt + C_GEO;
    } else {
      out->fm_skipped = 1;
    }
    (void)gt;
    // ---- :1171-1219 feature culling
    hipLaunchKernelGGL(k_cull, dim3(1), dim3(256), 0, st, h->f_k[p].get(), h->f_d[p].get(), cnt + C_F0 + p, gq, d_ng, cap, P.cull_max_new, P.cull_min_response,
                       h->b_k[bw].get(), h->b_d[bw].get(), h->b_sel.get(), cnt + C_B0 + bw, (int*)nullptr);
    // ---- :859-892 the 3D-2D correspondences of estimateCameraPose, from prev_frame_depth_
    hipLaunchKernelGGL(k_pnp_points, dim3(1), dim3(256), 0, st, gp1, gp2, d_ng, cap, h->d_depth[q].get(), rows, cols, (float)P.fx, (float)P.fy, (float)P.cx,
                       (float)P.cy, P.min_depth, P.max_depth, h->o_obj.get(), h->o_img.get(), cnt + C_PNP);
    // ---- :611-623 isKeyframe's match against the last keyframe (it depends on the culled set alone)
    const bool kf_match = h->has_last_kf && h->kf_n > 0;
    if (kf_match) {
      DVS_TRY(dvs_match_hamming_batch_device(h->ctx, h->b_d[bw].get(), cnt + C_B0 + bw, cap, h->b_d[h->bkf].get(), cnt + C_B0 + h->bkf, cap, 1, h->d_idx.get(),
                                             h->d_dist.get()));
      hipLaunchKernelGGL(k_compact_matches, dim3(1), dim3(256), 0, st, h->d_idx.get(), h->d_dist.get(), cnt + C_B0 + bw, cnt + C_B0 + h->bkf, h->b_k[bw].get(),
                         h->b_k[h->bkf].get(), cap, P.max_hamming, h->k_q.get(), h->k_t.get(), h->k_p1.get(), h->k_p2.get(), cnt + C_KFMATCH);
    }
    DVS_TRY(tracker_export(h));
    const int n_geo = n_match >= 8 ? rec[C_GEO] : n_match;
    const int n_pnp = rec[C_PNP];
    n_backend = rec[C_B0 + bw];
    out->n_geometric = n_geo;
    const bool kf_run = kf_match && n_backend > 0;      // :611
    const int n_kfm = kf_run ? rec[C_KFMATCH] : 0;
    // ---- :1237 / :899 PnP wants >= 5 matches and >= 6 points; :627 the keyframe gate >= 8 matches
    const bool do_pnp = n_geo >= 5 && n_pnp >= 6;
    if (n_geo >= 5) out->n_pnp_points = n_pnp;
    if (!do_pnp) out->pnp_skipped = 1;
    const double K4[4] = {P.fx, P.fy, P.cx, P.cy};
    unsigned char* d_pnp = (unsigned char*)h->d_rec.get() + kRecPnp;
    int* d_sel = (int*)((unsigned char*)h->d_rec.get() + kRecSel);
    if (do_pnp) {
      if (P.pnp_mode == 1) DVS_TRY(pnp_cv_device(h->ctx, h->o_obj.get(), h->o_img.get(), n_pnp, K4, P.pnp_iterations, P.pnp_reproj_err, P.pnp_confidence, h->d_inl.get(), d_pnp, d_sel));
      else DVS_TRY(pnp_own_device(h->ctx, h->o_obj.get(), h->o_img.get(), cnt + C_PNP, P.seed_base + 2ull * (unsigned long long)t + 1ull, K4, P.pnp_iterations,
                                  P.pnp_reproj_err, P.pnp_confidence, h->d_inl.get(), d_pnp));
    }
    const bool kf_gate = kf_run && n_kfm >= 8;
    if (kf_gate) {
      DVS_TRY(tracker_fm(h, h->k_p1.get(), h->k_p2.get(), cnt + C_KFMATCH, n_kfm, P.seed_base + 2ull * (unsigned long long)t + 1000003ull, h->d_mask.get()));
      hipLaunchKernelGGL(k_compact_mask, dim3(1), dim3(256), 0, st, h->d_mask.get(), cnt + C_KFMATCH, cap, (const int*)nullptr, (const int*)nullptr,
                         (const float*)nullptr, (const float*)nullptr, (int*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr, cnt + C_KFGEO);
    }
    if (do_pnp || kf_gate) DVS_TRY(tracker_export(h));
    // ---- :925-948 inverse motion, isMotionOutlier (:549-570), pose products, all in double
    if (do_pnp) {
      const unsigned char* r = h->h_rec.get() + kRecPnp;
      int nin = 0, succ = 0;
      memcpy(&nin, r, 4); memcpy(&succ, r + 4, 4);
      const bool have = P.pnp_mode == 1 ? ((const int*)(h->h_rec.get() + kRecSel))[0] >= 0 : succ != 0;
      if (have) { memcpy(out->rvec, r + 16, 24); memcpy(out->tvec, r + 40, 24); }
      if (!succ) {
        out->pnp_failed = 1;
      } else {
        out->n_pnp_inliers = nin;
        double Rr[9], Ri[9], ti[3];
        rodrigues(out->rvec, Rr);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ri[3 * i + j] = Rr[3 * j + i];                                     // :937
        for (int i = 0; i < 3; i++) ti[i] = -((Ri[3 * i] * out->tvec[0] + Ri[3 * i + 1] * out->tvec[1]) + Ri[3 * i + 2] * out->tvec[2]);   // :938
        const double tn = sqrt((ti[0] * ti[0] + ti[1] * ti[1]) + ti[2] * ti[2]);
        const double ca = (((Ri[0] + Ri[4]) + Ri[8]) - 1.0) / 2.0, ang = acos(ca < -1.0 ? -1.0 : (ca > 1.0 ? 1.0 : ca));
        if (tn > P.max_translation || ang > P.max_rotation) {
          out->motion_outlier = 1;
        } else {
          double Rn[9], tn3[3];
          for (int i = 0; i < 3; i++) tn3[i] = h->tt[i] + ((h->R[3 * i] * ti[0] + h->R[3 * i + 1] * ti[1]) + h->R[3 * i + 2] * ti[2]);   // :947
          for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rn[3 * i + j] = (h->R[3 * i] * Ri[j] + h->R[3 * i + 1] * Ri[3 + j]) + h->R[3 * i + 2] * Ri[6 + j];   // :948
          memcpy(h->R, Rn, sizeof(Rn)); memcpy(h->tt, tn3, sizeof(tn3));
          out->pose_updated = 1;
        }
      }
    }
    for (int k = 0; k < 9; k++) out->R[k] = h->R[k];
    for (int k = 0; k < 3; k++) out->t[k] = h->tt[k];
    // ---- :601-662 isKeyframe
    if (!h->has_last_kf) {
      h->has_last_kf = true;                            // :603-606 (the first frame publishes without asking isKeyframe)
      publish = true; out->kf_criterion = DVS_KF_NO_REFERENCE;
    } else {
      bool crit = false;
      if (kf_run) {
        const int n_kfg = kf_gate ? rec[C_KFGEO] : n_kfm;
        out->n_kf_matches = n_kfm; out->n_kf_geometric = n_kfg;
        crit = n_kfg < P.kf_min_matches;                // :651
      }
      if (crit || h->since_kf > P.kf_max_frames) {      // :655-657
        out->kf_criterion = (crit ? DVS_KF_FEW_MATCHES : 0) | (h->since_kf > P.kf_max_frames ? DVS_KF_MAX_FRAMES : 0);
        h->since_kf = 0; publish = true;
      } else {
        h->since_kf++;                                  // :660
      }
    }
  }
  out->n_backend = n_backend;
  h->blast = bw; h->last_n = n_backend;
  // ---- :699-790 publishKeyframe: pose -> quaternion, CDR payload on the device, last keyframe := this frame's backend set
  dvs_status ret = DVS_OK;
  if (publish) {
    out->is_keyframe = 1;
    out->keyframe_id = h->keyframe_id;
    if (cdr_out) {
      const double* R = h->R;
      dvs_keyframe_header hdr;
      memset(&hdr, 0, sizeof(hdr));
      hdr.stamp_sec = stamp_sec; hdr.stamp_nanosec = stamp_nanosec; hdr.frame_id = "camera_link"; hdr.keyframe_id = (uint64_t)h->keyframe_id;
      const double tr1 = ((1.0 + R[0]) + R[4]) + R[8];
      const double w = sqrt(tr1 > 0.0 ? tr1 : 0.0) / 2.0;
      hdr.rotation_xyzw[0] = (R[7] - R[5]) / (4 * w); hdr.rotation_xyzw[1] = (R[2] - R[6]) / (4 * w); hdr.rotation_xyzw[2] = (R[3] - R[1]) / (4 * w);
      hdr.rotation_xyzw[3] = w;
      for (int k = 0; k < 3; k++) hdr.translation[k] = h->tt[k];
      uint64_t* d_size = (uint64_t*)((unsigned char*)h->d_rec.get() + kRecCdr);
      DVS_TRY(dvs_publish_keyframe_device(h->ctx, &hdr, h->b_k[bw].get(), h->b_d[bw].get(), n_backend, h->d_depth[p].get(), rows, cols, (size_t)cols * 2,
                                          (float)P.fx, (float)P.fy, (float)P.cx, (float)P.cy, h->R, h->tt, h->d_cdr.get(), h->cdr_cap_dev, d_size, cnt + C_CDRN));
      DVS_TRY(tracker_export(h));
      uint64_t sz = 0;
      memcpy(&sz, h->h_rec.get() + kRecCdr, 8);
      out->cdr_bytes = sz; out->cdr_landmarks = rec[C_CDRN];
      if (sz > cdr_cap) {
        set_error("keyframe payload needs %llu bytes, cdr_out has %zu", (unsigned long long)sz, cdr_cap);
        ret = DVS_ERR_CAPACITY;
      } else {
        DVS_HIP(hipMemcpyAsync(cdr_out, h->d_cdr.get(), (size_t)sz, hipMemcpyDeviceToHost, st));
        DVS_HIP(hipStreamSynchronize(st));
      }
    }
    h->keyframe_id++;                                   // :729
    h->bkf = bw; h->kf_n = n_backend;                   // :779-780
  }
  advance();
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
  if (kps) DVS_HIP(hipMemcpyAsync(kps, h->b_k[h->blast].get(), m * sizeof(dvs_keypoint), hipMemcpyDeviceToHost, st));
  if (desc) DVS_HIP(hipMemcpyAsync(desc, h->b_d[h->blast].get(), m * 32, hipMemcpyDeviceToHost, st));
  if (sel_index) DVS_HIP(hipMemcpyAsync(sel_index, h->b_sel.get(), m * 4, hipMemcpyDeviceToHost, st));
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
  if (h->mo) { dvs_motion_destroy(h->mo); h->mo = nullptr; }
  h->mo_ring = DeviceBuf<uint16_t>(); h->mo_mask = DeviceBuf<uint8_t>();
  h->mo_lag = 0;
  motion_reset_state(h);
  if (!p) return DVS_OK;
  const size_t px = (size_t)h->P.rows * h->P.cols;
  dvs_status s = dvs_motion_create(&mp, h->device, &h->mo);
  if (s == DVS_OK) s = dvs_motion_set_stream(h->mo, h->ctx->stream);
  if (s == DVS_OK) s = h->mo_ring.alloc(px * (size_t)(lag + 1));
  if (s == DVS_OK) s = h->mo_mask.alloc(px);
  if (s != DVS_OK) {
    if (h->mo) { dvs_motion_destroy(h->mo); h->mo = nullptr; }
    h->mo_ring = DeviceBuf<uint16_t>(); h->mo_mask = DeviceBuf<uint8_t>();
    return s;
  }
  h->mo_lag = lag;
  return DVS_OK;
}

dvs_status dvs_tracker_get_motion_mask(dvs_tracker* h, uint8_t* mask, size_t step, double* R9, double* t3, int64_t* ref_frame_index, dvs_motion_stats* stats) {
  DVS_ARG(h && (!mask || step >= (size_t)h->P.cols));
  const bool used = h->mo && h->mo_ref >= 0;
  if (ref_frame_index) *ref_frame_index = used ? h->mo_ref : -1;
  for (int k = 0; k < 9; k++) if (R9) R9[k] = used ? h->mo_R[k] : (k % 4 == 0 ? 1.0 : 0.0);
  for (int k = 0; k < 3; k++) if (t3) t3[k] = used ? h->mo_t[k] : 0.0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!used) {
    if (mask) for (int r = 0; r < h->P.rows; r++) memset(mask + (size_t)r * step, 255, (size_t)h->P.cols);
    return DVS_OK;
  }
  DVS_HIP(hipSetDevice(h->device));
  if (stats) DVS_TRY(motion_last_stats(h->mo, stats));
  if (mask) {
    DVS_HIP(hipMemcpy2DAsync(mask, step, h->mo_mask.get(), (size_t)h->P.cols, (size_t)h->P.cols, (size_t)h->P.rows, hipMemcpyDeviceToHost, h->ctx->stream));
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
  if (kps) DVS_HIP(hipMemcpyAsync(kps, h->f_k[q].get(), (size_t)m * sizeof(dvs_keypoint), hipMemcpyDeviceToHost, st));
  if (desc) DVS_HIP(hipMemcpyAsync(desc, h->f_d[q].get(), (size_t)m * 32, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  return DVS_OK;
}

// include/dvslam_hip.h "Tracking against the map": that set against the backend's landmark table, prior R_, t_; the tracker itself
// launches nothing here
dvs_status dvs_tracker_track_map(dvs_tracker* h, dvs_backend* backend, dvs_maptrack* mt, int32_t apply, dvs_maptrack_result* result) {
  DVS_ARG(h && backend && mt && result && backend->device == h->device);
  if (!h->prev_valid) { set_error("dvs_tracker_track_map: no frame has been tracked"); return DVS_ERR_EMPTY; }
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  const int q = 1 - h->p;
  DVS_TRY(dvs_backend_track_frame(backend, mt, h->f_k[q].get(), h->f_d[q].get(), h->prev_n, h->R, h->tt, result));
  if (apply && result->status == DVS_MAPTRACK_OK) { memcpy(h->R, result->R, sizeof(h->R)); memcpy(h->tt, result->t, sizeof(h->tt)); }
  return DVS_OK;
}

// include/dvslam_hip.h "Landmark refresh": the same through the gated call
dvs_status dvs_tracker_track_map_gated(dvs_tracker* h, dvs_backend* backend, dvs_maptrack* mt, const dvs_maptrack_gates* gates, int32_t apply,
                                       dvs_maptrack_result* result) {
  DVS_ARG(h && backend && mt && result && backend->device == h->device);
  if (!h->prev_valid) { set_error("dvs_tracker_track_map_gated: no frame has been tracked"); return DVS_ERR_EMPTY; }
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  const int q = 1 - h->p;
  DVS_TRY(dvs_backend_track_frame_gated(backend, mt, gates, h->f_k[q].get(), h->f_d[q].get(), h->prev_n, h->R, h->tt, result));
  if (apply && result->status == DVS_MAPTRACK_OK) { memcpy(h->R, result->R, sizeof(h->R)); memcpy(h->tt, result->t, sizeof(h->tt)); }
  return DVS_OK;
}

// include/dvslam_hip.h "Relocalisation": that set against the backend's landmark table with no prior; the tracker itself launches nothing here.
// After a frame with tracking_reset the set may be empty: FEW_PAIRS, not an error
dvs_status dvs_tracker_relocalize(dvs_tracker* h, dvs_backend* backend, dvs_reloc* reloc, dvs_maptrack* mt, int32_t apply, dvs_reloc_result* result) {
  DVS_ARG(h && backend && reloc && mt && result && backend->device == h->device);
  if (!h->prev_valid) { set_error("dvs_tracker_relocalize: no frame has been tracked"); return DVS_ERR_EMPTY; }
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  const int q = 1 - h->p;
  DVS_TRY(dvs_backend_relocalize_frame(backend, reloc, mt, h->f_k[q].get(), h->f_d[q].get(), h->prev_n, result));
  if (apply && result->status == DVS_RELOC_OK) { memcpy(h->R, result->R, sizeof(h->R)); memcpy(h->tt, result->t, sizeof(h->tt)); }
  return DVS_OK;
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test.h)
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
  DeviceBuf<dvs_keypoint> d_k, d_bk; DeviceBuf<uint8_t> d_d, d_bd; DeviceBuf<int> d_q, d_sel, d_head;
  DVS_TRY(d_k.upload(k)); DVS_TRY(d_q.upload(q)); DVS_TRY(d_head.upload(head));
  DVS_TRY(d_bk.alloc(n)); DVS_TRY(d_d.alloc((size_t)n * 32)); DVS_TRY(d_bd.alloc((size_t)n * 32)); DVS_TRY(d_sel.alloc(n));
  DVS_HIP(hipMemset(d_d.get(), 0, (size_t)n * 32));
  hipLaunchKernelGGL(k_cull, dim3(1), dim3(256), 0, (hipStream_t) nullptr, d_k.get(), d_d.get(), d_head.get(), d_q.get(), d_head.get() + 1, n, max_new, min_response,
                     d_bk.get(), d_bd.get(), d_sel.get(), d_head.get() + 2, d_head.get() + 3);
  DVS_HIP(hipGetLastError());
  std::vector<int> sel((size_t)n);
  DVS_HIP(hipMemcpy(head.data(), d_head.get(), 16, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(sel.data(), d_sel.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
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
