// reloc.hip — relocalisation (include/dvslam_hip.h "Relocalisation", dvs_reloc_*): a frame's pose in the map with no prior.  Every landmark of
// the table searches ALL keypoints of the frame, the keypoints keep one landmark each, P3P RANSAC finds a pose on the kept pairs and the
// tracking against the map (map_track.hip) confirms it.  The rule is stated in the header and restated in numpy in tests/reloc_ref.py; this
// file is its device form:
//   k_rl_begin     a keypoint per lane: its proposal key cleared; the two row counts the matcher reads, the counters cleared
//   k_match_fp4    (match.hip, launch_match_fp4 with k = 2) the landmarks as query rows, the keypoints as train rows: per landmark the
//                  two nearest keypoints in (d, k) order on the matrix cores — ONE job of n_lm x n_kp
//   k_rl_propose   a landmark per lane: finite position, distance and ratio tests in integers, the proposal as ONE 64-bit atomicMin on
//                  (d << 40 | landmark row) at the best keypoint
//   k_rl_list      ONE workgroup: the kept pairs in ascending keypoint index by block_ops.h's ordered compaction — obj, img, rows,
//                  keypoints, distances — and the count RANSAC reads (0 below min_pairs: nothing is solved)
//   pnp_own_device (ransac.hip) dvs_solve_pnp_ransac's launches on the list where it lies
//   k_rl_record    the counts and the 64-byte PnP record as one 96-byte record, exported through the context's pinned block
// Then the host: Rodrigues in FP64, and dvs_maptrack_track_device on the caller's handle with that pose as the prior.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "block_ops.h"
#include "io_pinned.h"
#include "matcher.h"
#include "ransac_device.h"
#include "backend_internal.h"
#include "maptrack_internal.h"
#include "pose_host.h"

namespace dvs {

enum { RC_NLM = 0, RC_NKP = 1, RC_PROPOSED = 2, RC_PAIRS = 3, RC_NPNP = 4, RC_INTS = 8 };
constexpr unsigned long long kRlNoKey = ~0ull;
constexpr unsigned long long kRlRowMask = (1ull << 40) - 1ull;
struct RlRec { int n_proposed, n_pairs, r0, r1, r2, r3, r4, r5; PnpRecord pnp; };   // what crosses to the host: 96 bytes
static_assert(sizeof(RlRec) == 96 && offsetof(RlRec, pnp) == 32, "record layout");

__global__ __launch_bounds__(256) void k_rl_begin(int n_lm, int n_kp, unsigned long long* __restrict__ key, int* __restrict__ counters) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n_kp) key[k] = kRlNoKey;
  if (k < RC_INTS) counters[k] = k == RC_NLM ? n_lm : (k == RC_NKP ? n_kp : 0);
}

// state[j]: -1 the position is not finite, 0 no proposal, 1 proposed.  top_idx / top_dist: [n_lm][2] as k_match_fp4 left them (unused slot -1 / INT_MAX)
__global__ __launch_bounds__(256) void k_rl_propose(int n_lm, const float* __restrict__ xyz, const int* __restrict__ top_idx, const int* __restrict__ top_dist,
                                                    int max_hamming, int ratio_pct, signed char* __restrict__ state, unsigned long long* __restrict__ key,
                                                    int* __restrict__ counters) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_lm) return;
  const float x = xyz[3 * (size_t)j], y = xyz[3 * (size_t)j + 1], z = xyz[3 * (size_t)j + 2];
  const bool finite = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // (NaN compares false)
  const int best = top_idx[2 * (size_t)j], d_best = top_dist[2 * (size_t)j];
  const int d_second = top_idx[2 * (size_t)j + 1] >= 0 ? top_dist[2 * (size_t)j + 1] : -1;
  bool prop = false;
  if (finite && best >= 0) {
    const bool ratio_ok = d_second < 0 || ratio_pct <= 0 || (long long)d_best * 100 < (long long)ratio_pct * d_second;
    prop = d_best < max_hamming && ratio_ok;
  }
  state[j] = finite ? (prop ? 1 : 0) : -1;
  if (prop) {
    atomicMin(&key[best], ((unsigned long long)d_best << 40) | (unsigned long long)j);
    atomicAdd(&counters[RC_PROPOSED], 1);   // (the compiler makes it one add per wavefront)
  }
}

__global__ __launch_bounds__(256) void k_rl_list(int n_kp, const unsigned long long* __restrict__ key, const float* __restrict__ xyz,
                                                 const dvs_keypoint* __restrict__ kps, int min_pairs, float* __restrict__ obj, float* __restrict__ img,
                                                 int* __restrict__ p_lm, int* __restrict__ p_kp, int* __restrict__ p_dist, int* __restrict__ counters) {
  __shared__ int s_w[4];
  int m = 0;
  for (int k0 = 0; k0 < n_kp; k0 += 256) {
    const int k = k0 + (int)threadIdx.x;
    const unsigned long long q = k < n_kp ? key[k] : kRlNoKey;
    const bool have = q != kRlNoKey;
    int total;
    const int pos = m + block_rank256(have, s_w, total);
    if (have) {
      const int row = (int)(q & kRlRowMask);
      for (int a = 0; a < 3; a++) obj[3 * (size_t)pos + a] = xyz[3 * (size_t)row + a];
      img[2 * (size_t)pos] = kps[k].x; img[2 * (size_t)pos + 1] = kps[k].y;
      p_lm[pos] = row; p_kp[pos] = k; p_dist[pos] = (int)(q >> 40);
    }
    m += total;
  }
  if (threadIdx.x == 0) { counters[RC_PAIRS] = m; counters[RC_NPNP] = m >= min_pairs ? m : 0; }
}

__global__ void k_rl_record(const int* __restrict__ counters, const PnpRecord* __restrict__ pnp, RlRec* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  RlRec r;
  memset(&r, 0, sizeof(r));
  r.n_proposed = counters[RC_PROPOSED]; r.n_pairs = counters[RC_PAIRS];
  if (counters[RC_NPNP] > 0) {   // every field the estimator writes (`unused` stays zero)
    r.pnp.n_inliers = pnp->n_inliers; r.pnp.success = pnp->success;
    for (int k = 0; k < 3; k++) { r.pnp.rvec[k] = pnp->rvec[k]; r.pnp.tvec[k] = pnp->tvec[k]; }
  }
  *out = r;
}

static dvs_status reloc_check_params(const dvs_reloc_params& P) {
  for (int k = 0; k < 4; k++) DVS_ARG(__builtin_isfinite(P.K4[k]));
  DVS_ARG(P.K4[0] > 0 && P.K4[1] > 0);
  DVS_ARG(P.max_hamming >= 0 && P.max_hamming <= 257 && P.ratio_pct <= 100000);
  DVS_ARG(P.min_pairs >= 4);
  DVS_ARG(P.pnp_iterations >= 1 && P.pnp_iterations <= 1024);
  DVS_ARG(__builtin_isfinite(P.pnp_reproj_err) && P.pnp_reproj_err > 0);
  DVS_ARG(P.pnp_confidence > 0 && P.pnp_confidence < 1);
  DVS_ARG(P.min_pnp_inliers >= 0 && P.min_confirmed >= 0);
  return DVS_OK;
}

}  // namespace dvs

using namespace dvs;

struct dvs_reloc {
  dvs_reloc_params P;
  int device = 0;
  dvs_matcher* ctx = nullptr;      // the stream, RANSAC's scratch and the pinned block; works on the legacy default stream until set_stream
  DeviceBuf<int> counters;         // RC_INTS
  // per landmark (grow-only): the two nearest keypoints and the state
  Column<int, 2> top_idx, top_dist; Column<signed char> state;
  size_t c_lm = 0;
  // per keypoint (grow-only): the proposal keys and the list
  Column<unsigned long long> key; Column<float, 3> obj; Column<float, 2> img; Column<int> p_lm, p_kp, p_dist, p_inl;
  size_t c_kp = 0;
  DeviceBuf<PnpRecord> pnp;
  DeviceBuf<RlRec> d_rec;
  FrameStaging stage;              // of the host form
  // stage events, created by dvs_reloc_set_timing alone
  Event ev[4];
  bool timing = false, timed = false;
  // the last call
  int last_n_lm = 0, last_n_kp = 0, last_pairs = 0, last_inliers = 0;
  PnpRecord last_pnp = {};         // stage 4's record as it came back (zeros when nothing was solved)
};

static dvs_status rl_grow_kp(dvs_reloc* h, size_t n) { return grow_rows(h->c_kp, n, n + n / 4, h->key, h->obj, h->img, h->p_lm, h->p_kp, h->p_dist, h->p_inl); }
static dvs_status rl_grow_lm(dvs_reloc* h, size_t n) { return grow_rows(h->c_lm, n, n + n / 4, h->top_idx, h->top_dist, h->state); }

static dvs_status rl_check_args(const dvs_reloc* h, const dvs_maptrack* mt, const void* xyz, const void* ldesc, int n_lm, const void* kps, const void* kdesc,
                                int n_kp, const void* result) {
  DVS_ARG(h && mt && result && n_lm >= 0 && n_kp >= 0 && n_lm <= (1 << 30) - 1 && n_kp <= (1 << 30));   // n_lm * 2 and n_kp below 2^31
  DVS_ARG(maptrack_device(mt) == h->device);
  DVS_ARG(n_lm == 0 || (xyz && ldesc));
  DVS_ARG(n_kp == 0 || (kps && kdesc));
  DVS_ARG(((uintptr_t)ldesc & 15) == 0 && ((uintptr_t)kdesc & 15) == 0 && ((uintptr_t)xyz & 3) == 0 && ((uintptr_t)kps & 3) == 0);   // k_match_fp4 reads 16 bytes at a time
  return DVS_OK;
}

extern "C" {

void dvs_reloc_default_params(dvs_reloc_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_hamming = 50; p->ratio_pct = 75; p->min_pairs = 20;
  p->pnp_iterations = 512; p->pnp_reproj_err = 4.0; p->pnp_confidence = 0.99;
  p->min_pnp_inliers = 15; p->min_confirmed = 30; p->seed = 0;
}

dvs_status dvs_reloc_create(const dvs_reloc_params* params, int32_t device, dvs_reloc** out) {
  DVS_ARG(params && out);
  *out = nullptr;
  DVS_TRY(reloc_check_params(*params));
  DVS_TRY(check_device(device));
  dvs_reloc* h = new (std::nothrow) dvs_reloc();
  if (!h) { set_error("dvs_reloc_create: out of memory"); return DVS_ERR_HIP; }
  h->P = *params; h->device = device;
  auto alloc_all = [&]() -> dvs_status {
    DVS_TRY(dvs_matcher_create_on_stream(device, nullptr, &h->ctx));
    DVS_TRY(h->counters.alloc(RC_INTS)); DVS_TRY(h->pnp.alloc(1)); DVS_TRY(h->d_rec.alloc(1));
    DVS_HIP(hipMemset(h->counters.get(), 0, RC_INTS * sizeof(int)));
    DVS_HIP(hipMemset(h->pnp.get(), 0, sizeof(PnpRecord)));
    DVS_HIP(hipMemset(h->d_rec.get(), 0, sizeof(RlRec)));
    return DVS_OK;
  };
  const dvs_status s = alloc_all();
  if (s != DVS_OK) { dvs_reloc_destroy(h); return s; }
  *out = h;
  return DVS_OK;
}

void dvs_reloc_destroy(dvs_reloc* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->ctx) (void)hipStreamSynchronize(h->ctx->stream);
  dvs_matcher_destroy(h->ctx);
  delete h;
}

dvs_status dvs_reloc_set_stream(dvs_reloc* h, void* hip_stream) {
  DVS_ARG(h);
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  h->timed = false;
  return dvs_matcher_set_stream(h->ctx, hip_stream);
}

dvs_status dvs_reloc_set_timing(dvs_reloc* h, int32_t on) {
  DVS_ARG(h);
  DVS_HIP(hipSetDevice(h->device));
  if (on) for (Event& e : h->ev) if (!(hipEvent_t)e) DVS_HIP(e.create(true));
  h->timing = on != 0; h->timed = false;
  return DVS_OK;
}

dvs_status dvs_reloc_get_stage_ms(dvs_reloc* h, double* ms3) {
  DVS_ARG(h && ms3);
  if (!h->timing || !h->timed) { set_error("dvs_reloc_get_stage_ms: no timed call"); return DVS_ERR_EMPTY; }
  DVS_HIP(hipSetDevice(h->device));
  for (int k = 0; k < 3; k++) {
    float v = 0.f;
    DVS_HIP(hipEventElapsedTime(&v, h->ev[k], h->ev[k + 1]));
    ms3[k] = (double)v;
  }
  return DVS_OK;
}

dvs_status dvs_reloc_locate_device(dvs_reloc* h, dvs_maptrack* mt, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                   const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, dvs_reloc_result* result) {
  DVS_TRY(rl_check_args(h, mt, d_lm_xyz, d_lm_desc, n_lm, d_kps, d_desc, n_kp, result));
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  const dvs_reloc_params& P = h->P;
  h->last_n_lm = 0; h->last_n_kp = 0; h->last_pairs = 0; h->last_inliers = 0; h->timed = false;
  if ((size_t)n_kp > h->c_kp || (size_t)n_lm > h->c_lm) DVS_HIP(hipStreamSynchronize(st));   // nothing in flight reads what is freed
  DVS_TRY(rl_grow_kp(h, (size_t)(n_kp > 0 ? n_kp : 1)));   // (RANSAC's entry wants its arrays even for an empty list)
  DVS_TRY(rl_grow_lm(h, (size_t)n_lm));
  int* cnt = h->counters.get();
  const unsigned gk = (unsigned)((n_kp + 255) / 256), gl = (unsigned)((n_lm + 255) / 256);
  if (h->timing) DVS_HIP(hipEventRecord(h->ev[0], st));
  // ---- stage 1
  hipLaunchKernelGGL(k_rl_begin, dim3(gk > 0 ? gk : 1), dim3(256), 0, st, n_lm, n_kp, h->key.get(), cnt);
  if (n_lm > 0 && n_kp > 0) {   // (k_match_fp4 prefetches train rows by a clamped index: it wants at least one)
    launch_match_fp4(st, 2, 1, d_lm_desc, cnt + RC_NLM, n_lm, d_desc, cnt + RC_NKP, n_kp, nullptr, nullptr, h->top_idx.get(), h->top_dist.get());
    hipLaunchKernelGGL(k_rl_propose, dim3(gl), dim3(256), 0, st, n_lm, d_lm_xyz, (const int*)h->top_idx.get(), (const int*)h->top_dist.get(), P.max_hamming,
                       P.ratio_pct, h->state.get(), h->key.get(), cnt);
  }
  if (h->timing) DVS_HIP(hipEventRecord(h->ev[1], st));
  // ---- stages 2 and 3
  hipLaunchKernelGGL(k_rl_list, dim3(1), dim3(256), 0, st, n_kp, (const unsigned long long*)h->key.get(), d_lm_xyz, d_kps, P.min_pairs, h->obj.get(), h->img.get(),
                     h->p_lm.get(), h->p_kp.get(), h->p_dist.get(), cnt);
  DVS_HIP(hipGetLastError());
  if (h->timing) DVS_HIP(hipEventRecord(h->ev[2], st));
  // ---- stage 4
  DVS_TRY(pnp_own_device(h->ctx, h->obj.get(), h->img.get(), cnt + RC_NPNP, (unsigned long long)P.seed, P.K4, P.pnp_iterations, P.pnp_reproj_err,
                         P.pnp_confidence, h->p_inl.get(), h->pnp.get()));
  hipLaunchKernelGGL(k_rl_record, dim3(1), dim3(64), 0, st, (const int*)cnt, (const PnpRecord*)h->pnp.get(), h->d_rec.get());
  DVS_HIP(hipGetLastError());
  PinnedIo* io;
  DVS_TRY(matcher_pinned(h->ctx, sizeof(RlRec), &io));
  if (h->timing) DVS_HIP(hipEventRecord(h->ev[3], st));
  DVS_TRY(io->fetch(st, h->d_rec.get(), io->h(), sizeof(RlRec), 65536));   // the call's first wait
  if (h->timing) { DVS_HIP(hipEventSynchronize(h->ev[3])); h->timed = true; }
  RlRec rec;
  memcpy(&rec, io->h(), sizeof(rec));
  h->last_pnp = rec.pnp;
  const PnpRecord& pnp = rec.pnp;
  memset(result, 0, sizeof(*result));
  result->R[0] = result->R[4] = result->R[8] = 1.0;
  result->n_proposed = rec.n_proposed; result->n_pairs = rec.n_pairs;
  h->last_n_lm = n_lm; h->last_n_kp = n_kp; h->last_pairs = rec.n_pairs;
  if (rec.n_pairs < P.min_pairs) { result->status = DVS_RELOC_FEW_PAIRS; return DVS_OK; }
  result->pnp_inliers = pnp.n_inliers; result->pnp_success = pnp.success;
  h->last_inliers = pnp.n_inliers;
  bool finite = true;
  for (int k = 0; k < 3; k++) finite = finite && __builtin_isfinite(pnp.rvec[k]) && __builtin_isfinite(pnp.tvec[k]);
  if (!pnp.success || pnp.n_inliers < P.min_pnp_inliers || !finite) { result->status = DVS_RELOC_NO_POSE; return DVS_OK; }
  reloc_pose(pnp.rvec, pnp.tvec, result->pnp_R, result->pnp_t);
  // ---- stage 5
  DVS_TRY(dvs_maptrack_track_device(mt, d_lm_xyz, d_lm_desc, d_lm_id, n_lm, d_kps, d_desc, n_kp, result->pnp_R, result->pnp_t, &result->track));
  if (result->track.status == DVS_MAPTRACK_OK && result->track.n_inliers >= P.min_confirmed) {
    result->status = DVS_RELOC_OK;
    memcpy(result->R, result->track.R, sizeof(result->R)); memcpy(result->t, result->track.t, sizeof(result->t));
  } else {
    result->status = DVS_RELOC_NOT_CONFIRMED;
  }
  return DVS_OK;
}

dvs_status dvs_reloc_locate(dvs_reloc* h, dvs_maptrack* mt, const float* lm_xyz, const uint8_t* lm_desc, const int64_t* lm_id, int32_t n_lm,
                            const dvs_keypoint* kps, const uint8_t* desc, int32_t n_kp, dvs_reloc_result* result) {
  DVS_ARG(h && mt && result && n_lm >= 0 && n_kp >= 0 && n_lm <= (1 << 30) - 1 && n_kp <= (1 << 30));
  DVS_ARG((n_lm == 0 || (lm_xyz && lm_desc)) && (n_kp == 0 || (kps && desc)));
  // the image and the octave table are the confirming handle's
  DVS_TRY(stage_frame(h->stage, maptrack_params(mt), h->device, h->ctx->stream, lm_xyz, lm_desc, lm_id, n_lm, kps, desc, n_kp));
  const FrameStaging& S = h->stage;
  return dvs_reloc_locate_device(h, mt, S.xyz.get(), S.ldesc.get(), S.ids(lm_id, n_lm), n_lm, S.kps.get(), S.kdesc.get(), n_kp, result);
}

dvs_status dvs_reloc_get_pairs(dvs_reloc* h, int32_t cap, int32_t* lm_row, int32_t* kp_index, int32_t* dist, uint8_t* pnp_inlier, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  const int m = h->last_pairs;
  *n = m;
  if (m > cap && (lm_row || kp_index || dist || pnp_inlier)) { set_error("dvs_reloc_get_pairs: %d pairs, capacity %d", m, cap); return DVS_ERR_CAPACITY; }
  if (m == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  std::vector<int> inl;
  DVS_TRY(copy_out(lm_row, h->p_lm, (size_t)m, st)); DVS_TRY(copy_out(kp_index, h->p_kp, (size_t)m, st)); DVS_TRY(copy_out(dist, h->p_dist, (size_t)m, st));
  const int ni = h->last_inliers < m ? h->last_inliers : m;
  if (pnp_inlier && ni > 0) {
    inl.resize((size_t)ni);
    DVS_TRY(copy_out(inl.data(), h->p_inl, (size_t)ni, st));
  }
  DVS_HIP(hipStreamSynchronize(st));
  if (pnp_inlier) {
    memset(pnp_inlier, 0, (size_t)m);
    for (int i : inl) if (i >= 0 && i < m) pnp_inlier[i] = 1;   // RANSAC's ascending inlier indices as flags
  }
  return DVS_OK;
}

dvs_status dvs_backend_relocalize_frame(dvs_backend* b, dvs_reloc* h, dvs_maptrack* mt, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp,
                                        dvs_reloc_result* result) {
  DVS_ARG(b && h && mt && result && b->device == h->device);
  DVS_TRY(rl_check_args(h, mt, b->lm.xyz.get(), b->lm.desc.get(), b->nlm, d_kps, d_desc, n_kp, result));
  DVS_HIP(hipSetDevice(b->device));
  DVS_HIP(hipStreamSynchronize(b->ctx->stream));   // the table as the backend's last call left it
  return dvs_reloc_locate_device(h, mt, b->lm.xyz.get(), b->lm.desc.get(), (const int64_t*)b->lm.id.get(), b->nlm, d_kps, d_desc, n_kp, result);
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test_reloc.h)
dvs_status dvs_test_reloc_landmarks(dvs_reloc* h, int32_t cap, dvs_reloc_lm_record* rec, int32_t* n) {
  DVS_ARG(h && n && cap >= 0);
  *n = h->last_n_lm;
  if (!rec || *n == 0) return DVS_OK;
  if (*n > cap) { set_error("dvs_test_reloc_landmarks: %d rows, capacity %d", *n, cap); return DVS_ERR_CAPACITY; }
  const size_t nl = (size_t)*n, nk = (size_t)h->last_n_kp;
  for (size_t j = 0; j < nl; j++) { rec[j].best_k = -1; rec[j].d_best = -1; rec[j].d_second = -1; rec[j].proposed = 0; rec[j].kept = 0; }
  if (nk == 0) return DVS_OK;   // no keypoint: nothing was compared
  std::vector<int> ti(2 * nl), td(2 * nl);
  std::vector<signed char> stt(nl);
  std::vector<unsigned long long> key(nk);
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->ctx->stream;
  DVS_TRY(copy_out(ti.data(), h->top_idx, nl, st)); DVS_TRY(copy_out(td.data(), h->top_dist, nl, st));
  DVS_TRY(copy_out(stt.data(), h->state, nl, st)); DVS_TRY(copy_out(key.data(), h->key, nk, st));
  DVS_HIP(hipStreamSynchronize(st));
  for (size_t j = 0; j < nl; j++) {
    if (stt[j] < 0) continue;   // a position that is not finite: never compared
    rec[j].best_k = ti[2 * j]; rec[j].d_best = td[2 * j]; rec[j].d_second = ti[2 * j + 1] >= 0 ? td[2 * j + 1] : -1;
    rec[j].proposed = stt[j] == 1 ? 1 : 0;
    rec[j].kept = (stt[j] == 1 && key[(size_t)ti[2 * j]] != kRlNoKey && (key[(size_t)ti[2 * j]] & kRlRowMask) == (unsigned long long)j) ? 1 : 0;
  }
  return DVS_OK;
}

// (no device work) stage 4's record of the last locate call: what dvs_solve_pnp_ransac would have returned
dvs_status dvs_test_reloc_pnp_record(dvs_reloc* h, int32_t* n_inliers, int32_t* success, double* rvec3, double* tvec3) {
  DVS_ARG(h && n_inliers && success && rvec3 && tvec3);
  const PnpRecord& r = h->last_pnp;
  *n_inliers = r.n_inliers; *success = r.success; memcpy(rvec3, r.rvec, sizeof(r.rvec)); memcpy(tvec3, r.tvec, sizeof(r.tvec));
  return DVS_OK;
}
#endif

}  // extern "C"
