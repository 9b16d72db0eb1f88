// backend_internal.h — the mapping backend handle (dvs_backend, include/dvslam_hip.h) shared by backend.hip and loop_close.hip: the views of
// the landmark and observation tables that kernels take, the owners of the tables, the keyframe record and the handle itself.  Internal
// to the library, as loop_internal.h and bow_internal.h are.
#pragma once
#include <unordered_map>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "matcher.h"

namespace dvs {

typedef long long i64;

struct LmView { i64* id; i64* seen; int* cls; int* cnt; float* xyz; uint8_t* desc; };
struct ObView { i64* id; i64* frame; i64* lm; int* kf; int* cls; float* px; uint8_t* desc; };
struct PairRec { i64 id; int j, slot, status; float xyz[3], tri[3]; int pad; };   // 48 bytes
struct DetRec { double cx, cy, w, h; int cls, pad; };

// row of landmark `key` in the ascending id column, -1 if the table does not hold it
__device__ __forceinline__ int lm_find(const i64* __restrict__ id, int n, i64 key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (id[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && id[lo] == key) ? lo : -1;
}
__device__ __forceinline__ void copy32(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src) {   // one descriptor row, 16-byte aligned
  const uint4 a = reinterpret_cast<const uint4*>(src)[0], b = reinterpret_cast<const uint4*>(src)[1];
  reinterpret_cast<uint4*>(dst)[0] = a; reinterpret_cast<uint4*>(dst)[1] = b;
}

struct LmTable {
  DeviceBuf<i64> id, seen; DeviceBuf<int> cls, cnt; DeviceBuf<float> xyz; DeviceBuf<uint8_t> desc;
  size_t cap = 0;
  dvs_status alloc(size_t c) {
    DVS_TRY(id.alloc(c)); DVS_TRY(seen.alloc(c)); DVS_TRY(cls.alloc(c)); DVS_TRY(cnt.alloc(c)); DVS_TRY(xyz.alloc(c * 3)); DVS_TRY(desc.alloc(c * 32));
    cap = c;
    return DVS_OK;
  }
  LmView view() const { return LmView{id.get(), seen.get(), cls.get(), cnt.get(), xyz.get(), desc.get()}; }
};
struct ObTable {
  DeviceBuf<i64> id, frame, lm; DeviceBuf<int> kf, cls; DeviceBuf<float> px; DeviceBuf<uint8_t> desc;
  size_t cap = 0;
  dvs_status alloc(size_t c) {
    DVS_TRY(id.alloc(c)); DVS_TRY(frame.alloc(c)); DVS_TRY(lm.alloc(c)); DVS_TRY(kf.alloc(c)); DVS_TRY(cls.alloc(c)); DVS_TRY(px.alloc(c * 2));
    DVS_TRY(desc.alloc(c * 32));
    cap = c;
    return DVS_OK;
  }
  ObView view() const { return ObView{id.get(), frame.get(), lm.get(), kf.get(), cls.get(), px.get(), desc.get()}; }
};

struct KeyframeRec { uint64_t frame_id; i64 stamp; std::vector<uint64_t> obs_ids; double R[9], t[3]; };

}  // namespace dvs

struct dvs_backend {
  dvs_backend_params P;
  int device = 0;
  dvs_matcher* ctx = nullptr;
  // the map
  dvs::LmTable lm, lm_spare; dvs::ObTable ob, ob_spare;          // the spare pair receives dvs_backend_prune's compaction
  dvs::DeviceBuf<double> kf_R, kf_t;
  size_t cap_kf = 0;
  int nlm = 0, nob = 0;
  std::vector<dvs::KeyframeRec> kfs;                      // keyframes_
  std::unordered_map<uint64_t, int> kf_index;        // frame_id -> index
  dvs::i64 next_obs = 0, next_lm = 0;                     // next_observation_id_, next_global_landmark_id_
  // per-call staging and scratch (grow-only)
  dvs::DeviceBuf<float> s_px, s_xyz, q_px, g_xyz, tri_xyz, view_px, w_px, w_lxyz;
  dvs::DeviceBuf<uint8_t> s_desc, q_desc, g_desc;
  dvs::DeviceBuf<int> s_code, s_order, s_small, g_slot, d_best, ob_slot, v_cnt, v_fill, v_obs, view_kf, tri_status, a_int, w_flag, w_pos, w_oi, w_slot, w_cls,
      w_lmidx, w_lcls;
  dvs::DeviceBuf<dvs::i64> view_offs, view_oid, a_i64, w_lm, w_frame, w_lid;
  dvs::DeviceBuf<dvs::DetRec> s_det;
  dvs::DeviceBuf<dvs::PairRec> p_rec;
  dvs::DeviceBuf<int> p_flag, rem_kf;
  dvs::DeviceBuf<dvs::i64> rem_id;
  size_t c_pflag = 0, c_rem = 0;
  dvs::DeviceBuf<double> d_Rt, a_dbl;
  size_t c_n = 0, c_det = 0, c_glm = 0, c_vlm = 0, c_vob = 0, c_pair = 0, c_aint = 0, c_ai64 = 0, c_adbl = 0, c_wob = 0, c_wlm = 0;
  // host staging that asynchronous copies read until the call's last synchronisation
  std::vector<float> h_px, h_xyz;
  std::vector<int> h_int;
  std::vector<dvs::i64> h_i64;
  std::vector<double> h_dbl;
  std::vector<dvs::DetRec> h_det;
  // loop closing (loop_close.hip): anchors, fusion flags and lists, all grow-only
  dvs::DeviceBuf<int> f_anchor, f_obrow, f_flag, f_src, f_qbrow, f_qcls, f_propb, f_bsrc, f_redirect, f_partner;
  dvs::DeviceBuf<float> f_qpx;
  dvs::DeviceBuf<uint8_t> f_qdesc;
  dvs::DeviceBuf<dvs::i64> f_qoid, f_psurv, f_prem;
  dvs::DeviceBuf<unsigned long long> f_prope, f_beste;
  dvs::DeviceBuf<double> f_pe;
  size_t c_flm = 0, c_frow = 0, c_fob = 0, c_fq = 0;   // anchors; fusion per landmark row / per observation / per query observation
  // covisibility (covisibility.hip), all grow-only: per view / per keyframe / per landmark row / per observation / per requested row x keyframe
  dvs::DeviceBuf<int> cv_kf, cv_tmp, cv_list;                                    // per view: the keyframe where the view counts, keyframe -> landmarks CSR
  dvs::DeviceBuf<int> cv_cnt, cv_fill, cv_role, cv_f, cv_blk;                    // per keyframe (cv_blk: per 256-row block of a table)
  dvs::DeviceBuf<dvs::i64> cv_offs, cv_nboffs, cv_blkoffs;
  dvs::DeviceBuf<int> cv_lflag, cv_lpos, cv_uslot, cv_ucls;                      // per landmark row: in U, row in U; U's columns
  dvs::DeviceBuf<dvs::i64> cv_uid;
  dvs::DeviceBuf<float> cv_uxyz;
  dvs::DeviceBuf<uint8_t> cv_udesc;
  dvs::DeviceBuf<int> cv_oflag, cv_ocls, cv_olmidx;                              // per observation: in the window; the window's columns
  dvs::DeviceBuf<dvs::i64> cv_olm, cv_oframe;
  dvs::DeviceBuf<float> cv_opx;
  dvs::DeviceBuf<int> cv_w, cv_nbt, cv_nbi, cv_nbw, cv_nbc, cv_pki, cv_pkw;      // weights and neighbour lists, rows x keyframes; packed CSR
  size_t c_cvv = 0, c_cvk = 0, c_cvl = 0, c_cvo = 0, c_cvw = 0, c_cvb = 0;
};

namespace dvs {
// landmark -> views CSR over the whole table into view_offs / view_kf / view_px / view_oid, segments in observation order, on the
// handle's stream (backend.hip); nothing to do for an empty landmark table
dvs_status backend_views_build(dvs_backend* h);
// the local map of keyframe ref_frame_id ("Covisibility" in the header; covisibility.hip): U's positions, descriptors and ids compacted in
// ascending id into the handle's scratch, device pointers valid until the handle's next call; the stream has been synchronised.  The
// argument errors of the section are returned before any device work.
dvs_status backend_local_map(dvs_backend* h, uint64_t ref_frame_id, const dvs_covis_params* params, const float** d_xyz, const uint8_t** d_desc,
                             const i64** d_id, int* n);
}  // namespace dvs
