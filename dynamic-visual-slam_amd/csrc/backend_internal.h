// backend_internal.h — the mapping backend handle (dvs_backend, include/dvslam_hip.h) shared by backend.hip, loop_close.hip,
// covisibility.hip, kf_cull.hip, landmark_refresh.hip, lm_cull.hip and map_track.hip's recording: the views of the landmark and observation
// tables that kernels take and the one copy of a row of each, the owners of the tables, the keyframe record, the counter block, the row
// groups of per-call scratch and the handle itself.  What removes rows from the tables does it through table_compact.h, which builds on
// this header.  Internal to the library, as loop_internal.h and bow_internal.h are.
#pragma once
#include <stddef.h>
#include <tuple>
#include <unordered_map>
#include <utility>
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

// A table states its columns once, in columns(): owner, elements per row and element type are the member's Column type.  alloc, view,
// table_copy and the getters' byte counts (copy_out) all come from there.
template <class Table> dvs_status table_alloc(Table& t, size_t c) {
  DVS_TRY(std::apply([&](auto&... col) { return alloc_rows(c, col...); }, Table::columns(t)));
  t.cap = c;
  return DVS_OK;
}
template <class Table, size_t... I> dvs_status table_copy(Table& dst, const Table& src, size_t n, hipStream_t st, std::index_sequence<I...>) {
  const auto d = Table::columns(dst);
  const auto s = Table::columns(src);
  hipError_t e = hipSuccess;
  (void)(... && ((e = hipMemcpyAsync(std::get<I>(d).get(), std::get<I>(s).get(), n * std::get<I>(s).row_bytes, hipMemcpyDeviceToDevice, st)) == hipSuccess));
  DVS_HIP(e);
  return DVS_OK;
}
struct LmTable {
  Column<i64> id, seen; Column<int> cls, cnt; Column<float, 3> xyz; Column<uint8_t, 32> desc;
  size_t cap = 0;
  template <class S> static auto columns(S& t) { return std::tie(t.id, t.seen, t.cls, t.cnt, t.xyz, t.desc); }
  LmView view() const { return std::apply([](auto&... c) { return LmView{c.get()...}; }, columns(*this)); }
};
struct ObTable {
  Column<i64> id, frame, lm; Column<int> kf, cls; Column<float, 2> px; Column<uint8_t, 32> desc;
  size_t cap = 0;
  template <class S> static auto columns(S& t) { return std::tie(t.id, t.frame, t.lm, t.kf, t.cls, t.px, t.desc); }
  ObView view() const { return std::apply([](auto&... c) { return ObView{c.get()...}; }, columns(*this)); }
};
// a table of capacity `c` (at least `need` rows; doubled from the live one) with the first n rows of `live`, which it then replaces; the
// old blocks are freed by the assignment, after the stream has drained
template <class Table> dvs_status table_regrow(Table& live, size_t need, size_t n, hipStream_t st) {
  if (need <= live.cap) return DVS_OK;
  size_t c = std::max<size_t>(live.cap, 1);
  while (c < need) c *= 2;
  Table t;
  DVS_TRY(table_alloc(t, c));
  if (n) DVS_TRY(table_copy(t, live, n, st, std::make_index_sequence<std::tuple_size<decltype(Table::columns(t))>::value>()));
  DVS_HIP(hipStreamSynchronize(st));
  live = std::move(t);
  return DVS_OK;
}
// One row of a table into row p of another, every column: the only place that lists a table's columns for a copy.  A caller that changes
// a column stores it again behind the copy.
static_assert(std::tuple_size<decltype(LmTable::columns(std::declval<LmTable&>()))>::value == 6, "lm_row_copy writes every column of the landmark table");
__device__ __forceinline__ void lm_row_copy(const LmView& dst, size_t p, const LmView& src, size_t s) {
  dst.id[p] = src.id[s]; dst.seen[p] = src.seen[s]; dst.cls[p] = src.cls[s]; dst.cnt[p] = src.cnt[s];
  dst.xyz[3 * p] = src.xyz[3 * s]; dst.xyz[3 * p + 1] = src.xyz[3 * s + 1]; dst.xyz[3 * p + 2] = src.xyz[3 * s + 2];
  copy32(dst.desc + 32 * p, src.desc + 32 * s);
}
static_assert(std::tuple_size<decltype(ObTable::columns(std::declval<ObTable&>()))>::value == 7, "ob_row_copy writes every column of the observation table");
__device__ __forceinline__ void ob_row_copy(const ObView& dst, size_t p, const ObView& src, size_t s) {
  dst.id[p] = src.id[s]; dst.frame[p] = src.frame[s]; dst.lm[p] = src.lm[s]; dst.kf[p] = src.kf[s]; dst.cls[p] = src.cls[s];
  dst.px[2 * p] = src.px[2 * s]; dst.px[2 * p + 1] = src.px[2 * s + 1];
  copy32(dst.desc + 32 * p, src.desc + 32 * s);
}
// the spare table that receives a compaction of `live` and then changes places with it: as large as the live one
template <class Table> dvs_status table_match_spare(Table& spare, const Table& live) { return spare.cap != live.cap ? table_alloc(spare, live.cap) : DVS_OK; }

struct KeyframeRec { uint64_t frame_id; i64 stamp; std::vector<uint64_t> obs_ids; double R[9], t[3]; };

// The 256 ints of counters and small lists that kernels write and the host reads back, one block per handle (dvs_backend::s_small).
// add_keyframe uploads the whole block: its two lists, and zeros everywhere else.
struct FuseCounts { int n_query, n_sources, n_targets, n_proposals, n_fused, n_kept, n_anchored, pad; };   // n_anchored: k_anchors, cleared on its own;
                                                                                                          // n_kept: no longer written, the compaction's total is read instead
struct CullCounts { int n_culled, n_ob_removed, n_lm_removed, pad; };   // k_cull_walk; k_cull_ob_flag; k_cull_lm_flag
struct RefreshCounts { int n_bin[3], n_in_scope, n_without_views, max_views, n_changed, pad; };   // k_lr_bin; n_changed: k_lr_apply
struct LmCullCounts { int n_by_ratio, n_weak, pad[2]; };   // k_lc_decide
struct BackendSmall {
  int filtered[64];     // add_keyframe: the filtered class ids
  int classes[64];       //               the distinct unfiltered classes of the keyframe
  int class_cnt[64];     //               k_categorize: kept observations per class
  int counts[4];         // the call's one-block kernel: k_class_gather {landmarks of the class}, k_window_gather {observations, landmarks}.
                         // counts[0 .. 2] are no longer written by prune: its compactions' totals are read instead (table_compact.h)
  int marked, pad0[3];   // k_prune_mark: marked landmarks
  FuseCounts fuse;       // loop_close.hip
  int left_out, pad1[3];    // covisibility.hip, k_covis_ob_flag: rows left out of the local window
  CullCounts cull;          // kf_cull.hip
  RefreshCounts refresh;    // landmark_refresh.hip
  LmCullCounts lmcull;      // lm_cull.hip
  int pad2[28];
};
static_assert(sizeof(BackendSmall) == 256 * 4 && offsetof(BackendSmall, classes) == 64 * 4 && offsetof(BackendSmall, class_cnt) == 128 * 4 &&
              offsetof(BackendSmall, counts) == 192 * 4 && offsetof(BackendSmall, marked) == 196 * 4 && offsetof(BackendSmall, fuse) == 200 * 4 &&
              offsetof(BackendSmall, fuse.n_anchored) == 206 * 4 && offsetof(BackendSmall, left_out) == 208 * 4, "kernels and the upload keep these addresses");
static_assert(offsetof(BackendSmall, cull) == 212 * 4, "the culling counters take the padding behind left_out");
static_assert(offsetof(BackendSmall, refresh) == 216 * 4, "and the refresh counters the padding behind them");
static_assert(offsetof(BackendSmall, lmcull) == 224 * 4, "and the landmark culling counters the padding behind those");

// The eight columns a BA window hands out, in two halves by row domain; the sliding window and the local window each hold both.
struct WindowObs { Column<float, 2> px; Column<i64> lm; Column<int> cls; Column<i64> frame; Column<int> lmidx; };
struct WindowLms { Column<i64> id; Column<int> cls; Column<float, 3> xyz; };
inline dvs_status window_copy_out(const WindowObs& o, size_t no, const WindowLms& l, size_t nl, float* o_px, uint64_t* o_lm, int32_t* o_cls, uint64_t* o_frame,
                                  int32_t* o_lmidx, uint64_t* l_id, int32_t* l_cls, float* l_xyz, hipStream_t st) {
  if (no) { DVS_TRY(copy_out(o_px, o.px, no, st)); DVS_TRY(copy_out(o_lm, o.lm, no, st)); DVS_TRY(copy_out(o_cls, o.cls, no, st)); DVS_TRY(copy_out(o_frame, o.frame, no, st)); DVS_TRY(copy_out(o_lmidx, o.lmidx, no, st)); }
  if (nl) { DVS_TRY(copy_out(l_id, l.id, nl, st)); DVS_TRY(copy_out(l_cls, l.cls, nl, st)); DVS_TRY(copy_out(l_xyz, l.xyz, nl, st)); }
  return DVS_OK;
}

// Row groups (device_mem.h, grow_rows): per-call scratch, grow-only.  Each names its row domain, its need and its size rule once.  The
// rules differ because each was chosen with its call; they are kept as they were, so that a map grows through the same allocations.
struct KeyframeObRows {   // per observation of the keyframe being added: a quarter to spare
  Column<float, 2> s_px; Column<float, 3> s_xyz; Column<uint8_t, 32> s_desc; Column<float, 2> q_px; Column<uint8_t, 32> q_desc; Column<int> s_code, s_order, d_best;
  size_t cap = 0;
  dvs_status grow(size_t n) { return grow_rows(cap, n, n + n / 4, s_px, s_xyz, s_desc, q_px, q_desc, s_code, s_order, d_best); }
};
struct ClassLmRows {      // per landmark gathered for one class: half to spare
  Column<int> slot; Column<uint8_t, 32> desc; Column<float, 3> xyz;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2, slot, desc, xyz); }
};
struct ViewLmRows {       // views CSR and triangulation per landmark, one row more for the CSR's end
  Column<int> cnt, fill; Column<i64> offs; Column<float, 3> tri_xyz; Column<int> tri_status;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm + 1, nlm + 1 + nlm / 2, cnt, fill, offs, tri_xyz, tri_status); }
};
struct ViewObRows {       // views per observation: its landmark row; the CSR's values (observation row, keyframe, pixel, observation id)
  Column<int> slot, rows, kf; Column<float, 2> px; Column<i64> oid;
  size_t cap = 0;
  dvs_status grow(size_t nob) { return grow_rows(cap, nob, nob + nob / 2 + 64, slot, rows, kf, px, oid); }
};
struct SlidingObRows {    // the sliding window per observation: table row and landmark row, then the window's columns
  Column<int> oi, slot; WindowObs o;
  size_t cap = 0;
  dvs_status grow(size_t nob) { return grow_rows(cap, nob, nob + nob / 2, oi, slot, o.px, o.lm, o.cls, o.frame, o.lmidx); }
};
struct SlidingLmRows {    // the sliding window per landmark: the window's columns, then in-window flag and row in the window
  WindowLms l; Column<int> flag, pos;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm + 1, nlm + 1 + nlm / 2, l.id, l.cls, l.xyz, flag, pos); }
};
struct CompactLmRows {    // what removes rows from the tables (table_compact.h) per landmark row: stays, leaves
  Column<int> keep, gone;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 64, keep, gone); }
};
struct CompactObRows {    // and per observation row: stays, leaves; the ids and keyframe indices of the rows that leave
  Column<int> keep, gone, rem_kf; Column<i64> rem_id;
  size_t cap = 0;
  dvs_status grow(size_t nob) { return grow_rows(cap, nob, nob + nob / 2 + 64, keep, gone, rem_kf, rem_id); }
};
struct BlockRows {        // per 256-row block of a table: the ordered compaction's counts and their scan, which ends with the total
  Column<int> cnt; Column<i64, 1, 1> offs;
  size_t cap = 0;
  dvs_status grow(size_t nblk) { return grow_rows(cap, nblk, nblk + nblk / 2, cnt, offs); }
};
struct FuseLmRows {       // fusion per landmark row: flags, proposals, the resolved pairs and the pair list
  Column<int> flag, src, propb, bsrc, redirect, partner; Column<unsigned long long> prope, beste; Column<i64> psurv, prem; Column<double> pe;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 1, flag, src, propb, bsrc, redirect, partner, prope, beste, psurv, prem, pe); }
};
struct FuseQueryRows {    // fusion per observation of the query keyframe
  Column<float, 2> px; Column<int> cls; Column<i64> oid; Column<int> brow; Column<uint8_t, 32> desc;
  size_t cap = 0;
  dvs_status grow(size_t nq) { return grow_rows(cap, nq, nq + nq / 4, px, cls, oid, brow, desc); }
};
struct CovisObRows {      // covisibility per observation: the keyframe where the view counts, keyframe -> landmarks CSR; in-window flag, the local window's columns
  Column<int> kf, tmp, list, flag; WindowObs o;
  size_t cap = 0;
  dvs_status grow(size_t nob) { return grow_rows(cap, nob, nob + nob / 2 + 64, kf, tmp, list, flag, o.cls, o.lmidx, o.lm, o.frame, o.px); }
};
struct CovisKfRows {      // per keyframe, one row more for the CSRs' ends
  Column<int> cnt, fill, role, f, nbc; Column<i64> offs, nboffs;
  size_t cap = 0;
  dvs_status grow(size_t nkf) { return grow_rows(cap, nkf + 1, nkf + 1 + nkf / 2, cnt, fill, role, f, nbc, offs, nboffs); }
};
struct CovisLmRows {      // per landmark row: in U, row in U; U's columns (the local window's landmark half, and descriptors for the local map)
  Column<int> flag, pos, slot; WindowLms u; Column<uint8_t, 32> desc;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 64, flag, pos, slot, u.cls, u.id, u.xyz, desc); }
};
struct CovisWeightRows {  // requested rows x keyframes: weights and neighbour lists, packed CSR.  Exact: the full graph asks for nkf * nkf once
  Column<int> w, nbt, nbi, nbw, pki, pkw;
  size_t cap = 0;
  dvs_status grow(size_t n) { return grow_rows(cap, n, n, w, nbt, nbi, nbw, pki, pkw); }
};
struct CullKfRows {       // culling per keyframe, one row more for the scan's end: scope and protection from the host, n_k, the initial R_k, initially
                          // redundant candidates and their list, culled and kept flags, index in the table after the apply
  Column<uint8_t> state; Column<int> n_obs, r0, flag, walk, culled, keep; Column<i64> newidx;
  size_t cap = 0;
  dvs_status grow(size_t nkf) { return grow_rows(cap, nkf + 1, nkf + 1 + nkf / 2, state, n_obs, r0, flag, walk, culled, keep, newidx); }
};
struct CullLmRows {       // culling per landmark row: c(L), removed rows
  Column<int> c, removed;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 64, c, removed); }
};
struct RefreshLmRows {    // landmark refresh per landmark row: views, in scope; the three bins' lists; the chosen view (index into the views), its
                          // median and observation id; the viewing geometry
  Column<int> n, scope, list0, list1, list2, best, med, ncnt; Column<i64> oid; Column<double, 3> normal; Column<double, 2> range;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 64, n, scope, list0, list1, list2, best, med, ncnt, oid, normal, range); }
};
struct LmStatRows {      // the tracking statistics, a side table of the landmark table joined by id ("Landmark culling" in the header): after
                          // lm_stats_align row s is landmark row s.  The handle holds a live one and a spare the alignment and the cull write
  Column<i64> id; Column<int> visible, found;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 64, id, visible, found); }
};
struct StatView { i64* id; int* visible; int* found; };
inline StatView stat_view(const LmStatRows& t) { return StatView{t.id.get(), t.visible.get(), t.found.get()}; }
struct LmCullLmRows {     // landmark culling per landmark row: views, age in keyframes, the rule that holds (0: none), leaves; the culled ids and their
                          // reasons compacted
  Column<int> n, age, reason, mark, creason; Column<i64> cid;
  size_t cap = 0;
  dvs_status grow(size_t nlm) { return grow_rows(cap, nlm, nlm + nlm / 2 + 64, n, age, reason, mark, creason, cid); }
};

}  // namespace dvs

struct dvs_backend {
  dvs_backend_params P;
  int device = 0;
  dvs_matcher* ctx = nullptr;
  // the map
  dvs::LmTable lm, lm_spare; dvs::ObTable ob, ob_spare;          // the spare pair receives a compaction and changes places (table_compact.h)
  dvs::Column<double, 9> kf_R; dvs::Column<double, 3> kf_t;
  size_t cap_kf = 0;
  int nlm = 0, nob = 0;
  std::vector<dvs::KeyframeRec> kfs;                      // keyframes_
  std::unordered_map<uint64_t, int> kf_index;        // frame_id -> index
  dvs::i64 next_obs = 0, next_lm = 0;                     // next_observation_id_, next_global_landmark_id_
  // the counter block, the keyframe's pose
  dvs::DeviceBuf<dvs::BackendSmall> s_small;
  dvs::DeviceBuf<double> d_Rt;
  // row groups: add_keyframe and the views; the sliding window; the compaction (table_compact.h); fusion (loop_close.hip); covisibility
  // (covisibility.hip)
  dvs::KeyframeObRows kf_ob; dvs::ClassLmRows cls_lm; dvs::ViewLmRows v_lm; dvs::ViewObRows v_ob;
  dvs::SlidingObRows win_ob; dvs::SlidingLmRows win_lm;
  dvs::CompactLmRows cmp_lm; dvs::CompactObRows cmp_ob; dvs::BlockRows blk;
  dvs::FuseLmRows fuse_lm; dvs::FuseQueryRows fuse_q;
  dvs::CovisObRows cv_ob; dvs::CovisKfRows cv_kf; dvs::CovisLmRows cv_lm; dvs::CovisWeightRows cv_w;
  dvs::CullKfRows cull_kf; dvs::CullLmRows cull_lm;
  dvs::RefreshLmRows lr_lm;
  // landmark culling (lm_cull.hip): the statistics and their spare (not allocated before first use), the recording switch, the calls that recorded
  dvs::LmStatRows stat, stat_spare; int nstat = 0; int stats_on = 0; dvs::i64 n_recorded = 0;
  dvs::LmCullLmRows lc_lm;
  // single blocks (device_mem.h, grow): detections, candidate pairs, per-call arguments, anchors per landmark, landmark row per observation
  dvs::DeviceBuf<dvs::DetRec> s_det; dvs::DeviceBuf<dvs::PairRec> p_rec; dvs::DeviceBuf<int> a_int, f_obrow; dvs::Column<int> f_anchor; dvs::DeviceBuf<dvs::i64> a_i64; dvs::DeviceBuf<double> a_dbl;
  size_t c_det = 0, c_pair = 0, c_aint = 0, c_ai64 = 0, c_adbl = 0, c_flm = 0, c_fob = 0;
  // host staging that asynchronous copies read until the call's last synchronisation
  dvs::BackendSmall h_small;
  std::vector<float> h_px, h_xyz;
  std::vector<int> h_int;
  std::vector<dvs::i64> h_i64;
  std::vector<double> h_dbl;
  std::vector<dvs::DetRec> h_det;
};

namespace dvs {
// `n` ints of the counter block from device address `field` on, to dst: enqueued, then the stream is synchronised
inline dvs_status small_read(dvs_backend* h, const int* field, int* dst, int n = 1) {
  DVS_HIP(hipMemcpyAsync(dst, field, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->ctx->stream));
  DVS_HIP(hipStreamSynchronize(h->ctx->stream));
  return DVS_OK;
}
}  // namespace dvs

namespace dvs {
// landmark -> views CSR over the whole table into v_lm.offs and v_ob.kf / .px / .oid, segments in observation order, on the
// handle's stream (backend.hip); nothing to do for an empty landmark table
dvs_status backend_views_build(dvs_backend* h);
// the local map of keyframe ref_frame_id ("Covisibility" in the header; covisibility.hip): U's positions, descriptors and ids compacted in
// ascending id into the handle's scratch, device pointers valid until the handle's next call; the stream has been synchronised.  The
// argument errors of the section are returned before any device work.
dvs_status backend_local_map(dvs_backend* h, uint64_t ref_frame_id, const dvs_covis_params* params, const float** d_xyz, const uint8_t** d_desc,
                             const i64** d_id, int* n);
// What covisibility.hip shares with kf_cull.hip, all enqueued on the handle's stream:
// DVS_ERR_CAPACITY if the map holds more keyframes than the row kernel's LDS histogram takes
dvs_status covis_limit(const dvs_backend* h, const char* who);
// the covisibility row groups for the keyframes and tables as they stand and `rows` rows of weights
dvs_status covis_grow(dvs_backend* h, size_t rows);
// the views CSR, the counting views (cv_ob.kf: the keyframe where a view counts, or -1) and the keyframe -> landmarks CSR (cv_kf.offs,
// cv_ob.list); needs at least one landmark and one keyframe
dvs_status covis_prepare(dvs_backend* h);
// `rows` rows of W from keyframe row0 on into cv_w.w, and their neighbour lists at theta into cv_w.nbi / cv_w.nbw / cv_kf.nbc
dvs_status covis_rows(dvs_backend* h, int row0, int rows, int theta);
// the viewing geometry of every landmark row ("Landmark refresh" in the header; landmark_refresh.hip) into lr_lm.normal / .range / .ncnt:
// the views are rebuilt, everything is enqueued on the handle's stream; needs at least one landmark
dvs_status refresh_geometry(dvs_backend* h);
// the keyframes' observation_ids lose the ids in `gone` (:1303-1312); kf: the keyframe index of each removed row -> the keyframes that lost
// at least one id (backend.hip; table_compact.h's cascade for dvs_backend_prune and dvs_backend_cull_landmarks)
int backend_drop_observation_ids(dvs_backend* h, const std::vector<i64>& gone, const std::vector<int>& kf);
// the statistics aligned to the landmark table as it stands ("Landmark culling" in the header; lm_cull.hip): enqueued on the handle's stream;
// afterwards h->nstat == h->nlm and statistics row s is landmark row s
dvs_status lm_stats_align(dvs_backend* h);
}  // namespace dvs
