// loop.hip — loop candidates: a keyframe database with a direct index (every entry's FeatureVector and descriptor rows kept on the
// device) and node-guided, ratio-tested, one-to-one matching of a query frame against candidate entries.  The semantics are the
// header's (include/dvslam_hip.h, "loop candidates"); tests/loop_ref.py is their sequential restatement.  The inverted part (BowVectors,
// query, selection) is bow.hip's, reached through bow_internal.h: this file adds no copy of it.  Integers only.
//   k_loop_append    a transformed frame's rows and FeatureVector appended to the direct index (one block per frame)
//   k_loop_init      outputs unmatched, the per-candidate winner column at its maximum, n_matches 0 (-1: entry id out of range)
//   k_loop_propose   one wavefront per (candidate, 64 positions of the query's FeatureVector): the entry's features under the same nodes
//                    are staged through LDS in tiles of kMatchTileRows rows; per query feature a running (d1, j1, d2); a proposal does
//                    atomicMin(d1 << 32 | i) on its entry feature's slot
//   k_loop_resolve   a proposal stays where its i won the slot; the candidate's count
//   k_loop_set_points  an entry's 3D points (the block loop_verify.hip reads) copied from a batch in add_device's layout
// The minimum of a set does not depend on the order of arrival, so the result is the same under any schedule.
#include <limits.h>
#include <vector>
#include "common.h"
#include "device_mem.h"
#include "bow_internal.h"
#include "loop_internal.h"

namespace {
using namespace dvs;

constexpr int kBlock = 256;
constexpr int kMatchQueryBlock = 64;   // query features per workgroup of k_loop_propose: one wavefront, one feature per lane
constexpr int kMatchTileRows = 128;    // entry rows staged per trip: 128 * 32 B + 128 * 4 B = 4.5 KiB of LDS per workgroup

// the direct index: entry e owns rows [row_off[e], row_off[e + 1]) of every per-row block.  Its n descriptor rows fill desc; its
// FeatureVector has nn[e] <= n nodes (fv_nodes / fv_start, the first nn slots) and m[e] <= n features (fv_feat, the first m slots).
struct DirectIndex {
  const long long* row_off;
  const int* nn;
  const int* m;
  const uint4* desc;      // two per row
  const int* fv_nodes;
  const int* fv_start;    // node s holds fv_feat[fv_start[s] .. fv_start[s + 1]) — m[e] for the last node
  const int* fv_feat;
};

// frame f of a transformed batch (the vocabulary's own blocks) becomes entry first + f
__global__ __launch_bounds__(kBlock) void k_loop_append(int first, int stride_rows, const uint8_t* __restrict__ d_desc, const int* __restrict__ d_n,
                                                        const int* __restrict__ fv_nodes, const int* __restrict__ fv_offsets,
                                                        const int* __restrict__ fv_features, const int* __restrict__ n_fv_nodes,
                                                        long long* __restrict__ row_off, int* __restrict__ e_nn, int* __restrict__ e_m,
                                                        uint4* __restrict__ o_desc, int* __restrict__ o_nodes, int* __restrict__ o_start,
                                                        int* __restrict__ o_feat) {
  const int f = blockIdx.x;
  long long o = row_off[first];
  for (int g = 0; g < f; g++) o += min(max(d_n[g], 0), stride_rows);
  const int n = min(max(d_n[f], 0), stride_rows);
  const size_t base = (size_t)f * stride_rows, base1 = (size_t)f * (stride_rows + 1);
  const int nn = min(max(n_fv_nodes[f], 0), n);
  const int m = min(max(fv_offsets[base1 + nn], 0), n);
  const uint4* src = (const uint4*)(d_desc + base * 32);
  for (int r = threadIdx.x; r < 2 * n; r += kBlock) o_desc[2 * o + r] = src[r];
  for (int s = threadIdx.x; s < nn; s += kBlock) { o_nodes[o + s] = fv_nodes[base + s]; o_start[o + s] = fv_offsets[base1 + s]; }
  for (int r = threadIdx.x; r < m; r += kBlock) o_feat[o + r] = fv_features[base + r];
  if (threadIdx.x == 0) { e_nn[first + f] = nn; e_m[first + f] = m; row_off[first + f + 1] = o + n; }
}

__device__ __forceinline__ int clamp_count(const int* p, int cap) { return min(max(*p, 0), cap); }

// grid (x, cap_cand): everything a match writes starts from "unmatched"
__global__ __launch_bounds__(kBlock) void k_loop_init(int n_entries, int stride_rows, int key_stride, const int* __restrict__ d_entry_ids,
                                                      const int* __restrict__ d_n_cand, int cap_cand, int* __restrict__ train_idx,
                                                      int* __restrict__ dist, int* __restrict__ n_matches, unsigned long long* __restrict__ keys) {
  const int c = blockIdx.y;
  const int step = gridDim.x * kBlock, t0 = blockIdx.x * kBlock + threadIdx.x;
  for (int i = t0; i < stride_rows; i += step) { train_idx[(size_t)c * stride_rows + i] = -1; dist[(size_t)c * stride_rows + i] = INT_MAX; }
  for (int j = t0; j < key_stride; j += step) keys[(size_t)c * key_stride + j] = ~0ull;
  if (t0 == 0) {
    int v = 0;
    if (c < clamp_count(d_n_cand, cap_cand)) { const int id = d_entry_ids[c]; v = (id < 0 || id >= n_entries) ? -1 : 0; }
    n_matches[c] = v;
  }
}

// grid (positions of the query's FeatureVector / 64, cap_cand), 64 threads.  Position p of the query's feature list (ordered by node,
// then feature index) is feature i = q_feat[p] under node q_node[i]; its partners are the entry's list positions [a, b) under the same
// node.  Both lists are ascending in node id, so the block's partners lie between the smallest a and the largest b: that range is staged
// tile by tile, and a lane reads the part of a tile its own segment covers (lanes of one node read the same LDS rows: a broadcast).
__global__ __launch_bounds__(kMatchQueryBlock) void k_loop_propose(DirectIndex D, int n_entries, int stride_rows, int key_stride,
                                                                   const uint8_t* __restrict__ q_desc, const int* __restrict__ q_n_fv,
                                                                   const int* __restrict__ q_fv_offsets, const int* __restrict__ q_feat,
                                                                   const int* __restrict__ q_node, const int* __restrict__ d_entry_ids,
                                                                   const int* __restrict__ d_n_cand, int cap_cand, int max_distance, int ratio_num,
                                                                   int ratio_den, int* __restrict__ train_idx, int* __restrict__ dist,
                                                                   unsigned long long* __restrict__ keys) {
  __shared__ uint4 s_rows[kMatchTileRows * 2];
  __shared__ int s_j[kMatchTileRows];
  __shared__ int s_lo, s_hi;
  const int c = blockIdx.y;
  if (c >= clamp_count(d_n_cand, cap_cand)) return;
  const int e = d_entry_ids[c];
  if (e < 0 || e >= n_entries) return;
  const int qm = min(max(q_fv_offsets[min(max(*q_n_fv, 0), stride_rows)], 0), stride_rows);   // features in the query's FeatureVector
  if (blockIdx.x * kMatchQueryBlock >= qm) return;
  const long long eo = D.row_off[e];
  const int e_nn = D.nn[e], e_m = D.m[e];
  const int* e_nodes = D.fv_nodes + eo; const int* e_start = D.fv_start + eo; const int* e_feat = D.fv_feat + eo;
  const uint4* e_desc = D.desc + 2 * eo;
  const int p = blockIdx.x * kMatchQueryBlock + threadIdx.x;
  int i = -1, a = 0, b = 0;
  unsigned long long f0 = 0, f1 = 0, f2 = 0, f3 = 0;
  if (p < qm) {
    i = q_feat[p];
    const int node = q_node[i];
    int lo = 0, hi = e_nn;                            // first entry node >= node
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (e_nodes[mid] < node) lo = mid + 1; else hi = mid; }
    if (lo < e_nn && e_nodes[lo] == node) { a = e_start[lo]; b = lo + 1 < e_nn ? e_start[lo + 1] : e_m; }
    const uint4* row = (const uint4*)(q_desc + (size_t)i * 32);
    const uint4 x = row[0], y = row[1];
    f0 = (unsigned long long)x.y << 32 | x.x; f1 = (unsigned long long)x.w << 32 | x.z;
    f2 = (unsigned long long)y.y << 32 | y.x; f3 = (unsigned long long)y.w << 32 | y.z;
  }
  if (threadIdx.x == 0) { s_lo = INT_MAX; s_hi = 0; }
  __syncthreads();
  if (a < b) { atomicMin(&s_lo, a); atomicMax(&s_hi, b); }
  __syncthreads();
  const int lo = s_lo, hi = s_hi;
  int d1 = 257, d2 = 257, j1 = -1;                    // 257: above every distance; a lone partner leaves d2 there, read as 256 below
  for (int t = lo; t < hi; t += kMatchTileRows) {
    const int rows = min(kMatchTileRows, hi - t);
    __syncthreads();
    for (int h = threadIdx.x; h < 2 * rows; h += kMatchQueryBlock) {
      const int j = e_feat[t + (h >> 1)];
      s_rows[h] = e_desc[2 * (size_t)j + (h & 1)];
      if ((h & 1) == 0) s_j[h >> 1] = j;
    }
    __syncthreads();
    const int x1 = min(b, t + rows);
    for (int x = max(a, t); x < x1; x++) {             // ascending list position = ascending j within the node
      const uint4 u = s_rows[2 * (x - t)], v = s_rows[2 * (x - t) + 1];
      const int d = __popcll(((unsigned long long)u.y << 32 | u.x) ^ f0) + __popcll(((unsigned long long)u.w << 32 | u.z) ^ f1) +
                    __popcll(((unsigned long long)v.y << 32 | v.x) ^ f2) + __popcll(((unsigned long long)v.w << 32 | v.z) ^ f3);
      if (d < d1) { d2 = d1; d1 = d; j1 = s_j[x - t]; }   // strict: the lowest j keeps a tie
      else if (d < d2) d2 = d;
    }
  }
  d2 = min(d2, 256);
  if (j1 >= 0 && d1 <= max_distance && d1 * ratio_den <= d2 * ratio_num) {
    train_idx[(size_t)c * stride_rows + i] = j1;
    dist[(size_t)c * stride_rows + i] = d1;
    atomicMin(&keys[(size_t)c * key_stride + j1], (unsigned long long)d1 << 32 | (unsigned)i);
  }
}

// grid (query rows / 256, cap_cand)
__global__ __launch_bounds__(kBlock) void k_loop_resolve(int n_entries, int stride_rows, int key_stride, const int* __restrict__ d_entry_ids,
                                                         const int* __restrict__ d_n_cand, int cap_cand, const unsigned long long* __restrict__ keys,
                                                         int* __restrict__ train_idx, int* __restrict__ dist, int* __restrict__ n_matches) {
  const int c = blockIdx.y;
  if (c >= clamp_count(d_n_cand, cap_cand)) return;
  const int e = d_entry_ids[c];
  if (e < 0 || e >= n_entries) return;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool kept = false;
  if (i < stride_rows) {
    const int j = train_idx[(size_t)c * stride_rows + i];
    if (j >= 0) {
      kept = (int)(keys[(size_t)c * key_stride + j] & 0xffffffffu) == i;
      if (!kept) { train_idx[(size_t)c * stride_rows + i] = -1; dist[(size_t)c * stride_rows + i] = INT_MAX; }
    }
  }
  const unsigned long long bal = __ballot(kept);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&n_matches[c], __popcll(bal));
}

// frame f's points (rows f * stride_rows ... of d_xyz) become the points of entry first + f: no more rows than the entry has
__global__ __launch_bounds__(kBlock) void k_loop_set_points(int first, int stride_rows, const float* __restrict__ d_xyz, const int* __restrict__ d_n,
                                                            const long long* __restrict__ row_off, float* __restrict__ o_xyz) {
  const int f = blockIdx.x;
  const long long o = row_off[first + f], rows = row_off[first + f + 1] - o;
  const size_t n3 = 3 * (size_t)min((long long)min(max(d_n[f], 0), stride_rows), rows);
  const float* src = d_xyz + 3 * (size_t)f * stride_rows;
  for (size_t r = threadIdx.x; r < n3; r += kBlock) o_xyz[3 * o + r] = src[r];
}

}  // namespace

namespace {

dvs_status loop_reserve(dvs_loop_db* db, int more_entries, long long more_rows) {
  hipStream_t s = db->inv.voc->stream;
  const size_t ne = (size_t)db->inv.n_entries, need = ne + more_entries;
  DVS_TRY(grow_keep(db->row_off, db->cap_e_off, need + 1, ne + 1, s));
  DVS_TRY(grow_keep(db->e_nn, db->cap_e_nn, need, ne, s));
  DVS_TRY(grow_keep(db->e_m, db->cap_e_m, need, ne, s));
  if ((size_t)(db->rows_bound + more_rows) > db->cap_feat) {   // read the true count back before growing on the bound
    long long rows = 0;
    DVS_HIP(hipMemcpyAsync(&rows, db->row_off.get() + ne, sizeof(rows), hipMemcpyDeviceToHost, s));
    DVS_HIP(hipStreamSynchronize(s));
    db->rows_bound = rows;
    const size_t want = (size_t)(rows + more_rows);
    DVS_TRY(grow_keep(db->desc, db->cap_desc, 2 * want, 2 * (size_t)rows, s));
    DVS_TRY(grow_keep(db->fv_nodes, db->cap_nodes, want, (size_t)rows, s));
    DVS_TRY(grow_keep(db->fv_start, db->cap_start, want, (size_t)rows, s));
    const size_t xyz_before = db->cap_xyz;
    DVS_TRY(grow_keep(db->xyz, db->cap_xyz, 3 * want, 3 * (size_t)rows, s));
    if (db->cap_xyz != xyz_before)                // rows nobody gave points hold NaN (every byte 0xff)
      DVS_HIP(hipMemsetAsync(db->xyz.get() + 3 * (size_t)rows, 0xff, (db->cap_xyz - 3 * (size_t)rows) * sizeof(float), s));
    DVS_TRY(grow_keep(db->fv_feat, db->cap_feat, want, (size_t)rows, s));   // last: its capacity is the condition above
  }
  return DVS_OK;
}

// transform at di_levels, the BowVector to the inverted part, rows and FeatureVector to the direct index
dvs_status loop_append(dvs_loop_db* db, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes) {
  dvs_bow_vocab* v = db->inv.voc;
  const int first = db->inv.n_entries;
  DVS_TRY(loop_reserve(db, nframes, (long long)nframes * stride_rows));
  DVS_TRY(bow_db_add_device(&db->inv, d_desc, d_n, stride_rows, nframes, db->di_levels));
  hipLaunchKernelGGL(k_loop_append, dim3(nframes), dim3(kBlock), 0, v->stream, first, stride_rows, d_desc, d_n, v->o_fv_nodes.get(), v->o_fv_offsets.get(),
                     v->o_fv_features.get(), v->o_n_fv.get(), db->row_off.get(), db->e_nn.get(), db->e_m.get(), db->desc.get(), db->fv_nodes.get(),
                     db->fv_start.get(), db->fv_feat.get());
  if (hipGetLastError() != hipSuccess) {          // no entry without its direct-index rows: the inverted part steps back too
    db->inv.n_entries = first;
    set_error("dvs_loop_db_add: the direct-index append could not be launched");
    return DVS_ERR_HIP;
  }
  db->rows_bound += (long long)nframes * stride_rows;
  db->max_stride = std::max(db->max_stride, stride_rows);
  return DVS_OK;
}

dvs_status check_params(const dvs_loop_match_params* p, dvs_loop_match_params* out) {
  if (!p) { out->max_distance = 50; out->ratio_num = 3; out->ratio_den = 4; return DVS_OK; }
  if (p->max_distance < 0 || p->max_distance > 256 || p->ratio_den < 1 || p->ratio_den > 32767 || p->ratio_num < 0 || p->ratio_num > 32767) {
    set_error("match parameters max_distance=%d ratio=%d/%d: max_distance in 0..256, ratio_num in 0..32767, ratio_den in 1..32767", p->max_distance,
              p->ratio_num, p->ratio_den);
    return DVS_ERR_ARG;
  }
  *out = *p;
  return DVS_OK;
}

// the three match kernels on a query that has been transformed (at di_levels) into frame 0 of the vocabulary's own blocks
dvs_status enqueue_match(dvs_loop_db* db, const uint8_t* d_desc, int stride_rows, const int* d_entry_ids, const int* d_n_cand, int cap_cand,
                         const dvs_loop_match_params& P, int* d_train_idx, int* d_dist, int* d_n_matches) {
  if (cap_cand <= 0) return DVS_OK;
  dvs_bow_vocab* v = db->inv.voc;
  hipStream_t s = v->stream;
  const int key_stride = db->max_stride;
  if ((size_t)cap_cand * key_stride > db->cap_keys) {
    DVS_HIP(hipStreamSynchronize(s));             // an earlier match may still use the block this frees
    DVS_TRY(grow(db->keys, db->cap_keys, (size_t)cap_cand * key_stride));
  }
  const int n_entries = db->inv.n_entries;
  const int widest = std::max(std::max(stride_rows, key_stride), 1);
  hipLaunchKernelGGL(k_loop_init, dim3(std::min((widest + kBlock - 1) / kBlock, 64), cap_cand), dim3(kBlock), 0, s, n_entries, stride_rows, key_stride,
                     d_entry_ids, d_n_cand, cap_cand, d_train_idx, d_dist, d_n_matches, db->keys.get());
  if (stride_rows > 0 && n_entries > 0 && key_stride > 0) {
    const DirectIndex D{db->row_off.get(), db->e_nn.get(), db->e_m.get(), db->desc.get(), db->fv_nodes.get(), db->fv_start.get(), db->fv_feat.get()};
    hipLaunchKernelGGL(k_loop_propose, dim3((stride_rows + kMatchQueryBlock - 1) / kMatchQueryBlock, cap_cand), dim3(kMatchQueryBlock), 0, s, D, n_entries,
                       stride_rows, key_stride, d_desc, v->o_n_fv.get(), v->o_fv_offsets.get(), v->o_fv_features.get(), v->o_feat_node.get(), d_entry_ids,
                       d_n_cand, cap_cand, P.max_distance, P.ratio_num, P.ratio_den, d_train_idx, d_dist, db->keys.get());
    hipLaunchKernelGGL(k_loop_resolve, dim3((stride_rows + kBlock - 1) / kBlock, cap_cand), dim3(kBlock), 0, s, n_entries, stride_rows, key_stride,
                       d_entry_ids, d_n_cand, cap_cand, db->keys.get(), d_train_idx, d_dist, d_n_matches);
  }
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

// the host forms' output blocks: [cand][n] twice and [cand]
dvs_status host_outputs(dvs_loop_db* db, size_t cand, size_t n) {
  if (cand * n > db->cap_out_t || cand > db->cap_out_n) {
    DVS_HIP(hipStreamSynchronize(db->inv.voc->stream));
    DVS_TRY(grow(db->out_train, db->cap_out_t, cand * n));
    DVS_TRY(grow(db->out_dist, db->cap_out_d, cand * n));
    DVS_TRY(grow(db->out_n, db->cap_out_n, cand));
  }
  return DVS_OK;
}

bool frame_args_ok(const void* d_desc, const int* d_n, int stride_rows) {
  return d_n && stride_rows >= 0 && (stride_rows == 0 || d_desc) && ((uintptr_t)d_desc & 15) == 0;
}

}  // namespace

extern "C" {

dvs_status dvs_loop_match_default_params(dvs_loop_match_params* p) {
  DVS_ARG(p);
  return check_params(nullptr, p);
}

dvs_status dvs_loop_db_create(dvs_bow_vocab* voc, int32_t di_levels, dvs_loop_db** out) {
  DVS_ARG(voc && out && di_levels >= 0);
  *out = nullptr;
  DVS_HIP(hipSetDevice(voc->device));
  dvs_loop_db* db = new dvs_loop_db();
  db->di_levels = di_levels;
  dvs_status st = bow_db_init(&db->inv, voc);
  if (st == DVS_OK) st = db->row_off.alloc(65);
  if (st == DVS_OK) st = db->e_nn.alloc(64);
  if (st == DVS_OK) st = db->e_m.alloc(64);
  if (st == DVS_OK) {
    db->cap_e_off = 65; db->cap_e_nn = db->cap_e_m = 64;
    if (hipMemsetAsync(db->row_off.get(), 0, sizeof(long long), voc->stream) != hipSuccess) { set_error("dvs_loop_db_create: memset failed"); st = DVS_ERR_HIP; }
  }
  if (st != DVS_OK) { delete db; return st; }
  *out = db;
  return DVS_OK;
}

void dvs_loop_db_destroy(dvs_loop_db* db) {
  if (!db) return;
  (void)hipSetDevice(db->inv.voc->device);
  (void)hipStreamSynchronize(db->inv.voc->stream);
  delete db;
}

dvs_status dvs_loop_db_clear(dvs_loop_db* db) {
  DVS_ARG(db);
  db->inv.n_entries = 0;       // both offset blocks keep their leading 0
  db->inv.nnz_bound = 0;
  db->rows_bound = 0;
  if (db->cap_xyz) {           // the points are forgotten with the entries: every row reads as "no point" again
    DVS_HIP(hipSetDevice(db->inv.voc->device));
    DVS_HIP(hipMemsetAsync(db->xyz.get(), 0xff, db->cap_xyz * sizeof(float), db->inv.voc->stream));
  }
  return DVS_OK;
}

int32_t dvs_loop_db_size(const dvs_loop_db* db) { return db ? db->inv.n_entries : 0; }
int32_t dvs_loop_db_di_levels(const dvs_loop_db* db) { return db ? db->di_levels : -1; }

dvs_status dvs_loop_db_add_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t nframes,
                                  int32_t* first_entry_id) {
  DVS_ARG(db && nframes >= 0 && stride_rows >= 0 && (nframes == 0 || d_n) && (nframes == 0 || stride_rows == 0 || d_desc));
  DVS_ARG(((uintptr_t)d_desc & 15) == 0);
  DVS_ARG((size_t)nframes * ((size_t)stride_rows + 1) < 0x7fffffffu && (long long)db->inv.n_entries + nframes < 0x7fffffff);
  if (first_entry_id) *first_entry_id = db->inv.n_entries;
  if (nframes == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  return loop_append(db, d_desc, d_n, stride_rows, nframes);
}

dvs_status dvs_loop_db_add(dvs_loop_db* db, const uint8_t* desc, int32_t n, int32_t* entry_id) {
  DVS_ARG(db && n >= 0 && (n == 0 || desc) && db->inv.n_entries < 0x7ffffffe);
  dvs_bow_vocab* v = db->inv.voc;
  DVS_HIP(hipSetDevice(v->device));
  DVS_TRY(bow_stage_frame(v, desc, n));
  const int id = db->inv.n_entries;
  DVS_TRY(loop_append(db, v->in_desc.get(), v->in_n.get(), n, 1));
  DVS_HIP(hipStreamSynchronize(v->stream));
  if (entry_id) *entry_id = id;
  return DVS_OK;
}

dvs_status dvs_loop_db_query_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t max_results,
                                    int32_t max_id, int32_t* d_ids, double* d_scores, int32_t cap, int32_t* d_n_results) {
  DVS_ARG(db && frame_args_ok(d_desc, d_n, stride_rows) && cap >= 0 && d_n_results && max_id >= -1);
  const int limit = bow_query_limit(&db->inv, max_results, max_id);
  if (cap < limit || (limit > 0 && (!d_ids || !d_scores))) {
    set_error("dvs_loop_db_query_device: up to %d results need ids / scores of that capacity (cap %d)", limit, cap);
    return cap < limit ? DVS_ERR_CAPACITY : DVS_ERR_ARG;
  }
  if (db->inv.n_entries > 0) DVS_TRY(bow_transform_own(db->inv.voc, d_desc, d_n, stride_rows, 1, db->di_levels));
  return bow_db_query_own(&db->inv, stride_rows, max_results, max_id, d_ids, d_scores, d_n_results);
}

dvs_status dvs_loop_db_query(dvs_loop_db* db, const uint8_t* desc, int32_t n, int32_t max_results, int32_t max_id, int32_t* ids, double* scores,
                             int32_t cap, int32_t* n_results) {
  DVS_ARG(db && n >= 0 && (n == 0 || desc) && cap >= 0 && n_results && max_id >= -1);
  return bow_db_query_host(&db->inv, desc, n, max_results, max_id, db->di_levels, ids, scores, cap, n_results, "dvs_loop_db_query");
}

dvs_status dvs_loop_db_get_features(dvs_loop_db* db, int32_t id, int32_t* fv_nodes, int32_t* fv_offsets, int32_t* fv_features, int32_t cap_nodes,
                                    int32_t cap_features, int32_t* n_nodes, int32_t* n_features) {
  DVS_ARG(db && n_nodes && n_features && cap_nodes >= 0 && cap_features >= 0 && id >= 0 && id < db->inv.n_entries);
  hipStream_t s = db->inv.voc->stream;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  long long o = 0;
  int nn = 0, m = 0;
  DVS_HIP(hipMemcpyAsync(&o, db->row_off.get() + id, sizeof(o), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipMemcpyAsync(&nn, db->e_nn.get() + id, sizeof(int), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipMemcpyAsync(&m, db->e_m.get() + id, sizeof(int), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  *n_nodes = nn; *n_features = m;
  if (nn > cap_nodes || m > cap_features) {
    set_error("dvs_loop_db_get_features: entry %d has %d nodes and %d features (capacities %d, %d)", id, nn, m, cap_nodes, cap_features);
    return DVS_ERR_CAPACITY;
  }
  if (nn > 0 && fv_nodes) DVS_HIP(hipMemcpyAsync(fv_nodes, db->fv_nodes.get() + o, sizeof(int) * nn, hipMemcpyDeviceToHost, s));
  if (nn > 0 && fv_offsets) DVS_HIP(hipMemcpyAsync(fv_offsets, db->fv_start.get() + o, sizeof(int) * nn, hipMemcpyDeviceToHost, s));
  if (m > 0 && fv_features) DVS_HIP(hipMemcpyAsync(fv_features, db->fv_feat.get() + o, sizeof(int) * m, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  if (fv_offsets) fv_offsets[nn] = m;
  return DVS_OK;
}

dvs_status dvs_loop_db_get_descriptors(dvs_loop_db* db, int32_t id, uint8_t* desc, int32_t cap_rows, int32_t* n) {
  DVS_ARG(db && n && cap_rows >= 0 && id >= 0 && id < db->inv.n_entries);
  hipStream_t s = db->inv.voc->stream;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  long long be[2] = {0, 0};
  DVS_HIP(hipMemcpyAsync(be, db->row_off.get() + id, sizeof(be), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  const long long cnt = be[1] - be[0];
  *n = (int32_t)cnt;
  if (cnt > cap_rows) { set_error("dvs_loop_db_get_descriptors: entry %d has %lld rows (cap %d)", id, cnt, cap_rows); return DVS_ERR_CAPACITY; }
  if (cnt > 0 && desc) DVS_HIP(hipMemcpyAsync(desc, db->desc.get() + 2 * be[0], (size_t)cnt * 32, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  return DVS_OK;
}

dvs_status dvs_loopv_db_set_points(dvs_loop_db* db, int32_t entry_id, const float* xyz, int32_t n) {
  DVS_ARG(db && n >= 0 && (n == 0 || xyz) && entry_id >= 0 && entry_id < db->inv.n_entries);
  hipStream_t s = db->inv.voc->stream;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  long long be[2] = {0, 0};
  DVS_HIP(hipMemcpyAsync(be, db->row_off.get() + entry_id, sizeof(be), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  if (be[1] - be[0] != n) {
    set_error("dvs_loopv_db_set_points: entry %d has %lld rows, %d points given", entry_id, be[1] - be[0], n);
    return DVS_ERR_ARG;
  }
  if (n > 0) DVS_HIP(hipMemcpyAsync(db->xyz.get() + 3 * be[0], xyz, (size_t)n * 12, hipMemcpyHostToDevice, s));
  DVS_HIP(hipStreamSynchronize(s));
  return DVS_OK;
}

dvs_status dvs_loopv_db_set_points_device(dvs_loop_db* db, int32_t first_entry_id, const float* d_xyz, const int32_t* d_n, int32_t stride_rows,
                                         int32_t nframes) {
  DVS_ARG(db && nframes >= 0 && stride_rows >= 0 && (nframes == 0 || d_n) && (nframes == 0 || stride_rows == 0 || d_xyz));
  DVS_ARG(first_entry_id >= 0 && (long long)first_entry_id + nframes <= db->inv.n_entries);
  DVS_ARG((size_t)nframes * ((size_t)stride_rows + 1) < 0x7fffffffu);
  if (nframes == 0 || stride_rows == 0) return DVS_OK;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  hipLaunchKernelGGL(k_loop_set_points, dim3(nframes), dim3(kBlock), 0, db->inv.voc->stream, first_entry_id, stride_rows, d_xyz, d_n, db->row_off.get(),
                     db->xyz.get());
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status dvs_loopv_db_get_points(dvs_loop_db* db, int32_t id, float* xyz, int32_t cap_rows, int32_t* n) {
  DVS_ARG(db && n && cap_rows >= 0 && id >= 0 && id < db->inv.n_entries);
  hipStream_t s = db->inv.voc->stream;
  DVS_HIP(hipSetDevice(db->inv.voc->device));
  long long be[2] = {0, 0};
  DVS_HIP(hipMemcpyAsync(be, db->row_off.get() + id, sizeof(be), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  const long long cnt = be[1] - be[0];
  *n = (int32_t)cnt;
  if (cnt > cap_rows) { set_error("dvs_loopv_db_get_points: entry %d has %lld rows (cap %d)", id, cnt, cap_rows); return DVS_ERR_CAPACITY; }
  if (cnt > 0 && xyz) DVS_HIP(hipMemcpyAsync(xyz, db->xyz.get() + 3 * be[0], (size_t)cnt * 12, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  return DVS_OK;
}

dvs_status dvs_loop_db_match_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, const int32_t* d_entry_ids,
                                    const int32_t* d_n_cand, int32_t cap_cand, const dvs_loop_match_params* params, int32_t* d_train_idx,
                                    int32_t* d_dist, int32_t* d_n_matches) {
  DVS_ARG(db && frame_args_ok(d_desc, d_n, stride_rows) && cap_cand >= 0 && d_n_cand && (cap_cand == 0 || (d_entry_ids && d_n_matches)));
  DVS_ARG(cap_cand == 0 || stride_rows == 0 || (d_train_idx && d_dist));
  DVS_ARG((size_t)cap_cand * std::max((size_t)stride_rows, (size_t)db->max_stride) < 0x7fffffffu && cap_cand <= 65535);
  dvs_loop_match_params P;
  DVS_TRY(check_params(params, &P));
  if (cap_cand == 0) return DVS_OK;
  DVS_TRY(bow_transform_own(db->inv.voc, d_desc, d_n, stride_rows, 1, db->di_levels));
  return enqueue_match(db, d_desc, stride_rows, d_entry_ids, d_n_cand, cap_cand, P, d_train_idx, d_dist, d_n_matches);
}

dvs_status dvs_loop_db_match(dvs_loop_db* db, const uint8_t* desc, int32_t n, const int32_t* entry_ids, int32_t n_cand,
                             const dvs_loop_match_params* params, int32_t* train_idx, int32_t* dist, int32_t* n_matches) {
  DVS_ARG(db && n >= 0 && (n == 0 || desc) && n_cand >= 0 && n_cand <= 65535 && (n_cand == 0 || (entry_ids && n_matches)));
  DVS_ARG(n_cand == 0 || n == 0 || (train_idx && dist));
  DVS_ARG((size_t)n_cand * std::max((size_t)n, (size_t)db->max_stride) < 0x7fffffffu);
  dvs_loop_match_params P;
  DVS_TRY(check_params(params, &P));
  for (int c = 0; c < n_cand; c++)
    if (entry_ids[c] < 0 || entry_ids[c] >= db->inv.n_entries) {
      set_error("dvs_loop_db_match: candidate %d is entry id %d, the database holds %d entries", c, entry_ids[c], db->inv.n_entries);
      return DVS_ERR_ARG;
    }
  if (n_cand == 0) return DVS_OK;
  dvs_bow_vocab* v = db->inv.voc;
  hipStream_t s = v->stream;
  DVS_HIP(hipSetDevice(v->device));
  DVS_TRY(host_outputs(db, (size_t)n_cand, (size_t)n));
  if ((size_t)n_cand + 1 > db->cap_cand_ids) { DVS_HIP(hipStreamSynchronize(s)); DVS_TRY(grow(db->cand_ids, db->cap_cand_ids, (size_t)n_cand + 1)); }
  db->h_cand.assign(1, n_cand);
  db->h_cand.insert(db->h_cand.end(), entry_ids, entry_ids + n_cand);
  DVS_HIP(hipMemcpyAsync(db->cand_ids.get(), db->h_cand.data(), sizeof(int) * (n_cand + 1), hipMemcpyHostToDevice, s));
  DVS_TRY(bow_stage_frame(v, desc, n));
  DVS_TRY(bow_transform_own(v, v->in_desc.get(), v->in_n.get(), n, 1, db->di_levels));
  DVS_TRY(enqueue_match(db, v->in_desc.get(), n, db->cand_ids.get() + 1, db->cand_ids.get(), n_cand, P, db->out_train.get(), db->out_dist.get(),
                        db->out_n.get()));
  DVS_HIP(hipMemcpyAsync(n_matches, db->out_n.get(), sizeof(int) * n_cand, hipMemcpyDeviceToHost, s));
  if (n > 0) {
    DVS_HIP(hipMemcpyAsync(train_idx, db->out_train.get(), sizeof(int) * (size_t)n_cand * n, hipMemcpyDeviceToHost, s));
    DVS_HIP(hipMemcpyAsync(dist, db->out_dist.get(), sizeof(int) * (size_t)n_cand * n, hipMemcpyDeviceToHost, s));
  }
  DVS_HIP(hipStreamSynchronize(s));
  return DVS_OK;
}

dvs_status dvs_loop_db_detect_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t max_results,
                                     int32_t max_id, const dvs_loop_match_params* params, int32_t* d_ids, double* d_scores, int32_t* d_n_matches,
                                     int32_t* d_train_idx, int32_t* d_dist, int32_t cap, int32_t* d_n_results) {
  DVS_ARG(db && frame_args_ok(d_desc, d_n, stride_rows) && cap >= 0 && d_n_results && max_id >= -1);
  dvs_loop_match_params P;
  DVS_TRY(check_params(params, &P));
  const int limit = bow_query_limit(&db->inv, max_results, max_id);
  if (cap < limit) {
    set_error("dvs_loop_db_detect_device: up to %d results need outputs of that capacity (cap %d)", limit, cap);
    return DVS_ERR_CAPACITY;
  }
  DVS_ARG(limit == 0 || (d_ids && d_scores && d_n_matches && (stride_rows == 0 || (d_train_idx && d_dist))));
  DVS_ARG((size_t)limit * std::max((size_t)stride_rows, (size_t)db->max_stride) < 0x7fffffffu && limit <= 65535);
  DVS_TRY(bow_transform_own(db->inv.voc, d_desc, d_n, stride_rows, 1, db->di_levels));
  DVS_TRY(bow_db_query_own(&db->inv, stride_rows, max_results, max_id, d_ids, d_scores, d_n_results));
  return enqueue_match(db, d_desc, stride_rows, d_ids, d_n_results, limit, P, d_train_idx, d_dist, d_n_matches);
}

// dvs_loop_db_detect and dvs_loopv_db_detect_verify: one enqueue, one read-back; the verification (VP != NULL) reads the match where it
// lies and adds its records and masks to the same read-back
static dvs_status detect_host(dvs_loop_db* db, const uint8_t* desc, const float* xyz, int32_t n, int32_t max_results, int32_t max_id,
                              const dvs_loop_match_params* params, const dvs_loop_verify_params* VP, int32_t* ids, double* scores, int32_t* n_matches,
                              int32_t* train_idx, int32_t* dist, dvs_loop_verify_result* results, uint8_t* inlier_mask, int32_t cap, int32_t* n_results,
                              const char* what) {
  DVS_ARG(db && n >= 0 && (n == 0 || desc) && cap >= 0 && n_results && max_id >= -1);
  dvs_loop_match_params P;
  DVS_TRY(check_params(params, &P));
  const int limit = bow_query_limit(&db->inv, max_results, max_id);
  if (cap < limit) {
    set_error("%s: up to %d results need outputs of that capacity (cap %d)", what, limit, cap);
    return DVS_ERR_CAPACITY;
  }
  DVS_ARG(limit == 0 || (ids && scores && n_matches && (n == 0 || (train_idx && dist))));
  DVS_ARG((size_t)limit * std::max((size_t)n, (size_t)db->max_stride) < 0x7fffffffu && limit <= 65535);
  if (VP) DVS_ARG(limit == 0 || (results && (n == 0 || (xyz && inlier_mask))));
  *n_results = 0;
  if (limit == 0) return DVS_OK;
  dvs_bow_db* inv = &db->inv;
  dvs_bow_vocab* v = inv->voc;
  hipStream_t s = v->stream;
  DVS_HIP(hipSetDevice(v->device));
  DVS_TRY(host_outputs(db, (size_t)limit, (size_t)n));
  if (VP) {
    DVS_TRY(loop_verify_reserve(db, limit, n, VP->iterations));
    DVS_TRY(loop_verify_host_blocks(db, (size_t)limit, (size_t)n, false));
  }
  if ((size_t)limit > inv->cap_ids) {
    DVS_HIP(hipStreamSynchronize(s));
    DVS_TRY(grow(inv->ids, inv->cap_ids, (size_t)limit));
    DVS_TRY(grow(inv->scores, inv->cap_scores, (size_t)limit));
  }
  DVS_HIP(hipMemsetAsync(inv->ids.get(), 0, sizeof(int) * limit, s));          // what lies past the result count reads as zeros
  DVS_HIP(hipMemsetAsync(inv->scores.get(), 0, sizeof(double) * limit, s));
  DVS_TRY(bow_stage_frame(v, desc, n));
  if (VP && n > 0) DVS_HIP(hipMemcpyAsync(db->v_in_xyz.get(), xyz, (size_t)n * 12, hipMemcpyHostToDevice, s));
  DVS_TRY(bow_transform_own(v, v->in_desc.get(), v->in_n.get(), n, 1, db->di_levels));
  int* d_nr = inv->counters.get() + 1;
  DVS_TRY(bow_db_query_own(inv, n, max_results, max_id, inv->ids.get(), inv->scores.get(), d_nr));
  DVS_TRY(enqueue_match(db, v->in_desc.get(), n, inv->ids.get(), d_nr, limit, P, db->out_train.get(), db->out_dist.get(), db->out_n.get()));
  if (VP)
    DVS_TRY(loop_verify_enqueue(db, db->v_in_xyz.get(), v->in_n.get(), n, inv->ids.get(), d_nr, limit, db->out_train.get(), *VP, db->v_res.get(),
                                db->v_mask.get()));
  int nr = 0;
  DVS_HIP(hipMemcpyAsync(&nr, d_nr, sizeof(int), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipMemcpyAsync(ids, inv->ids.get(), sizeof(int) * limit, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipMemcpyAsync(scores, inv->scores.get(), sizeof(double) * limit, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipMemcpyAsync(n_matches, db->out_n.get(), sizeof(int) * limit, hipMemcpyDeviceToHost, s));
  if (n > 0) {
    DVS_HIP(hipMemcpyAsync(train_idx, db->out_train.get(), sizeof(int) * (size_t)limit * n, hipMemcpyDeviceToHost, s));
    DVS_HIP(hipMemcpyAsync(dist, db->out_dist.get(), sizeof(int) * (size_t)limit * n, hipMemcpyDeviceToHost, s));
  }
  if (VP) {
    DVS_HIP(hipMemcpyAsync(results, db->v_res.get(), sizeof(dvs_loop_verify_result) * limit, hipMemcpyDeviceToHost, s));
    if (n > 0) DVS_HIP(hipMemcpyAsync(inlier_mask, db->v_mask.get(), (size_t)limit * n, hipMemcpyDeviceToHost, s));
  }
  DVS_HIP(hipStreamSynchronize(s));
  *n_results = nr;
  return DVS_OK;
}

dvs_status dvs_loop_db_detect(dvs_loop_db* db, const uint8_t* desc, int32_t n, int32_t max_results, int32_t max_id,
                              const dvs_loop_match_params* params, int32_t* ids, double* scores, int32_t* n_matches, int32_t* train_idx,
                              int32_t* dist, int32_t cap, int32_t* n_results) {
  return detect_host(db, desc, nullptr, n, max_results, max_id, params, nullptr, ids, scores, n_matches, train_idx, dist, nullptr, nullptr, cap, n_results,
                     "dvs_loop_db_detect");
}

dvs_status dvs_loopv_db_detect_verify(dvs_loop_db* db, const uint8_t* desc, const float* xyz, int32_t n, int32_t max_results, int32_t max_id,
                                     const dvs_loop_match_params* match_params, const dvs_loop_verify_params* verify_params, int32_t* ids,
                                     double* scores, int32_t* n_matches, int32_t* train_idx, int32_t* dist, dvs_loop_verify_result* results,
                                     uint8_t* inlier_mask, int32_t cap, int32_t* n_results) {
  DVS_TRY(loop_verify_check_params(verify_params, "dvs_loopv_db_detect_verify"));
  return detect_host(db, desc, xyz, n, max_results, max_id, match_params, verify_params, ids, scores, n_matches, train_idx, dist, results, inlier_mask, cap,
                     n_results, "dvs_loopv_db_detect_verify");
}

}  // extern "C"
