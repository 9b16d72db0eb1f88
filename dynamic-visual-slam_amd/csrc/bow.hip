// bow.hip — place recognition: the DBoW2 vocabulary transform (OrbVocabulary) and the keyframe database (OrbDatabase) on the device.
// The semantics are the header's (include/dvslam_hip.h, "place recognition"); tests/bow_ref.py is their sequential restatement, and
// every double below is produced by the same IEEE operations in the same order as there (DESIGN.md "Place recognition"):
//   k_bow_descend   16 lanes per feature, lane c owns child c (+ 16 for k > 16); arg-min of (distance << 8 | c) over the group
//   k_bow_rank      a frame's (word, feature) and (node, feature) pairs ordered by counting: rank = pairs that compare smaller
//   k_bow_build     per frame: segment heads by a block scan, values by repeated addition, the L1 norm by ONE lane in ascending word id
//   k_db_append     a transformed frame appended to the database's CSR
//   k_db_query      a wavefront per entry: its words looked up in the query's (LDS), common terms added in ascending word id
//   k_db_select     results ordered by (raw, entry id) by counting; the first max_results written
// No atomics on doubles, no tree reductions of doubles anywhere.
#include <math.h>
#include <cmath>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "block_ops.h"
#include "common.h"
#include "device_mem.h"
#include "bow_internal.h"

namespace {
using namespace dvs;

constexpr int kGroup = 16;          // lanes per feature in the descent
constexpr int kBlock = 256;
constexpr int kQueryLdsRows = 4096; // a query of up to this many rows keeps its words in LDS (12 B each), a longer one reads them from memory

// One feature per 16-lane group.  The loop is uniform within a group (every lane of it follows the same winner), so the shuffles only
// ever read lanes that run the same iteration.
__global__ __launch_bounds__(kBlock) void k_bow_descend(VocabDev V, const uint8_t* __restrict__ d_desc, const int* __restrict__ d_n, int stride_rows,
                                                        int nid_level, int* __restrict__ feat_word, int* __restrict__ feat_node,
                                                        double* __restrict__ feat_weight) {
  const int f = blockIdx.y;
  const int n = min(max(d_n[f], 0), stride_rows);
  const int i = blockIdx.x * (kBlock / kGroup) + threadIdx.x / kGroup;
  if (i >= n) return;
  const int c = threadIdx.x % kGroup;
  const size_t o = (size_t)f * stride_rows + i;
  const uint4* row = (const uint4*)(d_desc + o * 32);
  const uint4 a = row[0], b = row[1];
  const unsigned long long f0 = (unsigned long long)a.y << 32 | a.x, f1 = (unsigned long long)a.w << 32 | a.z;
  const unsigned long long f2 = (unsigned long long)b.y << 32 | b.x, f3 = (unsigned long long)b.w << 32 | b.z;
  int cur = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
  int cnt = V.child_count[0];
  while (cnt > 0) {
    const int begin = V.child_begin[cur];
    unsigned key = 0xffffffffu;
    for (int ch = c; ch < cnt; ch += kGroup) {
      const uint4 p = V.desc[2 * (size_t)(begin + ch)], q = V.desc[2 * (size_t)(begin + ch) + 1];
      const int d = __popcll(((unsigned long long)p.y << 32 | p.x) ^ f0) + __popcll(((unsigned long long)p.w << 32 | p.z) ^ f1) +
                    __popcll(((unsigned long long)q.y << 32 | q.x) ^ f2) + __popcll(((unsigned long long)q.w << 32 | q.z) ^ f3);
      key = min(key, (unsigned)(d << 8 | ch));     // ties: the lowest child index, DBoW2's strict <
    }
    for (int m = kGroup / 2; m >= 1; m >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, m, kGroup));
    cur = begin + (int)(key & 0xff);
    if (++level == nid_level) nid = V.orig_id[cur];
    cnt = V.child_count[cur];
  }
  if (c == 0) {
    feat_word[o] = V.word_id[cur];
    feat_node[o] = nid >= 0 ? nid : V.orig_id[cur];   // a leaf above level L - levelsup: the leaf itself (deviation 1)
    feat_weight[o] = V.weight[cur];
  }
}

// rank of feature i among the frame's contributing features (weight > 0) by (word, i) and by (node, i): the number of those that
// compare smaller.  Sorted position r then holds the pair itself.
__global__ __launch_bounds__(kBlock) void k_bow_rank(const int* __restrict__ d_n, int stride_rows, const int* __restrict__ feat_word,
                                                     const int* __restrict__ feat_node, const double* __restrict__ feat_weight,
                                                     int* __restrict__ sw_word, int* __restrict__ sw_feat, int* __restrict__ sn_node,
                                                     int* __restrict__ fv_features) {
  __shared__ int s_w[kBlock], s_n[kBlock];
  const int f = blockIdx.y;
  const int n = min(max(d_n[f], 0), stride_rows);
  if (blockIdx.x * kBlock >= n) return;
  const size_t base = (size_t)f * stride_rows;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool mine = i < n && feat_weight[base + (i < n ? i : 0)] > 0.0;
  const int wi = mine ? feat_word[base + i] : 0, ni = mine ? feat_node[base + i] : 0;
  int rw = 0, rn = 0;
  for (int t = 0; t < n; t += kBlock) {
    const int j = t + threadIdx.x;
    const bool ok = j < n && feat_weight[base + (j < n ? j : 0)] > 0.0;
    __syncthreads();
    s_w[threadIdx.x] = ok ? feat_word[base + j] : -1;
    s_n[threadIdx.x] = ok ? feat_node[base + j] : -1;
    __syncthreads();
    const int m = min(kBlock, n - t);
    for (int u = 0; u < m; u++) {
      const int wj = s_w[u], nj = s_n[u], j2 = t + u;
      if (wj < 0) continue;
      rw += (wj < wi || (wj == wi && j2 < i)) ? 1 : 0;
      rn += (nj < ni || (nj == ni && j2 < i)) ? 1 : 0;
    }
  }
  if (mine) {
    sw_word[base + rw] = wi; sw_feat[base + rw] = i;
    sn_node[base + rn] = ni; fv_features[base + rn] = i;
  }
}

// heads of the runs of equal keys in sorted[0, m): keys[s] = the run's key, starts[s] = its first position, starts[count] = m
__device__ int segment_heads(const int* __restrict__ sorted, int m, int* __restrict__ keys, int* __restrict__ starts, int* s_wave) {
  int count = 0;
  for (int t = 0; t < m; t += kBlock) {
    const int r = t + threadIdx.x;
    const bool head = r < m && (r == 0 || sorted[r] != sorted[r - 1]);
    int total;
    const int s = count + block_rank256(head, s_wave, total);
    if (head) { keys[s] = sorted[r]; starts[s] = r; }
    count += total;
  }
  if (threadIdx.x == 0) starts[count] = m;
  return count;
}

// one block per frame
__global__ __launch_bounds__(kBlock) void k_bow_build(const int* __restrict__ d_n, int stride_rows, int weighting, const double* __restrict__ feat_weight,
                                                      const int* __restrict__ sw_word, const int* __restrict__ sw_feat, const int* __restrict__ sn_node,
                                                      int* __restrict__ seg_start, int* __restrict__ word_ids, double* __restrict__ word_values,
                                                      int* __restrict__ n_words, int* __restrict__ fv_nodes, int* __restrict__ fv_offsets,
                                                      int* __restrict__ n_fv_nodes) {
  __shared__ int s_wave[kBlock / 64];
  __shared__ int s_m;
  __shared__ double s_norm;
  const int f = blockIdx.x;
  const int n = min(max(d_n[f], 0), stride_rows);
  const size_t base = (size_t)f * stride_rows, base1 = (size_t)f * (stride_rows + 1);
  if (threadIdx.x == 0) s_m = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < n; i += kBlock) mine += feat_weight[base + i] > 0.0 ? 1 : 0;
  if (mine) atomicAdd(&s_m, mine);
  __syncthreads();
  const int m = s_m;
  // BowVector: one value per distinct word
  const int nw = segment_heads(sw_word + base, m, word_ids + base, seg_start + base1, s_wave);
  __syncthreads();
  for (int s = threadIdx.x; s < nw; s += kBlock) {
    const int r0 = seg_start[base1 + s], count = seg_start[base1 + s + 1] - r0;
    const double w = feat_weight[base + sw_feat[base + r0]];   // every feature of a word carries the word's weight
    double v = w;
    if (weighting == DVS_BOW_TF_IDF || weighting == DVS_BOW_TF)
      for (int c = 1; c < count; c++) v += w;                  // BowVector::addWeight once per feature: ((w + w) + w) + ...
    word_values[base + s] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {                                       // BowVector::normalize(L1): the map's order, one addition after another
    double norm = 0.0;
    for (int s = 0; s < nw; s++) norm += fabs(word_values[base + s]);
    s_norm = norm;
    n_words[f] = nw;
  }
  __syncthreads();
  const double norm = s_norm;
  if (norm > 0.0)
    for (int s = threadIdx.x; s < nw; s += kBlock) word_values[base + s] = word_values[base + s] / norm;
  // FeatureVector: CSR over the distinct nodes; the payload (fv_features) is the sorted feature list k_bow_rank wrote
  const int nn = segment_heads(sn_node + base, m, fv_nodes + base, fv_offsets + base1, s_wave);
  if (threadIdx.x == 0) n_fv_nodes[f] = nn;
}

// frame f of a transformed batch becomes entry first + f: block f copies its words behind those of the frames before it
__global__ __launch_bounds__(kBlock) void k_db_append(int first, int stride_rows, const int* __restrict__ word_ids, const double* __restrict__ word_values,
                                                      const int* __restrict__ n_words, long long* __restrict__ off, int* __restrict__ db_words,
                                                      double* __restrict__ db_values) {
  const int f = blockIdx.x;
  long long o = off[first];
  for (int g = 0; g < f; g++) o += n_words[g];
  const int n = n_words[f];
  const size_t base = (size_t)f * stride_rows;
  for (int s = threadIdx.x; s < n; s += kBlock) { db_words[o + s] = word_ids[base + s]; db_values[o + s] = word_values[base + s]; }
  if (threadIdx.x == 0) off[first + f + 1] = o + n;
}

// One wavefront per entry, the forward form of DBoW2's inverted-file walk: 64 of the entry's words at a time are looked up in the
// query's sorted words; the common ones add |q - e| - |q| - |e| to raw one after another in lane order = ascending word id.
__global__ __launch_bounds__(kBlock) void k_db_query(int n_entries, int max_id, const long long* __restrict__ off, const int* __restrict__ db_words,
                                                     const double* __restrict__ db_values, const int* __restrict__ q_words,
                                                     const double* __restrict__ q_values, const int* __restrict__ q_n, int use_lds,
                                                     double* __restrict__ raw_out, int* __restrict__ common_out, int* __restrict__ n_common_entries) {
  extern __shared__ double s_q[];                 // use_lds: qn values, then qn words
  const int qn = *q_n;
  const int* qw = q_words; const double* qv = q_values;
  if (use_lds) {
    int* s_w = (int*)(s_q + qn);
    for (int s = threadIdx.x; s < qn; s += kBlock) { s_q[s] = q_values[s]; s_w[s] = q_words[s]; }
    __syncthreads();
    qw = s_w; qv = s_q;
  }
  const int lane = threadIdx.x & 63;
  const int admissible = max_id < 0 ? n_entries : min(max_id, n_entries);
  for (int e = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < n_entries; e += gridDim.x * (kBlock / 64)) {
    double raw = 0.0;
    int common = 0;
    if (e < admissible && qn > 0) {
      const long long b = off[e], end = off[e + 1];
      const int q_last = qw[qn - 1];
      for (long long t = b; t < end; t += 64) {
        const long long r = t + lane;
        const int w = r < end ? db_words[r] : 0x7fffffff;
        if (__shfl(w, 0) > q_last) break;          // ascending: nothing further can be common
        int lo = 0, hi = qn;                        // first query word >= w
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (qw[mid] < w) lo = mid + 1; else hi = mid; }
        const bool found = r < end && lo < qn && qw[lo] == w;
        double term = 0.0;
        if (found) { const double q = qv[lo], v = db_values[r]; term = fabs(q - v) - fabs(q) - fabs(v); }
        unsigned long long mask = __ballot(found);
        common += __popcll(mask);
        while (mask) {
          const int j = __ffsll((long long)mask) - 1;
          raw += __shfl(term, j);
          mask &= mask - 1;
        }
      }
    }
    if (lane == 0) {
      raw_out[e] = raw; common_out[e] = common;
      if (common > 0) atomicAdd(n_common_entries, 1);
    }
  }
}

// entries with a common word, ordered by (raw, id) by counting; rank < limit is written.  limit <= 0: all.
__global__ __launch_bounds__(kBlock) void k_db_select(int n_entries, int limit, const double* __restrict__ raw, const int* __restrict__ common,
                                                      const int* __restrict__ n_common_entries, int* __restrict__ ids, double* __restrict__ scores,
                                                      int* __restrict__ n_results) {
  __shared__ double s_raw[kBlock];
  __shared__ int s_ok[kBlock];
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const bool mine = e < n_entries && common[e < n_entries ? e : 0] > 0;
  const double my = mine ? raw[e] : 0.0;
  int rank = 0;
  for (int t = 0; t < n_entries; t += kBlock) {
    const int j = t + threadIdx.x;
    __syncthreads();
    s_ok[threadIdx.x] = j < n_entries ? common[j] : 0;
    s_raw[threadIdx.x] = j < n_entries ? raw[j] : 0.0;
    __syncthreads();
    const int m = min(kBlock, n_entries - t);
    for (int u = 0; u < m; u++)
      if (s_ok[u] > 0 && (s_raw[u] < my || (s_raw[u] == my && t + u < e))) rank++;
  }
  if (mine && (limit <= 0 || rank < limit)) { ids[rank] = e; scores[rank] = -raw[e] / 2.0; }
  if (e == 0) n_results[0] = limit > 0 ? min(*n_common_entries, limit) : *n_common_entries;
}

// checks, then renumbers breadth-first so that every node's children are contiguous in child-list order
dvs_status build_vocab(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                       const double* weight, HostVocab* H) {
  if (k < 2 || k > DVS_BOW_MAX_K || L < 1 || L > DVS_BOW_MAX_L || weighting < 0 || weighting > 3 || scoring < 0 || scoring > 5) {
    set_error("vocabulary header k=%d L=%d scoring=%d weighting=%d: k in 2..%d, L in 1..%d, scoring in 0..5, weighting in 0..3", k, L, scoring, weighting,
              DVS_BOW_MAX_K, DVS_BOW_MAX_L);
    return DVS_ERR_ARG;
  }
  if (scoring != DVS_BOW_L1_NORM) {
    set_error("vocabulary scoring %d: only L1_NORM (0) is built", scoring);
    return DVS_ERR_UNSUPPORTED;
  }
  DVS_ARG(n >= 0 && (n == 0 || (parent && is_leaf && desc && weight)));
  const int N = n + 1;
  std::vector<int> nchild(N, 0), first(N + 1, 0);
  for (int j = 0; j < n; j++) {
    const int id = j + 1, p = parent[j];
    if (p < 0 || p >= id) { set_error("vocabulary node %d: parent id %d is not smaller than its own", id, p); return DVS_ERR_ARG; }
    if (p > 0 && is_leaf[p - 1]) { set_error("vocabulary node %d: its parent %d is marked as a leaf", id, p); return DVS_ERR_ARG; }
    if (!std::isfinite(weight[j])) { set_error("vocabulary node %d: weight is not finite", id); return DVS_ERR_ARG; }
    if (++nchild[p] > k) { set_error("vocabulary node %d has more than k = %d children", p, k); return DVS_ERR_ARG; }
  }
  for (int j = 0; j < n; j++)
    if (!is_leaf[j] && nchild[j + 1] == 0) { set_error("vocabulary node %d is not a leaf and has no children", j + 1); return DVS_ERR_ARG; }
  // child lists in file order (a counting sort by parent keeps it)
  for (int p = 0; p < N; p++) first[p + 1] = first[p] + nchild[p];
  std::vector<int> kids(n), fill(first.begin(), first.end() - 1);
  for (int j = 0; j < n; j++) kids[fill[parent[j]]++] = j + 1;
  std::vector<int> words(N, -1);
  int nw = 0;
  for (int j = 0; j < n; j++) if (is_leaf[j]) words[j + 1] = nw++;
  H->k = k; H->L = L; H->scoring = scoring; H->weighting = weighting; H->n_nodes = n; H->n_words = nw;
  H->desc.assign((size_t)N * 32, 0); H->child_begin.assign(N, 0); H->child_count.assign(N, 0); H->word_id.assign(N, -1); H->orig_id.assign(N, 0);
  H->weight.assign(N, 0.0);
  int next = 1;                                  // rows handed out so far; row r < next is a node whose own row is settled
  for (int r = 0; r < N; r++) {
    const int id = H->orig_id[r];
    H->child_begin[r] = next; H->child_count[r] = nchild[id];
    for (int c = 0; c < nchild[id]; c++) H->orig_id[next++] = kids[first[id] + c];
    if (id > 0) {
      memcpy(&H->desc[(size_t)r * 32], desc + (size_t)(id - 1) * 32, 32);
      H->weight[r] = weight[id - 1]; H->word_id[r] = words[id];
    }
  }
  return DVS_OK;
}

// the whole file in memory, then strtol / strtod token by token (ORBvoc.txt: 1.1 M lines of 35 tokens)
dvs_status parse_text(const char* path, HostVocab* H) {
  FILE* fp = fopen(path, "rb");
  if (!fp) { set_error("cannot open vocabulary file %s", path); return DVS_ERR_ARG; }
  std::string buf;
  char chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof(chunk), fp)) > 0) buf.append(chunk, got);
  fclose(fp);
  const char* p = buf.c_str();
  char* end = nullptr;
  long hdr[4];
  for (int i = 0; i < 4; i++) {
    hdr[i] = strtol(p, &end, 10);
    if (end == p) { set_error("%s: the first line must be 'k L scoring weighting'", path); return DVS_ERR_ARG; }
    p = end;
  }
  while (*p == ' ' || *p == '\t' || *p == '\r') p++;
  if (*p && *p != '\n') { set_error("%s: the first line must be 'k L scoring weighting'", path); return DVS_ERR_ARG; }
  std::vector<int32_t> parent; std::vector<uint8_t> leaf, desc; std::vector<double> weight;
  for (long line = 2;; line++) {
    while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
    if (!*p) break;
    const char* eol = strchr(p, '\n');
    if (!eol) eol = p + strlen(p);
    long v[34];
    for (int i = 0; i < 34; i++) {
      v[i] = strtol(p, &end, 10);
      if (end == p || end > eol || (*end != ' ' && *end != '\t') || (i >= 2 && (v[i] < 0 || v[i] > 255))) { set_error("%s:%ld: expected 'parent is_leaf d0 ... d31 weight'", path, line); return DVS_ERR_ARG; }
      p = end;
    }
    const double w = strtod(p, &end);
    if (end == p || end > eol) { set_error("%s:%ld: expected 'parent is_leaf d0 ... d31 weight'", path, line); return DVS_ERR_ARG; }
    p = end;
    while (*p == ' ' || *p == '\t' || *p == '\r') p++;
    if (*p && *p != '\n') { set_error("%s:%ld: more than 35 fields", path, line); return DVS_ERR_ARG; }
    if (v[0] < 0 || v[0] > 0x7ffffffe || parent.size() >= 0x7ffffff0u) { set_error("%s:%ld: parent id out of range", path, line); return DVS_ERR_ARG; }
    parent.push_back((int32_t)v[0]); leaf.push_back(v[1] > 0 ? 1 : 0); weight.push_back(w);
    for (int i = 0; i < 32; i++) desc.push_back((uint8_t)v[2 + i]);
  }
  auto small = [](long x) { return (int)std::max(-1L, std::min(x, 1000L)); };
  return build_vocab(small(hdr[0]), small(hdr[1]), small(hdr[2]), small(hdr[3]), (int)parent.size(), parent.data(), leaf.data(), desc.data(),
                     weight.data(), H);
}

// what a transform writes: caller's pointers, or the handle's own blocks where the caller passed none
struct BowOut {
  int* word_ids; double* word_values; int* n_words;
  int* fv_nodes; int* fv_offsets; int* fv_features; int* n_fv_nodes;
  int* feat_word; int* feat_node; double* feat_weight;
};

}  // namespace

namespace {

dvs_status ensure_scratch(dvs_bow_vocab* v, size_t frames, size_t rows) {
  const size_t need1 = frames * (rows + 1);
  if (need1 <= v->cap_rows && frames <= v->cap_frames) return DVS_OK;
  DVS_HIP(hipStreamSynchronize(v->stream));   // earlier work may still read the blocks this frees
  v->cap_rows = v->cap_frames = 0;
  const size_t c = need1 + need1 / 4, cf = frames + frames / 4;
  for (DeviceBuf<int>* b : {&v->sw_word, &v->sw_feat, &v->sn_node, &v->seg_start, &v->o_word_ids, &v->o_fv_nodes, &v->o_fv_offsets, &v->o_fv_features,
                            &v->o_feat_word, &v->o_feat_node})
    DVS_TRY(b->alloc(c));
  DVS_TRY(v->o_word_values.alloc(c));
  DVS_TRY(v->o_feat_weight.alloc(c));
  DVS_TRY(v->o_n_words.alloc(cf));
  DVS_TRY(v->o_n_fv.alloc(cf));
  v->cap_rows = c; v->cap_frames = cf;
  return DVS_OK;
}

BowOut own_outputs(dvs_bow_vocab* v) {
  return BowOut{v->o_word_ids.get(), v->o_word_values.get(), v->o_n_words.get(), v->o_fv_nodes.get(), v->o_fv_offsets.get(), v->o_fv_features.get(),
                v->o_n_fv.get(), v->o_feat_word.get(), v->o_feat_node.get(), v->o_feat_weight.get()};
}

// enqueues the three kernels of a transform; `o` complete (no NULLs)
dvs_status enqueue_transform(dvs_bow_vocab* v, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int levelsup, const BowOut& o) {
  if (nframes == 0) return DVS_OK;
  hipStream_t s = v->stream;
  if (stride_rows == 0 || v->H.n_nodes == 0) {   // an empty vocabulary or no rows: empty outputs
    DVS_HIP(hipMemsetAsync(o.n_words, 0, sizeof(int) * nframes, s));
    DVS_HIP(hipMemsetAsync(o.n_fv_nodes, 0, sizeof(int) * nframes, s));
    if (stride_rows == 0) DVS_HIP(hipMemsetAsync(o.fv_offsets, 0, sizeof(int) * nframes, s));
    else DVS_HIP(hipMemset2DAsync(o.fv_offsets, sizeof(int) * (stride_rows + 1), 0, sizeof(int), nframes, s));
    return DVS_OK;
  }
  const dim3 gd((stride_rows + kBlock / kGroup - 1) / (kBlock / kGroup), nframes), gr((stride_rows + kBlock - 1) / kBlock, nframes);
  hipLaunchKernelGGL(k_bow_descend, gd, dim3(kBlock), 0, s, v->V, d_desc, d_n, stride_rows, v->H.L - levelsup, o.feat_word, o.feat_node, o.feat_weight);
  hipLaunchKernelGGL(k_bow_rank, gr, dim3(kBlock), 0, s, d_n, stride_rows, o.feat_word, o.feat_node, o.feat_weight, v->sw_word.get(), v->sw_feat.get(),
                     v->sn_node.get(), o.fv_features);
  hipLaunchKernelGGL(k_bow_build, dim3(nframes), dim3(kBlock), 0, s, d_n, stride_rows, v->H.weighting, o.feat_weight, v->sw_word.get(), v->sw_feat.get(),
                     v->sn_node.get(), v->seg_start.get(), o.word_ids, o.word_values, o.n_words, o.fv_nodes, o.fv_offsets, o.n_fv_nodes);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

// one host frame into the handle's staging blocks
dvs_status stage_frame(dvs_bow_vocab* v, const uint8_t* desc, int n) {
  if ((size_t)n > v->cap_in || !v->in_n.get()) {
    DVS_HIP(hipStreamSynchronize(v->stream));
    v->cap_in = 0;
    DVS_TRY(v->in_desc.alloc((size_t)std::max(n, 256) * 32 * 2));
    v->cap_in = (size_t)std::max(n, 256) * 2;
    if (!v->in_n.get()) { DVS_TRY(v->in_n.alloc(1)); DVS_TRY(v->h_n.alloc(1)); }
  }
  if (n) DVS_HIP(hipMemcpyAsync(v->in_desc.get(), desc, (size_t)n * 32, hipMemcpyHostToDevice, v->stream));
  *v->h_n.get() = n;
  DVS_HIP(hipMemcpyAsync(v->in_n.get(), v->h_n.get(), sizeof(int), hipMemcpyHostToDevice, v->stream));
  return DVS_OK;
}

dvs_status create_vocab(int device, void* hip_stream, const HostVocab& H, dvs_bow_vocab** out) {
  DVS_TRY(check_device(device));
  dvs_bow_vocab* v = new dvs_bow_vocab();
  v->device = device; v->stream = (hipStream_t)hip_stream;
  dvs_status st = DVS_OK;
  auto up = [&](auto& buf, const auto& vec) { if (st == DVS_OK) st = buf.upload(vec); };
  up(v->desc, H.desc); up(v->child_begin, H.child_begin); up(v->child_count, H.child_count); up(v->word_id, H.word_id); up(v->orig_id, H.orig_id);
  up(v->weight, H.weight);
  if (st != DVS_OK) { delete v; return st; }
  v->V = VocabDev{(const uint4*)v->desc.get(), v->child_begin.get(), v->child_count.get(), v->word_id.get(), v->orig_id.get(), v->weight.get()};
  v->H.k = H.k; v->H.L = H.L; v->H.scoring = H.scoring; v->H.weighting = H.weighting; v->H.n_nodes = H.n_nodes; v->H.n_words = H.n_words;
  *out = v;
  return DVS_OK;
}

dvs_status db_reserve(dvs_bow_db* db, int more_entries, long long more_words) {
  dvs_bow_vocab* v = db->voc;
  const size_t ne = (size_t)db->n_entries + more_entries;
  DVS_TRY(grow_keep(db->off, db->cap_off, ne + 1, (size_t)db->n_entries + 1, v->stream));
  if ((size_t)(db->nnz_bound + more_words) > db->cap_nnz_w) {   // read the true count back before growing on the bound
    long long nnz = 0;
    DVS_HIP(hipMemcpyAsync(&nnz, db->off.get() + db->n_entries, sizeof(nnz), hipMemcpyDeviceToHost, v->stream));
    DVS_HIP(hipStreamSynchronize(v->stream));
    db->nnz_bound = nnz;
    DVS_TRY(grow_keep(db->words, db->cap_nnz_w, (size_t)(nnz + more_words), (size_t)nnz, v->stream));
    DVS_TRY(grow_keep(db->values, db->cap_nnz_v, (size_t)(nnz + more_words), (size_t)nnz, v->stream));
  }
  return DVS_OK;
}

}  // namespace

// what bow_train.hip builds on (bow_internal.h)
namespace dvs {
dvs_status bow_build_vocab(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                           const double* weight, HostVocab* H) {
  return build_vocab(k, L, scoring, weighting, n, parent, is_leaf, desc, weight, H);
}
dvs_status bow_create_vocab(int device, void* hip_stream, const HostVocab& H, dvs_bow_vocab** out) { return create_vocab(device, hip_stream, H, out); }
dvs_status bow_enqueue_descend(const VocabDev& V, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int nid_level, int* feat_word,
                               int* feat_node, double* feat_weight, hipStream_t s) {
  if (nframes <= 0 || stride_rows <= 0) return DVS_OK;
  const dim3 gd((stride_rows + kBlock / kGroup - 1) / (kBlock / kGroup), nframes);
  hipLaunchKernelGGL(k_bow_descend, gd, dim3(kBlock), 0, s, V, d_desc, d_n, stride_rows, nid_level, feat_word, feat_node, feat_weight);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status bow_db_init(dvs_bow_db* db, dvs_bow_vocab* voc) {
  db->voc = voc;
  DVS_TRY(db->off.alloc(1025));
  DVS_TRY(db->counters.alloc(2));
  DVS_HIP(hipMemsetAsync(db->off.get(), 0, sizeof(long long), voc->stream));
  db->cap_off = 1025;
  return DVS_OK;
}

dvs_status bow_stage_frame(dvs_bow_vocab* v, const uint8_t* desc, int n) { return stage_frame(v, desc, n); }

dvs_status bow_transform_own(dvs_bow_vocab* v, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int levelsup) {
  DVS_HIP(hipSetDevice(v->device));
  DVS_TRY(ensure_scratch(v, nframes, stride_rows));
  return enqueue_transform(v, d_desc, d_n, stride_rows, nframes, levelsup, own_outputs(v));
}

dvs_status bow_db_add_device(dvs_bow_db* db, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int levelsup) {
  dvs_bow_vocab* v = db->voc;
  DVS_HIP(hipSetDevice(v->device));
  DVS_TRY(ensure_scratch(v, nframes, stride_rows));
  DVS_TRY(db_reserve(db, nframes, (long long)nframes * stride_rows));
  const BowOut o = own_outputs(v);
  DVS_TRY(enqueue_transform(v, d_desc, d_n, stride_rows, nframes, levelsup, o));
  hipLaunchKernelGGL(k_db_append, dim3(nframes), dim3(kBlock), 0, v->stream, db->n_entries, stride_rows, o.word_ids, o.word_values, o.n_words, db->off.get(),
                     db->words.get(), db->values.get());
  DVS_HIP(hipGetLastError());
  db->n_entries += nframes;
  db->nnz_bound += (long long)nframes * stride_rows;
  return DVS_OK;
}

int bow_query_limit(const dvs_bow_db* db, int max_results, int max_id) {
  const int admissible = max_id < 0 ? db->n_entries : std::min(max_id, db->n_entries);
  return max_results > 0 ? std::min(max_results, admissible) : admissible;
}

// query + selection; results and their count to device memory
dvs_status bow_db_query_own(dvs_bow_db* db, int stride_rows, int max_results, int max_id, int* d_ids, double* d_scores, int* d_n_results) {
  dvs_bow_vocab* v = db->voc;
  hipStream_t s = v->stream;
  if (db->n_entries == 0) { DVS_HIP(hipMemsetAsync(d_n_results, 0, sizeof(int), s)); return DVS_OK; }
  if ((size_t)db->n_entries > db->cap_raw) {
    DVS_HIP(hipStreamSynchronize(s));
    DVS_TRY(grow(db->raw, db->cap_raw, (size_t)db->n_entries));
    DVS_TRY(grow(db->common, db->cap_common, (size_t)db->n_entries));
  }
  const BowOut o = own_outputs(v);
  DVS_HIP(hipMemsetAsync(db->counters.get(), 0, 2 * sizeof(int), s));
  const int use_lds = stride_rows <= kQueryLdsRows;
  const int blocks = std::min((db->n_entries + kBlock / 64 - 1) / (kBlock / 64), 4096);
  hipLaunchKernelGGL(k_db_query, dim3(blocks), dim3(kBlock), use_lds ? (size_t)stride_rows * 12 : 0, s, db->n_entries, max_id, db->off.get(),
                     db->words.get(), db->values.get(), o.word_ids, o.word_values, o.n_words, use_lds, db->raw.get(), db->common.get(), db->counters.get());
  hipLaunchKernelGGL(k_db_select, dim3((db->n_entries + kBlock - 1) / kBlock), dim3(kBlock), 0, s, db->n_entries, max_results > 0 ? max_results : 0,
                     db->raw.get(), db->common.get(), db->counters.get(), d_ids, d_scores, d_n_results);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status bow_db_query_host(dvs_bow_db* db, const uint8_t* desc, int n, int max_results, int max_id, int levelsup, int* ids, double* scores, int cap,
                             int* n_results, const char* what) {
  const int limit = bow_query_limit(db, max_results, max_id);
  if (cap < limit || (limit > 0 && (!ids || !scores))) {
    set_error("%s: up to %d results need ids / scores of that capacity (cap %d)", what, limit, cap);
    return cap < limit ? DVS_ERR_CAPACITY : DVS_ERR_ARG;
  }
  *n_results = 0;
  if (limit == 0) return DVS_OK;
  dvs_bow_vocab* v = db->voc;
  hipStream_t s = v->stream;
  DVS_HIP(hipSetDevice(v->device));
  if ((size_t)limit > db->cap_ids) {
    DVS_HIP(hipStreamSynchronize(s));
    DVS_TRY(grow(db->ids, db->cap_ids, (size_t)limit));
    DVS_TRY(grow(db->scores, db->cap_scores, (size_t)limit));
  }
  DVS_TRY(stage_frame(v, desc, n));
  DVS_TRY(bow_transform_own(v, v->in_desc.get(), v->in_n.get(), n, 1, levelsup));
  DVS_TRY(bow_db_query_own(db, n, max_results, max_id, db->ids.get(), db->scores.get(), db->counters.get() + 1));
  int nr = 0;
  DVS_HIP(hipMemcpyAsync(&nr, db->counters.get() + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  if (nr > 0) {
    DVS_HIP(hipMemcpyAsync(ids, db->ids.get(), sizeof(int) * nr, hipMemcpyDeviceToHost, s));
    DVS_HIP(hipMemcpyAsync(scores, db->scores.get(), sizeof(double) * nr, hipMemcpyDeviceToHost, s));
    DVS_HIP(hipStreamSynchronize(s));
  }
  *n_results = nr;
  return DVS_OK;
}
}  // namespace dvs

extern "C" {

dvs_status dvs_bow_vocab_load_text(int32_t device, void* hip_stream, const char* path, dvs_bow_vocab** out) {
  DVS_ARG(path && out);
  *out = nullptr;
  HostVocab H;
  DVS_TRY(parse_text(path, &H));
  return create_vocab(device, hip_stream, H, out);
}

dvs_status dvs_bow_vocab_from_arrays(int32_t device, void* hip_stream, int32_t k, int32_t L, int32_t scoring, int32_t weighting, int32_t n_nodes,
                                     const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc, const double* weight, dvs_bow_vocab** out) {
  DVS_ARG(out);
  *out = nullptr;
  HostVocab H;
  DVS_TRY(build_vocab(k, L, scoring, weighting, n_nodes, parent, is_leaf, desc, weight, &H));
  return create_vocab(device, hip_stream, H, out);
}

void dvs_bow_vocab_destroy(dvs_bow_vocab* voc) {
  if (!voc) return;
  (void)hipSetDevice(voc->device);
  (void)hipStreamSynchronize(voc->stream);
  delete voc;
}

dvs_status dvs_bow_vocab_info(const dvs_bow_vocab* voc, int32_t* k, int32_t* L, int32_t* scoring, int32_t* weighting, int32_t* n_nodes, int32_t* n_words) {
  DVS_ARG(voc);
  if (k) *k = voc->H.k;
  if (L) *L = voc->H.L;
  if (scoring) *scoring = voc->H.scoring;
  if (weighting) *weighting = voc->H.weighting;
  if (n_nodes) *n_nodes = voc->H.n_nodes;
  if (n_words) *n_words = voc->H.n_words;
  return DVS_OK;
}

dvs_status dvs_bow_vocab_synchronize(dvs_bow_vocab* voc) {
  DVS_ARG(voc);
  DVS_HIP(hipSetDevice(voc->device));
  DVS_HIP(hipStreamSynchronize(voc->stream));
  return DVS_OK;
}

dvs_status dvs_bow_transform_batch_device(dvs_bow_vocab* voc, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t nframes,
                                          int32_t levelsup, int32_t* d_word_ids, double* d_word_values, int32_t* d_n_words, int32_t* d_fv_nodes,
                                          int32_t* d_fv_offsets, int32_t* d_fv_features, int32_t* d_n_fv_nodes, int32_t* d_feat_word,
                                          int32_t* d_feat_node, double* d_feat_weight) {
  DVS_ARG(voc && nframes >= 0 && stride_rows >= 0 && (nframes == 0 || d_n) && (nframes == 0 || stride_rows == 0 || d_desc));
  DVS_ARG(((uintptr_t)d_desc & 15) == 0);
  DVS_ARG((size_t)nframes * ((size_t)stride_rows + 1) < 0x7fffffffu);
  DVS_HIP(hipSetDevice(voc->device));
  DVS_TRY(ensure_scratch(voc, nframes, stride_rows));
  BowOut o = own_outputs(voc);
  if (d_word_ids) o.word_ids = d_word_ids;
  if (d_word_values) o.word_values = d_word_values;
  if (d_n_words) o.n_words = d_n_words;
  if (d_fv_nodes) o.fv_nodes = d_fv_nodes;
  if (d_fv_offsets) o.fv_offsets = d_fv_offsets;
  if (d_fv_features) o.fv_features = d_fv_features;
  if (d_n_fv_nodes) o.n_fv_nodes = d_n_fv_nodes;
  if (d_feat_word) o.feat_word = d_feat_word;
  if (d_feat_node) o.feat_node = d_feat_node;
  if (d_feat_weight) o.feat_weight = d_feat_weight;
  return enqueue_transform(voc, d_desc, d_n, stride_rows, nframes, levelsup, o);
}

dvs_status dvs_bow_transform(dvs_bow_vocab* voc, const uint8_t* desc, int32_t n, int32_t levelsup, int32_t* word_ids, double* word_values,
                             int32_t cap_words, int32_t* n_words, int32_t* fv_nodes, int32_t* fv_offsets, int32_t* fv_features, int32_t cap_fv,
                             int32_t* n_fv_nodes, int32_t* feat_word, int32_t* feat_node, double* feat_weight) {
  DVS_ARG(voc && n >= 0 && (n == 0 || desc) && cap_words >= 0 && cap_fv >= 0);
  DVS_ARG((word_ids || word_values) ? n_words != nullptr : true);
  DVS_ARG((fv_nodes || fv_offsets || fv_features) ? n_fv_nodes != nullptr : true);
  if (((word_ids || word_values) && cap_words < n) || ((fv_nodes || fv_offsets || fv_features) && cap_fv < n)) {
    set_error("dvs_bow_transform: %d features need capacities of at least %d (cap_words %d, cap_fv %d)", n, n, cap_words, cap_fv);
    return DVS_ERR_CAPACITY;
  }
  DVS_HIP(hipSetDevice(voc->device));
  DVS_TRY(stage_frame(voc, desc, n));
  DVS_TRY(ensure_scratch(voc, 1, n));
  const BowOut o = own_outputs(voc);
  DVS_TRY(enqueue_transform(voc, voc->in_desc.get(), voc->in_n.get(), n, 1, levelsup, o));
  hipStream_t s = voc->stream;
  int nw = 0, nn = 0;
  DVS_HIP(hipMemcpyAsync(&nw, o.n_words, sizeof(int), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipMemcpyAsync(&nn, o.n_fv_nodes, sizeof(int), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  if (n_words) *n_words = nw;
  if (n_fv_nodes) *n_fv_nodes = nn;
  auto back = [&](void* dst, const void* src, size_t bytes) -> hipError_t { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
  DVS_HIP(back(word_ids, o.word_ids, sizeof(int) * nw));
  DVS_HIP(back(word_values, o.word_values, sizeof(double) * nw));
  DVS_HIP(back(fv_nodes, o.fv_nodes, sizeof(int) * nn));
  DVS_HIP(back(fv_offsets, o.fv_offsets, sizeof(int) * (nn + 1)));
  if (fv_features && nn) {
    int m = 0;
    DVS_HIP(hipMemcpyAsync(&m, o.fv_offsets + nn, sizeof(int), hipMemcpyDeviceToHost, s));
    DVS_HIP(hipStreamSynchronize(s));
    DVS_HIP(back(fv_features, o.fv_features, sizeof(int) * m));
  }
  const bool any = n > 0 && voc->H.n_nodes > 0;
  DVS_HIP(back(feat_word, o.feat_word, any ? sizeof(int) * n : 0));
  DVS_HIP(back(feat_node, o.feat_node, any ? sizeof(int) * n : 0));
  DVS_HIP(back(feat_weight, o.feat_weight, any ? sizeof(double) * n : 0));
  DVS_HIP(hipStreamSynchronize(s));
  if (!any && n > 0) {   // an empty vocabulary has no word: DBoW2 returns before the descent
    for (int i = 0; i < n; i++) { if (feat_word) feat_word[i] = -1; if (feat_node) feat_node[i] = 0; if (feat_weight) feat_weight[i] = 0.0; }
  }
  return DVS_OK;
}

dvs_status dvs_bow_db_create(dvs_bow_vocab* voc, dvs_bow_db** out) {
  DVS_ARG(voc && out);
  *out = nullptr;
  DVS_HIP(hipSetDevice(voc->device));
  dvs_bow_db* db = new dvs_bow_db();
  const dvs_status st = bow_db_init(db, voc);
  if (st != DVS_OK) { delete db; return st; }
  *out = db;
  return DVS_OK;
}

void dvs_bow_db_destroy(dvs_bow_db* db) {
  if (!db) return;
  (void)hipSetDevice(db->voc->device);
  (void)hipStreamSynchronize(db->voc->stream);
  delete db;
}

dvs_status dvs_bow_db_clear(dvs_bow_db* db) {
  DVS_ARG(db);
  db->n_entries = 0;       // offsets[0] stays 0: the blocks keep their size
  db->nnz_bound = 0;
  return DVS_OK;
}

int32_t dvs_bow_db_size(const dvs_bow_db* db) { return db ? db->n_entries : 0; }

dvs_status dvs_bow_db_add_device(dvs_bow_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t nframes,
                                 int32_t* first_entry_id_out) {
  DVS_ARG(db && nframes >= 0 && stride_rows >= 0 && (nframes == 0 || d_n) && (nframes == 0 || stride_rows == 0 || d_desc));
  DVS_ARG(((uintptr_t)d_desc & 15) == 0);
  DVS_ARG((size_t)nframes * ((size_t)stride_rows + 1) < 0x7fffffffu && (long long)db->n_entries + nframes < 0x7fffffff);
  if (first_entry_id_out) *first_entry_id_out = db->n_entries;
  if (nframes == 0) return DVS_OK;
  return bow_db_add_device(db, d_desc, d_n, stride_rows, nframes, 0);
}

dvs_status dvs_bow_db_add(dvs_bow_db* db, const uint8_t* desc, int32_t n, int32_t* entry_id) {
  DVS_ARG(db && n >= 0 && (n == 0 || desc) && db->n_entries < 0x7ffffffe);
  dvs_bow_vocab* v = db->voc;
  DVS_HIP(hipSetDevice(v->device));
  DVS_TRY(stage_frame(v, desc, n));
  const int id = db->n_entries;
  DVS_TRY(bow_db_add_device(db, v->in_desc.get(), v->in_n.get(), n, 1, 0));
  DVS_HIP(hipStreamSynchronize(v->stream));
  if (entry_id) *entry_id = id;
  return DVS_OK;
}

dvs_status dvs_bow_db_query_device(dvs_bow_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t max_results,
                                   int32_t max_id, int32_t* d_ids, double* d_scores, int32_t cap, int32_t* d_n_results) {
  DVS_ARG(db && d_n && stride_rows >= 0 && (stride_rows == 0 || d_desc) && cap >= 0 && d_n_results && max_id >= -1);
  DVS_ARG(((uintptr_t)d_desc & 15) == 0);
  const int limit = bow_query_limit(db, max_results, max_id);
  if (cap < limit || (limit > 0 && (!d_ids || !d_scores))) {
    set_error("dvs_bow_db_query_device: up to %d results need ids / scores of that capacity (cap %d)", limit, cap);
    return cap < limit ? DVS_ERR_CAPACITY : DVS_ERR_ARG;
  }
  if (db->n_entries > 0) DVS_TRY(bow_transform_own(db->voc, d_desc, d_n, stride_rows, 1, 0));   // an empty database: the count alone
  return bow_db_query_own(db, stride_rows, max_results, max_id, d_ids, d_scores, d_n_results);
}

dvs_status dvs_bow_db_query(dvs_bow_db* db, const uint8_t* desc, int32_t n, int32_t max_results, int32_t max_id, int32_t* ids, double* scores,
                            int32_t cap, int32_t* n_results) {
  DVS_ARG(db && n >= 0 && (n == 0 || desc) && cap >= 0 && n_results && max_id >= -1);
  return bow_db_query_host(db, desc, n, max_results, max_id, 0, ids, scores, cap, n_results, "dvs_bow_db_query");
}

dvs_status dvs_bow_db_get_entry(dvs_bow_db* db, int32_t id, int32_t* word_ids, double* word_values, int32_t cap, int32_t* n) {
  DVS_ARG(db && n && cap >= 0 && id >= 0 && id < db->n_entries);
  hipStream_t s = db->voc->stream;
  DVS_HIP(hipSetDevice(db->voc->device));
  long long be[2] = {0, 0};
  DVS_HIP(hipMemcpyAsync(be, db->off.get() + id, sizeof(be), hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  const long long cnt = be[1] - be[0];
  *n = (int32_t)cnt;
  if (cnt > cap) { set_error("dvs_bow_db_get_entry: entry %d has %lld words (cap %d)", id, cnt, cap); return DVS_ERR_CAPACITY; }
  if (cnt > 0 && word_ids) DVS_HIP(hipMemcpyAsync(word_ids, db->words.get() + be[0], sizeof(int) * cnt, hipMemcpyDeviceToHost, s));
  if (cnt > 0 && word_values) DVS_HIP(hipMemcpyAsync(word_values, db->values.get() + be[0], sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
  DVS_HIP(hipStreamSynchronize(s));
  return DVS_OK;
}

}  // extern "C"
