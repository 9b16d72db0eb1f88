// bow_train.hip — OrbVocabulary::create on the device: DBoW2's hierarchical k-means (HKmeansStep, initiateClustersKMpp, FORB::meanValue,
// setNodeWeights) over 32-byte descriptors.  The semantics are the header's (include/dvslam_hip.h, "vocabulary training");
// tests/bow_train_ref.py is their recursive, depth-first restatement, and the result equals it bit for bit: every quantity below is an
// integer, the only doubles are the final log() of the weights, taken on the host from device-counted integers.
//
// The tree is processed level by level: all nodes of one depth are the segments of one index permutation `perm`, and
// every stage runs over all of them at once.  A node that has converged is at a fixed point (its centres are the means of its groups,
// its groups the nearest centres), so further passes leave it as it is: the level runs until no node changed or the cap is reached.
//   k_seed_*        k-means++: min_dist update, ONE 64-bit prefix sum over the whole level (k_scan_*), a binary search per node for `cut`
//   k_assoc         a thread per feature: Hamming distance to its node's <= 32 centres, arg-min of (distance << 8 | c)
//   k_mean_small    nodes of up to kSmallNode features: a 32-lane group per node, lane = descriptor byte
//   k_counts_big    larger nodes: a workgroup per kChunkRows features, thread = descriptor bit, counters in LDS, integer atomics to memory
//   k_mean_big      the majority threshold over those counters
//   k_flag/k_scatter  the stable partition into the next level's segments, once per level: rank within a cluster = prefix sum of its flag
// Integer atomics only (sums, equal-valued stores): nothing depends on launch geometry or timing.  Per level the host reads the tree's new
// nodes; per batch of passes one convergence word.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "block_ops.h"
#include "common.h"
#include "device_mem.h"
#include "bow_internal.h"
#include "splitmix64.h"

namespace {
using namespace dvs;

constexpr int kBlock = 256;
constexpr int kScanChunk = kBlock * 4;   // elements per workgroup of the prefix sum
constexpr int kSmallNode = 256;          // up to this many features a 32-lane group computes a node's means
constexpr int kChunkRows = 512;          // features per workgroup of k_counts_big
constexpr int kPassBatch = 4;            // association passes enqueued between two reads of the convergence word
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;

struct LevelDev {
  const uint4* feat;             // [N][2] all training features, image order
  int P, M, k;                   // positions and nodes of this level
  const int* perm;               // [P] feature index, grouped by node, ascending position within the parent's list
  const int* fnode;              // [P] node of the position
  const int* seg;                // [M + 1] first position of node m
  const int* cbase;              // [M + 1] first centre slot of node m (min(k, size) slots each)
  const unsigned long long* key; // [M] sampler key
  uint4* centre;                 // [slots][2]
  int* nc;                       // [M] centres of node m
  uint8_t* done;                 // [M] seeding finished
  uint8_t* assoc;                // [P] cluster of the position
  int* min_dist;                 // [P]
  int* vals;                     // [P] what the prefix sum adds
  long long* G;                  // [P] inclusive prefix sum of vals
  int* last_changed;             // [M] last pass in which an association of the node changed (pass 1 counts; 0: trivial node)
  int* changed;                  // [kPassBatch] 1 if any association changed in that pass of the batch
};

__device__ __forceinline__ int ham(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popcll(((unsigned long long)(a0.y ^ b0.y) << 32) | (a0.x ^ b0.x)) + __popcll(((unsigned long long)(a0.w ^ b0.w) << 32) | (a0.z ^ b0.z)) +
         __popcll(((unsigned long long)(a1.y ^ b1.y) << 32) | (a1.x ^ b1.x)) + __popcll(((unsigned long long)(a1.w ^ b1.w) << 32) | (a1.z ^ b1.z));
}

__global__ __launch_bounds__(kBlock) void k_iota(int* __restrict__ perm, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) perm[i] = i;
}

// frames in batch layout -> one contiguous block in frame order; off[f] = features before frame f (host-clamped counts)
__global__ __launch_bounds__(kBlock) void k_compact(const uint4* __restrict__ src, int stride_rows, const int* __restrict__ off, uint4* __restrict__ feat) {
  const int f = blockIdx.y;
  const int n = off[f + 1] - off[f];
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j < 2 * n) feat[2 * (size_t)off[f] + j] = src[2 * (size_t)f * stride_rows + j];
}

// ---------------------------------------------------------------- 64-bit inclusive prefix sum of vals[0, P)
__global__ __launch_bounds__(kBlock) void k_scan_partial(const int* __restrict__ vals, int P, long long* __restrict__ bsum) {
  __shared__ long long sh[kBlock];
  const int base = blockIdx.x * kScanChunk + threadIdx.x * 4;
  long long s = 0;
  for (int i = 0; i < 4; i++) if (base + i < P) s += vals[base + i];
  s = block_sum<kBlock>(s, sh);
  if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// inclusive scan of one value per thread of the workgroup
__device__ long long block_scan_incl(long long v, long long* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    const long long x = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    sh[threadIdx.x] += x;
    __syncthreads();
  }
  return sh[threadIdx.x];
}

// one workgroup: bsum becomes its own exclusive scan
__global__ __launch_bounds__(kBlock) void k_scan_bsums(long long* __restrict__ bsum, int nb) {
  __shared__ long long sh[kBlock];
  long long carry = 0;
  for (int t0 = 0; t0 < nb; t0 += kBlock) {
    const int i = t0 + threadIdx.x;
    const long long v = i < nb ? bsum[i] : 0;
    const long long incl = block_scan_incl(v, sh);
    const long long total = sh[kBlock - 1];
    if (i < nb) bsum[i] = carry + incl - v;
    carry += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void k_scan_final(const int* __restrict__ vals, int P, const long long* __restrict__ bsum, long long* __restrict__ G) {
  __shared__ long long sh[kBlock];
  const int base = blockIdx.x * kScanChunk + threadIdx.x * 4;
  int v[4];
  long long s = 0;
  for (int i = 0; i < 4; i++) { v[i] = base + i < P ? vals[base + i] : 0; s += v[i]; }
  long long run = block_scan_incl(s, sh) - s + bsum[blockIdx.x];
  for (int i = 0; i < 4; i++) { run += v[i]; if (base + i < P) G[base + i] = run; }
}

// ---------------------------------------------------------------- a level's start and k-means++ seeding
__global__ __launch_bounds__(kBlock) void k_level_init(LevelDev Lv) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= Lv.P) return;
  const int m = Lv.fnode[p], b = Lv.seg[m], size = Lv.seg[m + 1] - b;
  Lv.assoc[p] = size <= Lv.k ? (uint8_t)(p - b) : (uint8_t)0xff;   // the trivial case: one cluster per feature, in order
}

__global__ __launch_bounds__(kBlock) void k_seed_init(LevelDev Lv) {
  const int m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= Lv.M) return;
  const int b = Lv.seg[m], size = Lv.seg[m + 1] - b, cb = Lv.cbase[m];
  if (size <= Lv.k) {
    for (int i = 0; i < size; i++) {
      const int row = Lv.perm[b + i];
      Lv.centre[2 * (size_t)(cb + i)] = Lv.feat[2 * (size_t)row];
      Lv.centre[2 * (size_t)(cb + i) + 1] = Lv.feat[2 * (size_t)row + 1];
    }
    Lv.nc[m] = size; Lv.done[m] = 1; Lv.last_changed[m] = 0;
    return;
  }
  const int pos = (int)(splitmix64(Lv.key[m]) % (unsigned long long)size);   // draw 0
  const int row = Lv.perm[b + pos];
  Lv.centre[2 * (size_t)cb] = Lv.feat[2 * (size_t)row];
  Lv.centre[2 * (size_t)cb + 1] = Lv.feat[2 * (size_t)row + 1];
  Lv.nc[m] = 1; Lv.done[m] = 0; Lv.last_changed[m] = 1;
}

// round r (1 .. k - 1): distance to the centre picked last; vals = min_dist of the nodes still seeding, 0 elsewhere
__global__ __launch_bounds__(kBlock) void k_seed_update(LevelDev Lv, int r) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= Lv.P) return;
  const int m = Lv.fnode[p], size = Lv.seg[m + 1] - Lv.seg[m];
  int v = 0;
  if (size > Lv.k && !Lv.done[m]) {
    const int row = Lv.perm[p];
    const size_t c = (size_t)(Lv.cbase[m] + r - 1);
    const int d = ham(Lv.feat[2 * (size_t)row], Lv.feat[2 * (size_t)row + 1], Lv.centre[2 * c], Lv.centre[2 * c + 1]);
    v = r == 1 ? d : min(Lv.min_dist[p], d);
    Lv.min_dist[p] = v;
  }
  Lv.vals[p] = v;
}

// round r: S = the node's sum; S == 0 ends its seeding short; else the first position whose inclusive prefix sum reaches cut
__global__ __launch_bounds__(kBlock) void k_seed_pick(LevelDev Lv, int r) {
  const int m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= Lv.M) return;
  const int b = Lv.seg[m], size = Lv.seg[m + 1] - b;
  if (size <= Lv.k || Lv.done[m]) return;
  const long long before = b > 0 ? Lv.G[b - 1] : 0;
  const long long S = Lv.G[b + size - 1] - before;
  if (S == 0) { Lv.done[m] = 1; return; }
  const long long cut = 1 + (long long)(splitmix64(Lv.key[m] + (unsigned long long)r * kGolden) % (unsigned long long)S);
  const long long target = before + cut;
  int lo = b, hi = b + size - 1;              // G[hi] >= target always
  while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (Lv.G[mid] >= target) hi = mid; else lo = mid + 1; }
  const int row = Lv.perm[lo];
  const size_t c = (size_t)(Lv.cbase[m] + r);
  Lv.centre[2 * c] = Lv.feat[2 * (size_t)row];
  Lv.centre[2 * c + 1] = Lv.feat[2 * (size_t)row + 1];
  Lv.nc[m] = r + 1;
  if (r + 1 == Lv.k) Lv.done[m] = 1;
}

// ---------------------------------------------------------------- association
// slot: this pass's word of Lv.changed
__global__ __launch_bounds__(kBlock) void k_assoc(LevelDev Lv, int pass, int slot) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= Lv.P) return;
  const int m = Lv.fnode[p], size = Lv.seg[m + 1] - Lv.seg[m];
  if (size <= Lv.k) return;
  const int row = Lv.perm[p];
  const uint4 f0 = Lv.feat[2 * (size_t)row], f1 = Lv.feat[2 * (size_t)row + 1];
  const int cb = Lv.cbase[m], n = Lv.nc[m];
  unsigned key = 0xffffffffu;
  for (int c = 0; c < n; c++) {
    const int d = ham(f0, f1, Lv.centre[2 * (size_t)(cb + c)], Lv.centre[2 * (size_t)(cb + c) + 1]);
    key = min(key, (unsigned)(d << 8 | c));     // ties: the first centre, DBoW2's strict <
  }
  const uint8_t a = (uint8_t)(key & 0xff);
  if (pass >= 2 && a != Lv.assoc[p]) { Lv.last_changed[m] = pass; Lv.changed[slot] = 1; }   // every writer stores the same value
  Lv.assoc[p] = a;
}

// ---------------------------------------------------------------- means: bit b set iff at least N/2 + N%2 members have it; an empty cluster keeps its centre
// 32 lanes per node of the list, lane = descriptor byte
__global__ __launch_bounds__(kBlock) void k_mean_small(LevelDev Lv, const int* __restrict__ small, int nsmall) {
  const int g = blockIdx.x * (kBlock / 32) + threadIdx.x / 32;
  if (g >= nsmall) return;
  const int lane = threadIdx.x & 31;
  const int m = small[g], b = Lv.seg[m], e = Lv.seg[m + 1], cb = Lv.cbase[m], n = Lv.nc[m];
  const uint8_t* feat = (const uint8_t*)Lv.feat;
  uint8_t* centre = (uint8_t*)Lv.centre;
  for (int c = 0; c < n; c++) {
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, members = 0;
    for (int p = b; p < e; p++) {
      if (Lv.assoc[p] != c) continue;
      const unsigned v = feat[(size_t)Lv.perm[p] * 32 + lane];
#pragma unroll
      for (int bit = 0; bit < 8; bit++) cnt[bit] += (v >> bit) & 1;
      members++;
    }
    if (members == 0) continue;
    const int thr = members / 2 + members % 2;
    unsigned out = 0;
#pragma unroll
    for (int bit = 0; bit < 8; bit++) out |= (cnt[bit] >= thr ? 1u : 0u) << bit;
    centre[(size_t)(cb + c) * 32 + lane] = (uint8_t)out;
  }
}

// chunk = (node, first position, end position, index of the node among the big ones); thread = descriptor bit, its own LDS column
__global__ __launch_bounds__(kBlock) void k_counts_big(LevelDev Lv, const int4* __restrict__ chunks, int* __restrict__ bigcnt, int* __restrict__ bign) {
  extern __shared__ int s_dyn[];                // [k][256] bit counters, [k] members
  __shared__ uint4 s_rows[kChunkRows * 2];
  __shared__ uint8_t s_assoc[kChunkRows];
  const int4 ch = chunks[blockIdx.x];
  const int m = ch.x, a = ch.y, rows = ch.z - ch.y, big = ch.w;
  const int n = Lv.nc[m], t = threadIdx.x;
  int* s_cnt = s_dyn;
  int* s_n = s_dyn + Lv.k * 256;
  for (int c = 0; c < n; c++) s_cnt[c * 256 + t] = 0;
  if (t < n) s_n[t] = 0;
  for (int j = t; j < 2 * rows; j += kBlock) s_rows[j] = Lv.feat[2 * (size_t)Lv.perm[a + (j >> 1)] + (j & 1)];
  for (int j = t; j < rows; j += kBlock) s_assoc[j] = Lv.assoc[a + j];
  __syncthreads();
  const uint8_t* bytes = (const uint8_t*)s_rows;
  const int byte = t >> 3, bit = t & 7;
  for (int i = 0; i < rows; i++) {
    const int c = s_assoc[i];
    if (c >= n) continue;
    s_cnt[c * 256 + t] += (bytes[i * 32 + byte] >> bit) & 1;
    if (t == 0) s_n[c]++;
  }
  __syncthreads();
  for (int c = 0; c < n; c++) {
    const int v = s_cnt[c * 256 + t];
    if (v) atomicAdd(&bigcnt[((size_t)big * Lv.k + c) * 256 + t], v);
  }
  if (t < n && s_n[t]) atomicAdd(&bign[big * Lv.k + t], s_n[t]);
}

// a thread per (big node, cluster, byte)
__global__ __launch_bounds__(kBlock) void k_mean_big(LevelDev Lv, const int* __restrict__ bignode, int nbig, const int* __restrict__ bigcnt,
                                                     const int* __restrict__ bign) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long long)nbig * Lv.k * 32) return;
  const int byte = (int)(i & 31), c = (int)((i >> 5) % Lv.k), big = (int)((i >> 5) / Lv.k);
  const int m = bignode[big];
  if (c >= Lv.nc[m]) return;
  const int members = bign[big * Lv.k + c];
  if (members == 0) return;
  const int thr = members / 2 + members % 2;
  const int* cnt = bigcnt + ((size_t)big * Lv.k + c) * 256 + byte * 8;
  unsigned out = 0;
  for (int bit = 0; bit < 8; bit++) out |= (cnt[bit] >= thr ? 1u : 0u) << bit;
  ((uint8_t*)Lv.centre)[(size_t)(Lv.cbase[m] + c) * 32 + byte] = (uint8_t)out;
}

// ---------------------------------------------------------------- the level's end: cluster sizes, stable partition into the next level
__global__ __launch_bounds__(kBlock) void k_csize(LevelDev Lv, int* __restrict__ csize) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= Lv.P) return;
  const int m = Lv.fnode[p], a = Lv.assoc[p];
  if (a < Lv.nc[m]) atomicAdd(&csize[Lv.cbase[m] + a], 1);
}

__global__ __launch_bounds__(kBlock) void k_flag(LevelDev Lv, int c) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p < Lv.P) Lv.vals[p] = Lv.assoc[p] == c ? 1 : 0;
}

// members of cluster c of every node: to dst[slot] + (members of the same cluster before it in the node); dst < 0: not carried on
__global__ __launch_bounds__(kBlock) void k_scatter(LevelDev Lv, int c, const int* __restrict__ dst, const int* __restrict__ dstnode, int next_P,
                                                    int* __restrict__ next_perm, int* __restrict__ next_fnode) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= Lv.P || Lv.assoc[p] != c) return;
  const int m = Lv.fnode[p], b = Lv.seg[m], slot = Lv.cbase[m] + c;
  const int d = dst[slot];
  if (d < 0) return;
  const long long rank = Lv.G[p] - (b > 0 ? Lv.G[b - 1] : 0) - 1;
  const long long q = d + rank;
  if (q < 0 || q >= next_P) return;
  next_perm[q] = Lv.perm[p];
  next_fnode[q] = dstnode[slot];
}

// one image's features: a word counts the image once (stamp = image index + 1, ascending from launch to launch)
__global__ __launch_bounds__(kBlock) void k_ni_count(const int* __restrict__ feat_word, int n, int n_words, int stamp_value, int* __restrict__ stamp,
                                                     int* __restrict__ Ni) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int w = feat_word[i];
  if (w < 0 || w >= n_words) return;
  if (atomicMax(&stamp[w], stamp_value) < stamp_value) atomicAdd(&Ni[w], 1);
}

inline int blocks_for(long long n) { return (int)((n + kBlock - 1) / kBlock); }

struct HNode { int begin, size; unsigned long long key; int tree; };

struct Trainer {
  int device = 0;
  hipStream_t s = nullptr;
  dvs_voc_train_params prm{};
  int N = 0, nimages = 0;
  std::vector<int> img_off;                       // [nimages + 1]
  DeviceBuf<uint4> feat, centre;
  DeviceBuf<int> perm_a, perm_b, fnode_a, fnode_b, seg, cbase, nc, min_dist, vals, last_changed, changed, csize, dst, dstnode, small, bignode, bigcnt, bign;
  DeviceBuf<int4> chunks;
  DeviceBuf<unsigned long long> key;
  DeviceBuf<long long> G, bsum;
  DeviceBuf<uint8_t> done, assoc;
  size_t cap_bigcnt = 0, cap_bign = 0;
  // the tree on the host, breadth-first: node 0 is the root
  std::vector<int> t_parent, t_first, t_count;
  std::vector<uint8_t> t_desc;
  dvs_voc_train_report rep{};

  dvs_status alloc() {
    const size_t n = (size_t)std::max(N, 1), mcap = n / 2 + 2;
    DVS_TRY(centre.alloc(2 * n));
    for (DeviceBuf<int>* b : {&perm_a, &perm_b, &fnode_a, &fnode_b, &min_dist, &vals, &csize, &dst, &dstnode}) DVS_TRY(b->alloc(n));
    for (DeviceBuf<int>* b : {&seg, &cbase, &nc, &last_changed, &small, &bignode}) DVS_TRY(b->alloc(mcap + 1));
    DVS_TRY(changed.alloc(kPassBatch));
    DVS_TRY(chunks.alloc(n / kChunkRows + n / kSmallNode + 2));
    DVS_TRY(key.alloc(mcap));
    DVS_TRY(G.alloc(n));
    DVS_TRY(bsum.alloc(n / kScanChunk + 2));
    DVS_TRY(done.alloc(mcap));
    DVS_TRY(assoc.alloc(n));
    return DVS_OK;
  }

  dvs_status scan(const LevelDev& Lv) {
    const int nb = (Lv.P + kScanChunk - 1) / kScanChunk;
    hipLaunchKernelGGL(k_scan_partial, dim3(nb), dim3(kBlock), 0, s, Lv.vals, Lv.P, bsum.get());
    hipLaunchKernelGGL(k_scan_bsums, dim3(1), dim3(kBlock), 0, s, bsum.get(), nb);
    hipLaunchKernelGGL(k_scan_final, dim3(nb), dim3(kBlock), 0, s, Lv.vals, Lv.P, bsum.get(), Lv.G);
    DVS_HIP(hipGetLastError());
    return DVS_OK;
  }

  template <class T>
  dvs_status up(T* d, const std::vector<T>& h) {
    if (!h.empty()) DVS_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return DVS_OK;
  }

  dvs_status run() {
    const int k = prm.k, L = prm.L;
    t_parent.assign(1, -1); t_first.assign(1, 0); t_count.assign(1, 0); t_desc.assign(32, 0);
    if (N == 0) return DVS_OK;
    std::vector<HNode> nodes(1, HNode{0, N, splitmix64(prm.seed), 0});
    int P = N;
    int* perm = perm_a.get(); int* fnode = fnode_a.get();
    int* perm2 = perm_b.get(); int* fnode2 = fnode_b.get();
    hipLaunchKernelGGL(k_iota, dim3(blocks_for(N)), dim3(kBlock), 0, s, perm, N);
    DVS_HIP(hipMemsetAsync(fnode, 0, sizeof(int) * N, s));
    std::vector<int> h_seg, h_cbase, h_small, h_bignode, h_nc, h_csize, h_last, h_dst, h_dstnode;
    std::vector<int4> h_chunks;
    std::vector<unsigned long long> h_key;
    std::vector<uint8_t> h_centre;
    for (int level = 1; !nodes.empty(); level++) {
      const int M = (int)nodes.size();
      h_seg.assign(M + 1, 0); h_cbase.assign(M + 1, 0); h_key.resize(M);
      h_small.clear(); h_bignode.clear(); h_chunks.clear();
      for (int m = 0; m < M; m++) {
        const HNode& nd = nodes[m];
        h_seg[m] = nd.begin; h_seg[m + 1] = nd.begin + nd.size;
        h_cbase[m + 1] = h_cbase[m] + std::min(k, nd.size);
        h_key[m] = nd.key;
        if (nd.size <= k) continue;
        if (nd.size <= kSmallNode) { h_small.push_back(m); continue; }
        const int big = (int)h_bignode.size();
        h_bignode.push_back(m);
        for (int a = nd.begin; a < nd.begin + nd.size; a += kChunkRows) h_chunks.push_back(make_int4(m, a, std::min(a + kChunkRows, nd.begin + nd.size), big));
      }
      const int slots = h_cbase[M], nsmall = (int)h_small.size(), nbig = (int)h_bignode.size();
      const bool iterate = nsmall + nbig > 0;
      DVS_TRY(up(seg.get(), h_seg)); DVS_TRY(up(cbase.get(), h_cbase)); DVS_TRY(up(key.get(), h_key));
      DVS_TRY(up(small.get(), h_small)); DVS_TRY(up(bignode.get(), h_bignode)); DVS_TRY(up(chunks.get(), h_chunks));
      if (nbig) {
        DVS_HIP(hipStreamSynchronize(s));
        DVS_TRY(grow(bigcnt, cap_bigcnt, (size_t)nbig * k * 256));
        DVS_TRY(grow(bign, cap_bign, (size_t)nbig * k));
      }
      const LevelDev Lv{feat.get(), P, M, k, perm, fnode, seg.get(), cbase.get(), key.get(), centre.get(), nc.get(), done.get(), assoc.get(),
                        min_dist.get(), vals.get(), G.get(), last_changed.get(), changed.get()};
      hipLaunchKernelGGL(k_level_init, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv);
      hipLaunchKernelGGL(k_seed_init, dim3(blocks_for(M)), dim3(kBlock), 0, s, Lv);
      int passes_run = 0;
      if (iterate) {
        for (int r = 1; r < k; r++) {
          hipLaunchKernelGGL(k_seed_update, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv, r);
          DVS_TRY(scan(Lv));
          hipLaunchKernelGGL(k_seed_pick, dim3(blocks_for(M)), dim3(kBlock), 0, s, Lv, r);
        }
        hipLaunchKernelGGL(k_assoc, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv, 1, 0);
        passes_run = 1;
        while (passes_run < prm.max_iterations) {
          const int batch = std::min(kPassBatch, prm.max_iterations - passes_run);
          DVS_HIP(hipMemsetAsync(changed.get(), 0, sizeof(int) * kPassBatch, s));
          for (int j = 0; j < batch; j++) {
            if (nsmall) hipLaunchKernelGGL(k_mean_small, dim3((nsmall + kBlock / 32 - 1) / (kBlock / 32)), dim3(kBlock), 0, s, Lv, small.get(), nsmall);
            if (nbig) {
              DVS_HIP(hipMemsetAsync(bigcnt.get(), 0, sizeof(int) * (size_t)nbig * k * 256, s));
              DVS_HIP(hipMemsetAsync(bign.get(), 0, sizeof(int) * (size_t)nbig * k, s));
              hipLaunchKernelGGL(k_counts_big, dim3((unsigned)h_chunks.size()), dim3(kBlock), sizeof(int) * (size_t)k * 257, s, Lv, chunks.get(), bigcnt.get(),
                                 bign.get());
              hipLaunchKernelGGL(k_mean_big, dim3(blocks_for((long long)nbig * k * 32)), dim3(kBlock), 0, s, Lv, bignode.get(), nbig, bigcnt.get(), bign.get());
            }
            hipLaunchKernelGGL(k_assoc, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv, passes_run + 1 + j, j);
          }
          DVS_HIP(hipGetLastError());
          passes_run += batch;
          int word = 0;                          // the one read-back per batch of passes: did the batch's last pass change anything?
          DVS_HIP(hipMemcpyAsync(&word, changed.get() + batch - 1, sizeof(int), hipMemcpyDeviceToHost, s));
          DVS_HIP(hipStreamSynchronize(s));
          if (!word) break;
        }
      }
      DVS_HIP(hipMemsetAsync(csize.get(), 0, sizeof(int) * slots, s));
      hipLaunchKernelGGL(k_csize, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv, csize.get());
      DVS_HIP(hipGetLastError());
      h_nc.resize(M); h_last.resize(M); h_csize.resize(slots); h_centre.resize((size_t)slots * 32);
      DVS_HIP(hipMemcpyAsync(h_nc.data(), nc.get(), sizeof(int) * M, hipMemcpyDeviceToHost, s));
      DVS_HIP(hipMemcpyAsync(h_last.data(), last_changed.get(), sizeof(int) * M, hipMemcpyDeviceToHost, s));
      DVS_HIP(hipMemcpyAsync(h_csize.data(), csize.get(), sizeof(int) * slots, hipMemcpyDeviceToHost, s));
      DVS_HIP(hipMemcpyAsync(h_centre.data(), centre.get(), (size_t)slots * 32, hipMemcpyDeviceToHost, s));
      DVS_HIP(hipStreamSynchronize(s));
      // the level's nodes join the tree; clusters of more than one member are the next level's nodes
      rep.levels_run = level;
      std::vector<HNode> next;
      h_dst.assign(slots, -1); h_dstnode.assign(slots, -1);
      int next_P = 0, max_nc = 0;
      for (int m = 0; m < M; m++) {
        const HNode& nd = nodes[m];
        const int n = h_nc[m];
        if (n < 0 || n > std::min(k, nd.size)) { set_error("dvs_voc_train: node with %d centres of %d features (k = %d)", n, nd.size, k); return DVS_ERR_HIP; }
        max_nc = std::max(max_nc, n);
        if (nd.size > k) {
          const int passes = std::min(h_last[m] + 1, prm.max_iterations);
          rep.max_passes = std::max(rep.max_passes, passes);
          if (h_last[m] >= prm.max_iterations) rep.nodes_capped++;
          if (n < k) rep.nodes_short_seeded++;
        }
        t_first[nd.tree] = (int)t_parent.size(); t_count[nd.tree] = n;
        for (int c = 0; c < n; c++) {
          const int slot = h_cbase[m] + c, members = h_csize[slot];
          const int id = (int)t_parent.size();
          t_parent.push_back(nd.tree); t_first.push_back(0); t_count.push_back(0);
          t_desc.insert(t_desc.end(), h_centre.begin() + (size_t)slot * 32, h_centre.begin() + (size_t)slot * 32 + 32);
          if (members == 0) rep.clusters_emptied++;
          if (level < L && members > 1) {
            h_dst[slot] = next_P; h_dstnode[slot] = (int)next.size();
            next.push_back(HNode{next_P, members, splitmix64(nd.key ^ (unsigned long long)(c + 1)), id});
            next_P += members;
          }
        }
      }
      if (next_P > P) { set_error("dvs_voc_train: the next level holds %d of %d features", next_P, P); return DVS_ERR_HIP; }
      if (!next.empty()) {
        DVS_TRY(up(dst.get(), h_dst)); DVS_TRY(up(dstnode.get(), h_dstnode));
        for (int c = 0; c < max_nc; c++) {
          hipLaunchKernelGGL(k_flag, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv, c);
          DVS_TRY(scan(Lv));
          hipLaunchKernelGGL(k_scatter, dim3(blocks_for(P)), dim3(kBlock), 0, s, Lv, c, dst.get(), dstnode.get(), next_P, perm2, fnode2);
        }
        DVS_HIP(hipGetLastError());
        DVS_HIP(hipStreamSynchronize(s));        // the host vectors uploaded above are rewritten for the next level
        std::swap(perm, perm2); std::swap(fnode, fnode2);
      }
      nodes.swap(next);
      P = next_P;
    }
    return DVS_OK;
  }

  // depth-first ids: a node's children get consecutive ids, then the subtree below child 0, below child 1, ...
  void number(int node, std::vector<int>& id_of, std::vector<int>& order) {
    for (int c = 0; c < t_count[node]; c++) { id_of[t_first[node] + c] = (int)order.size() + 1; order.push_back(t_first[node] + c); }
    for (int c = 0; c < t_count[node]; c++) number(t_first[node] + c, id_of, order);
  }

  dvs_status finish(dvs_bow_vocab** out) {
    const int n = (int)t_parent.size() - 1;
    std::vector<int> id_of(n + 1, 0), order;
    order.reserve(n);
    number(0, id_of, order);
    std::vector<int32_t> parent(n);
    std::vector<uint8_t> leaf(n), desc((size_t)n * 32);
    std::vector<double> weight(n, 0.0);
    for (int j = 0; j < n; j++) {
      const int t = order[j];
      parent[j] = id_of[t_parent[t]];
      leaf[j] = t_count[t] == 0 ? 1 : 0;
      memcpy(&desc[(size_t)j * 32], &t_desc[(size_t)t * 32], 32);
    }
    HostVocab H;
    DVS_TRY(bow_build_vocab(prm.k, prm.L, prm.scoring, prm.weighting, n, parent.data(), leaf.data(), desc.data(), weight.data(), &H));
    dvs_bow_vocab* v = nullptr;
    DVS_TRY(bow_create_vocab(device, (void*)s, H, &v));
    const dvs_status st = weights(v, H);
    if (st != DVS_OK) { dvs_bow_vocab_destroy(v); return st; }
    rep.n_nodes = H.n_nodes; rep.n_words = H.n_words;
    *out = v;
    return DVS_OK;
  }

  // setNodeWeights: TF / BINARY 1.0 per word; TF_IDF / IDF log(nimages / Ni) with Ni counted by the descent over every training feature
  dvs_status weights(dvs_bow_vocab* v, const HostVocab& H) {
    const int nw = H.n_words;
    if (nw == 0) return DVS_OK;
    std::vector<double> w(nw, 1.0);
    if (prm.weighting == DVS_BOW_TF_IDF || prm.weighting == DVS_BOW_IDF) {
      DeviceBuf<int> stamp, Ni;
      DVS_TRY(stamp.alloc(nw)); DVS_TRY(Ni.alloc(nw));
      DVS_HIP(hipMemsetAsync(stamp.get(), 0, sizeof(int) * nw, s));
      DVS_HIP(hipMemsetAsync(Ni.get(), 0, sizeof(int) * nw, s));
      DVS_HIP(hipMemcpyAsync(changed.get(), &N, sizeof(int), hipMemcpyHostToDevice, s));
      int* feat_word = vals.get();              // the level loop is over: its blocks hold the descent's outputs
      DVS_TRY(bow_enqueue_descend(v->V, (const uint8_t*)feat.get(), changed.get(), N, 1, H.L, feat_word, min_dist.get(), (double*)G.get(), s));
      for (int f = 0; f < nimages; f++) {
        const int cnt = img_off[f + 1] - img_off[f];
        if (cnt > 0) hipLaunchKernelGGL(k_ni_count, dim3(blocks_for(cnt)), dim3(kBlock), 0, s, feat_word + img_off[f], cnt, nw, f + 1, stamp.get(), Ni.get());
      }
      DVS_HIP(hipGetLastError());
      std::vector<int> h_ni(nw);
      DVS_HIP(hipMemcpyAsync(h_ni.data(), Ni.get(), sizeof(int) * nw, hipMemcpyDeviceToHost, s));
      DVS_HIP(hipStreamSynchronize(s));
      for (int i = 0; i < nw; i++) w[i] = h_ni[i] > 0 ? log((double)nimages / (double)h_ni[i]) : 0.0;
    }
    std::vector<double> rows(H.word_id.size(), 0.0);
    for (size_t r = 0; r < rows.size(); r++) if (H.word_id[r] >= 0) rows[r] = w[H.word_id[r]];
    DVS_HIP(hipMemcpyAsync(v->weight.get(), rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, s));
    DVS_HIP(hipStreamSynchronize(s));
    return DVS_OK;
  }
};

dvs_status check_params(const dvs_voc_train_params* p) {
  DVS_ARG(p != nullptr);
  if (p->k < 2 || p->k > DVS_BOW_MAX_K || p->L < 1 || p->L > DVS_BOW_MAX_L || p->weighting < 0 || p->weighting > 3 || p->scoring < 0 || p->scoring > 5 ||
      p->max_iterations < 1) {
    set_error("dvs_voc_train: k=%d L=%d weighting=%d scoring=%d max_iterations=%d: k in 2..%d, L in 1..%d, weighting in 0..3, scoring in 0..5, "
              "max_iterations >= 1", p->k, p->L, p->weighting, p->scoring, p->max_iterations, DVS_BOW_MAX_K, DVS_BOW_MAX_L);
    return DVS_ERR_ARG;
  }
  if (p->scoring != DVS_BOW_L1_NORM) {
    set_error("dvs_voc_train: scoring %d: only L1_NORM (0) is built", p->scoring);
    return DVS_ERR_UNSUPPORTED;
  }
  return DVS_OK;
}

constexpr long long kMaxFeatures = 0x3fffffff;

dvs_status train(Trainer& T, dvs_bow_vocab** out, dvs_voc_train_report* report) {
  DVS_TRY(T.alloc());
  DVS_TRY(T.run());
  DVS_TRY(T.finish(out));
  if (report) *report = T.rep;
  return DVS_OK;
}

// the arrays of dvs_bow_vocab_from_arrays back from the handle's rows
dvs_status read_arrays(const dvs_bow_vocab* v, std::vector<int32_t>& parent, std::vector<uint8_t>& leaf, std::vector<uint8_t>& desc, std::vector<double>& weight) {
  const int n = v->H.n_nodes, R = n + 1;
  DVS_HIP(hipSetDevice(v->device));
  DVS_HIP(hipStreamSynchronize(v->stream));
  std::vector<uint8_t> r_desc((size_t)R * 32);
  std::vector<int> r_begin(R), r_count(R), r_word(R), r_id(R);
  std::vector<double> r_weight(R);
  DVS_HIP(hipMemcpy(r_desc.data(), v->desc.get(), r_desc.size(), hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(r_begin.data(), v->child_begin.get(), sizeof(int) * R, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(r_count.data(), v->child_count.get(), sizeof(int) * R, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(r_word.data(), v->word_id.get(), sizeof(int) * R, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(r_id.data(), v->orig_id.get(), sizeof(int) * R, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(r_weight.data(), v->weight.get(), sizeof(double) * R, hipMemcpyDeviceToHost));
  parent.assign(n, 0); leaf.assign(n, 0); desc.assign((size_t)n * 32, 0); weight.assign(n, 0.0);
  for (int r = 0; r < R; r++) {
    const int id = r_id[r];
    if (id < 0 || id > n || r_begin[r] < 0 || r_count[r] < 0 || (long long)r_begin[r] + r_count[r] > R) { set_error("dvs_voc_get_arrays: inconsistent rows"); return DVS_ERR_HIP; }
    for (int c = 0; c < r_count[r]; c++) {
      const int kid = r_id[r_begin[r] + c];
      if (kid < 1 || kid > n) { set_error("dvs_voc_get_arrays: inconsistent rows"); return DVS_ERR_HIP; }
      parent[kid - 1] = id;
    }
    if (id > 0) {
      leaf[id - 1] = r_word[r] >= 0 ? 1 : 0;
      weight[id - 1] = r_weight[r];
      memcpy(&desc[(size_t)(id - 1) * 32], &r_desc[(size_t)r * 32], 32);
    }
  }
  return DVS_OK;
}

}  // namespace

extern "C" {

dvs_status dvs_voc_train_default_params(dvs_voc_train_params* p) {
  DVS_ARG(p != nullptr);
  p->k = 10; p->L = 5; p->weighting = DVS_BOW_TF_IDF; p->scoring = DVS_BOW_L1_NORM; p->seed = 0; p->max_iterations = 100;
  return DVS_OK;
}

dvs_status dvs_voc_train(int32_t device, void* hip_stream, const dvs_voc_train_params* params, const uint8_t* desc, const int32_t* image_counts,
                         int32_t nimages, dvs_bow_vocab** out, dvs_voc_train_report* report) {
  DVS_ARG(out != nullptr);
  *out = nullptr;
  DVS_TRY(check_params(params));
  DVS_ARG(nimages >= 0 && (nimages == 0 || image_counts));
  Trainer T;
  T.img_off.assign(nimages + 1, 0);
  long long total = 0;
  for (int f = 0; f < nimages; f++) {
    if (image_counts[f] < 0) { set_error("dvs_voc_train: image %d has a negative count %d", f, image_counts[f]); return DVS_ERR_ARG; }
    total += image_counts[f];
    if (total > kMaxFeatures) { set_error("dvs_voc_train: more than %lld features", kMaxFeatures); return DVS_ERR_ARG; }
    T.img_off[f + 1] = (int)total;
  }
  DVS_ARG(total == 0 || desc);
  DVS_TRY(check_device(device));
  T.device = device; T.s = (hipStream_t)hip_stream; T.prm = *params; T.N = (int)total; T.nimages = nimages;
  DVS_TRY(T.feat.alloc(2 * (size_t)std::max(T.N, 1)));
  if (T.N) DVS_HIP(hipMemcpyAsync(T.feat.get(), desc, (size_t)T.N * 32, hipMemcpyHostToDevice, T.s));
  return train(T, out, report);
}

dvs_status dvs_voc_train_device(int32_t device, void* hip_stream, const dvs_voc_train_params* params, const uint8_t* d_desc, const int32_t* d_n,
                                int32_t stride_rows, int32_t nframes, dvs_bow_vocab** out, dvs_voc_train_report* report) {
  DVS_ARG(out != nullptr);
  *out = nullptr;
  DVS_TRY(check_params(params));
  DVS_ARG(nframes >= 0 && stride_rows >= 0 && (nframes == 0 || d_n) && (nframes == 0 || stride_rows == 0 || d_desc));
  DVS_ARG(((uintptr_t)d_desc & 15) == 0);
  DVS_ARG((long long)nframes * stride_rows <= kMaxFeatures && nframes <= 65535);
  DVS_TRY(check_device(device));
  Trainer T;
  T.device = device; T.s = (hipStream_t)hip_stream; T.prm = *params; T.nimages = nframes;
  std::vector<int> counts(nframes, 0);
  if (nframes) {
    DVS_HIP(hipMemcpyAsync(counts.data(), d_n, sizeof(int) * nframes, hipMemcpyDeviceToHost, T.s));
    DVS_HIP(hipStreamSynchronize(T.s));
  }
  T.img_off.assign(nframes + 1, 0);
  for (int f = 0; f < nframes; f++) T.img_off[f + 1] = T.img_off[f] + std::min(std::max(counts[f], 0), stride_rows);   // clamped as the transform clamps
  T.N = T.img_off[nframes];
  DVS_TRY(T.feat.alloc(2 * (size_t)std::max(T.N, 1)));
  DeviceBuf<int> d_off;
  if (T.N) {
    DVS_TRY(d_off.upload(T.img_off));
    hipLaunchKernelGGL(k_compact, dim3(blocks_for(2LL * stride_rows), nframes), dim3(kBlock), 0, T.s, (const uint4*)d_desc, stride_rows, d_off.get(),
                       T.feat.get());
    DVS_HIP(hipGetLastError());
  }
  return train(T, out, report);   // ends synchronised: d_off is idle when it is freed
}

dvs_status dvs_voc_get_arrays(const dvs_bow_vocab* voc, int32_t cap, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int32_t* n_nodes) {
  DVS_ARG(voc && n_nodes && cap >= 0);
  const int n = voc->H.n_nodes;
  *n_nodes = n;
  if (cap < n) { set_error("dvs_voc_get_arrays: %d nodes (cap %d)", n, cap); return DVS_ERR_CAPACITY; }
  if (n == 0) return DVS_OK;
  std::vector<int32_t> p; std::vector<uint8_t> l, d; std::vector<double> w;
  DVS_TRY(read_arrays(voc, p, l, d, w));
  if (parent) memcpy(parent, p.data(), sizeof(int32_t) * n);
  if (is_leaf) memcpy(is_leaf, l.data(), n);
  if (desc) memcpy(desc, d.data(), (size_t)n * 32);
  if (weight) memcpy(weight, w.data(), sizeof(double) * n);
  return DVS_OK;
}

dvs_status dvs_voc_save_text(const dvs_bow_vocab* voc, const char* path) {
  DVS_ARG(voc && path);
  const int n = voc->H.n_nodes;
  std::vector<int32_t> p; std::vector<uint8_t> l, d; std::vector<double> w;
  if (n) DVS_TRY(read_arrays(voc, p, l, d, w));
  FILE* fp = fopen(path, "w");
  if (!fp) { set_error("dvs_voc_save_text: cannot open %s for writing", path); return DVS_ERR_ARG; }
  fprintf(fp, "%d %d %d %d\n", voc->H.k, voc->H.L, voc->H.scoring, voc->H.weighting);
  for (int j = 0; j < n; j++) {
    fprintf(fp, "%d %d", p[j], (int)l[j]);
    for (int b = 0; b < 32; b++) fprintf(fp, " %d", (int)d[(size_t)j * 32 + b]);
    fprintf(fp, " %.17g\n", w[j]);
  }
  const bool bad = ferror(fp) != 0;
  if (fclose(fp) != 0 || bad) { set_error("dvs_voc_save_text: writing %s failed", path); return DVS_ERR_ARG; }
  return DVS_OK;
}

}  // extern "C"
