// motion_seg.hip — motion segmentation from two depth images and their relative pose (include/dvslam_hip.h, dvs_motion_*): the keep mask
// the extractor's masked entry points read, made on the device.  The rule is stated in the header and restated in tests/motion_ref.py;
// everything here is integer or FP64 in a fixed order, so the tests compare bit for bit.
//
// One call is a fixed sequence on the handle's stream, whatever the images hold; the host reads nothing back but the optional statistics:
//   memset      the statistics record (2 KB)
//   k_seed      one thread per current pixel: back-project, transform, project, 3 x 3 gather from the reference, compare -> u8 seed image.
//               The nine gathers are the only irregular traffic; everything else in the call streams.
//   k_label_tile   one workgroup per 32 x 32 tile: union-find over the tile's seeds in LDS (ccl_union.h), then every pixel writes its
//               tile root as a GLOBAL linear index into parent[] (-1 off the seeds) and zeroes area[].  Row-major order inside a tile is the
//               order of the global indices, so the tile root is the smallest global index of the tile-local component.
//   k_merge_borders  one thread per pixel of a tile's first row / first column: unions with its (up to three) neighbours across the border.
//   k_flatten_count  one thread per pixel: label[p] = find(p), area[label] += 1 (one atomic per distinct root in a wavefront), roots counted.
//   k_dynamic_hdilate  dynamic[p] = area[label[p]] >= min_area; horizontal dilation from a 512-bit ballot row in LDS.
//   k_vdilate_mask   vertical running sum over the horizontally dilated image -> the mask; zeros counted.
//
// Coherence.  The eight XCDs' L2s are not coherent with each other for plain loads inside one launch, so the launches are cut such that
// no plain load ever reads what another workgroup writes in the SAME launch:
//   k_label_tile's unions are on LDS; its global writes (parent, area) are read by later launches only.
//   k_merge_borders is the one place where workgroups meet in global memory.  There EVERY read and every update of parent[] is an
//     agent-scope atomic (CclAgent below), and a union decides on the value its fetch_min RETURNED, never on a separate read; the seed
//     image it reads plainly was written by an earlier launch.
//   k_flatten_count reads parent[] (complete at the launch boundary) and writes label[] — another array — and area[] by atomic adds only.
//   k_dynamic_hdilate reads label[] / area[], k_vdilate_mask reads what k_dynamic_hdilate wrote.
// What bounds each launch: k_seed, k_dynamic_hdilate and k_vdilate_mask are straight-line per pixel (the last one a loop over its 16 rows).
// find / union end by construction — parents only ever decrease (ccl_union.h has the argument); in LDS a chain is at most 1024 long, in
// global memory at most rows * cols, and in practice a few links, since every tile hangs flat under its root before the merge begins.
// Nothing of a call survives into the next: seed, parent, area, label, dynamic, the dilated image and the mask are written for every
// pixel in every call, the record is cleared first.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>
#include <new>
#include "common.h"
#include "device_mem.h"
#include "ccl_union.h"
#include "motion_internal.h"

namespace dvs {

constexpr int kTile = DVS_MOTION_TILE;
static_assert(kTile == 32, "k_label_tile indexes a tile by li & 31, li >> 5");
// the statistics record: kStatSlots copies of S_INTS counters.  A workgroup adds to the copy its block index selects, so the integer adds of
// a launch spread over kStatSlots addresses instead of queueing on one; the host sums the copies (integer sums: any order, one result).
enum { S_VALID = 0, S_SEED, S_COMP, S_KEPT, S_DYN, S_MASKED, S_INTS = 8 };
constexpr int kStatSlots = 64;
__device__ __forceinline__ int* stat_slot(int* stats) {
  return stats + S_INTS * (int)((blockIdx.x + blockIdx.y * gridDim.x) & (kStatSlots - 1));
}

struct MoArgs {
  int rows, cols;
  double fx, fy, cx, cy;
  int dmin, dmax;
  double tau0, tau2;
  double R[9], t[3];
};

__device__ __forceinline__ void count_pred(bool pred, int* counter) {
  const unsigned long long b = __ballot(pred);
  if (b && (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) atomicAdd(counter, __popcll(b));
}

// stage 1 (one wavefront = 64 pixels of one row)
__global__ __launch_bounds__(256) void k_seed(MoArgs a, const uint8_t* __restrict__ ref, size_t rstep, const uint8_t* __restrict__ cur, size_t cstep,
                                              uint8_t* __restrict__ seed, int* __restrict__ stats) {
  const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
  bool reached = false, is_seed = false;
  const bool inb = u < a.cols && v < a.rows;
  if (inb) {
    const int d = reinterpret_cast<const uint16_t*>(cur + (size_t)v * cstep)[u];
    if (a.dmin < d && d <= a.dmax) {
      const double z = (double)d * 0.001;
      const double x = ((double)u - a.cx) * z / a.fx;
      const double y = ((double)v - a.cy) * z / a.fy;
      const double xr = a.R[0] * x + a.R[1] * y + a.R[2] * z + a.t[0];
      const double yr = a.R[3] * x + a.R[4] * y + a.R[5] * z + a.t[1];
      const double zr = a.R[6] * x + a.R[7] * y + a.R[8] * z + a.t[2];
      if (!(zr <= 0.0)) {
        const double ur = floor(a.fx * xr / zr + a.cx + 0.5);
        const double vr = floor(a.fy * yr / zr + a.cy + 0.5);
        if (1.0 <= ur && ur <= (double)(a.cols - 2) && 1.0 <= vr && vr <= (double)(a.rows - 2)) {   // as doubles: NaN and huge values fail here
          const int iu = (int)ur, iv = (int)vr;
          int m = 65536;
          bool ok = true;
#pragma unroll
          for (int dy = -1; dy <= 1; dy++) {
            const uint16_t* row = reinterpret_cast<const uint16_t*>(ref + (size_t)(iv + dy) * rstep);
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
              const int dd = row[iu + dx];
              ok = ok && (a.dmin < dd && dd <= a.dmax);
              m = min(m, dd);
            }
          }
          if (ok) {
            reached = true;
            const double tau = a.tau0 + a.tau2 * zr * zr;
            is_seed = zr < (double)m * 0.001 - tau;
          }
        }
      }
    }
    seed[(size_t)v * a.cols + u] = is_seed ? 1 : 0;
  }
  stats = stat_slot(stats);
  count_pred(reached, stats + S_VALID);
  count_pred(is_seed, stats + S_SEED);
}

// the forest in LDS: workgroup-scope atomics (one workgroup, one LDS)
struct CclLds {
  int* lab;
  __device__ __forceinline__ int load(int i) { return __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int fetch_min(int i, int v) { return __hip_atomic_fetch_min(lab + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
// the forest in global memory while other workgroups work on it: agent-scope atomics for every access
struct CclAgent {
  int* parent;
  __device__ __forceinline__ int load(int i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int fetch_min(int i, int v) { return __hip_atomic_fetch_min(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// a finished forest (written by an earlier launch): plain loads, no writes
struct CclRead {
  const int* parent;
  __device__ __forceinline__ int load(int i) { return parent[i]; }
};

__global__ __launch_bounds__(256) void k_label_tile(const uint8_t* __restrict__ seed, int rows, int cols, int* __restrict__ parent, int* __restrict__ area) {
  __shared__ int lab[kTile * kTile];
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int li = threadIdx.x + 256 * k, gx = tx0 + (li & 31), gy = ty0 + (li >> 5);
    lab[li] = (gx < cols && gy < rows && seed[(size_t)gy * cols + gx]) ? li : -1;
  }
  __syncthreads();
  CclLds m{lab};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int li = threadIdx.x + 256 * k, lx = li & 31, ly = li >> 5;
    if (m.load(li) < 0) continue;   // >= 0 exactly on the seeds, before and after any union
    // a set pixel above makes the two diagonals redundant: they are its row neighbours, joined to it by their own west links
    if (lx > 0 && m.load(li - 1) >= 0) ccl_unite(m, li, li - 1);
    if (ly > 0) {
      if (m.load(li - 32) >= 0) {
        ccl_unite(m, li, li - 32);
      } else {
        if (lx > 0 && m.load(li - 33) >= 0) ccl_unite(m, li, li - 33);
        if (lx < 31 && m.load(li - 31) >= 0) ccl_unite(m, li, li - 31);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int li = threadIdx.x + 256 * k, gx = tx0 + (li & 31), gy = ty0 + (li >> 5);
    if (gx >= cols || gy >= rows) continue;
    const size_t g = (size_t)gy * cols + gx;
    int out = -1;
    if (lab[li] >= 0) {
      const int r = ccl_find(m, li);
      out = (ty0 + (r >> 5)) * cols + tx0 + (r & 31);
    }
    parent[g] = out;
    area[g] = 0;
  }
}

// blockIdx.y = 0: the first rows of the tile rows 1.. (pixels (x, 32 b), neighbours in row 32 b - 1); 1: the first columns of the tile
// columns 1.. (pixels (32 b, y), neighbours in column 32 b - 1).  Together these are all 8-connected pairs that lie in two tiles.
__global__ __launch_bounds__(256) void k_merge_borders(const uint8_t* __restrict__ seed, int rows, int cols, int* parent) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  CclAgent m{parent};
  if (blockIdx.y == 0) {
    const int nb = (rows - 1) / kTile;
    if (i >= (long long)nb * cols) return;
    const int x = (int)(i % cols), y = ((int)(i / cols) + 1) * kTile;
    const int p = y * cols + x;
    if (!seed[p]) return;
    const int q = p - cols;   // a set pixel straight across makes the diagonals redundant: its row neighbours hang on it already (or by part 1)
    if (seed[q]) {
      ccl_unite(m, p, q);
    } else {
      if (x > 0 && seed[q - 1]) ccl_unite(m, p, q - 1);
      if (x + 1 < cols && seed[q + 1]) ccl_unite(m, p, q + 1);
    }
  } else {
    const int nb = (cols - 1) / kTile;
    if (i >= (long long)nb * rows) return;
    const int y = (int)(i % rows), x = ((int)(i / rows) + 1) * kTile;
    const int p = y * cols + x;
    if (!seed[p]) return;
    const int q = p - 1;      // likewise: its column neighbours hang on it already (or by part 0)
    if (seed[q]) {
      ccl_unite(m, p, q);
    } else {
      if (y > 0 && seed[q - cols]) ccl_unite(m, p, q - cols);
      if (y + 1 < rows && seed[q + cols]) ccl_unite(m, p, q + cols);
    }
  }
}

__global__ __launch_bounds__(256) void k_flatten_count(const int* __restrict__ parent, int n, int* __restrict__ label, int* area, int* __restrict__ stats) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  int root = -1;
  if (p < n && parent[p] >= 0) {
    CclRead m{parent};
    root = ccl_find(m, p);
  }
  if (p < n) label[p] = root;
  count_pred(root >= 0 && root == p, stat_slot(stats) + S_COMP);
  // area: one integer add per distinct root among the wavefront's lanes (neighbouring pixels mostly share theirs)
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  unsigned long long rem = __ballot(root >= 0);
  while (rem) {
    const int leader = __ffsll((long long)rem) - 1;
    const int r = __shfl(root, leader);
    const unsigned long long b = __ballot(root == r);
    if (lane == leader) atomicAdd(area + r, __popcll(b));
    rem &= ~b;
  }
}

// one workgroup per 256 pixels of one row.  Bit j of the 512-bit row in LDS is dynamic(x0 - 64 + j); the window of pixel x0 + i is bits
// 64 + i - r .. 64 + i + r, at most 63 wide, so it lies in one or two words.
__global__ __launch_bounds__(256) void k_dynamic_hdilate(const int* __restrict__ label, const int* __restrict__ area, int rows, int cols, int min_area, int r,
                                                         uint8_t* __restrict__ dyn, uint8_t* __restrict__ hd, int* __restrict__ stats) {
  __shared__ unsigned long long words[8];
  const int x0 = blockIdx.x * 256, y = blockIdx.y, tid = threadIdx.x;
  const size_t rowoff = (size_t)y * cols;
  stats = stat_slot(stats);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int xi = x0 - 64 + tid + 256 * k;
    bool d = false, kept_root = false;
    const bool own = xi >= x0 && xi < x0 + 256 && xi < cols;
    if (xi >= 0 && xi < cols) {
      const int l = label[rowoff + xi];
      if (l >= 0) {
        d = area[l] >= min_area;
        kept_root = d && l == (int)(rowoff + xi);
      }
    }
    if (own) dyn[rowoff + xi] = d ? 1 : 0;
    const unsigned long long b = __ballot(d);
    if ((tid & 63) == 0) words[4 * k + (tid >> 6)] = b;
    count_pred(own && d, stats + S_DYN);
    count_pred(own && kept_root, stats + S_KEPT);
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x >= cols) return;
  const int lo = 64 + tid - r, hi = 64 + tid + r;
  const unsigned long long mlo = ~0ull << (lo & 63), mhi = ~0ull >> (63 - (hi & 63));
  const int wlo = lo >> 6, whi = hi >> 6;
  const unsigned long long any = wlo == whi ? (words[wlo] & mlo & mhi) : ((words[wlo] & mlo) | (words[whi] & mhi));
  hd[rowoff + x] = any ? 1 : 0;
}

// a thread owns a column over 16 rows and keeps the sum of hd over [y - r, y + r] (rows outside the image add nothing)
__global__ __launch_bounds__(256) void k_vdilate_mask(const uint8_t* __restrict__ hd, int rows, int cols, int r, uint8_t* __restrict__ mask, size_t mstep,
                                                      int* __restrict__ stats) {
  const int x = blockIdx.x * 64 + threadIdx.x, y0 = (blockIdx.y * 4 + threadIdx.y) * 16;
  const bool inb = x < cols;
  int sum = 0, nmasked = 0;
  if (inb)
    for (int y = max(0, y0 - r); y <= min(rows - 1, y0 + r); y++) sum += hd[(size_t)y * cols + x];
  const int y1 = min(rows, y0 + 16);
  for (int y = y0; y < y1; y++) {   // y0, y1 are the wavefront's: threadIdx.y is its number
    nmasked += __popcll(__ballot(inb && sum > 0));
    if (inb) {
      mask[(size_t)y * mstep + x] = sum > 0 ? 0 : 255;
      if (y + r + 1 < rows) sum += hd[(size_t)(y + r + 1) * cols + x];
      if (y - r >= 0) sum -= hd[(size_t)(y - r) * cols + x];
    }
  }
  if (nmasked && threadIdx.x == 0) atomicAdd(stat_slot(stats) + S_MASKED, nmasked);
}

// the three labelling launches: seed image -> parent (scratch), label, area; the root count goes to stats[S_COMP]
static dvs_status launch_label(hipStream_t st, const uint8_t* seed, int rows, int cols, int* parent, int* label, int* area, int* stats) {
  const int n = rows * cols;
  hipLaunchKernelGGL(k_label_tile, dim3((cols + kTile - 1) / kTile, (rows + kTile - 1) / kTile), dim3(256), 0, st, seed, rows, cols, parent, area);
  const long long nh = (long long)((rows - 1) / kTile) * cols, nv = (long long)((cols - 1) / kTile) * rows;
  const long long nm = std::max<long long>(std::max(nh, nv), 1);
  hipLaunchKernelGGL(k_merge_borders, dim3((unsigned)((nm + 255) / 256), 2), dim3(256), 0, st, seed, rows, cols, parent);
  hipLaunchKernelGGL(k_flatten_count, dim3((n + 255) / 256), dim3(256), 0, st, (const int*)parent, n, label, area, stats);
  DVS_HIP(hipGetLastError());
  return DVS_OK;
}

dvs_status motion_check_params(const dvs_motion_params& P) {
  DVS_ARG(P.rows >= 1 && P.rows <= 4096 && P.cols >= 1 && P.cols <= 4096);
  DVS_ARG(__builtin_isfinite(P.fx) && __builtin_isfinite(P.fy) && __builtin_isfinite(P.cx) && __builtin_isfinite(P.cy) && P.fx > 0 && P.fy > 0);
  DVS_ARG(P.min_depth_mm >= 0 && P.min_depth_mm < P.max_depth_mm && P.max_depth_mm <= 65535);
  DVS_ARG(__builtin_isfinite(P.tau0_m) && __builtin_isfinite(P.tau2_per_m) && P.tau0_m >= 0 && P.tau2_per_m >= 0);
  DVS_ARG(P.min_area >= 1 && P.dilate_radius >= 0 && P.dilate_radius <= 31);
  return DVS_OK;
}

}  // namespace dvs

using namespace dvs;

struct dvs_motion {
  dvs_motion_params P;
  int device = 0;
  hipStream_t stream = nullptr;
  // the arena: one block per stage image, rows x cols packed, allocated at create and written whole by every call
  DeviceBuf<uint8_t> seed, dyn, hd;
  DeviceBuf<int> parent, label, area, stats;
  // staging of the host form (allocated by its first call)
  DeviceBuf<uint16_t> s_ref, s_cur;
  DeviceBuf<uint8_t> s_mask;
  bool staged = false;
};

namespace dvs {

dvs_status motion_last_stats(dvs_motion* h, dvs_motion_stats* out) {
  int all[kStatSlots * S_INTS], s[S_INTS] = {0};
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipMemcpyAsync(all, h->stats.get(), sizeof(all), hipMemcpyDeviceToHost, h->stream));
  DVS_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < kStatSlots * S_INTS; k++) s[k % S_INTS] += all[k];
  out->n_valid = s[S_VALID]; out->n_seed = s[S_SEED]; out->n_components = s[S_COMP]; out->n_components_kept = s[S_KEPT];
  out->n_dynamic = s[S_DYN]; out->n_masked = s[S_MASKED];
  return DVS_OK;
}

}  // namespace dvs

static dvs_status motion_check_call(const dvs_motion* h, const void* ref, size_t ref_step, const void* cur, size_t cur_step, const double* R9,
                                    const double* t3, const void* mask, size_t mask_step) {
  DVS_ARG(h && ref && cur && R9 && t3 && mask);
  const size_t drow = (size_t)h->P.cols * 2;
  DVS_ARG(ref_step >= drow && cur_step >= drow && ref_step % 2 == 0 && cur_step % 2 == 0 && mask_step >= (size_t)h->P.cols);
  for (int k = 0; k < 9; k++) DVS_ARG(__builtin_isfinite(R9[k]));
  for (int k = 0; k < 3; k++) DVS_ARG(__builtin_isfinite(t3[k]));
  return DVS_OK;
}

extern "C" {

void dvs_motion_default_params(dvs_motion_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_depth_mm = 300; p->max_depth_mm = 3000;
  p->tau0_m = 0.03; p->tau2_per_m = 0.005;
  p->min_area = 200; p->dilate_radius = 8;
}

dvs_status dvs_motion_create(const dvs_motion_params* params, int32_t device, dvs_motion** out) {
  DVS_ARG(params && out);
  *out = nullptr;
  DVS_TRY(motion_check_params(*params));
  DVS_TRY(check_device(device));
  dvs_motion* h = new (std::nothrow) dvs_motion();
  if (!h) { set_error("dvs_motion_create: out of memory"); return DVS_ERR_HIP; }
  h->P = *params; h->device = device;
  auto alloc_all = [&]() -> dvs_status {
    const size_t px = (size_t)h->P.rows * h->P.cols;
    DVS_TRY(h->seed.alloc(px)); DVS_TRY(h->dyn.alloc(px)); DVS_TRY(h->hd.alloc(px));
    DVS_TRY(h->parent.alloc(px)); DVS_TRY(h->label.alloc(px)); DVS_TRY(h->area.alloc(px)); DVS_TRY(h->stats.alloc(kStatSlots * S_INTS));
    DVS_HIP(hipMemset(h->stats.get(), 0, kStatSlots * S_INTS * sizeof(int)));
    return DVS_OK;
  };
  const dvs_status s = alloc_all();
  if (s != DVS_OK) { dvs_motion_destroy(h); return s; }
  *out = h;
  return DVS_OK;
}

void dvs_motion_destroy(dvs_motion* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;
}

dvs_status dvs_motion_set_stream(dvs_motion* h, void* hip_stream) {
  DVS_ARG(h);
  DVS_HIP(hipSetDevice(h->device));
  DVS_HIP(hipStreamSynchronize(h->stream));
  h->stream = (hipStream_t)hip_stream;
  return DVS_OK;
}

dvs_status dvs_motion_segment_device(dvs_motion* h, const uint16_t* d_ref, size_t ref_step, const uint16_t* d_cur, size_t cur_step, const double* R9,
                                     const double* t3, uint8_t* d_mask, size_t mask_step, dvs_motion_stats* stats) {
  DVS_TRY(motion_check_call(h, d_ref, ref_step, d_cur, cur_step, R9, t3, d_mask, mask_step));
  const dvs_motion_params& P = h->P;
  DVS_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  MoArgs a;
  a.rows = P.rows; a.cols = P.cols; a.fx = P.fx; a.fy = P.fy; a.cx = P.cx; a.cy = P.cy; a.dmin = P.min_depth_mm; a.dmax = P.max_depth_mm;
  a.tau0 = P.tau0_m; a.tau2 = P.tau2_per_m;
  memcpy(a.R, R9, sizeof(a.R)); memcpy(a.t, t3, sizeof(a.t));
  const int rows = P.rows, cols = P.cols;
  int* d_stats = h->stats.get();
  DVS_HIP(hipMemsetAsync(d_stats, 0, kStatSlots * S_INTS * sizeof(int), st));
  hipLaunchKernelGGL(k_seed, dim3((cols + 63) / 64, (rows + 3) / 4), dim3(64, 4), 0, st, a, (const uint8_t*)d_ref, ref_step, (const uint8_t*)d_cur, cur_step,
                     h->seed.get(), d_stats);
  DVS_TRY(launch_label(st, h->seed.get(), rows, cols, h->parent.get(), h->label.get(), h->area.get(), d_stats));
  hipLaunchKernelGGL(k_dynamic_hdilate, dim3((cols + 255) / 256, rows), dim3(256), 0, st, (const int*)h->label.get(), (const int*)h->area.get(), rows, cols,
                     P.min_area, P.dilate_radius, h->dyn.get(), h->hd.get(), d_stats);
  hipLaunchKernelGGL(k_vdilate_mask, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(64, 4), 0, st, (const uint8_t*)h->hd.get(), rows, cols, P.dilate_radius,
                     d_mask, mask_step, d_stats);
  DVS_HIP(hipGetLastError());
  if (stats) DVS_TRY(motion_last_stats(h, stats));
  return DVS_OK;
}

dvs_status dvs_motion_segment(dvs_motion* h, const uint16_t* ref, size_t ref_step, const uint16_t* cur, size_t cur_step, const double* R9, const double* t3,
                              uint8_t* mask, size_t mask_step, dvs_motion_stats* stats) {
  DVS_TRY(motion_check_call(h, ref, ref_step, cur, cur_step, R9, t3, mask, mask_step));
  DVS_HIP(hipSetDevice(h->device));
  const size_t rows = (size_t)h->P.rows, cols = (size_t)h->P.cols;
  if (!h->staged) {
    DVS_TRY(h->s_ref.alloc(rows * cols)); DVS_TRY(h->s_cur.alloc(rows * cols)); DVS_TRY(h->s_mask.alloc(rows * cols));
    h->staged = true;
  }
  hipStream_t st = h->stream;
  DVS_HIP(hipMemcpy2DAsync(h->s_ref.get(), cols * 2, ref, ref_step, cols * 2, rows, hipMemcpyHostToDevice, st));
  DVS_HIP(hipMemcpy2DAsync(h->s_cur.get(), cols * 2, cur, cur_step, cols * 2, rows, hipMemcpyHostToDevice, st));
  DVS_TRY(dvs_motion_segment_device(h, h->s_ref.get(), cols * 2, h->s_cur.get(), cols * 2, R9, t3, h->s_mask.get(), cols, nullptr));
  DVS_HIP(hipMemcpy2DAsync(mask, mask_step, h->s_mask.get(), cols, cols, rows, hipMemcpyDeviceToHost, st));
  DVS_HIP(hipStreamSynchronize(st));
  if (stats) DVS_TRY(motion_last_stats(h, stats));
  return DVS_OK;
}

#ifdef DVS_TEST_HOOKS   // libdvslam_hip_test.so only (include/dvslam_hip_test_motion.h)
dvs_status dvs_test_motion_label(int32_t device, const uint8_t* img, int32_t rows, int32_t cols, int32_t* labels, int32_t* areas) {
  DVS_ARG(img && labels && areas && rows >= 1 && rows <= 4096 && cols >= 1 && cols <= 4096);
  DVS_TRY(check_device(device));
  const size_t n = (size_t)rows * cols;
  DeviceBuf<uint8_t> d_img; DeviceBuf<int> d_parent, d_label, d_area, d_stats;
  DVS_TRY(d_img.alloc(n)); DVS_TRY(d_parent.alloc(n)); DVS_TRY(d_label.alloc(n)); DVS_TRY(d_area.alloc(n)); DVS_TRY(d_stats.alloc(kStatSlots * S_INTS));
  DVS_HIP(hipMemcpy(d_img.get(), img, n, hipMemcpyHostToDevice));
  DVS_HIP(hipMemset(d_stats.get(), 0, kStatSlots * S_INTS * sizeof(int)));
  DVS_TRY(launch_label(nullptr, d_img.get(), rows, cols, d_parent.get(), d_label.get(), d_area.get(), d_stats.get()));
  DVS_HIP(hipMemcpy(labels, d_label.get(), n * 4, hipMemcpyDeviceToHost));
  DVS_HIP(hipMemcpy(areas, d_area.get(), n * 4, hipMemcpyDeviceToHost));
  return DVS_OK;
}

dvs_status dvs_test_motion_stages(dvs_motion* h, uint8_t* seed, int32_t* labels, uint8_t* dynamic) {
  DVS_ARG(h);
  DVS_HIP(hipSetDevice(h->device));
  const size_t n = (size_t)h->P.rows * h->P.cols;
  DVS_HIP(hipStreamSynchronize(h->stream));
  if (seed) DVS_HIP(hipMemcpy(seed, h->seed.get(), n, hipMemcpyDeviceToHost));
  if (labels) DVS_HIP(hipMemcpy(labels, h->label.get(), n * 4, hipMemcpyDeviceToHost));
  if (dynamic) DVS_HIP(hipMemcpy(dynamic, h->dyn.get(), n, hipMemcpyDeviceToHost));
  return DVS_OK;
}
#endif

}  // extern "C"
