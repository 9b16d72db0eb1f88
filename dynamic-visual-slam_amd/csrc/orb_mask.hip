// orb_mask.hip — keep-mask filter of the FAST candidate lists (dvs_orb_extract*_masked, INTEGRATION.md §B1 "Keep masks").
//
// DynaSLAM / DS-SLAM style: corners on dynamic regions are dropped BEFORE the quad-tree distributes a level's quota, so the
// static scene gets the whole budget.  The filter sits between the per-cell FAST (k_fast_wave / k_fast_cell) and the quad-tree:
// it runs on the same stream and cell range right behind every FAST launch (orb.hip, launch_fast), so every schedule that reads
// the lists afterwards sees the filtered ones.  A candidate of level l at region-relative (cx, cy) is kept iff
//   mask[min(rows - 1, floor(Y))][min(cols - 1, floor(X))] != 0,   X = (float)(cx + minBorderX) * mvScaleFactor[l]  (Y alike)
// — the exact coordinates that keypoint would carry in the output (ORBextractor.cpp:886, 1149), so no output keypoint lies on a
// masked pixel.  FAST itself, its threshold fallback, the quotas and every later stage are untouched.
#include <hip/hip_runtime.h>
#include "orb_geom.h"

namespace dvs {

// One wavefront per cell, four cells per workgroup.  The list is compacted in place and in order: each 64-candidate chunk is read
// whole (and its mask bytes fetched) before any lane writes, and a kept candidate's new index nout + rank never exceeds its old one.
__global__ __launch_bounds__(256) void k_cand_mask(const Geom* __restrict__ g, const Cell* __restrict__ cells, const uint8_t* __restrict__ mask,
                                                   uint64_t mstep, uint64_t mfstride, uint32_t* __restrict__ cand, int* __restrict__ cellCount,
                                                   int c0, int c1) {
  const int ci = __builtin_amdgcn_readfirstlane(c0 + 4 * (int)blockIdx.x + ((int)threadIdx.x >> 6));
  if (ci >= c1) return;
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const Cell cell = cells[ci];
  const LevelGeom& L = g->lv[cell.level];
  int* countp = cellCount + (uint64_t)f * g->totalCells + ci;
  const int n = *countp;   // <= L.cellCap (FAST clamps it)
  uint32_t* list = cand + (uint64_t)f * g->candPerFrame + L.candOff + (uint64_t)cell.slot * L.cellCap;
  const uint8_t* m = mask + (uint64_t)f * mfstride;
  const int xmax = g->cols - 1, ymax = g->rows - 1;
  const float s = L.scale;   // 1.0f on level 0: X = cx + minBorderX exactly
  int nout = 0;
  for (int e0 = 0; e0 < n; e0 += 64) {
    const int e = e0 + lane;
    const uint32_t p = e < n ? list[e] : 0u;
    bool keep = false;
    if (e < n) {
      // one float32 multiply each (the file is built with -ffp-contract=off); coordinates are >= 16, so truncation is floor
      const float X = (float)(pt_x(p) + kMinBorder) * s, Y = (float)(pt_y(p) + kMinBorder) * s;
      const int x = min(xmax, (int)X), y = min(ymax, (int)Y);
      keep = m[(uint64_t)y * mstep + x] != 0;
    }
    const unsigned long long b = __ballot(keep);
    if (keep) list[nout + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] = p;
    nout += __popcll(b);
  }
  if (lane == 0 && nout != n) *countp = nout;
}

void launch_cand_mask(const Geom* d_geom, const Cell* d_cells, const CandMask& mk, uint32_t* cand, int* cellCount, int nimg, int c0, int c1,
                      hipStream_t st) {
  if (c1 <= c0 || nimg <= 0) return;
  hipLaunchKernelGGL(k_cand_mask, dim3((c1 - c0 + 3) / 4, nimg), dim3(256), 0, st, d_geom, d_cells, mk.mask, mk.step, mk.fstride, cand, cellCount,
                     c0, c1);
}

}  // namespace dvs
