// ransac_layout.h — the problem record of the robust estimators of ransac.hip, their limits, and how each of them lays its arrays out in
// ONE block: scratch slot 0 of the matcher context on the device, and the mirror of that block's [in | out] in the context's pinned block.
// A layout is stated once and carved by the host batch bodies and by the device forms of ransac_device.h alike; nothing outside this
// header computes an address inside such a block.  Needs device_mem.h alone (a stand-alone host program can include it).
#pragma once
#include <stddef.h>
#include <string.h>
#include "device_mem.h"

namespace dvs {

// One RANSAC problem of a batch (blockIdx.y of every kernel of ransac.hip): its correspondences are rows [off, off + n) of the point
// arrays, its hypotheses / counts / results slot `b` of the per-problem arrays.  The single-problem entry points are batches of one.
// 16 bytes.  The 64-bit word is the sampler's seed in the library's own estimators (and loop_verify.hip); in the OpenCV-procedure
// forms, whose samples the host draws, it is the number of iterations that HAVE a sample (k_ransac_select's capInSeed = 1 reads it).
struct RansacProb {
  int off, n;
  unsigned long long seed;
  __host__ __device__ static RansacProb seeded(int off, int n, unsigned long long seed) { return RansacProb{off, n, seed}; }
  __host__ __device__ static RansacProb sampled(int off, int n, int iterations) { return RansacProb{off, n, (unsigned long long)iterations}; }
  __host__ __device__ int sampled_iterations() const { return (int)seed; }
};
static_assert(sizeof(RansacProb) == 16, "the problem record is one 16-byte block of a layout's in region");

// ---- limits and sizes, for the host entry points and the device forms alike
constexpr int kFmMaxIters = 4096, kPnpMaxIters = 1024;   // hypotheses of one call (per problem)
constexpr int kFmOwnMinPoints = 8;                        // normalised 8-point
constexpr int kFmCvMinPoints = 8, kFmCvRansacPoints = 15; // cv::findFundamentalMat: LMedS for 8 .. 14, RANSAC from 15 on
constexpr int kFmCvFirstPass = 96;                        // iterations whose models the first RANSAC pass fits
constexpr int kPnpOwnMinPoints = 4, kPnpCvMinPoints = 6;
constexpr int kF7Roots = 3, kP3pPoses = 4;                // candidate models per sample: 7-point cubic, P3P quartic
constexpr int kFmModel = 9, kPosePnp = 12, kModelPnpCv = 18, kSel = 4;   // doubles per F / (R, t) / (rvec, tvec, R, pad); ints per select record
constexpr size_t kFmModelBytes = kFmModel * sizeof(double), kPosePnpBytes = kPosePnp * sizeof(double), kModelPnpCvBytes = kModelPnpCv * sizeof(double);
constexpr size_t kPnpRecord = 64;                        // bytes of a PnpRecord
constexpr size_t kScratchSlack = 64;                      // requested behind a device layout's last array

// The result of one PnP problem, as k_pnp_refine / k_pnpcv_refit write it and every host reader sees it.  rvec / tvec are meaningful where
// the estimator succeeded (the OpenCV-procedure form: wherever a model was selected); k_pnp_refine never writes `unused`.
struct PnpRecord { int32_t n_inliers, success; int32_t unused[2]; double rvec[3], tvec[3]; };
static_assert(sizeof(PnpRecord) == kPnpRecord && offsetof(PnpRecord, rvec) == 16 && offsetof(PnpRecord, tvec) == 40, "the 64-byte PnP result record");
// What k_ransac_select leaves per problem: 16 bytes.  `more`: the loop wanted more iterations than it had models for (LMedS: it succeeded).
struct SelRecord { int32_t best /* or -1 */, iterations, inliers, more; };
static_assert(sizeof(SelRecord) == kSel * sizeof(int), "the 16-byte select record");

// Which regions a block holds.  `points`: the correspondences and the per-correspondence results lie in the block (a host batch) or at
// addresses of the caller's (a device form, which imports [problem records | samples] alone).  `work`: the device-only arrays.
struct RansacRegions { bool points, work; };
constexpr RansacRegions kBatchDevice{true, true}, kBatchPinned{true, false}, kFormDevice{false, true}, kFormPinned{false, false};

// Alignment, for every (nprob >= 1, total >= 0, H >= 1): the in region is carved in units of 16 bytes from a base that hipMalloc /
// hipHostMalloc align far beyond that, so the problem records, every imported array and the end of the region sit on 16 bytes.  Behind
// it the unit is 4 bytes, and every double array is preceded only by the in region, by double arrays, by PAIRS of int arrays of equal
// length (valid + counts) and by 16-byte select records: every double* member sits on 8 bytes.  (Behind an odd number of
// OpenCV-procedure models the 64-byte PnP result records sit on 4: the device stores through them as it did, the host copies one out.)

// Fundamental matrix, own (cv = false: no samples, H models per problem) and OpenCV-procedure (7-point samples, 3 H models):
//   in   [problem records | pts1 | pts2 | samples 7 x H per problem]            imported
//   work [models 9 doubles each | valid | counts]                                device only
//   out  [select records | best model 9 doubles per problem | mask]              fetched (a device form: the select record, if anything)
struct FmLayout {
  RansacProb* probs = nullptr; float *p1 = nullptr, *p2 = nullptr; int32_t* samples = nullptr;
  double* models = nullptr; int *valid = nullptr, *counts = nullptr;
  int* sel = nullptr; double* F = nullptr; uint8_t* mask = nullptr;
  size_t sampb = 0, inb = 0, outb = 0, bytes = 0;   // the samples block, in, out, everything
  FmLayout() = default;
  FmLayout(uint8_t* base, RansacRegions r, bool cv, int nprob, int total, int H) {
    const size_t nsamples = (size_t)nprob * H, nmodels = cv ? kF7Roots * nsamples : nsamples;
    Carver c{base, 16};
    c.take(probs, nprob);
    if (r.points) { c.take(p1, 2 * (size_t)total); c.take(p2, 2 * (size_t)total); }
    sampb = c.used;
    if (cv) c.take(samples, 7 * nsamples);
    inb = c.used; sampb = inb - sampb;
    c.align = 4;
    if (r.work) { c.take(models, kFmModel * nmodels); c.take(valid, nmodels); c.take(counts, nmodels); }
    const size_t out0 = c.used;
    c.take(sel, kSel * (size_t)nprob); c.take(F, kFmModel * (size_t)nprob);
    if (r.points) c.take(mask, total);
    outb = c.used - out0; bytes = c.used;
  }
  // out of the fetched region: inlier counts (0 where nothing was selected), models, masks
  void unpack(int nprob, int total, double* F9, uint8_t* inlier_mask, int32_t* n_inliers) const {
    for (int b = 0; b < nprob; b++)
      if (n_inliers) n_inliers[b] = sel[kSel * b] >= 0 ? sel[kSel * b + 2] : 0;
    if (F9) memcpy(F9, F, (size_t)nprob * kFmModel * sizeof(double));
    if (total) memcpy(inlier_mask, mask, (size_t)total);
  }
};

// PnP, own (cv = false: P3P, 4 H poses per problem, the select records are work) and OpenCV-procedure (5-point EPnP samples, H models,
// no `valid`, the select records are results):
//   in   [problem records | object points | image points | samples 5 x H per problem]
//   work own [poses 12 doubles each | valid | counts | select records]     cv [models 18 doubles each | counts]
//   out  [result records 64 bytes per problem | inlier lists, concatenated like the points | cv: select records]
struct PnpLayout {
  RansacProb* probs = nullptr; float *obj = nullptr, *img = nullptr; int32_t* samples = nullptr;
  double* models = nullptr; int *valid = nullptr, *counts = nullptr;
  PnpRecord* rec = nullptr; int *inl = nullptr, *sel = nullptr;
  size_t sampb = 0, inb = 0, outb = 0, bytes = 0;
  PnpLayout() = default;
  PnpLayout(uint8_t* base, RansacRegions r, bool cv, int nprob, int total, int H) {
    const size_t nsamples = (size_t)nprob * H, nmodels = cv ? nsamples : kP3pPoses * nsamples;
    Carver c{base, 16};
    c.take(probs, nprob);
    if (r.points) { c.take(obj, 3 * (size_t)total); c.take(img, 2 * (size_t)total); }
    sampb = c.used;
    if (cv) c.take(samples, 5 * nsamples);
    inb = c.used; sampb = inb - sampb;
    c.align = 4;
    if (r.work && cv) { c.take(models, kModelPnpCv * nmodels); c.take(counts, nmodels); }
    if (r.work && !cv) { c.take(models, kPosePnp * nmodels); c.take(valid, nmodels); c.take(counts, nmodels); c.take(sel, kSel * (size_t)nprob); }
    const size_t out0 = c.used;
    if (r.points) {
      c.take(rec, nprob); c.take(inl, total);
      if (cv) c.take(sel, kSel * (size_t)nprob);
    }
    outb = c.used - out0; bytes = c.used;
  }
  // out of the fetched region; a pose is written where the estimator succeeded, or (the cv form, whose select records are fetched)
  // wherever a model was selected
  void unpack(int nprob, const int32_t* offsets, bool by_sel, double* rvec3, double* tvec3, int32_t* inliers, int32_t* n_inliers, int32_t* success) const {
    for (int b = 0; b < nprob; b++) {
      PnpRecord r;
      memcpy(&r, rec + b, sizeof(r));   // (a record may sit on 4 bytes)
      if (n_inliers) n_inliers[b] = r.n_inliers;
      success[b] = r.success;
      if (by_sel ? sel[kSel * b] >= 0 : r.success != 0) { memcpy(rvec3 + 3 * (size_t)b, r.rvec, sizeof(r.rvec)); memcpy(tvec3 + 3 * (size_t)b, r.tvec, sizeof(r.tvec)); }
      if (inliers && r.n_inliers > 0) memcpy(inliers + offsets[b], inl + offsets[b], (size_t)r.n_inliers * sizeof(int));
    }
  }
};

}  // namespace dvs
