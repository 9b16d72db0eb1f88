// dvslam/motion_segmentation.hpp — motion segmentation from two depth images, their relative pose and the intrinsics, as an object
// (dvs_motion_* of dvslam_hip.h; INTEGRATION.md "Motion segmentation"): the 8-bit keep mask the extractor's masked entry points read,
// 255 = keep, 0 = moving.  The reference has no counterpart (it filters YOLO boxes).  Not thread-safe; not copyable.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"

namespace dvslam {

class MotionSegmenter {
 public:
  // the defaults for the given image size and intrinsics; change fields of the returned struct before constructing
  static dvs_motion_params defaultParams(int rows, int cols, double fx, double fy, double cx, double cy) {
    dvs_motion_params p;
    dvs_motion_default_params(&p);
    p.rows = rows; p.cols = cols; p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
    return p;
  }
  explicit MotionSegmenter(const dvs_motion_params& params, int device = 0) : params_(params) {
    if (dvs_motion_create(&params, device, &h_) != DVS_OK) throw std::runtime_error(std::string("dvs_motion_create: ") + dvs_last_error());
  }
  ~MotionSegmenter() { dvs_motion_destroy(h_); }
  MotionSegmenter(const MotionSegmenter&) = delete;
  MotionSegmenter& operator=(const MotionSegmenter&) = delete;

  void setStream(void* hip_stream) {
    if (dvs_motion_set_stream(h_, hip_stream) != DVS_OK) throw std::runtime_error(std::string("dvs_motion_set_stream: ") + dvs_last_error());
  }
  // host images (16UC1 millimetres, `*_step` bytes between rows), R9 row-major and t3 with X_ref = R X_cur + t -> mask (rows x cols, packed)
  dvs_motion_stats segment(const uint16_t* ref, size_t ref_step, const uint16_t* cur, size_t cur_step, const double* R9, const double* t3,
                           std::vector<uint8_t>& mask) {
    mask.resize((size_t)params_.rows * (size_t)params_.cols);
    dvs_motion_stats st;
    if (dvs_motion_segment(h_, ref, ref_step, cur, cur_step, R9, t3, mask.data(), (size_t)params_.cols, &st) != DVS_OK)
      throw std::runtime_error(std::string("dvs_motion_segment: ") + dvs_last_error());
    return st;
  }
  // device images and mask, asynchronous on the handle's stream; stats != nullptr waits and fills it
  void segmentDevice(const uint16_t* d_ref, size_t ref_step, const uint16_t* d_cur, size_t cur_step, const double* R9, const double* t3, uint8_t* d_mask,
                     size_t mask_step, dvs_motion_stats* stats = nullptr) {
    if (dvs_motion_segment_device(h_, d_ref, ref_step, d_cur, cur_step, R9, t3, d_mask, mask_step, stats) != DVS_OK)
      throw std::runtime_error(std::string("dvs_motion_segment_device: ") + dvs_last_error());
  }
  dvs_motion* handle() const { return h_; }
  const dvs_motion_params& params() const { return params_; }

 private:
  dvs_motion_params params_;
  dvs_motion* h_ = nullptr;
};

}  // namespace dvslam
