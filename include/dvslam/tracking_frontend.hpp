// dvslam/tracking_frontend.hpp — Frontend::syncCallback (frontend.cpp:1068-1324) as an object: one track() per RGB-D frame, everything
// between the image upload and the result resident on the device (dvs_tracker_* of dvslam_hip.h; INTEGRATION.md "Tracking front end").
// The members syncCallback keeps — R_, t_, prev_kps_, prev_descriptors_, prev_frame_depth_, the last keyframe's features,
// frames_since_last_keyframe_, keyframe_id_ — live in the handle.  Not thread-safe; not copyable.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#ifdef DVSLAM_WITH_OPENCV
#include <opencv2/core/core.hpp>
#endif

namespace dvslam {

struct TrackResult {
  dvs_track_result r;             // counts, flags, rvec / tvec, R_ (row-major) / t_ after the frame, keyframe id
  std::vector<uint8_t> payload;   // Keyframe.msg CDR bytes when r.is_keyframe (hand them to publish_serialized_message), else empty
  bool isKeyframe() const { return r.is_keyframe != 0; }
  bool poseUpdated() const { return r.pose_updated != 0; }
};

class TrackingFrontend {
 public:
  // the reference's constants for the given frame size and intrinsics; change fields of the returned struct before constructing
  static dvs_tracker_params defaultParams(int rows, int cols, double fx, double fy, double cx, double cy) {
    dvs_tracker_params p;
    dvs_tracker_default_params(&p);
    p.rows = rows; p.cols = cols; p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
    return p;
  }
  explicit TrackingFrontend(const dvs_tracker_params& params, int device = 0) : params_(params) {
    if (dvs_tracker_create(&params, device, &h_) != DVS_OK) throw std::runtime_error(std::string("dvs_tracker_create: ") + dvs_last_error());
    cdr_.resize(dvs_keyframe_cdr_capacity("camera_link", params.orb.nfeatures + 3 * params.orb.nlevels));
  }
  ~TrackingFrontend() { dvs_tracker_destroy(h_); }
  TrackingFrontend(const TrackingFrontend&) = delete;
  TrackingFrontend& operator=(const TrackingFrontend&) = delete;

  // image: 8UC1 (channels 1) or BGR 8UC3 (channels 3), `step` bytes between rows; depth: 16UC1 millimetres
  TrackResult track(const uint8_t* image, int channels, size_t step, const uint16_t* depth, size_t depth_step, int32_t stamp_sec = 0,
                    uint32_t stamp_nanosec = 0) {
    TrackResult out;
    const dvs_status st = dvs_tracker_track(h_, image, channels, step, depth, depth_step, stamp_sec, stamp_nanosec, &out.r, cdr_.data(), cdr_.size());
    if (st != DVS_OK) throw std::runtime_error(std::string("dvs_tracker_track: ") + dvs_last_error());
    if (out.r.is_keyframe) out.payload.assign(cdr_.begin(), cdr_.begin() + (size_t)out.r.cdr_bytes);
    return out;
  }
  void reset() {
    if (dvs_tracker_reset(h_) != DVS_OK) throw std::runtime_error(std::string("dvs_tracker_reset: ") + dvs_last_error());
  }
  // the last frame's culled feature set (what a keyframe carries), in order; sel = indices into the depth-filtered set
  int backendFeatures(std::vector<dvs_keypoint>& kps, std::vector<uint8_t>& desc, std::vector<int32_t>* sel = nullptr) {
    const int cap = params_.orb.nfeatures + 3 * params_.orb.nlevels;
    kps.resize((size_t)cap); desc.resize((size_t)cap * 32);
    if (sel) sel->resize((size_t)cap);
    int32_t n = 0;
    if (dvs_tracker_get_backend_features(h_, kps.data(), desc.data(), sel ? sel->data() : nullptr, cap, &n) != DVS_OK)
      throw std::runtime_error(std::string("dvs_tracker_get_backend_features: ") + dvs_last_error());
    kps.resize((size_t)n); desc.resize((size_t)n * 32);
    if (sel) sel->resize((size_t)n);
    return n;
  }
  // the motion-mask opt-in (dvs_tracker_set_motion_mask): p's size and intrinsics are replaced by the tracker's, lag in 1..16; nullptr: off
  void setMotionMask(const dvs_motion_params* p, int lag = 4) {
    if (dvs_tracker_set_motion_mask(h_, p, lag) != DVS_OK) throw std::runtime_error(std::string("dvs_tracker_set_motion_mask: ") + dvs_last_error());
  }
  // what the last frame's extraction used: the mask (rows x cols packed; all 255 when none), the relative pose, the statistics; returns
  // the reference's frame index, -1 when the extraction was unmasked
  int64_t motionMask(std::vector<uint8_t>& mask, double* R9 = nullptr, double* t3 = nullptr, dvs_motion_stats* stats = nullptr) {
    mask.resize((size_t)params_.rows * (size_t)params_.cols);
    int64_t ref = -1;
    if (dvs_tracker_get_motion_mask(h_, mask.data(), (size_t)params_.cols, R9, t3, &ref, stats) != DVS_OK)
      throw std::runtime_error(std::string("dvs_tracker_get_motion_mask: ") + dvs_last_error());
    return ref;
  }
  dvs_tracker* handle() const { return h_; }
  const dvs_tracker_params& params() const { return params_; }

#ifdef DVSLAM_WITH_OPENCV
  // syncCallback's own types: current_frame_rgb (CV_8UC3 BGR, or CV_8UC1) and current_frame_depth (CV_16UC1)
  TrackResult track(const cv::Mat& image, const cv::Mat& depth, int32_t stamp_sec = 0, uint32_t stamp_nanosec = 0) {
    if (image.empty() || depth.empty() || image.rows != params_.rows || image.cols != params_.cols || depth.rows != params_.rows || depth.cols != params_.cols)
      throw std::invalid_argument("TrackingFrontend::track: image / depth size differs from the tracker's");
    const int ch = (image.type() >> 3) + 1;   // CV_MAT_CN / CV_MAT_DEPTH of the type code
    if ((image.type() & 7) != 0 /* CV_8U */ || (ch != 1 && ch != 3) || depth.type() != 2 /* CV_16UC1 */)
      throw std::invalid_argument("TrackingFrontend::track: 8UC1 / 8UC3 image and 16UC1 depth wanted");
    return track(image.data, ch, (size_t)image.step, reinterpret_cast<const uint16_t*>(depth.data), (size_t)depth.step, stamp_sec, stamp_nanosec);
  }
#endif

 private:
  dvs_tracker_params params_;
  dvs_tracker* h_ = nullptr;
  std::vector<uint8_t> cdr_;
};

}  // namespace dvslam
