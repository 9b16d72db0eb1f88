// dvslam/mapping_backend.hpp — the backend node's map (backend.cpp) as an object over dvs_backend_* (dvslam_hip.h; INTEGRATION.md
// "Mapping backend"): addKeyframe() is syncCallback without the ROS and marker parts, bundleAdjust() is bundleAdjustmentCallback.  The
// landmark and observation tables live on the device; class names are interned here (0 = "unlabeled").  One stated deviation from the
// reference: among candidates with EXACTLY equal reprojection error the lowest landmark id wins (the reference's unordered_map order is
// not reproduced).  Not thread-safe: the caller serialises addKeyframe and bundleAdjust.  Not copyable.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "sliding_window_ba.hpp"

namespace dvslam {

struct Detection {            // yolo_msgs Detection: bbox centre and size in pixels, class_name
  double cx, cy, w, h;
  std::string class_name;
};

struct MapLandmarks {
  std::vector<uint64_t> id; std::vector<int32_t> class_id, observation_count; std::vector<float> xyz; std::vector<uint8_t> desc;
  std::vector<int64_t> last_seen_ns, obs_offsets; std::vector<uint64_t> obs_ids;
};
struct MapObservations {
  std::vector<uint64_t> id, frame_id, landmark_id; std::vector<float> px; std::vector<uint8_t> desc; std::vector<int32_t> class_id;
};
struct MapKeyframes {
  std::vector<uint64_t> frame_id, obs_ids; std::vector<int64_t> stamp_ns, obs_offsets; std::vector<double> R, t;
};
// dvslam_hip.h "Loop closing on the map": a loop as the pose graph takes it (x_query = R_z x_entry + t_z, rvec = Log(R_z)), the graph the
// keyframes imply as the arrays of dvs_pgo_set_nodes / dvs_pgo_set_edges, the anchors, and the pairs a fusion kept
struct MapLoop {
  uint64_t query_frame_id, entry_frame_id;
  double rvec[3], tvec[3], w_rot, w_trans;
};
struct MapPoseGraph {
  std::vector<double> R, t, rvec, tvec, w_rot, w_trans; std::vector<uint8_t> fixed; std::vector<int32_t> ei, ej;
};
struct MapAnchors {
  std::vector<uint64_t> id; std::vector<int32_t> keyframe;
};
struct MapFusion {
  dvs_fuse_result counts;
  std::vector<uint64_t> survivor_id, removed_id; std::vector<double> error;   // ascending removed id
};

class MappingBackend {
 public:
  static dvs_backend_params defaultParams(double fx, double fy, double cx, double cy) {
    dvs_backend_params p;
    dvs_backend_default_params(&p);
    p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
    return p;
  }
  // filtered: filtered_objects_ by name (the reference filters "person"); p.n_filtered / p.filtered_class_ids are set from it
  explicit MappingBackend(dvs_backend_params p, const std::vector<std::string>& filtered = {"person"}, int device = 0) : device_(device) {
    names_.push_back("unlabeled"); ids_["unlabeled"] = 0;
    if (filtered.size() > DVS_BACKEND_MAX_FILTERED) throw std::invalid_argument("MappingBackend: too many filtered classes");
    p.n_filtered = (int32_t)filtered.size();
    for (size_t k = 0; k < filtered.size(); k++) p.filtered_class_ids[k] = intern(filtered[k]);
    params_ = p;
    if (dvs_backend_create(&params_, device, &h_) != DVS_OK) throw std::runtime_error(std::string("dvs_backend_create: ") + dvs_last_error());
  }
  ~MappingBackend() { dvs_backend_destroy(h_); }
  MappingBackend(const MappingBackend&) = delete;
  MappingBackend& operator=(const MappingBackend&) = delete;

  int32_t intern(const std::string& name) {
    const auto it = ids_.find(name);
    if (it != ids_.end()) return it->second;
    const int32_t id = (int32_t)names_.size();
    names_.push_back(name); ids_[name] = id;
    return id;
  }
  const std::string& className(int32_t id) const { return names_.at((size_t)id); }

  // payload: the Keyframe.msg CDR bytes (TrackingFrontend::track's, or a received SerializedMessage); detections in message order
  dvs_backend_result addKeyframe(const std::vector<uint8_t>& payload, const std::vector<Detection>& detections) {
    std::vector<dvs_detection> det(detections.size());
    for (size_t k = 0; k < det.size(); k++) det[k] = dvs_detection{detections[k].cx, detections[k].cy, detections[k].w, detections[k].h, intern(detections[k].class_name), 0};
    dvs_backend_result r;
    check(dvs_backend_add_keyframe_cdr(h_, payload.data(), payload.size(), det.data(), (int32_t)det.size(), &r), "dvs_backend_add_keyframe_cdr");
    return r;
  }

  // bundleAdjustmentCallback (:874-989) with nothing skipped when fewer than two keyframes are stored: window -> SlidingWindowBA::optimize(…, 20)
  // -> updateOptimizedResults on success -> pruneLandmarks at `now`
  OptimizationResult bundleAdjust(int32_t now_sec, uint32_t now_nanosec, int32_t* removed_landmarks = nullptr, int32_t* removed_observations = nullptr) {
    dvs_backend_count c;
    check(dvs_backend_counts(h_, &c), "dvs_backend_counts");
    const int32_t ck = params_.window, co = (int32_t)c.n_observations, cl = (int32_t)c.n_landmarks;
    std::vector<uint64_t> kid((size_t)ck), olm((size_t)co), ofr((size_t)co), lid((size_t)cl);
    std::vector<double> R((size_t)ck * 9), t((size_t)ck * 3);
    std::vector<float> px((size_t)co * 2), xyz((size_t)cl * 3);
    std::vector<int32_t> ocl((size_t)co), lcl((size_t)cl);
    int32_t nk = 0, no = 0, nl = 0;
    check(dvs_backend_get_window(h_, ck, co, cl, kid.data(), R.data(), t.data(), &nk, px.data(), olm.data(), ocl.data(), ofr.data(), nullptr, &no, lid.data(), lcl.data(),
                                 xyz.data(), &nl), "dvs_backend_get_window");
    std::vector<KeyframeData> kfs; std::vector<Landmark> lms; std::vector<Observation> obs;
    for (int32_t k = 0; k < nk; k++) kfs.emplace_back((int)kid[(size_t)k], &R[9 * (size_t)k], &t[3 * (size_t)k]);
    for (int32_t k = 0; k < nl; k++) lms.emplace_back(lid[(size_t)k], className(lcl[(size_t)k]), xyz[3 * (size_t)k], xyz[3 * (size_t)k + 1], xyz[3 * (size_t)k + 2], false);
    for (int32_t k = 0; k < no; k++) obs.emplace_back(px[2 * (size_t)k], px[2 * (size_t)k + 1], olm[(size_t)k], className(ocl[(size_t)k]), (int)ofr[(size_t)k]);
    if (!ba_) ba_.reset(new SlidingWindowBA(params_.fx, params_.fy, params_.cx, params_.cy));
    OptimizationResult res = ba_->optimize(kfs, lms, obs, 20);
    if (res.success) {
      std::vector<uint64_t> fid, ids; std::vector<double> Ro, to, X; std::vector<int32_t> cls;
      for (const auto& kv : res.optimized_poses) { fid.push_back((uint64_t)kv.first); Ro.insert(Ro.end(), kv.second.R, kv.second.R + 9); to.insert(to.end(), kv.second.t, kv.second.t + 3); }
      for (const auto& kv : res.optimized_landmarks) { ids.push_back(kv.first.first); cls.push_back(intern(kv.first.second)); X.insert(X.end(), kv.second.begin(), kv.second.end()); }
      check(dvs_backend_apply_optimized(h_, (int32_t)fid.size(), fid.data(), Ro.data(), to.data(), (int32_t)ids.size(), ids.data(), cls.data(), X.data()),
            "dvs_backend_apply_optimized");
    }
    int32_t rl = 0, ro = 0;
    check(dvs_backend_prune(h_, now_sec, now_nanosec, &rl, &ro), "dvs_backend_prune");
    if (removed_landmarks) *removed_landmarks = rl;
    if (removed_observations) *removed_observations = ro;
    return res;
  }

  dvs_backend_count counts() const {
    dvs_backend_count c;
    check(dvs_backend_counts(h_, &c), "dvs_backend_counts");
    return c;
  }
  MapLandmarks landmarks() const {
    const dvs_backend_count c = counts();
    const size_t n = (size_t)c.n_landmarks, m = (size_t)c.n_observations;
    MapLandmarks L;
    L.id.resize(n); L.class_id.resize(n); L.observation_count.resize(n); L.xyz.resize(n * 3); L.desc.resize(n * 32); L.last_seen_ns.resize(n);
    L.obs_offsets.resize(n + 1); L.obs_ids.resize(m);
    int32_t nn = 0; int64_t nm = 0;
    check(dvs_backend_get_landmarks(h_, (int32_t)n, (int64_t)m, L.id.data(), L.class_id.data(), L.xyz.data(), L.desc.data(), L.observation_count.data(),
                                    L.last_seen_ns.data(), L.obs_offsets.data(), L.obs_ids.data(), &nn, &nm), "dvs_backend_get_landmarks");
    L.obs_ids.resize((size_t)nm);
    return L;
  }
  MapObservations observations() const {
    const size_t n = (size_t)counts().n_observations;
    MapObservations O;
    O.id.resize(n); O.frame_id.resize(n); O.landmark_id.resize(n); O.px.resize(n * 2); O.desc.resize(n * 32); O.class_id.resize(n);
    int32_t nn = 0;
    check(dvs_backend_get_observations(h_, (int32_t)n, O.id.data(), O.frame_id.data(), O.px.data(), O.desc.data(), O.class_id.data(), O.landmark_id.data(), &nn),
          "dvs_backend_get_observations");
    return O;
  }
  MapKeyframes keyframes() const {
    const dvs_backend_count c = counts();
    const size_t n = (size_t)c.n_keyframes, m = (size_t)c.n_observations;
    MapKeyframes K;
    K.frame_id.resize(n); K.stamp_ns.resize(n); K.R.resize(n * 9); K.t.resize(n * 3); K.obs_offsets.resize(n + 1); K.obs_ids.resize(m);
    int32_t nn = 0; int64_t nm = 0;
    check(dvs_backend_get_keyframes(h_, (int32_t)n, (int64_t)m, K.frame_id.data(), K.stamp_ns.data(), K.R.data(), K.t.data(), K.obs_offsets.data(), K.obs_ids.data(),
                                    &nn, &nm), "dvs_backend_get_keyframes");
    K.obs_ids.resize((size_t)nm);
    return K;
  }
  // the keyframe index (row of keyframes()) of every landmark's lowest-id observation, -1 without one; landmarks in ascending id
  MapAnchors anchors() const {
    const size_t n = (size_t)counts().n_landmarks;
    MapAnchors A;
    A.id.resize(n); A.keyframe.resize(n);
    int32_t nn = 0;
    check(dvs_backend_get_anchors(h_, (int32_t)n, A.id.data(), A.keyframe.data(), &nn), "dvs_backend_get_anchors");
    return A;
  }
  // all keyframes as nodes (node 0 fixed), odometry edges between consecutive keyframes, then the loops in the order given
  MapPoseGraph buildPoseGraph(const std::vector<MapLoop>& loops, double odo_w_rot, double odo_w_trans) const {
    std::vector<uint64_t> q, e; std::vector<double> rv, tv, wr, wt;
    for (const MapLoop& l : loops) {
      q.push_back(l.query_frame_id); e.push_back(l.entry_frame_id); rv.insert(rv.end(), l.rvec, l.rvec + 3); tv.insert(tv.end(), l.tvec, l.tvec + 3);
      wr.push_back(l.w_rot); wt.push_back(l.w_trans);
    }
    const size_t cn = (size_t)counts().n_keyframes, ce = cn + loops.size();
    MapPoseGraph G;
    G.R.resize(cn * 9); G.t.resize(cn * 3); G.fixed.resize(cn); G.ei.resize(ce); G.ej.resize(ce); G.rvec.resize(ce * 3); G.tvec.resize(ce * 3); G.w_rot.resize(ce);
    G.w_trans.resize(ce);
    int32_t nn = 0, ne = 0;
    check(dvs_backend_build_pose_graph(h_, (int32_t)loops.size(), q.data(), e.data(), rv.data(), tv.data(), wr.data(), wt.data(), odo_w_rot, odo_w_trans, (int32_t)cn,
                                       (int32_t)ce, G.R.data(), G.t.data(), G.fixed.data(), G.ei.data(), G.ej.data(), G.rvec.data(), G.tvec.data(), G.w_rot.data(),
                                       G.w_trans.data(), &nn, &ne), "dvs_backend_build_pose_graph");
    G.ei.resize((size_t)ne); G.ej.resize((size_t)ne); G.rvec.resize((size_t)ne * 3); G.tvec.resize((size_t)ne * 3); G.w_rot.resize((size_t)ne); G.w_trans.resize((size_t)ne);
    return G;
  }
  // landmarks seen from the entry keyframes merged into the duplicates the query keyframe created (apply = false: a dry run)
  MapFusion fuse(uint64_t query_frame_id, const std::vector<uint64_t>& entry_frame_ids, const dvs_fuse_params* params = nullptr, bool apply = true) {
    const size_t cap = (size_t)counts().n_landmarks;
    MapFusion F;
    F.survivor_id.resize(cap + 1); F.removed_id.resize(cap + 1); F.error.resize(cap + 1);
    int32_t n = 0;
    check(dvs_backend_fuse(h_, query_frame_id, entry_frame_ids.data(), (int32_t)entry_frame_ids.size(), params, apply ? 1 : 0, &F.counts, (int32_t)cap,
                           F.survivor_id.data(), F.removed_id.data(), F.error.data(), &n), "dvs_backend_fuse");
    F.survivor_id.resize((size_t)n); F.removed_id.resize((size_t)n); F.error.resize((size_t)n);
    return F;
  }
  dvs_backend* handle() const { return h_; }
  const dvs_backend_params& params() const { return params_; }

 private:
  static void check(dvs_status st, const char* what) {
    if (st != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
  }
  dvs_backend_params params_;
  dvs_backend* h_ = nullptr;
  int device_ = 0;
  std::vector<std::string> names_;
  std::map<std::string, int32_t> ids_;
  std::unique_ptr<SlidingWindowBA> ba_;
};

}  // namespace dvslam
