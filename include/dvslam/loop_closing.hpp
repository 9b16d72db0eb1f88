// dvslam/loop_closing.hpp — header-only C++ adapter over dvs_backend_close_loop of dvslam_hip.h ("Loop closing on the map"; INTEGRATION.md
// "Loop closure"): verified loops applied to the map a MappingBackend keeps on the device.  closeLoop() solves the pose graph the keyframes
// imply on the caller's PoseGraph handle, writes the poses back, moves every landmark with its anchor keyframe on the device and, if asked,
// fuses the duplicate landmarks the drift created — ORB-SLAM's CorrectLoop and SearchAndFuse as published ideas.  The PoseGraph is used as
// a solver only: nodes and edges added to it through addNode / addEdge are replaced by the backend's graph.  Errors throw
// std::runtime_error.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "loop_detection.hpp"
#include "mapping_backend.hpp"
#include "pose_graph.hpp"

namespace dvslam {

struct LoopEdge : MapLoop {
  LoopEdge() : MapLoop() {}
  LoopEdge(uint64_t query_frame, uint64_t entry_frame, const double* rvec3, const double* tvec3, double w_rot_, double w_trans_) : MapLoop() {
    query_frame_id = query_frame; entry_frame_id = entry_frame; w_rot = w_rot_; w_trans = w_trans_;
    for (int k = 0; k < 3; k++) { rvec[k] = rvec3[k]; tvec[k] = tvec3[k]; }
  }
  // a verified candidate (x_query = R x_entry + t) between the keyframe that was queried and the keyframe of the candidate's entry
  LoopEdge(uint64_t query_frame, uint64_t entry_frame, const LoopCandidate& c, double w_rot_, double w_trans_) : MapLoop() {
    if (!c.verified) throw std::runtime_error("LoopEdge: the candidate is not verified");
    query_frame_id = query_frame; entry_frame_id = entry_frame; w_rot = w_rot_; w_trans = w_trans_;
    PoseGraph::rotationVector(c.R, rvec);
    for (int k = 0; k < 3; k++) tvec[k] = c.t[k];
  }
};
struct OdometryWeights { double w_rot, w_trans; };
struct FuseParams : dvs_fuse_params {
  FuseParams() { dvs_fuse_default_params(this); }
};

inline dvs_close_loop_result closeLoop(MappingBackend& map, PoseGraph& graph, const std::vector<LoopEdge>& loops, OdometryWeights odometry,
                                       const FuseParams* fuse = nullptr) {
  std::vector<uint64_t> q, e; std::vector<double> rv, tv, wr, wt;
  for (const LoopEdge& l : loops) {
    q.push_back(l.query_frame_id); e.push_back(l.entry_frame_id); rv.insert(rv.end(), l.rvec, l.rvec + 3); tv.insert(tv.end(), l.tvec, l.tvec + 3);
    wr.push_back(l.w_rot); wt.push_back(l.w_trans);
  }
  dvs_close_loop_result out;
  if (dvs_backend_close_loop(map.handle(), graph.handle(), (int32_t)loops.size(), q.data(), e.data(), rv.data(), tv.data(), wr.data(), wt.data(), odometry.w_rot,
                             odometry.w_trans, &graph.params(), fuse, &out) != DVS_OK)
    throw std::runtime_error(std::string("dvs_backend_close_loop: ") + dvs_last_error());
  return out;
}

}  // namespace dvslam
