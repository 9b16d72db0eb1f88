// dvslam/pose_graph.hpp — header-only C++ adapter over dvs_pgo_* of dvslam_hip.h ("Pose-graph optimisation"; INTEGRATION.md "Loop
// closure"): the consumer of a verified loop.  Nodes are keyframe poses (R, t) with x_world = R x + t, the layout MappingBackend::keyframes()
// returns; an edge (i, j, R_z, t_z) states x_i = R_z x_j + t_z; addLoop takes a verified LoopCandidate as it is (x_query = R x_entry + t).
// optimize() runs Levenberg-Marquardt on the device; correctPoints() moves landmarks along with their anchor keyframes.  The graph is
// collected on the host and handed over by optimize(): nodes or edges added afterwards take effect at the next optimize(), which starts
// again from the poses as added.  Errors throw std::runtime_error.  Not thread-safe, not copyable.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../dvslam_hip.h"
#include "loop_detection.hpp"

namespace dvslam {

#ifndef DVSLAM_POSE_DEFINED   // sliding_window_ba.hpp defines the same struct: a translation unit may include both
#define DVSLAM_POSE_DEFINED
struct Pose {
  double R[9];   // row-major
  double t[3];
};
#endif

class PoseGraph {
 public:
  explicit PoseGraph(int device = 0) {
    if (dvs_pgo_create(device, &h_) != DVS_OK) throw std::runtime_error(std::string("dvs_pgo_create: ") + dvs_last_error());
    dvs_pgo_default_params(&params_);
  }
  ~PoseGraph() { dvs_pgo_destroy(h_); }
  PoseGraph(const PoseGraph&) = delete;
  PoseGraph& operator=(const PoseGraph&) = delete;

  dvs_pgo_params& params() { return params_; }
  int nodes() const { return (int)fixed_.size(); }
  int edges() const { return (int)ei_.size(); }

  // returns the node's index
  int addNode(const double* R9, const double* t3, bool fixed = false) {
    R_.insert(R_.end(), R9, R9 + 9); t_.insert(t_.end(), t3, t3 + 3); fixed_.push_back(fixed ? 1 : 0);
    dirty_ = true;
    return nodes() - 1;
  }
  // x_i = R x_j + t; the rotation goes to the C-ABI as its principal rotation vector
  void addEdge(int i, int j, const double* R9, const double* t3, double w_rot, double w_trans) {
    double w[3];
    rotationVector(R9, w);
    ei_.push_back(i); ej_.push_back(j);
    rvec_.insert(rvec_.end(), w, w + 3); tvec_.insert(tvec_.end(), t3, t3 + 3);
    wrot_.push_back(w_rot); wtrans_.push_back(w_trans);
    dirty_ = true;
  }
  // a verified loop between keyframe node `query` and the node of the candidate's entry: the edge (query, entry, c.R, c.t) unchanged
  void addLoop(int query, int entry, const LoopCandidate& c, double w_rot, double w_trans) {
    if (!c.verified) throw std::runtime_error("PoseGraph::addLoop: the candidate is not verified");
    addEdge(query, entry, c.R, c.t, w_rot, w_trans);
  }

  dvs_pgo_summary optimize() {
    upload();
    dvs_pgo_summary s;
    check(dvs_pgo_solve(h_, &params_, &s), "dvs_pgo_solve");
    return s;
  }
  double cost() {
    upload();
    double c = 0;
    check(dvs_pgo_evaluate(h_, &c, nullptr, nullptr, nullptr, nullptr), "dvs_pgo_evaluate");
    return c;
  }
  // the current pose of node i (after optimize(): the optimised one)
  Pose pose(int i) {
    upload();
    if (i < 0 || i >= nodes()) throw std::out_of_range("PoseGraph::pose");
    std::vector<double> R((size_t)nodes() * 9), t((size_t)nodes() * 3);
    check(dvs_pgo_get_nodes(h_, R.data(), t.data()), "dvs_pgo_get_nodes");
    Pose p;
    for (int k = 0; k < 9; k++) p.R[k] = R[9 * (size_t)i + k];
    for (int k = 0; k < 3; k++) p.t[k] = t[3 * (size_t)i + k];
    return p;
  }
  std::vector<Pose> poses() {
    upload();
    std::vector<double> R((size_t)nodes() * 9), t((size_t)nodes() * 3);
    check(dvs_pgo_get_nodes(h_, R.data(), t.data()), "dvs_pgo_get_nodes");
    std::vector<Pose> out((size_t)nodes());
    for (size_t i = 0; i < out.size(); i++) {
      for (int k = 0; k < 9; k++) out[i].R[k] = R[9 * i + k];
      for (int k = 0; k < 3; k++) out[i].t[k] = t[3 * i + k];
    }
    return out;
  }
  // xyz: n points (x, y, z) in the world frame, moved in place with their anchor nodes from the poses as added to the current ones; an
  // anchor outside [0, nodes()) leaves its point as it is
  void correctPoints(float* xyz, const int32_t* anchor, int n) {
    upload();
    check(dvs_pgo_correct_points(h_, n, xyz, anchor), "dvs_pgo_correct_points");
  }
  void correctPoints(std::vector<std::array<float, 3>>& points, const std::vector<int32_t>& anchor) {
    if (points.size() != anchor.size()) throw std::invalid_argument("PoseGraph::correctPoints: one anchor per point");
    if (!points.empty()) correctPoints(points[0].data(), anchor.data(), (int)points.size());
  }
  std::vector<std::array<double, 7>> trace() const {
    int32_t n = 0;
    check(dvs_pgo_get_trace(h_, nullptr, 0, &n), "dvs_pgo_get_trace");
    std::vector<std::array<double, 7>> rows((size_t)n);
    if (n) check(dvs_pgo_get_trace(h_, rows[0].data(), n, &n), "dvs_pgo_get_trace");
    return rows;
  }
  dvs_pgo* handle() const { return h_; }

  // principal rotation vector of a rotation matrix by the library's own Log (dvslam_hip.h): angles up to about 3.1 rad
  static void rotationVector(const double* R, double* w) {
    const double v[3] = {(R[7] - R[5]) / 2, (R[2] - R[6]) / 2, (R[3] - R[1]) / 2};
    const double s = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), c = (R[0] + R[4] + R[8] - 1) / 2;
    const double k = s > 1e-12 ? std::atan2(s, c) / s : 1.0;
    for (int a = 0; a < 3; a++) w[a] = v[a] * k;
  }

 private:
  static void check(dvs_status st, const char* what) {
    if (st != DVS_OK) throw std::runtime_error(std::string(what) + ": " + dvs_last_error());
  }
  void upload() {
    if (!dirty_) return;
    check(dvs_pgo_set_nodes(h_, nodes(), R_.data(), t_.data(), fixed_.data()), "dvs_pgo_set_nodes");
    if (edges())
      check(dvs_pgo_set_edges(h_, edges(), ei_.data(), ej_.data(), rvec_.data(), tvec_.data(), wrot_.data(), wtrans_.data()), "dvs_pgo_set_edges");
    dirty_ = false;
  }
  dvs_pgo* h_ = nullptr;
  dvs_pgo_params params_;
  std::vector<double> R_, t_, rvec_, tvec_, wrot_, wtrans_;
  std::vector<uint8_t> fixed_;
  std::vector<int32_t> ei_, ej_;
  bool dirty_ = true;
};

}  // namespace dvslam
