// trust_region.h — the trust-region policy and the verdict on one trial step that the four Levenberg-Marquardt solvers follow
// (dvs_ba_solve, dvs_ba_solve_device, dvs_ba_solve_global in ba.hip; dvs_pgo_solve in pose_graph.hip): ceres::Solver defaults
// (trust_region_minimizer.cc / levenberg_marquardt_strategy.cc, Ceres 2.x).  Knows nothing about handles, summaries or streams: a
// solver feeds it one TrialRecord per trial step and gets a StepVerdict and, from the policy, "go on" or a termination code.
#pragma once
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <hip/hip_runtime.h>

namespace dvs {

// What a trial step left behind, wherever its numbers come from (the host's own sums, LmStatus, PgoStatus).  valid: the linear solve
// succeeded and the step is finite; model_change: decrease of the quadratic model along the step (> 0 is the verdict's test); cand_cost:
// cost of the candidate; sn, xn: SQUARED norms of the step and of the point it was taken from.
struct TrialRecord { int valid; double model_change, cand_cost, sn, xn; };

enum StepKind { kStepInvalid = 0, kStepAccepted = 1, kStepRejected = 2, kStepParameterTolerance = 3, kStepFunctionTolerance = 4 };
struct StepVerdict { int kind; double cost_change, rel; };   // zeros where a solver's trace row has zeros

constexpr double kMinRelativeDecrease = 1e-3;
constexpr int kGoOn = -1;   // not a termination code (0 converged, 1 iteration limit, 2 failed)
// what a loop does with an answer of the policy: true to go on, or the termination code into the solver's summary
inline bool go_on(int end, int32_t* termination) {
  if (end != kGoOn) *termination = end;
  return end == kGoOn;
}

// The verdict, in this order: invalid, parameter tolerance, function tolerance (both on the candidate, BEFORE acceptance), relative
// decrease.  Host and device: k_lm_norms takes the verdict the gated launches of an accepted step read (IEEE sqrt / divide on both).
__host__ __device__ inline StepVerdict trial_verdict(const TrialRecord& r, double x_cost, double ptol, double ftol) {
  StepVerdict v = {kStepInvalid, 0.0, 0.0};
  if (!r.valid || !(r.model_change > 0.0)) return v;
  v.cost_change = x_cost - r.cand_cost;
  if (sqrt(r.sn) <= ptol * (sqrt(r.xn) + ptol)) { v.kind = kStepParameterTolerance; return v; }
  if (fabs(v.cost_change) <= ftol * x_cost) { v.kind = kStepFunctionTolerance; return v; }
  v.rel = v.cost_change / r.model_change;
  v.kind = v.rel > kMinRelativeDecrease ? kStepAccepted : kStepRejected;
  return v;
}

// Who has the last word on a trial step whose record came from the device with k_lm_norms' verdict `dev_accept` beside it:
// the host alone ...
inline StepVerdict verdict_host_decides(const TrialRecord& r, double x_cost, double ptol, double ftol) { return trial_verdict(r, x_cost, ptol, ftol); }
// ... the device in place of the relative-decrease test, after the host's own validity and tolerance tests ...
inline StepVerdict verdict_device_decides_decrease(const TrialRecord& r, bool dev_accept, double x_cost, double ptol, double ftol) {
  StepVerdict v = trial_verdict(r, x_cost, ptol, ftol);
  if (v.kind == kStepAccepted || v.kind == kStepRejected) v.kind = dev_accept ? kStepAccepted : kStepRejected;
  return v;
}
// ... or the device outright: launches gated on its accept have run, the candidate IS the next point whatever the host's tests say
// (they could differ by a last bit of sqrt or pow); without the accept, the rule above
inline StepVerdict verdict_device_accept_applied(const TrialRecord& r, bool dev_accept, double x_cost, double ptol, double ftol) {
  if (!dev_accept) return verdict_device_decides_decrease(r, false, x_cost, ptol, ftol);
  const double cost_change = x_cost - r.cand_cost;
  return {kStepAccepted, cost_change, cost_change / r.model_change};
}

// Initial radius 1e4; radius /= max(1/3, 1 - (2 rho - 1)^3) on success (capped at 1e16), /= 2, 4, 8 .. on failure; the LM diagonal is
// kept across a rejected step and rebuilt after any other; the fifth invalid step in a row fails the solve.
struct TrustRegion {
  double radius = 1e4, decrease_factor = 2.0;
  bool reuse_diagonal = false;
  int iteration = 0, invalid = 0;
  // The loop head in two halves, each kGoOn or the termination code.  A solver that has the gradient norm of its point at hand takes
  // both at once (next); the pose graph's arrives with the record of the trial it enqueues in between.
  int before_trial(int max_iterations) const { return iteration >= max_iterations ? 1 : radius < 1e-32 ? 0 : kGoOn; }
  int count_trial(double gmax, double gtol) {
    if (gmax <= gtol) return 0;
    iteration++;
    return kGoOn;
  }
  int next(int max_iterations, double gmax, double gtol) { const int end = before_trial(max_iterations); return end != kGoOn ? end : count_trial(gmax, gtol); }
  // what the verdict does to the radius; kGoOn or the termination code
  int update(const StepVerdict& v) {
    if (v.kind == kStepInvalid) return ++invalid >= 5 ? 2 : shrink(false);
    if (v.kind > kStepRejected) return 0;   // a tolerance reached on the candidate
    invalid = 0;
    if (v.kind == kStepRejected) return shrink(true);
    radius = radius / std::max(1.0 / 3.0, 1.0 - pow(2.0 * v.rel - 1.0, 3));
    radius = std::min(1e16, radius);
    decrease_factor = 2.0; reuse_diagonal = false;
    return kGoOn;
  }
 private:
  int shrink(bool reuse) { radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = reuse; return kGoOn; }
};

}  // namespace dvs
