// Driver of dvslam::PoseGraph (include/dvslam/pose_graph.hpp) for tests/test_cpp_pose_graph.py and tests/test_pose_graph_cpu.py: builds the
// graph of a binary file through addNode / addEdge / addLoop, optimises, corrects the points of a second file, and prints the summary, the
// poses and the points as the bytes of their doubles / floats.  Exit 3 without a GPU, 2 without arguments.
//   graph file : int32 N, E, L; R [N][9], t [N][3] (double); fixed [N] (uint8); i, j [E] (int32); Rz [E][9], tz [E][3], w_rot, w_trans [E]
//                (double).  The last L edges go through addLoop as verified candidates.
//   points file: int32 n; xyz [n][3] (float); anchor [n] (int32)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <dvslam/pose_graph.hpp>

template <class T>
static std::vector<T> take(std::ifstream& f, size_t n) {
  std::vector<T> v(n);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
  if (!f) throw std::runtime_error("short file");
  return v;
}
static void hex(double x) { uint64_t u; std::memcpy(&u, &x, 8); std::printf(" %016" PRIx64, u); }
static void hexf(float x) { uint32_t u; std::memcpy(&u, &x, 4); std::printf(" %08" PRIx32, u); }

int main(int argc, char** argv) {
  if (dvs_device_count() < 1) { std::fprintf(stderr, "no HIP device: dvslam::PoseGraph has no CPU fallback\n"); return 3; }
  if (argc < 3) { std::fprintf(stderr, "usage: pose_graph_adapter graph.bin points.bin\n"); return 2; }
  try {
    std::ifstream gf(argv[1], std::ios::binary), pf(argv[2], std::ios::binary);
    const std::vector<int32_t> hdr = take<int32_t>(gf, 3);
    const size_t N = (size_t)hdr[0], E = (size_t)hdr[1], L = (size_t)hdr[2];
    const auto R = take<double>(gf, 9 * N), t = take<double>(gf, 3 * N);
    const auto fixed = take<uint8_t>(gf, N);
    const auto ei = take<int32_t>(gf, E), ej = take<int32_t>(gf, E);
    const auto Rz = take<double>(gf, 9 * E), tz = take<double>(gf, 3 * E), wr = take<double>(gf, E), wt = take<double>(gf, E);
    dvslam::PoseGraph pg;
    for (size_t n = 0; n < N; n++) pg.addNode(&R[9 * n], &t[3 * n], fixed[n] != 0);
    for (size_t e = 0; e < E; e++) {
      if (e + L < E) { pg.addEdge(ei[e], ej[e], &Rz[9 * e], &tz[3 * e], wr[e], wt[e]); continue; }
      dvslam::LoopCandidate c;
      c.Id = (dvslam::EntryId)ej[e]; c.Score = 0; c.verified = true;
      std::memcpy(c.R, &Rz[9 * e], sizeof(c.R)); std::memcpy(c.t, &tz[3 * e], sizeof(c.t));
      pg.addLoop(ei[e], ej[e], c, wr[e], wt[e]);
    }
    pg.params().max_iterations = 100; pg.params().function_tolerance = 1e-14; pg.params().parameter_tolerance = 1e-14;
    std::printf("cost"); hex(pg.cost()); std::printf("\n");
    const dvs_pgo_summary s = pg.optimize();
    std::printf("summary %d %d %d %d", s.termination, s.num_successful_steps, s.num_iterations, s.pcg_iterations);
    hex(s.initial_cost); hex(s.final_cost); std::printf("\n");
    const std::vector<dvslam::Pose> poses = pg.poses();
    const dvslam::Pose last = pg.pose((int)N - 1);
    if (std::memcmp(&last, &poses[N - 1], sizeof(last)) != 0) throw std::runtime_error("pose(i) != poses()[i]");
    for (size_t n = 0; n < N; n++) {
      std::printf("pose %zu", n);
      for (int k = 0; k < 9; k++) hex(poses[n].R[k]);
      for (int k = 0; k < 3; k++) hex(poses[n].t[k]);
      std::printf("\n");
    }
    std::printf("trace %zu\n", pg.trace().size());
    const size_t np = (size_t)take<int32_t>(pf, 1)[0];
    const auto xyz = take<float>(pf, 3 * np);
    const auto anchor = take<int32_t>(pf, np);
    std::vector<std::array<float, 3>> pts(np);
    for (size_t k = 0; k < np; k++) pts[k] = {xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]};
    pg.correctPoints(pts, anchor);
    for (size_t k = 0; k < np; k++) { std::printf("point %zu", k); for (int a = 0; a < 3; a++) hexf(pts[k][a]); std::printf("\n"); }
    // a candidate that is not verified is refused
    dvslam::LoopCandidate bad;
    bad.Id = 0; bad.Score = 0;
    try { pg.addLoop(1, 0, bad, 1.0, 1.0); std::printf("unverified accepted\n"); } catch (const std::runtime_error&) { std::printf("unverified refused\n"); }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pose_graph_adapter: %s\n", e.what());
    return 1;
  }
  return 0;
}
