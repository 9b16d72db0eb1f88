// dvslam::closeLoop (include/dvslam/loop_closing.hpp) and the loop-closing members of dvslam::MappingBackend over recorded keyframes:
//   loop_closing <keyframes.bin> <loop.bin> <fx> <fy> <cx> <cy>
// keyframes.bin: as tests/cpp/mapping_backend_adapter.cpp reads it.  loop.bin: uint64 query frame, uint64 entry frame, then 10 doubles:
// rvec, tvec, w_rot, w_trans of the loop and the odometry weights; then uint32 n and n uint64 entry frames of the fusion.
// Prints the anchors, the pose graph, the result of closeLoop without fusion and the map after it, a dry-run fusion and the map after the
// applied one, every array as its CRC-32.  tests/test_cpp_loop_closing.py holds the text against the Python mirror's.
// Exit code 0 = ok, 3 = no GPU, 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dvslam/loop_closing.hpp"

static_assert(sizeof(dvs_fuse_params) == 24 && sizeof(dvs_fuse_result) == 16 && sizeof(dvs_close_loop_result) == 64,
              "the ctypes mirror (dvslam_amd/backend.py) assumes these sizes");

template <class T>
static uint32_t crc(const std::vector<T>& v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < v.size() * sizeof(T); i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

static void print_map(const dvslam::MappingBackend& mb) {
  const dvslam::MapLandmarks L = mb.landmarks();
  const dvslam::MapObservations O = mb.observations();
  const dvslam::MapKeyframes K = mb.keyframes();
  std::printf("lm=%zu %08x %08x %08x %08x %08x %08x %08x %08x ob=%zu %08x %08x %08x %08x %08x %08x kf=%zu %08x %08x %08x %08x %08x %08x\n", L.id.size(), crc(L.id),
              crc(L.class_id), crc(L.xyz), crc(L.desc), crc(L.observation_count), crc(L.last_seen_ns), crc(L.obs_offsets), crc(L.obs_ids), O.id.size(), crc(O.id),
              crc(O.frame_id), crc(O.px), crc(O.desc), crc(O.class_id), crc(O.landmark_id), K.frame_id.size(), crc(K.frame_id), crc(K.stamp_ns), crc(K.R), crc(K.t),
              crc(K.obs_offsets), crc(K.obs_ids));
}

static bool rd(std::FILE* fh, void* p, size_t n) { return std::fread(p, 1, n, fh) == n; }

int main(int argc, char** argv) {
  dvslam::FuseParams fp;
  if (fp.max_descriptor_distance != 50.0 || fp.max_reprojection_distance != 5.0 || fp.fuse_neighbours != 2) return 1;
  if (dvs_device_count() < 1) { std::printf("no device: adapter compiled, nothing run\n"); return 3; }
  if (argc < 7) { std::fprintf(stderr, "usage: loop_closing keyframes.bin loop.bin fx fy cx cy\n"); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return 2;
  dvs_backend_params p = dvslam::MappingBackend::defaultParams(std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6]));
  p.initial_capacity = 64;
  dvslam::MappingBackend mb(p);
  uint32_t count = 0;
  if (!rd(fh, &count, 4)) return 2;
  for (uint32_t k = 0; k < count; k++) {
    uint32_t len = 0, ndet = 0;
    if (!rd(fh, &len, 4)) return 2;
    std::vector<uint8_t> payload(len);
    if (!rd(fh, payload.data(), len) || !rd(fh, &ndet, 4) || ndet != 0) return 2;
    mb.addKeyframe(payload, {});
  }
  std::fclose(fh);
  fh = std::fopen(argv[2], "rb");
  if (!fh) return 2;
  uint64_t frames[2]; double v[10]; uint32_t ne = 0;
  if (!rd(fh, frames, 16) || !rd(fh, v, 80) || !rd(fh, &ne, 4)) return 2;
  std::vector<uint64_t> entries(ne);
  if (ne && !rd(fh, entries.data(), 8 * (size_t)ne)) return 2;
  std::fclose(fh);
  const std::vector<dvslam::LoopEdge> loops(1, dvslam::LoopEdge(frames[0], frames[1], v, v + 3, v[6], v[7]));
  const dvslam::MapAnchors A = mb.anchors();
  std::printf("anchors %zu %08x %08x\n", A.id.size(), crc(A.id), crc(A.keyframe));
  const dvslam::MapPoseGraph G = mb.buildPoseGraph(std::vector<dvslam::MapLoop>(loops.begin(), loops.end()), v[8], v[9]);
  std::printf("graph %zu %zu %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", G.fixed.size(), G.ei.size(), crc(G.R), crc(G.t), crc(G.fixed), crc(G.ei), crc(G.ej), crc(G.rvec),
              crc(G.tvec), crc(G.w_rot), crc(G.w_trans));
  dvslam::PoseGraph pg;
  const dvs_close_loop_result r = dvslam::closeLoop(mb, pg, loops, dvslam::OdometryWeights{v[8], v[9]});
  unsigned long long c0, c1;
  std::memcpy(&c0, &r.summary.initial_cost, 8); std::memcpy(&c1, &r.summary.final_cost, 8);
  std::printf("close term=%d steps=%d its=%d pcg=%d cost=%016llx,%016llx nodes=%d edges=%d moved=%d fused=%d ", r.summary.termination, r.summary.num_successful_steps,
              r.summary.num_iterations, r.summary.pcg_iterations, c0, c1, r.n_nodes, r.n_edges, r.n_landmarks_moved, r.fuse.n_fused);
  print_map(mb);
  const dvslam::MapFusion D = mb.fuse(frames[0], entries, &fp, false);
  std::printf("dry %d %d %d %d %08x %08x %08x ", D.counts.n_sources, D.counts.n_targets, D.counts.n_proposals, D.counts.n_fused, crc(D.survivor_id), crc(D.removed_id),
              crc(D.error));
  print_map(mb);
  const dvslam::MapFusion F = mb.fuse(frames[0], entries);
  std::printf("fuse %d %d %d %d %08x %08x %08x ", F.counts.n_sources, F.counts.n_targets, F.counts.n_proposals, F.counts.n_fused, crc(F.survivor_id), crc(F.removed_id),
              crc(F.error));
  print_map(mb);
  return 0;
}
