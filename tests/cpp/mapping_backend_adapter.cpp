// dvslam::MappingBackend (include/dvslam/mapping_backend.hpp) over recorded keyframes read from a file:
//   mapping_backend_adapter <keyframes.bin> <fx> <fy> <cx> <cy> <ba_now_sec>
// File: uint32 count, then per keyframe { uint32 payload bytes, the Keyframe.msg CDR payload, uint32 detections,
// per detection { double cx, cy, w, h; uint32 name bytes; the name } }.  After every keyframe one line with the result record and the CRC-32 of
// every column of the three tables; after the last keyframe bundleAdjust(ba_now_sec, 0) and one more line.  tests/test_cpp_backend.py holds
// the text against the Python mirror's.  Exit code 0 = ok, 3 = no GPU, 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dvslam/mapping_backend.hpp"

static_assert(sizeof(dvs_backend_params) == 136 && sizeof(dvs_detection) == 40 && sizeof(dvs_backend_result) == 40,
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
  const dvs_backend_params d = dvslam::MappingBackend::defaultParams(500, 500, 320, 240);
  if (d.window != 5 || d.max_descriptor_distance != 50.0 || d.prune_min_observations != 2 || d.n_filtered != 0) return 1;
  if (dvs_device_count() < 1) { std::printf("no device: adapter compiled, nothing run\n"); return 3; }
  if (argc < 7) { std::fprintf(stderr, "usage: mapping_backend_adapter keyframes.bin fx fy cx cy ba_now_sec\n"); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return 2;
  dvs_backend_params p = dvslam::MappingBackend::defaultParams(std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]));
  p.initial_capacity = 64;
  dvslam::MappingBackend mb(p);
  uint32_t count = 0;
  if (!rd(fh, &count, 4)) return 2;
  for (uint32_t k = 0; k < count; k++) {
    uint32_t len = 0, ndet = 0;
    if (!rd(fh, &len, 4)) return 2;
    std::vector<uint8_t> payload(len);
    if (!rd(fh, payload.data(), len) || !rd(fh, &ndet, 4)) return 2;
    std::vector<dvslam::Detection> det(ndet);
    for (auto& dd : det) {
      double b[4]; uint32_t nl = 0;
      if (!rd(fh, b, 32) || !rd(fh, &nl, 4)) return 2;
      dd.cx = b[0]; dd.cy = b[1]; dd.w = b[2]; dd.h = b[3];
      dd.class_name.resize(nl);
      if (nl && !rd(fh, &dd.class_name[0], nl)) return 2;
    }
    const dvs_backend_result r = mb.addKeyframe(payload, det);
    std::printf("%u kept=%d filtered=%d assoc=%d created=%d moved=%d first=%lld,%lld ", k, r.n_kept, r.n_filtered, r.n_associated, r.n_created, r.n_moved,
                (long long)r.first_observation_id, (long long)r.first_landmark_id);
    print_map(mb);
  }
  std::fclose(fh);
  int32_t rl = 0, ro = 0;
  const dvslam::OptimizationResult res = mb.bundleAdjust(std::atoi(argv[6]), 0, &rl, &ro);
  unsigned long long cost;
  std::memcpy(&cost, &res.final_cost, 8);
  std::printf("ba success=%d iterations=%d cost=%016llx pruned=%d,%d ", res.success ? 1 : 0, res.iterations_completed, cost, rl, ro);
  print_map(mb);
  return 0;
}
