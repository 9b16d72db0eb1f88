// dvslam::globalBundleAdjust (include/dvslam/global_ba.hpp) over recorded keyframes:
//   global_ba_adapter <keyframes.bin> <fx> <fy> <cx> <cy>
// keyframes.bin: as tests/cpp/mapping_backend_adapter.cpp reads it.  Prints the result of a run capped at one iteration and the map after
// it, then the result of a run with the defaults and the map after it, every array as its CRC-32.  tests/test_cpp_global_ba.py holds the
// text against the Python mirror's.  Exit code 0 = ok, 3 = no GPU, 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dvslam/global_ba.hpp"

static_assert(sizeof(dvs_ba_global_params) == 40 && sizeof(dvs_ba_global_summary) == 40 && sizeof(dvs_backend_gba_result) == 56,
              "the ctypes mirrors (dvslam_amd/_lib.py, dvslam_amd/backend.py) assume these sizes");

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

static void print_run(const char* tag, const dvs_backend_gba_result& r, const dvslam::MappingBackend& mb) {
  unsigned long long c0, c1;
  std::memcpy(&c0, &r.summary.ba.initial_cost, 8); std::memcpy(&c1, &r.summary.ba.final_cost, 8);
  const dvslam::MapLandmarks L = mb.landmarks();
  const dvslam::MapObservations O = mb.observations();
  const dvslam::MapKeyframes K = mb.keyframes();
  std::printf("%s term=%d steps=%d its=%d solver=%d pcg=%d cost=%016llx,%016llx cams=%d lms=%d obs=%d left=%d lm=%zu %08x %08x ob=%zu %08x %08x kf=%zu %08x %08x\n", tag,
              r.summary.ba.termination, r.summary.ba.num_successful_steps, r.summary.ba.num_iterations, r.summary.ba.linear_solver, r.summary.pcg_iterations, c0, c1,
              r.n_cameras, r.n_landmarks, r.n_observations, r.n_left_out, L.id.size(), crc(L.id), crc(L.xyz), O.id.size(), crc(O.landmark_id), crc(O.px),
              K.frame_id.size(), crc(K.R), crc(K.t));
}

static bool rd(std::FILE* fh, void* p, size_t n) { return std::fread(p, 1, n, fh) == n; }

int main(int argc, char** argv) {
  dvslam::GlobalBaParams gp;
  if (gp.max_iterations != 50 || gp.max_pcg_iterations != 0 || gp.function_tolerance != 1e-6 || gp.gradient_tolerance != 1e-10 || gp.parameter_tolerance != 1e-8 ||
      gp.eta != 0.1)
    return 1;
  if (dvs_device_count() < 1) { std::printf("no device: adapter compiled, nothing run\n"); return 3; }
  if (argc < 6) { std::fprintf(stderr, "usage: global_ba_adapter keyframes.bin fx fy cx cy\n"); return 2; }
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
    if (!rd(fh, payload.data(), len) || !rd(fh, &ndet, 4) || ndet != 0) return 2;
    mb.addKeyframe(payload, {});
  }
  std::fclose(fh);
  dvslam::GlobalBA solver;
  solver.params().max_iterations = 1;
  print_run("capped", dvslam::globalBundleAdjust(mb, solver), mb);
  solver.params() = dvslam::GlobalBaParams();
  print_run("global", dvslam::globalBundleAdjust(mb, solver), mb);
  return 0;
}
