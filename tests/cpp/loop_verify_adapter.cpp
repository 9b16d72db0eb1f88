// dvslam::LoopDatabase's verification layer (include/dvslam/loop_detection.hpp: setPoints, getPoints, verify, detectVerified) from a host
// program: a vocabulary text file, the rows file of tests/cpp/loop_detection_adapter.cpp (the LAST frame is the query) and a points file
// (int32 frames, then per frame int32 n and n x 3 floats).  Prints, for detectVerified(top 3) and for verify() over match() against every
// entry, one line per candidate: id, verified, correspondences, iterations, the bytes of t and rms, R with 17 digits, the inlier rows;
// tests/test_cpp_loop_verify.py compares them with what the Python binding returns for the same inputs.
// Exit codes: 0 ok, 1 a check failed, 2 usage, 3 no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "dvslam/loop_detection.hpp"

static unsigned long long bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return (unsigned long long)b;
}

static void print_candidates(const char* tag, const std::vector<dvslam::LoopCandidate>& cands) {
  std::printf("%s %zu\n", tag, cands.size());
  for (const dvslam::LoopCandidate& c : cands) {
    std::printf("cand %u %d %d %d %zu t %016llx %016llx %016llx rms %016llx R", c.Id, c.verified ? 1 : 0, c.correspondences, c.iterations, c.matches.size(),
                bits(c.t[0]), bits(c.t[1]), bits(c.t[2]), bits(c.rms));
    for (int k = 0; k < 9; k++) std::printf(" %.17g", c.R[k]);
    std::printf(" inliers %zu", c.inliers.size());
    for (int i : c.inliers) std::printf(" %d", i);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (dvs_device_count() < 1) { std::fprintf(stderr, "no GPU: there is no CPU fallback\n"); return 3; }
  if (argc != 5) { std::fprintf(stderr, "usage: %s vocabulary.txt frames.bin points.bin seed\n", argv[0]); return 2; }
  std::vector<dvslam::DescriptorVector> frames;
  std::vector<dvslam::PointVector> points;
  {
    FILE* fp = std::fopen(argv[2], "rb");
    FILE* pp = std::fopen(argv[3], "rb");
    int32_t nf = 0, np = 0;
    if (!fp || !pp || std::fread(&nf, 4, 1, fp) != 1 || std::fread(&np, 4, 1, pp) != 1 || nf < 1 || np != nf) return 2;
    frames.resize(nf); points.resize(nf);
    for (int32_t f = 0; f < nf; f++) {
      int32_t n = 0, m = 0;
      if (std::fread(&n, 4, 1, fp) != 1 || std::fread(&m, 4, 1, pp) != 1 || n < 0 || m != n) return 2;
      frames[f].resize(n); points[f].resize(n);
      if (n && (std::fread(frames[f][0].data(), 32, n, fp) != (size_t)n || std::fread(points[f][0].data(), 12, n, pp) != (size_t)n)) return 2;
    }
    std::fclose(fp); std::fclose(pp);
  }
  try {
    dvslam::OrbVocabulary vocabulary(argv[1]);
    dvslam::LoopDatabase database(vocabulary, 1);
    std::vector<dvslam::EntryId> all;
    for (size_t f = 0; f + 1 < frames.size(); f++) {
      all.push_back(database.add(frames[f]));
      if (f != 2) database.setPoints(all.back(), points[f]);          // entry 2 never gets points
    }
    const dvslam::PointVector back = database.getPoints(1);
    if (back.size() != points[1].size() || std::memcmp(back[0].data(), points[1][0].data(), 12 * back.size()) != 0) {
      std::fprintf(stderr, "getPoints(1) is not what setPoints(1) stored\n");
      return 1;
    }
    const dvslam::PointVector none = database.getPoints(2);
    for (const dvslam::Point3& p : none)
      if (p[0] == p[0]) { std::fprintf(stderr, "an entry without points must read back as NaN\n"); return 1; }
    dvslam::VerifyParams vp;
    vp.iterations = 64; vp.seed = (uint64_t)std::strtoull(argv[4], nullptr, 10);
    vp.fx = 615; vp.fy = 615; vp.cx = 320; vp.cy = 240;
    print_candidates("detectVerified", database.detectVerified(frames.back(), points.back(), 3, -1, vp));
    std::vector<dvslam::LoopCandidate> cands = database.match(frames.back(), all);
    if (cands[0].verified || !cands[0].inliers.empty()) return 1;      // as constructed
    database.verify(points.back(), cands, vp);
    print_candidates("verify", cands);
    bool threw = false;
    try { dvslam::VerifyParams bad = vp; bad.fx = 0; database.verify(points.back(), cands, bad); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::fprintf(stderr, "a focal length of 0 must be refused\n"); return 1; }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
