// backend.cpp:735-777 with the triangulation on the device: dvslam::associateAndTriangulate (one batched dvs_triangulate_landmarks before
// the walk) against the reference's order of operations — associateSequential whose onMatch triangulates the ONE matched landmark at match
// time from its current position (dvs_triangulate_landmarks with nlm = 1).  Landmark 5 is chosen by observations 0 and 1 and moves to
// its triangulated position after the first, so observation 1 is re-evaluated and falls to its twin 210.  Exit 0 = ok, 3 = no GPU.
#include <cstdio>
#include <cstring>
#include <vector>
#include "dvslam/triangulation.hpp"

int main() {
  if (dvs_device_count() < 1) { std::printf("no device: triangulation adapter compiled, nothing run\n"); return 3; }
  dvs_matcher* m = nullptr;
  if (dvs_matcher_create(0, &m) != DVS_OK) return 1;
  const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};   // the new keyframe's pose (associateObservation)
  const double fx = 600, fy = 600, cx = 320, cy = 240;
  const int nkf = 6, nlm = 300, nobs = 200;
  std::vector<double> kR((size_t)nkf * 9, 0.0), kt((size_t)nkf * 3, 0.0);   // stored keyframes: x_cam = X + t, centres on a 1.2 m line
  for (int k = 0; k < nkf; k++) { kR[9 * k] = kR[9 * k + 4] = kR[9 * k + 8] = 1.0; kt[3 * k] = 0.6 - 0.24 * k; kt[3 * k + 1] = -0.05 * (k % 2); }
  uint32_t s = 7;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  std::vector<uint8_t> lmd((size_t)nlm * 32), obd((size_t)nobs * 32);
  std::vector<float> lmx((size_t)nlm * 3), obp((size_t)nobs * 2);
  std::vector<int64_t> offs(1, 0);
  std::vector<int32_t> vkf;
  std::vector<float> vpx;
  for (int j = 0; j < nlm; j++) {
    for (int k = 0; k < 32; k++) lmd[(size_t)j * 32 + k] = (uint8_t)rnd();
    const float X0 = -1.0f + 2.0f * (rnd() % 1000) / 1000.f, X1 = -0.7f + 1.4f * (rnd() % 1000) / 1000.f, X2 = 2.0f + (rnd() % 1000) / 500.f;
    // the database position: 1 mm off the views' point (landmark 5: 4 cm, about 10 px in the new keyframe)
    lmx[3 * j] = X0 + (j == 5 ? 0.04f : 0.001f * (float)((int)(rnd() % 3) - 1)); lmx[3 * j + 1] = X1; lmx[3 * j + 2] = X2;
    const int nv = j == 5 ? 4 : j == 210 ? 0 : (int)(rnd() % 6);   // 0..5 stored views, a few skipped ids among them
    for (int v = 0; v < nv; v++) {
      const int k = (j + 2 * v) % nkf;
      if (j != 5 && rnd() % 8 == 0) { vkf.push_back(-1); vpx.push_back(0.f); vpx.push_back(0.f); }
      const double X = X0 + kt[3 * k], Y = X1 + kt[3 * k + 1], Z = X2 + kt[3 * k + 2];
      vkf.push_back(k); vpx.push_back((float)(fx * X / Z + cx)); vpx.push_back((float)(fy * Y / Z + cy));
    }
    offs.push_back((int64_t)vkf.size());
  }
  // twin of landmark 5: same descriptor, 1.5 cm from 5's database position (about 3.5 px), no views
  memcpy(&lmd[(size_t)210 * 32], &lmd[(size_t)5 * 32], 32);
  lmx[3 * 210] = lmx[3 * 5] - 0.015f; lmx[3 * 210 + 1] = lmx[3 * 5 + 1]; lmx[3 * 210 + 2] = lmx[3 * 5 + 2];
  for (int i = 0; i < nobs; i++) {
    const int j = i < 2 ? 5 : (i * 7) % 150;   // observations 0 and 1 both see landmark 5; others see landmarks below 150, some twice
    memcpy(&obd[(size_t)i * 32], &lmd[(size_t)j * 32], 32);
    for (int f = 0; f < 6; f++) obd[(size_t)i * 32 + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
    const float jit = i < 2 ? 0.f : 1.f;
    obp[2 * i] = (float)(fx * lmx[3 * j] / lmx[3 * j + 2] + cx) + jit * ((int)(rnd() % 300) - 150) / 100.f;
    obp[2 * i + 1] = (float)(fy * lmx[3 * j + 1] / lmx[3 * j + 2] + cy) + jit * ((int)(rnd() % 300) - 150) / 100.f;
  }
  // (a) the reference's order: triangulate the matched landmark at match time, from its position at that moment
  std::vector<float> live = lmx;
  int calls = 0, moved = 0;
  auto onMatch = [&](int, int j, float* xyz) {
    const int64_t o[2] = {0, offs[j + 1] - offs[j]};
    int32_t st = -1;
    calls++;
    if (dvs_triangulate_landmarks(m, nkf, kR.data(), kt.data(), fx, fy, cx, cy, 1, o, vkf.data() + offs[j], vpx.data() + 2 * offs[j], xyz, xyz, &st) != DVS_OK)
      return false;
    moved += st == DVS_TRI_UPDATED;
    return st == DVS_TRI_UPDATED;
  };
  std::vector<int32_t> want;
  try {
    want = dvslam::associateSequential(m, obd.data(), obp.data(), nobs, lmd.data(), live.data(), nlm, R, t, fx, fy, cx, cy, 50.0, 5.0, onMatch);
  } catch (const std::exception& e) { std::printf("%s\n", e.what()); return 1; }
  // (b) the adapter
  std::vector<float> db = lmx;
  std::vector<int32_t> tri_status, got;
  try {
    got = dvslam::associateAndTriangulate(m, obd.data(), obp.data(), nobs, lmd.data(), db.data(), nlm, R, t, fx, fy, cx, cy, 50.0, 5.0, nkf, kR.data(),
                                          kt.data(), offs.data(), vkf.data(), vpx.data(), &tri_status);
  } catch (const std::exception& e) { std::printf("%s\n", e.what()); return 1; }
  std::vector<int32_t> snap(nobs, -1);
  if (dvs_associate(m, obd.data(), obp.data(), nobs, lmd.data(), lmx.data(), nlm, R, t, fx, fy, cx, cy, 50.0, 5.0, snap.data()) != DVS_OK) return 1;
  int diff = 0, assoc = 0, twice = 0;
  std::vector<int> hits(nlm, 0);
  for (int i = 0; i < nobs; i++) { diff += got[i] != want[i]; assoc += want[i] >= 0; if (want[i] >= 0) twice += ++hits[want[i]] == 2; }
  const bool same_db = memcmp(db.data(), live.data(), db.size() * 4) == 0;
  std::printf("associations %d (%d landmarks matched twice), triangulations %d (%d moved), adapter vs one-by-one loop: %d differences, db equal %d, "
              "obs0 -> %d, obs1 -> %d (snapshot %d), status of 5: %d\n",
              assoc, twice, calls, moved, diff, (int)same_db, got[0], got[1], snap[1], tri_status[5]);
  dvs_matcher_destroy(m);
  if (diff != 0 || !same_db || got[0] != 5 || got[1] != 210 || snap[1] != 5 || tri_status[5] != DVS_TRI_UPDATED || twice < 2 || moved < 20) return 1;
  return 0;
}
