// orbfe::MapPointStore and orbfe::ORBMatcher::trackLocalMapStored (orb_slam2_ros2_amd/host/orbfe_shim.hpp), the OpenCV-free mirror of
// the map-point store: a round trip through the RAII class, then Tracking::trackLocalMap's device work on one extracted
// frame with a local map made of its own keypoints at 10 m under the identity pose, named by id.
// Usage: test_mpstore_shim <image.raw> <w> <h>   prints "MPSTORE_SHIM_OK <points> <matches> <edges> <good>", or "NO_DEVICE" (exit 3).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2_ros2_amd/host/orbfe_shim.hpp"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int w = atoi(argv[2]), h = atoi(argv[3]);
  std::vector<uint8_t> img((size_t)w * h);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(img.data(), 1, img.size(), f) != img.size()) return 2;
  fclose(f);
  try {
    orbfe::ORBExtractor ex({img.data(), w, h, (size_t)w}, 2000, 8, 1.2f, "", 20, 7);
    std::vector<orbfe_keypoint> kps;
    std::vector<orbfe::Descriptor> desc;
    ex.extract(kps, desc);
    const size_t n = kps.size();
    const float fx = 718.856f, fy = 718.856f, cx = 607.1928f, cy = 185.2157f, depth = 10.f;
    std::vector<uint64_t> ids(n);
    std::vector<float> pos(3 * n), view(3 * n), maxD(n), minD(n);
    for (size_t i = 0; i < n; ++i) {
      ids[i] = 1000 + 3 * (n - i);  // gapped, descending
      const float X[3] = {(kps[i].x - cx) / fx * depth, (kps[i].y - cy) / fy * depth, depth};
      const float nrm = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
      for (int a = 0; a < 3; ++a) pos[3 * i + a] = X[a], view[3 * i + a] = X[a] / nrm;
      maxD[i] = nrm * 1.05f * std::pow(1.2f, (float)kps[i].octave), minD[i] = nrm * 0.5f;  // predictLevel gives the keypoint's octave
    }
    orbfe::MapPointStore store(0, 1024, 64);
    store.upsert(ids, ORBFE_MP_ALL, pos, view, maxD, minD, desc);
    std::vector<float> p2, v2, mx2, mn2;
    std::vector<orbfe::Descriptor> d2;
    int64_t used = 0, reserved = 0;
    if (!store.fetch(ids, p2, v2, mx2, mn2, d2) || p2 != pos || v2 != view || mx2 != maxD || mn2 != minD || d2 != desc || store.size(&used, &reserved) != n ||
        used != (int64_t)(64 * n) || reserved <= used)
      return fprintf(stderr, "the store's round trip differs\n"), 1;
    if (store.fetch({ids[0], 7}, p2, v2, mx2, mn2, d2)) return fprintf(stderr, "fetch of an id the store does not hold succeeded\n"), 1;
    // the frame's pose: the truth (identity) a few centimetres off (0.09 in all); the optimisation must at least halve that
    const float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcw[3] = {0.03f, -0.02f, 0.04f}, bounds[4] = {0.f, (float)w, 0.f, (float)h};
    const double pose0[7] = {0, 0, 0, 1, 0.03, -0.02, 0.04};
    std::vector<float> sig2(8), inv(8);
    for (int l = 0; l < 8; ++l) sig2[l] = std::pow(std::pow(1.2f, (float)l), 2.f), inv[l] = 1.f / sig2[l];
    const std::vector<uint8_t> flags(n, 7);
    const orbfe::ORBMatcher matcher(0.8f);
    const orbfe::ORBMatcher::Intrinsics K = {fx, fy, cx, cy, bounds[0], bounds[1], bounds[2], bounds[3]};
    const auto r = matcher.trackLocalMapStored(ex.context(), ex.slot(), store, ids, flags, {}, {}, Rcw, tcw, bounds, pose0, K, fx * 0.537166f, sig2, inv);
    int held = 0, self = 0;
    for (size_t i = 0; i < n; ++i) held += r.assigned[i] >= 0, self += r.assigned[i] == (int32_t)i;
    double off = 0;
    for (int a = 0; a < 3; ++a) off += std::fabs(r.poseSE3[4 + a]);
    if (!r.optimised() || r.nMatches != held || self < (int)(0.9 * held) || r.nMatches < (int)(n / 2) || r.nGood < r.nEdges / 2 || off > 0.045)
      return fprintf(stderr, "trackLocalMapStored: matches %d held %d self %d edges %d good %d pose off %.4f\n", r.nMatches, held, self, r.nEdges, r.nGood, off), 1;
    // an id the store does not hold: the call throws, naming it
    std::vector<uint64_t> bad = ids;
    bad[n / 2] = 999999;
    bool threw = false;
    try {
      matcher.trackLocalMapStored(ex.context(), ex.slot(), store, bad, flags, {}, {}, Rcw, tcw, bounds, pose0, K, fx * 0.537166f, sig2, inv);
    } catch (const std::exception& e) {
      threw = strstr(e.what(), "999999") != nullptr;
    }
    if (!threw) return fprintf(stderr, "an absent id did not throw\n"), 1;
    store.erase({ids[1]});
    if (store.size() != n - 1) return fprintf(stderr, "erase\n"), 1;
    printf("MPSTORE_SHIM_OK %zu %d %d %d\n", n, r.nMatches, r.nEdges, r.nGood);
    return 0;
  } catch (const std::exception& e) {
    if (strstr(e.what(), "no HIP device") || strstr(e.what(), "no usable HIP device")) {
      printf("NO_DEVICE\n");
      return 3;
    }
    fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}
