// The forward-fuse bodies of orbfe_loopfuse_dropin.hpp over the minimal types of test_fuse_dropin.cpp (included for its types, loader and
// printer; its main is renamed away), linked to liborbfe_hip.so.  The map written by tests/test_gpu_fuse_points.py (keyframes 1 .. K are
// the targets, points below 1000 the loop group, in id order with one null pointer among them) is built four times:
//   A  the chain of the existing bodies, orbfe::dropin::fuse(pkf, pts, map, true, 4.0f, 0.8f, 8) per target in order
//   B  orbfe::dropin::fuseLoopPoints<Camera, Frame>(targets, pts, map, store): one device call and the replay
//   C  orbfe::dropin::fuse(pkf, pts, map, false, 3.0f, 0.6f, 8) on target 1
//   D  orbfe::dropin::fuse<Camera, Frame>(store, pkf, pts, map, false, 3.0f, 0.6f) on target 1
// Exit code 0 and "OK <nFuse A> <nFuse B> <re-evaluations> <extra calls> <nFuse D>" when A and B, and C and D, end in equal maps (slots,
// observations, bad flags) with equal counts.
#define main plain_main
#include "test_fuse_dropin.cpp"
#undef main

#include "orbfe_loopfuse_dropin.hpp"

struct Access {
  static uint64_t id(const KeyFrame::SharedPtr& k) { return (uint64_t)k->id; }
  static void bounds(const KeyFrame::SharedPtr& k, float b[4]) { orbfe::dropin::Bodies::bounds(k, b); }
};

static void group(World& w, std::vector<KeyFrame::SharedPtr>& targets, std::vector<MapPoint::SharedPtr>& pts) {
  for (const auto& k : w.kfs)
    if (k.first >= 1 && k.first < 100) targets.push_back(k.second);
  for (const auto& p : w.pts)
    if (p.first < 1000 && p.second) pts.push_back(p.second);
  pts.insert(pts.begin() + 7, MapPoint::SharedPtr());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  ORB_SLAM2_ROS2::ORBExtractor::mnLevels = 8;
  World A = load(argv[1]), B = load(argv[1]), C = load(argv[1]), D = load(argv[1]);
  if (dump(A) != dump(B)) return 3;
  std::vector<KeyFrame::SharedPtr> tA, tB, tC, tD;
  std::vector<MapPoint::SharedPtr> pA, pB, pC, pD;
  group(A, tA, pA), group(B, tB, pB), group(C, tC, pC), group(D, tD, pD);
  if (tA.size() < 2 || pA.size() < 20) return 3;
  int nA = 0;
  for (auto& pkf : tA) nA += orbfe::dropin::fuse(pkf, pA, A.map, true, 4.0f, 0.8f, 8);
  orbfe::dropin::KeyframeStore<Access> store(640, 480, 8);
  const int nB = orbfe::dropin::fuseLoopPoints<Camera, Frame>(tB, pB, B.map, store);
  const long long reeval = orbfe::dropin::fuseLoopReevaluations(), extra = orbfe::dropin::fuseLoopExtraCalls();
  const std::string a = dump(A), b = dump(B);
  if (a != b || nA != nB || A.map->nReplaced != B.map->nReplaced || orbfe::dropin::fuseLoopLastCount() != nB || store.size() != tB.size()) {
    std::fprintf(stderr, "loop fuse: maps differ: %d vs %d fuses, %d vs %d replaces, %zu vs %zu bytes of state, %zu stored\n", nA, nB, A.map->nReplaced,
                 B.map->nReplaced, a.size(), b.size(), store.size());
    return 1;
  }
  const int nC = orbfe::dropin::fuse(tC[0], pC, C.map, false, 3.0f, 0.6f, 8);
  const int nD = orbfe::dropin::fuse<Camera, Frame>(store, tD[0], pD, D.map, false, 3.0f, 0.6f);  // (same ids: the keyframe is resident already)
  if (dump(C) != dump(D) || nC != nD || C.map->nReplaced != D.map->nReplaced) {
    std::fprintf(stderr, "single fuse: maps differ: %d vs %d fuses, %d vs %d replaces\n", nC, nD, C.map->nReplaced, D.map->nReplaced);
    return 1;
  }
  std::printf("OK %d %d %lld %lld %d\n", nA, nB, reeval, extra, nD);
  return 0;
}
