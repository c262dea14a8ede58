// The two bodies of orbfe_kfstore_dropin.hpp over the minimal types of test_fuse_dropin.cpp / test_tri_dropin.cpp (included for their
// types, loaders and printers; their main is renamed away), linked to liborbfe_hip.so.  tests/test_gpu_kfstore.py builds this file twice:
//   (default)       the map of fs.write_dropin_input twice: copy A through orbfe::dropin::fuseMapPoints, copy B through the store.  The
//                   selection of fuseMapPoints iterates unordered sets of POINTERS, so two copies of a map select in different orders
//                   and end in different (equally valid) maps; B therefore runs the forward fuse and fuseIntoKeyframes(.., store) on
//                   the orders A's containers gave.  Equal final maps (slots, observations, bad flags), fuse, replace, flag and
//                   re-evaluation counts.  The limit: the one-line overload fuseMapPoints(cur, map, store) runs on a third copy, where
//                   only what does not depend on that order is compared (the store's size, updateConnections, the number of targets).
//   -DKFSTORE_TRI   the input of test_gpu_triangulation.py's drop-in test twice through createNewMapPoints, without and with the store:
//                   equal mlpAddedMPs (slot, neighbour, train, origin, position bits).  The store is first filled the way the fuse
//                   overload fills it -- every keyframe from features and bounds alone, no stereo columns (what ensureFeatures inserts;
//                   the fuse body itself cannot run on these types, which have no map-point model) -- so createNewMapPoints meets
//                   entries without stereo and must replace them: with depth and right_u left at -1 no record would be a stereo one.
// Exit code 0 and one line "OK ..." when the two runs agree.
#define main plain_main
#ifdef KFSTORE_TRI
#include "test_tri_dropin.cpp"
#else
#include "test_fuse_dropin.cpp"
#endif
#undef main

#include <sstream>

#include "orbfe_kfstore_dropin.hpp"

#ifdef KFSTORE_TRI

struct Access {  // the minimal KeyFrame has no id and no bounds: the input index, the image
  static uint64_t id(const KeyFrame::SharedPtr& k) { return (uint64_t)(k->inputIdx + 1); }
  static void bounds(const KeyFrame::SharedPtr&, float b[4]) { b[0] = 0, b[1] = 640, b[2] = 0, b[3] = 480; }
};

struct World {
  std::vector<KeyFrame::SharedPtr> kfs;
  KeyFrame::SharedPtr cur;
  std::unordered_map<std::size_t, MapPoint::SharedPtr> unproc;
};

static World load(const char* path, bool first) {  // (the parser of test_tri_dropin.cpp's main)
  std::ifstream in(path);
  World w;
  const float fx = rd(in), fy = rd(in), cx = rd(in), cy = rd(in);
  const cv::Mat kinv = mat(in, 3, 3);
  const float bl = rd(in);
  int nl = 0, nkf = 0;
  in >> nl;
  std::vector<float> sf;
  for (int l = 0; l < nl; ++l) sf.push_back(rd(in));
  if (first) Camera::mfFx = fx, Camera::mfFy = fy, Camera::mfCx = cx, Camera::mfCy = cy, Camera::mKInv = kinv, Camera::mfBl = bl, Frame::sf = sf;
  in >> nkf;
  for (int k = 0; k < nkf; ++k) {
    auto kf = std::make_shared<KeyFrame>();
    kf->inputIdx = k - 1;
    int n = 0;
    in >> n;
    kf->Tcw = mat(in, 4, 4), kf->Twc = mat(in, 4, 4), kf->Ow = mat(in, 3, 1);
    for (int i = 0; i < n; ++i) {
      cv::KeyPoint kp;
      kp.pt.x = rd(in), kp.pt.y = rd(in);
      in >> kp.octave;
      double d, r;
      int fl;
      in >> d >> r >> fl;
      cv::Mat ds(1, 32, CV_8U);
      for (int b = 0; b < 32; ++b) {
        int v;
        in >> v;
        ds.data[b] = (uint8_t)v;
      }
      kf->kps.push_back(kp), kf->desc.push_back(ds), kf->depth.push_back(d), kf->ru.push_back(r);
      MapPoint::SharedPtr mp;
      if (fl & 1) {
        mp = std::make_shared<MapPoint>();
        mp->inMap = (fl & 2) != 0;
      }
      kf->mps.push_back(mp);
      if (k == 0) {
        int u;
        in >> u;
        cv::Mat p = mat(in, 3, 1);
        if (u) {
          auto m = MapPoint::create(p);
          m->fromUnproc = true;
          w.unproc[(std::size_t)i] = m;
        }
      }
    }
    int nn = 0;
    in >> nn;
    for (int j = 0; j < nn; ++j) {
      unsigned node;
      int c;
      in >> node >> c;
      auto& v = kf->mFeatVec[node];
      for (int q = 0; q < c; ++q) {
        unsigned id;
        in >> id;
        v.push_back(id);
      }
    }
    if (k == 0) w.cur = kf;
    else w.kfs.push_back(kf);
  }
  w.cur->conn = w.kfs;
  return w;
}

// the neighbours' allocation order decides the std::map order of loop 1: both worlds are printed with the neighbour's INPUT index
static std::string dump(const World& w, const std::list<MapPoint::SharedPtr>& added) {
  std::ostringstream o;
  for (auto& m : added) {
    const bool slot = w.cur->mps[(size_t)m->query] == m;
    o << m->query << ' ' << m->nbIdx << ' ' << m->train << ' ' << (m->fromUnproc ? 1 : 0) << ' ' << bits(m->pos[0]) << ' ' << bits(m->pos[1]) << ' '
      << bits(m->pos[2]) << ' ' << (slot ? 1 : 0) << '\n';
  }
  return o.str();
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  World A = load(argv[1], true), B = load(argv[1], false);
  // loop 1 orders the neighbours by pointer (T2): give both runs the same order by sorting B's keyframes as A's pointers sort
  std::map<KeyFrame::SharedPtr, int> orderA;
  for (auto& k : A.kfs) orderA.emplace(k, 0);
  std::vector<KeyFrame::SharedPtr> sortedB(B.kfs.begin(), B.kfs.end());
  std::sort(sortedB.begin(), sortedB.end());
  std::vector<KeyFrame::SharedPtr> contents(B.kfs.size());
  {
    size_t r = 0;
    for (auto& it : orderA) {  // the r-th smallest pointer of B gets the contents of A's r-th neighbour
      KeyFrame& src = *B.kfs[(size_t)it.first->inputIdx];
      contents[r++] = std::make_shared<KeyFrame>(src);
    }
    for (size_t i = 0; i < sortedB.size(); ++i) *sortedB[i] = *contents[i];
    B.cur->conn = sortedB;
  }
  auto mapA = std::make_shared<Map>(), mapB = std::make_shared<Map>();
  std::list<MapPoint::SharedPtr> addedA, addedB;
  orbfe::dropin::createNewMapPoints<Camera, Frame>(A.cur, A.unproc, mapA, addedA);
  orbfe::dropin::KeyframeStore<Access> store(640, 480, (int)Frame::sf.size());
  {
    std::vector<KeyFrame::SharedPtr> all(sortedB);
    all.push_back(B.cur);
    for (const auto& kf : all) {  // as a fuse that ran first on this store leaves them: features and bounds, no stereo, no FeatureVector
      std::vector<uint8_t> d(kf->kps.size() * 32);
      for (size_t i = 0; i < kf->kps.size(); ++i) std::memcpy(&d[32 * i], kf->desc[i].data, 32);
      float b[4];
      Access::bounds(kf, b);
      if (orbfe_kfstore_add(store.get(), Access::id(kf), (int32_t)kf->kps.size(), (const orbfe_keypoint*)kf->kps.data(), d.data(), nullptr, nullptr, b) !=
          ORBFE_OK)
        return 5;
      orbfe_kfstore_info i;
      if (!store.info(kf, &i) || i.has_stereo || i.has_bow) return 5;
    }
  }
  orbfe::dropin::createNewMapPoints<Camera, Frame>(B.cur, B.unproc, mapB, addedB, store);
  int nStereo = 0;
  for (const auto& kf : sortedB) {
    orbfe_kfstore_info i;
    if (!store.info(kf, &i) || !i.has_stereo || !i.has_bow) return 6;  // replaced from the keyframe's getters
  }
  for (auto& m : addedB) nStereo += (m->fromUnproc && m->nbIdx >= 0) ? 1 : 0;  // own-stereo records: they need cur's depth and right_u
  const std::string a = dump(A, addedA), b = dump(B, addedB);
  if (a != b || A.unproc.size() != B.unproc.size() || store.size() != B.kfs.size() + 1) {
    std::fprintf(stderr, "differ: %zu vs %zu points added, %zu vs %zu unprocessed left, %zu stored\n", addedA.size(), addedB.size(), A.unproc.size(),
                 B.unproc.size(), store.size());
    return 1;
  }
  // a second call finds every keyframe resident: nothing is inserted, and with every slot now decided nothing is added
  const size_t before = addedB.size();
  orbfe::dropin::createNewMapPoints<Camera, Frame>(B.cur, B.unproc, mapB, addedB, store);
  if (store.size() != B.kfs.size() + 1) return 4;
  std::printf("OK %zu %zu %zu %d\n", addedA.size(), store.size(), addedB.size() - before, nStereo);
  return 0;
}

#else

struct Access {
  static uint64_t id(const KeyFrame::SharedPtr& k) { return (uint64_t)k->id; }
  static void bounds(const KeyFrame::SharedPtr& k, float b[4]) { orbfe::dropin::Bodies::bounds(k, b); }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  ORB_SLAM2_ROS2::ORBExtractor::mnLevels = 8;
  World A = load(argv[1]), B = load(argv[1]);
  if (dump(A) != dump(B)) return 3;
  // the selection iterates unordered sets of pointers: give B the order A's containers produce by running B on A's selection
  std::vector<int> kfOrder;
  std::vector<long> mpOrder;
  selection(A.cur, kfOrder, mpOrder);
  orbfe::dropin::fuseMapPoints<Camera, Frame>(A.cur, A.map);
  const int nFuseA = orbfe::dropin::fuseLastCount();
  const long long flagsA = orbfe::dropin::fuseDeviceFlagUses(), reevalA = orbfe::dropin::fuseReevaluations();
  // B: the same forward fuse and the same target order, the inverse fuses through the store
  orbfe::dropin::KeyframeStore<Access> store(640, 480, ORB_SLAM2_ROS2::ORBExtractor::mnLevels);
  std::vector<MapPoint::SharedPtr> vTargetMps;
  for (long id : mpOrder) vTargetMps.push_back(B.pts[id]);
  int nFuseB = orbfe::dropin::fuse(B.cur, vTargetMps, B.map, false, 3.0f, 0.6f, ORB_SLAM2_ROS2::ORBExtractor::mnLevels);
  std::vector<KeyFrame::SharedPtr> targets;
  for (int id : kfOrder) targets.push_back(B.kfs[id]);
  nFuseB += orbfe::dropin::fuseIntoKeyframes<Camera, Frame>(B.cur, targets, B.map, 0.6f, store);
  const long long flagsB = orbfe::dropin::fuseDeviceFlagUses(), reevalB = orbfe::dropin::fuseReevaluations();
  KeyFrame::updateConnections(B.cur);
  const std::string a = dump(A), b = dump(B);
  if (a != b || nFuseA != nFuseB || A.map->nReplaced != B.map->nReplaced || flagsA != flagsB || reevalA != reevalB || store.size() != kfOrder.size()) {
    std::fprintf(stderr, "maps differ: %d vs %d fuses, %d vs %d replaces, %lld vs %lld flags, %zu vs %zu bytes of state, %zu stored\n", nFuseA, nFuseB,
                 A.map->nReplaced, B.map->nReplaced, flagsA, flagsB, a.size(), b.size(), store.size());
    return 1;
  }
  // the whole one-line body on a third copy: it selects by its own pointers, so only its bookkeeping is compared
  World C = load(argv[1]);
  orbfe::dropin::fuseMapPoints<Camera, Frame>(C.cur, C.map, store);  // (same ids: every keyframe is resident already)
  if (store.size() != kfOrder.size() || KeyFrame::nUpdateConnections != 3) return 4;
  std::printf("OK %d %lld %lld %d %zu\n", nFuseB, flagsB, reevalB, B.map->nReplaced, kfOrder.size());
  return 0;
}

#endif
