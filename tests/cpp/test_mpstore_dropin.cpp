// orbfe::dropin::trackLocalMap(store, ...) (orbfe_mpstore_dropin.hpp: the local map points named by id in a device-resident map-point
// store, orbfe_track_local_map_stored) against the existing orbfe::dropin::trackLocalMap (orbfe_track_local_map with the points'
// arrays), on stand-in Frame / MapPoint / Camera classes with the reference's accessor names, over the stand-in opencv2/core.hpp of
// tests/cpp/stubs, linked to liborbfe_hip.so.
//   test_mpstore_dropin compare <L.raw> <R.raw> <w> <h>
//   test_mpstore_dropin latency <L.raw> <R.raw> <w> <h> <iterations>
// compare: twin frames and twin local maps (test_dropin.cpp's trackchain scene); A goes through the array overload, B through the
// store.  Rounds, each on fresh frames: as built; after setPos on some points of both maps WITH touch on B's; after setPos with touch of
// points that are OUTSIDE the list for two frames and then return; after a change
// of B's twin of further points WITHOUT touch, which verify() must name -- exactly those ids -- before a touch repairs it.  Compared,
// all of it exactly (the same kernels run on the same arrays): the return value, nGood, the map point of every feature, the counters of
// every map point, the pose to the bit.  Exit code 0 and one line "MPSTORE_DROPIN_OK ...".
// latency: the time of the two overloads up to and including the device call (and whole), on the same frame and list, interleaved,
// measured over THESE STAND-IN CLASSES (an accessor is
// a cv::Mat clone without the reference's mutex), not over the reference's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../orb_slam2_ros2_amd/host/orbfe_mpstore_dropin.hpp"

namespace ref {  // ---- stand-ins with the reference's accessor names ----------------------------------------------------------------
struct Camera {
  static inline float mfFx = 718.856f, mfFy = 718.856f, mfCx = 607.1928f, mfCy = 185.2157f, mfBf = 718.856f * 0.537166f, mfBl = 0.537166f;
  static inline cv::Mat mDistCoeff;
};

struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  std::size_t mId = 0;
  cv::Mat mPos, mView, mDesc;
  float mMax = 0.f, mMin = 0.f;
  bool mbBad = false, mbInMap = true;
  int nInlier = 0, nMatchInTrack = 0;
  static inline long nAccessorCalls = 0;  // getPos / getViewDirection / getDistance / getDesc
  std::size_t getID() { return mId; }
  bool isBad() const { return mbBad; }
  bool isInMap() const { return mbInMap; }
  cv::Mat getPos() const { return ++nAccessorCalls, mPos.clone(); }
  void setPos(cv::Mat p) { mPos = p.clone(); }
  cv::Mat getViewDirection() const { return ++nAccessorCalls, mView.clone(); }
  void getDistance(float& mx, float& mn) const { ++nAccessorCalls, mx = mMax, mn = mMin; }
  cv::Mat getDesc() { return ++nAccessorCalls, mDesc; }
  void addInlierInTrack() { ++nInlier; }
  void addMatchInTrack() { ++nMatchInTrack; }
  // MapPoint::isInVision / predictLevel (src/MapPoint.cc:141-201) in the reference's float / double mix: the fall-back bodies call them
  template <class FramePtr>
  bool isInVision(FramePtr f, float& dist, cv::Point2f& uv, float& cosTheta) {
    float R[9], t[3], X[3], D[3], pc[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R[3 * r + c] = f->mRcw.template at<float>(r, c);
      t[r] = f->mtcw.template at<float>(r, 0), X[r] = mPos.at<float>(r), D[r] = mView.at<float>(r);
    }
    for (int r = 0; r < 3; ++r) {
      const float s = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2];
      pc[r] = (float)((double)s + (double)t[r]);
    }
    if (pc[2] < 0.f) return false;
    const float distance = std::sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
    dist = distance;
    if (!(distance < mMax && distance > mMin)) return false;
    const float u = pc[0] / pc[2] * Camera::mfFx + Camera::mfCx, v = pc[1] / pc[2] * Camera::mfFy + Camera::mfCy;
    uv.x = u, uv.y = v;
    if (!(u < f->mfMaxU && v < f->mfMaxV && u > f->mfMinU && v > f->mfMinV)) return false;
    float vd[3];
    for (int r = 0; r < 3; ++r) vd[r] = R[3 * r] * D[0] + R[3 * r + 1] * D[1] + R[3 * r + 2] * D[2];
    const double nn = (double)vd[0] * vd[0] + (double)vd[1] * vd[1] + (double)vd[2] * vd[2];
    const double dot = (double)vd[0] * pc[0] + (double)vd[1] * pc[1] + (double)vd[2] * pc[2];
    cosTheta = (float)(dot / (double)(distance * (float)std::sqrt(nn)));
    return !(cosTheta < 0.5f);
  }
  int predictLevel(float distance) const {
    const int level = (int)std::lrintf((float)std::log((double)(mMax / distance)) / std::log(1.2f));
    return level < 0 ? 0 : (level > 7 ? 7 : level);
  }
};

struct Frame {
  typedef std::shared_ptr<Frame> SharedPtr;
  static inline std::vector<float> mvfScaledFactors;
  static float getScaledFactor(const int& l) { return mvfScaledFactors[l]; }
  static float getScaledFactor2(const int& l) { return std::pow(getScaledFactor(l), 2); }
  static float getScaledFactorInv(const int& l) { return 1.0f / getScaledFactor(l); }
  static float getScaledFactorInv2(const int& l) { return std::pow(getScaledFactorInv(l), 2); }
  cv::Mat mLeftIm, mRightIm;
  ORB_SLAM2_ROS2::ORBExtractor::SharedPtr mpExtractorLeft, mpExtractorRight;
  std::vector<cv::KeyPoint> mvFeatsLeft, mvFeatsRight;
  std::vector<cv::Mat> mvLeftDescriptor, mRightDescriptor;
  std::vector<double> mvDepths, mvFeatsRightU;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw, mtcw;
  float mfMaxU = 0, mfMaxV = 0, mfMinU = 0, mfMinV = 0;
  int mnN = 0;
  Frame(cv::Mat l, cv::Mat r) : mLeftIm(l), mRightIm(r) {  // Frame::Frame stereo (src/Frame.cc:85-111), on one thread
    mpExtractorLeft = std::make_shared<ORB_SLAM2_ROS2::ORBExtractor>(mLeftIm, 2000, 8, 1.2f, "", 20, 7);
    mpExtractorRight = std::make_shared<ORB_SLAM2_ROS2::ORBExtractor>(mRightIm, 2000, 8, 1.2f, "", 20, 7);
    mpExtractorLeft->extract(mvFeatsLeft, mvLeftDescriptor);
    mpExtractorRight->extract(mvFeatsRight, mRightDescriptor);
    mvpMapPoints.resize(mvFeatsLeft.size(), nullptr);
  }
  const std::vector<cv::Mat>& getLeftDescriptor() const { return mvLeftDescriptor; }
  MapPoint::SharedPtr getMapPoint(std::size_t idx) { return mvpMapPoints[idx]; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) { mvpMapPoints[idx] = p; }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
  const cv::KeyPoint& getLeftKeyPoint(const std::size_t& i) const { return mvFeatsLeft[i]; }
  const double& getRightU(const std::size_t& i) const { return mvFeatsRightU[i]; }
  void setPose(cv::Mat T) {
    mRcw = cv::Mat(3, 3, CV_32F), mtcw = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) mRcw.at<float>(r, c) = T.at<float>(r, c);
      mtcw.at<float>(r, 0) = T.at<float>(r, 3);
    }
  }
  void getPose(cv::Mat& R, cv::Mat& t) { R = mRcw.clone(), t = mtcw.clone(); }
  cv::Point2f project2UV(const cv::Mat& p3dW, bool& isPositive) {  // VirtualFrame::project2UV: float pose, pinhole
    float pc[3];
    for (int r = 0; r < 3; ++r)
      pc[r] = mRcw.at<float>(r, 0) * p3dW.at<float>(0) + mRcw.at<float>(r, 1) * p3dW.at<float>(1) + mRcw.at<float>(r, 2) * p3dW.at<float>(2) +
              mtcw.at<float>(r, 0);
    isPositive = pc[2] > 0;
    return cv::Point2f(pc[0] / pc[2] * Camera::mfFx + Camera::mfCx, pc[1] / pc[2] * Camera::mfFy + Camera::mfCy);
  }
};
}  // namespace ref

using PointList = std::vector<ref::MapPoint::SharedPtr>;

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (int c; (c = fgetc(f)) != EOF;) out.push_back((uint8_t)c);
  fclose(f);
  return true;
}

static uint64_t g_seed = 777;
static double rnd() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_seed >> 11) / 9007199254740992.0;
}

static ref::Frame::SharedPtr make_frame(const cv::Mat& ml, const cv::Mat& mr, int w, int h) {
  auto f = std::make_shared<ref::Frame>(ml, mr);
  ref::Frame::mvfScaledFactors = ORB_SLAM2_ROS2::ORBExtractor::getScaledFactors();
  orbfe::dropin::searchByStereo<ref::Camera>(f);
  f->mfMinU = 0, f->mfMinV = 0, f->mfMaxU = (float)w, f->mfMaxV = (float)h;
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T.at<float>(r, c) = r == c ? 1.f : 0.f;
  T.at<float>(0, 3) = 0.04f, T.at<float>(1, 3) = -0.02f, T.at<float>(2, 3) = 0.05f;  // the estimate: a few centimetres off the truth (identity)
  f->setPose(T);
  return f;
}

// the local map, twice: most keypoints back-projected at their stereo depth (true pose = identity), descriptors a few bits off; points
// that project nowhere near a feature; bad / not-in-map points; null entries; a point listed twice.  Ids with gaps, in no order.
static void make_map(const ref::Frame& F, PointList& listA, PointList& listB, PointList& extraA, PointList& extraB) {
  auto add = [&](PointList& la, PointList& lb, const float* X, const cv::Mat& desc, bool bad, bool inMap, size_t id) {
    for (auto* lst : {&la, &lb}) {
      auto p = std::make_shared<ref::MapPoint>();
      p->mId = id;
      p->mPos = cv::Mat(3, 1, CV_32F), p->mView = cv::Mat(3, 1, CV_32F);
      const float nrm = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
      for (int a = 0; a < 3; ++a) p->mPos.at<float>(a) = X[a], p->mView.at<float>(a) = X[a] / nrm;
      p->mMax = nrm * 1.8f, p->mMin = nrm * 0.6f;
      p->mDesc = desc.clone();
      p->mbBad = bad, p->mbInMap = inMap;
      lst->push_back(p);
    }
  };
  const size_t n = F.mvFeatsLeft.size();
  size_t next = 0;
  auto id = [&] {  // descending, gapped, unique: the list is in no id order
    const size_t k = next++;
    return 100000 - 5 * k + k % 3;
  };
  for (size_t i = 0; i < n; ++i) {
    if (i % 5 == 4) continue;
    const auto& kp = F.mvFeatsLeft[i];
    const double d = F.mvDepths[i] > 0 ? F.mvDepths[i] : 6.0 + 20.0 * rnd();
    const float X[3] = {(float)((kp.pt.x - ref::Camera::mfCx) / ref::Camera::mfFx * d), (float)((kp.pt.y - ref::Camera::mfCy) / ref::Camera::mfFy * d), (float)d};
    cv::Mat desc = F.mvLeftDescriptor[i].clone();
    for (int k = 0; k < 5; ++k) {
      const int bit = (int)(rnd() * 256) % 256;
      desc.data[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    }
    add(listA, listB, X, desc, i % 61 == 7, i % 47 != 9, id());
  }
  for (int i = 0; i < 200; ++i) {
    const float X[3] = {(float)(-15 + 30 * rnd()), (float)(-4 + 8 * rnd()), (float)(3 + 30 * rnd())};
    cv::Mat desc(1, 32, CV_8U);
    for (int k = 0; k < 32; ++k) desc.data[k] = (uint8_t)(rnd() * 256);
    add(listA, listB, X, desc, false, true, id());
  }
  listA.insert(listA.begin() + 10, nullptr), listB.insert(listB.begin() + 10, nullptr);  // the reference's lists hold null entries
  listA.push_back(listA[20]), listB.push_back(listB[20]);                                // ... and may name a point twice
  for (int i = 0; i < 40; ++i) {  // points a frame may hold that are not in the local map (processLastFrame's temporary points)
    const float X[3] = {1.f + 0.05f * i, 0.5f, 9.f + 0.1f * i};
    cv::Mat desc(1, 32, CV_8U);
    std::memset(desc.data, 0, 32);
    add(extraA, extraB, X, desc, i % 10 == 3, true, 200000 + 17 * (size_t)i);
  }
}

// what a frame holds on entry: a fifth of the features a point of the list, some of them a point outside it
static void hold(ref::Frame& F, const PointList& list, const PointList& extra) {
  uint64_t s = 4242;
  for (size_t i = 0; i < F.mvpMapPoints.size(); ++i)
    if (i % 5 == 1) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const size_t j = (size_t)(s >> 33) % list.size();
      if (i % 25 == 1)
        F.mvpMapPoints[i] = extra[(i / 25) % extra.size()];
      else if (list[j])
        F.mvpMapPoints[i] = list[j];
    }
}

static int g_fails = 0;
static void expect(bool ok, const char* round, const char* what) {
  if (!ok) fprintf(stderr, "%s: %s\n", round, what), ++g_fails;
}

static size_t index_in(const PointList& list, const PointList& extra, const ref::MapPoint::SharedPtr& p) {
  const auto a = std::find(list.begin(), list.end(), p);
  if (a != list.end()) return (size_t)(a - list.begin());
  return list.size() + (size_t)(std::find(extra.begin(), extra.end(), p) - extra.begin());
}

static int mode_compare(int argc, char** argv) {
  if (argc < 6) return 2;
  const int w = atoi(argv[4]), h = atoi(argv[5]);
  std::vector<uint8_t> L, R;
  if (!read_file(argv[2], L) || !read_file(argv[3], R) || L.size() != (size_t)w * h || R.size() != L.size()) return 2;
  cv::Mat ml(h, w, CV_8UC1, L.data()), mr(h, w, CV_8UC1, R.data());
  PointList listA, listB, extraA, extraB;
  {
    auto F0 = make_frame(ml, mr, w, h);
    make_map(*F0, listA, listB, extraA, extraB);
  }
  orbfe::dropin::MapPointStore<> store(0, 4096, 64);  // pages of 4096 rows: the ids above span several
  int nA0 = 0, goodA0 = 0, kept0 = 0;
  auto round = [&](const char* name, const PointList& listA, const PointList& listB) {
    auto FA = make_frame(ml, mr, w, h), FB = make_frame(ml, mr, w, h);
    hold(*FA, listA, extraA), hold(*FB, listB, extraB);
    for (const PointList* lst : std::initializer_list<const PointList*>{&listA, &listB, &extraA, &extraB})
      for (const auto& p : *lst)
        if (p) p->nInlier = p->nMatchInTrack = 0;
    int goodA = -2, goodB = -2;
    const int nA = orbfe::dropin::trackLocalMap<ref::Camera>(FA, listA, 3.f, goodA);
    const int nB = orbfe::dropin::trackLocalMap<ref::Camera>(store, FB, listB, 3.f, goodB);
    expect(nA == nB, name, "the return value differs");
    expect(goodA == goodB, name, "nGood differs");
    int kept = 0, assign_diff = 0;
    for (size_t i = 0; i < FA->mvpMapPoints.size(); ++i) {
      const auto a = FA->mvpMapPoints[i], b = FB->mvpMapPoints[i];
      if ((a == nullptr) != (b == nullptr) || (a && index_in(listA, extraA, a) != index_in(listB, extraB, b))) ++assign_diff;
      kept += a != nullptr;
    }
    expect(assign_diff == 0, name, "the frames' map points differ");
    int cnt_diff = 0;
    for (size_t i = 0; i < listA.size(); ++i)
      if (listA[i]) cnt_diff += listA[i]->nMatchInTrack != listB[i]->nMatchInTrack || listA[i]->nInlier != listB[i]->nInlier;
    for (size_t i = 0; i < extraA.size(); ++i) cnt_diff += extraA[i]->nMatchInTrack != extraB[i]->nMatchInTrack || extraA[i]->nInlier != extraB[i]->nInlier;
    expect(cnt_diff == 0, name, "addMatchInTrack / addInlierInTrack counts differ");
    bool pose_same = true;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose_same = pose_same && !std::memcmp(&FA->mRcw.at<float>(r, c), &FB->mRcw.at<float>(r, c), 4);
      pose_same = pose_same && !std::memcmp(&FA->mtcw.at<float>(r, 0), &FB->mtcw.at<float>(r, 0), 4);
    }
    expect(pose_same, name, "the optimised poses differ");
    expect(nA > 800 && goodA > 300, name, "the scene is too thin to say anything");
    nA0 = nA, goodA0 = goodA, kept0 = kept;
  };
  round("as built", listA, listB);
  const int n1 = nA0, g1 = goodA0;
  expect(store.verify(listB).empty() && store.verify(extraB).empty(), "as built", "verify names points that did not change");
  expect(store.size() > 1500, "as built", "the store holds fewer points than the list");
  // the first call read every point's accessors once (ensure); the next one reads none
  {
    auto FB = make_frame(ml, mr, w, h);
    hold(*FB, listB, extraB);
    const long before = ref::MapPoint::nAccessorCalls;
    int good = 0;
    orbfe::dropin::trackLocalMap<ref::Camera>(store, FB, listB, 3.f, good);
    long tail = 0;  // (the replay's getPos per inlier, as in the array overload)
    for (const auto& p : FB->mvpMapPoints) tail += p != nullptr;
    expect(ref::MapPoint::nAccessorCalls - before <= tail + 200, "second call", "the stored overload read the accessors of points that did not change");
  }
  // setPos on every seventh point of both maps, WITH touch on the store's side
  auto move = [&](ref::MapPoint& p, float by) {
    cv::Mat q = p.mPos.clone();
    q.at<float>(0) += by, q.at<float>(2) -= 0.5f * by;
    p.setPos(q);
  };
  for (size_t i = 0; i < listA.size(); i += 7)
    if (listA[i]) {
      move(*listA[i], 0.03f), move(*listB[i], 0.03f);
      store.touch(listB[i]->getID());
    }
  store.touch(123456789);  // a touch of a point the store has never seen is dropped at the flush
  round("after setPos with touch", listA, listB);
  expect(store.verify(listB).empty(), "after setPos with touch", "verify names points whose touch was flushed");
  // a point that changes, WITH touch, while it is OUTSIDE the local map: a frame passes without it, then it comes back -- and must be
  // tracked with its new position, as the array overload tracks it (the move is large enough to change what it matches)
  {
    PointList awayA, awayB, restA, restB;
    for (size_t i = 0; i < listA.size(); ++i) {
      const bool away = listA[i] && i % 13 == 5 && i != 20 && i + 1 != listA.size();
      (away ? awayA : restA).push_back(listA[i]), (away ? awayB : restB).push_back(listB[i]);
    }
    for (size_t k = 0; k < awayA.size(); ++k) {
      move(*awayA[k], 0.4f), move(*awayB[k], 0.4f);
      store.touch(awayB[k]->getID());
    }
    round("touched while outside the list", restA, restB);
    expect(awayB.size() > 100 && store.staleCount() == awayB.size(), "touched while outside the list", "the touched points are not all kept as stale");
    round("a second frame without them", restA, restB);
    expect(store.staleCount() == awayB.size(), "a second frame without them", "stale points were forgotten");
    round("back in the list", listA, listB);
    expect(store.staleCount() == 0 && store.verify(listB).empty(), "back in the list", "the returning points were not read again");
  }
  // a change WITHOUT touch: verify names exactly those ids, the overloads disagree until the touch comes
  std::vector<uint64_t> silent;
  for (size_t i = 3; i < listB.size(); i += 11)
    if (listB[i] && i != 20 && i + 1 != listB.size()) {
      if (i % 2)
        move(*listB[i], 0.5f), move(*listA[i], 0.5f);
      else
        listB[i]->mDesc.data[5] ^= 0x10, listA[i]->mDesc.data[5] ^= 0x10;
      silent.push_back(listB[i]->getID());
    }
  std::vector<uint64_t> named = store.verify(listB);
  std::sort(silent.begin(), silent.end()), std::sort(named.begin(), named.end());
  expect(silent.size() > 100 && named == silent, "change without touch", "verify does not name exactly the changed ids");
  for (uint64_t i : silent) store.touch(i);
  {  // flush with a lookup, as an integrator with a map-wide index by id calls it: the stale points it reaches are read at once
    std::map<uint64_t, ref::MapPoint::SharedPtr> byId;
    for (const auto& p : listB)
      if (p) byId[p->getID()] = p;
    const uint64_t unreachable = silent.front();
    store.flush([&](uint64_t id) { return id == unreachable ? ref::MapPoint::SharedPtr() : byId[id]; });
    expect(store.staleCount() == 1 && store.verify(listB) == std::vector<uint64_t>{unreachable}, "flush with a lookup", "the reachable stale points were not read");
  }
  round("after the late touch", listA, listB);
  expect(store.verify(listB).empty(), "after the late touch", "verify still names points");
  // erase: the points go in again from their accessors on the next call
  std::vector<uint64_t> some;
  for (size_t i = 0; i < 50; ++i)
    if (listB[i]) some.push_back(listB[i]->getID());
  const size_t held = store.size();
  for (size_t k = 0; k < 5; ++k) store.touch(some[k]);
  store.flush();
  expect(store.staleCount() == 5, "erase", "touched points are not stale after flush()");
  store.erase(some);
  expect(store.staleCount() == 0, "erase", "erased ids stay in the stale set");
  expect(store.size() == held - some.size(), "erase", "the store's size after erase");
  round("after erase", listA, listB);
  expect(store.size() == held, "after erase", "the erased points did not come back");
  printf("MPSTORE_DROPIN_OK %d %d %d %d %zu %zu\n", n1, g1, nA0, kept0, silent.size(), store.size());
  return g_fails == 0 ? 0 : 1;
}

static int mode_latency(int argc, char** argv) {
  if (argc < 7) return 2;
  const int w = atoi(argv[4]), h = atoi(argv[5]), iters = std::max(atoi(argv[6]), 5);
  std::vector<uint8_t> L, R;
  if (!read_file(argv[2], L) || !read_file(argv[3], R) || L.size() != (size_t)w * h || R.size() != L.size()) return 2;
  cv::Mat ml(h, w, CV_8UC1, L.data()), mr(h, w, CV_8UC1, R.data());
  PointList listA, listB, extraA, extraB;
  auto F = make_frame(ml, mr, w, h);
  make_map(*F, listA, listB, extraA, extraB);
  orbfe::dropin::MapPointStore<> store;
  const auto held0 = F->mvpMapPoints;
  cv::Mat R0 = F->mRcw.clone(), t0 = F->mtcw.clone();
  std::vector<double> ta, ts, tca, tcs;  // whole overload | up to and including the device call
  using Clock = std::chrono::steady_clock;
  for (int it = -3; it < iters; ++it) {  // interleaved, three warm-up rounds; the frame is put back before every call
    for (int which = 0; which < 2; ++which) {
      F->mvpMapPoints = held0, F->mRcw = R0.clone(), F->mtcw = t0.clone();
      int good = 0;
      Clock::time_point deviceDone;
      const auto a = Clock::now();
      if (which == 0)
        orbfe::dropin::Bodies::trackLocalMap<ref::Camera>(F, listA, 3.f, 0.8f, 8, good, 30, &deviceDone);
      else
        orbfe::dropin::Bodies::trackLocalMapStored<ref::Camera>(store, F, listB, 3.f, 0.8f, 8, good, 30, &deviceDone);
      const auto b = Clock::now();
      if (it < 0) continue;
      (which == 0 ? ta : ts).push_back(std::chrono::duration<double, std::milli>(b - a).count());
      (which == 0 ? tca : tcs).push_back(std::chrono::duration<double, std::milli>(deviceDone - a).count());
    }
  }
  for (auto* t : {&ta, &ts, &tca, &tcs}) std::sort(t->begin(), t->end());
  // to_call: the marshalling up to and including the device call; whole: with the side-effect replay (Bodies::trackLocalMapReplay, one
  // function for both overloads) behind it
  printf("MPSTORE_LATENCY stand-in-classes points=%zu iters=%d arrays_to_call_ms_p50=%.4f arrays_to_call_ms_p10=%.4f stored_to_call_ms_p50=%.4f "
         "stored_to_call_ms_p10=%.4f arrays_whole_ms_p50=%.4f stored_whole_ms_p50=%.4f\n",
         listA.size(), iters, tca[tca.size() / 2], tca[tca.size() / 10], tcs[tcs.size() / 2], tcs[tcs.size() / 10], ta[ta.size() / 2], ts[ts.size() / 2]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    if (!strcmp(argv[1], "compare")) return mode_compare(argc, argv);
    if (!strcmp(argv[1], "latency")) return mode_latency(argc, argv);
  } catch (const std::exception& e) {
    if (strstr(e.what(), "no HIP device") || strstr(e.what(), "no usable HIP device")) {
      printf("NO_DEVICE\n");
      return 3;
    }
    fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  return 2;
}
