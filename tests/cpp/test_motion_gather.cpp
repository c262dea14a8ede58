// orbfe::dropin::Bodies::trackMotionModelSlots (host/orbfe_dropin.hpp) WITHOUT a device: the body runs over stand-in Frame / MapPoint /
// Camera / extractor / store classes up to the device call, and this program defines orbfe_track_motion_model_slots and
// orbfe_get_capacity itself (the executable's definitions take the place of the library's): the stub records everything `in` points to
// and answers with a canned `out`.  Checked: the slots and pairs, the gathered flags and ids, the three poses, bounds, camera, level
// tables and parameters; what the store was asked to hold; the replayed side effects -- the temporary points created from temp_pos in
// feature order into the last frame and the caller's vector, addMatchInTrack per excluded hit and per accepted query, setMapPoints, the
// nulling, addInlierInTrack, setPose -- for each verdict; and every fallback condition (the fallback's first statement is the last
// frame's unProject, which throws here).
// Run by tests/test_track_motion_host.py.  Exit code 0 and one line "MOTION_GATHER_OK".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <stdexcept>

#include "../../orb_slam2_ros2_amd/host/orbfe_dropin.hpp"

// ---- the stub -------------------------------------------------------------------------------------------------------------------------
static const int kCap = 16;  // the fake context's capacity (features per frame)
static int g_cap = kCap;
struct Recorded {
  int calls = 0;
  orbfe_ctx* ctx = nullptr;
  int32_t slot = -1, pair = -1, lastSlot = -1, lastPair = -1;
  orbfe_mpstore* store = nullptr;
  orbfe_motion_slots_input in;
  std::vector<uint8_t> flags;
  std::vector<uint64_t> ids;
  std::vector<float> sig2, invSig2;
  orbfe_camera cam;
} g_rec;
struct Canned {
  int32_t verdict = 0;
  std::vector<int32_t> assigned, hits, qMatches;
  std::vector<uint8_t> inlier, temp;
  std::vector<float> tempPos;
  float Tcw[12];
} g_can;

extern "C" int32_t orbfe_get_capacity(const orbfe_ctx*) { return g_cap; }
extern "C" orbfe_status orbfe_track_motion_model_slots(orbfe_ctx* ctx, int32_t slot, int32_t pair, int32_t last_slot, int32_t last_pair,
                                                       orbfe_mpstore* store, const orbfe_motion_slots_input* in,
                                                       const orbfe_motion_slots_output* out) {
  Recorded& r = g_rec;
  ++r.calls, r.ctx = ctx, r.slot = slot, r.pair = pair, r.lastSlot = last_slot, r.lastPair = last_pair, r.store = store, r.in = *in;
  const size_t NF = (size_t)g_cap;
  r.flags.assign(in->last_flags, in->last_flags + NF), r.ids.assign(in->last_ids, in->last_ids + NF);
  r.sig2.assign(in->level_sigma2, in->level_sigma2 + 8), r.invSig2.assign(in->level_inv_sigma2, in->level_inv_sigma2 + 8);
  r.cam = *in->cam;
  const Canned& c = g_can;
  *out->verdict = c.verdict, *out->passes = 2, *out->n_matches = 0, *out->n_edges = 0, *out->n_inliers = 0, *out->n_in_map = 0;
  for (size_t f = 0; f < NF; ++f) {
    out->assigned[f] = f < c.assigned.size() ? c.assigned[f] : -1;
    out->final_assigned[f] = -1;
    out->excluded_hits[f] = f < c.hits.size() ? c.hits[f] : 0;
    out->query_matches[f] = f < c.qMatches.size() ? c.qMatches[f] : 0;
    out->inlier[f] = f < c.inlier.size() ? c.inlier[f] : 0;
    out->temp[f] = f < c.temp.size() ? c.temp[f] : 0;
    for (int a = 0; a < 3; ++a) out->temp_pos[3 * f + a] = 3 * f + a < c.tempPos.size() ? c.tempPos[3 * f + a] : 0.f;
  }
  std::memcpy(out->Tcw, c.Tcw, sizeof c.Tcw);
  return ORBFE_OK;
}

// ---- stand-ins with the reference's accessor names ----------------------------------------------------------------------------------
namespace ref {
struct Camera {
  static inline float mfFx = 718.856f, mfFy = 718.5f, mfCx = 607.1928f, mfCy = 185.2157f, mfBf = 386.1448f, mfBl = 0.537166f;
  static inline cv::Mat mDistCoeff;
};
struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  static inline std::size_t nextId = 500;
  static inline int created = 0;
  cv::Mat mPos;
  std::size_t mId = 0;
  bool mbBad = false, mbInMap = true;
  int nInlier = 0, nMatchInTrack = 0;
  static SharedPtr create(cv::Mat p3dW) {  // MapPoint::create(p3dW): a temporary point, not in the map
    auto p = std::make_shared<MapPoint>();
    p->mPos = p3dW.clone(), p->mId = nextId++, p->mbInMap = false;
    ++created;
    return p;
  }
  std::size_t getID() const { return mId; }
  bool isBad() const { return mbBad; }
  bool isInMap() const { return mbInMap; }
  cv::Mat getPos() const { return mPos.clone(); }
  void addInlierInTrack() { ++nInlier; }
  void addMatchInTrack() { ++nMatchInTrack; }
  template <class F>
  bool isInVision(F, float&, cv::Point2f&, float&) { return false; }  // (named by the fallback's bodies; never reached here)
};
struct FakeDevice {  // what the body asks of ORBExtractor::device()
  bool res = true;
  int sl = 0;
  orbfe_ctx* ctx = (orbfe_ctx*)(uintptr_t)0x1000;
  bool resident() const { return res; }
  orbfe_ctx* context() const { return ctx; }
  int slot() const { return sl; }
};
struct FakeExtractor {
  FakeDevice dev;
  const FakeDevice& device() const { return dev; }
};
struct Fallback : std::runtime_error {
  Fallback() : std::runtime_error("the bodies were taken") {}
};
struct Frame {
  static float getScaledFactor2(const int& l) { return std::pow(std::pow(1.2f, (float)l), 2); }
  static float getScaledFactorInv2(const int& l) { return std::pow(1.0f / std::pow(1.2f, (float)l), 2); }
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw, mtcw, mRwc, mtwc;
  float mfMaxU = 1241.f, mfMaxV = 376.f, mfMinU = 0.5f, mfMinV = 0.25f;
  std::shared_ptr<FakeExtractor> mpExtractorLeft = std::make_shared<FakeExtractor>(), mpExtractorRight = std::make_shared<FakeExtractor>();
  explicit Frame(int leftSlot, size_t n) : mvFeatsLeft(n), mvpMapPoints(n) { mpExtractorLeft->dev.sl = leftSlot, mpExtractorRight->dev.sl = leftSlot + 1; }
  int unProject(std::vector<MapPoint::SharedPtr>&) { throw Fallback(); }  // the first statement of the fallback
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  // (what the bodies of the fallback name; never reached here)
  std::vector<cv::Mat> mvLeftDescriptor;
  std::vector<double> mvFeatsRightU;
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
  const double& getRightU(const std::size_t& i) const { return mvFeatsRightU[i]; }
  MapPoint::SharedPtr getMapPoint(std::size_t idx) { return mvpMapPoints[idx]; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) { mvpMapPoints[(size_t)idx] = p; }
  void getPose(cv::Mat& R, cv::Mat& t) { R = mRcw.clone(), t = mtcw.clone(); }
  cv::Point2f project2UV(const cv::Mat&, bool& isPositive) { return isPositive = true, cv::Point2f(0, 0); }
  void setPose(cv::Mat T) {
    mRcw = cv::Mat(3, 3, CV_32F), mtcw = cv::Mat(3, 1, CV_32F), mRwc = cv::Mat(3, 3, CV_32F), mtwc = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) mRcw.at<float>(r, c) = T.at<float>(r, c), mRwc.at<float>(c, r) = T.at<float>(r, c);
      mtcw.at<float>(r, 0) = T.at<float>(r, 3);
    }
    for (int r = 0; r < 3; ++r) {
      float s = 0.f;
      for (int c = 0; c < 3; ++c) s += mRwc.at<float>(r, c) * mtcw.at<float>(c, 0);
      mtwc.at<float>(r, 0) = -s;
    }
  }
};
struct FakeStore {  // what the body asks of dropin::MapPointStore<>
  std::vector<uint64_t> ensured;
  template <class P>
  uint64_t id(const P& p) const { return (uint64_t)p->getID(); }
  template <class P>
  void ensure(const std::vector<P>& pts) {
    for (const auto& p : pts) ensured.push_back((uint64_t)p->getID());
  }
  orbfe_mpstore* get() const { return (orbfe_mpstore*)(uintptr_t)0x2000; }
};
}  // namespace ref

static int fails = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) fprintf(stderr, "line %d: %s\n", __LINE__, #cond), ++fails; \
  } while (0)

static cv::Mat pose4(float yaw, float tx, float ty, float tz) {
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T.at<float>(r, c) = r == c ? 1.f : 0.f;
  T.at<float>(0, 0) = std::cos(yaw), T.at<float>(0, 2) = -std::sin(yaw), T.at<float>(2, 0) = std::sin(yaw), T.at<float>(2, 2) = std::cos(yaw);
  T.at<float>(0, 3) = tx, T.at<float>(1, 3) = ty, T.at<float>(2, 3) = tz;
  return T;
}
static ref::MapPoint::SharedPtr point(std::size_t id, bool inMap = true, bool bad = false) {
  auto p = std::make_shared<ref::MapPoint>();
  p->mPos = cv::Mat(3, 1, CV_32F);
  p->mPos.at<float>(0) = (float)id, p->mPos.at<float>(1) = 1.f, p->mPos.at<float>(2) = 9.f;
  p->mId = id, p->mbInMap = inMap, p->mbBad = bad;
  return p;
}

struct World {
  std::shared_ptr<ref::Frame> cur, last;
  std::vector<ref::MapPoint::SharedPtr> pts;  // the last frame's points on entry
  ref::FakeStore store;
  std::vector<ref::MapPoint::SharedPtr> temps;
};
// Ten current features in slots 2 / 3, eight last-frame features in slots 0 / 1:
//   last 0: in-map point 40 | 1: local point 41 | 2: nothing | 3: a bad point 43 | 4: in-map point 44 | 5: nothing | 6: in-map 46 | 7: in-map 47
static World world() {
  World w;
  w.cur = std::make_shared<ref::Frame>(2, 10), w.last = std::make_shared<ref::Frame>(0, 8);
  w.cur->setPose(pose4(0.02f, 0.1f, 0.2f, 0.3f)), w.last->setPose(pose4(-0.01f, 0.4f, 0.5f, 0.6f));
  w.pts = {point(40), point(41, false), nullptr, point(43, true, true), point(44), nullptr, point(46), point(47)};
  w.last->mvpMapPoints = w.pts;
  return w;
}
static bool run(World& w) { return orbfe::dropin::Bodies::trackMotionModelSlots<ref::Camera>(w.store, w.cur, w.last, w.temps); }

int main() {
  // the device's answer: temporaries at last features 2 and 3 (the bad point's feature has depth, 5 has none); search 1 gave frame
  // feature 1 <- last 0, 4 <- last 2 (a temporary), 6 <- last 4, 7 <- last 6, 8 <- last 7; last 1 was accepted twice but lost its feature
  // both times; feature 6 was met three times as an excluded candidate; the optimisation kept 1, 4 and 8
  g_can.assigned = {-1, 0, -1, -1, 2, -1, 4, 6, 7, -1};
  g_can.hits = {0, 0, 0, 0, 1, 0, 3, 0, 0, 0};
  g_can.qMatches = {1, 2, 1, 0, 1, 0, 1, 1};
  g_can.inlier = {0, 1, 0, 0, 1, 0, 0, 0, 1, 0};
  g_can.temp = {0, 0, 1, 1, 0, 0, 0, 0};
  g_can.tempPos.assign(24, 0.f);
  for (int a = 0; a < 3; ++a) g_can.tempPos[6 + a] = 2.5f + a, g_can.tempPos[9 + a] = -1.25f * (a + 1);
  const float T[12] = {0.6f, 0.f, -0.8f, 0.f, 1.f, 0.f, 0.8f, 0.f, 0.6f, 1.5f, -2.5f, 3.5f};
  std::memcpy(g_can.Tcw, T, sizeof T);

  for (int verdict = 1; verdict <= 3; ++verdict) {
    g_can.verdict = verdict;
    g_rec = Recorded();
    ref::MapPoint::created = 0;
    const std::size_t firstNew = ref::MapPoint::nextId;
    World w = world();
    const cv::Mat R0 = w.cur->mRcw.clone();
    const bool ok = run(w);
    EXPECT(ok == (verdict == ORBFE_MOTION_ACCEPT));
    // what went to the device
    const Recorded& r = g_rec;
    EXPECT(r.calls == 1 && r.ctx == (orbfe_ctx*)(uintptr_t)0x1000 && r.store == (orbfe_mpstore*)(uintptr_t)0x2000);
    EXPECT(r.slot == 2 && r.pair == 1 && r.lastSlot == 0 && r.lastPair == 0);
    const uint8_t wantFlags[8] = {3, 1, 0, 0, 3, 0, 3, 3};
    const uint64_t wantIds[8] = {40, 41, 0, 0, 44, 0, 46, 47};
    for (int i = 0; i < kCap; ++i) EXPECT(r.flags[(size_t)i] == (i < 8 ? wantFlags[i] : 0) && r.ids[(size_t)i] == (i < 8 ? wantIds[i] : 0));
    EXPECT((w.store.ensured == std::vector<uint64_t>{40, 41, 44, 46, 47}));
    EXPECT(r.in.last_pos == nullptr);
    for (int k = 0; k < 9; ++k) {
      EXPECT(r.in.Rcw[k] == R0.at<float>(k / 3, k % 3) && r.in.last_Rcw[k] == w.last->mRcw.at<float>(k / 3, k % 3));
      EXPECT(r.in.last_Rwc[k] == w.last->mRwc.at<float>(k / 3, k % 3));
    }
    EXPECT(r.in.tcw[0] == 0.1f && r.in.tcw[1] == 0.2f && r.in.tcw[2] == 0.3f && r.in.last_tcw[2] == 0.6f);
    for (int k = 0; k < 3; ++k) EXPECT(r.in.last_twc[k] == w.last->mtwc.at<float>(k, 0));
    EXPECT(r.in.bounds[0] == 0.5f && r.in.bounds[1] == 1241.f && r.in.bounds[2] == 0.25f && r.in.bounds[3] == 376.f);
    EXPECT(r.cam.fx == 718.856f && r.cam.fy == 718.5f && r.cam.cx == 607.1928f && r.cam.cy == 185.2157f && r.cam.bf == 386.1448f && r.in.baseline == 0.537166f);
    for (int l = 0; l < 8; ++l) EXPECT(r.sig2[(size_t)l] == ref::Frame::getScaledFactor2(l) && r.invSig2[(size_t)l] == ref::Frame::getScaledFactorInv2(l));
    EXPECT(r.in.th == 15.f && r.in.th_second == 30.f && r.in.ratio == 0.9f && r.in.min_threshold == 50 && r.in.min_matches == 20 && r.in.min_inliers == 10);
    // Frame::unProject replayed: two new points in feature order at the device's positions, the bad point replaced, the null one without
    // depth still null; the caller's vector is the last frame's
    EXPECT(ref::MapPoint::created == 2);
    auto& L = w.last->mvpMapPoints;
    EXPECT(L.size() == 8 && w.temps == L && L[0] == w.pts[0] && L[1] == w.pts[1] && L[4] == w.pts[4] && L[6] == w.pts[6] && L[7] == w.pts[7] && !L[5]);
    EXPECT(L[2] && L[3] && L[2]->getID() == firstNew && L[3]->getID() == firstNew + 1 && !L[2]->isInMap() && L[3] != w.pts[3]);
    EXPECT(L[2] && L[2]->mPos.at<float>(0) == 2.5f && L[2]->mPos.at<float>(2) == 4.5f && L[3] && L[3]->mPos.at<float>(1) == -2.5f);
    // the searches' side effects: query matches, plus the excluded hits of the point the feature ended up with
    const int wantMatch[8] = {1, 2, 1 + 1, 0, 1 + 3, 0, 1, 1};
    for (int i = 0; i < 8; ++i)
      if (L[(size_t)i]) EXPECT(L[(size_t)i]->nMatchInTrack == wantMatch[i]);
    EXPECT(w.pts[3]->nMatchInTrack == 0);
    auto& C = w.cur->mvpMapPoints;
    if (verdict == ORBFE_MOTION_REJECT_MATCHES) {  // the frame is written, nothing else happened
      for (int f = 0; f < 10; ++f) EXPECT(C[(size_t)f] == (g_can.assigned[(size_t)f] >= 0 ? L[(size_t)g_can.assigned[(size_t)f]] : nullptr));
      for (const auto& p : L) EXPECT(!p || p->nInlier == 0);
      EXPECT(w.cur->mRcw.at<float>(0, 0) == R0.at<float>(0, 0) && w.cur->mtcw.at<float>(0, 0) == 0.1f);
    } else {  // OptimizePoseOnly's tail: the inliers stay and count, the others are emptied, the pose is the device's Tcw
      for (int f = 0; f < 10; ++f) EXPECT(C[(size_t)f] == (g_can.inlier[(size_t)f] ? L[(size_t)g_can.assigned[(size_t)f]] : nullptr));
      EXPECT(L[0]->nInlier == 1 && L[2]->nInlier == 1 && L[7]->nInlier == 1 && L[4]->nInlier == 0 && L[6]->nInlier == 0 && L[1]->nInlier == 0);
      for (int k = 0; k < 9; ++k) EXPECT(w.cur->mRcw.at<float>(k / 3, k % 3) == T[k]);
      for (int k = 0; k < 3; ++k) EXPECT(w.cur->mtcw.at<float>(k, 0) == T[9 + k]);
    }
  }
  // ---- every fallback condition takes the bodies (whose first statement throws here) and makes no device call ----
  auto falls = [&](const char* what, const std::function<void(World&)>& change) {
    World w = world();
    change(w);
    g_rec = Recorded();
    bool threw = false;
    try {
      run(w);
    } catch (const ref::Fallback&) {
      threw = true;
    }
    if (!threw || g_rec.calls != 0) fprintf(stderr, "no fallback: %s\n", what), ++fails;
  };
  falls("the current left slot is no longer resident", [](World& w) { w.cur->mpExtractorLeft->dev.res = false; });
  falls("the current right slot is no longer resident", [](World& w) { w.cur->mpExtractorRight->dev.res = false; });
  falls("the last left slot is no longer resident", [](World& w) { w.last->mpExtractorLeft->dev.res = false; });
  falls("the last frame has no right extractor", [](World& w) { w.last->mpExtractorRight.reset(); });
  falls("the last frame is no slot pair", [](World& w) { w.last->mpExtractorRight->dev.sl = 3; });
  falls("an odd left slot", [](World& w) { w.cur->mpExtractorLeft->dev.sl = 1, w.cur->mpExtractorRight->dev.sl = 2; });
  falls("both frames in one slot", [](World& w) { w.cur->mpExtractorLeft->dev.sl = 0, w.cur->mpExtractorRight->dev.sl = 1; });
  falls("two contexts", [](World& w) {
    w.last->mpExtractorLeft->dev.ctx = (orbfe_ctx*)(uintptr_t)0x1100, w.last->mpExtractorRight->dev.ctx = (orbfe_ctx*)(uintptr_t)0x1100;
  });
  falls("the current frame holds a point", [](World& w) { w.cur->mvpMapPoints[3] = point(90); });
  g_cap = 2049;
  falls("more than 2048 features", [](World&) {});
  g_cap = kCap;
  ref::Camera::mDistCoeff = cv::Mat(1, 5, CV_32F);
  for (int i = 0; i < 5; ++i) ref::Camera::mDistCoeff.at<float>(i) = i == 1 ? 0.01f : 0.f;
  falls("a distorting camera", [](World&) {});
  ref::Camera::mDistCoeff = cv::Mat();
  // a bad point the current frame holds does not count as held
  {
    World w = world();
    w.cur->mvpMapPoints[3] = point(91, true, true);
    g_rec = Recorded();
    g_can.verdict = 1;
    run(w);
    EXPECT(g_rec.calls == 1);
  }
  printf("MOTION_GATHER_%s\n", fails == 0 ? "OK" : "FAIL");
  return fails == 0 ? 0 : 1;
}
