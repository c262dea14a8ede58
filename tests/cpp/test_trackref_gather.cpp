// orbfe::dropin::Bodies::trackReference (host/orbfe_dropin.hpp) WITHOUT a device: the body runs over stand-in Frame / KeyFrame / MapPoint /
// Camera / extractor / store classes up to the device call, and this program defines orbfe_track_reference_stored and orbfe_get_capacity
// itself (the executable's definitions take the place of the library's): the stub records everything `in` points to and answers with a
// canned `out`.  Checked: the gathered arrays bit for bit (good, pos, frame_good, frame_pos, right_u, pose, bounds, level tables, camera,
// parameters, the FeatureVector CSR taken from mFeatVec), the replayed side effects (mBowVec / mFeatVec / mbBowComputed, addMatchInTrack
// and the slot per match with the last match winning, the nulling, addInlierInTrack, setPose; REJECT_MATCHES with the frame written and
// nothing else), and every fallback condition (the fallback's first statement is the frame's computeBow, which throws here).
// Run by tests/test_track_reference_host.py.  Exit code 0 and one line "GATHER_OK".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>

#include "../../orb_slam2_ros2_amd/host/orbfe_dropin.hpp"

// ---- the stub -------------------------------------------------------------------------------------------------------------------------
static const int kCap = 16;  // the fake context's capacity (features per frame)
static int g_cap = kCap;
struct Recorded {
  int calls = 0;
  orbfe_ctx* ctx = nullptr;
  int32_t slot = -1;
  const orbfe_vocab* vocab = nullptr;
  orbfe_kfstore* store = nullptr;
  orbfe_trackref_input in;
  std::vector<uint8_t> good, frameGood;
  std::vector<float> pos, framePos, sig2, invSig2;
  std::vector<double> rightU;
  orbfe_camera cam;
  std::vector<uint32_t> nodes, features;
  std::vector<int32_t> offsets;
  bool hadFrameGood = false, hadRightU = false, hadBowOut = false;
} g_rec;
struct Canned {
  int32_t verdict = 0, nMatches = 0, nEdges = 0, nInliers = 0;
  std::vector<orbfe_bow_match> matches;
  std::vector<uint8_t> inlier;
  float Tcw[12];
  std::vector<uint32_t> words, nodes, feats;
  std::vector<double> values;
  std::vector<int32_t> offsets;
} g_can;

extern "C" int32_t orbfe_get_capacity(const orbfe_ctx*) { return g_cap; }
extern "C" orbfe_status orbfe_track_reference_stored(orbfe_ctx* ctx, int32_t slot, const orbfe_vocab* vocab, orbfe_kfstore* store,
                                                     const orbfe_trackref_input* in, const orbfe_trackref_output* out) {
  Recorded& r = g_rec;
  ++r.calls, r.ctx = ctx, r.slot = slot, r.vocab = vocab, r.store = store, r.in = *in;
  const size_t n = (size_t)in->n, NF = (size_t)g_cap, nl = 8;
  r.good.assign(in->good, in->good + n), r.pos.assign(in->pos, in->pos + 3 * n);
  r.hadFrameGood = in->frame_good != nullptr, r.hadRightU = in->right_u != nullptr, r.hadBowOut = out->bow != nullptr;
  if (in->frame_good) r.frameGood.assign(in->frame_good, in->frame_good + NF), r.framePos.assign(in->frame_pos, in->frame_pos + 3 * NF);
  if (in->right_u) r.rightU.assign(in->right_u, in->right_u + NF);
  r.sig2.assign(in->level_sigma2, in->level_sigma2 + nl), r.invSig2.assign(in->level_inv_sigma2, in->level_inv_sigma2 + nl);
  r.cam = *in->cam;
  r.nodes.clear(), r.offsets.clear(), r.features.clear();
  if (in->node_offsets) {
    r.nodes.assign(in->nodes, in->nodes + in->n_nodes), r.offsets.assign(in->node_offsets, in->node_offsets + in->n_nodes + 1);
    r.features.assign(in->features, in->features + r.offsets.back());
  }
  const Canned& c = g_can;
  *out->verdict = c.verdict, *out->n_matches = c.nMatches, *out->n_edges = c.nEdges, *out->n_inliers = c.nInliers;
  for (size_t k = 0; k < c.matches.size(); ++k) out->matches[k] = c.matches[k];
  for (size_t f = 0; f < NF; ++f) out->inlier[f] = f < c.inlier.size() ? c.inlier[f] : 0;
  std::memcpy(out->Tcw, c.Tcw, sizeof c.Tcw);
  if (out->bow) {
    const orbfe_bow_out* b = out->bow;
    std::copy(c.words.begin(), c.words.end(), b->words), std::copy(c.values.begin(), c.values.end(), b->values);
    std::copy(c.nodes.begin(), c.nodes.end(), b->nodes), std::copy(c.offsets.begin(), c.offsets.end(), b->node_offsets);
    std::copy(c.feats.begin(), c.feats.end(), b->features);
    *b->n_words = (int32_t)c.words.size(), *b->n_nodes = (int32_t)c.nodes.size();
  }
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
  cv::Mat mPos;
  bool mbBad = false;
  int nInlier = 0, nMatchInTrack = 0;
  bool isBad() const { return mbBad; }
  bool isInMap() const { return true; }
  cv::Mat getPos() const { return mPos.clone(); }
  void addInlierInTrack() { ++nInlier; }
  void addMatchInTrack() { ++nMatchInTrack; }
};
struct FakeDevice {  // what the body asks of ORBExtractor::device()
  bool res = true;
  bool resident() const { return res; }
  orbfe_ctx* context() const { return (orbfe_ctx*)(uintptr_t)0x1000; }
  int slot() const { return 1; }
};
struct FakeExtractor {
  FakeDevice dev;
  const FakeDevice& device() const { return dev; }
};
struct Fallback : std::runtime_error {
  Fallback() : std::runtime_error("the bodies were taken") {}
};
struct VirtualFrame {
  static float getScaledFactor2(const int& l) { return std::pow(std::pow(1.2f, (float)l), 2); }
  static float getScaledFactorInv2(const int& l) { return std::pow(1.0f / std::pow(1.2f, (float)l), 2); }
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<double> mvFeatsRightU;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw, mtcw;
  float mfMaxU = 1241.f, mfMaxV = 376.f, mfMinU = 0.5f, mfMinV = 0.25f;
  std::vector<cv::Mat> mvLeftDescriptor;
  std::map<unsigned, double> mBowVec;
  std::map<unsigned, std::vector<unsigned>> mFeatVec;
  bool mbBowComputed = false;
  void computeBow() { throw Fallback(); }  // the first statement of Bodies::searchByBow: the fallback was taken
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
  const double& getRightU(const std::size_t& i) const { return mvFeatsRightU[i]; }
  void setPose(cv::Mat T) {
    mRcw = cv::Mat(3, 3, CV_32F), mtcw = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) mRcw.at<float>(r, c) = T.at<float>(r, c);
      mtcw.at<float>(r, 0) = T.at<float>(r, 3);
    }
  }
  cv::Point2f project2UV(const cv::Mat&, bool& isPositive) { return isPositive = true, cv::Point2f(0, 0); }
};
struct Frame : VirtualFrame {
  std::shared_ptr<FakeExtractor> mpExtractorLeft = std::make_shared<FakeExtractor>();
};
struct KeyFrame : VirtualFrame {
  std::size_t mnId = 0;
};
struct FakeStore {  // what the body asks of dropin::KeyframeStore<>
  bool present = true, hasBow = true;
  int n = 0;
  template <class K>
  bool info(const K&, orbfe_kfstore_info* out) const {
    *out = orbfe_kfstore_info();
    out->n = n, out->has_bow = hasBow ? 1 : 0;
    return present;
  }
  template <class K>
  uint64_t id(const K& k) const { return (uint64_t)k->mnId; }
  orbfe_kfstore* get() const { return (orbfe_kfstore*)(uintptr_t)0x2000; }
  int levels() const { return 8; }
};
struct FakeVocab {
  const orbfe_vocab* handle() const { return (const orbfe_vocab*)(uintptr_t)0x3000; }
};
}  // namespace ref

static int fails = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) fprintf(stderr, "line %d: %s\n", __LINE__, #cond), ++fails; \
  } while (0)

static cv::Mat pose4(const float* R, const float* t) {
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T.at<float>(r, c) = r == c ? 1.f : 0.f;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T.at<float>(r, c) = R[3 * r + c];
    T.at<float>(r, 3) = t[r];
  }
  return T;
}
static ref::MapPoint::SharedPtr point(float x, float y, float z, bool bad = false) {
  auto p = std::make_shared<ref::MapPoint>();
  p->mPos = cv::Mat(3, 1, CV_32F);
  p->mPos.at<float>(0) = x, p->mPos.at<float>(1) = y, p->mPos.at<float>(2) = z;
  p->mbBad = bad;
  return p;
}

struct World {
  std::shared_ptr<ref::Frame> F = std::make_shared<ref::Frame>();
  std::shared_ptr<ref::KeyFrame> K = std::make_shared<ref::KeyFrame>();
  ref::FakeStore store;
  std::shared_ptr<ref::FakeVocab> voc = std::make_shared<ref::FakeVocab>();
  float R0[9] = {0.99f, -0.01f, 0.02f, 0.0125f, 0.98f, -0.03f, -0.02f, 0.03f, 0.97f}, t0[3] = {0.25f, -0.5f, 0.125f};
  // twelve frame features (capacity 16), six keyframe features: 0 .. 4 good, 5 bad, none at 3 (null)
  World() {
    for (int f = 0; f < 12; ++f) {
      cv::KeyPoint kp;
      kp.pt.x = 100.f + 7.f * f, kp.pt.y = 50.f + 3.f * f, kp.octave = f % 4;
      F->mvFeatsLeft.push_back(kp), F->mvFeatsRightU.push_back(f % 3 == 0 ? -1.0 : 90.0 + 1.5 * f), F->mvpMapPoints.push_back(nullptr);
    }
    F->setPose(pose4(R0, t0));
    for (int i = 0; i < 6; ++i) K->mvpMapPoints.push_back(i == 3 ? nullptr : point(1.f + i, 2.f - i, 10.f + 0.5f * i, i == 5));
    K->mnId = 4711;
    store.n = 6;
  }
  bool run() { return orbfe::dropin::Bodies::trackReference<ref::Camera>(store, voc, F, K, 0.7f, true); }
};

static void canned(int verdict, std::vector<orbfe_bow_match> m, std::vector<int> inliers) {
  g_can = Canned();
  g_can.verdict = verdict, g_can.nMatches = (int32_t)m.size(), g_can.matches = m, g_can.inlier.assign(kCap, 0);
  for (int f : inliers) g_can.inlier[(size_t)f] = 1;
  g_can.nInliers = (int32_t)inliers.size(), g_can.nEdges = (int32_t)inliers.size() + 1;
  const float T[12] = {1.f, 0.f, 0.f, 0.f, 0.5f, -0.5f, 0.f, 0.5f, 0.5f, 3.f, 4.f, 5.f};
  std::memcpy(g_can.Tcw, T, sizeof T);
  g_can.words = {3, 9, 40}, g_can.values = {0.25, 0.5, 0.25}, g_can.nodes = {2, 7}, g_can.offsets = {0, 2, 5}, g_can.feats = {1, 4, 0, 2, 3};
}

int main() {
  // 1. ACCEPT, the transform in the call, a frame that arrives with points: feature 2 a good one, feature 6 a bad one, feature 9 a good one
  {
    World w;
    auto own2 = point(7.f, 8.f, 9.f), own6 = point(1.f, 1.f, 1.f, true), own9 = point(-2.f, 0.5f, 20.f);
    w.F->mvpMapPoints[2] = own2, w.F->mvpMapPoints[6] = own6, w.F->mvpMapPoints[9] = own9;
    // matches (query, train): feature 4 is named twice, the later one (train 1) keeps it; feature 7 takes train 4
    canned(ORBFE_TRACKREF_ACCEPT, {{4, 0, 11}, {7, 4, 3}, {4, 1, 20}}, {2, 4});
    g_rec = Recorded();
    const bool ok = w.run();
    const Recorded& r = g_rec;
    EXPECT(ok && r.calls == 1 && r.ctx == (orbfe_ctx*)(uintptr_t)0x1000 && r.slot == 1 && r.store == (orbfe_kfstore*)(uintptr_t)0x2000);
    EXPECT(r.vocab == (const orbfe_vocab*)(uintptr_t)0x3000 && r.hadBowOut && r.in.n_nodes == 0 && !r.in.nodes && !r.in.node_offsets && !r.in.features);
    EXPECT(r.in.kf_id == 4711 && r.in.n == 6);
    EXPECT((r.good == std::vector<uint8_t>{1, 1, 1, 0, 1, 0}));  // null and bad points are not good
    for (int i = 0; i < 6; ++i) {
      const bool g = i != 3 && i != 5;
      EXPECT(r.pos[3 * i] == (g ? 1.f + i : 0.f) && r.pos[3 * i + 1] == (g ? 2.f - i : 0.f) && r.pos[3 * i + 2] == (g ? 10.f + 0.5f * i : 0.f));
    }
    EXPECT(r.hadFrameGood && (int)r.frameGood.size() == kCap);
    for (int f = 0; f < kCap; ++f) {
      EXPECT(r.frameGood[f] == (f == 2 || f == 9 ? 1 : 0));  // the bad point of feature 6 is not flagged; nothing beyond the 12 features
      const float want[3] = {f == 2 ? 7.f : f == 9 ? -2.f : 0.f, f == 2 ? 8.f : f == 9 ? 0.5f : 0.f, f == 2 ? 9.f : f == 9 ? 20.f : 0.f};
      EXPECT(std::memcmp(&r.framePos[3 * f], want, 12) == 0);
    }
    EXPECT(r.hadRightU && (int)r.rightU.size() == kCap);
    for (int f = 0; f < kCap; ++f) EXPECT(r.rightU[f] == (f >= 12 || f % 3 == 0 ? -1.0 : 90.0 + 1.5 * f));
    EXPECT(std::memcmp(r.in.Rcw, w.R0, 36) == 0 && std::memcmp(r.in.tcw, w.t0, 12) == 0);
    EXPECT(r.in.bounds[0] == 0.5f && r.in.bounds[1] == 1241.f && r.in.bounds[2] == 0.25f && r.in.bounds[3] == 376.f);
    for (int l = 0; l < 8; ++l) EXPECT(r.sig2[l] == ref::VirtualFrame::getScaledFactor2(l) && r.invSig2[l] == ref::VirtualFrame::getScaledFactorInv2(l));
    EXPECT(r.cam.fx == 718.856f && r.cam.fy == 718.5f && r.cam.cx == 607.1928f && r.cam.cy == 185.2157f && r.cam.bf == 386.1448f && r.cam.k1 == 0.f);
    EXPECT(r.in.levelsup == 4 && r.in.ratio == 0.7f && r.in.dist_threshold == 50 && r.in.check_orientation == 1 && r.in.min_matches == 10 &&
           r.in.min_inliers == 10);
    // the replay: the frame's BoW, a counter per MATCH, the slots with the last match winning, the nulling, the inlier counters, the pose
    EXPECT(w.F->mbBowComputed && (w.F->mBowVec == std::map<unsigned, double>{{3, 0.25}, {9, 0.5}, {40, 0.25}}));
    EXPECT((w.F->mFeatVec == std::map<unsigned, std::vector<unsigned>>{{2, {1, 4}}, {7, {0, 2, 3}}}));
    auto& kp = w.K->mvpMapPoints;
    EXPECT(kp[0]->nMatchInTrack == 1 && kp[1]->nMatchInTrack == 1 && kp[4]->nMatchInTrack == 1 && kp[2]->nMatchInTrack == 0);
    for (int f = 0; f < 12; ++f) EXPECT(w.F->mvpMapPoints[f] == (f == 2 ? own2 : f == 4 ? kp[1] : nullptr));  // 7, 6 and 9: no inliers
    EXPECT(own2->nInlier == 1 && kp[1]->nInlier == 1 && kp[0]->nInlier == 0 && kp[4]->nInlier == 0 && own9->nInlier == 0 && own6->nInlier == 0);
    for (int r_ = 0; r_ < 3; ++r_) {
      for (int c = 0; c < 3; ++c) EXPECT(w.F->mRcw.at<float>(r_, c) == g_can.Tcw[3 * r_ + c]);
      EXPECT(w.F->mtcw.at<float>(r_, 0) == g_can.Tcw[9 + r_]);
    }
  }
  // 2. REJECT_MATCHES: the frame is written (slots and addMatchInTrack), nothing is nulled, no inlier counter, the pose stays; a frame
  //    that holds nothing sends no frame arrays
  {
    World w;
    canned(ORBFE_TRACKREF_REJECT_MATCHES, {{5, 2, 9}, {8, 0, 1}}, {});
    g_rec = Recorded();
    EXPECT(!w.run() && g_rec.calls == 1 && !g_rec.hadFrameGood && g_rec.in.frame_pos == nullptr);
    auto& kp = w.K->mvpMapPoints;
    for (int f = 0; f < 12; ++f) EXPECT(w.F->mvpMapPoints[f] == (f == 5 ? kp[2] : f == 8 ? kp[0] : nullptr));
    EXPECT(kp[2]->nMatchInTrack == 1 && kp[0]->nMatchInTrack == 1 && kp[2]->nInlier == 0 && kp[0]->nInlier == 0);
    EXPECT(w.F->mRcw.at<float>(0, 0) == w.R0[0] && w.F->mtcw.at<float>(2, 0) == w.t0[2] && w.F->mbBowComputed);
  }
  // 3. REJECT_INLIERS: everything of ACCEPT happens, the answer is false
  {
    World w;
    canned(ORBFE_TRACKREF_REJECT_INLIERS, {{5, 2, 9}}, {5});
    g_rec = Recorded();
    EXPECT(!w.run() && w.F->mvpMapPoints[5] == w.K->mvpMapPoints[2] && w.K->mvpMapPoints[2]->nInlier == 1 && w.F->mtcw.at<float>(0, 0) == 3.f);
  }
  // 4. a frame whose computeBow has run: its FeatureVector goes up as CSR, no vocabulary, no BoW comes back, the vectors stay
  {
    World w;
    w.F->mbBowComputed = true;
    w.F->mBowVec = {{1, 1.0}};
    w.F->mFeatVec = {{5, {3, 0, 7}}, {11, {2}}, {12, {9, 10}}};
    canned(ORBFE_TRACKREF_ACCEPT, {}, {});
    g_rec = Recorded();
    w.run();
    const Recorded& r = g_rec;
    EXPECT(r.calls == 1 && r.vocab == nullptr && !r.hadBowOut && r.in.n_nodes == 3);
    EXPECT((r.nodes == std::vector<uint32_t>{5, 11, 12}) && (r.offsets == std::vector<int32_t>{0, 3, 4, 6}) &&
           (r.features == std::vector<uint32_t>{3, 0, 7, 2, 9, 10}));
    EXPECT((w.F->mBowVec == std::map<unsigned, double>{{1, 1.0}}) && w.F->mFeatVec.size() == 3);
  }
  // 5. the fallbacks: not in the store, no FeatureVector there, a slot no longer resident, more than 2048 features, a distorting camera
  for (int c = 0; c < 5; ++c) {
    World w;
    if (c == 0) w.store.present = false;
    if (c == 1) w.store.hasBow = false;
    if (c == 2) w.F->mpExtractorLeft->dev.res = false;
    if (c == 3) g_cap = 2049;
    if (c == 4) {
      ref::Camera::mDistCoeff = cv::Mat(4, 1, CV_32F);
      for (int i = 0; i < 4; ++i) ref::Camera::mDistCoeff.at<float>(i) = i == 0 ? -0.25f : 0.f;
    }
    g_rec = Recorded();
    bool fell = false;
    try {
      w.run();
    } catch (const ref::Fallback&) {
      fell = true;
    }
    EXPECT(fell && g_rec.calls == 0);
    g_cap = kCap, ref::Camera::mDistCoeff = cv::Mat();
  }
  {  // (and 2048 features are still the one call)
    World w;
    canned(ORBFE_TRACKREF_REJECT_MATCHES, {}, {});
    g_rec = Recorded();
    g_cap = 2048;
    w.run();
    EXPECT(g_rec.calls == 1);
    g_cap = kCap;
  }
  printf("GATHER_%s\n", fails == 0 ? "OK" : "FAIL");
  return fails == 0 ? 0 : 1;
}
