// orbfe::dropin::trackReference (orbfe_reloc_dropin.hpp: ONE device call, orbfe_track_reference_stored) against the reference's body of
// Tracking::trackReference (src/Tracking.cc:360-371) on the existing bodies -- searchByBow(frame, keyframe) with 0.7 / true, the 10-match
// test, OptimizePoseOnly, the 10-inlier test -- on stand-in Frame / KeyFrame / MapPoint / Camera classes with the reference's accessor
// names, over the stand-in opencv2/core.hpp of tests/cpp/stubs and host/compat's DBoW3::Vocabulary, linked to liborbfe_hip.so.
//   test_trackref_dropin <L.raw> <R.raw> <w> <h> <vocabulary.txt>
// One small map per scenario, built twice: frame A and keyframe A go through the bodies, their twins B through trackReference.  The
// keyframe is a jittered, bit-flipped subset of the frame's features with map points at the stereo depth; the frame's pose is a few
// centimetres off.  Compared, all of it exactly (the same kernels run on the same lists): the verdict, the frame's final map points,
// the pose to the bit, both counters (addMatchInTrack, addInlierInTrack) of every map point, and the frame's BowVector / FeatureVector
// / mbBowComputed.
// Exit code 0 and one line "TRACKREF_OK <accepted:matches:points held at the end:store used, per scenario>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>

#include "../../orb_slam2_ros2_amd/host/compat/DBoW3/DBoW3.h"
#include "../../orb_slam2_ros2_amd/host/orbfe_reloc_dropin.hpp"

namespace ref {  // ---- stand-ins with the reference's accessor names ----------------------------------------------------------------
struct Camera {
  static inline float mfFx = 718.856f, mfFy = 718.856f, mfCx = 607.1928f, mfCy = 185.2157f, mfBf = 718.856f * 0.537166f, mfBl = 0.537166f;
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

struct VirtualFrame {
  static inline std::vector<float> mvfScaledFactors;
  static inline std::shared_ptr<DBoW3::Vocabulary> mpVoc;
  static float getScaledFactor(const int& l) { return mvfScaledFactors[l]; }
  static float getScaledFactor2(const int& l) { return std::pow(getScaledFactor(l), 2); }
  static float getScaledFactorInv(const int& l) { return 1.0f / getScaledFactor(l); }
  static float getScaledFactorInv2(const int& l) { return std::pow(getScaledFactorInv(l), 2); }
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<double> mvDepths, mvFeatsRightU;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw, mtcw;
  float mfMaxU = 0, mfMaxV = 0, mfMinU = 0, mfMinV = 0;
  std::vector<cv::Mat> mvLeftDescriptor;
  DBoW3::BowVector mBowVec;
  DBoW3::FeatureVector mFeatVec;
  bool mbBowComputed = false;
  int nTransforms = 0;
  void computeBow() {  // include/ORB_SLAM2/Frame.h:224-231
    if (mbBowComputed) return;
    mpVoc->transform(mvLeftDescriptor, mBowVec, mFeatVec, 4);
    mbBowComputed = true;
    ++nTransforms;
  }
  MapPoint::SharedPtr getMapPoint(std::size_t idx) { return mvpMapPoints[idx]; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) { mvpMapPoints[idx] = p; }
  void setMapPointsNull() { std::fill(mvpMapPoints.begin(), mvpMapPoints.end(), nullptr); }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
  const std::vector<cv::Mat>& getDescriptor() const { return mvLeftDescriptor; }
  std::vector<double> getDepth() const { return mvDepths; }
  std::vector<double> getRightU() const { return mvFeatsRightU; }
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

struct Frame : VirtualFrame {
  typedef std::shared_ptr<Frame> SharedPtr;
  cv::Mat mLeftIm, mRightIm;
  ORB_SLAM2_ROS2::ORBExtractor::SharedPtr mpExtractorLeft, mpExtractorRight;
  std::vector<cv::KeyPoint> mvFeatsRight;
  std::vector<cv::Mat> mRightDescriptor;
  int mnN = 0;
  Frame(cv::Mat l, cv::Mat r) : mLeftIm(l), mRightIm(r) {
    mpExtractorLeft = std::make_shared<ORB_SLAM2_ROS2::ORBExtractor>(mLeftIm, 2000, 8, 1.2f, "", 20, 7);
    mpExtractorRight = std::make_shared<ORB_SLAM2_ROS2::ORBExtractor>(mRightIm, 2000, 8, 1.2f, "", 20, 7);
    mnN = orbfe::dropin::createStereo<Camera>(this);
    mvpMapPoints.resize(mvFeatsLeft.size(), nullptr);
  }
};

struct KeyFrame : VirtualFrame {
  typedef std::shared_ptr<KeyFrame> SharedPtr;
  std::size_t mnId = 0;
  bool mbBad = false;
  std::size_t getID() const { return mnId; }
  bool isBad() const { return mbBad; }
};
}  // namespace ref

struct Access {
  static uint64_t id(const ref::KeyFrame::SharedPtr& k) { return (uint64_t)k->mnId; }
  static void bounds(const ref::KeyFrame::SharedPtr& k, float b[4]) { orbfe::dropin::Bodies::bounds(k, b); }
};

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize((size_t)n);
  const bool ok = fread(out.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

static cv::Mat pose4(float tx, float ty, float tz) {
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T.at<float>(r, c) = r == c ? 1.f : 0.f;
  T.at<float>(0, 3) = tx, T.at<float>(1, 3) = ty, T.at<float>(2, 3) = tz;
  return T;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const int w = atoi(argv[3]), h = atoi(argv[4]);
  std::vector<uint8_t> L, R;
  if (!read_file(argv[1], L) || !read_file(argv[2], R) || L.size() != (size_t)w * h || R.size() != L.size()) return 2;
  cv::Mat ml(h, w, CV_8UC1, L.data()), mr(h, w, CV_8UC1, R.data());
  ref::VirtualFrame::mpVoc = std::make_shared<DBoW3::Vocabulary>(std::string(argv[5]));
  int fails = 0;
  auto expect = [&](bool ok, int sc, const char* what) {
    if (!ok) fprintf(stderr, "scenario %d: %s\n", sc, what), ++fails;
  };
  orbfe::dropin::KeyframeStore<Access> store(w, h, 8);
  // good keyframe points, points the frame arrives with (the last of them metres off), the frame's BoW computed before the call, the
  // keyframe in the store, and what the body should say
  struct Scenario {
    int points, own;
    bool bowBefore, stored, accept;
  };
  const Scenario scenarios[] = {{200, 0, false, true, true}, {150, 80, true, true, true}, {6, 0, false, true, false}, {120, 0, false, false, true}};
  std::string report;
  for (int sc = 0; sc < 4; ++sc) {
    const Scenario& S = scenarios[sc];
    auto make = [&]() {
      auto f = std::make_shared<ref::Frame>(ml, mr);
      f->mfMinU = 0, f->mfMinV = 0, f->mfMaxU = (float)w, f->mfMaxV = (float)h;
      f->setPose(pose4(0.04f, -0.02f, 0.05f));
      return f;
    };
    auto FA = make();
    ref::VirtualFrame::mvfScaledFactors = ORB_SLAM2_ROS2::ORBExtractor::getScaledFactors();
    auto FB = make();  // (B's frame comes last and stays resident in its extraction slot)
    ref::Frame::SharedPtr F[2] = {FA, FB};
    const size_t n = FA->mvFeatsLeft.size();
    if (FB->mvFeatsLeft.size() != n) return 1;
    uint64_t sd = 991 + (uint64_t)sc;
    auto rnd = [&]() {
      sd = sd * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(sd >> 11) / 9007199254740992.0;
    };
    auto point = [&](const cv::KeyPoint& kp, double d, double off) {
      auto p = std::make_shared<ref::MapPoint>();
      p->mPos = cv::Mat(3, 1, CV_32F);
      p->mPos.at<float>(0) = (float)((kp.pt.x - ref::Camera::mfCx) / ref::Camera::mfFx * d + off);
      p->mPos.at<float>(1) = (float)((kp.pt.y - ref::Camera::mfCy) / ref::Camera::mfFy * d - off);
      p->mPos.at<float>(2) = (float)(d + off);
      return p;
    };
    // the keyframe: every third feature of the frame, a pixel or two off, six bits off; the first `points` of them hold a point
    ref::KeyFrame::SharedPtr K[2] = {std::make_shared<ref::KeyFrame>(), std::make_shared<ref::KeyFrame>()};
    int made = 0;
    for (size_t i = 0; i < n; i += 3) {
      const cv::KeyPoint kp = FA->mvFeatsLeft[i];
      const float dx = (float)((rnd() - 0.5) * 3.0), dy = (float)((rnd() - 0.5) * 3.0);
      int bits[6];
      for (int& b : bits) b = (int)(rnd() * 256) % 256;
      const double d = FA->mvDepths[i] > 0 ? FA->mvDepths[i] : 6.0 + 20.0 * rnd();
      const bool has = made < S.points;
      for (auto& kf : K) {
        cv::KeyPoint q = kp;
        q.pt.x = kp.pt.x + dx, q.pt.y = kp.pt.y + dy;
        cv::Mat ds = FA->mvLeftDescriptor[i].clone();
        for (int b : bits) ds.data[b / 8] ^= (uint8_t)(1u << (b % 8));
        ref::MapPoint::SharedPtr p;
        if (has) {
          p = point(kp, d, 0.0);
          p->mbBad = made % 41 == 7;
        }
        kf->mvFeatsLeft.push_back(q), kf->mvLeftDescriptor.push_back(ds), kf->mvpMapPoints.push_back(p);
        kf->mvDepths.push_back(-1.0), kf->mvFeatsRightU.push_back(-1.0);
      }
      ++made;
    }
    // what the frame arrives with: points of its own on features the keyframe does not cover, the last eight metres off, one bad
    std::vector<ref::MapPoint::SharedPtr> ownPts[2];
    for (int k = 0, f = 1; k < S.own && (size_t)f < n; ++k, f += 3) {
      const cv::KeyPoint kp = FA->mvFeatsLeft[(size_t)f];
      const double d = FA->mvDepths[(size_t)f] > 0 ? FA->mvDepths[(size_t)f] : 8.0 + 10.0 * rnd();
      for (int c = 0; c < 2; ++c) {
        auto p = point(kp, d, k >= S.own - 8 ? 3.0 : 0.0);
        p->mbBad = k == 5;
        F[c]->mvpMapPoints[(size_t)f] = p;
        ownPts[c].push_back(p);
      }
    }
    for (int k = 0; k < 2; ++k) {
      K[k]->mnId = (std::size_t)(10 * sc + 1);
      K[k]->mfMinU = 0, K[k]->mfMinV = 0, K[k]->mfMaxU = (float)w, K[k]->mfMaxV = (float)h;
      K[k]->setPose(pose4(0.f, 0.f, 0.1f));
    }
    if (S.bowBefore) FA->computeBow(), FB->computeBow();
    // A: the reference's body on the existing bodies
    std::vector<cv::DMatch> matchesA;
    const int nMatches = orbfe::dropin::searchByBow(FA, K[0], matchesA, false, false, 0.7f, true);
    const bool okA = nMatches >= 10 && orbfe::dropin::OptimizePoseOnly<ref::Camera>(FA) >= 10;
    // B: one call
    if (S.stored) store.ensureBow(K[1]);
    const int before = FB->nTransforms;
    const bool okB = orbfe::dropin::trackReference<ref::Camera>(store, ref::VirtualFrame::mpVoc, FB, K[1]);
    orbfe_kfstore_info info;
    expect(store.info(K[1], &info) == S.stored, sc, "the fallback must not insert the keyframe");
    expect(S.stored ? FB->nTransforms == before : FB->nTransforms == before + 1, sc, "the frame's transform ran in the wrong place");
    expect(okA == okB, sc, "the verdicts differ");
    expect(okA == S.accept, sc, "the scenario did not go the way it was built to");
    expect(FB->mbBowComputed && FA->mBowVec == FB->mBowVec && FA->mFeatVec == FB->mFeatVec && !FB->mFeatVec.empty(), sc, "the frames' BoW differ");
    int assign_diff = 0, held = 0;
    auto index_of = [&](int c, const ref::MapPoint::SharedPtr& p) {
      const auto a = std::find(K[c]->mvpMapPoints.begin(), K[c]->mvpMapPoints.end(), p) - K[c]->mvpMapPoints.begin();
      if ((size_t)a < K[c]->mvpMapPoints.size()) return (long)a;
      return -1 - (long)(std::find(ownPts[c].begin(), ownPts[c].end(), p) - ownPts[c].begin());
    };
    for (size_t f = 0; f < n; ++f) {
      auto a = FA->mvpMapPoints[f], b = FB->mvpMapPoints[f];
      held += a != nullptr;
      if ((a == nullptr) != (b == nullptr)) {
        ++assign_diff;
        continue;
      }
      if (a) assign_diff += index_of(0, a) != index_of(1, b);
    }
    expect(assign_diff == 0, sc, "the frames' map points differ");  // (the same kernels on the same lists: nothing may differ)
    int pose_diff = 0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose_diff += std::memcmp(&FA->mRcw.at<float>(r, c), &FB->mRcw.at<float>(r, c), 4) != 0;
      pose_diff += std::memcmp(&FA->mtcw.at<float>(r, 0), &FB->mtcw.at<float>(r, 0), 4) != 0;
    }
    expect(pose_diff == 0, sc, "the poses differ in a bit");
    int match_diff = 0, inlier_diff = 0, visits = 0;
    auto counters = [&](const ref::MapPoint::SharedPtr& a, const ref::MapPoint::SharedPtr& b) {
      if (!a) return;
      match_diff += a->nMatchInTrack != b->nMatchInTrack;
      inlier_diff += std::abs(a->nInlier - b->nInlier);
      visits += a->nMatchInTrack;
    };
    for (size_t i = 0; i < K[0]->mvpMapPoints.size(); ++i) counters(K[0]->mvpMapPoints[i], K[1]->mvpMapPoints[i]);
    for (size_t i = 0; i < ownPts[0].size(); ++i) counters(ownPts[0][i], ownPts[1][i]);
    expect(match_diff == 0, sc, "the addMatchInTrack counts differ");
    expect(inlier_diff == 0, sc, "the addInlierInTrack counts differ");
    expect(visits == nMatches, sc, "one addMatchInTrack per match");
    if (sc == 1) expect(held > 100 && FB->mvpMapPoints[1] != nullptr && FB->mvpMapPoints[1] == ownPts[1][0], sc, "the frame's own points should have stayed");
    if (sc == 2) expect(nMatches < 10 && held <= nMatches && (nMatches == 0 || held > 0), sc, "six points end at the first test, with the frame written");
    char buf[64];
    snprintf(buf, sizeof buf, " %d:%d:%d:%d", okB ? 1 : 0, nMatches, held, S.stored ? 1 : 0);
    report += buf;
    if (S.stored) store.erase(K[1]);
  }
  printf("TRACKREF_%s%s\n", fails == 0 ? "OK" : "FAIL", report.c_str());
  return fails == 0 ? 0 : 1;
}
