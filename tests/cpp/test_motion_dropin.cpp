// orbfe::dropin::trackMotionModel (orbfe_motion_dropin.hpp: ONE device call, orbfe_track_motion_model_slots) against the reference's body of
// Tracking::trackMotionModel (src/Tracking.cc:384-405) on the existing bodies -- Frame::unProject, the two searchByProjection and
// OptimizePoseOnly of Bodies::trackMotionModel, the isInMap count -- on stand-in Frame / MapPoint / Camera classes with the reference's
// accessor names, over the stand-in opencv2/core.hpp of tests/cpp/stubs, linked to liborbfe_hip.so.
//   test_motion_dropin <lastL.raw> <lastR.raw> <curL.raw> <curR.raw> <w> <h>
// One small map per scenario, built twice: last frame A and frame A go through the bodies, their twins B through the one call.  The last
// frame's points sit at its stereo depth; the predicted pose is a few centimetres off.  Compared, all of it exactly (the same kernels run
// on the same lists): the verdict, the temporary points and their positions to the bit, the frame's final map points, the pose to the
// bit, both counters (addMatchInTrack, addInlierInTrack) of every point of the last frame.
// Exit code 0 and one line "MOTION_OK <accepted:matches:points held at the end:temporaries:device call, per scenario>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../orb_slam2_ros2_amd/host/orbfe_motion_dropin.hpp"

namespace ref {  // ---- stand-ins with the reference's accessor names ----------------------------------------------------------------
struct Camera {
  static inline float mfFx = 718.856f, mfFy = 718.856f, mfCx = 607.1928f, mfCy = 185.2157f, mfBf = 718.856f * 0.537166f, mfBl = 0.537166f;
  static inline cv::Mat mDistCoeff;
};

struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  static inline std::size_t mnNextId = 0;
  cv::Mat mPos;
  std::size_t mId = 0;
  bool mbBad = false, mbIsInMap = true;
  int nInlier = 0, nMatchInTrack = 0;
  static SharedPtr create(cv::Mat p3dW) {  // a temporary point: not in the map
    auto p = std::make_shared<MapPoint>();
    p->mPos = p3dW.clone(), p->mId = mnNextId++, p->mbIsInMap = false;
    return p;
  }
  std::size_t getID() const { return mId; }
  bool isBad() const { return mbBad; }
  bool isInMap() const { return mbIsInMap; }
  cv::Mat getPos() const { return mPos.clone(); }
  cv::Mat getViewDirection() const { return cv::Mat(); }
  cv::Mat getDesc() const { return cv::Mat(); }
  void getDistance(float& mx, float& mn) const { mx = 0.f, mn = 0.f; }
  void addInlierInTrack() { ++nInlier; }
  void addMatchInTrack() { ++nMatchInTrack; }
  template <class F>
  bool isInVision(F, float&, cv::Point2f&, float&) { return false; }  // (bFuse searches only)
};

struct Frame {
  typedef std::shared_ptr<Frame> SharedPtr;
  static inline std::vector<float> mvfScaledFactors;
  static float getScaledFactor(const int& l) { return mvfScaledFactors[l]; }
  static float getScaledFactor2(const int& l) { return std::pow(getScaledFactor(l), 2); }
  static float getScaledFactorInv(const int& l) { return 1.0f / getScaledFactor(l); }
  static float getScaledFactorInv2(const int& l) { return std::pow(getScaledFactorInv(l), 2); }
  std::vector<cv::KeyPoint> mvFeatsLeft, mvFeatsRight;
  std::vector<double> mvDepths, mvFeatsRightU;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw, mtcw, mRwc, mtwc;
  float mfMaxU = 0, mfMaxV = 0, mfMinU = 0, mfMinV = 0;
  std::vector<cv::Mat> mvLeftDescriptor, mRightDescriptor;
  cv::Mat mLeftIm, mRightIm;
  ORB_SLAM2_ROS2::ORBExtractor::SharedPtr mpExtractorLeft, mpExtractorRight;
  int mnN = 0;
  Frame(cv::Mat l, cv::Mat r) : mLeftIm(l), mRightIm(r) {
    mpExtractorLeft = std::make_shared<ORB_SLAM2_ROS2::ORBExtractor>(mLeftIm, 2000, 8, 1.2f, "", 20, 7);
    mpExtractorRight = std::make_shared<ORB_SLAM2_ROS2::ORBExtractor>(mRightIm, 2000, 8, 1.2f, "", 20, 7);
    mnN = orbfe::dropin::createStereo<Camera>(this);
    mvpMapPoints.resize(mvFeatsLeft.size(), nullptr);
  }
  MapPoint::SharedPtr getMapPoint(std::size_t idx) { return mvpMapPoints[idx]; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) { mvpMapPoints[idx] = p; }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
  const std::vector<cv::Mat>& getDescriptor() const { return mvLeftDescriptor; }
  std::vector<double> getDepth() const { return mvDepths; }
  std::vector<double> getRightU() const { return mvFeatsRightU; }
  const double& getRightU(const std::size_t& i) const { return mvFeatsRightU[i]; }
  void setPose(cv::Mat T) {  // VirtualFrame::setPose: mRwc = mRcw.t(), mtwc = -mRwc * mtcw in float
    mRcw = cv::Mat(3, 3, CV_32F), mtcw = cv::Mat(3, 1, CV_32F), mRwc = cv::Mat(3, 3, CV_32F), mtwc = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) mRcw.at<float>(r, c) = T.at<float>(r, c), mRwc.at<float>(c, r) = T.at<float>(r, c);
      mtcw.at<float>(r, 0) = T.at<float>(r, 3);
    }
    for (int r = 0; r < 3; ++r)
      mtwc.at<float>(r, 0) = -(mRwc.at<float>(r, 0) * mtcw.at<float>(0, 0) + mRwc.at<float>(r, 1) * mtcw.at<float>(1, 0) + mRwc.at<float>(r, 2) * mtcw.at<float>(2, 0));
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
  // Frame::unProject: a feature whose point is null or bad and whose depth is not negative gets MapPoint::create(mRwc * p3dC + mtwc),
  // p3dC = depth * ((pt - c) / f, 1) with the pixel terms in float and the depth a double
  int unProject(std::vector<MapPoint::SharedPtr>& mapPoints) {
    mapPoints.assign(mvFeatsLeft.size(), nullptr);
    int nCreated = 0;
    for (std::size_t idx = 0; idx < mvFeatsLeft.size(); ++idx) {
      auto pMp = mvpMapPoints[idx];
      if (pMp && !pMp->isBad()) {
        mapPoints[idx] = pMp;
        continue;
      }
      const double depth = mvDepths[idx];
      if (depth < 0) continue;
      const float x = (mvFeatsLeft[idx].pt.x - Camera::mfCx) / Camera::mfFx, y = (mvFeatsLeft[idx].pt.y - Camera::mfCy) / Camera::mfFy;
      const float pc[3] = {(float)(depth * x), (float)(depth * y), (float)depth};
      cv::Mat p3dW(3, 1, CV_32F);
      for (int r = 0; r < 3; ++r) {
        const float row = mRwc.at<float>(r, 0) * pc[0] + mRwc.at<float>(r, 1) * pc[1] + mRwc.at<float>(r, 2) * pc[2];
        p3dW.at<float>(r) = (float)((double)row + (double)mtwc.at<float>(r, 0));
      }
      mapPoints[idx] = MapPoint::create(p3dW);
      ++nCreated;
    }
    mvpMapPoints = mapPoints;
    return nCreated;
  }
};
}  // namespace ref

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
  if (argc < 7) return 2;
  const int w = atoi(argv[5]), h = atoi(argv[6]);
  std::vector<uint8_t> img[4];
  for (int k = 0; k < 4; ++k)
    if (!read_file(argv[1 + k], img[k]) || img[k].size() != (size_t)w * h) return 2;
  cv::Mat lastL(h, w, CV_8UC1, img[0].data()), lastR(h, w, CV_8UC1, img[1].data()), curL(h, w, CV_8UC1, img[2].data()), curR(h, w, CV_8UC1, img[3].data());
  std::vector<uint8_t> flat((size_t)w * h, 96);
  cv::Mat blankR(h, w, CV_8UC1, flat.data());
  int fails = 0;
  auto expect = [&](bool ok, int sc, const char* what) {
    if (!ok) fprintf(stderr, "scenario %d: %s\n", sc, what), ++fails;
  };
  orbfe::dropin::MapPointStore<> store;
  // every `every`-th feature of the last frame holds a point (the first `limit` of them), and whether the last frame has depth (without
  // it -- its right image is blank, on the host and on the device alike -- no temporary point is made); what the body should say; whether B's current frame arrives holding a point (the fallback)
  struct Scenario {
    int every, limit;
    bool depth, accept, holds;
  };
  const Scenario scenarios[] = {{2, 100000, true, true, false}, {3, 12, false, false, false}, {40, 6, true, false, false}, {2, 100000, true, true, true}};
  std::string report;
  for (int sc = 0; sc < 4; ++sc) {
    const Scenario& S = scenarios[sc];
    uint64_t sd = 4711 + (uint64_t)sc;
    auto rnd = [&]() {
      sd = sd * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(sd >> 11) / 9007199254740992.0;
    };
    // one side: the last frame with its points, the current frame with the predicted pose
    struct Side {
      ref::Frame::SharedPtr last, cur;
      std::vector<ref::MapPoint::SharedPtr> pts, temps;
    };
    auto make = [&](uint64_t seed) {
      sd = seed;
      Side s;
      s.last = std::make_shared<ref::Frame>(lastL, S.depth ? lastR : blankR);  // (a blank right image: no stereo match, no depth anywhere)
      ref::Frame::mvfScaledFactors = ORB_SLAM2_ROS2::ORBExtractor::getScaledFactors();
      s.cur = std::make_shared<ref::Frame>(curL, curR);
      for (auto f : {s.last, s.cur}) f->mfMinU = 0, f->mfMinV = 0, f->mfMaxU = (float)w, f->mfMaxV = (float)h;
      s.last->setPose(pose4(0.f, 0.f, 0.1f));
      s.cur->setPose(pose4(0.03f, -0.02f, 0.14f));
      const size_t n = s.last->mvFeatsLeft.size();
      int made = 0;
      for (size_t i = 0; i < n; ++i) {
        if (i % (size_t)S.every != 0 || made >= S.limit) continue;
        const cv::KeyPoint kp = s.last->mvFeatsLeft[i];
        const double d = s.last->mvDepths[i] > 0 ? s.last->mvDepths[i] : 6.0 + 20.0 * rnd();
        const double off = made % 29 == 3 ? 3.0 : 0.0;  // some points metres off
        auto p = std::make_shared<ref::MapPoint>();
        p->mPos = cv::Mat(3, 1, CV_32F);
        p->mPos.at<float>(0) = (float)((kp.pt.x - ref::Camera::mfCx) / ref::Camera::mfFx * d + off);
        p->mPos.at<float>(1) = (float)((kp.pt.y - ref::Camera::mfCy) / ref::Camera::mfFy * d - off);
        p->mPos.at<float>(2) = (float)(d + off - 0.1);
        p->mId = 100000 * (size_t)(sc + 1) + i;
        p->mbBad = made % 41 == 7, p->mbIsInMap = made % 5 != 4;
        s.last->mvpMapPoints[i] = p;
        ++made;
      }
      s.pts = s.last->mvpMapPoints;
      return s;
    };
    // A: the reference's body on the existing bodies (its frame is resident while it runs)
    Side A = make(4711 + (uint64_t)sc);
    {
      std::vector<ref::MapPoint::SharedPtr> mapPoints;
      A.last->unProject(mapPoints);
      std::swap(mapPoints, A.temps);
    }
    int nGood = 0;
    const int nMatches = orbfe::dropin::Bodies::trackMotionModel<ref::Camera>(A.cur, A.last, 0.9f, nGood);
    bool okA = false;
    if (nMatches >= 20) {
      int inLiers = 0;
      for (const auto& p : A.cur->getMapPoints()) inLiers += (p && p->isInMap()) ? 1 : 0;
      okA = inLiers >= 10;
    }
    // B: one call
    Side B = make(4711 + (uint64_t)sc);
    if (S.holds) B.cur->mvpMapPoints[5] = B.pts[0];
    const bool okB = orbfe::dropin::trackMotionModel<ref::Camera>(B.cur, B.last, store, B.temps);
    if (S.holds) {  // the bodies were taken; A did not start with that point, so only the verdicts are compared
      expect(okB == S.accept, sc, "the fallback's verdict");
      report += okB ? " 1:-:-:-:0" : " 0:-:-:-:0";
      continue;
    }
    const size_t n = A.last->mvFeatsLeft.size(), nc = A.cur->mvFeatsLeft.size();
    expect(okA == okB, sc, "the verdicts differ");
    expect(okA == S.accept, sc, "the scenario did not go the way it was built to");
    // the temporary points: in the same places, at the same positions to the bit, in the last frame and in the caller's vector
    int temp_diff = 0, temps = 0;
    expect(B.temps.size() == n && A.temps.size() == n && B.last->mvpMapPoints == B.temps, sc, "processLastFrame's vectors");
    for (size_t i = 0; i < n && i < B.temps.size(); ++i) {
      const auto a = A.temps[i], b = B.temps[i];
      if ((a == nullptr) != (b == nullptr)) {
        ++temp_diff;
        continue;
      }
      if (!a) continue;
      const bool ta = a != A.pts[i], tb = b != B.pts[i];
      temps += ta;
      temp_diff += ta != tb || a->isInMap() != b->isInMap();
      for (int k = 0; k < 3; ++k) temp_diff += std::memcmp(&a->mPos.at<float>(k), &b->mPos.at<float>(k), 4) != 0;
    }
    expect(temp_diff == 0, sc, "the temporary points differ");
    expect(S.depth ? temps > 50 : temps == 0, sc, "temporaries where the last frame has depth, and only there");
    auto index_of = [&](const Side& s, const ref::MapPoint::SharedPtr& p) {
      return (long)(std::find(s.last->mvpMapPoints.begin(), s.last->mvpMapPoints.end(), p) - s.last->mvpMapPoints.begin());
    };
    int assign_diff = 0, held = 0;
    for (size_t f = 0; f < nc; ++f) {
      auto a = A.cur->mvpMapPoints[f], b = B.cur->mvpMapPoints[f];
      held += a != nullptr;
      if ((a == nullptr) != (b == nullptr)) {
        ++assign_diff;
        continue;
      }
      if (a) assign_diff += index_of(A, a) != index_of(B, b) || (size_t)index_of(A, a) >= n;
    }
    expect(assign_diff == 0, sc, "the frames' map points differ");  // (the same kernels on the same lists: nothing may differ)
    int pose_diff = 0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose_diff += std::memcmp(&A.cur->mRcw.at<float>(r, c), &B.cur->mRcw.at<float>(r, c), 4) != 0;
      pose_diff += std::memcmp(&A.cur->mtcw.at<float>(r, 0), &B.cur->mtcw.at<float>(r, 0), 4) != 0;
    }
    expect(pose_diff == 0, sc, "the poses differ in a bit");
    int match_diff = 0, inlier_diff = 0, visits = 0;
    for (size_t i = 0; i < n; ++i) {
      const auto a = A.last->mvpMapPoints[i], b = B.last->mvpMapPoints[i];
      if (!a || !b) continue;
      match_diff += a->nMatchInTrack != b->nMatchInTrack;
      inlier_diff += std::abs(a->nInlier - b->nInlier);
      visits += a->nMatchInTrack;
    }
    expect(match_diff == 0, sc, "the addMatchInTrack counts differ");
    expect(inlier_diff == 0, sc, "the addInlierInTrack counts differ");
    expect(visits >= nMatches, sc, "one addMatchInTrack per match at least");
    if (sc == 0) expect(nMatches > 200 && held > 100, sc, "a thousand points should track");
    if (sc == 1) expect(nMatches < 20 && held > 0 && held <= nMatches, sc, "twelve points end at the first test, with the frame written");
    if (sc == 2) expect(nMatches >= 20 && held > 20, sc, "temporaries track, six map points are too few to be accepted");
    char buf[64];
    snprintf(buf, sizeof buf, " %d:%d:%d:%d:1", okB ? 1 : 0, nMatches, held, temps);
    report += buf;
  }
  printf("MOTION_%s%s\n", fails == 0 ? "OK" : "FAIL", report.c_str());
  return fails == 0 ? 0 : 1;
}
