// orbfe::dropin::relocRefine (orbfe_reloc_dropin.hpp: ONE device call, orbfe_reloc_refine_stored) against the chain of the existing
// bodies in Tracking.cc's order (src/Tracking.cc:565-584, :612-629): setCurrFrameAttrib, OptimizePoseOnly, searchByProjection(frame,
// keyframe, 10), OptimizePoseOnly, searchByProjection(frame, keyframe, 3), on stand-in Frame / KeyFrame / MapPoint / Camera classes with
// the reference's accessor names, over the stand-in opencv2/core.hpp of tests/cpp/stubs, linked to liborbfe_hip.so.
//   test_reloc_refine_dropin <L.raw> <R.raw> <w> <h>
// One small map per scenario, built twice: frame A and keyframe A go through the chain, their twins B through relocRefine.  The keyframe
// is a jittered, bit-flipped subset of the frame's features with map points at the stereo depth; the PnP pose is a few centimetres off.
// Compared: the verdict, the frame's final map points, the pose, and both counters (addMatchInTrack, addInlierInTrack) of every map point.
// Exit code 0 and one line "RELOC_OK <verdict and inliers per scenario>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>

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
  template <class FramePtr>
  bool isInVision(FramePtr, float&, cv::Point2f&, float&) { return false; }  // (bFuse only)
};

struct VirtualFrame {
  static inline std::vector<float> mvfScaledFactors;
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
  MapPoint::SharedPtr getMapPoint(std::size_t idx) { return mvpMapPoints[idx]; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) { mvpMapPoints[idx] = p; }
  void setMapPointsNull() { std::fill(mvpMapPoints.begin(), mvpMapPoints.end(), nullptr); }
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

struct RelocBowParam {  // include/ORB_SLAM2/Tracking.h:25-34, the two members setCurrFrameAttrib reads
  std::vector<std::vector<cv::DMatch>> mvAllMatches;
  std::vector<std::map<std::size_t, std::size_t>> mvPnPId2MatchID;
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
  if (argc < 5) return 2;
  const int w = atoi(argv[3]), h = atoi(argv[4]);
  std::vector<uint8_t> L, R;
  if (!read_file(argv[1], L) || !read_file(argv[2], R) || L.size() != (size_t)w * h || R.size() != L.size()) return 2;
  cv::Mat ml(h, w, CV_8UC1, L.data()), mr(h, w, CV_8UC1, R.data());
  int fails = 0;
  auto expect = [&](bool ok, int sc, const char* what) {
    if (!ok) fprintf(stderr, "scenario %d: %s\n", sc, what), ++fails;
  };
  orbfe::dropin::KeyframeStore<Access> store(w, h, 8);
  // seeds (PnP inliers), further good keyframe points the searches can find, and what the chain should say
  struct Scenario {
    int seeds, others;
    bool accept;
  };
  const Scenario scenarios[] = {{100, 50, true}, {30, 400, true}, {5, 100, false}, {30, 6, false}};
  std::string report;
  for (int sc = 0; sc < 4; ++sc) {
    auto make = [&]() {
      auto f = std::make_shared<ref::Frame>(ml, mr);
      f->mfMinU = 0, f->mfMinV = 0, f->mfMaxU = (float)w, f->mfMaxV = (float)h;
      return f;
    };
    auto FA = make();
    ref::VirtualFrame::mvfScaledFactors = ORB_SLAM2_ROS2::ORBExtractor::getScaledFactors();
    auto FB = make();  // (B's frame comes last and stays resident in its extraction slot)
    const size_t n = FA->mvFeatsLeft.size();
    if (FB->mvFeatsLeft.size() != n) return 1;
    uint64_t sd = 777 + (uint64_t)sc;
    auto rnd = [&]() {
      sd = sd * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(sd >> 11) / 9007199254740992.0;
    };
    // the keyframe: every third feature of the frame, a pixel or two off, six bits off; the first `seeds + others` of them hold a point
    ref::KeyFrame::SharedPtr K[2] = {std::make_shared<ref::KeyFrame>(), std::make_shared<ref::KeyFrame>()};
    ref::RelocBowParam rbp;
    rbp.mvAllMatches.resize(1), rbp.mvPnPId2MatchID.resize(1);
    std::vector<std::size_t> vInliers;
    const Scenario& S = scenarios[sc];
    int made = 0;
    for (size_t i = 0; i < n; i += 3) {
      const cv::KeyPoint kp = FA->mvFeatsLeft[i];
      const float dx = (float)((rnd() - 0.5) * 3.0), dy = (float)((rnd() - 0.5) * 3.0);
      int bits[6];
      for (int& b : bits) b = (int)(rnd() * 256) % 256;
      const double d = FA->mvDepths[i] > 0 ? FA->mvDepths[i] : 6.0 + 20.0 * rnd();
      const bool has = made < S.seeds + S.others;
      for (auto& kf : K) {
        cv::KeyPoint q = kp;
        q.pt.x = kp.pt.x + dx, q.pt.y = kp.pt.y + dy;
        cv::Mat ds = FA->mvLeftDescriptor[i].clone();
        for (int b : bits) ds.data[b / 8] ^= (uint8_t)(1u << (b % 8));
        ref::MapPoint::SharedPtr p;
        if (has) {
          p = std::make_shared<ref::MapPoint>();
          p->mPos = cv::Mat(3, 1, CV_32F);
          p->mPos.at<float>(0) = (float)((kp.pt.x - ref::Camera::mfCx) / ref::Camera::mfFx * d);
          p->mPos.at<float>(1) = (float)((kp.pt.y - ref::Camera::mfCy) / ref::Camera::mfFy * d);
          p->mPos.at<float>(2) = (float)d;
          p->mbBad = made % 41 == 7;
        }
        kf->mvFeatsLeft.push_back(q), kf->mvLeftDescriptor.push_back(ds), kf->mvpMapPoints.push_back(p);
      }
      if (made < S.seeds) {  // a BoW match (frame feature i, keyframe feature `made`) that PnP kept
        const std::size_t matchID = rbp.mvAllMatches[0].size();
        rbp.mvAllMatches[0].emplace_back((int)i, made, 0.f);
        rbp.mvPnPId2MatchID[0][vInliers.size()] = matchID;
        vInliers.push_back(vInliers.size());
      }
      ++made;
    }
    for (int k = 0; k < 2; ++k) {
      K[k]->mnId = (std::size_t)(10 * sc + 1);
      K[k]->mfMinU = 0, K[k]->mfMinV = 0, K[k]->mfMaxU = (float)w, K[k]->mfMaxV = (float)h;
      K[k]->setPose(pose4(0.f, 0.f, sc == 1 ? 1.0f : 0.1f));  // (scenario 1 searches forward: octaves [o, 7])
    }
    const cv::Mat T0 = pose4(0.04f, -0.02f, 0.05f);
    cv::Mat Rcw(3, 3, CV_32F), tcw(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Rcw.at<float>(r, c) = T0.at<float>(r, c);
      tcw.at<float>(r, 0) = T0.at<float>(r, 3);
    }
    // A: the bodies in Tracking.cc's order
    orbfe::dropin::Bodies::setCurrFrameAttrib<ref::Camera>(FA, K[0], rbp, 0, vInliers, Rcw, tcw);
    bool okA = false;
    int nInliers = orbfe::dropin::OptimizePoseOnly<ref::Camera>(FA);
    const int firstInliers = nInliers;
    if (nInliers >= 50)
      okA = true;
    else if (nInliers >= 10) {
      std::vector<cv::DMatch> matches2;
      int nAddition = orbfe::dropin::searchByProjection<ref::Camera>(FA, K[0], matches2, 10.f, false, 0.9f);
      if (nAddition + nInliers >= 50) {
        nInliers = orbfe::dropin::OptimizePoseOnly<ref::Camera>(FA);
        okA = true;
        if (nInliers < 50) {
          nAddition = orbfe::dropin::searchByProjection<ref::Camera>(FA, K[0], matches2, 3.f, false, 0.9f);
          okA = nAddition + nInliers >= 50;
        }
      }
    }
    // B: one call
    const bool okB = orbfe::dropin::relocRefine<ref::Camera>(store, FB, K[1], rbp, 0, vInliers, Rcw, tcw);
    expect(okA == okB, sc, "the verdicts differ");
    expect(okA == S.accept, sc, "the scenario did not go the way it was built to");
    int assign_diff = 0, held = 0;
    for (size_t f = 0; f < n; ++f) {
      auto a = FA->mvpMapPoints[f], b = FB->mvpMapPoints[f];
      held += a != nullptr;
      if ((a == nullptr) != (b == nullptr)) {
        ++assign_diff;
        continue;
      }
      if (!a) continue;
      const auto ia = std::find(K[0]->mvpMapPoints.begin(), K[0]->mvpMapPoints.end(), a) - K[0]->mvpMapPoints.begin();
      const auto ib = std::find(K[1]->mvpMapPoints.begin(), K[1]->mvpMapPoints.end(), b) - K[1]->mvpMapPoints.begin();
      assign_diff += ia != ib;
    }
    expect(assign_diff <= 1, sc, "the frames' map points differ");  // (an edge exactly on a threshold may flip)
    double pose_diff = 0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose_diff = std::max(pose_diff, (double)std::fabs(FA->mRcw.at<float>(r, c) - FB->mRcw.at<float>(r, c)));
      pose_diff = std::max(pose_diff, (double)std::fabs(FA->mtcw.at<float>(r, 0) - FB->mtcw.at<float>(r, 0)));
    }
    expect(pose_diff < 1e-5, sc, "the poses differ");
    int match_diff = 0, inlier_diff = 0, visits = 0;
    for (size_t i = 0; i < K[0]->mvpMapPoints.size(); ++i) {
      const auto a = K[0]->mvpMapPoints[i], b = K[1]->mvpMapPoints[i];
      if (!a) continue;
      match_diff += a->nMatchInTrack != b->nMatchInTrack;
      inlier_diff += std::abs(a->nInlier - b->nInlier);
      visits += a->nMatchInTrack;
    }
    expect(match_diff <= 2 * assign_diff, sc, "the addMatchInTrack counts differ");
    expect(inlier_diff <= 2 * assign_diff, sc, "the addInlierInTrack counts differ");
    if (sc == 1) expect(visits > 300 && held > 200, sc, "the search should have added hundreds of points");
    if (sc == 2) expect(firstInliers < 10 && visits == 0, sc, "five seeds end at the first test");
    char buf[64];
    snprintf(buf, sizeof buf, " %d:%d:%d:%d", okB ? 1 : 0, firstInliers, held, visits);
    report += buf;
    store.erase(K[1]);
  }
  printf("RELOC_%s%s\n", fails == 0 ? "OK" : "FAIL", report.c_str());
  return fails == 0 ? 0 : 1;
}
