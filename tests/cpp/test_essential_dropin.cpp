// dropin::optimizeEssentialGraph (orbfe_essential_dropin.hpp) over minimal KeyFrame / MapPoint / Map / Sim3Ret types: the whole body of
// Optimizer::optimizeEssentialGraph -- vertex selection and the corrected / uncorrected Sim3 choice, the three edge sources with the
// graphTh and sAlreadyConnected rules, the measurements, the device call, the poses and the map points written back -- on the scene
// tests/test_essential_graph_host.py writes.
//   test_essential_dropin IN build   everything up to the device call (no device needed): prints the graph and the refusals
//   test_essential_dropin IN full    the whole function: prints the poses and the map points afterwards
// IN: nkf maxid | per keyframe: id bad parent(-1: none) pose[12] nLoopEdges ids.. nCov (id weight).. | nCorrected (id model[12]).. |
//     nNoCorrected (id model[12]).. | nLoopConn (id1 k ids..).. | loopId currId graphTh | nMp (bad pos[3] refId loopKfId loopRefId)..
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <set>

#include <opencv2/opencv.hpp>

// the two cv::Mat operations the function's tail uses, for the stand-in cv::Mat of tests/cpp/stubs (declared there, defined nowhere)
namespace cv {
Mat operator/(const Mat& a, double s) {
  Mat o(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) o.at<float>(r, c) = (float)(a.at<float>(r, c) / s);
  return o;
}
}  // namespace cv

#include "orbfe_essential_dropin.hpp"

namespace {

struct KeyFrame;
using KeyFramePtr = std::shared_ptr<KeyFrame>;

struct KeyFrame {
  static std::size_t maxId;
  static std::size_t getMaxID() { return maxId; }
  std::size_t id = 0;
  bool bad = false;
  cv::Mat R, t;
  std::weak_ptr<KeyFrame> parent;
  std::vector<KeyFramePtr> loopEdges;
  std::vector<std::pair<KeyFramePtr, int>> cov;  // in descending weight, as getConnectedKfs returns them
  int posesSet = 0;
  bool isBad() const { return bad; }
  std::size_t getID() const { return id; }
  void getPose(cv::Mat& Rcw, cv::Mat& tcw) const {
    Rcw = R;
    tcw = t;
  }
  void setPose(const cv::Mat& Rcw, const cv::Mat& tcw) {
    R = Rcw.clone();
    t = tcw.clone();
    ++posesSet;
  }
  int getWeight(const KeyFramePtr& o) const {
    for (auto& c : cov)
      if (c.first == o) return c.second;
    return 0;
  }
  std::vector<KeyFramePtr> getLoopEdges() const { return loopEdges; }
  std::weak_ptr<KeyFrame> getParent() const { return parent; }
  std::vector<KeyFramePtr> getConnectedKfs(int th) const {
    std::vector<KeyFramePtr> v;
    for (auto& c : cov)
      if (c.second >= th) v.push_back(c.first);
    return v;
  }
};
std::size_t KeyFrame::maxId = 0;

struct MapPoint {
  cv::Mat pos;
  bool bad = false;
  KeyFramePtr ref, loopKf, loopRef;
  int descriptors = 0, normals = 0;
  bool isBad() const { return bad; }
  KeyFramePtr getLoopKF() const { return loopKf; }
  KeyFramePtr getLoopRefKF() const { return loopRef; }
  void setLoopRefKF(KeyFramePtr p) { loopRef = p; }
  KeyFramePtr getRefKF() const { return ref; }
  cv::Mat getPos() const { return pos; }
  void setPos(const cv::Mat& p) { pos = p.clone(); }
  void updateDescriptor() { ++descriptors; }
  void updateNormalAndDepth() { ++normals; }
};

struct Map {
  std::vector<KeyFramePtr> kfs;
  std::vector<std::shared_ptr<MapPoint>> mps;
  bool updated = false;
  std::vector<KeyFramePtr> getAllKeyFrames() const { return kfs; }
  std::vector<std::shared_ptr<MapPoint>> getAllMapPoints() const { return mps; }
  void setUpdate(bool b) { updated = b; }
};

// the reference's Sim3Ret (include/ORB_SLAM2/Sim3Solver.h) with its arithmetic spelled in float, every sum left to right
struct Sim3Ret {
  Sim3Ret() = default;
  Sim3Ret(const cv::Mat& Rqp, const cv::Mat& tqp, const float& s) : mfS(s) {
    Rqp.copyTo(mRqp);
    tqp.copyTo(mtqp);
  }
  Sim3Ret inv() const {
    Sim3Ret S;
    S.mfS = 1.0f / mfS;
    S.mRqp = cv::Mat(3, 3, CV_32F);
    S.mtqp = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) S.mRqp.at<float>(r, c) = mRqp.at<float>(c, r);
    for (int r = 0; r < 3; ++r) {
      const float v = (S.mRqp.at<float>(r, 0) * mtqp.at<float>(0) + S.mRqp.at<float>(r, 1) * mtqp.at<float>(1)) + S.mRqp.at<float>(r, 2) * mtqp.at<float>(2);
      S.mtqp.at<float>(r) = -S.mfS * v;
    }
    return S;
  }
  cv::Mat mRqp, mtqp;
  float mfS = 0.f;
};
cv::Mat operator*(const Sim3Ret& S, const cv::Mat& Q) {
  cv::Mat o(3, 1, CV_32F);
  for (int r = 0; r < 3; ++r) {
    const float v = (S.mRqp.at<float>(r, 0) * Q.at<float>(0) + S.mRqp.at<float>(r, 1) * Q.at<float>(1)) + S.mRqp.at<float>(r, 2) * Q.at<float>(2);
    o.at<float>(r) = S.mfS * v + S.mtqp.at<float>(r);
  }
  return o;
}

unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}
unsigned long long bits(double f) {
  unsigned long long u;
  std::memcpy(&u, &f, 8);
  return u;
}

Sim3Ret readSim3(std::istream& in, float s = 1.f) {
  cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) in >> R.at<float>(r, c);
  for (int r = 0; r < 3; ++r) in >> t.at<float>(r);
  return Sim3Ret(R, t, s);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN build|full\n", argv[0]), 2;
  const bool full = std::string(argv[2]) == "full";
  std::ifstream in(argv[1]);
  int nkf = 0;
  in >> nkf >> KeyFrame::maxId;
  auto map = std::make_shared<Map>();
  std::map<long, KeyFramePtr> byId;
  struct Links {
    long parent;
    std::vector<long> loops;
    std::vector<std::pair<long, int>> cov;
  };
  std::vector<Links> links((size_t)nkf);
  for (int k = 0; k < nkf; ++k) {
    auto kf = std::make_shared<KeyFrame>();
    int bad = 0, n = 0;
    in >> kf->id >> bad >> links[(size_t)k].parent;
    kf->bad = bad != 0;
    const Sim3Ret pose = readSim3(in);
    kf->R = pose.mRqp, kf->t = pose.mtqp;
    in >> n;
    links[(size_t)k].loops.resize((size_t)n);
    for (auto& v : links[(size_t)k].loops) in >> v;
    in >> n;
    links[(size_t)k].cov.resize((size_t)n);
    for (auto& v : links[(size_t)k].cov) in >> v.first >> v.second;
    byId[(long)kf->id] = kf;
    map->kfs.push_back(kf);
  }
  map->kfs.push_back(nullptr);  // (getAllKeyFrames may hold a null: :775)
  for (int k = 0; k < nkf; ++k) {
    auto& kf = map->kfs[(size_t)k];
    if (links[(size_t)k].parent >= 0) kf->parent = byId.at(links[(size_t)k].parent);
    for (long v : links[(size_t)k].loops) kf->loopEdges.push_back(byId.at(v));
    for (auto& v : links[(size_t)k].cov) kf->cov.push_back({byId.at(v.first), v.second});
  }
  std::map<KeyFramePtr, Sim3Ret> corrected, noCorrected;
  for (auto* m : {&corrected, &noCorrected}) {
    int n = 0;
    in >> n;
    for (int i = 0; i < n; ++i) {
      long id;
      in >> id;
      (*m)[byId.at(id)] = readSim3(in);
    }
  }
  std::map<KeyFramePtr, std::set<KeyFramePtr>> loopConn;
  int nConn = 0;
  in >> nConn;
  for (int i = 0; i < nConn; ++i) {
    long id1;
    int k;
    in >> id1 >> k;
    for (int j = 0; j < k; ++j) {
      long id2;
      in >> id2;
      loopConn[byId.at(id1)].insert(byId.at(id2));
    }
  }
  long loopId, currId;
  int graphTh;
  in >> loopId >> currId >> graphTh;
  KeyFramePtr pLoopKf = byId.at(loopId), pCurrKf = byId.at(currId);
  int nMp = 0;
  in >> nMp;
  for (int i = 0; i < nMp; ++i) {
    auto mp = std::make_shared<MapPoint>();
    int bad;
    long ref, lk, lr;
    mp->pos = cv::Mat(3, 1, CV_32F);
    in >> bad >> mp->pos.at<float>(0) >> mp->pos.at<float>(1) >> mp->pos.at<float>(2) >> ref >> lk >> lr;
    mp->bad = bad != 0;
    if (ref >= 0) mp->ref = byId.at(ref);
    if (lk >= 0) mp->loopKf = byId.at(lk);
    if (lr >= 0) mp->loopRef = byId.at(lr);
    map->mps.push_back(mp);
  }
  if (!in) return fprintf(stderr, "input ends early\n"), 2;

  using namespace orbfe::dropin;
  {
    // the graph, in both modes (std::map and std::set of shared_ptr iterate in address order: the reader takes the order of the loop
    // connections' edges from here)
    auto G = buildEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, corrected, noCorrected, true);
    for (size_t v = 0; v < G.ids.size(); ++v) {
      printf("v %zu %d", G.ids[v], (int)G.fixed[v]);
      for (int k = 0; k < 8; ++k) printf(" %016llx", bits(G.estimates[8 * v + (size_t)k]));
      printf("\n");
    }
    for (size_t e = 0; e < G.v0.size(); ++e) {
      printf("e %zu %zu", G.ids[(size_t)G.v0[e]], G.ids[(size_t)G.v1[e]]);
      for (int k = 0; k < 8; ++k) printf(" %016llx", bits(G.meas[8 * e + (size_t)k]));
      printf("\n");
    }
  }
  if (!full) {
    auto refused = [&](const char* what, auto&& f) {
      try {
        f();
        printf("%s: NOT refused\n", what);
      } catch (const std::invalid_argument&) {
        printf("%s: invalid_argument\n", what);
      } catch (const std::runtime_error&) {
        printf("%s: runtime_error\n", what);
      }
    };
    refused("free scale", [&] { buildEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, corrected, noCorrected, false); });
    refused("free scale, whole function", [&] { optimizeEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, corrected, noCorrected, false); });
    auto scaled = corrected;
    scaled.begin()->second.mfS = 1.5f;
    refused("mfS != 1", [&] { buildEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, scaled, noCorrected, true); });
    auto scaledNo = noCorrected;
    scaledNo.begin()->second.mfS = 0.5f;
    refused("mfS != 1, uncorrected", [&] { buildEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, corrected, scaledNo, true); });
    byId.at(0)->bad = true;  // no good keyframe of id 0: refused before anything is launched or written
    refused("no keyframe 0", [&] { optimizeEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, corrected, noCorrected, true); });
    int touched = 0;
    for (auto& kf : map->kfs) touched += kf ? kf->posesSet : 0;
    printf("poses set: %d, map updated: %d\n", touched, (int)map->updated);
    return 0;
  }
  optimizeEssentialGraph<Sim3Ret>(loopConn, map, pLoopKf, pCurrKf, graphTh, corrected, noCorrected, true);
  for (auto& kf : map->kfs) {
    if (!kf) continue;
    printf("kf %zu %d", kf->id, kf->posesSet);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) printf(" %08x", bits(kf->R.at<float>(r, c)));
    for (int r = 0; r < 3; ++r) printf(" %08x", bits(kf->t.at<float>(r)));
    printf("\n");
  }
  for (auto& mp : map->mps)
    printf("mp %08x %08x %08x %d %d %d\n", bits(mp->pos.at<float>(0)), bits(mp->pos.at<float>(1)), bits(mp->pos.at<float>(2)), mp->descriptors,
           mp->normals, mp->loopRef ? 1 : 0);
  printf("map updated: %d\n", (int)map->updated);
  return 0;
}
