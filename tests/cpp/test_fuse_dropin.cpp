// The fuseMapPoints drop-in (orbfe_fuse_dropin.hpp) over minimal Camera / Frame / KeyFrame / MapPoint / Map types, linked to
// liborbfe_hip.so.  The map written by tests/test_gpu_fuse.py is built twice: copy A goes through orbfe::dropin::fuseMapPoints, copy B
// through the reference-shaped chain of the existing bodies (the forward orbfe::dropin::fuse, then orbfe::dropin::fuse(pkf, cur, map) per
// target, then updateConnections) with the targets and the forward fuse's map points in the order A's containers give.  Exit code 0 and
// "OK <nFuse total> <device-flag uses> <re-evaluations> <replaces>" when the two final maps are equal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <unordered_set>

#include <opencv2/opencv.hpp>

namespace ref {
struct Camera {
  static inline float mfFx = 0, mfFy = 0, mfCx = 0, mfCy = 0, mfBl = 0;
};
struct Frame {
  static inline std::vector<float> sf;
  static float getScaledFactor(const int& l) { return sf[(size_t)l]; }
};

struct KeyFrame;
struct Map {
  typedef std::shared_ptr<Map> SharedPtr;
  int nReplaced = 0;
};

struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  long id = 0;
  float pos[3], view[3], mMax = 0, mMin = 0;
  bool bad = false, inMap = true;
  cv::Mat desc;
  std::map<int, std::pair<KeyFrame*, std::size_t>> obs;  // by keyframe id
  bool isBad() const { return bad; }
  bool isInMap() const { return inMap; }
  int getObsNum() const { return (int)obs.size(); }
  cv::Mat getDesc() const { return desc; }
  cv::Mat getPos() const { return vec(pos); }
  cv::Mat getViewDirection() const { return vec(view); }
  void getDistance(float& mx, float& mn) const { mx = mMax, mn = mMin; }
  void addMatchInTrack() {}
  static cv::Mat vec(const float* v) {
    cv::Mat m(3, 1, CV_32F);
    for (int a = 0; a < 3; ++a) m.at<float>(a) = v[a];
    return m;
  }
  void addObservation(std::shared_ptr<KeyFrame> kf, std::size_t idx) { addObservation(kf.get(), idx); }
  void addObservation(KeyFrame* kf, std::size_t idx);
  void updateNormalAndDepth();
  static void replace(SharedPtr keep, SharedPtr drop, Map::SharedPtr map);
  // MapPoint::isInVision (src/MapPoint.cc:141-171) in the float / double mix csrc/k_guided.hip documents
  template <class FramePtr>
  bool isInVision(FramePtr f, float& dist, cv::Point2f& uv, float& cosTheta) {
    float R[9], t[3], pc[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R[3 * r + c] = f->mRcw.template at<float>(r, c);
      t[r] = f->mtcw.template at<float>(r, 0);
    }
    for (int r = 0; r < 3; ++r) {
      const float s = R[3 * r] * pos[0] + R[3 * r + 1] * pos[1] + R[3 * r + 2] * pos[2];
      pc[r] = (float)((double)s + (double)t[r]);
    }
    if (pc[2] < 0.f) return false;
    const float x = pc[0], y = pc[1], z = pc[2];
    const float distance = std::sqrt(x * x + y * y + z * z);
    dist = distance;
    if (!(distance < mMax && distance > mMin)) return false;
    const float u = x / z * Camera::mfFx + Camera::mfCx, v = y / z * Camera::mfFy + Camera::mfCy;
    uv.x = u, uv.y = v;
    if (!(u < f->mfMaxU && v < f->mfMaxV && u > f->mfMinU && v > f->mfMinV)) return false;
    float vd[3];
    for (int r = 0; r < 3; ++r) vd[r] = R[3 * r] * view[0] + R[3 * r + 1] * view[1] + R[3 * r + 2] * view[2];
    const double nn = (double)vd[0] * (double)vd[0] + (double)vd[1] * (double)vd[1] + (double)vd[2] * (double)vd[2];
    const float vabs = (float)std::sqrt(nn);
    const double dot = (double)vd[0] * (double)pc[0] + (double)vd[1] * (double)pc[1] + (double)vd[2] * (double)pc[2];
    cosTheta = (float)(dot / (double)(distance * vabs));
    return !(cosTheta < 0.5f);
  }
  int predictLevel(float distance) const {
    const float lr = (float)std::log((double)(mMax / distance));
    const int level = (int)std::lrintf(lr / std::log(1.2f));
    return level < 0 ? 0 : (level > 7 ? 7 : level);
  }
};

struct KeyFrame {
  typedef std::shared_ptr<KeyFrame> SharedPtr;
  int id = 0;
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<cv::Mat> mvLeftDescriptor;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw, mtcw;
  float centre[3];
  float mfMinU = 0, mfMaxU = 0, mfMinV = 0, mfMaxV = 0;
  std::vector<SharedPtr> conn;
  static inline int nUpdateConnections = 0;
  static float getScaledFactor2(const int& l) { return std::pow(Frame::getScaledFactor(l), 2); }
  std::vector<SharedPtr> getOrderedConnectedKfs(int n) { return std::vector<SharedPtr>(conn.begin(), conn.begin() + std::min<size_t>((size_t)n, conn.size())); }
  bool isBad() const { return false; }
  void getPose(cv::Mat& R, cv::Mat& t) const { R = mRcw.clone(), t = mtcw.clone(); }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  MapPoint::SharedPtr getMapPoint(std::size_t i) { return mvpMapPoints[i]; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) {
    if ((size_t)idx >= mvpMapPoints.size()) mvpMapPoints.resize((size_t)idx + 1);  // (keyframes that only observe have no feature arrays)
    mvpMapPoints[(size_t)idx] = p;
  }
  static void updateConnections(SharedPtr) { ++nUpdateConnections; }
};

static int hamming(const cv::Mat& a, const cv::Mat& b) {
  int d = 0;
  for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a.data[i] ^ b.data[i]));
  return d;
}
// MapPoint::addObservation (src/MapPoint.cc:21-45): a second feature of the same keyframe keeps the closer descriptor
void MapPoint::addObservation(KeyFrame* kf, std::size_t idx) {
  auto it = obs.find(kf->id);
  if (it == obs.end()) {
    obs[kf->id] = {kf, idx};
    return;
  }
  if (kf->mvLeftDescriptor.empty()) return;
  const int d1 = hamming(kf->mvLeftDescriptor[it->second.second], desc), d2 = hamming(kf->mvLeftDescriptor[idx], desc);
  it->second.second = d1 < d2 ? it->second.second : idx;
}
// MapPoint::updateNormalAndDepth (src/MapPoint.cc:429-484) with a valid reference keyframe: the mean viewing direction
void MapPoint::updateNormalAndDepth() {
  if (obs.empty()) {
    bad = true;
    return;
  }
  float v[3] = {0, 0, 0};
  for (const auto& o : obs)
    for (int a = 0; a < 3; ++a) v[a] = v[a] + (pos[a] - o.second.first->centre[a]);
  const double nrm = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
  for (int a = 0; a < 3; ++a) view[a] = nrm > 0 ? (float)((double)v[a] * (1.0 / nrm)) : v[a];
}
// MapPoint::replace (src/MapPoint.cc:213-233)
void MapPoint::replace(SharedPtr keep, SharedPtr drop, Map::SharedPtr map) {
  drop->bad = true;
  auto old = drop->obs;
  drop->obs.clear();
  for (const auto& o : old) {
    if (keep->obs.count(o.first)) continue;
    o.second.first->setMapPoint((int)o.second.second, keep);
    keep->addObservation(o.second.first, o.second.second);
  }
  keep->updateNormalAndDepth();
  ++map->nReplaced;
}
}  // namespace ref

#include "orbfe_fuse_dropin.hpp"

using namespace ref;

struct World {
  std::map<int, KeyFrame::SharedPtr> kfs;
  std::map<long, MapPoint::SharedPtr> pts;
  KeyFrame::SharedPtr cur;
  Map::SharedPtr map = std::make_shared<Map>();
};

static float rd(std::istream& in) {
  double v;
  in >> v;
  return (float)v;
}
static cv::Mat rdDesc(std::istream& in) {
  cv::Mat d(1, 32, CV_8U);
  for (int b = 0; b < 32; ++b) {
    int v;
    in >> v;
    d.data[b] = (uint8_t)v;
  }
  return d;
}

static World load(const char* path) {
  std::ifstream in(path);
  World w;
  Camera::mfFx = rd(in), Camera::mfFy = rd(in), Camera::mfCx = rd(in), Camera::mfCy = rd(in), Camera::mfBl = rd(in);
  int nl = 0, nkf = 0;
  in >> nl;
  Frame::sf.clear();
  for (int l = 0; l < nl; ++l) Frame::sf.push_back(rd(in));
  in >> nkf;
  for (int k = 0; k < nkf; ++k) {
    auto kf = std::make_shared<KeyFrame>();
    int n = 0;
    in >> kf->id >> n;
    for (int a = 0; a < 3; ++a) kf->centre[a] = rd(in);
    kf->mRcw = cv::Mat(3, 3, CV_32F), kf->mtcw = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) kf->mRcw.at<float>(r, c) = rd(in);
    for (int r = 0; r < 3; ++r) kf->mtcw.at<float>(r, 0) = rd(in);
    kf->mfMinU = rd(in), kf->mfMaxU = rd(in), kf->mfMinV = rd(in), kf->mfMaxV = rd(in);
    for (int i = 0; i < n; ++i) {
      cv::KeyPoint kp;
      kp.pt.x = rd(in), kp.pt.y = rd(in);
      in >> kp.octave;
      kf->mvFeatsLeft.push_back(kp);
      kf->mvLeftDescriptor.push_back(rdDesc(in));
    }
    kf->mvpMapPoints.resize((size_t)n);
    w.kfs[kf->id] = kf;
    if (k == 0) w.cur = kf;
  }
  for (int k = 0; k < nkf; ++k) {  // the covisibility lists, strongest first
    int id = 0, c = 0;
    in >> id >> c;
    for (int j = 0; j < c; ++j) {
      int o;
      in >> o;
      w.kfs[id]->conn.push_back(w.kfs[o]);
    }
  }
  int np = 0;
  in >> np;
  for (int p = 0; p < np; ++p) {
    auto m = std::make_shared<MapPoint>();
    int inmap = 0, nobs = 0;
    in >> m->id;
    for (int a = 0; a < 3; ++a) m->pos[a] = rd(in);
    for (int a = 0; a < 3; ++a) m->view[a] = rd(in);
    m->mMax = rd(in), m->mMin = rd(in);
    in >> inmap;
    m->inMap = inmap != 0;
    m->desc = rdDesc(in);
    in >> nobs;
    for (int o = 0; o < nobs; ++o) {
      int kid;
      std::size_t feat;
      in >> kid >> feat;
      m->obs[kid] = {w.kfs[kid].get(), feat};
    }
    w.pts[m->id] = m;
  }
  for (int k = 0; k < nkf; ++k) {  // the slots
    int id = 0, c = 0;
    in >> id >> c;
    for (int j = 0; j < c; ++j) {
      int feat;
      long pid;
      in >> feat >> pid;
      w.kfs[id]->setMapPoint(feat, w.pts[pid]);
    }
  }
  return w;
}

static std::string dump(const World& w) {
  std::ostringstream o;
  for (const auto& k : w.kfs) {
    o << "K" << k.first;
    for (size_t i = 0; i < k.second->mvpMapPoints.size(); ++i)
      if (k.second->mvpMapPoints[i]) o << ' ' << i << ':' << k.second->mvpMapPoints[i]->id;
    o << '\n';
  }
  for (const auto& p : w.pts) {
    o << "P" << p.first << ' ' << p.second->bad;
    for (const auto& ob : p.second->obs) o << ' ' << ob.first << ':' << ob.second.second;
    o << '\n';
  }
  return o.str();
}

// the selection of LocalMapping::fuseMapPoints (src/LocalMapping.cc:354-397) on this copy's pointers: the iteration orders as ids
static void selection(KeyFrame::SharedPtr cur, std::vector<int>& kfOrder, std::vector<long>& mpOrder) {
  std::unordered_set<KeyFrame::SharedPtr> sTargetKfs;
  std::unordered_set<MapPoint::SharedPtr> sTargetMps, sNoMps;
  sTargetKfs.insert(cur);
  for (auto item : cur->getOrderedConnectedKfs(10)) {
    int nNum = 0;
    sTargetKfs.insert(item);
    for (auto pkf : item->getOrderedConnectedKfs(100))
      if (sTargetKfs.find(pkf) == sTargetKfs.end()) {
        sTargetKfs.insert(pkf);
        if (++nNum == 5) break;
      }
  }
  for (auto& pkf : sTargetKfs)
    for (auto& p : pkf->getMapPoints())
      if (p && !p->isBad()) sTargetMps.insert(p);
  for (auto& p : cur->getMapPoints())
    if (p && !p->isBad()) sNoMps.insert(p);
  for (auto& pkf : sTargetKfs) kfOrder.push_back(pkf->id);
  for (auto& p : sTargetMps)
    if (!sNoMps.count(p)) mpOrder.push_back(p->id);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  ORB_SLAM2_ROS2::ORBExtractor::mnLevels = 8;
  World A = load(argv[1]), B = load(argv[1]);
  if (dump(A) != dump(B)) return 3;
  std::vector<int> kfOrder;
  std::vector<long> mpOrder;
  selection(A.cur, kfOrder, mpOrder);
  orbfe::dropin::fuseMapPoints<Camera, Frame>(A.cur, A.map);
  const long long flags = orbfe::dropin::fuseDeviceFlagUses(), reeval = orbfe::dropin::fuseReevaluations();
  const int nFuseA = orbfe::dropin::fuseLastCount();
  // B: the reference-shaped chain of the existing bodies
  std::vector<MapPoint::SharedPtr> vTargetMps;
  for (long id : mpOrder) vTargetMps.push_back(B.pts[id]);
  int nFuse = orbfe::dropin::fuse(B.cur, vTargetMps, B.map, false, 3.0f, 0.6f, ORB_SLAM2_ROS2::ORBExtractor::mnLevels);
  for (int id : kfOrder) nFuse += orbfe::dropin::fuse<Camera>(B.kfs[id], B.cur, B.map, 0.6f);
  KeyFrame::updateConnections(B.cur);
  const std::string a = dump(A), b = dump(B);
  if (a != b || nFuseA != nFuse || A.map->nReplaced != B.map->nReplaced || KeyFrame::nUpdateConnections != 2) {
    std::fprintf(stderr, "maps differ: %d vs %d fuses, %d vs %d replaces, %zu vs %zu bytes of state\n", nFuseA, nFuse, A.map->nReplaced, B.map->nReplaced, a.size(), b.size());
    return 1;
  }
  std::printf("OK %d %lld %lld %d %zu\n", nFuse, flags, reeval, B.map->nReplaced, kfOrder.size());
  return 0;
}
