// The createNewMapPoints drop-in (orbfe_mapping_dropin.hpp) over minimal Camera / Frame / KeyFrame / MapPoint / Map types, linked to
// liborbfe_hip.so.  Input (written by tests/test_gpu_triangulation.py): camera, KInv, baseline, scale factors, then the current keyframe
// and its neighbours.  Output: the neighbour order the drop-in chose (input indices), then one line per entry of mlpAddedMPs:
// query, the neighbour's input index and train index (-1 -1 for a tail point), kind of origin, the position as float bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <list>
#include <map>
#include <memory>
#include <unordered_map>

#include <opencv2/opencv.hpp>

namespace ORB_SLAM2_ROS2 {
struct Camera {
  static float mfFx, mfFy, mfCx, mfCy, mfBl;
  static cv::Mat mKInv;
};
float Camera::mfFx, Camera::mfFy, Camera::mfCx, Camera::mfCy, Camera::mfBl;
cv::Mat Camera::mKInv;
struct Frame {
  static std::vector<float> sf;
  static float getScaledFactor(const int& l) { return sf[(size_t)l]; }
};
std::vector<float> Frame::sf;

struct KeyFrame;
struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  float pos[3];
  bool inMap = false, fromUnproc = false;
  int query = -1, nbIdx = -1, train = -1;
  static SharedPtr create(cv::Mat p) {
    auto m = std::make_shared<MapPoint>();
    for (int a = 0; a < 3; ++a) m->pos[a] = p.at<float>(a);
    return m;
  }
  bool isBad() const { return false; }
  bool isInMap() const { return inMap; }
  cv::Mat getPos() const {
    cv::Mat p(3, 1, CV_32F);
    for (int a = 0; a < 3; ++a) p.at<float>(a) = pos[a];
    return p;
  }
  void addAttriInit(std::shared_ptr<KeyFrame>, std::size_t q) { query = (int)q; }
  void addObservation(std::shared_ptr<KeyFrame> kf, std::size_t t);
  void updateDescriptor() {}
  void updateNormalAndDepth() {}
};

struct KeyFrame {
  typedef std::shared_ptr<KeyFrame> SharedPtr;
  int inputIdx = -1;
  std::vector<cv::KeyPoint> kps;
  std::vector<cv::Mat> desc;
  std::vector<MapPoint::SharedPtr> mps;
  std::vector<double> depth, ru;
  std::map<unsigned, std::vector<unsigned>> mFeatVec;
  cv::Mat Tcw, Twc, Ow;
  std::vector<SharedPtr> conn;
  std::vector<SharedPtr> getOrderedConnectedKfs(int n) { return std::vector<SharedPtr>(conn.begin(), conn.begin() + std::min<size_t>(n, conn.size())); }
  bool isBad() const { return false; }
  cv::Mat getFrameCenter() const { return Ow; }
  void computeBow() {}
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return kps; }
  const std::vector<cv::Mat>& getDescriptor() const { return desc; }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mps; }
  const std::vector<double>& getDepth() const { return depth; }
  const std::vector<double>& getRightU() const { return ru; }
  cv::Mat getPose() const { return Tcw; }
  cv::Mat getPoseInv() const { return Twc; }
  void setMapPoint(int idx, MapPoint::SharedPtr p) { mps[(size_t)idx] = p; }
};
void MapPoint::addObservation(std::shared_ptr<KeyFrame> kf, std::size_t t) { nbIdx = kf->inputIdx, train = (int)t; }

struct Map {
  typedef std::shared_ptr<Map> SharedPtr;
  void insertMapPoint(MapPoint::SharedPtr p, SharedPtr) { p->inMap = true; }
};
}  // namespace ORB_SLAM2_ROS2

#include "orbfe_mapping_dropin.hpp"

using namespace ORB_SLAM2_ROS2;

static float rd(std::istream& in) {
  double v;
  in >> v;
  return (float)v;
}
static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}
static cv::Mat mat(std::istream& in, int r, int c) {
  cv::Mat m(r, c, CV_32F);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) m.at<float>(i, j) = rd(in);
  return m;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  Camera::mfFx = rd(in), Camera::mfFy = rd(in), Camera::mfCx = rd(in), Camera::mfCy = rd(in);
  Camera::mKInv = mat(in, 3, 3);
  Camera::mfBl = rd(in);
  int nl = 0, nkf = 0;
  in >> nl;
  for (int l = 0; l < nl; ++l) Frame::sf.push_back(rd(in));
  in >> nkf;
  std::vector<KeyFrame::SharedPtr> kfs;
  KeyFrame::SharedPtr cur;
  std::unordered_map<std::size_t, MapPoint::SharedPtr> unproc;
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
          unproc[(std::size_t)i] = m;
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
    if (k == 0) cur = kf;
    else kfs.push_back(kf);
  }
  cur->conn = kfs;
  auto map = std::make_shared<Map>();
  std::list<MapPoint::SharedPtr> added;
  orbfe::dropin::createNewMapPoints<Camera, Frame>(cur, unproc, map, added);
  std::map<KeyFrame::SharedPtr, int> order;
  for (auto& k : kfs) order.emplace(k, 0);
  for (auto& it : order) std::printf("%d ", it.first->inputIdx);
  std::printf("\n");
  for (auto& m : added) {
    const bool slot = cur->mps[(size_t)m->query] == m;
    std::printf("%d %d %d %d %08x %08x %08x %d\n", m->query, m->nbIdx, m->train, m->fromUnproc ? 1 : 0, bits(m->pos[0]), bits(m->pos[1]),
                bits(m->pos[2]), slot ? 1 : 0);
  }
  return 0;
}
