// The DBoW3 drop-in (orb_slam2_ros2_amd/host/compat/DBoW3/DBoW3.h) through the compiler and at run time; tests/test_bow_vocab.py (host-only
// modes) and tests/test_gpu_bow.py (device modes) drive it.  cv::Mat / cv::KeyPoint come from the stand-in tests/cpp/stubs/opencv2/core.hpp.
//   score <vocab.txt> <vectors.txt>                     size(), then DBoW's L1 score of every pair of BowVectors in the file (host only)
//   transform <vocab.txt> <desc.raw> <n> <levelsup>     Vocabulary::transform (std::vector<cv::Mat> and cv::Mat forms) on the device
//   searchbow <vocab.txt> <f.raw> <n1> <k.raw> <n2> <fv_f.txt> <fv_k.txt>
//                                                       orbfe::dropin::searchByBow with FeatureVectors made by computeBow on the device,
//                                                       then with the given ones (the restatement's): both match lists
#include <DBoW3/DBoW3.h>

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>

namespace {

struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  bool isBad() const { return false; }
  bool isInMap() const { return true; }
  void addMatchInTrack() {}
};

// the members VirtualFrame::computeBow and ORBMatcher::searchByBow touch (include/ORB_SLAM2/Frame.h:224-231)
struct BowFrame {
  typedef std::shared_ptr<BowFrame> SharedPtr;
  std::vector<cv::Mat> mvLeftDescriptor;
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  DBoW3::BowVector mBowVec;
  DBoW3::FeatureVector mFeatVec;
  const DBoW3::Vocabulary* mpVoc = nullptr;
  void computeBow() {
    if (mBowVec.empty()) mpVoc->transform(mvLeftDescriptor, mBowVec, mFeatVec, 4);
  }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
};

uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}
double from_bits(uint64_t u) {
  double v;
  std::memcpy(&v, &u, 8);
  return v;
}

std::vector<cv::Mat> read_desc(const char* path, int n) {
  std::vector<uint8_t> raw((size_t)n * 32);
  std::FILE* f = std::fopen(path, "rb");
  if (!f || std::fread(raw.data(), 1, raw.size(), f) != raw.size()) throw std::runtime_error(std::string("cannot read ") + path);
  std::fclose(f);
  std::vector<cv::Mat> d;
  for (int i = 0; i < n; ++i) {
    cv::Mat m(1, 32, CV_8U);
    std::memcpy(m.data, &raw[(size_t)i * 32], 32);
    d.push_back(m);
  }
  return d;
}

// `n_nodes` then per node: `node count f0 f1 ..`
DBoW3::FeatureVector read_fv(const char* path) {
  std::ifstream is(path);
  DBoW3::FeatureVector fv;
  size_t nn = 0;
  is >> nn;
  for (size_t i = 0; i < nn; ++i) {
    unsigned node = 0;
    size_t c = 0;
    is >> node >> c;
    auto& v = fv[node];
    v.resize(c);
    for (auto& x : v) is >> x;
  }
  return fv;
}

void print(const DBoW3::BowVector& v, const DBoW3::FeatureVector& fv) {
  std::printf("%zu %zu\n", v.size(), fv.size());
  for (const auto& w : v) std::printf("W %u %016" PRIx64 "\n", w.first, bits(w.second));
  for (const auto& n : fv) {
    std::printf("N %u", n.first);
    for (unsigned f : n.second) std::printf(" %u", f);
    std::printf("\n");
  }
}

BowFrame::SharedPtr frame(const DBoW3::Vocabulary& voc, const char* path, int n, bool withMapPoints) {
  auto F = std::make_shared<BowFrame>();
  F->mpVoc = &voc;
  F->mvLeftDescriptor = read_desc(path, n);
  F->mvFeatsLeft.resize((size_t)n);
  F->mvpMapPoints.resize((size_t)n);
  if (withMapPoints)
    for (auto& p : F->mvpMapPoints) p = std::make_shared<MapPoint>();
  return F;
}

int run(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "score" && argc == 4) {
    DBoW3::Vocabulary voc(argv[2]);
    std::ifstream is(argv[3]);
    size_t pairs = 0;
    is >> pairs;
    std::printf("SCORE_OK %u %d\n", voc.size(), (int)voc.empty());
    auto readv = [&]() {
      DBoW3::BowVector v;
      size_t c = 0;
      is >> c;
      for (size_t i = 0; i < c; ++i) {
        unsigned w = 0;
        std::string hex;
        is >> w >> hex;
        v[w] = from_bits(std::stoull(hex, nullptr, 16));
      }
      return v;
    };
    for (size_t p = 0; p < pairs; ++p) {
      const DBoW3::BowVector a = readv(), b = readv();
      std::printf("%016" PRIx64 "\n", bits(voc.score(a, b)));
    }
    return 0;
  }
  if (mode == "transform" && argc == 6) {
    DBoW3::Vocabulary voc(argv[2]);
    const int n = std::atoi(argv[4]), levelsup = std::atoi(argv[5]);
    const auto d = read_desc(argv[3], n);
    DBoW3::BowVector v, v2;
    DBoW3::FeatureVector fv, fv2;
    voc.transform(d, v, fv, levelsup);
    cv::Mat rows(n, 32, CV_8U);
    for (int i = 0; i < n; ++i) std::memcpy(rows.data + (size_t)i * rows.step, d[(size_t)i].data, 32);
    voc.transform(rows, v2, fv2, levelsup);
    std::printf("TRANSFORM_OK %d ", (int)(v == v2 && fv == fv2));
    print(v, fv);
    return 0;
  }
  if (mode == "searchbow" && argc == 9) {
    DBoW3::Vocabulary voc(argv[2]);
    const int n1 = std::atoi(argv[4]), n2 = std::atoi(argv[6]);
    auto match = [&](bool device) {
      auto F = frame(voc, argv[3], n1, false), K = frame(voc, argv[5], n2, true);
      if (!device) {  // the restatement's FeatureVectors; a non-empty BowVector keeps computeBow from running
        F->mFeatVec = read_fv(argv[7]), K->mFeatVec = read_fv(argv[8]);
        F->mBowVec[0] = 1.0, K->mBowVec[0] = 1.0;
      }
      std::vector<cv::DMatch> m;
      orbfe::dropin::searchByBow(F, K, m, false, false, 0.8f, false);
      return std::make_tuple(m, F->mFeatVec, K->mFeatVec);
    };
    const auto dev = match(true), ref = match(false);
    const auto& md = std::get<0>(dev);
    const auto& mr = std::get<0>(ref);
    bool same = md.size() == mr.size();
    for (size_t i = 0; same && i < md.size(); ++i)
      same = md[i].queryIdx == mr[i].queryIdx && md[i].trainIdx == mr[i].trainIdx && md[i].distance == mr[i].distance;
    const bool fv_same = std::get<1>(dev) == std::get<1>(ref) && std::get<2>(dev) == std::get<2>(ref);
    std::printf("SEARCHBOW_OK %zu %zu %d %d\n", md.size(), mr.size(), (int)same, (int)fv_same);
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of tests/cpp/test_bow.cpp\n");
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    return run(argc, argv);
  } catch (const std::exception& e) {
    std::printf("ERROR %s\n", e.what());
    return 1;
  }
}
