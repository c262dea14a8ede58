// orbfe_sim3_dropin.hpp -- the reference's Sim3Solver (include/ORB_SLAM2/Sim3Solver.h, src/Sim3Solver.cc) on the device Sim3 RANSAC
// sets (orbfe_sim3, include/orbfe.h).  INTEGRATION.md section 14:
//     using DeviceSim3Solver = orbfe::Sim3Solver<KeyFrame, Sim3Ret, Camera>;
// is what LoopClosing::computeSim3 (src/LoopClosing.cc:300-415) names instead of Sim3Solver, and what orbfe::dropin::sim3Candidates
// (orbfe_reloc_dropin.hpp) takes as its Sim3SolverT.  A template over the reference's types, like the other drop-ins: KeyFrameT gives
// getMapPoint / getPose / getLeftKeyPoint / getScaledFactor2, Sim3RetT is the reference's Sim3Ret (mRqp, mtqp, mfS, error()), CameraT
// gives mfFx .. mfCy.  The public interface is the reference's: create(pKfp, pKfq, pqMatches, vbChoose, ...) with its vbChoose filter
// (Sim3Solver.cc:173-182) and iterate(int, Sim3Ret&, bool&, vector<size_t>&), which is Ransac<Sim3Ret>::iterate exactly.
// As in the reference, create ignores bFixScale and nMinSet (S1: the scale is fixed, three pairs a sample).  Solvers created one after
// another on a thread before the first iterate of any of them form one orbfe_sim3 set, in creation order (computeSim3's first loop); the
// set is uploaded at that first iterate.  Solvers with other RANSAC parameters start a set of their own.  A failed library call throws
// std::runtime_error.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/opencv.hpp>

#include "orbfe.h"

namespace orbfe {
namespace sim3_detail {

struct Batch {
  std::vector<int64_t> offsets{0};
  std::vector<float> posP, posQ, poseP, poseQ;
  std::vector<int32_t> octP, octQ;
  orbfe_sim3_params params{3, 100, 0.4f, 0.99f};
  orbfe_sim3* set = nullptr;
  std::mutex mu;

  ~Batch() {
    if (set) orbfe_sim3_destroy(set);
  }
};

// the batch solvers created on this thread join until one of them iterates
inline std::weak_ptr<Batch>& open_batch() {
  static thread_local std::weak_ptr<Batch> b;
  return b;
}

inline void check(orbfe_status st) {
  if (st != ORBFE_OK) throw std::runtime_error(std::string("orbfe_sim3: ") + orbfe_last_error(nullptr));
}

inline void push3(std::vector<float>& v, const cv::Mat& m) {
  for (int r = 0; r < 3; ++r) v.push_back(m.at<float>(r));
}
inline void push_pose(std::vector<float>& v, const cv::Mat& R, const cv::Mat& t) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v.push_back(R.at<float>(r, c));
  push3(v, t);
}

}  // namespace sim3_detail

template <class KeyFrameT, class Sim3RetT, class CameraT>
class Sim3Solver {
 public:
  typedef std::shared_ptr<Sim3Solver> SharedPtr;
  typedef std::shared_ptr<KeyFrameT> KeyFramePtr;

  static SharedPtr create(KeyFramePtr pKfp, KeyFramePtr pKfq, const std::vector<cv::DMatch>& pqMatches, std::vector<bool>& vbChoose,
                          bool /*bFixScale*/ = true, int /*nMinSet*/ = 3, int nMaxIterations = 100, float fRatio = 0.4, float fProb = 0.99) {
    using sim3_detail::Batch;
    std::shared_ptr<Batch> b = sim3_detail::open_batch().lock();
    const bool same = b && b->params.max_iterations == nMaxIterations && b->params.ratio == fRatio && b->params.prob == fProb;
    if (!b || b->set || !same) {
      b = std::make_shared<Batch>();
      b->params = orbfe_sim3_params{3, nMaxIterations, fRatio, fProb};
      sim3_detail::open_batch() = b;
    }
    SharedPtr s(new Sim3Solver());
    s->mpBatch = b;
    s->mnProblem = (int)b->offsets.size() - 1;
    cv::Mat Rpw, tpw, Rqw, tqw;
    pKfp->getPose(Rpw, tpw);
    pKfq->getPose(Rqw, tqw);
    sim3_detail::push_pose(b->poseP, Rpw, tpw);
    sim3_detail::push_pose(b->poseQ, Rqw, tqw);
    int jdx = 0;
    for (const auto& pqMatch : pqMatches) {
      const int qIdx = pqMatch.queryIdx, pIdx = pqMatch.trainIdx;
      auto pMpP = pKfp->getMapPoint(pIdx);
      auto pMpQ = pKfq->getMapPoint(qIdx);
      if (!pMpP || pMpP->isBad() || !pMpQ || pMpQ->isBad()) {
        vbChoose[jdx++] = false;
        continue;
      }
      sim3_detail::push3(b->posP, pMpP->getPos());
      sim3_detail::push3(b->posQ, pMpQ->getPos());
      b->octP.push_back(pKfp->getLeftKeyPoint(pIdx).octave);
      b->octQ.push_back(pKfq->getLeftKeyPoint(qIdx).octave);
      ++s->mnN;
      ++jdx;
    }
    b->offsets.push_back(b->offsets.back() + (int64_t)s->mnN);
    return s;
  }

  bool iterate(int nIterations, Sim3RetT& modelRet, bool& bNoMore, std::vector<std::size_t>& vnInlierIndices) {
    sim3_detail::Batch& b = *mpBatch;
    std::lock_guard<std::mutex> lk(b.mu);
    upload(b);
    float model[12] = {};
    int32_t has = modelRet.error() ? 0 : 1;
    if (has) {
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) model[3 * r + c] = modelRet.mRqp.template at<float>(r, c);
        model[9 + r] = modelRet.mtqp.template at<float>(r);
      }
    }
    const int64_t cap = (int64_t)(vnInlierIndices.size() > (std::size_t)mnN ? vnInlierIndices.size() : (std::size_t)mnN) + 1;
    std::vector<int32_t> buf((std::size_t)cap);
    for (std::size_t i = 0; i < vnInlierIndices.size(); ++i) buf[i] = (int32_t)vnInlierIndices[i];
    int64_t k = (int64_t)vnInlierIndices.size();
    int32_t ret = 0, no_more = 0;
    sim3_detail::check(orbfe_sim3_iterate(b.set, mnProblem, nIterations, model, &has, buf.data(), &k, cap, &ret, &no_more));
    if (no_more) bNoMore = true;
    if (has) {
      modelRet.mRqp = cv::Mat(3, 3, CV_32F);
      modelRet.mtqp = cv::Mat(3, 1, CV_32F);
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) modelRet.mRqp.template at<float>(r, c) = model[3 * r + c];
        modelRet.mtqp.template at<float>(r) = model[9 + r];
      }
      modelRet.mfS = 1.0f;
    }
    vnInlierIndices.assign(buf.begin(), buf.begin() + k);
    return ret != 0;
  }

  /// the set's problem this solver is, and its number of correspondences (after the vbChoose filter)
  int problem() const { return mnProblem; }
  int size() const { return mnN; }

  Sim3Solver(const Sim3Solver&) = delete;
  Sim3Solver& operator=(const Sim3Solver&) = delete;

 private:
  Sim3Solver() = default;

  static void upload(sim3_detail::Batch& b) {
    if (b.set) return;
    int max_oct = 0;
    for (int32_t o : b.octP) max_oct = o > max_oct ? o : max_oct;
    for (int32_t o : b.octQ) max_oct = o > max_oct ? o : max_oct;
    std::vector<float> sigma2((std::size_t)max_oct + 1);
    for (int l = 0; l <= max_oct; ++l) sigma2[(std::size_t)l] = KeyFrameT::getScaledFactor2(l);
    orbfe_camera cam{};
    cam.fx = CameraT::mfFx;
    cam.fy = CameraT::mfFy;
    cam.cx = CameraT::mfCx;
    cam.cy = CameraT::mfCy;
    sim3_detail::check(orbfe_sim3_create(0, (int32_t)b.offsets.size() - 1, b.offsets.data(), b.posP.data(), b.posQ.data(), b.octP.data(),
                                         b.octQ.data(), b.poseP.data(), b.poseQ.data(), sigma2.data(), (int32_t)sigma2.size(), &cam,
                                         &b.params, &b.set));
  }

  std::shared_ptr<sim3_detail::Batch> mpBatch;  ///< the set this solver belongs to
  int mnProblem = 0;                            ///< its problem in the set
  int mnN = 0;                                  ///< its number of correspondences
};

}  // namespace orbfe
