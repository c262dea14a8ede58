// orbfe_kfdb_dropin_impl.hpp -- the bodies of the drop-in KeyFrameDB (orbfe_kfdb_dropin.hpp); src/KeyFrameDB.cc becomes one line that
// includes this file.  The rules are KeyFrameDB.cc's; the count, the word filter, the scores and
// the score filter run on the device (orbfe_kfdb_query on the calling thread's orbfe::dropin::matcherContext()), the group filter on the
// host over the caller's own covisibility lists (orbfe_kfdb_group_filter).
// Define ORBFE_KFDB_OWN_TYPES to bring KeyFrame / Frame from elsewhere (tests/cpp/test_kfdb_dropin.cpp) instead of the reference's headers.
#pragma once

#ifndef ORBFE_KFDB_OWN_TYPES
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/KeyFrameDB.h"
#endif

#include <algorithm>

#include "orbfe_dropin.hpp"
#include "orbfe_kfdb_dropin.hpp"

namespace ORB_SLAM2_ROS2 {

namespace kfdb_detail {
inline void split(const DBoW3::BowVector& v, std::vector<uint32_t>& words, std::vector<double>& values) {
  words.clear();
  values.clear();
  words.reserve(v.size());
  values.reserve(v.size());
  for (const auto& item : v) {  // a std::map: words ascending
    words.push_back((uint32_t)item.first);
    values.push_back(item.second);
  }
}
// the device the database lives on: the one orbfe::dropin::matcherContext() uses
inline int32_t device() { return 0; }
}  // namespace kfdb_detail

KeyFrameDB::KeyFrameDB(std::size_t nWordNum) { orbfe::check(nullptr, orbfe_kfdb_create(kfdb_detail::device(), (int32_t)nWordNum, &mpDb)); }

KeyFrameDB::~KeyFrameDB() { orbfe_kfdb_destroy(mpDb); }

void KeyFrameDB::addKeyFrame(KeyFramePtr pKf) {
  pKf->computeBow();
  std::vector<uint32_t> words;
  std::vector<double> values;
  kfdb_detail::split(pKf->getBowVec(), words, values);
  const uint64_t id = (uint64_t)pKf->getID();
  const int64_t offsets[2] = {0, (int64_t)words.size()};
  std::unique_lock<std::mutex> lock(mMutex);
  if (mKfs.count(id)) return;  // the reference's std::set: nothing changes
  orbfe::check(nullptr, orbfe_kfdb_add(mpDb, 1, &id, offsets, words.data(), values.data()));
  mKfs.emplace(id, pKf);
  mBad.emplace(id, false);
}

void KeyFrameDB::eraseKeyFrame(KeyFramePtr pKf) {
  const uint64_t id = (uint64_t)pKf->getID();
  std::unique_lock<std::mutex> lock(mMutex);
  orbfe::check(nullptr, orbfe_kfdb_erase(mpDb, 1, &id));
  mKfs.erase(id);
  mBad.erase(id);
}

std::vector<KeyFrameDB::Survivor> KeyFrameDB::query(const DBoW3::BowVector& bow, const std::vector<uint64_t>& ignore, const double* minScore) {
  std::vector<uint32_t> words;
  std::vector<double> values;
  kfdb_detail::split(bow, words, values);
  std::vector<Survivor> out;
  std::unique_lock<std::mutex> lock(mMutex);
  // isBad() as it is now: only the flags that changed travel
  std::vector<uint64_t> ids;
  std::vector<uint8_t> flags;
  for (auto& item : mKfs) {
    const bool bad = item.second->isBad();
    bool& held = mBad[item.first];
    if (bad != held) {
      ids.push_back(item.first);
      flags.push_back(bad ? 1 : 0);
      held = bad;
    }
  }
  if (!ids.empty()) orbfe::check(nullptr, orbfe_kfdb_set_bad(mpDb, (int32_t)ids.size(), ids.data(), flags.data()));
  const size_t cap = std::max<size_t>(mKfs.size(), 1);
  std::vector<uint64_t> sid(cap);
  std::vector<int32_t> cnt(cap);
  std::vector<double> score(cap);
  const orbfe_kfdb_query_in q{words.data(), values.data(), (int32_t)words.size(), ignore.data(), (int32_t)ignore.size(), minScore};
  int64_t n = 0;
  orbfe_ctx* ctx = orbfe::dropin::matcherContext();
  orbfe::check(ctx, orbfe_kfdb_query(ctx, mpDb, &q, sid.data(), cnt.data(), score.data(), (int64_t)cap, &n));
  out.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) out.push_back(Survivor{mKfs.at(sid[(size_t)i]), score[(size_t)i]});
  return out;
}

void KeyFrameDB::groupFilter(const std::vector<Survivor>& survivors, std::vector<KeyFramePtr>& candidateKfs) {
  const size_t n = survivors.size();
  std::vector<uint64_t> ids(n), conn, out(std::max<size_t>(n, 1));
  std::vector<double> scores(n);
  std::vector<int64_t> offsets(n + 1, 0);
  std::unordered_map<uint64_t, KeyFramePtr> byId;
  for (size_t i = 0; i < n; ++i) {
    ids[i] = (uint64_t)survivors[i].kf->getID();
    scores[i] = survivors[i].score;
    byId.emplace(ids[i], survivors[i].kf);
    for (const auto& pKf : survivors[i].kf->getOrderedConnectedKfs(10)) {  // covisibility: the caller's map state, asked for the survivors only
      if (!pKf || pKf->isBad()) continue;
      conn.push_back((uint64_t)pKf->getID());
    }
    offsets[i + 1] = (int64_t)conn.size();
  }
  int64_t n_out = 0;
  orbfe::check(nullptr, orbfe_kfdb_group_filter((int64_t)n, ids.data(), scores.data(), offsets.data(), conn.data(), out.data(), &n_out));
  for (int64_t i = 0; i < n_out; ++i) candidateKfs.push_back(byId.at(out[(size_t)i]));
}

double KeyFrameDB::minScore(KeyFramePtr pFrame) {
  auto vConnected = pFrame->getConnectedKfs(15);
  if (vConnected.empty()) return 0;
  double minScore = 1;
  const DBoW3::BowVector& bow = pFrame->getBowVec();
  std::vector<uint64_t> inDb;
  {
    std::unique_lock<std::mutex> lock(mMutex);
    for (auto& kf : vConnected) {
      if (!kf || kf->isBad()) continue;
      const uint64_t id = (uint64_t)kf->getID();
      if (mKfs.count(id) && mKfs.at(id) == kf) {
        inDb.push_back(id);
      } else {  // not in the database yet: its similarity on the host, DBoW's L1 score as computeSimilarity runs it
        const double score = DBoW3::Vocabulary::l1Score(bow, kf->getBowVec());
        if (score < minScore) minScore = score;
      }
    }
  }
  if (!inDb.empty()) {
    std::vector<uint32_t> words;
    std::vector<double> values;
    kfdb_detail::split(bow, words, values);
    std::vector<double> scores(inDb.size());
    const orbfe_kfdb_query_in q{words.data(), values.data(), (int32_t)words.size(), nullptr, 0, nullptr};
    orbfe_ctx* ctx = orbfe::dropin::matcherContext();
    orbfe::check(ctx, orbfe_kfdb_score(ctx, mpDb, &q, inDb.data(), (int32_t)inDb.size(), scores.data()));
    for (double score : scores)
      if (score < minScore) minScore = score;
  }
  return minScore;
}

void KeyFrameDB::findRelocKfs(FramePtr pFrame, std::vector<KeyFramePtr>& candidateKfs) {
  candidateKfs.clear();
  pFrame->computeBow();
  groupFilter(query(pFrame->getBowVec(), {}, nullptr), candidateKfs);
}

void KeyFrameDB::findLoopCloseKfs(KeyFramePtr pFrame, std::vector<KeyFramePtr>& candidateKfs) {
  pFrame->computeBow();
  std::vector<uint64_t> ignore;
  for (auto& item : pFrame->getAllConnected()) {
    KeyFramePtr pKf = item.first.lock();
    if (pKf && !pKf->isBad()) ignore.push_back((uint64_t)pKf->getID());
  }
  const double floor = minScore(pFrame);
  groupFilter(query(pFrame->getBowVec(), ignore, &floor), candidateKfs);
}

}  // namespace ORB_SLAM2_ROS2
