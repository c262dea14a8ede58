// ransac_replay.h -- what the reference's Ransac<T> template holds (include/ORB_SLAM2/Ransac.hpp), for the speculated sets: a problem's
// state, the records of one speculation, and the ONE replay of an iterate call from those records.  PnPSolver and Sim3Solver differ in
// four switches (PnpPolicy, Sim3Policy below).  Host only, no HIP: tests/cpp/test_ransac_replay.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ransac {

struct PnpPolicy {
  static constexpr int kMinSet = 4;
  static constexpr bool kCheckClears = false;    // P1: checkInliers appends to the caller's list
  static constexpr bool kEntryMatters = true;    // P2: the entry pose is counted again, so an entry state breaks the prediction
  static constexpr bool kTracksSkipped = false;
};
struct Sim3Policy {
  static constexpr int kMinSet = 3;
  static constexpr bool kCheckClears = true;     // S2: every checkInliers clears the list
  static constexpr bool kEntryMatters = false;   // modelFunc always writes: the entry model and list change no result
  static constexpr bool kTracksSkipped = true;   // computeSim3 never iterates a candidate it discarded after making its solver
};

// one problem (solver) of a set
struct Prob {
  int32_t off = 0, n = 0, words = 0, min_inlier = 0, max_it = 0;
  int32_t cur = 0, best = 0;
  bool called = false;
  bool skipped = false;  // the caller left it out where the schedule had it: speculations leave it out until it is called again
  float best_model[12] = {};
  std::vector<int32_t> best_list;
};

// what one speculated call found: its hypotheses [h0, h0 + nh) of the download, the record of its entry model (-1: none), the engine
// before it and after each hypothesis
struct CallRec {
  int32_t prob, n, h0, nh, entry_hyp;
  uint32_t engine_start;
  std::vector<uint32_t> after;
};

// the speculation being replayed: recs[next] is the call expected next
struct Records {
  std::vector<CallRec> recs;
  size_t next = 0;
};
inline void drop_records(Records& R) {
  R.recs.clear();
  R.next = 0;
}

// one hypothesis as the device recorded it; refined: a usable refine record exists
struct HypView {
  bool degen;
  const float* model;
  const uint64_t* mask;
  int32_t count;
  bool refined;
  const float* ref_model;
  const uint64_t* ref_mask;
  int32_t ref_count;
};

// the hypotheses a call of n iterations may still try
inline int32_t budget(const Prob& p, int min_set, int32_t n, int32_t cur) { return p.n >= min_set ? std::max(0, std::min(n, p.max_it - cur)) : 0; }

// the set bits of m[0 .. words), ascending, appended to list
inline void append_bits(const uint64_t* m, int32_t words, std::vector<int32_t>& list) {
  for (int32_t w = 0; w < words; ++w)
    for (uint64_t b = m[w]; b; b &= b - 1) list.push_back(w * 64 + __builtin_ctzll(b));
}

enum Verdict { kDone, kSpeculationFailed, kInconsistent, kNoEntryRecord, kNoRefineRecord, kNoRoom };

// Ransac<T>::iterate(n_iterations, model, bNoMore, inliers) of `problem`, replayed from the records.  The call's record is the next one
// when the call is the predicted one, an empty one when the budget is spent, else recs[0] of a new speculation:
// speculate(problem, n, entry model, has entry model, entry list, its length) fills R.recs and whatever view(h) reads, false on failure.
// The replay runs on copies, committed only when the result fits `cap`; every other exit but kDone has dropped the records and left
// the problem, the engine and the caller's arguments alone (kNoRoom: *n_inliers is the room needed).
template <class Policy, class View, class Speculate>
Verdict iterate(std::vector<Prob>& probs, Records& R, uint32_t& engine, int32_t problem, int32_t n_iterations, float* model, int32_t* has_model,
                int32_t* inliers, int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more, View&& view, Speculate&& speculate) {
  Prob& pr = probs[(size_t)problem];
  *ret = 0;
  const int32_t k = budget(pr, Policy::kMinSet, n_iterations, pr.cur);
  // the next record serves this call if the call is the predicted one: same problem and n, engine untouched, no entry state that counts
  const bool pending = R.next > 0 && R.next < R.recs.size();
  bool hit = pending && !(Policy::kEntryMatters && (*has_model || *n_inliers));
  if (hit) {
    const CallRec& r = R.recs[R.next];
    hit = r.prob == problem && r.n == n_iterations && r.engine_start == engine && r.nh == k;
  }
  if (Policy::kTracksSkipped) {
    if (!hit && pending) {
      // The caller left out problems the schedule had before this one: they would break every round's prediction, so later schedules
      // omit them.
      const size_t end = std::min(R.recs.size(), R.next + probs.size());
      size_t j = R.next;
      while (j < end && R.recs[j].prob != problem) ++j;
      if (j < end)
        for (size_t i = R.next; i < j; ++i) probs[(size_t)R.recs[i].prob].skipped = true;
    }
    pr.skipped = false;
  }
  if (pr.n < Policy::kMinSet) {  // P5, S5
    if (hit) R.next += 1;
    else drop_records(R);
    pr.called = true;
    *no_more = 1;
    return kDone;
  }
  const CallRec spent{problem, n_iterations, 0, 0, -1, engine, {}};
  const CallRec* r = &spent;
  if (hit) {
    r = &R.recs[R.next++];
  } else if (k == 0) {  // the budget is spent: nothing for the device
    drop_records(R);
  } else {
    const bool has_entry = Policy::kEntryMatters && *has_model;
    if (!speculate(problem, n_iterations, model, has_entry, inliers, Policy::kEntryMatters ? *n_inliers : 0)) return drop_records(R), kSpeculationFailed;
    if (R.recs.empty()) return drop_records(R), kInconsistent;
    r = &R.recs[0];
    R.next = 1;
  }
  if (r->nh != k || r->prob != problem || r->after.size() != (size_t)k) return drop_records(R), kInconsistent;
  // replay Ransac::iterate on copies
  std::vector<int32_t> list(inliers, inliers + *n_inliers);
  float cur_model[12];
  std::memcpy(cur_model, model, sizeof cur_model);
  bool has = *has_model != 0;
  int32_t cur = pr.cur, best = pr.best;
  bool best_changed = false;
  float best_model[12];
  std::vector<int32_t> best_list;
  // the inliers of the model as it stands: a degenerate sample leaves it, and it is counted again (P2)
  const uint64_t* st_mask = nullptr;
  int32_t st_cnt = 0;
  if (r->entry_hyp >= 0) {
    const HypView e = view((size_t)r->entry_hyp);
    st_mask = e.mask;
    st_cnt = e.count;
  }
  bool success = false;
  uint32_t eng = engine;
  for (int32_t i = 0; i < r->nh; ++i) {
    const HypView o = view((size_t)(r->h0 + i));
    if (!o.degen) {
      std::memcpy(cur_model, o.model, sizeof cur_model);
      has = true;
      st_mask = o.mask;
      st_cnt = o.count;
    }
    eng = r->after[(size_t)i];
    if (has) {
      if (!st_mask) return drop_records(R), kNoEntryRecord;
      if (Policy::kCheckClears) list.clear();
      append_bits(st_mask, pr.words, list);
      if (st_cnt > pr.min_inlier) {
        if (st_cnt > best) {
          best = st_cnt;
          best_changed = true;
          std::memcpy(best_model, cur_model, sizeof best_model);
          best_list = list;
        }
        if (!o.refined) return drop_records(R), kNoRefineRecord;
        std::memcpy(cur_model, o.ref_model, sizeof cur_model);
        st_mask = o.ref_mask;
        st_cnt = o.ref_count;
        list.clear();
        append_bits(st_mask, pr.words, list);
        if (st_cnt > pr.min_inlier) {
          success = true;  // P3, S3: the budget is not spent
          break;
        }
      }
    }
    ++cur;
  }
  const std::vector<int32_t>* res = &list;
  const float* res_model = cur_model;
  bool res_has = has;
  if (!success && (best_changed ? best : pr.best) > 0) {  // P4, S4
    res = best_changed ? &best_list : &pr.best_list;
    res_model = best_changed ? best_model : pr.best_model;
    res_has = true;
  }
  if ((int64_t)res->size() > cap) {
    *n_inliers = (int64_t)res->size();
    return drop_records(R), kNoRoom;
  }
  // commit
  *ret = success || res != &list;
  std::copy(res->begin(), res->end(), inliers);
  *n_inliers = (int64_t)res->size();
  std::memcpy(model, res_model, 12 * sizeof(float));
  *has_model = res_has ? 1 : 0;
  if (!success && cur >= pr.max_it) *no_more = 1;
  pr.cur = cur;
  pr.called = true;
  if (best_changed) {
    pr.best = best;
    std::memcpy(pr.best_model, best_model, sizeof best_model);
    pr.best_list = std::move(best_list);
  }
  engine = eng;
  if (success) drop_records(R);
  return kDone;
}

}  // namespace ransac
