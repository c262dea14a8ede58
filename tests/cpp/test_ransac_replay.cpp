// The one replay of Ransac<T>::iterate (csrc/ransac_replay.h), compiled by the host compiler alone and run on the tables
// tests/test_ransac_replay.py writes: the speculations' records are data here, as they are for the library, which downloads them.
//   test_ransac_replay IN OUT
// IN (little-endian 32-bit words; floats and mask halves as their bits):
//   n_scenario | per scenario:
//     policy (0 PnpPolicy, 1 Sim3Policy) n_prob n_spec n_call engine | per problem: n min_inlier max_it
//     per speculation, in the order the calls will ask for them:
//       n_rec n_hyp | per record: prob n h0 nh entry_hyp engine_start after[nh]
//       per hypothesis: words degen count refined ref_count model[12] ref_model[12] mask[2 * words] ref_mask[2 * words]
//     per call: problem n_iterations set_engine (0: leave it) has model[12] cap n_inliers inliers[n_inliers]
// OUT (32-bit words), per call:
//   verdict ret no_more has model[12] n_inliers inliers[..] engine cur best skipped (a bit per problem) n_speculations-so-far |
//   speculated (0 / 1) and, if so, what speculate received: problem n has_entry entry_len
// A call that asks for a speculation when the scenario has none left gets a failed one.  Prints OK and returns 0 when everything ran.
#include <cstdio>
#include <cstdlib>

#include "ransac_replay.h"

using namespace ransac;

static std::vector<int32_t> read_all(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  std::vector<int32_t> v;
  int32_t buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(int32_t), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

struct Reader {
  const std::vector<int32_t>& v;
  size_t at = 0;
  const int32_t* take(size_t n) {
    if (at + n > v.size()) {
      fprintf(stderr, "input ends early (%zu + %zu > %zu)\n", at, n, v.size());
      exit(2);
    }
    const int32_t* p = v.data() + at;
    at += n;
    return p;
  }
  int32_t one() { return *take(1); }
};

// one hypothesis of a speculation, as a download would hold it
struct Hyp {
  int32_t degen, count, refined, ref_count;
  float model[12], ref_model[12];
  std::vector<uint64_t> mask, ref_mask;
};
struct Spec {
  std::vector<CallRec> recs;
  std::vector<Hyp> hyps;
};

static void words64(Reader& r, int32_t words, std::vector<uint64_t>& out) {
  out.resize((size_t)words);
  if (words) std::memcpy(out.data(), r.take(2 * (size_t)words), 8 * (size_t)words);
}

static Spec read_spec(Reader& r) {
  Spec s;
  const int32_t n_rec = r.one(), n_hyp = r.one();
  for (int32_t i = 0; i < n_rec; ++i) {
    const int32_t* p = r.take(6);
    CallRec c{p[0], p[1], p[2], p[3], p[4], (uint32_t)p[5], {}};
    const int32_t* a = r.take((size_t)c.nh);
    c.after.assign(a, a + c.nh);
    s.recs.push_back(std::move(c));
  }
  s.hyps.resize((size_t)n_hyp);
  for (Hyp& h : s.hyps) {
    const int32_t* p = r.take(5);
    h.degen = p[1], h.count = p[2], h.refined = p[3], h.ref_count = p[4];
    std::memcpy(h.model, r.take(12), sizeof h.model);
    std::memcpy(h.ref_model, r.take(12), sizeof h.ref_model);
    words64(r, p[0], h.mask);
    words64(r, p[0], h.ref_mask);
  }
  return s;
}

template <class Policy>
static void scenario(Reader& r, int32_t n_prob, int32_t n_spec, int32_t n_call, uint32_t engine, std::vector<int32_t>& out) {
  std::vector<Prob> probs((size_t)n_prob);
  for (Prob& p : probs) {
    const int32_t* v = r.take(3);
    p.n = v[0], p.min_inlier = v[1], p.max_it = v[2];
    p.words = (p.n + 63) / 64;
  }
  std::vector<Spec> specs;
  for (int32_t i = 0; i < n_spec; ++i) specs.push_back(read_spec(r));
  Records R;
  const Spec* live = nullptr;  // the speculation whose download the records index
  int32_t n_speculations = 0;
  for (int32_t c = 0; c < n_call; ++c) {
    const int32_t* a = r.take(4);
    const int32_t problem = a[0], n_iterations = a[1];
    if (a[2]) engine = (uint32_t)a[2];
    int32_t has = a[3], ret = -1, no_more = 0;
    float model[12];
    std::memcpy(model, r.take(12), sizeof model);
    const int64_t cap = r.one();
    int64_t n_inliers = r.one();
    const int32_t* entry = r.take((size_t)n_inliers);
    std::vector<int32_t> buf(entry, entry + n_inliers);
    buf.resize((size_t)std::max<int64_t>(cap, n_inliers));  // exactly the room the caller declares: a write past it is a finding
    int32_t asked[5] = {0, 0, 0, 0, 0};
    const Verdict v = iterate<Policy>(
        probs, R, engine, problem, n_iterations, model, &has, buf.data(), &n_inliers, cap, &ret, &no_more,
        [&](size_t h) {
          const Hyp& o = live->hyps.at(h);
          return HypView{o.degen != 0, o.model, o.mask.data(), o.count, o.refined != 0, o.ref_model, o.ref_mask.data(), o.ref_count};
        },
        [&](int32_t p, int32_t n, const float*, bool has_entry, const int32_t*, int64_t entry_len) {
          const int32_t got[5] = {1, p, n, has_entry, (int32_t)entry_len};
          std::memcpy(asked, got, sizeof asked);
          if (n_speculations == n_spec) return false;
          live = &specs[(size_t)n_speculations++];
          R.recs = live->recs;
          return true;
        });
    const int32_t head[4] = {(int32_t)v, ret, no_more, has};
    out.insert(out.end(), head, head + 4);
    int32_t bits[12];
    std::memcpy(bits, model, sizeof bits);
    out.insert(out.end(), bits, bits + 12);
    out.push_back((int32_t)n_inliers);
    if (v == kDone) out.insert(out.end(), buf.begin(), buf.begin() + n_inliers);
    const Prob& p = probs[(size_t)problem];
    int32_t skipped = 0;
    for (int32_t q = 0; q < n_prob; ++q) skipped |= (int32_t)probs[(size_t)q].skipped << q;
    const int32_t tail[5] = {(int32_t)engine, p.cur, p.best, skipped, n_speculations};
    out.insert(out.end(), tail, tail + 5);
    out.insert(out.end(), asked, asked + (asked[0] ? 5 : 1));
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  const std::vector<int32_t> in = read_all(argv[1]);
  Reader r{in};
  std::vector<int32_t> out;
  const int32_t n_scenario = r.one();
  for (int32_t s = 0; s < n_scenario; ++s) {
    const int32_t* h = r.take(5);
    if (h[0] == 0) scenario<PnpPolicy>(r, h[1], h[2], h[3], (uint32_t)h[4], out);
    else scenario<Sim3Policy>(r, h[1], h[2], h[3], (uint32_t)h[4], out);
  }
  if (r.at != in.size()) return fprintf(stderr, "%zu words of input left over\n", in.size() - r.at), 2;
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) return perror(argv[2]), 2;
  fclose(f);
  printf("OK %d scenarios\n", n_scenario);
  return 0;
}
