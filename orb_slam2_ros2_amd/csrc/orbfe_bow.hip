// orbfe_bow.hip -- host side of the bag-of-words entry points (include/orbfe.h): the ORB-SLAM2 text vocabulary parser, the per-device
// copy of the tree, orbfe_bow_transform / orbfe_bow_slots.  The transform's rules are listed at the top of k_bow.hip.
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "orbfe_ctx.h"

void launch_bow(hipStream_t s, const uint8_t* d_desc, size_t desc_img_stride, const int32_t* d_counts, int count_step, int n_fixed, int n_img, int cap,
                const BowVocabDev& vd, int levelsup, uint64_t* d_wkey, uint64_t* d_nkey, double* d_wts, size_t key_stride, uint32_t* o_words,
                double* o_values, uint32_t* o_nodes, int32_t* o_offsets, uint32_t* o_features, int32_t* o_counts);

namespace {
constexpr int kMaxDevices = 64;
}

struct orbfe_vocab {
  int32_t k = 0, L = 0, n_nodes = 0, n_words = 0;
  // the parse, in node-id order
  std::vector<int32_t> parent, word_id;
  std::vector<uint8_t> is_leaf, desc;
  std::vector<double> weight;
  // the device layout (orbfe_internal.h), by position
  std::vector<BowChild> rec;
  std::vector<uint8_t> cdesc;
  std::vector<double> cweight;
  int32_t root_nc = 0;
  // one copy per HIP device, made by the first call that needs it there (every context on the device shares it); a failed upload
  // leaves nothing behind and the next call tries again
  struct Dev {
    std::mutex mu;
    std::atomic<bool> ready{false};
    BowChild* rec = nullptr;
    uint4* desc = nullptr;
    double* weight = nullptr;
  };
  mutable Dev dev[kMaxDevices];
};

namespace {

inline bool is_blank(char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f'; }

// one integer token of [p, e): optional sign, decimal digits, then a blank or the line's end
bool parse_int(const char*& p, const char* e, long long& out) {
  while (p < e && is_blank(*p)) ++p;
  if (p == e) return false;
  bool neg = false;
  if (*p == '-' || *p == '+') neg = *p++ == '-';
  if (p == e || *p < '0' || *p > '9') return false;
  long long v = 0;
  while (p < e && *p >= '0' && *p <= '9') {
    if (v < (1ll << 40)) v = v * 10 + (*p - '0');
    ++p;
  }
  if (p < e && !is_blank(*p)) return false;
  out = neg ? -v : v;
  return true;
}

// a decimal number: [+-] digits [. digits] [e [+-] digits], as `ssnode >> weight` reads it -- no nan / inf / hex; std::from_chars rounds
// correctly and does not depend on the process's LC_NUMERIC
bool parse_double(const char*& p, const char* e, double& out) {
  while (p < e && is_blank(*p)) ++p;
  const char* q = p;
  while (q < e && !is_blank(*q)) ++q;
  const char* b = p;
  if (b < q && *b == '+') ++b;
  const char* c = b;
  if (c < q && *c == '-') ++c;
  bool digit = false, ok = c < q;
  for (const char* x = c; x < q && ok; ++x) {
    digit |= *x >= '0' && *x <= '9';
    ok = (*x >= '0' && *x <= '9') || *x == '.' || *x == 'e' || *x == 'E' || ((*x == '+' || *x == '-') && (x[-1] == 'e' || x[-1] == 'E'));
  }
  if (!ok || !digit || (b != p && *b == '-')) return false;
  const auto r = std::from_chars(b, q, out, std::chars_format::general);
  if (r.ec != std::errc() || r.ptr != q) return false;
  p = q;
  return true;
}

orbfe_status bad(const char* path, long line, const char* what) {
  return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_load_txt: %s:%ld: %s", path, line, what);
}

orbfe_status load_txt(const char* path, orbfe_vocab& v) {
  FILE* fp = std::fopen(path, "rb");
  if (!fp) return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_load_txt: cannot open %s", path);
  std::vector<char> buf;
  {
    std::fseek(fp, 0, SEEK_END);
    const long sz = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    buf.resize(sz > 0 ? (size_t)sz + 1 : 1);
    const size_t got = sz > 0 ? std::fread(buf.data(), 1, (size_t)sz, fp) : 0;
    std::fclose(fp);
    if (sz < 0 || got != (size_t)sz) return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_load_txt: cannot read %s", path);
    buf[got] = 0;
  }
  const char* p = buf.data();
  const char* const end = p + buf.size() - 1;
  auto line_end = [&](const char* s) {
    const void* nl = std::memchr(s, '\n', (size_t)(end - s));
    return nl ? (const char*)nl : end;
  };
  // header
  const char* e = line_end(p);
  long long hk, hL, hs, hw;
  if (!parse_int(p, e, hk) || !parse_int(p, e, hL) || !parse_int(p, e, hs) || !parse_int(p, e, hw)) return bad(path, 1, "malformed header (want `k L scoring weighting`)");
  while (p < e && is_blank(*p)) ++p;
  if (p != e) return bad(path, 1, "malformed header (extra tokens)");
  if (hk < 2 || hk > 20) return bad(path, 1, "k outside 2..20");
  if (hL < 1 || hL > 10) return bad(path, 1, "L outside 1..10");
  if (hs != 0 || hw != 0) return bad(path, 1, "scoring / weighting other than 0 0 (L1 norm, TF-IDF)");
  v.k = (int32_t)hk;
  v.L = (int32_t)hL;
  const size_t guess = (size_t)(end - buf.data()) / 80 + 1;
  v.parent.reserve(guess);
  v.is_leaf.reserve(guess);
  v.desc.reserve(guess * 32);
  v.weight.reserve(guess);
  v.word_id.reserve(guess);
  std::vector<int32_t> nchild, depth;
  nchild.reserve(guess);
  depth.reserve(guess);
  // the root
  v.parent.push_back(-1);
  v.is_leaf.push_back(0);
  v.desc.insert(v.desc.end(), 32, 0);
  v.weight.push_back(0.0);
  v.word_id.push_back(-1);
  nchild.push_back(0);
  depth.push_back(0);
  int32_t words = 0;
  long line = 1;
  p = e < end ? e + 1 : end;
  while (p < end) {
    e = line_end(p);
    ++line;
    const char* s = p;
    p = e < end ? e + 1 : end;
    while (s < e && is_blank(*s)) ++s;
    if (s == e) continue;  // blank line: skipped (documented)
    const long long id = (long long)v.parent.size();
    if (id >= 0x7FFFFFFF) return bad(path, line, "too many nodes");
    long long pid, leaf, b;
    if (!parse_int(s, e, pid) || !parse_int(s, e, leaf)) return bad(path, line, "truncated or malformed line");
    if (leaf != 0 && leaf != 1) return bad(path, line, "is_leaf other than 0 / 1");
    if (pid < 0 || pid >= id) return bad(path, line, "parent id not below the node's own id");
    if (v.is_leaf[(size_t)pid]) return bad(path, line, "parent is a leaf");
    if (nchild[(size_t)pid] >= v.k) return bad(path, line, "more than k children under one node");
    if (depth[(size_t)pid] + 1 > v.L) return bad(path, line, "depth > L");
    for (int i = 0; i < 32; ++i) {
      if (!parse_int(s, e, b)) return bad(path, line, "truncated or malformed line");
      if (b < 0 || b > 255) return bad(path, line, "descriptor byte outside 0..255");
      v.desc.push_back((uint8_t)b);
    }
    double w;
    if (!parse_double(s, e, w)) return bad(path, line, "truncated or malformed line (weight)");
    while (s < e && is_blank(*s)) ++s;
    if (s != e) return bad(path, line, "extra tokens");
    ++nchild[(size_t)pid];
    v.parent.push_back((int32_t)pid);
    v.is_leaf.push_back((uint8_t)leaf);
    v.weight.push_back(w);
    v.word_id.push_back(leaf ? words++ : -1);
    nchild.push_back(0);
    depth.push_back(depth[(size_t)pid] + 1);
  }
  v.n_nodes = (int32_t)v.parent.size();
  v.n_words = words;
  for (int32_t i = 0; i < v.n_nodes; ++i)
    if (!v.is_leaf[(size_t)i] && nchild[(size_t)i] == 0)
      return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_load_txt: %s: inner node %d has no children", path, i);
  // positions: a node's children in file order, blocks handed out in node-id order (a parent's id is below its children's, so every
  // block is placed before any of its members is visited -- no breadth-first order of the file is assumed)
  std::vector<int32_t> first(v.n_nodes, -1), fill(v.n_nodes, 0), pos(v.n_nodes, -1);
  int32_t next = 0;
  for (int32_t i = 0; i < v.n_nodes; ++i)
    if (nchild[(size_t)i]) {
      first[(size_t)i] = next;
      next += nchild[(size_t)i];
    }
  for (int32_t i = 1; i < v.n_nodes; ++i) {
    const int32_t par = v.parent[(size_t)i];
    pos[(size_t)i] = first[(size_t)par] + fill[(size_t)par]++;
  }
  v.root_nc = nchild[0];
  v.rec.resize((size_t)std::max(next, 1));
  v.cdesc.assign((size_t)std::max(next, 1) * 32, 0);
  v.cweight.assign((size_t)std::max(next, 1), 0.0);
  for (int32_t i = 1; i < v.n_nodes; ++i) {
    const size_t q = (size_t)pos[(size_t)i];
    v.rec[q] = BowChild{first[(size_t)i], nchild[(size_t)i], v.is_leaf[(size_t)i] ? (uint32_t)v.word_id[(size_t)i] : 0xFFFFFFFFu, (uint32_t)i};
    std::memcpy(&v.cdesc[q * 32], &v.desc[(size_t)i * 32], 32);
    v.cweight[q] = v.weight[(size_t)i];
  }
  return ORBFE_OK;
}

}  // namespace

// the vocabulary's copy on the context's device, made once per device (also asked for by orbfe_trackref.hip)
orbfe_status vocab_on_device(orbfe_ctx* c, const orbfe_vocab* v, BowVocabDev& out) {
  if (c->device < 0 || c->device >= kMaxDevices) return fail(c, ORBFE_EBADARG, "bow: device %d beyond the vocabulary's table", c->device);
  orbfe_vocab::Dev& d = v->dev[c->device];
  if (!d.ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(d.mu);  // one upload per device, whichever contexts ask at once
    if (!d.ready.load(std::memory_order_relaxed)) {
      const size_t np = v->rec.size();
      auto up = [&](void** dst, const void* src, size_t bytes) {
        if (hipMalloc(dst, bytes) != hipSuccess) return false;
        return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
      };
      if (!(up((void**)&d.rec, v->rec.data(), np * sizeof(BowChild)) && up((void**)&d.desc, v->cdesc.data(), np * 32) &&
            up((void**)&d.weight, v->cweight.data(), np * sizeof(double)))) {
        for (void* q : {(void*)d.rec, (void*)d.desc, (void*)d.weight})
          if (q) (void)hipFree(q);
        d.rec = nullptr, d.desc = nullptr, d.weight = nullptr;
        return fail(c, ORBFE_EDEVICE, "bow: upload of the vocabulary (%zu MB) to device %d failed", np * (32 + sizeof(BowChild) + 8) >> 20, c->device);
      }
      d.ready.store(true, std::memory_order_release);
    }
  }
  out = BowVocabDev{d.rec, d.desc, d.weight, 0, v->root_nc, v->L};
  return ORBFE_OK;
}

namespace {

struct BowLayout {
  ScratchRegion up, out;  // the descriptors a caller uploads (empty for slots) | the result block
  size_t o_desc, o_wkey, o_nkey, o_wts;
  size_t o_words, o_values, o_nodes, o_offsets, o_features, o_counts;  // the result block's fields
  size_t np2, total;
};
BowLayout bow_layout(size_t n_img, size_t cap, size_t upload_bytes) {
  BowLayout l;
  for (l.np2 = 1; l.np2 < cap;) l.np2 <<= 1;
  ScratchLayout L;
  l.o_desc = upload_bytes ? L.open(l.up).take(upload_bytes) : 0;
  l.o_wkey = L.close(l.up).take<uint64_t>(n_img * l.np2), l.o_nkey = L.take<uint64_t>(n_img * l.np2), l.o_wts = L.take<double>(n_img * l.np2);
  l.o_values = L.open(l.out).take<double>(n_img * cap), l.o_words = L.take<uint32_t>(n_img * cap), l.o_nodes = L.take<uint32_t>(n_img * cap);
  l.o_features = L.take<uint32_t>(n_img * cap);
  l.o_offsets = L.take<int32_t>(n_img * (cap + 1));  // k_bow's node offsets: cap + 1 per image, the last one the feature count
  l.o_counts = L.take<int32_t>(n_img * 2);
  l.total = L.close(l.out).end();
  return l;
}

// the common tail: launch, one copy of the result block (to `stage_at` in the staging buffer), one synchronisation, the caller's arrays
orbfe_status run_bow(orbfe_ctx* c, StagedIo& io, const BowVocabDev& vd, const uint8_t* d_desc, size_t desc_img_stride, const int32_t* d_counts, int count_step,
                     int n_fixed, int n_img, int cap, int levelsup, const BowLayout& l, size_t stage_at, const orbfe_bow_out* out) {
  launch_bow(c->stream, d_desc, desc_img_stride, d_counts, count_step, n_fixed, n_img, cap, vd, levelsup, io.dev<uint64_t>(l.o_wkey),
             io.dev<uint64_t>(l.o_nkey), io.dev<double>(l.o_wts), l.np2, io.dev<uint32_t>(l.o_words), io.dev<double>(l.o_values),
             io.dev<uint32_t>(l.o_nodes), io.dev<int32_t>(l.o_offsets), io.dev<uint32_t>(l.o_features), io.dev<int32_t>(l.o_counts));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(l.out, stage_at));
  drain_timers(c);
  const size_t cp = std::max(cap, 1);
  for (int i = 0; i < n_img; ++i) {
    int32_t cnt[2];
    io.get(cnt, l.o_counts + 8 * (size_t)i, 8);
    if (cnt[0] < 0 || cnt[0] > cap || cnt[1] < 0 || cnt[1] > cap) return fail(c, ORBFE_EDEVICE, "bow: corrupt counts %d %d", cnt[0], cnt[1]);
    int32_t kept = 0;
    io.get(&kept, l.o_offsets + 4 * ((size_t)i * (cap + 1) + cnt[1]), 4);
    if (kept < 0 || kept > cap) return fail(c, ORBFE_EDEVICE, "bow: corrupt feature count %d", kept);
    const size_t o = (size_t)i * cp;
    if (out->words) io.get(out->words + o, l.o_words + 4 * o, 4 * (size_t)cnt[0]);
    if (out->values) io.get(out->values + o, l.o_values + 8 * o, 8 * (size_t)cnt[0]);
    if (out->n_words) out->n_words[i] = cnt[0];
    if (out->nodes) io.get(out->nodes + o, l.o_nodes + 4 * o, 4 * (size_t)cnt[1]);
    if (out->node_offsets) io.get(out->node_offsets + (size_t)i * (cap + 1), l.o_offsets + 4 * (size_t)i * (cap + 1), 4 * ((size_t)cnt[1] + 1));
    if (out->features) io.get(out->features + o, l.o_features + 4 * o, 4 * (size_t)kept);
    if (out->n_nodes) out->n_nodes[i] = cnt[1];
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_vocab_load_txt(const char* path, orbfe_vocab** out) {
  if (!path || !out) return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_load_txt: NULL argument");
  *out = nullptr;
  std::unique_ptr<orbfe_vocab> v(new (std::nothrow) orbfe_vocab());
  if (!v) return fail(nullptr, ORBFE_ENOMEM, "orbfe_vocab_load_txt: out of memory");
  try {
    TRY(load_txt(path, *v));
  } catch (const std::bad_alloc&) {
    return fail(nullptr, ORBFE_ENOMEM, "orbfe_vocab_load_txt: out of memory");
  }
  *out = v.release();
  return ORBFE_OK;
}

orbfe_status orbfe_vocab_info_get(const orbfe_vocab* v, orbfe_vocab_info* out) {
  if (!v || !out) return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_info_get: NULL argument");
  *out = orbfe_vocab_info{v->k, v->L, v->n_nodes, v->n_words};
  return ORBFE_OK;
}

orbfe_status orbfe_vocab_export(const orbfe_vocab* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int32_t* word_id) {
  if (!v) return fail(nullptr, ORBFE_EBADARG, "orbfe_vocab_export: NULL vocabulary");
  const size_t n = (size_t)v->n_nodes;
  if (parent) std::memcpy(parent, v->parent.data(), 4 * n);
  if (is_leaf) std::memcpy(is_leaf, v->is_leaf.data(), n);
  if (desc) std::memcpy(desc, v->desc.data(), 32 * n);
  if (weight) std::memcpy(weight, v->weight.data(), 8 * n);
  if (word_id) std::memcpy(word_id, v->word_id.data(), 4 * n);
  return ORBFE_OK;
}

void orbfe_vocab_destroy(orbfe_vocab* v) {
  if (!v) return;
  DeviceScope restore;  // the caller's current device, as it was
  for (int d = 0; d < kMaxDevices; ++d) {
    orbfe_vocab::Dev& x = v->dev[d];
    if (!x.rec && !x.desc && !x.weight) continue;
    (void)hipSetDevice(d);  // no call may still use the vocabulary (include/orbfe.h)
    (void)hipFree(x.rec);
    (void)hipFree(x.desc);
    (void)hipFree(x.weight);
  }
  delete v;
}

orbfe_status orbfe_bow_transform(orbfe_ctx* c, const orbfe_vocab* v, const uint8_t* desc, int32_t n, int32_t levelsup, const orbfe_bow_out* out) {
  ApiLock api_lk(c);
  if (!c || !v || !out || n < 0 || levelsup < 0 || (n > 0 && !desc))
    return fail(c, ORBFE_EBADARG, "bow_transform: bad arguments (n %d, levelsup %d)", n, levelsup);
  if (n > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_ECAPACITY, "bow_transform: %d features, at most %d", n, ORBFE_BOW_MAX_FEATURES);
  HIP_TRY(c, hipSetDevice(c->device));
  BowVocabDev vd;
  TRY(vocab_on_device(c, v, vd));
  const BowLayout l = bow_layout(1, (size_t)n, (size_t)n * 32);
  StagedIo io;
  TRY(io.reserve(c, l.total, l.up.end + l.out.bytes()));
  io.put(l.o_desc, desc, (size_t)n * 32);
  if (n) HIP_TRY(c, io.upload(l.up));
  return run_bow(c, io, vd, io.dev<uint8_t>(l.o_desc), 0, nullptr, 1, n, 1, n, levelsup, l, l.up.end, out);
}

orbfe_status orbfe_bow_slots(orbfe_ctx* c, const orbfe_vocab* v, int32_t slot0, int32_t n_slots, int32_t slot_step, int32_t levelsup,
                             const orbfe_bow_out* out) {
  ApiLock api_lk(c);
  if (!c || !v || !out || levelsup < 0 || slot0 < 0 || n_slots < 0 || slot_step < 1 ||
      (n_slots > 0 && (int64_t)slot0 + (int64_t)(n_slots - 1) * slot_step >= c->cfg.max_images))
    return fail(c, ORBFE_EBADARG, "bow_slots: bad arguments (slot0 %d, %d slots, step %d, levelsup %d)", slot0, n_slots, slot_step, levelsup);
  if (n_slots == 0) return ORBFE_OK;
  if (c->cfg.n_features > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_ECAPACITY, "bow_slots: capacity %d above %d", c->cfg.n_features, ORBFE_BOW_MAX_FEATURES);
  TRY(slots_idle(c, slot0, (n_slots - 1) * slot_step + 1, "bow_slots"));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  BowVocabDev vd;
  TRY(vocab_on_device(c, v, vd));
  const int NF = c->cfg.n_features;
  const BowLayout l = bow_layout((size_t)n_slots, (size_t)NF, 0);
  StagedIo io;
  TRY(io.reserve(c, l.total, l.out.bytes()));
  return run_bow(c, io, vd, c->d_desc + (size_t)slot0 * NF * 32, (size_t)NF * slot_step, c->d_n_kp + slot0, slot_step, 0, n_slots, NF, levelsup, l, 0,
                 out);
}

}  // extern "C"
