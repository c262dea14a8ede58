// test_scratch_layout.cpp -- csrc/scratch_layout.h, csrc/search_area_layout.h and the layout part of csrc/pose_call.h, host only (no HIP
// header, no device): the padding rule, regions, that a reservation sized from the guided search's layout is exactly what the search
// takes, the grid build's LDS rule, and the pose-only workspace of the tracking calls.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../orb_slam2_ros2_amd/csrc/pose_call.h"
#include "../../orb_slam2_ros2_amd/csrc/search_area_layout.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static size_t padded(size_t bytes) { return ((bytes < 8 ? 8 : bytes) + 255) & ~(size_t)255; }

int main() {
  // offsets are multiples of 256, consecutive takes do not overlap, an empty take still advances
  {
    ScratchLayout L;
    size_t prev_end = 0;
    for (size_t bytes : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)255, (size_t)256, (size_t)257, (size_t)100000}) {
      const size_t o = L.take(bytes);
      CHECK(o % 256 == 0);
      CHECK(o == prev_end);                 // contiguous: no hole, no overlap
      CHECK(L.end() >= o + bytes);          // the array fits
      CHECK(L.end() > o);                   // take(0) advances too
      CHECK(L.end() == o + padded(bytes));  // the one padding rule
      prev_end = L.end();
    }
  }
  // a layout started at a non-zero offset continues from there
  {
    ScratchLayout L(1024);
    CHECK(L.end() == 1024);
    CHECK(L.take(10) == 1024);
    CHECK(L.take(10) == 1280);
    CHECK(L.end() == 1536);
  }
  // the typed take equals the byte take
  {
    ScratchLayout A, B;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65}) {
      CHECK(A.take<int32_t>(n) == B.take(n * 4));
      CHECK(A.take<double>(n) == B.take(n * 8));
      CHECK(A.take<uint8_t>(n) == B.take(n));
      CHECK(A.end() == B.end());
    }
  }
  // a region's begin and end enclose exactly its takes
  {
    ScratchLayout L;
    ScratchRegion r, empty;
    const size_t before = L.take(300);
    L.open(r);
    const size_t first = L.take(1), last = L.take(600);
    L.close(r);
    const size_t after = L.take(5);
    CHECK(before + padded(300) == r.begin);
    CHECK(r.begin == first && r.end == last + padded(600) && r.end == after);
    CHECK(r.bytes() == padded(1) + padded(600));
    CHECK(r.upto(last).begin == r.begin && r.upto(last).bytes() == padded(1));
    L.open(empty);
    L.close(empty);
    CHECK(empty.bytes() == 0 && empty.begin == L.end());
  }
  // the guided search: end() is reached exactly by the takes the search performs, behind any prefix, with and without frame bounds
  {
    const float bounds[4] = {-20.5f, 1260.25f, -12.f, 390.5f};
    const float bad[4] = {10.f, 5.f, 0.f, 100.f};
    AreaGrid ag = {0, 0, 0, 0};
    CHECK(!area_grid(1241, 376, bad, &ag));
    for (const float* b : {(const float*)nullptr, (const float*)bounds})
      for (size_t nq : {(size_t)0, (size_t)1, (size_t)1000})
        for (size_t nt : {(size_t)0, (size_t)1, (size_t)2000})
          for (size_t start : {(size_t)0, (size_t)4096}) {
            CHECK(area_grid(1241, 376, b, &ag));
            if (!b) CHECK(ag.rows == 8 && ag.cols == 20 && ag.clip_w == 1241 && ag.clip_h == 376);
            else CHECK(ag.rows == 9 && ag.cols == 21 && ag.clip_w == 1260 && ag.clip_h == 390);
            const size_t ncells = (size_t)ag.rows * ag.cols;
            const SearchAreaLayout l = search_area_layout(start, ag, nt, nq);
            const size_t in_bytes = padded(nq * 8) + padded(nq * 4) + 2 * padded(nq) + padded(nq * 32) + padded(nt);
            const size_t grid_bytes = padded((ncells + 1) * 4) + padded(nt * 4);
            const size_t out_bytes = 4 * padded(nq * 4) + padded(nt * 4);
            CHECK(l.in.begin == start && l.o_q == start && l.in.bytes() == in_bytes);
            CHECK(l.o_co == l.in.end && l.out.begin == l.in.end + grid_bytes && l.o_bi == l.out.begin);
            CHECK(l.out.bytes() == out_bytes && l.out.end == l.end());
            CHECK(l.end() == start + in_bytes + grid_bytes + out_bytes);
            CHECK(l.o_eh + padded(nt * 4) == l.end());  // the last array ends where the reservation ends
            const size_t offs[] = {l.o_q, l.o_r, l.o_lo, l.o_hi, l.o_d, l.o_ex, l.o_co, l.o_cf, l.o_bi, l.o_bd, l.o_sd, l.o_nc, l.o_eh, l.end()};
            for (size_t i = 0; i + 1 < sizeof offs / sizeof offs[0]; ++i) CHECK(offs[i] % 256 == 0 && offs[i] < offs[i + 1]);
          }
  }
  // the grid build's LDS rule: counters (2 ncells + 1) words, lists 2 n words; lists in LDS up to 56 KB in all, counters over 60 KB refused.
  // Both sums are 4 mod 8 bytes, so neither limit is met exactly by any (ncells, n): the cases are the nearest sizes on either side.
  {
    const size_t KB56 = 56 * 1024, KB60 = 60 * 1024;
    for (size_t ncells : {(size_t)1, (size_t)160, (size_t)189, (size_t)7000})
      for (size_t n : {(size_t)0, (size_t)1, (size_t)2000, (size_t)7167, (size_t)8000}) {
        const AreaGridLds g = area_grid_lds(ncells, n);
        const size_t counters = (2 * ncells + 1) * 4, all = counters + n * 8;
        CHECK(all % 8 == 4 && counters % 8 == 4);
        CHECK(!g.refused);
        CHECK(g.in_lds == (all <= KB56 ? 1 : 0));
        CHECK(g.bytes == (g.in_lds ? all : counters));
      }
    // 56 KB: ncells + n = 7167 is 4 bytes under it (the most that fits), one feature or one cell more is 4 bytes over
    const AreaGridLds fit = area_grid_lds(160, 7007), over_n = area_grid_lds(160, 7008), over_c = area_grid_lds(161, 7007);
    CHECK(fit.in_lds == 1 && fit.bytes == KB56 - 4 && !fit.refused);
    CHECK(over_n.in_lds == 0 && over_n.bytes == (2 * 160 + 1) * 4 && !over_n.refused);
    CHECK(over_c.in_lds == 0 && over_c.bytes == (2 * 161 + 1) * 4 && !over_c.refused);
    // 60 KB of counters: 7679 cells are 4 bytes under it (the largest grid accepted), one cell more is refused, whatever n is
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2000}) {
      const AreaGridLds last = area_grid_lds(7679, n), refused = area_grid_lds(7680, n);
      CHECK(!last.refused && last.in_lds == 0 && last.bytes == KB60 - 4);
      CHECK(refused.refused);
    }
    // n = 0: the counters alone, in LDS while they fit 56 KB
    CHECK(area_grid_lds(160, 0).in_lds == 1 && area_grid_lds(160, 0).bytes == 1284 && !area_grid_lds(160, 0).refused);
    CHECK(area_grid_lds(7167, 0).in_lds == 1 && area_grid_lds(7167, 0).bytes == KB56 - 4);
    CHECK(area_grid_lds(7168, 0).in_lds == 0 && area_grid_lds(7168, 0).bytes == KB56 + 4);
  }
  // the pose-only workspace (pose_call.h) for one and two optimisations: its three takes, each inside a region of the caller's with a
  // take of the caller's own between them -- every field inside its region, aligned by the one padding rule, disjoint from the others;
  // p_init and p_opt hold k * 7 doubles
  for (size_t k : {(size_t)1, (size_t)2})
    for (size_t nf : {(size_t)1, (size_t)500, (size_t)2048}) {
      ScratchLayout L(512);
      ScratchRegion seed, list, results;
      PoseWorkspace W(nf, k);
      FrameUpload U;
      const size_t own0 = L.take(24);
      const size_t own1 = W.take_seed(L.open(seed)).close(seed).take(24);
      const size_t own2 = W.take_list(L.open(list)).close(list).take(24);
      const size_t own3 = U.take(W.take_results(L.open(results)).close(results), nf, 8).take(24);
      CHECK(W.NF == nf && W.k == k);
      struct Field {
        size_t off, bytes;
        const ScratchRegion* in;
      };
      const ScratchRegion whole = {own0, L.end()};
      const Field fields[] = {{own0, 24, &whole},          {W.o_p0, k * 7 * 8, &seed},   {own1, 24, &whole},         {W.o_xw, nf * 24, &list},
                              {W.o_ms, nf * 24, &list},    {W.o_info, nf * 8, &list},    {W.o_sig, nf * 4, &list},   {own2, 24, &whole},
                              {W.o_p1, k * 7 * 8, &results}, {W.o_ng, 8, &results},      {W.o_eo, nf * 4, &results}, {W.o_ei, nf, &results},
                              {U.o_ru, nf * 8, &whole},    {U.o_s2, 8 * 4, &whole},      {U.o_is2, 8 * 4, &whole},   {own3, 24, &whole}};
      size_t prev_end = 512;
      for (const Field& f : fields) {  // (in take order: each starts where the one before it ends, padding included)
        CHECK(f.off % 256 == 0);
        CHECK(f.off == prev_end);
        CHECK(f.off >= f.in->begin && f.off + f.bytes <= f.in->end);
        prev_end = f.off + padded(f.bytes);
      }
      CHECK(prev_end == L.end());
      CHECK(seed.bytes() == padded(k * 56) && list.bytes() == 2 * padded(nf * 24) + padded(nf * 8) + padded(nf * 4));
      CHECK(results.bytes() == padded(k * 56) + padded(8) + padded(nf * 4) + padded(nf));
    }
  if (failures) return 1;
  std::printf("SCRATCH_LAYOUT_OK\n");
  return 0;
}
