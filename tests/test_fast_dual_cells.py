"""k_fast's dual-polarity bookkeeping on hand-built cells, against the oracle's per-cell FAST.

A pixel is DUAL when FAST's necessary test (the four opposite ring pairs 0/8, 2/10, 4/12, 6/14) passes for both polarities.  k_fast
lists it as dark, tags the entry in a wave-uniform branch of the test trip and raises a per-cell flag; the scoring loop runs its
second-polarity part (the back list, its overflow rescan, V = max(A, B)) only behind that flag.  On ordinary frames about one cell in a
hundred holds such a pixel, so these cells are built by hand: every case states on the CPU (a numpy restatement of the test and of the
arc scores, no GPU needed) what its image holds, and the device's candidate lists must equal the oracle's on every level.

Geometry (orbfe_create: region = size - 32, 30-px grid, the last column / row of cells clipped to the region):
  * 92 x 92 is the smallest context with 2 x 2 cells on level 0: interiors 30 and 24 wide / high, level 1 one cell of 39 x 39.
  * Its interiors are even and at most 30 wide, so it has no leftover row (the rows are dealt out evenly to the row groups, ih mod rpi of
    them take a trip of their own) and lane 63 never holds a pixel: the geometry edges use 96 x 94 (cell (0, 0): 32 x 31 interior pixels,
    two row groups of 15 rows, row 30 left over, lane 63 = column 31 of the second group).
  * A cell wider than 32 interior columns is walked 64 columns at a time with one row group (the grid never makes a cell of more than
    59 interior columns, so a second column block does not occur): 110 x 122, interiors 39 and 33 wide.  With 6 + 4 cells it is also
    the smallest two-level context in which ORBFE_FAST_CPW=2 makes a wave loop (a launch has at least eight waves: cells 8 and 9 are
    second cells), and the one whose level-0 cell is nearly the launch's largest, so that its back list can overflow.
  * "Both polarities are corners" cannot be built: a dark corner needs 9 contiguous ring pixels below v - t, a bright one 9 above
    v + t, and the ring has 16.  What V = max(A, B) has to get right is the dual pixel whose listed (dark) polarity is no corner and
    whose bright one is (V = B, A <= t), next to the reverse; `both` builds those at several strengths."""
import numpy as np
import pytest

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
        (-1, 3)]  # (dx, dy), cv::FAST's circle of 16
T_HI, T_LO = 20, 7


# ---- numpy restatement (arrays are indexed [y - 3, x - 3]) ------------------------------------------------------------------------
def _ring(img):
    im = img.astype(np.int32)
    h, w = im.shape
    return np.stack([im[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING]), im[3:h - 3, 3:w - 3]


def necessary(img, t):
    """(bright passes, dark passes) of the 9-read necessary test"""
    r, v = _ring(img)
    hi = np.stack([np.maximum(r[k], r[k + 8]) for k in (0, 2, 4, 6)])
    lo = np.stack([np.minimum(r[k], r[k + 8]) for k in (0, 2, 4, 6)])
    return hi.min(0) - v > t, v - lo.max(0) > t


def arc_scores(img):
    """A (dark ring) and B (bright ring): max over the 16 arcs of 9 of the smallest margin"""
    r, v = _ring(img)
    d = v[None] - r
    a = np.max(np.stack([np.min(np.stack([d[(k + j) % 16] for j in range(9)]), 0) for k in range(16)]), 0)
    b = np.max(np.stack([np.min(np.stack([-d[(k + j) % 16] for j in range(9)]), 0) for k in range(16)]), 0)
    return a, b


def level0_cells(w, h):
    """{(row, col): (x0, y0, pw, ph)} as orbfe_create lays them out"""
    def axis(n):
        reg = n - 32
        k = reg // 30
        c = reg // k
        out = []
        for j in range(k):
            ini = 16 + j * c
            if ini >= n - 16 - 6:
                continue
            out.append((ini, min(ini + c + 6, n - 16) - ini))
        return out
    return {(i, j): (x0, y0, pw, ph) for i, (y0, ph) in enumerate(axis(h)) for j, (x0, pw) in enumerate(axis(w))}


def interior(arr, cell):
    x0, y0, pw, ph = cell
    return arr[y0:y0 + ph - 6, x0:x0 + pw - 6]


def q_cap(w, h, scale=1.2):
    """entries of k_fast's queue in the one launch of a two-level context (fast_lds_layout over the launch's largest patch)"""
    w1, h1 = int(np.rint(np.float32(w) / np.float32(scale))), int(np.rint(np.float32(h) / np.float32(scale)))
    cells = list(level0_cells(w, h).values()) + list(level0_cells(w1, h1).values())
    mpw, mph = max(c[2] for c in cells), max(c[3] for c in cells)
    return ((2 * (mpw - 6) * (mph - 6) + 15) & ~15) // 2


def stamp(img, x, y, kind, up=60, down=60):
    """a dual pixel at (x, y) of a flat image: ring 1..9 brighter and 10..16 darker (`bright`: a bright corner whose even pairs all hold
    one darker pixel), the reverse (`dark`), or only the eight even ring pixels set (`none`: dual, no corner of either polarity)"""
    v = int(img[y, x])
    for k, (dx, dy) in enumerate(RING):
        if kind == "none":
            if k % 2 == 0:
                img[y + dy, x + dx] = v + up if k < 8 else v - down
        else:
            first = 1 <= k <= 9
            img[y + dy, x + dx] = (v + up if first else v - down) if kind == "bright" else (v - down if first else v + up)


# ---- the cases: (width, height, image, check(img) run on the CPU) ------------------------------------------------------------------
def _flat(w, h):
    return np.full((h, w), 128, np.uint8)


def case_one_polarity():
    """(a) dual pixels whose dark polarity alone is a corner, whose bright one alone is, and with no corner at all"""
    w = h = 92
    img = _flat(w, h)
    pts = [(24, 24, "dark"), (36, 24, "bright"), (24, 36, "none"), (40, 40, "bright"), (60, 26, "dark"), (26, 60, "bright"), (62, 62, "none")]
    for x, y, k in pts:
        stamp(img, x, y, k)

    def check(im):
        nb, nd = necessary(im, T_HI)
        a, b = arc_scores(im)
        for x, y, k in pts:
            assert nb[y - 3, x - 3] and nd[y - 3, x - 3], (x, y)
            assert (a[y - 3, x - 3] > T_HI) == (k == "dark") and (b[y - 3, x - 3] > T_HI) == (k == "bright"), (x, y, k)
        cells = level0_cells(w, h)
        assert len(cells) == 4 and all(interior(nb & nd, c).any() for c in cells.values())
    return w, h, img, check


def case_both():
    """(b) V = max(A, B): bright corners of several strengths on dual pixels whose listed dark polarity scores below the threshold,
    two of them neighbours of a dark corner so that the 3 x 3 maximum is taken between scores of both polarities"""
    w = h = 92
    img = _flat(w, h)
    pts = [(24, 24, "bright", 30, 25), (38, 24, "bright", 100, 25), (24, 38, "dark", 90, 30), (40, 42, "bright", 45, 110)]
    for x, y, k, up, down in pts:
        stamp(img, x, y, k, up, down)
    img[43, 41] = 255  # a lone bright dot beside the last one: a dark corner (score 127) next to a dual bright corner
    stamp(img, 60, 60, "bright", 70, 70)
    img[60, 61] = 128 - 90  # the dual pixel's right neighbour far below its ring: a bright corner beside it

    def check(im):
        nb, nd = necessary(im, T_HI)
        a, b = arc_scores(im)
        for x, y, k, up, down in pts:
            assert nb[y - 3, x - 3] and nd[y - 3, x - 3]
            big, small = (b, a) if k == "bright" else (a, b)
            assert big[y - 3, x - 3] > T_HI >= small[y - 3, x - 3]
        assert (nb & nd)[57, 57] and b[57, 57] > T_HI
    return w, h, img, check


def case_edges():
    """(c) cell (0, 0) of 96 x 94: 32 x 31 interior pixels from (19, 19), row groups 0 .. 14 and 15 .. 29, row 30 in the leftover trip.
    Dual pixels in lane 0 and lane 63 of a trip, in the first and the last interior column, in the first rows of both row groups, in the
    leftover row (whose unused lanes sit on row 31, outside the interior, where the row-1 cell has a dual pixel)"""
    w, h = 96, 94
    img = _flat(w, h)
    pts = [(19, 19, "bright"), (50, 35, "dark"), (19, 34, "bright"), (50, 49, "bright"), (34, 49, "dark"), (50, 19, "none"), (34, 34, "bright"),
           (26, 50, "bright"), (50, 58, "dark"), (72, 34, "bright"), (76, 49, "dark")]
    for x, y, k in pts:
        stamp(img, x, y, k)

    def check(im):
        cells = level0_cells(w, h)
        assert cells[(0, 0)] == (16, 16, 38, 37) and cells[(0, 1)][2] - 6 == 26 and cells[(1, 0)][1] + 3 == 50
        nb, nd = necessary(im, T_HI)
        for x, y, k in pts:
            assert nb[y - 3, x - 3] and nd[y - 3, x - 3], (x, y)
    return w, h, img, check


def case_wide():
    """(d) 110 x 122: cells 39 and 33 interior columns wide (64 columns per trip, one row group), dual pixels in their first and last
    columns and rows"""
    w, h = 110, 122
    img = _flat(w, h)
    pts = [(19, 19, "bright"), (57, 19, "dark"), (19, 48, "dark"), (57, 48, "bright"), (40, 33, "none"), (58, 30, "bright"), (90, 19, "dark"),
           (90, 48, "bright"), (70, 40, "dark"), (30, 70, "bright"), (80, 100, "dark")]
    for x, y, k in pts:
        stamp(img, x, y, k)

    def check(im):
        cells = level0_cells(w, h)
        assert len(cells) == 6 and cells[(0, 0)] == (16, 16, 45, 36) and cells[(0, 1)] == (55, 16, 39, 36)
        nb, nd = necessary(im, T_HI)
        for x, y, k in pts:
            assert nb[y - 3, x - 3] and nd[y - 3, x - 3], (x, y)
    return w, h, img, check


def case_overflow():
    """(e) a grey ramp 11 (x + 2 y) mod 256: away from the wrap every even ring pair has one pixel 22 ... 66 above and one as far below
    the centre, near it the pairs are dark or bright on both sides -- every pixel survives, four in ten are dual, and the survivors plus
    the back list exceed the queue in the two 39 x 30 cells of level 0"""
    w, h = 110, 122
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((11 * (xx + 2 * yy)) % 256).astype(np.uint8)
    pts = [(25, 22), (40, 30), (30, 41), (50, 46), (28, 55), (45, 70)]  # bright corners on dual pixels, early and late in the cells' queues
    for x, y in pts:
        img[y, x] = 128
        stamp(img, x, y, "bright")

    def check(im):
        nb, nd = necessary(im, T_HI)
        a, b = arc_scores(im)
        for x, y in pts:
            assert nb[y - 3, x - 3] and nd[y - 3, x - 3] and b[y - 3, x - 3] > T_HI >= a[y - 3, x - 3]
        cap = q_cap(w, h)
        for rc in ((0, 0), (1, 0)):
            c = level0_cells(w, h)[rc]
            surv, dual = int(interior(nb | nd, c).sum()), int(interior(nb & nd, c).sum())
            assert surv + dual > cap and dual > 64, (rc, surv, dual, cap)
    return w, h, img, check


def case_fallback():
    """(f) cell (0, 0) holds nothing at the high threshold and dual pixels at the low one; cell (0, 1) has a corner at the high
    threshold AND weaker dual pixels, which the low threshold must not bring in"""
    w = h = 92
    img = _flat(w, h)
    weak = [(24, 24, "bright"), (38, 30, "dark"), (28, 44, "none"), (44, 44, "bright")]
    for x, y, k in weak:
        stamp(img, x, y, k, 12, 12)
    stamp(img, 60, 24, "bright", 12, 12)
    stamp(img, 62, 40, "dark")

    def check(im):
        cells = level0_cells(w, h)
        a, b = arc_scores(im)
        assert not interior(np.maximum(a, b) > T_HI, cells[(0, 0)]).any() and interior(np.maximum(a, b) > T_LO, cells[(0, 0)]).any()
        assert interior(np.maximum(a, b) > T_HI, cells[(0, 1)]).any()
        nb, nd = necessary(im, T_LO)
        nbh, ndh = necessary(im, T_HI)
        for x, y, k in weak:
            assert nb[y - 3, x - 3] and nd[y - 3, x - 3] and not (nbh[y - 3, x - 3] or ndh[y - 3, x - 3])
    return w, h, img, check


def case_neighbours():
    """(g) level-0 cells with many dual pixels beside cells with corners and no dual pixel at all (lone dots: a centre above its whole
    ring); with ORBFE_FAST_CPW=2 the waves of cells (0, 0) and (0, 1) go on to the level-1 cells 8 and 9, which have none either"""
    w, h = 110, 122
    img = _flat(w, h)
    for y in range(20, 48, 9):
        for x in range(20, 52, 9):
            stamp(img, x, y, ("bright", "dark", "none")[((x - 20) // 9 + 2 * ((y - 20) // 9)) % 3])
    for x, y in ((62, 22), (75, 30), (88, 25), (66, 44), (30, 60), (40, 70), (75, 60), (30, 90), (70, 100), (84, 88)):
        img[y, x] = 230

    def check(im):
        cells = level0_cells(w, h)
        nb, nd = necessary(im, T_HI)
        dual = nb & nd
        assert interior(dual, cells[(0, 0)]).sum() >= 12
        for rc in ((0, 1), (1, 0), (1, 1), (2, 0), (2, 1)):
            assert not interior(dual, cells[rc]).any() and interior(nb | nd, cells[rc]).any()
    return w, h, img, check


CASES = {"one_polarity": case_one_polarity, "both": case_both, "edges": case_edges, "wide": case_wide, "overflow": case_overflow,
         "fallback": case_fallback, "neighbours": case_neighbours}
_reference = {}


def reference(orc, name):
    """the case and the oracle's candidate lists of both levels, computed once and shared by the device runs"""
    if name not in _reference:
        w, h, img, check = CASES[name]()
        ex = orc.extractor(img, n_features=500, n_levels=2, th_hi=T_HI, th_lo=T_LO)
        ex.extract()  # (the candidate lists are a by-product of the extraction)
        _reference[name] = (w, h, img, check, [ex.candidates(l).copy() for l in range(2)])
    return _reference[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_case_holds_what_it_claims(orc, name):
    """CPU only: the dual pixels, corners and counts each case is built for are there, and the oracle finds corners on level 0"""
    w, h, img, check, cand = reference(orc, name)
    assert img.shape == (h, w)
    check(img)
    assert len(cand[0]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cpw,shards", [(None, None), ("2", None), ("2", "1")])
@pytest.mark.parametrize("name", list(CASES))
def test_dual_cells_against_the_oracle(orc, monkeypatch, name, cpw, shards):
    """k_fast's candidates of both levels equal the oracle's: one cell per wave, with ORBFE_FAST_CPW=2 (in the 110 x 122 contexts waves
    0 and 1 then take a second cell), and with one list per level instead of the sharded ones (the other instantiations)."""
    from orb_slam2_ros2_amd import _lib
    w, h, img, check, cand = reference(orc, name)
    if cpw is not None:
        monkeypatch.setenv("ORBFE_FAST_CPW", cpw)
    if shards is not None:
        monkeypatch.setenv("ORBFE_FAST_SHARDS", shards)
    ctx = _lib.Context(w, h, n_features=500, n_levels=2, fast_hi=T_HI, fast_lo=T_LO, max_images=1)
    try:
        ctx.extract(img)
        for l in range(2):
            got = ctx.debug_candidates(0, l)
            assert got.shape == cand[l].shape and np.array_equal(got, cand[l]), f"{name}: level {l} candidates differ ({got.shape} vs {cand[l].shape})"
    finally:
        ctx.close()
