"""k_brief's rolled keypoint loop: a wave works through N keypoints (a kernel argument; ORBFE_BRIEF_KPW, read when the context is
created, forces it), wave w of a block taking keypoints base + w + 4 i, through two window buffers in turn and a three-stage pipeline
(list entry of i + 2, window and sin / cos of i + 1, tests of i).  Every case compares ALL keypoint records and descriptors byte for
byte with the CPU oracle, for N = 1, 2, 3, 8, 16, through the launch of a frame or two (N keypoints forced there as well; the eight
row-table workgroups ride behind the descriptor blocks) and through the batch launch (three or more images: the separate kernels).
What a case is built for is asserted on the CPU, from the oracle's own output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KPWS = [1, 2, 3, 8, 16]
WAVES = 4                      # waves of a descriptor workgroup: wave w takes keypoints base + w + 4 i
FX, BF = 400.0, 200.0


def _noise(w, h, seed, b):
    """block noise (b-pixel blocks at a random phase): corners everywhere, the border included"""
    rng = np.random.default_rng(seed)
    ox, oy = rng.integers(0, b, 2)
    g = rng.integers(0, 256, ((h + 2 * b) // b + 1, (w + 2 * b) // b + 1)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((b, b), np.uint8))[oy:oy + h, ox:ox + w])


def _white(w, h, seed):
    """white noise: corners everywhere, the border included"""
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def _assert_equal(results, refs, what):
    for i, ((kps, desc), (rk, rd)) in enumerate(zip(results, refs)):
        assert len(kps) == len(rk) and np.array_equal(kps, rk), f"{what}: keypoint records of image {i}"
        assert desc.shape == rd.shape and np.array_equal(desc, rd), f"{what}: descriptors of image {i}"


def _wave_of(k, n):
    """(block, wave, step) of list position k with n keypoints a wave"""
    return k // (WAVES * n), k % WAVES, (k % (WAVES * n)) // WAVES


def _run_both_shapes(Context, w, h, nf, nl, imgs, refs, what):
    """imgs[0] alone (the launch of a frame or two), then imgs[0], imgs[1], imgs[0] as a batch (the separate kernels), buffers reused"""
    ctx = Context(w, h, n_features=nf, n_levels=nl, max_images=3)
    try:
        assert ctx.n_features == nf
        _assert_equal([ctx.extract(imgs[0])], refs[:1], what + ", one image")
        _assert_equal(ctx.extract_batch([imgs[0], imgs[1], imgs[0]]), [refs[0], refs[1], refs[0]], what + ", batch of three")
        _assert_equal(ctx.extract_batch([imgs[1], imgs[0]]), [refs[1], refs[0]], what + ", two images")
    finally:
        ctx.close()


# ---- loop ends ----------------------------------------------------------------------------------------------------------------
ENDS_NF = [1, 7, 8, 9, 63, 65, 130]
ENDS_GEOM = (160, 120, 3)


@pytest.fixture(scope="module")
def ends(orc):
    w, h, nl = ENDS_GEOM
    imgs = [_white(w, h, 1), _white(w, h, 2)]
    refs = {nf: [orc.extractor(im, n_features=nf, n_levels=nl).extract() for im in imgs] for nf in ENDS_NF}
    for nf in ENDS_NF:   # rich in corners: every slot of every list is used
        assert all(len(k) == nf for k, _ in refs[nf]), (nf, [len(k) for k, _ in refs[nf]])
    return imgs, refs


@pytest.mark.parametrize("kpw", KPWS)
def test_loop_ends(monkeypatch, ends, kpw):
    """one keypoint in all; a last wave with one keypoint; a last block with idle waves; counts one below / at / one above a block"""
    from orb_slam2_ros2_amd._lib import Context
    monkeypatch.setenv("ORBFE_BRIEF_KPW", str(kpw))
    imgs, refs = ends
    w, h, nl = ENDS_GEOM
    for nf in ENDS_NF:
        _run_both_shapes(Context, w, h, nf, nl, imgs, refs[nf], f"N = {kpw}, {nf} features")


# ---- unused tail --------------------------------------------------------------------------------------------------------------
TAIL_GEOM = (92, 92, 2)
TAIL_NF = 500


@pytest.fixture(scope="module")
def tail(orc):
    w, h, nl = TAIL_GEOM
    imgs = [_white(w, h, 2), _white(w, h, 4)]
    refs = [orc.extractor(im, n_features=TAIL_NF, n_levels=nl).extract() for im in imgs]
    for n in (len(k) for k, _ in refs):
        assert n > 0 and all((n // (WAVES * kpw) + 2) * WAVES * kpw <= TAIL_NF for kpw in KPWS), n   # the image yields fewer: whole blocks without a used slot
        assert any(n % (WAVES * kpw) for kpw in KPWS), n        # ... and a block that straddles the count
        assert n % WAVES, n                                     # ... inside which the waves' own counts differ
    return imgs, refs


@pytest.mark.parametrize("kpw", KPWS)
def test_unused_tail(monkeypatch, tail, kpw):
    """the list is level-major, its unused slots are the tail: waves that straddle the count (the pipeline runs on through skipped
    keypoints: the buffer parity behind one), waves and blocks with no used slot"""
    from orb_slam2_ros2_amd._lib import Context
    monkeypatch.setenv("ORBFE_BRIEF_KPW", str(kpw))
    imgs, refs = tail
    w, h, nl = TAIL_GEOM
    _run_both_shapes(Context, w, h, TAIL_NF, nl, imgs, refs, f"N = {kpw}, unused tail")


# ---- buffer reuse, both call shapes -------------------------------------------------------------------------------------------
SHAPES_GEOM = (160, 120, 3)
SHAPES_NF = 301
N_BATCH = 32


@pytest.fixture(scope="module")
def shapes(orc):
    w, h, nl = SHAPES_GEOM
    imgs = [_noise(w, h, 8300 + i, 3 + i % 4) for i in range(N_BATCH)]
    imgs[5] = np.full((h, w), 90, np.uint8)     # a flat ground: no keypoint at all
    refs = [orc.extractor(im, n_features=SHAPES_NF, n_levels=nl).extract() for im in imgs]
    return imgs, refs


def _holds_level_change_inside_a_wave(kps, n):
    """a wave with three or more used keypoints, two consecutive ones of which (k, k + 4) lie on different levels (other plane, other
    stride) and all of whose windows differ"""
    octv, cnt = kps["octave"], len(kps)
    for k in range(cnt - WAVES):
        b, wv, st = _wave_of(k, n)
        if st + 1 >= n or octv[k] == octv[k + WAVES]:
            continue
        first = b * WAVES * n + wv
        mine = [j for j in range(first, min(first + WAVES * n, cnt), WAVES)]
        pts = {(kps["x"][j], kps["y"][j], octv[j]) for j in mine}
        if len(mine) >= 3 and len(pts) == len(mine):
            return True
    return False


@pytest.mark.parametrize("kpw", KPWS)
def test_buffer_reuse_batch_of_32(monkeypatch, shapes, kpw):
    """the batch shape (the separate kernels): for N >= 3 waves hold three or more used keypoints with different windows, among them
    consecutive ones of different levels -- a window or a table read one keypoint late shows there"""
    from orb_slam2_ros2_amd._lib import Context
    monkeypatch.setenv("ORBFE_BRIEF_KPW", str(kpw))
    imgs, refs = shapes
    w, h, nl = SHAPES_GEOM
    if kpw >= 3:
        assert sum(_holds_level_change_inside_a_wave(k, kpw) for k, _ in refs) >= 8
    assert any(len(k) == SHAPES_NF for k, _ in refs) and any(len(k) == 0 for k, _ in refs)
    ctx = Context(w, h, n_features=SHAPES_NF, n_levels=nl, max_images=N_BATCH)
    try:
        _assert_equal(ctx.extract_batch(imgs), refs, f"N = {kpw}, batch of {N_BATCH}")
    finally:
        ctx.close()


@pytest.mark.parametrize("kpw", KPWS)
def test_one_and_two_image_calls_and_their_row_tables(monkeypatch, orc, shapes, kpw):
    """the fused small path with the row-table workgroups behind the descriptor blocks: features equal the oracle's, and the slot's row
    table is the one k_rowtable builds -- the stereo match that reads it equals the oracle's (as test_stereo_row_table_edge_cases checks)"""
    from orb_slam2_ros2_amd._lib import Context
    monkeypatch.setenv("ORBFE_BRIEF_KPW", str(kpw))
    imgs, refs = shapes
    w, h, nl = SHAPES_GEOM
    left = imgs[0]
    right = np.ascontiguousarray(np.roll(left, -7, axis=1))   # the left image shifted: disparity 7
    exl, exr = orc.extractor(left, n_features=SHAPES_NF, n_levels=nl), orc.extractor(right, n_features=SHAPES_NF, n_levels=nl)
    (okl, odl), (okr, odr) = exl.extract(), exr.extract()
    om, oru, odp, obr, obd = exl.stereo_match(exr, okl, odl, okr, odr, FX, BF)
    assert om > 20
    ctx = Context(w, h, n_features=SHAPES_NF, n_levels=nl, max_images=2)
    try:
        def check(what):
            nm, ru, dp, br, bd = ctx.stereo_match(0, 1, FX, BF)
            n = len(okl)
            assert nm == om, what
            assert np.array_equal(ru[:n].view(np.int64), oru.view(np.int64)) and np.array_equal(dp[:n].view(np.int64), odp.view(np.int64)), what
            assert np.array_equal(br[:n], obr) and np.array_equal(bd[:n], obd), what
        _assert_equal(ctx.extract_batch([left, right]), [(okl, odl), (okr, odr)], f"N = {kpw}, two-image call")
        check("row table of the two-image call")
        _assert_equal([ctx.extract_slot(1, imgs[1])], [refs[1]], f"N = {kpw}, one-image call, another image")   # the slot's table is rewritten
        _assert_equal([ctx.extract_slot(0, left), ctx.extract_slot(1, right)], [(okl, odl), (okr, odr)], f"N = {kpw}, one-image calls")
        check("row table of the one-image call")
    finally:
        ctx.close()


# ---- borders ------------------------------------------------------------------------------------------------------------------
BORDER_GEOMS = [(93, 96, 2), (1241, 160, 3)]    # widths whose row stride is not the width; a few cell rows high (1241 x 96 is refused: 16 root strips at most)
BORDER_NF = [300, 1000]
# how near the oracle's keypoints of level 0 come to (left, right, top, bottom).  19 is the nearest a keypoint may lie.  At 1241 columns
# no keypoint of the oracle comes nearer than 22 to the right border (30 noise images x 3 levels searched, planted corners included:
# the oracle's cell grid of that width ends there), this image's nearest is 34; the 93-column image holds the right border at 19 with
# a stride that is not the width.
BORDER_REACH = [(19, 19, 19, 19), (19, 34, 19, 19)]


@pytest.fixture(scope="module")
def borders(orc):
    out = []
    for (w, h, nl), nf, want in zip(BORDER_GEOMS, BORDER_NF, BORDER_REACH):
        imgs = [_white(w, h, 2), _white(w, h, 6)]
        refs = [orc.extractor(im, n_features=nf, n_levels=nl).extract() for im in imgs]
        kps = refs[0][0]
        m = kps["octave"] == 0          # level 0: level coordinates are the keypoint's own
        x, y = np.rint(kps["x"][m]).astype(int), np.rint(kps["y"][m]).astype(int)
        assert (x.min(), w - 1 - x.max(), y.min(), h - 1 - y.max()) == want, (w, h)
        out.append((imgs, refs))
    return out


@pytest.mark.parametrize("kpw", KPWS)
def test_borders(monkeypatch, borders, kpw):
    """keypoints 19 px from the borders: the 48-byte rows of a window's last row stay inside the plane; strides that are not the width"""
    from orb_slam2_ros2_amd._lib import Context
    monkeypatch.setenv("ORBFE_BRIEF_KPW", str(kpw))
    for (w, h, nl), nf, (imgs, refs) in zip(BORDER_GEOMS, BORDER_NF, borders):
        _run_both_shapes(Context, w, h, nf, nl, imgs, refs, f"N = {kpw}, {w} x {h}")
