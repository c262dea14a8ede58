"""The three ways an image enters the library besides the grey extraction -- colour (k_cvt_gray), the RGB-D tail (k_frame_rgbd) and the
host stream with its records (k_pack_records) -- at the widths, strides and fill states where they can go wrong: every residue of w % 4,
a second and a third workgroup column of the conversion, caller strides above the row, a full slot with a ragged last workgroup, the
`icdist < 0` exit of the undistortion, a captured launch sequence whose key changes, tickets that reuse buffers with fewer pairs.
Every comparison is bit-exact (bytes, integers, un-contracted fp32 / fp64) against the CPU oracle and numpy restatements
(tests/input_shapes.py)."""
import numpy as np
import pytest

import input_shapes as ish
from orb_slam2_ros2_amd import synth

pytestmark = pytest.mark.gpu

FX, BF = 718.856, 386.1448
GEOM = {333: ish.S, 334: ish.S, 335: ish.S, 336: ish.S, 1024: ish.WIDE, 1025: ish.WIDE, 1027: ish.WIDE, 2050: ish.WIDE3}
PAIRS = [(1, 0), (2, 0), (1, 1), (2, 1)]                       # (colour order, grey variant)
COLOR_CASES = [(w, o, v) for w in (333, 1027) for o, v in PAIRS] + [(w, *PAIRS[i % 4]) for i, w in enumerate((334, 335, 336, 1024, 1025, 2050))]


def _context(w, max_images=1, n_features=None, **kw):
    from orb_slam2_ros2_amd._lib import Context
    g = GEOM[w]
    return Context(w, g["h"], n_features=n_features or g["n_features"], n_levels=g["n_levels"], max_images=max_images, **kw)


def _oracle_features(orc, gray, w, n_features=None, levels_that_may_be_empty=()):
    """the oracle extractor's result on `gray`; every level must have keypoints, so that a quiet input cannot pass vacuously"""
    g = GEOM[w]
    k, d = orc.extractor(gray, n_features=n_features or g["n_features"], n_levels=g["n_levels"]).extract()
    per_level = np.bincount(k["octave"], minlength=g["n_levels"])
    assert all(c > 0 for lv, c in enumerate(per_level) if lv not in levels_that_may_be_empty), per_level
    return k, d


def _planes(ctx, slot=0):
    return [ctx.pyramid(slot, lv, blurred) for lv in range(ctx.n_levels) for blurred in (False, True)]


def _depth_images(w, h, dtype, seed):
    """(contiguous depth, the same as a column range of a wider image whose other columns hold another valid depth, scale)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(1, 30000, (h, w)).astype(np.uint16)
    raw[rng.random((h, w)) < 0.2] = 0                                              # holes in the depth map
    depth, scale, other = (raw, 5000.0, 7777) if dtype == np.uint16 else ((raw / np.float32(5000)).astype(np.float32), 1.0, 1.5)
    return depth, scale, other


def _column_range(depth, other, extra=8, x0=3):
    h, w = depth.shape
    big = np.full((h, w + extra), other, depth.dtype)
    big[:, x0:x0 + w] = depth
    view = big[:, x0:x0 + w]
    assert view.strides[0] == (w + extra) * depth.itemsize and not view.flags.c_contiguous
    return view


@pytest.mark.parametrize("w,h,accepted", [(1027, 96, False), (2050, 96, False), (1027, ish.W_H, True), (2050, ish.W3_H, True)])
def test_wide_geometries_and_the_root_strip_limit(w, h, accepted):
    """why the wide images here are 104 and 168 rows high: at 96 rows a level has more than 16 root strips and orbfe_create refuses it"""
    from orb_slam2_ros2_amd._lib import Context, ImageSizeError
    if accepted:
        Context(w, h, n_features=500, n_levels=2, max_images=1).close()
    else:
        with pytest.raises(ImageSizeError, match="root strips"):
            Context(w, h, n_features=500, n_levels=2, max_images=1)


# ---- 1. colour to grey ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,order,variant", COLOR_CASES)
def test_color_conversion_at_every_row_tail_and_workgroup_column(orc, w, order, variant):
    """k_cvt_gray takes four pixels per thread and 1024 per workgroup column and writes whole words: widths with 1..3 leftover pixels, with a
    second and third column, from contiguous rows and from rows 3 w + 5 bytes apart.  Level 0 against the integer formula and the oracle,
    the features against the oracle extractor on that grey image, and every plane of the pyramid against what orbfe_extract of the grey
    image leaves on the same context: what the conversion writes past column w is seen by nothing."""
    h = GEOM[w]["h"]
    f = 2 + (w + order + variant) % 3
    img = ish.color_image(f, w, h)
    strided = ish.padded_rows(img, 5)
    gray = ish.gray_numpy(img, order, variant)
    assert np.array_equal(orc.cvt_gray(img, order, variant), gray)
    assert gray[0, 0] != gray[0, w - 1] and len(set(gray[h - 1, w - 4:].tolist())) == 4       # the marker colours are distinct greys
    ok, od = _oracle_features(orc, gray, w)
    ctx = _context(w, gray_variant=variant)
    try:
        # the staging buffer at its final size, then noise where the staged colour rows have their padding: the bytes behind a row's
        # 3 w are whatever an earlier call left there
        ctx.extract_color(ish.color_image(f + 1, w, h), order)
        ctx.extract(np.random.default_rng(w).integers(0, 256, (h, w)).astype(np.uint8))
        seen = []
        for name, src in (("contiguous", img), ("rows 3w+5 apart", strided)):
            k, d = ctx.extract_color(src, order)
            assert np.array_equal(ctx.pyramid(0, 0, False), gray), name
            ish.assert_keypoints_equal(k, ok)
            assert np.array_equal(d, od), name
            seen.append(_planes(ctx))
        k, d = ctx.extract(gray)
        ish.assert_keypoints_equal(k, ok)
        want = _planes(ctx)
        for planes in seen:
            assert len(planes) == 2 * GEOM[w]["n_levels"] and all(np.array_equal(a, b) for a, b in zip(planes, want))
    finally:
        ctx.close()


# ---- 2. the RGB-D tail ---------------------------------------------------------------------------------------------------------------
_FEATURES = {}


def _gray_features(orc, w, n_features):
    """(grey image, oracle keypoints, oracle descriptors) of a geometry: computed once, shared, never written"""
    key = (w, n_features)
    if key not in _FEATURES:
        gray = synth.mono_image(2 + w % 3, w, GEOM[w]["h"], n_rect=ish.N_RECT)
        # (a level either fills its quota or, by the quota rule test_sparse_image_levels_... pins, stays empty: the one geometry with fewer
        #  keypoints than n_features -- 335 at 2000: level 0 is empty, 1356 keypoints -- is there for the -1 tail alone)
        k, d = _oracle_features(orc, gray, w, n_features, levels_that_may_be_empty=(0,) if n_features == 2000 else ())
        for a in (gray, k, d):
            a.setflags(write=False)
        _FEATURES[key] = (gray, k, d)
    return _FEATURES[key]


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("w,n_features", [(333, 300), (335, 300), (333, 1000), (335, 1000), (1027, 500), (335, 2000)])
def test_rgbd_tail_full_slot_strided_depth_and_every_undistortion_exit(orc, w, n_features, depth_dtype):
    """k_frame_rgbd with a slot that is full (n == n_features: no -1 tail, 300 = 256 + 44 lanes) and one that is not (335 at 2000: 1356 =
    5 * 256 + 76 keypoints, then 644 entries of -1; at 1000 these images fill the slot as well: 322 / 268 / 223 / 187); four cameras -- TUM's
    coefficients, k1 == 0 with the other four set (keypoints keep their bytes, depth still looked up), k1 = -4 and -8 (at least 10
    keypoints leave the five iterations through `icdist < 0`, counted with the numpy restatement); depth contiguous and as a column
    range of a wider image; a float image holding NaN, +inf, -1, 0 and 1e-30 under keypoints.  Through orbfe_frame_rgbd after an
    extraction and through orbfe_frame_rgbd_image, against orc.undistort_points and orc.rgbd_lookup, bit for bit."""
    h = GEOM[w]["h"]
    gray, ok, od = _gray_features(orc, w, n_features)
    n = len(ok)
    xy = np.stack([ok["x"], ok["y"]], 1)
    depth, scale, other = _depth_images(w, h, depth_dtype, 9 + w)
    specials = []
    if depth_dtype == np.float32:
        depth = depth.copy()
        vals = np.array([np.nan, np.inf, -1.0, 0.0, 1e-30], np.float32)
        for i in range(40):                                      # from the extracted (int)x, (int)y: the pixel the lookup reads
            depth[int(ok["y"][i * 7 % n]), int(ok["x"][i * 7 % n])] = vals[i % 5]
        specials = [i * 7 % n for i in range(40)]
    layouts = {"contiguous": depth, "column range": _column_range(depth, other)}
    ctx = _context(w, n_features=n_features)
    report = []
    try:
        nf = ctx.n_features
        assert 0 < n <= nf
        if n_features in (300, 500):
            assert n == nf                                         # a full slot: no lane takes the `i >= n` branch
        if n_features == 2000:
            assert n < nf and n % 256 and (nf - n) > 256           # a -1 tail that starts inside a workgroup and spans whole ones
        for cam_name, cam in ish.cameras(w, h).items():
            K, D = ish.cam_arrays(cam)
            xyu = orc.undistort_points(xy, K, D)
            und_np, n_exit = ish.undistort_numpy(xy, cam)
            assert np.array_equal(xyu.view(np.int32), und_np.view(np.int32))
            if cam_name.startswith("k1_-"):
                assert 10 <= n_exit < n, (cam_name, n_exit)
                report.append(f"{cam_name}: {n_exit} of {n} through icdist < 0")
            if cam_name == "k1_zero":
                assert np.array_equal(xyu.view(np.int32), xy.view(np.int32))
            else:
                assert (xyu != xy).any()
            wd, wru = orc.rgbd_lookup(xy, xyu, depth, scale, cam["bf"])
            assert (wd > 0).sum() > 0.5 * n and (wd < 0).sum() > 0.1 * n
            if specials:                                           # NaN, -1 and 0 are "no depth"; +inf and 1e-30 are depths
                assert (wd[specials] == -1).any() and np.isinf(wd[specials]).any() and (wru[specials] < -1e30).any()
            for lay_name, dimg in layouts.items():
                for entry in ("frame_rgbd", "frame_rgbd_image"):
                    if entry == "frame_rgbd":
                        k, d = ctx.extract(gray)
                        ish.assert_keypoints_equal(k, ok)
                        ku, dd, ru = ctx.frame_rgbd(0, cam, dimg, scale)
                    else:
                        ku, d, dd, ru = ctx.frame_rgbd_image(gray, cam, dimg, scale, 0)
                        assert len(ku) == n
                    what = (cam_name, lay_name, entry)
                    assert np.array_equal(d, od), what
                    assert np.array_equal(np.stack([ku["x"][:n], ku["y"][:n]], 1).view(np.int32), xyu.view(np.int32)), what
                    for fld in ("size", "angle", "response", "octave", "class_id"):
                        assert np.array_equal(ku[fld][:n].view(np.int32), ok[fld].view(np.int32)), what + (fld,)
                    assert dd.shape == (nf,) and ru.shape == (nf,)
                    assert np.array_equal(np.isnan(dd[:n]), np.isnan(wd)) and np.array_equal(np.isnan(ru[:n]), np.isnan(wru)), what
                    assert np.array_equal(dd[:n].view(np.int64), wd.view(np.int64)), what
                    assert np.array_equal(ru[:n].view(np.int64), wru.view(np.int64)), what
                    assert (dd[n:] == -1).all() and (ru[n:] == -1).all(), what
                    k2, _ = ctx.fetch_features(0)                  # undistorted in place on the device
                    assert k2.tobytes() == ku[:n].tobytes(), what
        print(f"w {w} n_features {n_features} {np.dtype(depth_dtype).name}: {n} keypoints; " + "; ".join(report))
    finally:
        ctx.close()


# ---- 3. one call against two, and the key of the captured sequence -----------------------------------------------------------------------
@pytest.mark.parametrize("w", [334, 1025])
def test_one_call_rgbd_frame_equals_the_two_calls(orc, w):
    """orbfe_frame_rgbd_image against orbfe_extract_color / orbfe_extract followed by orbfe_frame_rgbd (as tests/test_frame_glue.py at
    640 x 480), repeated with changing images on both slots so that the captured sequences are replayed"""
    h = GEOM[w]["h"]
    cam = ish.cameras(w, h)["tum"]
    ctx, ref = _context(w, max_images=2), _context(w, max_images=1)
    try:
        for color_order, depth_dtype in ((0, np.uint16), (2, np.uint16), (1, np.float32), (0, None)):
            for rep, f in enumerate((2, 2, 3, 4)):
                img = synth.mono_image(f, w, h, n_rect=ish.N_RECT) if color_order == 0 else ish.color_image(f, w, h)
                depth, scale = None, 1.0
                if depth_dtype is not None:
                    depth, scale, other = _depth_images(w, h, depth_dtype, 11 + rep)
                    if rep & 1:
                        depth = _column_range(depth, other)
                slot = rep & 1
                ku, d, dd, ru = ctx.frame_rgbd_image(img, cam, depth, scale, color_order, slot=slot)
                k0, d0 = ref.extract_color(img, color_order) if color_order else ref.extract(img)
                ku0, dd0, ru0 = ref.frame_rgbd(0, cam, depth, scale)
                n = len(k0)
                what = (color_order, depth_dtype, rep)
                assert len(ku) == n and np.array_equal(d, d0), what
                assert ku.tobytes() == ku0[:n].tobytes(), what
                assert np.array_equal(dd.view(np.int64), dd0.view(np.int64)) and np.array_equal(ru.view(np.int64), ru0.view(np.int64)), what
                if color_order == 0:
                    ok, od = _oracle_features(orc, img, w)
                    assert n == len(ok) and np.array_equal(d, od), what
                assert all(np.array_equal(a, b) for a, b in zip(_planes(ctx, slot), _planes(ref, 0))), what
    finally:
        ctx.close(), ref.close()


def test_captured_sequence_follows_every_field_of_its_key(orc):
    """extract_lane keys the captured launch sequence of orbfe_frame_rgbd_image on colour order, depth type, depth stride, depth scale and
    camera.  On one context, per slot: A, B, A, C, A, D, A, E, A, F, A, where B..F differ from A in exactly one of those fields.  Every
    result equals the same request on a fresh context, byte for byte: a sequence replayed under a stale key would not."""
    w = 333
    h = GEOM[w]["h"]
    img = ish.color_image(3, w, h)
    ok, _ = _oracle_features(orc, ish.gray_numpy(img, 1, 0), w)
    raw, scale, _ = _depth_images(w, h, np.uint16, 5)
    # A's rows are 4 w bytes apart, so that a float image of the same stride exists (C)
    d_a = _column_range(raw, 7777, extra=w, x0=0)
    d_b = _column_range(raw, 7777, extra=w + 8, x0=3)                            # B: another stride
    d_c = raw.astype(np.float32)                                                 # C: another type, the same stride
    assert d_a.strides[0] == d_c.strides[0] == 4 * w and d_b.strides[0] == 4 * w + 16
    cam = ish.cameras(w, h)["tum"]
    req = {"A": (img, cam, d_a, scale, 1), "B": (img, cam, d_b, scale, 1), "C": (img, cam, d_c, scale, 1),
           "D": (img, cam, d_a, 1000.0, 1),                                      # D: another depth scale
           "E": (img, dict(cam, k1=0.1), d_a, scale, 1),                         # E: another k1
           "F": (img, cam, d_a, scale, 2)}                                       # F: another colour order
    want = {}
    for name, r in req.items():
        fresh = _context(w, max_images=1)
        try:
            ku, d, dd, ru = fresh.frame_rgbd_image(*r)
            want[name] = (ku.tobytes(), d.tobytes(), dd.tobytes(), ru.tobytes())
        finally:
            fresh.close()
    assert len(ok) * 28 == len(want["A"][0])
    # the requests are told apart by their results (B and C read the same values through another layout: theirs equal A's)
    assert want["B"] == want["A"] and want["C"] == want["A"]
    assert len({want[q] for q in "ADEF"}) == 4
    ctx = _context(w, max_images=2)
    try:
        for slot in (0, 1):
            for step, name in enumerate("ABACADAEAFA"):
                ku, d, dd, ru = ctx.frame_rgbd_image(*req[name], slot=slot)
                assert (ku.tobytes(), d.tobytes(), dd.tobytes(), ru.tobytes()) == want[name], (slot, step, name)
    finally:
        ctx.close()


# ---- 4. the host stream and its records ------------------------------------------------------------------------------------------------
_STEREO = {}


def _stereo_reference(orc, ref_ctx, w, h, key, L, R):
    """(device results on contiguous copies on a second context == the oracle's), once per pair content"""
    if (w, key) not in _STEREO:
        (lk, ld), (rk, rd) = ref_ctx.extract_batch([np.ascontiguousarray(L), np.ascontiguousarray(R)])
        nm, ru, dp, _, _ = ref_ctx.stereo_match(0, 1, FX, BF)
        o = orc.stereo_frame(L, R, n_features=300, n_levels=4, fx=FX, bf=BF)
        nl = len(o["lk"])
        assert lk.tobytes() == o["lk"].tobytes() and rk.tobytes() == o["rk"].tobytes() and np.array_equal(ld, o["ld"]) and np.array_equal(rd, o["rd"])
        assert nm == o["n_matches"] and np.array_equal(ru[:nl].view(np.int64), o["right_u"].view(np.int64))
        assert np.array_equal(dp[:nl].view(np.int64), o["depth"].view(np.int64))
        _STEREO[(w, key)] = dict(lk=lk, ld=ld, rk=rk, rd=rd, nm=nm, ru=ru, dp=dp)
    return _STEREO[(w, key)]


def _record(nf, lk, ld, ru, dp, nm):
    """the documented record: int32 count | int32 n_matches | 8 zero bytes | keypoints [nf x 28] | descriptors [nf x 32] | right_u [nf] f64 |
    depth [nf] f64, every entry past the count zero"""
    n = len(lk)
    rec = np.zeros(16 + nf * 76, np.uint8)
    rec[0:8] = np.array([n, nm], np.int32).view(np.uint8)
    o = 16
    for a, size in ((lk, 28), (ld, 32), (ru[:n], 8), (dp[:n], 8)):
        b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)
        assert len(b) == n * size
        rec[o:o + len(b)] = b
        o += nf * size
    assert o == len(rec)
    return rec


@pytest.mark.parametrize("w,stride,pinned", [(333, 352, True), (333, 352, False), (335, 340, True), (335, 340, False)])
def test_stream_with_strides_pitch_blank_images_and_shrinking_tickets(orc, w, stride, pinned):
    """orbfe_stream_submit / _wait / _pack_records with stride > width, image_pitch > stride * height (the unused bytes 0xA5), n_features 300:
    five tickets of 3, 3, 3, 3 and 1 pairs, so that every buffer set is reused and the last ticket has fewer pairs than the one before
    it in its buffers; each 3-pair ticket holds a pair with a blank left and one with a blank right image.  Host results against
    extract_batch + stereo_match on a second context and against orc.stereo_frame; the records against the documented layout."""
    import torch
    from orb_slam2_ros2_amd._lib import PinnedArray
    h, nf = ish.S_H, 300
    pitch = stride * h + 640
    frames = {f: synth.stereo_pair(f, w, h, n_rect=ish.N_RECT) for f in (2, 3, 4)}
    blank = np.full((h, w), 96, np.uint8)
    tickets_pairs = []                                             # per ticket: [(key, L, R)]
    for k, n_pairs in enumerate((3, 3, 3, 3, 1)):
        f = 2 + k % 3
        kinds = [("full", f), ("blank_left", 2 + (k + 1) % 3), ("blank_right", 2 + (k + 2) % 3)]
        rot = (k + k // 3) % 3                                     # a buffer set sees the kinds at other positions when it is reused
        kinds = (kinds[rot:] + kinds[:rot]) if n_pairs == 3 else kinds[:1]
        tickets_pairs.append([((kind, g), blank if kind == "blank_left" else frames[g][0], blank if kind == "blank_right" else frames[g][1])
                              for kind, g in kinds])
    keep, bufs = [], []
    for pairs in tickets_pairs:
        n = len(pairs)
        if pinned:
            pl, pr = PinnedArray((n, pitch), np.uint8), PinnedArray((n, pitch), np.uint8)
            keep += [pl, pr]
            la, ra = pl.array, pr.array
        else:
            la, ra = np.zeros((n, pitch), np.uint8), np.zeros((n, pitch), np.uint8)
        la[...] = 0xA5
        ra[...] = 0xA5
        for p, (_, L, R) in enumerate(pairs):
            la[p, :stride * h].reshape(h, stride)[:, :w] = L
            ra[p, :stride * h].reshape(h, stride)[:, :w] = R
        bufs.append((la, ra))
    ctx, ref = _context(w, max_images=6), _context(w, max_images=2)
    try:
        assert ctx.n_features == nf and ctx.record_bytes() == 16 + 300 * 76
        outs = [ctx.alloc_batch_results(3, pinned) for _ in range(3)]
        rec = torch.empty((3, ctx.record_bytes()), dtype=torch.uint8, device="cuda")
        tickets = []

        def check(k):
            pairs = tickets_pairs[k]
            n = len(pairs)
            ctx.stream_wait(tickets[k])
            o = outs[k % 3]
            kps, desc, counts = o["kps"].reshape(-1, nf)[:2 * n], o["desc"].reshape(-1, nf, 32)[:2 * n], o["counts"][:2 * n]
            ru, dp, nms = o["right_u"].reshape(-1, nf)[:n], o["depth"].reshape(-1, nf)[:n], o["n_matches"][:n]
            rec.fill_(0xEE)
            torch.cuda.synchronize()
            ctx.stream_pack_records(tickets[k], n, rec.data_ptr())
            got = rec.cpu().numpy()
            for p, (key, L, R) in enumerate(pairs):
                r = _stereo_reference(orc, ref, w, h, key, L, R)
                what = (k, p, key)
                nl, nr = int(counts[2 * p]), int(counts[2 * p + 1])
                assert (nl, nr) == (len(r["lk"]), len(r["rk"])), what
                assert nl == (0 if key[0] == "blank_left" else 300) and nr == (0 if key[0] == "blank_right" else 300), what
                assert kps[2 * p, :nl].tobytes() == r["lk"].tobytes() and kps[2 * p + 1, :nr].tobytes() == r["rk"].tobytes(), what
                assert np.array_equal(desc[2 * p, :nl], r["ld"]) and np.array_equal(desc[2 * p + 1, :nr], r["rd"]), what
                assert int(nms[p]) == r["nm"] and (r["nm"] >= 20 if key[0] == "full" else r["nm"] == 0), what
                assert np.array_equal(ru[p].view(np.int64), r["ru"].view(np.int64)) and np.array_equal(dp[p].view(np.int64), r["dp"].view(np.int64)), what
                want = _record(nf, r["lk"], r["ld"], r["ru"], r["dp"], r["nm"])
                if key[0] == "blank_left":
                    assert not want.any()                          # a header of zeros and zeros
                assert np.array_equal(got[p], want), what + (np.flatnonzero(got[p] != want)[:8].tolist(),)
            assert (got[n:] == 0xEE).all(), k                      # nothing is written behind the ticket's own pairs

        for k, pairs in enumerate(tickets_pairs):
            if k >= 3:
                check(k - 3)                                       # its result arrays and device buffers are about to be reused
            la, ra = bufs[k]
            tickets.append(ctx.stream_submit(la, ra, len(pairs), FX, BF, outs[k % 3], stride=stride, image_pitch=pitch))
        for k in range(len(tickets_pairs) - 3, len(tickets_pairs)):
            check(k)
        assert tickets == list(range(5))
    finally:
        ctx.close(), ref.close()
        for pa in keep:
            pa.free()
