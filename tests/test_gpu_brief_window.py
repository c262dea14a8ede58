"""k_brief's window geometry: the 37 x 37 window arrives in LDS as 37 rows of 48 bytes by two 16-byte LDS-DMA instructions per
keypoint, into one of two buffers per wave, and the list entry and sin / cos of a keypoint come through the scalar cache.  Small
images (160 x 120, 3 levels) put keypoints ON the border the window may touch -- distance 19 from each side, on every level -- and at
every alignment of the window's first column and row; descriptors are compared bit for bit with the CPU oracle, once through the
batch launch (32 images) and once as a single pair (the launch that also delivers to host memory and builds the row tables)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, NL = 160, 120, 3
NF = 301          # not a multiple of the 8 keypoints a descriptor workgroup takes (4 waves x 2 keypoints): the last wave has one
N_IMG = 32
PAIR = (0, 11)    # a full image and one with an odd count below NF: the wave of its last keypoint holds an unused list slot
FX, BF = 400.0, 200.0


def _image(i):
    """block noise (3 .. 6 pixel blocks at a random phase: corners everywhere, the border included); image 5: a flat ground"""
    rng = np.random.default_rng(7000 + i)
    if i == 5:
        return np.full((H, W), 90, np.uint8)
    b = 3 + i % 4
    ox, oy = rng.integers(0, b, 2)
    g = rng.integers(0, 256, ((H + 2 * b) // b + 1, (W + 2 * b) // b + 1)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((b, b), np.uint8))[oy:oy + H, ox:ox + W])


@pytest.fixture(scope="module")
def images():
    return [_image(i) for i in range(N_IMG)]


@pytest.fixture(scope="module")
def reference(orc, images):
    """(keypoints, descriptors) of every image by the oracle, computed once"""
    return [orc.extractor(im, n_features=NF, n_levels=NL).extract() for im in images]


def _cases(ctx, results):
    """which of the window's edge cases the fetched keypoints hold: level coordinates are keypoint / scale factor of its octave"""
    sf = ctx.scale_factors()
    seen = set()
    for kps, _ in results:
        n = len(kps)
        if 0 < n < ctx.n_features:
            seen.add("short")
            if n % 2:
                seen.add("unused slot beside a keypoint")   # a wave takes keypoints 2 j and 2 j + 1
        for l in range(NL):
            li = ctx.level_info(l)
            m = kps["octave"] == l
            x = np.rint(kps["x"][m] / sf[l]).astype(int)
            y = np.rint(kps["y"][m] / sf[l]).astype(int)
            for name, hit in (("left", x == 19), ("right", x == li.width - 20), ("top", y == 19), ("bottom", y == li.height - 20)):
                if hit.any():
                    seen.add((name, l))
            seen.update(("x residue", int(r)) for r in set((x - 18) % 4))
            seen.update(("y parity", int(r)) for r in set((y - 18) % 2))
    return seen


def _assert_equal(results, reference, idx, what):
    for (kps, desc), i in zip(results, idx):
        rk, rd = reference[i]
        assert len(kps) == len(rk) and np.array_equal(kps, rk), f"{what}: keypoints of image {i}"
        assert np.array_equal(desc, rd), f"{what}: descriptors of image {i}"


def test_batch_of_32_images_equals_the_oracle(images, reference):
    from orb_slam2_ros2_amd._lib import Context
    ctx = Context(W, H, n_features=NF, n_levels=NL, max_images=N_IMG)
    assert ctx.n_features == NF and NF % 8 != 0
    res = ctx.extract_batch(images)
    seen = _cases(ctx, res)
    ctx.close()
    want = {(side, l) for side in ("left", "right", "top", "bottom") for l in range(NL)}
    want |= {("x residue", r) for r in range(4)} | {("y parity", r) for r in range(2)} | {"short", "unused slot beside a keypoint"}
    assert want <= seen, f"the inputs no longer produce: {sorted(want - seen, key=str)}"
    assert any(len(k) == NF for k, _ in res) and any(len(k) == 0 for k, _ in res)
    _assert_equal(res, reference, range(N_IMG), "batch")


def test_single_pair_equals_the_oracle(images, reference):
    from orb_slam2_ros2_amd._lib import Context
    ctx = Context(W, H, n_features=NF, n_levels=NL, max_images=2)
    left, right, _, _, _ = ctx.frame_stereo(images[PAIR[0]], images[PAIR[1]], FX, BF)
    seen = _cases(ctx, [left, right])
    again = ctx.extract_batch([images[PAIR[1]], images[PAIR[0]]])   # the two-image launch without the row tables, buffers reused
    ctx.close()
    want = {("x residue", r) for r in range(4)} | {("y parity", r) for r in range(2)} | {"short", "unused slot beside a keypoint"}
    want |= {(side, NL - 1) for side in ("left", "right", "top", "bottom")}
    assert want <= seen, f"the inputs no longer produce: {sorted(want - seen, key=str)}"
    assert len(left[0]) == NF
    _assert_equal([left, right], reference, PAIR, "pair")
    _assert_equal(again, reference, PAIR[::-1], "pair, swapped")
