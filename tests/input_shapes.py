"""Shared by tests/test_gpu_input_shapes.py and the CPU tests beside it: the geometries, images, cameras and numpy restatements with which
the colour, RGB-D and stream inputs are tested away from 640 x 480.  No test lives here."""
import numpy as np

from orb_slam2_ros2_amd import synth

# S (333..336 wide): every residue of w % 4.  WIDE (1024, 1025, 1027): one workgroup column of k_cvt_gray (1024 pixels), then a second
# holding 1 and 3 pixels.  WIDE3 (2050): three columns.  The wide images are 104 and 168 rows high, not 96: the device quadtree holds
# at most 16 root strips (round((w - 32) / (h - 32)) of a level, ORBFE_MAX_STRIPS), and orbfe_create refuses 1024..1027 x 96 (level 1,
# 853..856 x 80: 17 strips) and 2050 x 96 (32) with ORBFE_EBADSIZE.  104 and 168 are the first heights, in steps of 8, at which every
# level has at most 16; the oracle fills both quotas (273 / 227) there as it does at 96.
S_H, W_H, W3_H = 257, 104, 168
S = dict(h=S_H, n_levels=4, n_features=300)
WIDE = dict(h=W_H, n_levels=2, n_features=500)
WIDE3 = dict(h=W3_H, n_levels=2, n_features=500)
N_RECT = 80
TUM_COEF = dict(k1=0.231222, k2=-0.784899, p1=-0.003257, p2=-0.000105, k3=0.917205)
GRAY_COEF = {0: (4899, 9617, 1868, 14), 1: (9798, 19235, 3735, 15)}
MARKERS = np.array([(255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)], np.uint8)


def color_image(seed, w, h):
    """three different planes plus noise (as tests/test_frame_glue.py), with the extreme colours in the first column and the last four
    columns of the first and the last row: the pixels a conversion that mishandles a row's tail gets wrong"""
    g = synth.mono_image(seed, w, h, n_rect=N_RECT)
    rng = np.random.default_rng(seed)
    img = np.stack([g, np.roll(g, 3, 1), (255 - g)], 2).astype(np.int32) + rng.integers(-6, 7, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    for y in (0, h - 1):
        for i, x in enumerate((0, w - 4, w - 3, w - 2, w - 1)):
            img[y, x] = MARKERS[(i + (y != 0)) % 5]
    return img


def padded_rows(a, pad_bytes, fill=0xA5):
    """a (h, ...) as a view into a buffer filled with `fill` whose rows are pad_bytes further apart than a's"""
    h = a.shape[0]
    row = int(np.prod(a.shape[1:])) * a.dtype.itemsize
    buf = np.full((h, row + pad_bytes), fill, np.uint8)
    view = buf[:, :row].view(a.dtype).reshape((h,) + a.shape[1:])
    view[...] = a
    assert view.base is not None and view.strides[0] == row + pad_bytes and not view.flags.c_contiguous
    return view


def gray_numpy(img, order, variant):
    cr, cg, cb, shift = GRAY_COEF[variant]
    r, g, b = (img[..., 0], img[..., 1], img[..., 2]) if order == 1 else (img[..., 2], img[..., 1], img[..., 0])
    half = 1 << (shift - 1)
    return ((r.astype(np.int64) * cr + g.astype(np.int64) * cg + b.astype(np.int64) * cb + half) >> shift).astype(np.uint8)


def camera(w, h, **coef):
    """intrinsics scaled to the geometry: fx = fy = 0.8 w, the principal point half a pixel off centre"""
    cam = dict(fx=0.8 * w, fy=0.8 * w, cx=w / 2 + 0.5, cy=h / 2 - 0.5, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, bf=40.0)
    cam.update(coef)
    return cam


def cameras(w, h):
    """the four cameras of the RGB-D tail: TUM's coefficients; k1 == 0 with the other four set (Camera.cc:31 looks at k1 alone); two with
    a radial term strong enough that 1 + k1 r2 + .. turns negative inside the image (the `icdist < 0` exit of the undistortion)"""
    rest = {k: v for k, v in TUM_COEF.items() if k != "k1"}
    return {"tum": camera(w, h, **TUM_COEF), "k1_zero": camera(w, h, k1=0.0, **rest), "k1_-4": camera(w, h, k1=-4.0, **rest),
            "k1_-8": camera(w, h, k1=-8.0, **rest)}


def cam_arrays(cam):
    return (np.array([cam[q] for q in ("fx", "fy", "cx", "cy")], np.float32), np.array([cam[q] for q in ("k1", "k2", "p1", "p2", "k3")], np.float32))


def undistort_numpy(xy, cam):
    """cv::undistortPoints with P = K as Camera::undistortPoints calls it (src/Camera.cc:29-39): five fixed iterations in float64 on float32
    inputs, every operation in the order of the C sources, leaving through `icdist < 0` with the normalised input.
    -> (undistorted (n, 2) float32, number of points that left through the exit)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    K, D = cam_arrays(cam)
    if D[0] == 0:
        return xy.copy(), 0
    fx, fy, cx, cy = (np.float64(v) for v in K)
    k0, k1, k2, k3, k4 = (np.float64(v) for v in D)
    ifx, ify = 1.0 / fx, 1.0 / fy
    u, v = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    x0, y0 = (u - cx) * ifx, (v - cy) * ify
    x, y = x0.copy(), y0.copy()
    live = np.ones(len(xy), bool)          # still iterating
    with np.errstate(all="ignore"):
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2)
            out = live & (icdist < 0)
            x[out], y[out] = x0[out], y0[out]
            live &= ~out
            dx = 2 * k2 * x * y + k3 * (r2 + 2 * x * x) + 0 * r2 + 0 * r2 * r2
            dy = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y + 0 * r2 + 0 * r2 * r2
            x = np.where(live, (x0 - dx) * icdist, x)
            y = np.where(live, (y0 - dy) * icdist, y)
        xx, yy, ww = fx * x + 0 * y + cx, 0 * x + fy * y + cy, 1.0 / (0 * x + 0 * y + 1)
        und = np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], 1)
    return und, int((~live).sum())


def assert_keypoints_equal(k, ok):
    assert len(k) == len(ok)
    for f in ("x", "y", "angle", "response", "octave"):
        assert np.array_equal(k[f].view(np.int32), ok[f].view(np.int32)), f
