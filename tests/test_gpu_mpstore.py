"""The device-resident map-point store (orbfe_mpstore) and orbfe_track_local_map_stored.

The store: a paged direct index over 64-byte rows, tested at its page edges with rows_per_page = 64.  The stored call: every output of
orbfe_track_output, compared as integers, against orbfe_track_local_map given the arrays orbfe_mpstore_fetch returns for the same ids --
the array call itself is checked against the oracle in tests/test_track_chain.py, whose scene builder this file imports."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "view_dir", "max_dist", "min_dist", "desc")
EDGE_IDS = np.array([0, 1, 63, 64, 65, 127, 128, 300, 511], np.uint64)       # page edges of rows_per_page = 64, max_pages = 8


def _rows(rng, n):
    return dict(pos=rng.normal(0, 10, (n, 3)).astype(np.float32), view_dir=rng.normal(0, 1, (n, 3)).astype(np.float32),
                max_dist=rng.uniform(10, 50, n).astype(np.float32), min_dist=rng.uniform(0.1, 5, n).astype(np.float32),
                desc=rng.integers(0, 256, (n, 32)).astype(np.uint8))


def _bytes_equal(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in FIELDS)


def _status_of(fn):
    from orb_slam2_ros2_amd._lib import OrbfeError
    with pytest.raises(OrbfeError) as ei:
        fn()
    return ei.value.status


# ---- the store on its own ---------------------------------------------------------------------------------------------------------
def test_round_trip_masks_erase_and_refusals():
    from orb_slam2_ros2_amd._lib import MP_DESC, MP_NORMAL_DEPTH, MP_POS, MapPointStore
    rng = np.random.default_rng(1)
    st = MapPointStore(rows_per_page=64, max_pages=8)
    assert st.size() == dict(n_points=0, bytes_used=0, bytes_reserved=0)
    n = len(EDGE_IDS)
    rows = _rows(rng, n)
    order = rng.permutation(n)
    st.upsert(EDGE_IDS[order], **{k: rows[k][order] for k in FIELDS})
    assert _bytes_equal(st.fetch(EDGE_IDS), rows)
    assert _bytes_equal(st.fetch(EDGE_IDS[::-1]), {k: rows[k][::-1] for k in FIELDS})
    rep = np.array([64, 64, 511, 0, 64], np.uint64)                            # a fetch may name an id more than once
    at = [int(np.flatnonzero(EDGE_IDS == i)[0]) for i in rep]
    assert _bytes_equal(st.fetch(rep), {k: rows[k][at] for k in FIELDS})
    page = 64 * 65                                                             # 64 rows of 64 bytes and their presence bytes
    assert len(np.unique(EDGE_IDS // 64)) == 5                                 # pages 0, 1, 2, 4 (id 300) and 7 (id 511)
    assert st.size() == dict(n_points=9, bytes_used=9 * 64, bytes_reserved=5 * page)
    # each field mask alone changes exactly its fields
    new = _rows(rng, n)
    for mask, keys in ((MP_POS, ("pos",)), (MP_NORMAL_DEPTH, ("view_dir", "max_dist", "min_dist")), (MP_DESC, ("desc",))):
        half = np.arange(0, n, 2)
        st.upsert(EDGE_IDS[half], fields=mask, **{k: new[k][half] for k in keys})
        for k in keys:
            rows[k][half] = new[k][half]
        assert _bytes_equal(st.fetch(EDGE_IDS), rows), mask
    # erase: the id is gone, the others stay; unknown ids are ignored; inserting again works
    st.erase([64, 9999, 2])
    assert _status_of(lambda: st.fetch([64])) == 1 and _status_of(lambda: st.fetch([0, 64])) == 1
    keep = EDGE_IDS != 64
    kept = {k: rows[k][keep] for k in FIELDS}
    assert _bytes_equal(st.fetch(EDGE_IDS[keep]), kept) and st.size()["n_points"] == 8
    one = _rows(rng, 1)
    st.upsert([64], **one)
    for k in FIELDS:
        rows[k][EDGE_IDS == 64] = one[k]
    assert _bytes_equal(st.fetch(EDGE_IDS), rows) and len(st) == 9
    # refusals change nothing
    two = _rows(rng, 2)
    size = st.size()
    assert _status_of(lambda: st.upsert([0, 2], fields=MP_POS, pos=two["pos"])) == 1             # id 2 is new: a partial mask
    assert _status_of(lambda: st.upsert([400, 401], fields=MP_DESC, desc=two["desc"])) == 1      # ... on a page that does not exist
    assert _status_of(lambda: st.upsert([1, 1], **two)) == 1                                     # listed twice
    assert _status_of(lambda: st.upsert([7, 1, 8, 7], **_rows(rng, 4))) == 1
    assert _status_of(lambda: st.upsert([3, 512], **two)) == 4                                   # ORBFE_ECAPACITY
    assert _status_of(lambda: st.upsert([2 ** 40], **_rows(rng, 1))) == 4
    assert _status_of(lambda: st.upsert([0], fields=0)) == 1 and _status_of(lambda: st.upsert([0], fields=8, **_rows(rng, 1))) == 1
    assert _status_of(lambda: st.upsert([0], fields=MP_POS)) == 1                                # the array the mask names is missing
    assert st.size() == size and _bytes_equal(st.fetch(EDGE_IDS), rows)
    for i in (2, 3, 7, 8, 400, 401):
        assert _status_of(lambda: st.fetch([i])) == 1
    st.upsert([], **_rows(rng, 0))
    assert _bytes_equal(st.fetch([]), _rows(rng, 0))
    st.close()


def test_default_pages_and_a_large_id():
    """the default geometry (16384 rows per page, 4096 pages): a page is 16384 * 65 bytes, an id near the top of the range has its place"""
    from orb_slam2_ros2_amd._lib import MapPointStore
    rng = np.random.default_rng(2)
    st = MapPointStore()
    ids = np.array([16383, 16384, 16384 * 4096 - 1], np.uint64)
    rows = _rows(rng, 3)
    st.upsert(ids, **rows)
    assert _bytes_equal(st.fetch(ids), rows) and st.size() == dict(n_points=3, bytes_used=192, bytes_reserved=3 * 16384 * 65)
    assert _status_of(lambda: st.upsert([16384 * 4096], **_rows(rng, 1))) == 4
    st.close()


# ---- the stored call against the array call ---------------------------------------------------------------------------------------------
N_MP = 300


class _Bed:
    """One frame in slot 0 of a context, ~300 of test_track_chain's map points under gapped, shuffled ids in a store of 64-row pages."""

    def __init__(self):
        import test_track_chain as T
        from orb_slam2_ros2_amd._lib import Context, MapPointStore
        self.T = T
        self.ctx = Context(T.W, T.H, n_features=T.NF, max_images=2)
        full = T._scene(self.ctx, 3)
        rng = np.random.default_rng(7)
        N = len(full["pos"])
        sel = np.sort(rng.permutation(N)[:N_MP])
        new_of = np.full(N, -1, np.int32)
        new_of[sel] = np.arange(N_MP, dtype=np.int32)
        held = full["held"].copy()
        held[held >= 0] = new_of[held[held >= 0]]                              # a holder outside the subset: the feature is free
        self.s = dict(full, held=held, flags=full["flags"][sel].copy(), **{k: full[k][sel] for k in ("pos", "view_dir", "max_dist", "min_dist")},
                      desc_mp=full["mp_desc"][sel])
        self.ids = (rng.permutation(3 * N_MP)[:N_MP] * 2 + 5).astype(np.uint64)          # gapped, in no order, over ~29 pages
        self.store = MapPointStore(rows_per_page=64, max_pages=512)
        self.rows = dict(pos=self.s["pos"], view_dir=self.s["view_dir"], max_dist=self.s["max_dist"], min_dist=self.s["min_dist"], desc=self.s["desc_mp"])
        self.store.upsert(self.ids, **self.rows)
        sig2 = (T.SF * T.SF).astype(np.float32)
        self.tail = (self.s["Rcw"], self.s["tcw"], (T.FX, T.FY, T.CX, T.CY, T.BF), (0.0, float(T.W), 0.0, float(T.H)), self.s["pose_se3"], sig2,
                     (np.float32(1.0) / sig2).astype(np.float32))

    def stored(self, ids, flags, ctx=None, **kw):
        return (ctx or self.ctx).track_local_map_stored(0, self.store, ids, flags, *self.tail, right_u=self.s["right_u"], **kw)

    def arrays(self, ids, flags, ctx=None, rows=None, **kw):
        r = self.store.fetch(ids) if rows is None else rows
        return (ctx or self.ctx).track_local_map(0, r["pos"], r["view_dir"], r["max_dist"], r["min_dist"], r["desc"], flags, *self.tail,
                                                 right_u=self.s["right_u"], **kw)


@pytest.fixture(scope="module")
def bed():
    b = _Bed()
    yield b
    b.store.close()
    b.ctx.close()


def _same(a, b):
    """every output of orbfe_track_output, as integers"""
    return (all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in ("assigned", "edge_of", "inlier")) and
            np.array_equal(a["pose"].view(np.uint64), b["pose"].view(np.uint64)) and all(a[k] == b[k] for k in ("n_matches", "n_edges", "n_good")))


def test_stored_call_equals_array_call(bed):
    s, ids = bed.s, bed.ids
    assert _bytes_equal(bed.store.fetch(ids), bed.rows) and len(np.unique(ids // 64)) > 8
    # ids a gapped permutation, held entries, bad and not-in-map points as the scene has them
    g, a = bed.stored(ids, s["flags"], held=s["held"]), bed.arrays(ids, s["flags"], held=s["held"], rows=bed.rows)
    assert _same(g, a) and g["n_edges"] >= 30 and g["n_good"] > 20 and (s["held"] >= 0).sum() > 5
    assert (g["assigned"] != s["held"]).sum() > 100 and np.abs(g["pose"] - s["pose_se3"]).max() > 1e-4          # it searched and it moved
    # extras: points the frame holds from an earlier stage that are not in the local map carry flag bits 0-1 only
    fl = s["flags"].copy()
    extras = np.unique(s["held"][s["held"] >= 0])[::2]
    fl[extras] &= 3
    g2, a2 = bed.stored(ids, fl, held=s["held"]), bed.arrays(ids, fl, held=s["held"])
    assert _same(g2, a2) and not _same(g2, g)
    # no held entries
    assert _same(bed.stored(ids, s["flags"]), bed.arrays(ids, s["flags"]))
    # an id listed twice: the array call gets the row twice
    ids2, fl2 = ids.copy(), s["flags"].copy()
    ids2[10], ids2[200] = ids2[150], ids2[20]
    fl2[[10, 150, 20, 200]] = 7
    r2 = bed.store.fetch(ids2)
    assert np.array_equal(r2["pos"][10], bed.rows["pos"][150]) and np.array_equal(r2["desc"][200], bed.rows["desc"][20])
    assert _same(bed.stored(ids2, fl2, held=s["held"]), bed.arrays(ids2, fl2, held=s["held"], rows=r2))
    # n_mp = 0
    e = bed.stored(ids[:0], fl[:0])
    assert _same(e, bed.arrays(ids[:0], fl[:0])) and e["n_matches"] == 0 and (e["assigned"] == -1).all()
    # a list too short for min_matches: no optimisation
    few = bed.stored(ids[:25], s["flags"][:25])
    assert _same(few, bed.arrays(ids[:25], s["flags"][:25])) and few["n_edges"] == -1 and 0 < few["n_matches"] < 30


def test_stored_call_after_a_position_update_and_from_two_contexts(bed):
    from orb_slam2_ros2_amd._lib import MP_POS, Context
    from orb_slam2_ros2_amd import synth
    s, ids, T = bed.s, bed.ids, bed.T
    before = bed.stored(ids, s["flags"], held=s["held"])
    half = np.arange(0, N_MP, 2)
    moved = bed.rows["pos"].copy()
    moved[half] += np.random.default_rng(9).normal(0, 0.02, (len(half), 3)).astype(np.float32)
    try:
        bed.store.upsert(ids[half], fields=MP_POS, pos=moved[half])
        rows = dict(bed.rows, pos=moved)
        assert _bytes_equal(bed.store.fetch(ids), rows)
        g, a = bed.stored(ids, s["flags"], held=s["held"]), bed.arrays(ids, s["flags"], held=s["held"], rows=rows)
        assert _same(g, a) and not np.array_equal(g["pose"], before["pose"])
        # one store, two contexts: the second extracts the same frame into its own slot 0
        ctx2 = Context(T.W, T.H, n_features=T.NF, max_images=2)
        ctx2.extract_batch(list(synth.stereo_pair(3)))
        g2 = bed.stored(ids, s["flags"], ctx=ctx2, held=s["held"])
        assert _same(g2, bed.arrays(ids, s["flags"], ctx=ctx2, held=s["held"], rows=rows)) and _same(g2, g)
        ctx2.close()
    finally:
        bed.store.upsert(ids[half], fields=MP_POS, pos=bed.rows["pos"][half])
    assert _same(bed.stored(ids, s["flags"], held=s["held"]), before)


def test_absent_id_is_one_error_and_leaves_nothing_behind(bed):
    from orb_slam2_ros2_amd import _lib
    s, ids, T = bed.s, bed.ids, bed.T
    good = bed.arrays(ids, s["flags"], held=s["held"], rows=bed.rows)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    Rcw, tcw, cam, bounds, p0, s2, is2 = bed.tail
    fp = _lib.FramePose((C.c_float * 9)(*f32(Rcw).reshape(9)), (C.c_float * 3)(*f32(tcw).reshape(3)), *[float(np.float32(b)) for b in bounds])
    cm = _lib.Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
    held, ru, p0 = np.ascontiguousarray(s["held"], np.int32), np.ascontiguousarray(s["right_u"], np.float64), np.ascontiguousarray(p0, np.float64)
    gone = [int(ids[40]), int(ids[7])]
    for bad_ids in (ids, np.concatenate([ids[:5], np.array([10 ** 12, 2 ** 63], np.uint64), ids[5:-2]])):     # erased rows; ids past the capacity
        bed.store.erase(gone)
        out = dict(assigned=np.full(T.NF, 0x5A5A5A5A, np.int32), edge_of=np.full(T.NF, 0x5A5A5A5A, np.int32), inlier=np.full(T.NF, 0x5A, np.uint8),
                   pose=np.full(7, 12345.678), cnt=np.full(3, 0x5A5A5A5A, np.int32))
        ref = {k: v.copy() for k, v in out.items()}
        bid = np.ascontiguousarray(bad_ids, np.uint64)
        ti = _lib.TrackStoredInput(len(bid), *[_lib.ptr(a) for a in (bid, s["flags"], held, ru, s2, is2, p0)], 3.0, 0.8, 50, 30)
        cp = out["cnt"].ctypes.data
        to = _lib.TrackOutput(_lib.ptr(out["assigned"]), _lib.ptr(out["edge_of"]), _lib.ptr(out["inlier"]), C.c_void_p(cp), C.c_void_p(cp + 4),
                              C.c_void_p(cp + 8), _lib.ptr(out["pose"]))
        st = bed.ctx.lib.orbfe_track_local_map_stored(bed.ctx.h, 0, bed.store.h, C.byref(fp), C.byref(cm), C.byref(ti), C.byref(to))
        assert st == 1 and all(np.array_equal(out[k], ref[k]) for k in out)
        msg = bed.ctx.lib.orbfe_last_error(bed.ctx.h).decode()
        first = next(int(i) for i in bad_ids if int(i) in gone or int(i) >= 64 * 512)
        assert str(first) in msg, msg
        assert _status_of(lambda: bed.stored(ids, s["flags"], held=s["held"])) == 1
        # the next correct call on the same context: nothing of the refused one is left in the scratch
        at = [40, 7]
        bed.store.upsert(ids[at], **{k: bed.rows[k][at] for k in FIELDS})
        assert _same(bed.stored(ids, s["flags"], held=s["held"]), good)
    # a store on another device cannot be made here; NULL ids with n_mp > 0
    ti = _lib.TrackStoredInput(5, None, *[_lib.ptr(a) for a in (s["flags"], held, ru, s2, is2, p0)], 3.0, 0.8, 50, 30)
    assert bed.ctx.lib.orbfe_track_local_map_stored(bed.ctx.h, 0, bed.store.h, C.byref(fp), C.byref(cm), C.byref(ti), C.byref(to)) == 1


def test_the_2048_feature_rule_stays(bed):
    from orb_slam2_ros2_amd._lib import Context
    ctx = Context(640, 240, n_features=2100, n_levels=6, max_images=2)
    sig2 = np.ones(6, np.float32)
    st = _status_of(lambda: ctx.track_local_map_stored(0, bed.store, bed.ids[:4], np.full(4, 7, np.uint8), np.eye(3), np.zeros(3), (400, 400, 320, 120, 200),
                                                       (0.0, 640.0, 0.0, 240.0), np.array([0, 0, 0, 1, 0, 0, 0.0]), sig2, sig2))
    assert st == 2                                                             # ORBFE_EBADSIZE
    ctx.close()


def test_stored_calls_while_another_thread_adds_pages(bed):
    """the lock: 200 upserts, each to a row of a page the store does not have yet (so the page table is rewritten 200 times), beside
    200 stored calls that must all see their own rows untouched"""
    s, ids = bed.s, bed.ids
    want = bed.arrays(ids, s["flags"], held=s["held"], rows=bed.rows)
    first_page = int(ids.max()) // 64 + 1
    assert first_page + 200 <= 512
    pages0 = bed.store.size()["bytes_reserved"] // (64 * 65)
    rng = np.random.default_rng(11)
    err = []

    def writer():
        try:
            for k in range(200):
                bed.store.upsert([(first_page + k) * 64 + k % 64], **_rows(rng, 1))
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = threading.Thread(target=writer)
    th.start()
    try:
        results = [bed.stored(ids, s["flags"], held=s["held"]) for _ in range(200)]
    finally:
        th.join()
    assert not err, err
    assert all(_same(r, want) for r in results)
    assert bed.store.size()["bytes_reserved"] // (64 * 65) == pages0 + 200 and _bytes_equal(bed.store.fetch(ids), bed.rows)
    bed.store.erase([(first_page + k) * 64 + k % 64 for k in range(200)])
    assert len(bed.store) == N_MP


# ---- the drop-in layer ------------------------------------------------------------------------------------------------------------------
def test_dropin_overload_equals_the_array_overload(tmp_path):
    """tests/cpp/test_mpstore_dropin.cpp compare: orbfe::dropin::trackLocalMap(store, ...) against the existing trackLocalMap on twin frames
    and twin maps of stand-in classes -- return value, nGood, every feature's map point, both counters of every map point, the pose to
    the bit; again after setPos with touch; verify() names exactly the points changed without a touch; erased points come back"""
    import subprocess

    from orb_slam2_ros2_amd import synth
    from test_mpstore_host import build_dropin_test
    exe = build_dropin_test(tmp_path)
    L, R = synth.stereo_pair(3)
    L.tofile(tmp_path / "L.raw")
    R.tofile(tmp_path / "R.raw")
    out = subprocess.run([exe, "compare", str(tmp_path / "L.raw"), str(tmp_path / "R.raw"), "1241", "376"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    f = out.stdout.split()
    assert f[0] == "MPSTORE_DROPIN_OK" and int(f[1]) > 800 and int(f[2]) > 300 and int(f[5]) > 100, out.stdout


def test_shim_store_and_stored_call(tmp_path):
    """tests/cpp/test_mpstore_shim.cpp: the OpenCV-free mirror -- orbfe::MapPointStore's round trip and ORBMatcher::trackLocalMapStored on a
    frame whose local map is its own keypoints at 10 m"""
    import subprocess

    from orb_slam2_ros2_amd import synth
    from test_mpstore_host import build_shim_test
    exe = build_shim_test(tmp_path)
    synth.stereo_pair(3)[0].tofile(tmp_path / "L.raw")
    out = subprocess.run([exe, str(tmp_path / "L.raw"), "1241", "376"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    f = out.stdout.split()
    assert f[0] == "MPSTORE_SHIM_OK" and int(f[2]) >= int(f[1]) // 2 and int(f[3]) >= 30, out.stdout
