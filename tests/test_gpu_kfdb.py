"""The keyframe database on the device (orbfe_kfdb_*, _lib.KeyFrameDB) against the restatement of KeyFrameDB's rules
(tests/kfdb_restatement.py): survivor ids and counts equal, scores equal as int64 views, group-filter candidates equal -- on product BoW
vectors of extracted frames, on every hand-built case of tests/test_kfdb_host.py, above the LDS query size and at 20 000 keyframes."""
import subprocess
import threading

import numpy as np
import pytest

import kfdb_restatement as K
from bow_restatement import score_l1
from orb_slam2_ros2_amd import synth, synth_vocab
from orb_slam2_ros2_amd._lib import Context, KeyFrameDB, OrbfeError, Vocabulary, group_filter
from test_kfdb_host import CASES, ROOT, STUBS, COMPAT, HOST, build, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(1241, 376, n_features=2000, n_levels=8, device_id=0, max_images=64)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["trained_k10_L4", "full_k10_L5"])
def product(request, ctx, tmp_path_factory):
    """BoW vectors of 128 extracted synth frames (the four content classes in turn) under one vocabulary"""
    voc = synth_vocab.trained(0, k=10, L=4) if request.param == "trained_k10_L4" else synth_vocab.full(4, 10, 5)
    p = tmp_path_factory.mktemp("voc") / "v.txt"
    synth_vocab.write_txt(p, voc)
    v = Vocabulary.load_txt(str(p))
    bows = []
    for b in range(2):
        imgs = [synth.stereo_pair_content(f, synth.CONTENT_CLASSES[f % 4])[0] for f in range(64 * b, 64 * b + 64)]
        ctx.extract_batch(imgs)
        bows += [(w, x) for w, x, *_ in ctx.bow_slots(v, 0, 64, 4)]
    yield int(voc["is_leaf"].sum()), bows
    v.close()


def as_dict(w, x):
    return {int(a): float(b) for a, b in zip(w, x)}


def from_dict(d):
    k = sorted(d)
    return np.array(k, np.uint32), np.array([d[i] for i in k], np.float64)


def check_query(got, want, what=""):
    ids, counts, scores = got
    assert ids.tolist() == list(want), what
    assert counts.tolist() == [c for c, _ in want.values()], what
    assert np.array_equal(scores.view(np.int64), np.array([s for _, s in want.values()], np.float64).view(np.int64)), what


def device_reloc(db, ctx, q, conn, bad):
    ids, _, scores = db.query(ctx, *from_dict(q))
    return group_filter(ids, scores, [[c for c in conn.get(int(k), []) if c not in bad] for k in ids]).tolist()


def device_loop(db, ctx, q, all_connected, connected15, conn, bad, R):
    """findLoopCloseKfs as the drop-in runs it: minScore from orbfe_kfdb_score (the host's l1Score for a keyframe not in the database)"""
    ignore = [k for k in all_connected if k not in bad]
    if not connected15:
        floor = 0.0
    else:
        floor = 1.0
        for k in connected15:
            if k in bad:
                continue
            s = float(db.score(ctx, *from_dict(q), [k])[0])
            if s < floor:
                floor = s
    ids, counts, scores = db.query(ctx, *from_dict(q), ignore=ignore, min_score=floor)
    cands = group_filter(ids, scores, [[c for c in conn.get(int(k), []) if c not in bad] for k in ids]).tolist()
    return (ids, counts, scores), cands


def covisibility(ids, seed):
    """sequence neighbours (+-6) ordered by a seeded weight, ten at most"""
    rng = np.random.default_rng(seed)
    conn = {}
    for i, k in enumerate(ids):
        nb = [ids[j] for j in range(max(0, i - 6), min(len(ids), i + 7)) if j != i]
        w = rng.random(len(nb))
        conn[k] = [nb[j] for j in np.argsort(-w, kind="stable")][:10]
    return conn


def test_product_vectors_reloc_and_loop(ctx, product):
    n_words, bows = product
    db = KeyFrameDB(n_words)
    R = K.Restatement()
    kf_ids = [1000 + 7 * i for i in range(96)]          # frames 0..95 are keyframes, 96..127 stay outside
    for k, (w, x) in zip(kf_ids, bows[:96]):
        db.add(k, w, x)
        R.add(k, as_dict(w, x))
    assert len(db) == 96
    bad = {kf_ids[5], kf_ids[40]}
    for k in bad:
        db.set_bad(k)
        R.set_bad(k)
    conn = covisibility(kf_ids, 3)
    n_survivors = 0
    for f in list(range(0, 96, 9)) + list(range(96, 128, 3)):
        q = as_dict(*bows[f])
        got = db.query(ctx, *bows[f])
        check_query(got, R.query(q), f"reloc frame {f}")
        n_survivors += len(got[0])
        assert device_reloc(db, ctx, q, conn, bad) == R.reloc(q, conn), f"reloc candidates frame {f}"
    assert n_survivors > 20
    for f in range(0, 96, 11):   # a keyframe's own vector, loop mode: its neighbours ignored, the nearest ones set the floor
        k = kf_ids[f]
        q = as_dict(*bows[f])
        all_connected = conn[k]
        connected15 = [c for c in conn[k] if abs(kf_ids.index(c) - f) <= 2]
        (ids, counts, scores), cands = device_loop(db, ctx, q, all_connected, connected15, conn, bad, R)
        ignore = [c for c in all_connected if c not in bad]
        check_query((ids, counts, scores), R.query(q, ignore, R.min_score(q, connected15)), f"loop keyframe {f}")
        assert cands == R.loop(q, all_connected, connected15, conn), f"loop candidates keyframe {f}"
        check_query(db.query(ctx, *bows[f]), R.query(q), f"reloc keyframe {f}")   # its own vector in relocalisation mode too
    db.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_known_cases_on_the_device(ctx, case):
    R = build(case)
    db = KeyFrameDB(100)
    for k, b in case["kfs"].items():
        db.add(k, *from_dict(b))
    for k, b in case.get("dup", []):
        db.add(k, *from_dict(b))
    for k in case.get("erase", []):
        db.erase(k)
    for k in case.get("bad", []):
        db.set_bad(k)
    assert len(db) == len(R.kfs)
    surv, cands = run_case(R, case)
    conn, bad = case.get("conn", {}), set(case.get("bad", []))
    if case.get("mode", "reloc") == "reloc":
        check_query(db.query(ctx, *from_dict(case["q"])), surv, case["name"])
        assert device_reloc(db, ctx, case["q"], conn, bad) == cands == case["cands"]
    else:
        got, dc = device_loop(db, ctx, case["q"], case["all_connected"], case["connected15"], conn, bad, R)
        check_query(got, surv, case["name"])
        assert dc == cands == case["cands"]
    db.close()


def test_bad_words_are_rejected(ctx):
    db = KeyFrameDB(50)
    for w in ([3, 50], [5, 4], [4, 4]):   # outside the vocabulary, unsorted, repeated
        with pytest.raises(OrbfeError) as ei:
            db.add(1, np.array(w, np.uint32), np.ones(len(w)))
        assert ei.value.status == 1, w
        with pytest.raises(OrbfeError) as ei:
            db.query(ctx, np.array(w, np.uint32), np.ones(len(w)))
        assert ei.value.status == 1, w
    assert len(db) == 0
    with pytest.raises(OrbfeError) as ei:   # set_bad and score of an id that is not there
        db.set_bad(9)
    assert ei.value.status == 1
    db.add(9, np.array([1, 2], np.uint32), np.ones(2))
    with pytest.raises(OrbfeError) as ei:
        db.score(ctx, np.array([1], np.uint32), np.ones(1), [9, 10])
    assert ei.value.status == 1
    db.erase([9, 12345])          # unknown ids are ignored
    assert len(db) == 0
    db.close()


def test_query_beyond_lds_takes_the_global_path(ctx):
    rng = np.random.default_rng(8)
    n_words = 200000
    R = K.Restatement()
    db = KeyFrameDB(n_words)
    for k in range(300):
        w = np.unique(rng.integers(0, n_words, 3000)).astype(np.uint32)
        x = rng.random(len(w))
        db.add(k, w, x)
        R.add(k, as_dict(w, x))
    for nq in (8192, 8193, 20000, 65535):   # 8192 words fit LDS; above that, global memory
        w = np.sort(rng.choice(n_words, nq, replace=False)).astype(np.uint32)
        x = rng.random(nq)
        q = as_dict(w, x)
        check_query(db.query(ctx, w, x), R.query(q), f"nq {nq}")
        ign = list(range(0, 300, 7))
        check_query(db.query(ctx, w, x, ignore=ign, min_score=0.01), R.query(q, ign, 0.01), f"nq {nq} loop")
        ids = [3, 77, 150]
        s = db.score(ctx, w, x, ids)
        assert np.array_equal(s.view(np.int64), np.array([score_l1(q, R.kfs[k]) for k in ids]).view(np.int64))
    db.close()


def _zipf_bow(rng, n_words, n):
    w = np.unique(np.minimum(rng.zipf(1.3, n), n_words) - 1).astype(np.uint32)
    w = np.unique((w.astype(np.uint64) * 2654435761 % n_words).astype(np.uint32))   # spread the frequent words over the space
    x = rng.random(len(w))
    return w, x / x.sum()


def test_twenty_thousand_keyframes(ctx, product):
    n_vocab, bows = product
    rng = np.random.default_rng(21)
    n_words = max(1 << 20, n_vocab)
    db = KeyFrameDB(n_words)
    R = K.Restatement()
    next_id = 0
    for call in range(5):   # five adds (the capacity grows), erases in between
        ids, ws, xs = [], [], []
        for _ in range(4000 if call < 4 else 4000 + 400):
            w, x = _zipf_bow(rng, n_words, int(rng.integers(20, 400)))
            ids.append(next_id)
            ws.append(w)
            xs.append(x)
            next_id += 1
        off = np.concatenate([[0], np.cumsum([len(w) for w in ws])])
        db.add(ids, np.concatenate(ws), np.concatenate(xs), off)
        for k, w, x in zip(ids, ws, xs):
            R.add(k, as_dict(w, x))
        gone = rng.choice(ids, 100, replace=False).tolist()
        db.erase(gone)
        for k in gone:
            R.erase(k)
    for i, (w, x) in enumerate(bows):   # the product vectors as keyframes too (their words are below n_vocab)
        db.add(500000 + i, w, x)
        R.add(500000 + i, as_dict(w, x))
    bad = rng.choice(list(R.kfs), 300, replace=False).tolist()
    db.set_bad(bad)
    for k in bad:
        R.set_bad(k)
    assert len(db) == len(R.kfs) >= 20000
    for f in (0, 17, 64, 127):   # product queries
        q = as_dict(*bows[f])
        check_query(db.query(ctx, *bows[f]), R.query(q), f"product frame {f}")
        ign = [500000 + j for j in range(max(0, f - 3), f + 4)]
        check_query(db.query(ctx, *bows[f], ignore=ign, min_score=0.05), R.query(q, ign, 0.05), f"product frame {f} loop")
    for _ in range(3):   # Zipf queries: many survivors
        w, x = _zipf_bow(rng, n_words, 1000)
        got = db.query(ctx, w, x)
        check_query(got, R.query(as_dict(w, x)), "zipf query")
        assert len(got[0]) > 0
    db.close()


def test_two_threads_on_two_contexts_share_one_database(ctx, product):
    _, bows = product
    db = KeyFrameDB(1 << 20)
    for i, (w, x) in enumerate(bows[:100]):
        db.add(i, w, x)
    queries = [(bows[f], [f + 1, f + 2], None if f % 2 else 0.02) for f in range(0, 128, 5)]
    serial = [db.query(ctx, *b, ignore=ig, min_score=ms) for b, ig, ms in queries]
    errors = []

    def worker(seed):
        try:
            c = Context(640, 480, n_features=500, n_levels=4, device_id=0, max_images=1)
            for it in range(150):
                k = (it * 3 + seed) % len(queries)
                b, ig, ms = queries[k]
                got = db.query(c, *b, ignore=ig, min_score=ms)
                for g, s in zip(got, serial[k]):
                    assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), f"thread {seed} call {it}"
            c.close()
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(s,)) for s in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[0]
    db.close()


def test_dropin_keyframedb_over_minimal_types(product, tmp_path):
    """tests/cpp/test_kfdb_dropin.cpp: the drop-in KeyFrameDB's addKeyFrame / findRelocKfs / findLoopCloseKfs on shared_ptr keyframes;
    the candidates equal the ones the restatement wrote to the file"""
    n_words, bows = product
    R = K.Restatement()
    ids = list(range(60))
    for k in ids:
        R.add(k, as_dict(*bows[k]))
    bad = {7, 30}
    for k in bad:
        R.set_bad(k)
    conn = covisibility(ids, 5)
    cases = []
    for f in (61, 70, 90, 100):   # relocalisation of frames outside
        cases.append(("reloc", f, [], [], R.reloc(as_dict(*bows[f]), conn)))
    for f in (3, 20, 45):        # loop: a new keyframe (not in the database yet) queried with its neighbours connected
        all_c = conn[f - 1][:4]
        c15 = conn[f - 1][:2]
        cases.append(("loop", f + 200, all_c, c15, None))
    with open(tmp_path / "in.txt", "w") as fh:
        fh.write(f"{n_words} {len(bows)}\n")
        for w, x in bows:
            fh.write(f"{len(w)} " + " ".join(f"{a} {int(np.float64(b).view(np.uint64)):016x}" for a, b in zip(w, x)) + "\n")
        fh.write(f"{len(ids)} " + " ".join(map(str, ids)) + "\n")
        fh.write(f"{len(bad)} " + " ".join(map(str, sorted(bad))) + "\n")
        for k in ids:
            fh.write(f"{len(conn[k])} " + " ".join(map(str, conn[k])) + "\n")
        fh.write(f"{len(cases)}\n")
        for mode, f, all_c, c15, want in cases:
            if mode == "loop":   # the new keyframe is frame f - 200's vector; the restatement's answer before it is added
                q = as_dict(*bows[f - 200])
                want = R.loop(q, all_c, c15, conn)
            fh.write(f"{mode} {f} {len(all_c)} {' '.join(map(str, all_c))} {len(c15)} {' '.join(map(str, c15))} {len(want)} {' '.join(map(str, want))}\n")
    exe = str(tmp_path / "test_kfdb_dropin")
    pkg = f"{ROOT}/orb_slam2_ros2_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + COMPAT, "-I" + STUBS, "-I" + HOST, "-I" + f"{ROOT}/include", "-o", exe,
                           f"{ROOT}/tests/cpp/test_kfdb_dropin.cpp", "-L" + pkg, "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "in.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[:2] == ["KFDB_DROPIN_OK", str(len(cases))], r.stdout
