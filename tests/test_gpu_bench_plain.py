"""The plain benchmark line and its output dump: `bench.py` without --full times the step loop and prints the headline keys only;
--dump-outputs writes the last step's results as float32 / float64 arrays.  One rank, and two gloo ranks on cuda:0 (the bench's own test
hooks, as tests/test_gpu_two_ranks.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("verified_pairs", "host_io", "sequence", "roofline", "cpu_baseline", "cfg3", "ba", "latency")


def _run(args, env):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", "8", "--steps", "3", "--warmup", "1", "--prewarm-seconds", "0.1"] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1, "ONE JSON line on stdout is the contract"
    return json.loads(lines[0])


def _clean_env(**extra):
    env = dict(os.environ, **extra)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_plain_line_and_dumped_outputs(tmp_path):
    d = _run(["--gpus", "1", "--dump-outputs", str(tmp_path / "a")], _clean_env())
    assert all(k in d for k in HEAD) and not any(k in d for k in EXTRAS)
    assert d["steps"] == 3 and d["unit"] == "stereo pairs/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 8) < 1e-6 * 8      # pairs per step = value x seconds per step
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(a) == {"counts", "n_matches", "sample_pairs", "keypoints", "descriptors", "right_u", "depth"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["counts"].shape == (8, 2) and a["n_matches"].shape == (8,) and a["sample_pairs"].shape == (8,)
    assert a["keypoints"].shape == (8, 2, 2000, 7) and a["descriptors"].shape == (8, 2, 2000, 32)
    assert a["right_u"].shape == (8, 2000) and a["depth"].shape == (8, 2000)
    assert (a["counts"] > 0).all() and (a["n_matches"] > 0).all()
    assert np.array_equal(a["sample_pairs"], np.arange(8))
    for p in range(8):   # the sampled pairs' arrays agree with the counts: filled up to the count, zero past it
        for e in range(2):
            n = int(a["counts"][p, e])
            assert (a["keypoints"][p, e, n:] == 0).all() and (a["descriptors"][p, e, n:] == 0).all()
            assert (a["keypoints"][p, e, :n, 2] > 0).all()                     # keypoint size
            assert a["descriptors"][p, e, :n].max() <= 255 and (a["descriptors"][p, e, :n] == np.round(a["descriptors"][p, e, :n])).all()
    # the same arguments give the same outputs
    _run(["--gpus", "1", "--dump-outputs", str(tmp_path / "b")], _clean_env())
    for k, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / (k + ".npy"))), k


def test_plain_line_with_two_gloo_ranks_on_one_gpu():
    d = _run(["--gpus", "2"], _clean_env(ORBFE_BENCH_ONE_DEVICE="1", ORBFE_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert all(k in d for k in HEAD) and not any(k in d for k in EXTRAS)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 3
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 16) < 1e-6 * 16     # 8 pairs per rank and step
