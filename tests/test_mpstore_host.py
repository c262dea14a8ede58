"""The map-point store's surface without a device: the header declares its entry points and the library exports them, the bindings
exist and mirror the structure, the drop-in overload goes through the compiler against the reference's real class declarations, the
test program of the drop-in layer compiles and links, and the store's host-side bookkeeping (the paged index) runs as a stand-alone
program under the host compiler's sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/ORB_SLAM2"

ENTRY_POINTS = ["orbfe_mpstore_create", "orbfe_mpstore_destroy", "orbfe_mpstore_upsert", "orbfe_mpstore_erase", "orbfe_mpstore_fetch",
                "orbfe_mpstore_size", "orbfe_track_local_map_stored"]


def test_header_declares_and_library_exports_the_entry_points():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ENTRY_POINTS:
        assert re.search(r"\b(orbfe_status|void)\s+" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert re.search(r"\}\s*orbfe_track_stored_input\s*;", hdr)
    for name, value in (("ORBFE_MP_POS", 1), ("ORBFE_MP_NORMAL_DEPTH", 2), ("ORBFE_MP_DESC", 4), ("ORBFE_MP_ALL", 7)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u\b", hdr), name
    assert (_lib.MP_POS, _lib.MP_NORMAL_DEPTH, _lib.MP_DESC, _lib.MP_ALL) == (1, 2, 4, 7)
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4          # the store only adds


def test_bindings_exist_and_mirror_the_structure():
    from orb_slam2_ros2_amd import _lib
    for m in ("upsert", "erase", "fetch", "size", "close"):
        assert callable(getattr(_lib.MapPointStore, m)), m
    assert callable(_lib.Context.track_local_map_stored)
    # x86-64 / LP64: int32 n_mp (+ 4 bytes of padding), seven pointers, two floats, two int32
    assert ctypes.sizeof(_lib.TrackStoredInput) == 8 + 7 * 8 + 16
    # orbfe_track_input with ids in place of the five point arrays: the remaining fields in the same order
    a, b = [f[0] for f in _lib.TrackInput._fields_], [f[0] for f in _lib.TrackStoredInput._fields_]
    assert b == ["n_mp", "ids"] + [f for f in a[1:] if f not in ("pos", "view_dir", "max_dist", "min_dist", "desc")]


def test_create_checks_its_arguments_before_it_looks_for_a_device():
    from orb_slam2_ros2_amd._lib import MapPointStore, OrbfeError
    for kw in (dict(rows_per_page=-1), dict(max_pages=-1), dict(rows_per_page=(1 << 20) + 1), dict(max_pages=(1 << 16) + 1)):   # ORBFE_MP_MAX_*
        with pytest.raises(OrbfeError) as ei:
            MapPointStore(**kw)
        assert ei.value.status == 1


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_mpstore_body.cpp: orbfe::dropin::trackLocalMap(store, ...) and MapPointStore<>'s touch / flush /
    ensure / erase / verify instantiated with the reference's Frame.h / MapPoint.h / Camera.h / Tracking.h (symlinks; Frame.h as a
    temporary copy with INTEGRATION section 3's friend line)"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_mpstore_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def build_dropin_test(out_dir):
    """tests/cpp/test_mpstore_dropin.cpp over the stand-in opencv2/core.hpp, linked to liborbfe_hip.so (tests/test_gpu_mpstore.py runs it)"""
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = os.path.join(str(out_dir), "test_mpstore_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_mpstore_dropin.cpp"), "-L" + pkg, "-lorbfe_hip", "-pthread",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    return exe


def build_shim_test(out_dir):
    """tests/cpp/test_mpstore_shim.cpp: orbfe::MapPointStore and ORBMatcher::trackLocalMapStored of host/orbfe_shim.hpp (no OpenCV)"""
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = os.path.join(str(out_dir), "test_mpstore_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mpstore_shim.cpp"),
                           "-L" + pkg, "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shim_test_program_compiles_and_fails_loudly_without_device(tmp_path):
    import torch
    exe = build_shim_test(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("a device is present: tests/test_gpu_mpstore.py runs the program")
    from orb_slam2_ros2_amd import synth
    synth.stereo_pair(0, 640, 240, n_rect=100)[0].tofile(tmp_path / "L.raw")
    r = subprocess.run([exe, str(tmp_path / "L.raw"), "640", "240"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stdout.strip() == "NO_DEVICE"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dropin_test_program_compiles_and_links(tmp_path):
    exe = build_dropin_test(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2                                # no mode given: usage


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_index_stand_alone(tmp_path):
    """tests/cpp/test_mpstore_index.cpp: mpstore_index.h has no HIP in it, so the page and row arithmetic at the page edges, the duplicate
    check, the first-upsert mask rule and the capacity rule run here, with the host compiler's address and undefined-behaviour sanitizers
    when this g++ has their runtimes (a stand-alone program; nothing of it is loaded into python)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_mpstore_index.cpp")
    exe = str(tmp_path / "t")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"), "-o", exe, src]
    mode = "address + undefined-behaviour sanitizers"
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain; anything
        # else the sanitized build says is a failure of this test
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        mode = "no sanitizer runtime on this machine: plain build"
        subprocess.check_call(base, timeout=300)
    print("test_mpstore_index.cpp:", mode)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout + r.stderr)[-2000:]
