"""The keyframe store's surface without a device: the header declares its entry points and the built library exports them, the ABI
version is unchanged (the store only adds), the bindings exist, the drop-in header goes through the compiler against the reference's real
class declarations, and the store's host-side bookkeeping (slab allocator, id map) runs as a stand-alone program under the host
compiler's sanitizers."""
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

ENTRY_POINTS = ["orbfe_kfstore_create", "orbfe_kfstore_destroy", "orbfe_kfstore_add", "orbfe_kfstore_add_from_slot", "orbfe_kfstore_set_bow",
                "orbfe_kfstore_erase", "orbfe_kfstore_size", "orbfe_kfstore_info_get", "orbfe_kfstore_fetch", "orbfe_fuse_into_keyframes_stored",
                "orbfe_create_new_map_points_stored"]


def test_header_declares_and_library_exports_the_entry_points():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ENTRY_POINTS:
        assert re.search(r"\b(orbfe_status|void)\s+" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    for typ in ("orbfe_kfstore_info", "orbfe_fuse_pose", "orbfe_tri_state"):
        assert re.search(r"\}\s*" + typ + r"\s*;", hdr), typ
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4


def test_bindings_exist_and_mirror_the_structures():
    from orb_slam2_ros2_amd import _lib
    for m in ("add", "add_from_slot", "set_bow", "erase", "fetch", "info", "__len__", "close"):
        assert callable(getattr(_lib.KeyframeStore, m)), m
    assert callable(_lib.Context.fuse_into_keyframes_stored) and callable(_lib.Context.create_new_map_points_stored)
    # the ctypes mirrors against the C layout (x86-64 / LP64): int32 n + pointer + 35 floats + two pointers; 12 floats; 7 int32 + 4 floats + (4 bytes of padding) int64
    assert ctypes.sizeof(_lib.TriState) == 8 + 8 + 35 * 4 + 4 + 16 and ctypes.sizeof(_lib.FusePose) == 48 and ctypes.sizeof(_lib.KfstoreInfo) == 56


def test_create_checks_its_arguments_before_it_looks_for_a_device():
    from orb_slam2_ros2_amd._lib import KeyframeStore, OrbfeError
    for kw in (dict(width=0, height=480), dict(width=640, height=480, n_levels=0), dict(width=640, height=480, n_levels=17),
               dict(width=640, height=480, slab_bytes=-1)):
        with pytest.raises(OrbfeError) as ei:
            KeyframeStore(**kw)
        assert ei.value.status == 1


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_kfstore_body.cpp: orbfe_kfstore_dropin.hpp with the reference's LocalMapping.h / KeyFrame.h /
    MapPoint.h / Map.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION section 3's friend line), the two bodies of
    INTEGRATION section 12 and the insertions of KeyFrame::create / deleteKeyFrame"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_kfstore_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_bookkeeping_stand_alone(tmp_path):
    """tests/cpp/test_kfstore_alloc.cpp: kfstore_alloc.h has no HIP in it, so the slab and id-map rules run here, with the host compiler's
    address and undefined-behaviour sanitizers when this g++ has their runtimes (a stand-alone program; nothing of it is loaded into python)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_kfstore_alloc.cpp")
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
    print("test_kfstore_alloc.cpp:", mode)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout + r.stderr)[-2000:]
