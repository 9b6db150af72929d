"""CPU-only checks of the device pose solve's C entry point (pvnet_pose_solve, include/pvnet_vote.h): both builds export it, and
every bad argument is rejected with the documented code before any HIP call -- so these run on a machine without a GPU."""
import ctypes as C
import os
import re

import pytest

from pvnet_amd import build, voting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -3
W_NONE, W_EXPLICIT, W_COV = 0, 1, 2


@pytest.fixture(scope="module")
def libs():
    build.build()
    out = []
    for path in (voting.LIB_PATH, voting.DEV_LIB_PATH):
        lib = C.CDLL(path)
        lib.pvnet_pose_solve.restype = C.c_int
        lib.pvnet_pose_solve.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        out.append(lib)
    return out


def test_header_declares_the_entry_and_its_constants():
    hdr = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
    assert re.search(r"\bint pvnet_pose_solve\s*\(", hdr)
    consts = dict(re.findall(r"#define (PVNET_POSE_\w+)\s+(-?\d+)", hdr))
    assert consts == {"PVNET_POSE_W_NONE": "0", "PVNET_POSE_W_EXPLICIT": "1", "PVNET_POSE_W_COV_F32": "2",
                      "PVNET_POSE_MAX_PN": "64"}
    assert "pvnet_pose_solve" not in open(os.path.join(ROOT, "include", "pvnet_pnp.h")).read()


def test_both_builds_export_pvnet_pose_solve(libs):
    for lib in libs:
        assert hasattr(lib, "pvnet_pose_solve")
        assert lib.pvnet_vote_abi_version() == 9


def test_bad_arguments_are_rejected_without_a_device(libs):
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    st = (C.c_int64 * 3)(18, 2, 1)

    def call(lib, pts2d=p, f64=0, strides=st, pts3d=p, weights=None, kind=W_NONE, K=p, kpi=0, n=4, pn=9, iters=200, rt=p,
             poses=None, status=None):
        return lib.pvnet_pose_solve(pts2d, f64, strides, pts3d, weights, kind, K, kpi, n, pn, iters, rt, poses, status, None)

    for lib in libs:
        assert call(lib, pts2d=None) == BADARG
        assert call(lib, strides=None) == BADARG
        assert call(lib, pts3d=None) == BADARG
        assert call(lib, K=None) == BADARG
        assert call(lib, rt=None, poses=None) == BADARG      # nothing to write
        assert call(lib, n=-1) == BADARG
        assert call(lib, iters=0) == BADARG
        assert call(lib, kind=3) == BADARG
        assert call(lib, kind=-1) == BADARG
        assert call(lib, kind=W_EXPLICIT, weights=None) == BADARG
        assert call(lib, kind=W_COV, weights=None) == BADARG
        assert call(lib, pn=5) == UNSUPPORTED                 # the linear start needs 6 points
        assert call(lib, pn=65) == UNSUPPORTED                # a lane per key-point
        assert call(lib, n=0) == 0                            # nothing to do, nothing enqueued


def test_python_entry_refuses_host_tensors():
    import numpy as np
    import torch
    from pvnet_amd import pnp as P
    with pytest.raises(RuntimeError, match="CUDA"):
        P.pnp_batch_device(np.zeros((9, 3)), torch.zeros((2, 9, 2)), P.LINEMOD_K)


def test_release_library_kernel_count_and_resources():
    """the pose kernel is one kernel of the release library (at most 55 in all), and the register check passes with it"""
    import subprocess
    import sys
    build.build()
    lib = C.CDLL(voting.LIB_PATH)
    lib.pvnet_vote_build_info.restype = C.c_char_p
    nrel = int(re.search(r"(\d+) kernels", lib.pvnet_vote_build_info().decode()).group(1))
    assert nrel <= 55
    assert b"pose_solve_kernel" in open(voting.LIB_PATH, "rb").read()
    assert "pose_solve.hip" in build.VOTE_TU
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "pose_solve_kernel" in r.stdout
