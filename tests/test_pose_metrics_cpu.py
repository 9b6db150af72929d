"""CPU-only checks of the device pose metrics' C entry point (pvnet_pose_metrics, include/pvnet_vote.h): both builds export it and
its workspace query, the ABI stays 9, every bad argument is rejected with the documented code before any HIP call (so these run
on a machine without a GPU), and the release library keeps within its kernel budget and register rule."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from pvnet_amd import build, voting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
SYM_PROJ = 1
KERNELS = ("metrics_points_kernel", "metrics_search_kernel", "metrics_final_kernel")


@pytest.fixture(scope="module")
def libs():
    build.build()
    out = []
    for path in (voting.LIB_PATH, voting.DEV_LIB_PATH):
        lib = C.CDLL(path)
        lib.pvnet_pose_metrics_workspace_bytes.restype = C.c_size_t
        lib.pvnet_pose_metrics_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.pvnet_pose_metrics.restype = C.c_int
        lib.pvnet_pose_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        out.append(lib)
    return out


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
    assert re.search(r"\bint pvnet_pose_metrics\s*\(", hdr)
    assert re.search(r"\bsize_t pvnet_pose_metrics_workspace_bytes\s*\(\s*int n,\s*int max_points,\s*int flags\s*\)", hdr)
    assert re.search(r"#define PVNET_METRIC_SYM_PROJECTION\s+1\b", hdr)
    assert "#define PVNET_VOTE_ABI_VERSION 9" in re.sub(r"\s+", " ", hdr)


def test_both_builds_export_the_metrics_and_keep_abi_9(libs):
    for lib in libs:
        assert hasattr(lib, "pvnet_pose_metrics") and hasattr(lib, "pvnet_pose_metrics_workspace_bytes")
        assert lib.pvnet_vote_abi_version() == 9


def test_workspace_bytes(libs):
    for lib in libs:
        assert lib.pvnet_pose_metrics_workspace_bytes(0, 100, 0) == 0
        assert lib.pvnet_pose_metrics_workspace_bytes(4, 0, 0) == 0
        one = lib.pvnet_pose_metrics_workspace_bytes(4, 1000, 0)
        two = lib.pvnet_pose_metrics_workspace_bytes(4, 1000, SYM_PROJ)
        # [n, searches, max_points] packed words + [n, tiles, 2] tile sums, rounded up to 256 B
        assert one >= 4 * 1000 * 8 + 4 * 4 * 16 and one % 256 == 0
        assert two >= one + 4 * 1000 * 8
        assert lib.pvnet_pose_metrics_workspace_bytes(32, 20000, 0) < lib.pvnet_pose_metrics_workspace_bytes(64, 20000, 0)


def test_bad_arguments_are_rejected_without_a_device(libs):
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    th = (C.c_double * 4)(5.0, 0.1, 5.0, 5.0)

    def call(lib, pred=p, tgt=p, f64=1, model=p, offs=p, diam=p, sym=p, ncls=3, maxp=500, ids=None, K=p, kpi=0, n=4, flags=0,
             thr=th, err=p, ok=p, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_pose_metrics_workspace_bytes(max(n, 1), max(maxp, 1), flags)
        return lib.pvnet_pose_metrics(pred, tgt, f64, model, offs, diam, sym, ncls, maxp, ids, K, kpi, n, flags, thr, err, ok,
                                      status, ws, wsb, None)

    for lib in libs:
        for name in ("pred", "tgt", "model", "offs", "diam", "sym", "K", "thr", "err", "ok"):
            assert call(lib, **{name: None}) == BADARG, name
        assert call(lib, ncls=0) == BADARG
        assert call(lib, maxp=0) == BADARG
        assert call(lib, n=-1) == BADARG
        assert call(lib, flags=2) == BADARG                    # an unknown flag
        assert call(lib, ws=C.c_void_p(0x2004)) == BADARG      # misaligned workspace
        assert call(lib, ws=None) == WORKSPACE
        assert call(lib, wsb=lib.pvnet_pose_metrics_workspace_bytes(4, 500, 0) - 8) == WORKSPACE
        assert call(lib, flags=SYM_PROJ, wsb=lib.pvnet_pose_metrics_workspace_bytes(4, 500, 0)) == WORKSPACE
        assert call(lib, maxp=(1 << 24) + 1) == UNSUPPORTED
        assert call(lib, n=65536) == UNSUPPORTED
        assert call(lib, n=40000, flags=SYM_PROJ) == UNSUPPORTED
        assert call(lib, n=0, ws=None, wsb=0) == 0               # nothing to do, nothing enqueued


def test_python_entry_refuses_host_tensors():
    import numpy as np
    import torch
    from pvnet_amd import evaluation as E
    with pytest.raises(RuntimeError, match="CUDA"):
        E.pose_metrics_device(torch.zeros((2, 3, 4), dtype=torch.float64), np.zeros((2, 3, 4)), np.eye(3), None)
    with pytest.raises(RuntimeError, match="CUDA"):
        E.pose_metrics_device(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), np.eye(3), None)
    ev = E.Evaluator(models={"cat": np.zeros((4, 3))}, diameters={"cat": 0.1}, points_3d={"cat": np.zeros((9, 3))})
    with pytest.raises(RuntimeError, match="CUDA"):
        ev.evaluate_batch(torch.zeros((2, 9, 2)), np.zeros((2, 3, 4)), "cat")
    assert ev.add_recorder == [] and ev.proj_mean_diffs == []


def test_release_library_kernel_budget_and_resources():
    """the three metric kernels are in the release library (at most 55 kernels in all), and the register check passes with them"""
    build.build()
    lib = C.CDLL(voting.LIB_PATH)
    lib.pvnet_vote_build_info.restype = C.c_char_p
    nrel = int(re.search(r"(\d+) kernels", lib.pvnet_vote_build_info().decode()).group(1))
    assert nrel <= 55
    blob = open(voting.LIB_PATH, "rb").read()
    assert all(k.encode() in blob for k in KERNELS)
    assert "pose_metrics.hip" in build.VOTE_TU
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert all(k in r.stdout for k in KERNELS)
