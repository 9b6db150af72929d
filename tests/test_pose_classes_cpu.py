"""CPU-only checks of the pose solve per class (include/pvnet_poses.h, libpvnet_poses.so: pvnet_amd/csrc/pose_classes.hip on the shared
solver pvnet_amd/csrc/pose_core.h; pnp.pnp_classes_device, voting.MultiPoseEvalWrapper): the registry row and its place, the header's
constants and parameter list against pvnet_amd/_abi.py, the library's one kernel and its register check, the voting library's kernel
count and ABI version unchanged, every bad argument refused before any HIP call, where the shared header is a dependency, the Python
refusals, and that the shared cases (tests/pose_classes_cases.py) can tell the classes apart.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build
from pvnet_amd import pnp as P
from tests import pose_cases
from tests import pose_classes_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_poses.h")).read()
CORE = os.path.join(build.CSRC, "pose_core.h")
BADARG, UNSUPPORTED = -1, -3
PARAMETERS = ["pts2d", "pts2d_f64", "pts2d_strides", "pts3d", "weights", "weight_kind", "K", "k_per_image", "vote_status", "b", "nk", "pn",
              "max_iterations", "rt", "poses", "status", "stream"]
# the device solver's helpers, by the names they had in pose_solve.hip
HELPERS = ["struct Shared", "cross_matrix", "matmul3", "det3", "inverse3", "rotation_and_right_jacobian", "matrix_to_angle_axis", "jacobi3",
           "jacobi12", "dlt_pose", "evaluate", "cost_of", "solve6", "refine", "covariance_weight"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_poses_library()


def test_registry_row_and_its_place():
    for table in (build.SIDE_LIBRARIES, _abi.SIDE_LIBRARIES):
        names = list(table)
        assert "poses" in names and names.index("poses") < names.index("trunk")
        assert names[-5:] == ["trunk", "stem", "decoder", "tail", "texture"]
    assert build.SIDE_LIBRARIES["poses"][:2] == (["pose_classes.hip"], "pvnet_poses.h")
    assert _abi.SIDE_LIBRARIES["poses"] == (_abi.POSES_LIB_PATH, _abi.POSES_ABI_VERSION, _abi.POSES_PROTOTYPES)
    assert _abi.POSES_LIB_PATH.endswith("libpvnet_poses.so") and callable(_abi.load_poses_library)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_abi.load_poses_library()" in entry


def test_header_constants_and_parameter_list_are_mirrored():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert returns == {"pvnet_poses_abi_version": "int", "pvnet_pose_solve_classes": "int"} and set(returns) == set(_abi.POSES_PROTOTYPES)
    consts = dict((n, int(v.strip("()"))) for n, v in re.findall(r"^#define\s+PVNET_POSES_(\w+)\s+(\(?-?\d+\)?)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.POSES_ABI_VERSION == 1
    assert consts == {"W_NONE": 0, "W_EXPLICIT": 1, "W_COV_F32": 2, "MAX_PN": 64, "MAX_CLASSES": 63, "MAX_ITEMS": (2 ** 31 - 1) // 12, "ABSENT": -3}
    for name, value in consts.items():
        assert getattr(_abi, "POSES_" + name) == value, name
    # the weight kinds and the point limit are pvnet_pose_solve's, the class limit is the per-class vote's, the status is the function's
    assert (_abi.POSES_W_NONE, _abi.POSES_W_EXPLICIT, _abi.POSES_W_COV_F32) == (_abi.POSE_W_NONE, _abi.POSE_W_EXPLICIT, _abi.POSE_W_COV_F32)
    vote_hdr = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
    assert int(re.search(r"#define PVNET_POSE_MAX_PN\s+(\d+)", vote_hdr).group(1)) == _abi.POSES_MAX_PN
    assert _abi.POSES_MAX_CLASSES == _abi.CLASSES_MAX - 1 and P.POSE_ABSENT == _abi.POSES_ABSENT and P.POSE_FAILED == -2
    assert int(re.search(r"#define PVNET_S_SKIPPED\s+(\d+)", vote_hdr).group(1)) == _abi.S_SKIPPED
    # the parameter list, position by position
    decl = re.search(r"^int pvnet_pose_solve_classes\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    assert [re.search(r"(\w+)(?:\[\d+\])?\s*$", d).group(1) for d in decl] == PARAMETERS
    args = _abi.POSES_PROTOTYPES["pvnet_pose_solve_classes"][1]
    assert len(args) == len(PARAMETERS)
    ints = {"pts2d_f64", "weight_kind", "k_per_image", "b", "nk", "pn", "max_iterations"}
    for name, d, a in zip(PARAMETERS, decl, args):
        if name in ints:
            assert a is C.c_int and re.match(r"\s*int\s+\w+$", d), name
        elif name == "pts2d_strides":
            assert a is C.POINTER(C.c_int64) and "const int64_t pts2d_strides[4]" in d
        else:
            assert a is C.c_void_p and "*" in d, name
    # the function's signature is the issue's, pnp_batch_device's with vote_status
    sig = inspect.signature(P.pnp_classes_device)
    assert list(sig.parameters) == ["points_3d", "points_2d", "camera_matrix", "weights_2d", "covariance", "vote_status", "max_iterations", "out"]
    assert sig.parameters["max_iterations"].default == 200 == inspect.signature(P.pnp_batch_device).parameters["max_iterations"].default


def test_library_has_one_kernel_under_a_name_of_its_own_and_passes_the_register_check(lib):
    blob = open(_abi.POSES_LIB_PATH, "rb").read()
    assert b"gfx950" in blob and lib.pvnet_poses_abi_version() == 1
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as chk
    (src, text), = chk.side_assembly("poses")
    assert os.path.basename(src) == "pose_classes.hip"
    own = [k[0] for k in chk.kernels(text)]
    assert len(own) == 1 and "pose_classes_kernel" in own[0]
    assert own[0].encode() + b".kd" in blob
    # the vote library's kernels, release and development build, by their descriptor symbols (as pvnet_amd.build counts them)
    vote = set().union(*(re.findall(rb"[\w$.]+\.kd(?=\x00)", open(path, "rb").read()) for path in (_abi.LIB_PATH, _abi.DEV_LIB_PATH)))
    assert len(vote) > 55 and own[0].encode() + b".kd" not in vote and not any(b"pose_classes_kernel" in v for v in vote)
    assert any(b"pose_solve_kernel" in v for v in vote)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--poses"], capture_output=True, text=True)
    assert r.returncode == 0 and "checked 1 kernels, 0 without" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for path in (_abi.LIB_PATH, _abi.DEV_LIB_PATH):
        assert b"pose_classes_kernel" not in open(path, "rb").read()
        assert not hasattr(C.CDLL(path), "pvnet_pose_solve_classes")
    assert not hasattr(C.CDLL(_abi.POSES_LIB_PATH), "pvnet_pose_solve") and b"pose_solve_kernel" not in blob


def test_the_vote_library_keeps_its_abi_and_kernel_count(lib):
    vlib = C.CDLL(_abi.LIB_PATH)
    assert vlib.pvnet_vote_abi_version() == _abi.ABI_VERSION == 9
    vlib.pvnet_vote_build_info.restype = C.c_char_p
    assert 0 < int(re.search(r"(\d+) kernels", vlib.pvnet_vote_build_info().decode()).group(1)) <= 55
    assert hasattr(vlib, "pvnet_pose_solve") and b"pose_solve_kernel" in open(_abi.LIB_PATH, "rb").read()


def test_bad_arguments_are_refused_without_a_device(lib):
    p = C.c_void_p(0x1000)   # never dereferenced: validation returns before any HIP call
    st = (C.c_int64 * 4)(54, 18, 2, 1)

    def call(pts2d=p, f64=0, strides=st, pts3d=p, weights=None, kind=_abi.POSES_W_NONE, K=p, kpi=0, vs=None, b=4, nk=3, pn=9, iters=200,
             rt=p, poses=None, status=None):
        return lib.pvnet_pose_solve_classes(pts2d, f64, strides, pts3d, weights, kind, K, kpi, vs, b, nk, pn, iters, rt, poses, status, None)

    for name in ("pts2d", "strides", "pts3d", "K"):
        assert call(**{name: None}) == BADARG, name
    assert call(rt=None, poses=None) == BADARG                     # nothing to write
    assert call(b=-1) == BADARG and call(iters=0) == BADARG and call(iters=-5) == BADARG
    assert call(nk=0) == BADARG and call(nk=-2) == BADARG
    assert call(kind=3) == BADARG and call(kind=-1) == BADARG
    assert call(kind=_abi.POSES_W_EXPLICIT) == BADARG and call(kind=_abi.POSES_W_COV_F32) == BADARG   # a kind without weights
    assert call(pn=5) == UNSUPPORTED and call(pn=65) == UNSUPPORTED
    assert call(nk=_abi.POSES_MAX_CLASSES + 1) == UNSUPPORTED
    assert call(b=_abi.POSES_MAX_ITEMS // 63 + 1, nk=63) == UNSUPPORTED and call(b=2 ** 31 - 1, nk=2) == UNSUPPORTED   # b nk beyond the index range
    assert call(b=0) == 0 and call(b=0, vs=p, poses=p, status=p) == 0   # nothing to do, nothing enqueued
    assert call(b=0, nk=0) == BADARG and call(b=0, pn=5) == UNSUPPORTED  # checked all the same


def test_the_shared_solver_is_one_header_two_libraries_depend_on():
    assert os.path.exists(CORE) and CORE in build.DEPS
    assert {n for n in build.SIDE_LIBRARIES if CORE in build._side(n)[1]} == {"poses"}
    assert CORE in build.SIDE_LIBRARIES["poses"][2]
    core = open(CORE).read()
    solve = open(os.path.join(build.CSRC, "pose_solve.hip")).read()
    classes = open(os.path.join(build.CSRC, "pose_classes.hip")).read()
    for name in HELPERS:
        pat = re.escape(name) + (r"\b" if name.startswith("struct") else r"\s*\(")
        assert re.search(pat, core), name
        assert not re.search(pat, solve) and not re.search(pat, classes), name
    for text in (solve, classes):
        assert '#include "pose_core.h"' in text and "PVNET_POSE_KERNEL(" in text
    # the no-contraction rule travels with the header, at file scope and before any code
    pragma = re.search(r"^#pragma clang fp contract\(off\)$", core, re.M)
    assert pragma and pragma.start() < core.index("namespace {") < core.index("struct Shared")
    assert "fp contract" not in re.sub(r"//.*", "", solve) and "fp contract" not in re.sub(r"//.*", "", classes)
    assert "pose_solve_kernel" in solve and "PoseArgs" in solve and 'extern "C" int pvnet_pose_solve(' in solve


def test_python_refusals_need_no_device():
    import torch
    from pvnet_amd import voting
    import pvnet_amd
    assert pvnet_amd.pnp_classes_device is P.pnp_classes_device and pvnet_amd.MultiPoseEvalWrapper is voting.MultiPoseEvalWrapper
    assert {"pnp_classes_device", "MultiPoseEvalWrapper"} <= set(pvnet_amd.__all__)
    X = np.zeros((2, 9, 3))
    good = torch.zeros((3, 2, 9, 2))
    with pytest.raises(RuntimeError, match="CUDA"):
        P.pnp_classes_device(X, good, P.LINEMOD_K)                                   # no CPU fallback
    with pytest.raises(RuntimeError, match="CUDA"):
        P.pnp_classes_device(X, good.numpy(), P.LINEMOD_K)
    for bad in (torch.zeros((3, 9, 2)), torch.zeros((3, 2, 9, 3)), torch.zeros((3, 2, 9, 2), dtype=torch.float16)):
        with pytest.raises(RuntimeError, match=r"\[b,nk,pn,2\]"):
            P.pnp_classes_device(X, bad, P.LINEMOD_K)
    for bad in (np.zeros((3, 9, 3)), np.zeros((2, 8, 3)), np.zeros((9, 3))):
        with pytest.raises(RuntimeError, match=r"points_3d must be \[nk,pn,3\]"):
            P.pnp_classes_device(bad, good, P.LINEMOD_K)
    with pytest.raises(ValueError, match="not both"):
        P.pnp_classes_device(X, good, P.LINEMOD_K, weights_2d=np.zeros((3, 2, 9, 3)), covariance=np.zeros((3, 2, 9, 2, 2)))
    with pytest.raises(RuntimeError, match="same number of object points"):
        P.pnp_classes_device([np.zeros((9, 3)), np.zeros((8, 3))], good, P.LINEMOD_K)
    with pytest.raises(RuntimeError, match="list of nk arrays"):
        P.pnp_classes_device([np.zeros((9, 2)), np.zeros((9, 2))], good, P.LINEMOD_K)
    # the wrapper
    with pytest.raises(RuntimeError, match="same number of object points"):
        voting.MultiPoseEvalWrapper([np.zeros((9, 3)), np.zeros((8, 3))], P.LINEMOD_K)
    with pytest.raises(RuntimeError, match=r"\[nk,pn,3\]"):
        voting.MultiPoseEvalWrapper(np.zeros((9, 3)), P.LINEMOD_K)
    with pytest.raises(RuntimeError, match=r"K must be \[3,3\]"):
        voting.MultiPoseEvalWrapper(X, np.zeros((2, 3, 3)))
    wrap = voting.MultiPoseEvalWrapper([X[0], X[1]], P.LINEMOD_K)
    assert wrap.points_3d.shape == (2, 9, 3)
    sig = inspect.signature(voting.MultiPoseEvalWrapper.__init__)
    assert list(sig.parameters)[1:] == ["points_3d", "K", "round_hyp_num", "inlier_thresh", "max_num", "min_num", "max_iterations"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[3:]] == [512, 0.99, 30000, 5, 200]
    fsig = inspect.signature(voting.MultiPoseEvalWrapper.forward)
    assert [n for n, q in fsig.parameters.items() if q.kind is q.POSITIONAL_OR_KEYWORD][1:] == \
        ["seg_pred_or_labels", "vertex_pred", "use_argmax", "K", "return_all"]
    seg, field = torch.zeros((1, 3, 8, 8)), torch.zeros((1, 18, 8, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        wrap(seg, field)
    with pytest.raises(RuntimeError, match="vn = 9"):
        wrap(seg, torch.zeros((1, 16, 8, 8)))
    with pytest.raises(RuntimeError, match="C = 3"):
        wrap(torch.zeros((1, 4, 8, 8)), field)
    with pytest.raises(RuntimeError, match=r"labels must be \[b,h,w\]"):
        wrap(seg, field, use_argmax=False)


@pytest.mark.parametrize("layout", CC.LAYOUTS)
def test_the_cases_tell_the_classes_apart(layout):
    """On the noise-free cases the host solver with the right table reaches every ground-truth pose within pose_cases.BAR_POSE; with
    another class's points -- class 0's for every item, or the table indexed by the image instead of the class -- every item it gets
    wrong is left with a pose error above BAR_POSE and the device tests' ATOL, and with a reprojection cost far above the right
    table's.  So a kernel that mixes up the table cannot pass tests/test_pose_classes_device.py."""
    b, nk, pn = layout
    X, x2, gt = CC.case(b, nk, pn)
    assert nk == 1 or min(np.abs(np.sort(np.ptp(X[j], 0)) - np.sort(np.ptp(X[k], 0))).max() for j in range(nk) for k in range(j)) > 1e-3
    right, status = CC.host_loop(X, x2, P.LINEMOD_K)
    assert (status >= 0).all() and np.abs(right - gt).max() <= pose_cases.BAR_POSE
    right_cost = CC.reprojection_cost(X, x2, P.LINEMOD_K, right)
    assert right_cost.max() < 1e-12
    mistakes = {"class 0's points for all": lambda i, k: 0, "the table indexed by the image": lambda i, k: i % nk}
    for what, taken in mistakes.items():
        wrong = np.array([[taken(i, k) != k for k in range(nk)] for i in range(b)])
        if not wrong.any():   # a single class, or a single image of class 0 only: the layout cannot show this mistake
            assert nk == 1 or (b == 1 and what.startswith("the table"))
            continue
        poses, _ = CC.host_loop(X, x2, P.LINEMOD_K, points=lambda i, k: X[taken(i, k)])
        err = np.abs(poses - gt).reshape(b, nk, -1).max(-1)
        with np.errstate(all="ignore"):
            cost = CC.reprojection_cost(X, x2, P.LINEMOD_K, poses)
        print(f"{what} {layout}: least pose error of a wrong item {err[wrong].min():.2e}, least cost {np.nanmin(cost[wrong]):.2e}")
        assert (err[wrong] > 1e3 * pose_cases.BAR_POSE).all(), what
        assert not (cost[wrong] <= 1e-6).any(), what      # px^2: the right table's is below 1e-12
        assert np.abs(poses[~wrong] - right[~wrong]).max() == 0.0
