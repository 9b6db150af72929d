"""CPU-only checks of the targets of several objects (include/pvnet_class_targets.h, libpvnet_class_targets.so): every bad argument
rejected with the documented code before any HIP call, the register rule for every kernel, the one copy of kp_target and the two
libraries that compile it, the float64 restatement (tests/class_targets_restatement.py) against what the reference recorded at one
class and against a per-class composition of the single-class restatement on every label builder -- with four planted mistakes that
the comparison must catch --, and the Python entries' refusal of host tensors.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build
from tests import class_targets_cases as CASES
from tests.class_targets_restatement import class_weight_scale, vertex_targets_classes_f64
from tests.targets_restatement import vertex_targets_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_class_targets.h")).read()
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
EXPORTS = {"pvnet_class_targets_abi_version", "pvnet_vertex_targets_classes", "pvnet_head_metrics_ckp",
           "pvnet_head_metrics_ckp_workspace_bytes", "pvnet_head_grad_ckp", "pvnet_head_grad_ckp_workspace_bytes"}
KERNELS = ("vertex_targets_classes_kernel", "head_partial_ckp_kernel", "head_partial_ckp_general_kernel", "head_final_ckp_kernel",
           "head_grad_ckp_wsum_kernel", "head_grad_ckp_final_kernel", "head_grad_ckp_kernel", "head_grad_ckp_general_kernel",
           "head_grad_ckp_status_kernel")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vertex_targets.npz")
KP_TARGET_BODY = "sqrt(vx * vx + vy * vy)"   # the line of kp_target that nothing else in the project has a reason to hold


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_class_targets_library()


def test_header_table_and_limits():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS == set(_abi.CLASS_TARGETS_PROTOTYPES)
    # the fused calls take the single-class calls' arguments, type for type; the targets call takes class_num behind weight_scale
    assert _abi.CLASS_TARGETS_PROTOTYPES["pvnet_head_metrics_ckp"] == _abi.TARGETS_PROTOTYPES["pvnet_head_metrics_kp"]
    assert _abi.CLASS_TARGETS_PROTOTYPES["pvnet_head_grad_ckp"] == _abi.TARGETS_PROTOTYPES["pvnet_head_grad_kp"]
    one, many = _abi.TARGETS_PROTOTYPES["pvnet_vertex_targets"][1], _abi.CLASS_TARGETS_PROTOTYPES["pvnet_vertex_targets_classes"][1]
    assert many == one[:5] + [C.c_int] + one[5:]
    decl = re.search(r"^int pvnet_vertex_targets_classes\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    assert "weight_scale" in decl[4] and decl[5].strip() == "int class_num"
    defines = dict(re.findall(r"^#define\s+(PVNET_\w+)\s+(\d+)", HDR, re.M))
    assert defines == {"PVNET_CLASS_TARGETS_ABI_VERSION": "1", "PVNET_CLASS_TARGETS_MAX_CLASSES": "64", "PVNET_CLASS_TARGETS_MAX_TABLE": "1024"}
    assert _abi.CLASS_TARGETS_MAX_CLASSES == 64 == _abi.CLASSES_MAX and _abi.CLASS_TARGETS_MAX_TABLE == 1024
    assert 63 * 16 <= _abi.CLASS_TARGETS_MAX_TABLE and 13 * 78 <= _abi.CLASS_TARGETS_MAX_TABLE
    assert '#include "pvnet_targets.h"' in HDR   # PVNET_TARGETS_F_MOTION, the head's flags and codes: by value, not defined again
    # the registry: a row of its own, in both tables at the same place, not the last one
    names = list(build.SIDE_LIBRARIES)
    assert names == list(_abi.SIDE_LIBRARIES) and "class_targets" in names and names[-1] == "texture"
    assert build.SIDE_LIBRARIES["class_targets"][:2] == (["class_targets.hip"], "pvnet_class_targets.h")
    assert build.SIDE_LIBRARIES["targets"][0] == ["head_targets.hip"]


def test_library_is_built_and_its_workspaces_are_the_single_class_ones(lib):
    assert lib.pvnet_class_targets_abi_version() == _abi.CLASS_TARGETS_ABI_VERSION == 1
    blob = open(_abi.CLASS_TARGETS_LIB_PATH, "rb").read()
    assert b"gfx950" in blob and all(k.encode() in blob for k in KERNELS)
    one = _abi.load_targets_library()
    for b, h, w in ((1, 480, 640), (32, 480, 640), (1, 1, 1), (3, 37, 53)):
        assert lib.pvnet_head_metrics_ckp_workspace_bytes(b, h, w) == one.pvnet_head_metrics_kp_workspace_bytes(b, h, w) > 0
        assert lib.pvnet_head_grad_ckp_workspace_bytes(b, h, w) == one.pvnet_head_grad_kp_workspace_bytes(b, h, w) > 0
    for ws in (lib.pvnet_head_metrics_ckp_workspace_bytes, lib.pvnet_head_grad_ckp_workspace_bytes):
        assert ws(0, 480, 640) == 0 and ws(4, 0, 640) == 0 and ws(4, 480, 0) == 0 and ws(65536, 8, 8) == 0
        assert ws(1, 1 << 16, 1 << 16) == 0


def test_bad_arguments_are_rejected_without_a_device(lib):
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    s4, s3 = (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 3)(1, 1, 1)
    U8, I16, I32, I64, F32 = 0, 1, 2, 3, 4

    def targets(mask=p, mdt=I64, ms=s3, hc=p, wsc=None, cn=4, b=4, h=96, w=128, vn=9, flags=0, vt=p, ts=s4, vw=p, wstr=s3):
        return lib.pvnet_vertex_targets_classes(mask, mdt, ms, hc, wsc, cn, b, h, w, vn, flags, vt, ts, vw, wstr, None)

    for name in ("mask", "ms", "hc", "ts", "wstr"):
        assert targets(**{name: None}) == BADARG, name
    assert targets(vt=None, vw=None) == BADARG and targets(vt=None, vw=None, ts=None, wstr=None) == BADARG   # nothing asked for
    assert targets(vn=0) == BADARG and targets(vn=-1) == BADARG
    assert targets(b=-1) == BADARG and targets(h=0) == BADARG and targets(w=0) == BADARG
    assert targets(flags=1) == BADARG and targets(flags=128) == BADARG     # only the motion flag is known here
    assert targets(mdt=99) == BADARG and targets(mdt=-1) == BADARG
    assert targets(mdt=I16) == UNSUPPORTED and targets(mdt=F32) == UNSUPPORTED
    assert targets(b=65536) == UNSUPPORTED and targets(h=1 << 16, w=1 << 16) == UNSUPPORTED
    # the class count: 2 .. 64, and a table of at most 1 024 key-points
    assert targets(cn=1) == BADARG and targets(cn=0) == BADARG and targets(cn=-5) == BADARG and targets(cn=65) == BADARG
    assert targets(cn=65, b=0) == BADARG and targets(cn=1, b=0) == BADARG
    assert targets(cn=64, vn=17) == UNSUPPORTED and targets(cn=14, vn=79) == UNSUPPORTED and targets(cn=2, vn=1025) == UNSUPPORTED
    for cn, vn in ((2, 9), (64, 16), (14, 78), (2, 1024), (64, 2), (3, 17)):
        assert targets(cn=cn, vn=vn, b=0) == 0, (cn, vn)
    for mdt in (U8, I32, I64):
        for flags in (0, _abi.TARGETS_F_MOTION):
            assert targets(mdt=mdt, b=0, flags=flags) == 0                 # nothing to do, nothing enqueued
    assert targets(b=0, vt=None, ts=None) == 0 and targets(b=0, vw=None, wstr=None) == 0 and targets(b=0, wsc=p) == 0

    def metrics(seg=p, ss=s4, nc=4, vp=p, vs=s4, hc=p, wsc=None, mask=p, mdt=I64, ms=s3, b=4, h=96, w=128, vn=9, sigma=1.0, flags=0,
                losses=p, counts=p, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_head_metrics_ckp_workspace_bytes(max(b, 1), max(h, 1), max(w, 1))
        return lib.pvnet_head_metrics_ckp(seg, ss, nc, vp, vs, hc, wsc, mask, mdt, ms, b, h, w, vn, sigma, flags, losses, counts, status,
                                          ws, wsb, None)

    def grad(seg=p, ss=s4, nc=4, vp=p, vs=s4, hc=p, wsc=None, mask=p, mdt=I64, ms=s3, b=4, h=96, w=128, vn=9, sigma=1.0, flags=0,
             up=p, gs=p, gss=s4, gv=p, gvs=s4, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_head_grad_ckp_workspace_bytes(max(b, 1), max(h, 1), max(w, 1))
        return lib.pvnet_head_grad_ckp(seg, ss, nc, vp, vs, hc, wsc, mask, mdt, ms, b, h, w, vn, sigma, flags, up, gs, gss, gv, gvs,
                                       status, ws, wsb, None)

    for call, small in ((metrics, lib.pvnet_head_metrics_ckp_workspace_bytes(4, 96, 128)),
                        (grad, lib.pvnet_head_grad_ckp_workspace_bytes(4, 96, 128))):
        for name in ("seg", "ss", "vp", "vs", "hc", "mask", "ms"):
            assert call(**{name: None}) == BADARG, (call.__name__, name)
        assert call(nc=1) == BADARG and call(nc=0) == BADARG and call(nc=65) == BADARG and call(nc=65, b=0) == BADARG
        assert call(nc=64, vn=17) == UNSUPPORTED and call(nc=14, vn=79) == UNSUPPORTED
        assert call(nc=64, vn=16, b=0) == 0 and call(nc=14, vn=78, b=0) == 0 and call(nc=2, b=0) == 0
        assert call(b=-1) == BADARG and call(h=0) == BADARG and call(w=0) == BADARG
        assert call(vn=0) == BADARG and call(vn=-3) == BADARG
        assert call(sigma=0.0) == BADARG and call(sigma=-1.0) == BADARG and call(sigma=float("nan")) == BADARG
        assert call(sigma=float("inf")) == BADARG
        assert call(flags=128) == BADARG                                   # an unknown flag
        assert call(flags=1 | 2) == BADARG and call(flags=4 | 8) == BADARG and call(flags=16 | 32) == BADARG
        assert call(mdt=99) == BADARG and call(mdt=-1) == BADARG
        assert call(mdt=I16) == UNSUPPORTED and call(mdt=F32) == UNSUPPORTED
        assert call(ws=C.c_void_p(0x2004)) == BADARG                       # misaligned workspace
        assert call(ws=None) == WORKSPACE
        assert call(wsb=small - 1) == WORKSPACE and call(b=8, wsb=small) == WORKSPACE
        assert call(b=65536) == UNSUPPORTED
        assert call(h=1 << 16, w=1 << 16) == UNSUPPORTED
        for mdt in (U8, I32, I64):
            assert call(mdt=mdt, b=0, ws=None, wsb=0) == 0
        for flags in (1, 2, 4, 8, 1 | 8, 2 | 4, 16, 32, 64, 64 | 1 | 4 | 16):   # the head's flags and the motion flag
            assert call(flags=flags, b=0) == 0
        assert call(wsc=p, b=0) == 0
    assert metrics(losses=None) == BADARG and metrics(counts=None) == BADARG
    assert grad(gs=None, gv=None) == BADARG and grad(up=None) == BADARG
    assert grad(gss=None) == BADARG and grad(gvs=None) == BADARG           # a gradient without its strides
    assert grad(gs=None, gss=None, b=0) == 0 and grad(gv=None, gvs=None, b=0) == 0
    assert grad(gs=None, gss=None, ws=None) == WORKSPACE and grad(gv=None, gvs=None, ws=None) == WORKSPACE


def test_register_check_covers_the_new_translation_unit(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as chk
    (src, text), = chk.side_assembly("class_targets")
    assert src.endswith("class_targets.hip")
    ks = chk.kernels(text)
    for k in KERNELS:
        assert any(k in name for name, _, _, _ in ks), k
    assert len(ks) == 27   # as libpvnet_targets.so: nine kernels, the two fast per-pixel ones in 3 element types x 3 load policies
    for name, nfv, vmax, scratch in ks:
        assert nfv - (vmax + 1) >= chk.SLACK and scratch == 0, name
        assert "ClassKpSource" in name or "ClassTargetArgs" in name, name
    # the fused forward on float32 predictions stays in head_partial_kp_kernel's class: four waves per SIMD
    for name, nfv, _, _ in ks:
        if "head_partial_ckp_kernelILi0E" in name:
            assert 512 // ((nfv + 7) // 8 * 8) == 4, (name, nfv)
    # no other library holds a kernel of these names
    for other in build.SIDE_LIBRARIES:
        if other != "class_targets":
            blob = open(_abi.SIDE_LIBRARIES[other].path, "rb").read()
            assert not any(k.encode() in blob for k in KERNELS), other


def test_one_copy_of_the_target_shared_by_the_two_libraries_alone():
    shared = os.path.join(build.CSRC, "kp_target.h")
    assert os.path.exists(shared)
    users = {n for n in build.SIDE_LIBRARIES if shared in build._side(n)[1]}
    assert users == {"targets", "class_targets"}
    assert shared not in build.DEPS
    # kp_target's body occurs in exactly one file among what the two libraries are made of
    files = sorted(set(build._side("targets")[1]) | set(build._side("class_targets")[1]))
    assert [f for f in files if KP_TARGET_BODY in open(f).read()] == [shared]
    text = open(shared).read()
    assert len(re.findall(r"\bvoid kp_target\(", text)) == 1 and len(re.findall(r"\bfloat kp_weight\(", text)) == 1
    for tu in ("head_targets.hip", "class_targets.hip"):
        src = open(os.path.join(build.CSRC, tu)).read()
        assert '#include "kp_target.h"' in src and "kp_target(" in src and not re.search(r"\bvoid kp_target\(", src)
    assert "contract(off)" in text   # the definition carries its own rounding rule


def test_restatement_at_one_class_equals_the_reference_bit_for_bit():
    """nk = 1 against what the reference's own compute_vertex_hcoords returned (tests/golden/vertex_targets.npz): the targets bit for
    bit on every case, mask values of 2 included (no target there, here as there); the weights wherever the mask is 0 or 1, and 0
    where the reference's mask.float() gives 2 -- the one deliberate difference"""
    g = np.load(GOLDEN)
    names = [str(n) for n in g["cases"]]
    assert len(names) >= 5
    seen_two = False
    for n in names:
        mask, hc = g[n + ".mask"], g[n + ".hcoords"]
        for key, motion in (("ref", False), ("ref_motion", True)):
            ref = np.ascontiguousarray(np.transpose(g[f"{n}.{key}"], (2, 0, 1)))
            got, weights = vertex_targets_classes_f64(mask[None], hc[None, None], use_motion=motion)
            assert got.dtype == np.float32 and np.array_equal(CASES.bits(got[0]), CASES.bits(ref)), (n, key)
            one, wone = vertex_targets_f64(mask[None], hc[None], use_motion=motion)
            assert np.array_equal(CASES.bits(got), CASES.bits(one))
            binary = (mask == 0) | (mask == 1)
            assert np.array_equal(weights[0, 0][binary], wone[0, 0][binary]) and np.all(weights[0, 0][~binary] == 0.0)
            seen_two |= bool((wone[0, 0][~binary] == 2.0).any())
    assert seen_two


def compose(labels, hc, weight_scale, motion, mistake=None):
    """the per-class composition of the single-class restatement, written apart from tests/class_targets_restatement.py (indexed
    assignment, not np.where) -- and with one of four mistakes planted on request"""
    b, h, w = labels.shape
    nk, vn = hc.shape[1], hc.shape[2]
    ws = class_weight_scale(weight_scale, b, nk)
    lab = np.where(labels >= nk + 1, nk, labels) if mistake == "clamp" else labels
    vertex, weights = np.zeros((b, 2 * vn, h, w), np.float32), np.zeros((b, 1, h, w), np.float32)
    for k in range(nk):
        own = lab == k + 1
        row = (k + 1) % nk if mistake == "row" else k          # class l reads hcoords[l] instead of hcoords[l - 1]
        v, _ = vertex_targets_f64(own.astype(np.int64), hc[:, row], None, motion)
        if mistake == "add":
            vertex = vertex + v
        else:
            sel = np.broadcast_to(own[:, None], vertex.shape)
            vertex[sel] = v[sel]
        for i in range(b):
            weights[i, 0][own[i]] = np.float32(k + 1) if mistake == "weight" else ws[i, k]
    return vertex, weights


def equal_bits(a, c):
    return np.array_equal(CASES.bits(a[0]), CASES.bits(c[0])) and np.array_equal(CASES.bits(a[1]), CASES.bits(c[1]))


@pytest.mark.parametrize("builder", sorted(CASES.BUILDERS))
@pytest.mark.parametrize("class_num,vn", [(2, 9), (4, 4), (14, 3)])
def test_restatement_equals_the_per_class_composition(builder, class_num, vn):
    b, h, w = 3, 24, 40
    labels = CASES.BUILDERS[builder](b, h, w, class_num)
    hc = CASES.class_keypoints(labels, class_num, vn, seed=class_num + vn, minus_zero=True)
    scale = np.linspace(-0.5, 1.5, b * (class_num - 1)).astype(np.float32).reshape(b, class_num - 1)
    for motion in (False, True):
        for ws in (None, scale[:, 0].copy(), scale):
            got = vertex_targets_classes_f64(labels, hc, ws, motion)
            assert got[0].dtype == np.float32 and got[1].dtype == np.float32
            assert equal_bits(got, compose(labels, hc, ws, motion)), (builder, motion)
            fg = (labels >= 1) & (labels < class_num)
            assert np.all(CASES.bits(got[0])[np.broadcast_to(~fg[:, None], got[0].shape)] == 0)   # +0.0, not -0.0
            assert np.all(CASES.bits(got[1])[~fg[:, None]] == 0)
    if builder == "absent" and class_num > 2:
        assert not (labels == class_num - 1).any()
    if builder == "planted":
        assert all((labels == v).any() for v in (0, -1, class_num, 255))
    if builder == "empty":
        assert not labels[1].any() and labels[0].any()


@pytest.mark.parametrize("mistake", ["row", "weight", "clamp", "add"])
def test_planted_mistakes_fail_the_comparison_on_the_stripe_images(mistake):
    b, h, w, class_num, vn = 2, 16, 40, 4, 4
    caught = {}
    for name in ("stripes3", "stripes5", "planted"):   # (`planted` is the period-5 stripes with labels outside the classes)
        labels = CASES.BUILDERS[name](b, h, w, class_num)
        hc = CASES.class_keypoints(labels, class_num, vn, seed=7, minus_zero=True)
        right = vertex_targets_classes_f64(labels, hc)
        assert equal_bits(right, compose(labels, hc, None, False))
        if mistake == "add":   # the case holds a target of -0.0, which a sum with another class's +0.0 loses
            assert (CASES.bits(right[0]) == 0x80000000).any()
        caught[name] = not equal_bits(right, compose(labels, hc, None, False, mistake))
    # labels >= class_num exist on the planted image only; every other mistake shows on each stripe image
    assert caught["planted"] and (mistake == "clamp" or all(caught.values())), (mistake, caught)
    assert mistake != "clamp" or not (caught["stripes3"] or caught["stripes5"])


def test_python_entries_refuse_host_tensors():
    import torch
    from pvnet_amd import validation as V
    seg, vp = torch.zeros((1, 3, 8, 8), requires_grad=True), torch.zeros((1, 4, 8, 8), requires_grad=True)
    labels, hc = torch.zeros((1, 8, 8), dtype=torch.int64), torch.zeros((1, 2, 2, 3), dtype=torch.float64)
    up = torch.ones((1, 2), dtype=torch.float64)
    packed = torch.zeros((1, 7, 8, 8), requires_grad=True)
    for call in (lambda: V.vertex_targets_classes_device(labels, hc),
                 lambda: V.head_metrics_from_class_keypoints(seg, vp, labels, hc),
                 lambda: V.head_grad_from_class_keypoints(seg, vp, labels, hc, up),
                 lambda: V.HeadMetrics().from_class_keypoints(seg, vp, labels, hc),
                 lambda: V.HeadLoss().from_class_keypoints(seg, vp, labels, hc),
                 lambda: V.HeadLoss().packed_from_class_keypoints(packed, 3, labels, hc)):
        with pytest.raises(RuntimeError, match="CUDA tensor \\(there is no CPU fallback\\)"):   # the siblings' message
            call()
