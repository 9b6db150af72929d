"""CPU-only checks of the targets from key-points (include/pvnet_targets.h, libpvnet_targets.so): the header's exports against the
prototype table of pvnet_amd/_abi.py, the built library, every bad argument rejected with the documented code before any HIP call,
the register rule for every new kernel, the Python entries' refusal of host tensors, and the float64 restatement against what the
reference's own compute_vertex_hcoords returned (tests/golden/vertex_targets.npz), bit for bit.
What holds for every side library alike (header against table, the built library's symbols, the register tool's selection, the loud
failure without it) is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_targets.h")).read()
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
EXPORTS = {"pvnet_targets_abi_version", "pvnet_vertex_targets", "pvnet_head_metrics_kp", "pvnet_head_metrics_kp_workspace_bytes",
           "pvnet_head_grad_kp", "pvnet_head_grad_kp_workspace_bytes"}
KERNELS = ("vertex_targets_kernel", "head_partial_kp_kernel", "head_partial_kp_general_kernel", "head_final_kp_kernel",
           "head_grad_kp_wsum_kernel", "head_grad_kp_final_kernel", "head_grad_kp_kernel", "head_grad_kp_general_kernel",
           "head_grad_kp_status_kernel")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vertex_targets.npz")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_targets_library()


def test_header_declares_the_exports_and_every_one_has_a_prototype():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS
    # byte counts are size_t, in and out
    assert _abi.TARGETS_PROTOTYPES["pvnet_head_metrics_kp_workspace_bytes"][0] is C.c_size_t
    assert _abi.TARGETS_PROTOTYPES["pvnet_head_grad_kp_workspace_bytes"][0] is C.c_size_t
    for name, pos in (("pvnet_head_metrics_kp", -2), ("pvnet_head_grad_kp", -2)):
        decl = re.search(r"^int %s\s*\((.*?)\);" % name, HDR, re.M | re.S).group(1).split(",")
        assert "size_t workspace_bytes" in decl[pos] and _abi.TARGETS_PROTOTYPES[name][1][pos] is C.c_size_t
    # the fused calls take the head's arguments with the target and the weights (4 arguments) replaced by hcoords and weight_scale (2)
    head, kp = _abi.HEAD_PROTOTYPES["pvnet_head_metrics"][1], _abi.TARGETS_PROTOTYPES["pvnet_head_metrics_kp"][1]
    assert len(kp) == len(head) - 2 and kp[:5] == head[:5] and kp[7:] == head[9:]
    grad, kpg = _abi.TRAIN_PROTOTYPES["pvnet_head_grad"][1], _abi.TARGETS_PROTOTYPES["pvnet_head_grad_kp"][1]
    assert len(kpg) == len(grad) - 2 and kpg[:5] == grad[:5] and kpg[7:] == grad[9:]
    assert kp[14] is C.c_double and kpg[14] is C.c_double   # sigma
    # it defines only what is new and includes pvnet_head.h for the rest
    assert re.findall(r"^#define\s+(PVNET_\w+)\s+\d+", HDR, re.M) == ["PVNET_TARGETS_ABI_VERSION", "PVNET_TARGETS_F_MOTION"]
    assert '#include "pvnet_head.h"' in HDR
    motion = int(re.search(r"^#define\s+PVNET_TARGETS_F_MOTION\s+(\d+)", HDR, re.M).group(1))
    assert motion == _abi.TARGETS_F_MOTION
    head_flags = [int(v) for v in re.findall(r"^#define\s+PVNET_HEAD_F_\w+\s+(\d+)", open(os.path.join(ROOT, "include", "pvnet_head.h")).read(), re.M)]
    assert all(motion & f == 0 for f in head_flags)   # the new flag collides with none of the head's


def test_library_is_built_for_gfx950_and_exports_the_symbols(lib):
    assert lib.pvnet_targets_abi_version() == _abi.TARGETS_ABI_VERSION == 1
    blob = open(_abi.TARGETS_LIB_PATH, "rb").read()
    assert all(k.encode() in blob for k in KERNELS)
    tu = {n: build.SIDE_LIBRARIES[n][0] for n in ("head", "train", "targets")}
    assert tu["targets"] == ["head_targets.hip"]
    assert not set(tu["targets"]) & (set(build.VOTE_TU) | set(tu["head"]) | set(tu["train"]))
    assert tu["head"] == ["head_metrics.hip"] and tu["train"] == ["head_grad.hip"]   # the other libraries' shapes have not moved


def test_workspace_bytes(lib):
    head, train = _abi.load_head_library(), _abi.load_train_library()
    for b, h, w in ((1, 480, 640), (32, 480, 640), (1, 1, 1), (3, 37, 53)):   # the same records as the calls they mirror
        assert lib.pvnet_head_metrics_kp_workspace_bytes(b, h, w) == head.pvnet_head_metrics_workspace_bytes(b, h, w) > 0
        assert lib.pvnet_head_grad_kp_workspace_bytes(b, h, w) == train.pvnet_head_grad_workspace_bytes(b, h, w) > 0
    for ws in (lib.pvnet_head_metrics_kp_workspace_bytes, lib.pvnet_head_grad_kp_workspace_bytes):
        assert ws(0, 480, 640) == 0 and ws(4, 0, 640) == 0 and ws(4, 480, 0) == 0 and ws(65536, 8, 8) == 0
        assert ws(1, 1 << 16, 1 << 16) == 0 and ws(1, 32768, 32768) >= (1 << 20)


def test_bad_arguments_are_rejected_without_a_device(lib):
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    s4, s3 = (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 3)(1, 1, 1)
    U8, I16, I32, I64, F32 = 0, 1, 2, 3, 4

    def targets(mask=p, mdt=I64, ms=s3, hc=p, wsc=None, b=4, h=96, w=128, vn=9, flags=0, vt=p, ts=s4, vw=p, wstr=s3):
        return lib.pvnet_vertex_targets(mask, mdt, ms, hc, wsc, b, h, w, vn, flags, vt, ts, vw, wstr, None)

    for name in ("mask", "ms", "hc", "ts", "wstr"):
        assert targets(**{name: None}) == BADARG, name
    assert targets(vt=None, vw=None) == BADARG and targets(vt=None, vw=None, ts=None, wstr=None) == BADARG   # nothing asked for
    assert targets(vn=0) == BADARG and targets(vn=-1) == BADARG
    assert targets(b=-1) == BADARG and targets(h=0) == BADARG and targets(w=0) == BADARG
    assert targets(flags=1) == BADARG and targets(flags=128) == BADARG     # only the motion flag is known here
    assert targets(mdt=99) == BADARG and targets(mdt=-1) == BADARG
    assert targets(mdt=I16) == UNSUPPORTED and targets(mdt=F32) == UNSUPPORTED
    assert targets(b=65536) == UNSUPPORTED and targets(h=1 << 16, w=1 << 16) == UNSUPPORTED
    for mdt in (U8, I32, I64):
        for flags in (0, _abi.TARGETS_F_MOTION):
            assert targets(mdt=mdt, b=0, flags=flags) == 0                 # nothing to do, nothing enqueued
    assert targets(b=0, vt=None, ts=None) == 0 and targets(b=0, vw=None, wstr=None) == 0 and targets(b=0, wsc=p) == 0

    def metrics(seg=p, ss=s4, nc=2, vp=p, vs=s4, hc=p, wsc=None, mask=p, mdt=I64, ms=s3, b=4, h=96, w=128, vn=9, sigma=1.0, flags=0,
                losses=p, counts=p, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_head_metrics_kp_workspace_bytes(max(b, 1), max(h, 1), max(w, 1))
        return lib.pvnet_head_metrics_kp(seg, ss, nc, vp, vs, hc, wsc, mask, mdt, ms, b, h, w, vn, sigma, flags, losses, counts, status,
                                         ws, wsb, None)

    def grad(seg=p, ss=s4, nc=2, vp=p, vs=s4, hc=p, wsc=None, mask=p, mdt=I64, ms=s3, b=4, h=96, w=128, vn=9, sigma=1.0, flags=0,
             up=p, gs=p, gss=s4, gv=p, gvs=s4, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_head_grad_kp_workspace_bytes(max(b, 1), max(h, 1), max(w, 1))
        return lib.pvnet_head_grad_kp(seg, ss, nc, vp, vs, hc, wsc, mask, mdt, ms, b, h, w, vn, sigma, flags, up, gs, gss, gv, gvs,
                                      status, ws, wsb, None)

    for call, small in ((metrics, lib.pvnet_head_metrics_kp_workspace_bytes(4, 96, 128)), (grad, lib.pvnet_head_grad_kp_workspace_bytes(4, 96, 128))):
        for name in ("seg", "ss", "vp", "vs", "hc", "mask", "ms"):
            assert call(**{name: None}) == BADARG, (call.__name__, name)
        assert call(nc=1) == BADARG and call(nc=0) == BADARG
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
    (src, text), = chk.side_assembly("targets")
    assert src.endswith("head_targets.hip")
    ks = chk.kernels(text)
    for k in KERNELS:
        assert any(k in name for name, _, _, _ in ks), k
    assert len(ks) >= len(KERNELS)
    for name, nfv, vmax, scratch in ks:
        assert nfv - (vmax + 1) >= chk.SLACK and scratch == 0, name
    # the two head libraries hold none of these kernels
    for other in ("head", "train"):
        assert not any("_kp_" in name for _, asm in chk.side_assembly(other) for name, _, _, _ in chk.kernels(asm))


def test_python_entries_refuse_host_tensors():
    import torch
    from pvnet_amd import validation as V
    seg, vp = torch.zeros((1, 2, 8, 8), requires_grad=True), torch.zeros((1, 4, 8, 8), requires_grad=True)
    mask, hc = torch.zeros((1, 8, 8), dtype=torch.int64), torch.zeros((1, 2, 3), dtype=torch.float64)
    up = torch.ones((1, 2), dtype=torch.float64)
    packed = torch.zeros((1, 6, 8, 8), requires_grad=True)
    for call in (lambda: V.vertex_targets_device(mask, hc),
                 lambda: V.head_metrics_from_keypoints(seg, vp, mask, hc),
                 lambda: V.head_grad_from_keypoints(seg, vp, mask, hc, up),
                 lambda: V.HeadMetrics().from_keypoints(seg, vp, mask, hc),
                 lambda: V.HeadLoss().from_keypoints(seg, vp, mask, hc),
                 lambda: V.HeadLoss().packed_from_keypoints(packed, 2, mask, hc)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
    assert callable(V.ValStep.enqueue_from_keypoints)
    src = open(os.path.join(ROOT, "pvnet_amd", "validation.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M)


def test_restatement_equals_the_reference_bit_for_bit():
    """tests/targets_restatement.py against what the reference's own compute_vertex_hcoords returned for the fixture's inputs, with
    use_motion off and on: np.array_equal on float32 (NaN-free inputs), not a tolerance -- every float64 operation of the formula is
    correctly rounded in numpy on both sides and the float32 rounding happens once."""
    from tests.targets_restatement import vertex_targets_f64
    g = np.load(GOLDEN)
    names = [str(n) for n in g["cases"]]
    assert len(names) >= 5
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz") and f != "vertex_targets.npz")
    assert os.path.getsize(GOLDEN) <= largest
    seen = dict(two=False, n_zero=False, n_tiny=False, hz_zero=False, hz_other=False, outside=False, empty=False, odd=False, f32=False)
    for n in names:
        mask, hc = g[n + ".mask"], g[n + ".hcoords"]
        h, w = mask.shape
        vn = hc.shape[0]
        for key, motion in (("ref", False), ("ref_motion", True)):
            ref = np.transpose(g[f"{n}.{key}"], (2, 0, 1))   # the loader's permute(2, 0, 1)
            got, weights = vertex_targets_f64(mask[None], hc[None], use_motion=motion)
            assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == (1, 2 * vn, h, w)
            assert not np.isnan(ref).any()
            assert np.array_equal(got[0], ref), (n, key)
            assert np.array_equal(weights[0, 0], mask.astype(np.float32))   # mask.float(), linemod_dataset.py:227
            assert np.all(got[0][:, mask != 1] == 0.0)
        # what the case is there for
        hc64 = hc.astype(np.float64)
        ys, xs = np.nonzero(mask == 1)
        seen["two"] |= bool((mask == 2).any())
        seen["empty"] |= len(ys) == 0
        seen["odd"] |= (h * w) % 8 != 0
        seen["f32"] |= hc.dtype == np.float32
        seen["hz_zero"] |= bool((hc64[:, 2] == 0).any())
        seen["hz_other"] |= bool(((hc64[:, 2] != 0) & (hc64[:, 2] != 1)).any())
        for hx, hy, hz in hc64:
            if len(ys):
                nrm = np.sqrt((hx - xs * hz) ** 2 + (hy - ys * hz) ** 2)
                seen["n_zero"] |= bool((nrm == 0).any())
                seen["n_tiny"] |= bool(((nrm > 0) & (nrm < 1e-3)).any())
            if hz == 1:
                seen["outside"] |= not (0 <= hx < w and 0 <= hy < h)
    assert all(seen.values()), seen
    # n = 0 gives 0 / 1e-3 = 0, and 0 < n < 1e-3 gives a vector shorter than 1: both differ from a plain normalisation
    ref = np.transpose(g["values_012_near_keypoints.ref"], (2, 0, 1))
    assert ref[0, 6, 8] == 0.0 and ref[1, 6, 8] == 0.0
    assert 0.3 < ref[2, 5, 9] < 0.34 and ref[3, 5, 9] == 0.0   # 5e-4 / (5e-4 + 1e-3) = 1 / 3


def test_restatement_weight_scale_two_columns_and_nan():
    from tests.targets_restatement import vertex_targets_f64
    mask = np.array([[[0, 1, 2], [1, 1, 0]], [[1, 0, 0], [0, 0, 3]]])
    hc = np.array([[[1.0, 1.0, 1.0], [5.0, -2.0, 1.0]], [[np.nan, 0.0, 1.0], [2.0, 2.0, 1.0]]])
    v, wgt = vertex_targets_f64(mask, hc, weight_scale=np.array([0.0, 0.5], np.float32))
    assert np.all(wgt[0] == 0.0) and np.array_equal(wgt[1, 0], np.array([[0.5, 0, 0], [0, 0, 1.5]], np.float32))
    assert np.isnan(v[1, 0, 0, 0]) and np.isnan(v[1, 1, 0, 0]) and int(np.isnan(v).sum()) == 2   # only that image's mask == 1 pixel
    v2, _ = vertex_targets_f64(mask, hc[:, :, :2])   # [b,vn,2] is hz = 1
    assert np.array_equal(v2[0], v[0])
