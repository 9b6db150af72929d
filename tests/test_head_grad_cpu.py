"""CPU-only checks of the head losses' backward (include/pvnet_train.h, libpvnet_train.so): the header's exports against the prototype
table of pvnet_amd/_abi.py, the built library, every bad argument rejected with the documented code before any HIP call, the register
rule, the Python entry's refusal of host tensors, and the float64 restatement against the fixture's recorded columns, the reference's
recorded float32 gradients and a finite difference of the forward's restatement.
What holds for every side library alike (header against table, the built library's symbols, the register tool's selection, the loud
failure without it) is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_train.h")).read()
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
KERNELS = ("head_grad_wsum_kernel", "head_grad_final_kernel", "head_grad_kernel", "head_grad_general_kernel", "head_grad_status_kernel")
GOLDEN = os.path.join(ROOT, "tests", "golden", "head_grad.npz")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_train_library()


def test_header_declares_the_exports_and_every_one_has_a_prototype():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == {"pvnet_train_abi_version", "pvnet_head_grad_workspace_bytes", "pvnet_head_grad"}
    assert _abi.TRAIN_PROTOTYPES["pvnet_head_grad_workspace_bytes"][0] is C.c_size_t   # a byte count is not cut to 32 bits
    args = _abi.TRAIN_PROTOTYPES["pvnet_head_grad"][1]
    decl = re.search(r"^int pvnet_head_grad\s*\((.*?)\);", HDR, re.M | re.S).group(1)
    assert len(args) == 27 and args[25] is C.c_size_t and "size_t workspace_bytes" in decl and args[16] is C.c_double
    # the forward's inputs, in the forward's order and types
    assert args[:18] == _abi.HEAD_PROTOTYPES["pvnet_head_metrics"][1][:18]
    # no second family of flags: the header defines its version and nothing else, and includes pvnet_head.h for the rest
    assert re.findall(r"^#define\s+(PVNET_\w+)\s+\d+", HDR, re.M) == ["PVNET_TRAIN_ABI_VERSION"]
    assert '#include "pvnet_head.h"' in HDR


def test_library_is_built_for_gfx950_and_exports_the_symbols(lib):
    assert lib.pvnet_train_abi_version() == _abi.TRAIN_ABI_VERSION == 1
    blob = open(_abi.TRAIN_LIB_PATH, "rb").read()
    assert all(k.encode() in blob for k in KERNELS)
    assert build.SIDE_LIBRARIES["train"][0] == ["head_grad.hip"]
    assert "head_grad.hip" not in build.VOTE_TU and "head_grad.hip" not in build.SIDE_LIBRARIES["head"][0]
    assert build.SIDE_LIBRARIES["head"][0] == ["head_metrics.hip"]   # the head library's shape has not moved


def test_workspace_bytes(lib):
    ws = lib.pvnet_head_grad_workspace_bytes
    assert ws(0, 480, 640) == 0 and ws(4, 0, 640) == 0 and ws(4, 480, 0) == 0 and ws(65536, 8, 8) == 0
    one = ws(1, 480, 640)
    assert one % 256 == 0 and one >= 16 + 300 * 12       # two coefficients, a float64 sum and a flag per 1 024 pixels
    assert ws(32, 480, 640) >= 32 * (16 + 300 * 12) and ws(32, 480, 640) < (1 << 20)
    assert ws(1, 1, 1) > 0 and ws(1, 32768, 32768) >= (1 << 23)


def test_bad_arguments_are_rejected_without_a_device(lib):
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    s4, s3 = (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 3)(1, 1, 1)
    U8, I16, I32, I64, F32 = 0, 1, 2, 3, 4

    def call(seg=p, ss=s4, nc=2, vp=p, vs=s4, vt=p, ts=s4, vw=p, wstr=s3, mask=p, mdt=I64, ms=s3, b=4, h=96, w=128, vn=9, sigma=1.0,
             flags=0, up=p, gs=p, gss=s4, gv=p, gvs=s4, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_head_grad_workspace_bytes(max(b, 1), max(h, 1), max(w, 1))
        return lib.pvnet_head_grad(seg, ss, nc, vp, vs, vt, ts, vw, wstr, mask, mdt, ms, b, h, w, vn, sigma, flags, up, gs, gss, gv, gvs,
                                   status, ws, wsb, None)

    # the forward's list
    for name in ("seg", "ss", "vp", "vs", "vt", "ts", "vw", "wstr", "mask", "ms"):
        assert call(**{name: None}) == BADARG, name
    assert call(nc=1) == BADARG and call(nc=0) == BADARG          # C >= 2
    assert call(b=-1) == BADARG and call(h=0) == BADARG and call(w=0) == BADARG and call(vn=0) == BADARG
    assert call(sigma=0.0) == BADARG and call(sigma=-1.0) == BADARG and call(sigma=float("nan")) == BADARG
    assert call(sigma=float("inf")) == BADARG
    assert call(flags=64) == BADARG                                # an unknown flag
    assert call(flags=1 | 2) == BADARG and call(flags=4 | 8) == BADARG and call(flags=16 | 32) == BADARG   # two types / policies at once
    assert call(mdt=99) == BADARG and call(mdt=-1) == BADARG
    assert call(mdt=I16) == UNSUPPORTED and call(mdt=F32) == UNSUPPORTED
    assert call(ws=C.c_void_p(0x2004)) == BADARG                   # misaligned workspace
    assert call(ws=None) == WORKSPACE
    assert call(wsb=lib.pvnet_head_grad_workspace_bytes(4, 96, 128) - 1) == WORKSPACE
    assert call(b=8, wsb=lib.pvnet_head_grad_workspace_bytes(4, 96, 128)) == WORKSPACE
    assert call(b=65536) == UNSUPPORTED
    assert call(h=1 << 16, w=1 << 16) == UNSUPPORTED
    for mdt in (U8, I32, I64):
        assert call(mdt=mdt, b=0, ws=None, wsb=0) == 0             # nothing to do, nothing enqueued
    for flags in (1, 2, 4, 8, 1 | 8, 2 | 4, 16, 32):
        assert call(flags=flags, b=0) == 0
    # the backward's own
    assert call(gs=None, gv=None) == BADARG                        # nothing asked for
    assert call(gs=None, gv=None, gss=None, gvs=None) == BADARG
    assert call(up=None) == BADARG
    assert call(gss=None) == BADARG and call(gvs=None) == BADARG   # a gradient without its strides
    assert call(gs=None, gss=None, b=0) == 0 and call(gv=None, gvs=None, b=0) == 0   # one half, its stride array not needed
    assert call(gs=None, gss=None, ws=None) == WORKSPACE and call(gv=None, gvs=None, ws=None) == WORKSPACE   # (valid up to the workspace)


def test_register_check_covers_the_new_translation_unit(lib):
    tool = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as chk
    (src, text), = chk.side_assembly("train")
    assert src.endswith("head_grad.hip")
    ks = chk.kernels(text)
    assert len(ks) >= 5 and all(any(k in name for name, _, _, _ in ks) for k in KERNELS)
    for name, nfv, vmax, scratch in ks:
        assert nfv - (vmax + 1) >= chk.SLACK and scratch == 0, name
    # the rule bites: the gradient kernel with its allocation cut to what it uses is rejected
    name, nfv, vmax, _ = next(k for k in ks if "head_grad_kernel" in k[0])
    i = text.index(".amdhsa_kernel " + name)
    tight = text[:i] + re.sub(r"\.amdhsa_next_free_vgpr \d+", f".amdhsa_next_free_vgpr {vmax + 1}", text[i:], count=1)
    assert any(n == name and f - (v + 1) < chk.SLACK for n, f, v, _ in chk.kernels(tight))
    tight_file = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"head_grad_tight_{os.getpid()}.s")
    try:
        open(tight_file, "w").write(tight)
        r = subprocess.run([sys.executable, tool, tight_file], capture_output=True, text=True)
        assert r.returncode == 1 and "uses its last granule" in r.stdout
    finally:
        os.remove(tight_file)


def test_python_entry_refuses_host_tensors_and_imports_no_oracle():
    import torch
    from pvnet_amd import validation as V
    seg, vp = torch.zeros((1, 2, 8, 8), requires_grad=True), torch.zeros((1, 4, 8, 8), requires_grad=True)
    mask, vt, vw = torch.zeros((1, 8, 8), dtype=torch.int64), torch.zeros((1, 4, 8, 8)), torch.zeros((1, 1, 8, 8))
    up = torch.ones((1, 2), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="CUDA"):
        V.head_grad_device(seg, vp, mask, vt, vw, up)
    with pytest.raises(RuntimeError, match="CUDA"):
        V.HeadLoss()(seg, vp, mask, vt, vw)
    with pytest.raises(RuntimeError, match="CUDA"):
        V.HeadLoss().packed(torch.zeros((1, 6, 8, 8), requires_grad=True), 2, mask, vt, vw)
    src = open(os.path.join(ROOT, "pvnet_amd", "validation.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.delitem(_abi._side_libs, "train", raising=False)
    monkeypatch.setitem(_abi.SIDE_LIBRARIES, "train", _abi.SIDE_LIBRARIES["train"]._replace(path=str(tmp_path / "nope.so")))
    from pvnet_amd import validation as V
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.head_grad_workspace_bytes(1, 8, 8)


def test_restatement_reproduces_the_fixture_and_brackets_the_reference():
    """the float64 restatement the GPU tests compare against IS the one that wrote the fixture's float64 columns, bit for bit; and the
    reference's recorded float32 gradients lie within float32 rounding of it.

    In what sense: per ELEMENT the reference's float32 result may be off by 100 % (its softmax - 1 cancels), so the statement is
    over the tensor's largest entry.  Every reference gradient is a handful of float32 operations on quantities no larger than the
    largest entry's own factors (a probability <= 1; |p|, |t| <= 8 with w^2 sigma^2 <= 4 against a largest entry of w): 32 half-ulps,
    2^-24 each, of the largest entry cover that chain with room, and a wrong formula misses by orders of magnitude more."""
    from tests.head_grad_restatement import head_grad_f64
    g = np.load(GOLDEN)
    names = [str(n) for n in g["cases"]]
    assert {"typical", "boundary", "all_background", "sigma_half_weighted", "tied_logits"} <= set(names)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "head_metrics.npz"))
    for n in names:
        seg = g[n + ".seg_pred"]
        assert seg.shape[0] <= 2 and seg.shape[2] <= 24 and seg.shape[3] <= 32 and g[n + ".vertex_pred"].shape[1] <= 6
        us, uv = g[n + ".upstream_seg"], g[n + ".upstream_vertex"]
        gs, gv, status = head_grad_f64(seg, g[n + ".vertex_pred"], g[n + ".mask"], g[n + ".vertex"], g[n + ".vertex_weights"], us, uv,
                                       float(g[n + ".sigma"]))
        assert gs.tobytes() == g[n + ".f64_grad_seg"].tobytes(), n
        assert gv.tobytes() == g[n + ".f64_grad_vertex"].tobytes(), n
        assert not status.any()
        for ref32, f64 in ((g[n + ".ref32_grad_seg"], gs), (g[n + ".ref32_grad_vertex"], gv)):
            assert ref32.dtype == np.float32 and ref32.shape == f64.shape
            dist = np.abs(ref32.astype(np.float64) - f64).max()
            print(f"{n}: |ref32 - f64| max {dist:.2e} = {dist / max(np.abs(f64).max(), 1e-300) / 2.0 ** -24:.2f} half-ulps of the largest entry")
            assert dist <= 32 * 2.0 ** -24 * np.abs(f64).max(), n
        if seg.shape[0] > 1:
            assert us[0] != us[-1] and uv[0] != uv[-1]   # non-uniform upstream gradients
    assert any(float(g[n + ".sigma"]) != 1.0 for n in names)
    w = g["sigma_half_weighted.vertex_weights"].astype(np.float64)
    assert ((w != 0.0) & (w != 1.0)).any()
    assert np.all(g["all_background.f64_grad_vertex"] == 0.0)   # w = 0: exact zeros
    eq = g["tied_logits.seg_pred"][:, 0] == g["tied_logits.seg_pred"][:, 1]
    assert eq.mean() > 0.25
    margin = np.abs(g["tied_logits.seg_pred"][:, 0].astype(np.float64) - g["tied_logits.seg_pred"][:, 1].astype(np.float64))
    assert (margin > 20.0).any()   # where softmax - 1 has cancelled in float32 and the restatement's form has not
    small = np.abs(g["tied_logits.f64_grad_seg"])
    assert (small[small > 0.0].min() < 1e-12) and np.all(small > 0.0)
    d = g["boundary.vertex_pred"].astype(np.float64) - g["boundary.vertex"].astype(np.float64)
    for sign in (1.0, -1.0):   # the knee itself and both sides of it, on both branches
        assert (d == sign).any() and (sign * d > 1.0).any() and ((sign * d < 1.0) & (sign * d > 0.99)).any()
    # at the knee itself the second branch is taken: |d| = 1 is not < 1 / sigma^2
    k = 2.0 / (4 * 128 + 1e-3)   # u_v / D of the boundary case: one image of 8 x 16 pixels, 4 planes, weight 1
    assert np.all(g["boundary.f64_grad_vertex"][d == 1.0] == k) and np.all(g["boundary.f64_grad_vertex"][d == -1.0] == -k)


def test_restatement_matches_a_finite_difference_of_the_forward():
    """ties the gradient to the forward the project ships: a three-point finite difference of tests/head_restatement.head_metrics_f64
    in every input element of a tiny case.  With step eps the truncation error of the central difference is eps^2 f''' / 6 and the
    rounding error ~ 2^-52 |f| / eps; at eps = 1e-5, losses of order 1 and third derivatives of order 1 both are ~1e-10, so 1e-7 of
    the largest gradient entry (~1e-2 here) is two orders above what the method can do and five below a wrong formula.  The inputs
    keep |d| at least 0.05 away from the knee, where the loss is not twice differentiable."""
    from tests.head_grad_restatement import head_grad_f64
    from tests.head_restatement import head_metrics_f64
    rng = np.random.default_rng(7)
    b, C, h, w, vn, sigma = 2, 3, 3, 4, 2, 0.8
    seg = rng.normal(0.0, 2.0, (b, C, h, w))
    mask = rng.integers(0, C, (b, h, w))
    vw = rng.uniform(0.0, 1.5, (b, 1, h, w)) * (rng.random((b, 1, h, w)) < 0.8)
    vt = rng.normal(0.0, 1.0, (b, 2 * vn, h, w))
    vp = vt + rng.normal(0.0, 2.0, vt.shape)
    d = np.abs(vw * (vp - vt))
    vp = np.where(np.abs(d - 1.0 / sigma ** 2) < 0.05, vp + 0.2, vp)
    d = np.abs(vw * (vp - vt))
    assert (np.abs(d - 1.0 / sigma ** 2) >= 0.05).all() and (d < 1.0 / sigma ** 2).any() and (d > 1.0 / sigma ** 2).any()
    us, uv = np.array([0.7, 1.3]), np.array([2.0, 0.4])

    def total(seg_, vp_):
        losses, _, _ = head_metrics_f64(seg_, vp_, mask, vt, vw, sigma)
        return float(np.dot(us, losses[:, 0]) + np.dot(uv, losses[:, 1]))

    gs, gv, _ = head_grad_f64(seg, vp, mask, vt, vw, us, uv, sigma)
    eps = 1e-5
    for x, grad, which in ((seg, gs, 0), (vp, gv, 1)):
        fd = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            hi, lo = x.copy(), x.copy()
            hi[idx] += eps
            lo[idx] -= eps
            fd[idx] = (total(hi, vp) - total(lo, vp) if which == 0 else total(seg, hi) - total(seg, lo)) / (2 * eps)
        err = np.abs(fd - grad).max()
        print(f"finite difference vs restatement, input {which}: max |difference| {err:.2e}, largest entry {np.abs(grad).max():.2e}")
        assert np.abs(grad).max() > 1e-3
        assert err <= 1e-7 * np.abs(grad).max()
