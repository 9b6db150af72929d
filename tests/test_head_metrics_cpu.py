"""CPU-only checks of the head metrics (include/pvnet_head.h, libpvnet_head.so): the header's exports and constants by name and value,
the library's kernels, every bad argument rejected with the documented code before any HIP call, the register rule, the Python entry's
refusal of host tensors, and the float64 restatement against the fixture's recorded column.  What holds for every side library alike
(header against table, the built library's symbols, the register tool's selection, the loud failure without it) is in
tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_head.h")).read()
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
KERNELS = ("head_partial_kernel", "head_partial_general_kernel", "head_final_kernel")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_head_library()


def test_header_declares_the_exports_and_every_one_has_a_prototype():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == {"pvnet_head_abi_version", "pvnet_head_metrics_workspace_bytes", "pvnet_head_metrics"}
    assert _abi.HEAD_PROTOTYPES["pvnet_head_metrics_workspace_bytes"][0] is C.c_size_t   # a byte count is not cut to 32 bits
    # one argument type per declared parameter
    decl = re.search(r"^int pvnet_head_metrics\s*\((.*?)\);", HDR, re.M | re.S).group(1)
    assert len(_abi.HEAD_PROTOTYPES["pvnet_head_metrics"][1]) == len(decl.split(",")) == 24
    assert _abi.HEAD_PROTOTYPES["pvnet_head_metrics"][1][22] is C.c_size_t and "size_t workspace_bytes" in decl
    defines = dict(re.findall(r"^#define\s+PVNET_HEAD_(\w+)\s+(\d+)\b", HDR, re.M))
    assert len(defines) == 8
    for name, value in defines.items():
        assert getattr(_abi, "HEAD_" + name) == int(value), name


def test_library_is_built_for_gfx950_and_exports_the_symbols(lib):
    assert lib.pvnet_head_abi_version() == _abi.HEAD_ABI_VERSION == 1
    blob = open(_abi.HEAD_LIB_PATH, "rb").read()
    assert all(k.encode() in blob for k in KERNELS)
    assert "head_metrics.hip" in build.SIDE_LIBRARIES["head"][0] and "head_metrics.hip" not in build.VOTE_TU


def test_workspace_bytes(lib):
    ws = lib.pvnet_head_metrics_workspace_bytes
    assert ws(0, 480, 640) == 0 and ws(4, 0, 640) == 0 and ws(4, 480, 0) == 0 and ws(65536, 8, 8) == 0
    one = ws(1, 480, 640)
    assert one % 256 == 0 and one >= 300 * 32          # a record (three float64 sums, four packed counts) per 1 024 pixels
    assert ws(32, 480, 640) >= 32 * 300 * 32 and ws(32, 480, 640) < (1 << 20)
    assert ws(1, 1, 1) > 0 and ws(1, 32768, 32768) >= (1 << 25)


def test_bad_arguments_are_rejected_without_a_device(lib):
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    s4, s3 = (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 3)(1, 1, 1)
    U8, I16, I32, I64, F32 = 0, 1, 2, 3, 4

    def call(seg=p, ss=s4, nc=2, vp=p, vs=s4, vt=p, ts=s4, vw=p, wstr=s3, mask=p, mdt=I64, ms=s3, b=4, h=96, w=128, vn=9, sigma=1.0,
             flags=0, losses=p, counts=p, status=None, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_head_metrics_workspace_bytes(max(b, 1), max(h, 1), max(w, 1))
        return lib.pvnet_head_metrics(seg, ss, nc, vp, vs, vt, ts, vw, wstr, mask, mdt, ms, b, h, w, vn, sigma, flags, losses, counts,
                                      status, ws, wsb, None)

    for name in ("seg", "ss", "vp", "vs", "vt", "ts", "vw", "wstr", "mask", "ms", "losses", "counts"):
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
    assert call(wsb=lib.pvnet_head_metrics_workspace_bytes(4, 96, 128) - 1) == WORKSPACE
    assert call(b=8, wsb=lib.pvnet_head_metrics_workspace_bytes(4, 96, 128)) == WORKSPACE
    assert call(b=65536) == UNSUPPORTED
    assert call(h=1 << 16, w=1 << 16) == UNSUPPORTED
    for mdt in (U8, I32, I64):
        assert call(mdt=mdt, b=0, ws=None, wsb=0) == 0             # nothing to do, nothing enqueued
    for flags in (1, 2, 4, 8, 1 | 8, 2 | 4, 16, 32):
        assert call(flags=flags, b=0) == 0


def test_register_check_covers_the_new_translation_unit(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as chk
    (src, text), = chk.side_assembly("head")
    assert src.endswith("head_metrics.hip")
    ks = chk.kernels(text)
    assert len(ks) >= 3 and all(any(k in name for name, _, _, _ in ks) for k in KERNELS)
    for name, nfv, vmax, scratch in ks:
        assert nfv - (vmax + 1) >= chk.SLACK and scratch == 0, name
    # the rule bites: the same kernel with its allocation cut to what it uses is rejected
    name, nfv, vmax, _ = ks[0]
    i = text.index(".amdhsa_kernel " + name)
    tight = text[:i] + re.sub(r"\.amdhsa_next_free_vgpr \d+", f".amdhsa_next_free_vgpr {vmax + 1}", text[i:], count=1)
    assert any(n == name and f - (v + 1) < chk.SLACK for n, f, v, _ in chk.kernels(tight))


def test_python_entry_refuses_host_tensors_and_imports_no_oracle():
    import torch
    from pvnet_amd import validation as V
    seg, vp = torch.zeros((1, 2, 8, 8)), torch.zeros((1, 4, 8, 8))
    mask, vt, vw = torch.zeros((1, 8, 8), dtype=torch.int64), torch.zeros((1, 4, 8, 8)), torch.zeros((1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        V.head_metrics_device(seg, vp, mask, vt, vw)
    with pytest.raises(RuntimeError, match="CUDA"):
        V.HeadMetrics()(seg, vp, mask, vt, vw)
    src = open(os.path.join(ROOT, "pvnet_amd", "validation.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M)


def test_restatement_reproduces_the_fixture_exactly():
    """the float64 restatement the GPU tests compare against IS the one that wrote the fixture's float64 column: every loss
    bit for bit, every count equal; and the recorded reference outputs lie within float32 rounding of it"""
    from tests.head_restatement import head_metrics_f64
    g = np.load(os.path.join(ROOT, "tests", "golden", "head_metrics.npz"))
    names = [str(n) for n in g["cases"]]
    assert {"typical", "boundary", "all_background", "all_foreground", "tied_logits", "sigma_3_odd_size"} <= set(names)
    for n in names:
        seg = g[n + ".seg_pred"]
        assert seg.shape[2] <= 96 and seg.shape[3] <= 128 and g[n + ".vertex_pred"].shape[1] <= 18 and seg.shape[1] == 2
        f64, counts, status = head_metrics_f64(seg, g[n + ".vertex_pred"], g[n + ".mask"], g[n + ".vertex"], g[n + ".vertex_weights"],
                                               float(g[n + ".sigma"]))
        assert f64.tobytes() == g[n + ".f64"].tobytes(), n
        assert np.array_equal(counts, g[n + ".counts"]) and not status.any(), n
        ref32 = g[n + ".ref32"]
        assert ref32.dtype == np.float32 and ref32.shape == f64.shape
        assert np.all(np.abs(ref32.astype(np.float64) - f64) <= 4e-7 * np.abs(f64)), n   # a few float32 roundings, no more
    assert any(float(g[n + ".sigma"]) != 1.0 for n in names)
    assert np.all(g["all_background.f64"][:, 1] == 0.0)   # sum w = 0: 0 / 1e-3
    eq = g["tied_logits.seg_pred"][:, 0] == g["tied_logits.seg_pred"][:, 1]
    assert eq.mean() > 0.25
    d = np.abs(g["boundary.vertex_pred"].astype(np.float64) - g["boundary.vertex"].astype(np.float64))
    assert (d == 1.0).any() and (d > 1.0).any() and ((d < 1.0) & (d > 0.99)).any()   # the knee itself and both sides of it
