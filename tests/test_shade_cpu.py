"""CPU-only checks of the shaded vertex-colour renderer (include/pvnet_shade.h, libpvnet_shade.so, pvnet_amd/shade.py): the registry
row, the header's constants against pvnet_amd/_abi.py, every bad argument rejected before any HIP call, the kernels' assembly (one 64-bit
atomic minimum per path of the triangle kernel, nothing contracted, the register rule), the numpy restatement
(tests/shade_restatement.py) against the depth restatement and against an independent float64 ray caster of the reference's GLSL
formulas, ``ColorMeshes`` and ``read_ply``.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build, render, shade
from tests import depth_restatement as DR
from tests import shade_restatement as SR
from tests.render_cases import BADARG, UNSUPPORTED, camera, i32, pose, refuses_the_pvnet_render_list, smooth_colors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_shade.h")).read()
EXPORTS = {"pvnet_shade_abi_version", "pvnet_shade_workspace_bytes", "pvnet_render_color"}
H, W = 48, 64


@pytest.fixture(scope="module")
def lib():
    build.build_side("shade")
    return _abi.load_shade_library()


def test_registry_row():
    assert build.SIDE_LIBRARIES["shade"][:2] == (["shade.hip"], "pvnet_shade.h")
    zbuffer, color = os.path.join(build.CSRC, "zbuffer_core.h"), os.path.join(build.CSRC, "pixel_color.h")
    stages, plane = os.path.join(build.CSRC, "mesh_core.h"), os.path.join(build.CSRC, "depth_core.h")
    assert build.SIDE_LIBRARIES["shade"][2] == [zbuffer, color]
    # the headers rebuild exactly the libraries that compile them
    assert {n for n in build.SIDE_LIBRARIES if stages in build._side(n)[1]} == {"raster", "depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if plane in build._side(n)[1]} == {"depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if zbuffer in build._side(n)[1]} == {"depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if color in build._side(n)[1]} == {"shade", "texture"}
    text = open(os.path.join(build.CSRC, "shade.hip")).read()
    assert '#include "pixel_color.h"' in text and '#include "zbuffer_core.h"' in open(color).read()
    assert '#include "mesh_core.h"' in open(zbuffer).read() and '#include "depth_core.h"' in open(zbuffer).read()
    assert '#include "zbuffer_core.h"' in open(os.path.join(build.CSRC, "depth.hip")).read()
    assert _abi.SIDE_LIBRARIES["shade"] == (_abi.SHADE_LIB_PATH, _abi.SHADE_ABI_VERSION, _abi.SHADE_PROTOTYPES)
    assert _abi.load_shade_library.args == ("shade",)


def test_abi_version_and_constants_are_mirrored():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS == set(_abi.SHADE_PROTOTYPES)
    decl = re.search(r"^int pvnet_render_color\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.SHADE_PROTOTYPES["pvnet_render_color"][1]
    assert len(decl) == len(args) == 32
    # pvnet_render_depth's list through far, and its tail behind the seven new arguments
    depth_args = _abi.DEPTH_PROTOTYPES["pvnet_render_depth"][1]
    assert args[:18] == depth_args[:18] and args[25:] == depth_args[18:]
    for k, (word, typ) in {2: ("vertex_offset", _abi._i32p), 8: ("mesh_id", _abi._i32p), 12: ("image_id", _abi._i32p), 13: ("label", _abi._i32p),
                           17: ("float far", C.c_float), 18: ("uint8_t* colors", C.c_void_p), 19: ("double* normals", C.c_void_p),
                           20: ("int shading", C.c_int), 21: ("float ambient", C.c_float), 22: ("uint8_t* bg_color", _abi._u8p),
                           23: ("uint8_t* bg_image", C.c_void_p), 24: ("uint8_t* rgb_out", C.c_void_p), 25: ("depth_out", C.c_void_p),
                           26: ("label_out", C.c_void_p), 27: ("visible_out", C.c_void_p), 28: ("status_out", C.c_void_p),
                           30: ("ws_bytes", C.c_size_t), 31: ("stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_SHADE_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.SHADE_ABI_VERSION == 1
    assert consts.pop("WS_COOP_COUNT_OFFSET") == 0
    assert len(consts) == 12
    for name, value in consts.items():
        assert getattr(_abi, "SHADE_" + name) == value, name
        if hasattr(_abi, "DEPTH_" + name):   # the limits and bits of pvnet_render_depth under this header's names
            assert getattr(_abi, "DEPTH_" + name) == value, name
    assert {n for n in consts if not hasattr(_abi, "DEPTH_" + n)} == {"MAX_FACES", "NONE", "FLAT", "PHONG"}
    assert _abi.SHADE_MAX_INSTANCES < (1 << 10) - 1 and _abi.SHADE_MAX_FACES == 1 << 22   # instance << 22 | face, below all ones
    assert (SR.NONE, SR.FLAT, SR.PHONG) == (_abi.SHADE_NONE, _abi.SHADE_FLAT, _abi.SHADE_PHONG)
    assert shade.SHADING == SR.SHADING


def test_library_is_built_with_its_exports_and_none_of_the_other_libraries_kernels(lib):
    assert lib.pvnet_shade_abi_version() == 1
    blob = open(_abi.SHADE_LIB_PATH, "rb").read()
    for kernel in (b"shade_setup_kernel", b"shade_clear_kernel", b"shade_tri_kernel", b"shade_resolve_kernel"):
        assert kernel in blob
    for other in (b"depth_tri_kernel", b"depth_resolve_kernel", b"depth_setup_kernel", b"depth_clear_kernel", b"triangle_kernel",
                  b"expand_kernel"):
        assert other not in blob
    raw = C.CDLL(_abi.SHADE_LIB_PATH)
    assert not hasattr(raw, "pvnet_render") and not hasattr(raw, "pvnet_render_depth") and not hasattr(raw, "pvnet_vote_v3")


def test_workspace_bytes_is_monotone_and_rejects_bad_sizes(lib):
    f = lib.pvnet_shade_workspace_bytes
    base = dict(q=4, P=100, T=200, b=2, h=60, w=80)
    assert f(*base.values()) > 0 and f(*base.values()) % 16 == 0
    for name in base:
        prev = 0
        for step in (0, 1, 2, 7, 64, 1000):
            n = f(*{**base, name: base[name] + step}.values())
            assert n >= prev > -1, name
            prev = n
    assert f(4, 100, 200, 2, 61, 80) > f(4, 100, 200, 2, 60, 80) and f(5, 100, 200, 2, 60, 80) > f(4, 100, 200, 2, 60, 80)
    assert f(4, 100, 200, 3, 60, 80) > f(4, 100, 200, 2, 60, 80) and f(4, 100, 200, 2, 60, 82) > f(4, 100, 200, 2, 60, 80)
    assert f(4, 100, 200, 2, 60, 80) >= 2 * 60 * 80 * 8   # one 64-bit word per pixel
    for bad in (dict(h=1), dict(w=1), dict(h=0), dict(w=-5), dict(q=-1), dict(P=-1), dict(T=-1), dict(b=-1), dict(h=40000)):
        assert f(*{**base, **bad}.values()) == 0, bad
    assert f(0, 0, 0, 0, 2, 2) == 16


def test_bad_arguments_are_rejected_without_a_device(lib):
    p = C.c_void_p(0x1000)   # never dereferenced: validation returns before any HIP call
    voff, foff = i32(0, 12, 20), i32(0, 20, 32)
    ws_n = lib.pvnet_shade_workspace_bytes(3, 20, 32, 2, 20, 24)
    black = (C.c_uint8 * 3)(0, 0, 0)

    def call(vertices=p, faces=p, voff=voff, foff=foff, M=2, P=20, T=32, q=3, mesh=i32(0, 1, 1), poses=p, K=p, kper=0,
             image=i32(0, 0, 1), label=i32(1, 2, 3), b=2, h=20, w=24, far=float("inf"), colors=p, normals=None, shading=1, ambient=0.5,
             bg=black, bg_image=None, rgb=p, depth=None, labels=None, visible=None, status=None, ws=p, nbytes=ws_n):
        return lib.pvnet_render_color(vertices, faces, voff, foff, M, P, T, q, mesh, poses, K, kper, image, label, b, h, w, far, colors,
                                      normals, shading, ambient, bg, bg_image, rgb, depth, labels, visible, status, ws, nbytes, None)

    # what is new
    assert call(rgb=None) == BADARG and call(rgb=None, depth=p, labels=p) == BADARG   # no rgb_out
    assert call(colors=None) == BADARG and call(bg=None) == BADARG
    for shading in (-1, 3, 100):
        assert call(shading=shading) == BADARG, shading
    for ambient in (float("nan"), -0.5, -1e-30, float("-inf"), float("inf")):
        assert call(ambient=ambient) == BADARG, ambient
    assert call(shading=2) == BADARG and call(shading=2, normals=None, colors=p) == BADARG   # Phong without normals
    # the depth library's list
    for far in (0.0, -0.0, -1.0, float("-inf"), float("nan")):
        assert call(far=far) == BADARG, far
    refuses_the_pvnet_render_list(call, ws_n, _abi.SHADE_MAX_MESHES, _abi.SHADE_MAX_INSTANCES, _abi.SHADE_MAX_SIDE, _abi.SHADE_MAX_IMAGES)
    big = _abi.SHADE_MAX_FACES + 1   # a mesh with more faces than the word's 22 bits name
    assert call(M=1, voff=i32(0, 20), foff=i32(0, big), T=big, mesh=i32(0, 0, 0)) == UNSUPPORTED
    # the all-good call would reach the device: everything optional absent, b == 0 enqueues nothing
    assert call(b=0, q=0) == 0 and call(b=0, q=0, shading=2, normals=p, ambient=0.0, bg_image=p) == 0


def fused_f64_per(expression):
    """the fused float64 operations this compiler, with the library's flags, spends on ONE ``expression`` of doubles a and b"""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as CK
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "one.hip")
        with open(src, "w") as fh:
            fh.write("#include <hip/hip_runtime.h>\n#pragma STDC FP_CONTRACT OFF\n"
                     "__global__ void one(double* p) { const double a = p[1], b = p[2]; p[0] = %s; }\n" % expression)
        CK.compile_to_asm(src, os.path.join(d, "one.s"))
        code = "\n".join(line.split(";")[0] for line in open(os.path.join(d, "one.s")).read().splitlines())
    return len(re.findall(r"\bv_(fma|fmac)_f64(_e32|_e64)?\b", code))


def test_assembly_one_atomic_minimum_nothing_contracted_and_the_register_rule():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--shade"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "checked 4 kernels, 0 without" in r.stdout
    assert all("scratch   0 B" in line for line in r.stdout.splitlines() if " allocates " in line)   # no spills
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as CK
    (_, asm), = CK.side_assembly("shade")
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())
    by_kernel = {name: "\n".join(c) for name, (c, _) in CK.kernel_code(asm).items()}
    tri, = [c for n, c in by_kernel.items() if "shade_tri_kernel" in n]
    # the 64-bit unsigned minimum is one global atomic on each of the triangle kernel's two paths, not a compare-and-swap loop, and no
    # other kernel has one
    assert len(re.findall(r"\bglobal_atomic_umin_x2\b", code)) == 2 == len(re.findall(r"\bglobal_atomic_umin_x2\b", tri))
    assert "cmpswap" not in code
    # the predicate has no division, and the resolve kernel finds its pixel without one: any fused float32 multiply-add would be a
    # contraction
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)(mk|ak)?_f32\b", code)
    # float64: the only fused operations are those of the divisions' and square roots' own expansions.  Divisions: the triangle kernel's
    # 13 (tests/test_depth_cpu.py); in the resolve kernel the projection's six, l1 and l2, the three w_k, the attribute's nine (eye
    # point, colour, normal) and the diffuse term's two.  Square roots: |e|, |g|, |n|.
    divisions, roots = len(re.findall(r"\bv_div_fixup_f64\b", code)), len(re.findall(r"\bv_rsq_f64", code))
    assert (divisions, roots) == (13 + 22, 3)
    per_division, per_root = fused_f64_per("a / b"), fused_f64_per("sqrt(a)")
    assert per_division > 0 and per_root > 0 and fused_f64_per("a * b + a") == 0
    assert len(re.findall(r"\bv_(fma|fmac)_f64(_e32|_e64)?\b", code)) == per_division * divisions + per_root * roots
    assert "v_mul_f64" in code and "v_add_f64" in code and "v_mul_f32" in code
    modes = re.findall(r"\.amdhsa_float_denorm_mode_32 (\d)", asm) + re.findall(r"\.amdhsa_float_denorm_mode_16_64 (\d)", asm)
    assert len(modes) == 8 and set(modes) == {"3"}   # denormals kept in every kernel
    for banned in ("printf", "__assert_fail"):
        assert banned not in asm


# ---- ColorMeshes and read_ply -------------------------------------------------------------------------------------------------------------
def test_color_meshes_validation_and_computed_normals():
    v, f = render.icosphere(2, 0.1)
    col = smooth_colors(v)
    table = shade.ColorMeshes([(v, f, col), (*render.box_mesh(0.1, 0.2, 0.3), np.full((8, 3), 200, np.int64), np.ones((8, 3)))])
    assert isinstance(table, render.DeviceMeshes) and table.count == 2 and table.total_vertices == len(v) + 8
    assert table.colors.dtype == np.uint8 and table.colors.shape == (len(v) + 8, 3) and table.normals.shape == (len(v) + 8, 3)
    assert np.array_equal(table.colors[:len(v)], col) and (table.colors[len(v):] == 200).all()
    assert np.array_equal(table.normals[len(v):], np.ones((8, 3)))               # given normals are taken as they are
    # a sphere's normals are its normalised positions
    assert np.abs(table.normals[:len(v)] - v / np.linalg.norm(v, axis=1, keepdims=True)).max() < 1e-12
    assert np.abs(shade.vertex_normals(v, f[:, ::-1]) + table.normals[:len(v)]).max() < 1e-12   # the winding decides the side
    mv, mf, mc, mn = table.mesh(1)
    assert len(mv) == 8 and len(mf) == 12 and (mc == 200).all() and mn.shape == (8, 3)
    lone = shade.vertex_normals(np.zeros((4, 3)), np.array([[0, 1, 2]]))          # no area, and a vertex no face names
    assert not lone.any()
    for bad in ([(v, f)], [(v, f, col[:-1])], [(v, f, col.astype(np.float64))], [(v, f, col.astype(np.int64) + 200)],
                [(v, f, col, np.ones((3, 3)))], [(v, f, col, np.full((len(v), 3), np.nan))], [(v, f + len(v), col)]):
        with pytest.raises(ValueError):
            shade.ColorMeshes(bad)


def write_ply(path, v, f, colors=None, normals=None, binary=False, extra=False):
    props = ["property float x", "property float y", "property float z"]
    cols = [("x", "<f4", v[:, 0]), ("y", "<f4", v[:, 1]), ("z", "<f4", v[:, 2])]
    if normals is not None:
        props += ["property double nx", "property double ny", "property double nz"]
        cols += [("nx", "<f8", normals[:, 0]), ("ny", "<f8", normals[:, 1]), ("nz", "<f8", normals[:, 2])]
    if extra:
        props += ["property ushort quality"]
        cols += [("quality", "<u2", np.arange(len(v)) % 7)]
    if colors is not None:
        props += ["property uchar red", "property uchar green", "property uchar blue"]
        cols += [("red", "u1", colors[:, 0]), ("green", "u1", colors[:, 1]), ("blue", "u1", colors[:, 2])]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by the test",
            "element vertex %d" % len(v)] + props + ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        if binary:
            rec = np.zeros(len(v), np.dtype([(n, t) for n, t, _ in cols]))
            for n, _, val in cols:
                rec[n] = val
            fh.write(rec.tobytes())
            frec = np.zeros(len(f), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            frec["n"], frec["v"] = 3, f
            fh.write(frec.tobytes())
        else:
            for i in range(len(v)):
                fh.write((" ".join(repr(float(val[i])) if t[-2] == "f" else str(int(val[i])) for _, t, val in cols) + "\n").encode())
            for face in f:
                fh.write(("3 %d %d %d\n" % tuple(face)).encode())


@pytest.mark.parametrize("binary", [False, True])
def test_read_ply_round_trips(tmp_path, binary):
    v, f = render.icosphere(1, 0.1)
    v32 = v.astype(np.float32)
    col, nrm = smooth_colors(v), shade.vertex_normals(v, f)
    full = str(tmp_path / "full.ply")
    write_ply(full, v32, f, col, nrm, binary=binary, extra=True)
    got = shade.read_ply(full)
    assert got["vertices"].dtype == np.float64 and np.array_equal(got["vertices"], v32.astype(np.float64))
    assert got["faces"].dtype == np.int32 and np.array_equal(got["faces"], f)
    assert got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], col)
    assert np.array_equal(got["normals"], nrm)   # float64, and repr() round trips in ASCII
    shade.ColorMeshes([(got["vertices"], got["faces"], got["colors"], got["normals"])])
    bare = str(tmp_path / "bare.ply")
    write_ply(bare, v32, f, binary=binary)
    got = shade.read_ply(bare)
    assert got["colors"] is None and got["normals"] is None and np.array_equal(got["faces"], f) and len(got["vertices"]) == len(v)
    quad = str(tmp_path / "quad.ply")
    with open(quad, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                 b"property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError):
        shade.read_ply(quad)
    with pytest.raises(ValueError):
        shade.read_ply(__file__)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def coloured(mesh):
    v, f = mesh
    return v, f, smooth_colors(v), shade.vertex_normals(v, f)


MESHES = [coloured(render.box_mesh(0.15, 0.1, 0.2)), coloured(render.l_prism_mesh(0.2, 0.08)), coloured(render.icosphere(1, 0.1)),
          coloured(render.icosphere(2, 0.1))]


def test_restated_depth_labels_and_visible_are_the_depth_restatements():
    K = camera(H, W)
    rng = np.random.default_rng(20261019)
    scenes = []
    for _ in range(3):   # three instances per image, two images, overlapping
        inst = []
        for img in range(2):
            for m in rng.choice(4, 3, replace=False):
                t = (rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05), rng.uniform(0.4, 0.7))
                inst.append((int(m), pose(rng.normal(size=3), rng.uniform(0, np.pi), t), K, img, int(rng.integers(1, 256))))
        scenes.append(inst)
    p = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))
    scenes.append([(1, p, K, 0, 3), (1, p.copy(), K, 0, 7)])   # an exact tie
    for inst in scenes:
        for far in (np.inf, 0.55):
            rgb, depth, label, visible, status = SR.render(MESHES, inst, 2, H, W, far=far, shading="flat", background=(9, 8, 7))
            wd, wl, wv, wst = DR.render([m[:2] for m in MESHES], inst, 2, H, W, far)
            assert np.array_equal(depth.view(np.uint32), wd.view(np.uint32)) and np.array_equal(label, wl)
            assert np.array_equal(visible, wv) and np.array_equal(status, wst) and label.any()
            assert (rgb[label == 0] == (9, 8, 7)).all() and rgb.dtype == np.uint8 and rgb.shape == (2, H, W, 3)
    # shading "none" of a mesh of one colour is that colour, whatever the pose; ambient 1 saturates the light
    v, f, _, n = MESHES[3]
    one = [(v, f, np.tile(np.array([[10, 128, 250]], np.uint8), (len(v), 1)), n)]
    inst = [(0, pose((1, 0, 1), 0.3, (0.01, 0.0, 0.5)), K, 0, 1)]
    rgb, _, label, _, _ = SR.render(one, inst, 1, H, W, shading="none")
    assert label.any() and (rgb[label != 0] == (10, 128, 250)).all()
    for shading in ("flat", "phong"):
        rgb, _, label, _, _ = SR.render(one, inst, 1, H, W, shading=shading, ambient=1.0)
        assert (rgb[label != 0] == (10, 128, 250)).all()
        dark, _, _, _, _ = SR.render(one, inst, 1, H, W, shading=shading, ambient=0.0)
        lit = dark[label != 0].astype(int)
        assert (lit <= (10, 128, 250)).all() and lit[:, 2].max() > 240 and lit[:, 2].min() < 150   # the centre faces the light, the rim not


# ---- the independent ray caster ----------------------------------------------------------------------------------------------------------
def ray_hits(vertices, faces, pose_, K, h, w):
    """A ray through every pixel centre, the nearest triangle by Moeller-Trumbore in camera space, the TRUE barycentrics of the hit
    -> (label [h,w] bool, face [h,w], barycentrics [h,w,3])"""
    cam = np.asarray(vertices, np.float64) @ pose_[:, :3].T + pose_[:, 3]
    Kinv = np.linalg.inv(K)
    best = np.full((h, w), np.inf)
    hit = np.full((h, w), -1, np.int64)
    bary = np.zeros((h, w, 3))
    proj = cam @ K.T
    uv = proj[:, :2] / proj[:, 2:]
    for fi, face in enumerate(np.asarray(faces, np.int64)):
        lo, hi = np.floor(uv[face].min(0)).astype(int) - 1, np.ceil(uv[face].max(0)).astype(int) + 1   # rays that can hit it at all
        x0, x1, y0, y1 = max(lo[0], 0), min(hi[0], w - 1), max(lo[1], 0), min(hi[1], h - 1)
        if x0 > x1 or y0 > y1:
            continue
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        d = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64) @ Kinv.T
        a, b, c = cam[face]
        e1, e2 = b - a, c - a
        pvec = np.cross(d, e2)
        det = pvec @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tvec = -a                                    # the origin is the camera
            uu = (pvec @ tvec) * inv
            qvec = np.cross(tvec, e1)
            vv = (d @ qvec) * inv
            tt = (e2 @ qvec) * inv
        ok = (det != 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 0)
        depth = tt * d[..., 2]
        view = best[y0:y1 + 1, x0:x1 + 1]
        take = ok & (depth < view)
        view[take] = depth[take]
        hit[y0:y1 + 1, x0:x1 + 1][take] = fi
        bary[y0:y1 + 1, x0:x1 + 1][take] = np.stack([1 - uu - vv, uu, vv], -1)[take]
    return np.isfinite(best), hit, bary


def glsl_shade(hits, vertices, faces, colors, normals, pose_, K, shading, ambients, vertex_light=True, normal_w=True):
    """The reference's shaders on the hits of ``ray_hits`` (lib/utils/opengl_render_backend.py:38-45, 60-73, 90-100), written from
    them and not from pvnet_shade.h:
        v_eye_pos = the interpolated camera-space position;  v_L = normalize(light - v_eye_pos) PER VERTEX, light = the camera origin;
        v_normal = normalize(u_nm * vec4(a_normal, 1.0)).xyz per vertex, u_nm = inverse(model view)^T (line 158): the FOUR-vector
                   is normalised, its fourth component being 1 - t . (R a_normal) for a rigid pose [R|t];
        flat:  face_normal = normalize(cross(dFdx(v_eye_pos), dFdy(v_eye_pos))), the derivatives as the differences to the hits of
               the neighbouring pixels' rays with the triangle's plane, turned towards the viewer;
        light_diffuse_w = max(dot(normalize(v_L), normalize(normal)), 0);  light_w = min(ambient + light_diffuse_w, 1);
        gl_FragColor = light_w * v_color, stored as an 8-bit channel: round(255 * value).
    (The reference's view matrix also flips y and z, OpenCV to OpenGL: a rotation of the camera frame that leaves every dot product,
    length and the fourth component as they are.)
    The two switches exist to ATTRIBUTE differences, the shaders are both True: ``vertex_light=False`` takes the light vector from the
    hit point itself, ``normal_w=False`` normalises the rotated three-vector R a_normal.
    -> {ambient: rgb [h,w,3] float64, not rounded}"""
    label, hit, bary = hits
    h, w = label.shape
    cam = np.asarray(vertices, np.float64) @ pose_[:, :3].T + pose_[:, 3]
    mv = np.eye(4)
    mv[:3] = pose_
    if normal_w:
        n4 = np.concatenate([np.asarray(normals, np.float64), np.ones((len(cam), 1))], 1) @ np.linalg.inv(mv)   # rows: u_nm (n, 1)
        nrm = (n4 / np.linalg.norm(n4, axis=1, keepdims=True))[:, :3]
    else:
        nrm = np.asarray(normals, np.float64) @ pose_[:, :3].T
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    vL = -cam / np.linalg.norm(cam, axis=1, keepdims=True)
    col = np.asarray(colors, np.float64) / 255.0
    Kinv = np.linalg.inv(K)
    ys, xs = np.nonzero(label)
    fidx = np.asarray(faces, np.int64)[hit[ys, xs]]
    bw = bary[ys, xs]
    interp = lambda attr: (attr[fidx] * bw[..., None]).sum(1)   # noqa: E731
    L = interp(vL) if vertex_light else -interp(cam)
    L = L / np.linalg.norm(L, axis=1, keepdims=True)
    if shading == "phong":
        n = interp(nrm)
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
    else:
        a, b, c = cam[fidx[:, 0]], cam[fidx[:, 1]], cam[fidx[:, 2]]
        plane_n = np.cross(b - a, c - a)

        def on_plane(px, py):   # the eye position of a pixel's ray on this triangle's plane
            d = np.stack([px, py, np.ones_like(px)], -1).astype(np.float64) @ Kinv.T
            return d * ((plane_n * a).sum(1) / (plane_n * d).sum(1))[:, None]

        here = on_plane(xs, ys)
        n = np.cross(on_plane(xs + 1, ys) - here, on_plane(xs, ys + 1) - here)
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(((n * here).sum(1) > 0)[:, None], -n, n)   # towards the viewer
    diffuse = np.maximum((L * n).sum(1), 0.0)
    out = {}
    for ambient in ambients:
        light = np.minimum(ambient + diffuse, 1.0)
        img = np.zeros((h, w, 3))
        img[ys, xs] = 255.0 * light[:, None] * interp(col)
        out[ambient] = img
    return out


ORACLE_H, ORACLE_W = 240, 320
ORACLE_K = np.array([[300.0, 0.0, 160.3], [0.0, 301.0, 119.8], [0.0, 0.0, 1.0]])
ORACLE_SCENES = {   # an icosphere of 80 px radius (0.16 at z = 0.6 under f = 300), and a box
    "sphere": (coloured(render.icosphere(3, 0.16)), pose((1, 2, 3), 0.7, (0.01, -0.005, 0.6))),
    "box": (coloured(render.box_mesh(0.3, 0.22, 0.26)), pose((2, -1, 1), 0.9, (-0.02, 0.01, 0.7))),
}
ORACLE_AMBIENTS = (0.2, 0.5)
# the largest measured difference to the shaders as they are written, per scene and shading (the test's docstring); the bar is one more
MEASURED_ORACLE = {("sphere", "flat"): 0.547, ("sphere", "phong"): 0.749, ("box", "flat"): 4.410, ("box", "phong"): 35.527}
# with both named terms removed the ray caster and the definition are the same function of the same float64 inputs but for the float32
# rounding of the screen vertices (1e-5 grey levels): what is left is the rounding to uint8, half a grey level
ROUNDING_BAR = 0.5 + 0.01


@pytest.fixture(scope="module")
def oracle_geometry():
    """per scene, computed once: the restatement's winning faces, the ray caster's hits, its interior pixels"""
    out = {}
    for name, ((v, f, col, nrm), p) in ORACLE_SCENES.items():
        _, owner, status = SR.instance_layers(v, f, p, ORACLE_K, ORACLE_H, ORACLE_W)
        assert status == 0
        hits = ray_hits(v, f, p, ORACLE_K, ORACLE_H, ORACLE_W)
        out[name] = (owner, hits, interior_pixels(hits[0]))
    return out


def interior_pixels(label):
    """the pixels whose eight neighbours carry the same label in the ray caster's own label image"""
    pad = np.pad(label, 1)
    interior = label.copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            interior &= pad[dy:dy + label.shape[0], dx:dx + label.shape[1]]
    return interior


def oracle_differences(name, shading, geometry, **switches):
    """{ambient: |restatement - ray caster| over the interior pixels, grey levels}"""
    (v, f, col, nrm), p = ORACLE_SCENES[name]
    owner, hits, interior = geometry
    want = glsl_shade(hits, v, f, col, nrm, p, ORACLE_K, shading, ORACLE_AMBIENTS, **switches)
    ys, xs = np.nonzero(interior)
    out = {}
    for ambient in ORACLE_AMBIENTS:
        got = SR.shade_pixels(v, f, col, nrm, p, ORACLE_K, owner[ys, xs], xs, ys, SR.SHADING[shading], ambient).astype(np.float64)
        assert got.max() > 100
        out[ambient] = np.abs(got - want[ambient][ys, xs])
    return out


@pytest.mark.parametrize("shading", ["flat", "phong"])
@pytest.mark.parametrize("name", sorted(ORACLE_SCENES))
def test_restatement_against_the_glsl_ray_caster(oracle_geometry, name, shading):
    """MEASURED (240 x 320, interior pixels: those whose eight neighbours carry the ray caster's own label, 20 947 of 21 607 covered
    pixels on the sphere and 20 943 of 21 629 on the box, 3.1 / 3.2 % left out; the restatement's uint8 against the ray caster's
    unrounded value).  Largest difference in grey levels at ambient 0.2 / 0.5 (mean; 99.9 % quantile):
                       the shaders as written               light from the hit point   three-vector normal   both removed
        sphere, flat    0.547 /  0.531 (0.25; 0.52)          0.500                      0.547                 0.500
        sphere, Phong   0.749 /  0.737 (0.25; 0.65)          0.775                      0.540                 0.500
        box, flat       4.410 /  4.391 (1.52 / 0.50; 4.18)   0.500                      4.410                 0.500
        box, Phong     35.418 / 35.527 (5.48 / 3.68; 33.9)  40.255                      5.248                 0.500
    The definition differs from the shaders in TWO deliberate ways, both named in include/pvnet_shade.h:
      1. the shaders normalise the vector to the light per VERTEX and interpolate it (v_L); the definition takes the direction from the
         pixel's own eye point (the light is at the camera).  Worth up to 4.4 grey levels (flat) and 5.2 (Phong) on a face of 0.3 m seen
         from 0.7 m, nothing beyond the rounding on the sphere's small faces;
      2. the shaders transform a normal as the FOUR-vector (a_normal, 1) by inverse(model view)^T and normalise all four components
         (line 44), which shortens each vertex normal by 1 / sqrt(1 + (1 - t . R a_normal)^2) before interpolation; the definition
         interpolates R a_normal itself, as the issue prescribes.  On the box, whose eight corner normals point far apart, that weighting
         moves the interpolated normal by many degrees: up to 35.5 grey levels, mean 3.7 .. 5.5.  On the sphere 0.2.  Flat shading does
         not read the normals.
    With both terms switched off in the ray caster every case is within 0.500: nothing else differs.  Two bars: the shaders as written
    under the measured maximum of that scene and shading plus one grey level (for the rounding boundary); both terms removed under
    the uint8 rounding alone.  No interior pixel is excluded.  profiles/shade_probe.txt records the same."""
    owner, hits, interior = oracle_geometry[name]
    covered, kept = int(hits[0].sum()), int(interior.sum())
    assert covered > 10000 and covered - kept <= 0.10 * covered, (covered, kept)
    assert (owner[interior] >= 0).all()   # the restatement covers every interior pixel
    worst = {}
    for what, switches in (("shaders", {}), ("light from the hit point", dict(vertex_light=False)),
                           ("three-vector normal", dict(normal_w=False)), ("both", dict(vertex_light=False, normal_w=False))):
        for ambient, diff in oracle_differences(name, shading, oracle_geometry[name], **switches).items():
            print(f"ray caster ({what}), {name}, {shading}, ambient {ambient}: largest difference {diff.max():.3f} grey levels, mean "
                  f"{diff.mean():.3f}, 99.9 % below {np.quantile(diff, 0.999):.3f}, over {kept} of {covered} covered pixels")
            worst[what] = max(worst.get(what, 0.0), float(diff.max()))
    # with the two named terms taken out of the ray caster nothing is left but the rounding to uint8
    assert worst["both"] <= ROUNDING_BAR, worst
    # the shaders as they are written: the measured maximum plus one grey level, per scene and shading
    assert worst["shaders"] <= MEASURED_ORACLE[(name, shading)] + 1.0, worst
