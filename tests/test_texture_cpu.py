"""CPU-only checks of the textured renderer (include/pvnet_texture.h, libpvnet_texture.so, pvnet_amd/texture.py): the registry row, the
header's constants against pvnet_amd/_abi.py, the completeness of every side library's build dependencies, the built library and its
assembly, every bad argument rejected before any HIP call, ``TexturedMeshes`` and ``read_textured_ply``, and the numpy restatement
(tests/texture_restatement.py): a known answer that needs no restatement to state, perspective against affine interpolation, an
independent float64 ray caster, and the depth and shade restatements on the same inputs.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from pvnet_amd import _abi, build, render, shade, texture
from tests import depth_restatement as DR
from tests import shade_restatement as SR
from tests import test_shade_cpu as TS   # its oracle: the scenes, the ray caster, the GLSL shading; its PLY writer
from tests import texture_restatement as TR
from tests.render_cases import (BADARG, UNSUPPORTED, WORKSPACE, camera, i32, pose, refuses_the_pvnet_render_list, smooth_colors,
                                smooth_texture, spherical_uv)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_texture.h")).read()
EXPORTS = {"pvnet_texture_abi_version", "pvnet_texture_workspace_bytes", "pvnet_render_textured"}
KERNELS = (b"texture_setup_kernel", b"texture_clear_kernel", b"texture_tri_kernel", b"texture_resolve_kernel")
H, W = 48, 64


@pytest.fixture(scope="module")
def lib():
    build.build_side("texture")
    return _abi.load_texture_library()


# ---- 1. the registry row and the ABI mirror ---------------------------------------------------------------------------------------------
def test_registry_row():
    core, plane = os.path.join(build.CSRC, "mesh_core.h"), os.path.join(build.CSRC, "depth_core.h")
    zbuffer, color = os.path.join(build.CSRC, "zbuffer_core.h"), os.path.join(build.CSRC, "pixel_color.h")
    assert build.SIDE_LIBRARIES["texture"] == (["texture.hip"], "pvnet_texture.h", [zbuffer, color])
    assert list(build.SIDE_LIBRARIES)[-1] == "texture" == list(_abi.SIDE_LIBRARIES)[-1]
    assert _abi.SIDE_LIBRARIES["texture"] == (_abi.TEXTURE_LIB_PATH, _abi.TEXTURE_ABI_VERSION, _abi.TEXTURE_PROTOTYPES)
    assert _abi.load_texture_library.args == ("texture",)
    # each shared header holds its bodies under its own guard
    for header, guard, body in (("mesh_core.h", "PVNET_MESH_CORE_H_", "same_side"), ("depth_core.h", "PVNET_DEPTH_CORE_H_", "pixel_depth"),
                                ("zbuffer_core.h", "PVNET_ZBUFFER_CORE_H_", "tri_body"), ("pixel_color.h", "PVNET_PIXEL_COLOR_H_", "pixel_color")):
        text = open(os.path.join(build.CSRC, header)).read()
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        assert f"#ifndef {guard}" in code and "__device__" in code and body in code, header
    # each shared header rebuilds the libraries that compile it, and nothing else
    assert {n for n in build.SIDE_LIBRARIES if core in build._side(n)[1]} == {"raster", "depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if plane in build._side(n)[1]} == {"depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if zbuffer in build._side(n)[1]} == {"depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if color in build._side(n)[1]} == {"shade", "texture"}
    assert "_abi.load_texture_library()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import pvnet_amd   # the front end is exported from the package
    for name in ("TexturedMeshes", "render_textured", "read_textured_ply", "texture_workspace_bytes"):
        assert getattr(pvnet_amd, name) is getattr(texture, name) and name in pvnet_amd.__all__


def test_abi_version_and_constants_are_mirrored():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS == set(_abi.TEXTURE_PROTOTYPES)
    decl = re.search(r"^int pvnet_render_textured\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.TEXTURE_PROTOTYPES["pvnet_render_textured"][1]
    assert len(decl) == len(args) == 38
    # pvnet_render_color's list through normals, and its tail behind the six new arguments
    color_args = _abi.SHADE_PROTOTYPES["pvnet_render_color"][1]
    color_decl = re.search(r"^int pvnet_render_color\s*\((.*?)\);", open(os.path.join(ROOT, "include", "pvnet_shade.h")).read(),
                           re.M | re.S).group(1).split(",")
    assert args[:20] == color_args[:20] and args[26:] == color_args[20:]
    norm = lambda d: " ".join(d.split())   # noqa: E731
    assert [norm(d) for d in decl[:20]] == [norm(d) for d in color_decl[:20]] and [norm(d) for d in decl[26:]] == [norm(d) for d in color_decl[20:]]
    for k, (word, typ) in {19: ("double* normals", C.c_void_p), 20: ("const float* uv", C.c_void_p), 21: ("const uint32_t* texels", C.c_void_p),
                           22: ("const int64_t* tex_offset", _abi._i64p), 23: ("const int32_t* tex_h", _abi._i32p),
                           24: ("const int32_t* tex_w", _abi._i32p), 25: ("int filter", C.c_int), 26: ("int shading", C.c_int),
                           27: ("float ambient", C.c_float), 37: ("stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)
    assert _abi.TEXTURE_PROTOTYPES["pvnet_texture_workspace_bytes"] == _abi.SHADE_PROTOTYPES["pvnet_shade_workspace_bytes"]
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_TEXTURE_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.TEXTURE_ABI_VERSION == 1
    assert consts.pop("WS_COOP_COUNT_OFFSET") == 0
    assert len(consts) == 15
    for name, value in consts.items():
        assert getattr(_abi, "TEXTURE_" + name) == value, name
    # the limits and codes of the shade library under this header's names
    same_name = {"LANE_PIXELS", "MAX_INSTANCES", "MAX_MESHES", "MAX_IMAGES", "MAX_FACES", "S_NONFINITE", "S_BEHIND", "S_BADFACE"}
    renamed = {"MAX_IMAGE_SIDE": "MAX_SIDE", "SHADING_NONE": "NONE", "SHADING_FLAT": "FLAT", "SHADING_PHONG": "PHONG"}
    for name in same_name:
        assert consts[name] == getattr(_abi, "SHADE_" + name), name
    for name, theirs in renamed.items():
        assert consts[name] == getattr(_abi, "SHADE_" + theirs), name
    assert set(consts) - same_name - set(renamed) == {"MAX_SIDE", "NEAREST", "BILINEAR"}
    assert _abi.TEXTURE_MAX_SIDE == 16384 and (_abi.TEXTURE_NEAREST, _abi.TEXTURE_BILINEAR) == (0, 1) == (TR.NEAREST, TR.BILINEAR)
    assert texture.FILTER == TR.FILTER and texture.SHADING is shade.SHADING
    for said in ("THIS PROJECT'S OWN definition", "a belief, not a checked fact", "alpha is ignored", "no mip levels and no repeat wrap"):
        assert said in " ".join(HDR.replace("*", " ").split()), said


# ---- 2. build dependencies ---------------------------------------------------------------------------------------------------------------
def reachable(sources):
    """the files of pvnet_amd/csrc/ reachable from ``sources`` through #include "..." (this test's own walk of the text)"""
    seen, todo = set(), list(sources)
    while todo:
        path = todo.pop()
        for inc in re.findall(r'#\s*include\s*"([^"]+)"', open(path).read()):
            nxt = os.path.join(build.CSRC, inc)
            if os.path.exists(nxt) and nxt not in seen:
                seen.add(nxt)
                todo.append(nxt)
    return seen


@pytest.mark.parametrize("name", sorted(build.SIDE_LIBRARIES))
def test_build_dependencies_are_complete(name):
    src, deps, _ = build._side(name)
    assert len(deps) == len(set(deps)) and all(os.path.exists(d) for d in deps)
    missing = reachable(src) - set(deps)
    assert not missing, missing
    assert reachable(deps) <= set(deps)   # closed: a listed header's own includes are listed too


SHARED = {"raster": {"mesh_core.h"}, "depth": {"mesh_core.h", "depth_core.h", "zbuffer_core.h"},
          "shade": {"mesh_core.h", "depth_core.h", "zbuffer_core.h", "pixel_color.h"},
          "texture": {"mesh_core.h", "depth_core.h", "zbuffer_core.h", "pixel_color.h"}}   # the shared headers each renderer compiles


def test_texture_reaches_the_inner_headers_only():
    every = set().union(*SHARED.values())
    common = {"vote_common.h", "pvnet_rng.h"}   # what every library of the project compiles
    assert every == {os.path.basename(p) for p in reachable([os.path.join(build.CSRC, "texture.hip")])} - common
    for name, want in SHARED.items():   # what a library's sources reach, and what rebuilds it: these and no other shared header
        names = {os.path.basename(p) for p in reachable(build._side(name)[0])}
        assert names - common == want and "vote_common.h" in names, name
        assert {os.path.basename(p) for p in build._side(name)[1]} & every == want, name
    for gone in ("mesh_stages.h", "depth_plane.h", "raster_common.h"):   # no forwarding header is left
        assert not os.path.exists(os.path.join(build.CSRC, gone)), gone
    # a library is stale when a shared header is newer than it
    for name, want in SHARED.items():
        _, deps, target = build._side(name)
        assert all(os.path.join(build.CSRC, header) in deps for header in want)
        assert build.fresh(target, deps) == (os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps))
    with tempfile.NamedTemporaryFile() as target:
        for header in sorted(every):
            path = os.path.join(build.CSRC, header)
            stamp = os.path.getmtime(path)
            os.utime(target.name, (stamp - 10, stamp - 10))
            assert not build.fresh(target.name, [path]), header
            os.utime(target.name, (stamp, stamp))
            assert build.fresh(target.name, [path]), header


def test_the_z_buffer_and_the_pixel_colour_are_written_once():
    """the sharing is real: among the translation units and headers of the three z-buffer libraries, the atomic minimum of the walk, the
    call that makes a triangle's depth plane and the resolve kernels' pixel split each occur in exactly one file"""
    files = set()
    for name in ("depth", "shade", "texture"):
        files |= {p for p in build._side(name)[1] if os.path.dirname(p) == build.CSRC}
    assert {os.path.basename(p) for p in files} >= {"depth.hip", "shade.hip", "texture.hip", "zbuffer_core.h", "pixel_color.h"}
    code = {p: "\n".join(line.split("//")[0] for line in open(p).read().splitlines()) for p in files}
    for what, where in (("atomicMin(", "zbuffer_core.h"), ("= make_plane(", "zbuffer_core.h"), ("__umul64hi(", "pixel_color.h")):
        assert [os.path.basename(p) for p, text in code.items() if what in text] == [where], what


# ---- 3. the built library ----------------------------------------------------------------------------------------------------------------
def test_library_is_built_with_its_exports_and_none_of_the_other_libraries_kernels(lib):
    assert lib.pvnet_texture_abi_version() == 1
    blob = open(_abi.TEXTURE_LIB_PATH, "rb").read()
    for kernel in KERNELS:
        assert kernel in blob
    for other in (b"shade_tri_kernel", b"shade_resolve_kernel", b"shade_setup_kernel", b"shade_clear_kernel", b"depth_tri_kernel",
                  b"depth_resolve_kernel", b"depth_setup_kernel", b"depth_clear_kernel", b"triangle_kernel", b"expand_kernel"):
        assert other not in blob
    for name in ("raster", "depth", "shade"):   # and no other library holds a kernel of this one
        other = open(_abi.SIDE_LIBRARIES[name].path, "rb").read()
        assert not any(kernel in other for kernel in KERNELS), name
    raw = C.CDLL(_abi.TEXTURE_LIB_PATH)
    for fn in ("pvnet_render", "pvnet_render_depth", "pvnet_render_color", "pvnet_shade_workspace_bytes", "pvnet_vote_v3"):
        assert not hasattr(raw, fn), fn
    for fn in EXPORTS:
        assert hasattr(raw, fn), fn


# ---- 4. the assembly ---------------------------------------------------------------------------------------------------------------------
def test_assembly_one_atomic_minimum_nothing_contracted_and_the_register_rule():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--texture"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "checked 4 kernels, 0 without" in r.stdout
    assert all("scratch   0 B" in line for line in r.stdout.splitlines() if " allocates " in line)   # no spills
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as CK
    (_, asm), = CK.side_assembly("texture")
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())
    by_kernel = {name: "\n".join(c) for name, (c, _) in CK.kernel_code(asm).items()}
    assert len(by_kernel) == 4
    tri, = [c for n, c in by_kernel.items() if "texture_tri_kernel" in n]
    # as in the shade library: one 64-bit unsigned minimum on each of the triangle kernel's two paths, no compare-and-swap loop
    assert len(re.findall(r"\bglobal_atomic_umin_x2\b", code)) == 2 == len(re.findall(r"\bglobal_atomic_umin_x2\b", tri))
    assert "cmpswap" not in code
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)(mk|ak)?_f32\b", code)
    # float64: the only fused operations are those of the divisions' and square roots' own expansions.  Divisions: the shade library's
    # 13 + 22 (tests/test_shade_cpu.py) and the two of u = A(u_.) and v = A(v_.); the texel blend has none.  Square roots: |e|, |g|, |n|.
    divisions, roots = len(re.findall(r"\bv_div_fixup_f64\b", code)), len(re.findall(r"\bv_rsq_f64", code))
    assert (divisions, roots) == (13 + 22 + 2, 3)
    per_division, per_root = TS.fused_f64_per("a / b"), TS.fused_f64_per("sqrt(a)")
    assert per_division > 0 and per_root > 0 and TS.fused_f64_per("a * b + a") == 0
    assert len(re.findall(r"\bv_(fma|fmac)_f64(_e32|_e64)?\b", code)) == per_division * divisions + per_root * roots
    assert "v_mul_f64" in code and "v_add_f64" in code and "v_floor_f64" in code
    modes = re.findall(r"\.amdhsa_float_denorm_mode_32 (\d)", asm) + re.findall(r"\.amdhsa_float_denorm_mode_16_64 (\d)", asm)
    assert len(modes) == 8 and set(modes) == {"3"}   # denormals kept in every kernel
    # the instance table and the textures' sides travel in the setup kernel's arguments: within the 4 KB a launch may carry
    assert max(int(n) for n in re.findall(r"\.amdhsa_kernarg_size (\d+)", asm)) <= 4096
    for banned in ("printf", "__assert_fail"):
        assert banned not in asm


# ---- 5. bad arguments --------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_is_the_shade_librarys(lib):
    build.build_side("shade")
    f, g = lib.pvnet_texture_workspace_bytes, _abi.load_shade_library().pvnet_shade_workspace_bytes
    for q in (0, 1, 4, 768, 769):
        for b in (0, 1, 3):
            for h, w in ((2, 2), (33, 47), (48, 64), (480, 640), (32768, 2)):
                for P, T in ((0, 0), (100, 200)):
                    assert f(q, P, T, b, h, w) == g(q, P, T, b, h, w) > 0, (q, P, T, b, h, w)
    base = dict(q=4, P=100, T=200, b=2, h=60, w=80)
    for bad in (dict(h=1), dict(w=1), dict(h=0), dict(w=-5), dict(q=-1), dict(P=-1), dict(T=-1), dict(b=-1), dict(h=40000), dict(w=32769)):
        assert f(*{**base, **bad}.values()) == 0 == g(*{**base, **bad}.values()), bad


def test_bad_arguments_are_rejected_without_a_device(lib):
    p = C.c_void_p(0x1000)   # never dereferenced: validation returns before any HIP call
    i64 = lambda *v: (C.c_int64 * len(v))(*v)   # noqa: E731
    voff, foff = i32(0, 12, 20), i32(0, 20, 32)
    ws_n = lib.pvnet_texture_workspace_bytes(3, 20, 32, 2, 20, 24)
    black = (C.c_uint8 * 3)(0, 0, 0)

    def call(vertices=p, faces=p, voff=voff, foff=foff, M=2, P=20, T=32, q=3, mesh=i32(0, 1, 1), poses=p, K=p, kper=0,
             image=i32(0, 0, 1), label=i32(1, 2, 3), b=2, h=20, w=24, far=float("inf"), colors=p, normals=None, uv=p, texels=p,
             toff=i64(0, 15, 15), th=i32(5, 0), tw=i32(3, 0), filt=0, shading=1, ambient=0.5, bg=black, bg_image=None, rgb=p, depth=None,
             labels=None, visible=None, status=None, ws=p, nbytes=ws_n):
        return lib.pvnet_render_textured(vertices, faces, voff, foff, M, P, T, q, mesh, poses, K, kper, image, label, b, h, w, far, colors,
                                         normals, uv, texels, toff, th, tw, filt, shading, ambient, bg, bg_image, rgb, depth, labels, visible,
                                         status, ws, nbytes, None)

    good = dict(b=0, q=0)   # the all-good call would reach the device: b == 0 enqueues nothing
    assert call(**good) == 0 and call(**good, filt=1, shading=2, normals=p, bg_image=p) == 0
    # what is new.  A textured mesh without uv or texels
    assert call(uv=None) == BADARG and call(texels=None) == BADARG and call(**good, uv=None) == BADARG
    assert call(**good, uv=None, texels=None, toff=i64(0, 0, 0), th=i32(0, 0), tw=i32(0, 0)) == 0   # nothing textured: neither is needed
    # the host arrays themselves
    assert call(toff=None) == BADARG and call(th=None) == BADARG and call(tw=None) == BADARG
    # sides negative, or only one of them zero
    assert call(th=i32(-5, 0), tw=i32(-3, 0)) == BADARG and call(th=i32(5, -1)) == BADARG and call(tw=i32(3, -1)) == BADARG
    assert call(th=i32(5, 0), tw=i32(0, 0), toff=i64(0, 0, 0)) == BADARG and call(th=i32(0, 0), tw=i32(3, 0), toff=i64(0, 0, 0)) == BADARG
    assert call(th=i32(5, 2), tw=i32(3, 0), toff=i64(0, 15, 15)) == BADARG
    # offsets that do not increase by th * tw
    for toff in (i64(0, 14, 14), i64(0, 16, 16), i64(1, 16, 16), i64(0, 15, 16), i64(0, 15, 14), i64(0, 0, 15), i64(-15, 0, 0)):
        assert call(toff=toff) == BADARG, list(toff)
    assert call(**good, toff=i64(0, 15, 19), th=i32(5, 2), tw=i32(3, 2)) == 0
    # a filter outside 0 .. 1
    for filt in (-1, 2, 100):
        assert call(filt=filt) == BADARG, filt
    assert call(**good, filt=1) == 0
    # a side beyond the limit; 2^31 texels or more
    side = _abi.TEXTURE_MAX_SIDE
    assert call(th=i32(side + 1, 0), tw=i32(1, 0), toff=i64(0, side + 1, side + 1)) == UNSUPPORTED
    assert call(th=i32(1, 0), tw=i32(side + 1, 0), toff=i64(0, side + 1, side + 1)) == UNSUPPORTED
    assert call(**good, th=i32(side, 0), tw=i32(side, 0), toff=i64(0, side * side, side * side)) == 0
    assert call(**good, M=8, voff=i32(0, 12, *[20] * 7), foff=i32(0, 20, *[32] * 7), th=i32(*[side] * 8), tw=i32(*[side] * 8),
                toff=i64(*[k * side * side for k in range(9)])) == UNSUPPORTED   # 8 * 2^28 texels
    assert call(**good, M=8, voff=i32(0, 12, *[20] * 7), foff=i32(0, 20, *[32] * 7), th=i32(*[side] * 7, side - 1), tw=i32(*[side] * 8),
                toff=i64(*[k * side * side for k in range(8)], 8 * side * side - side)) == 0   # 2^31 - 2^14
    # colours may be absent only when every mesh an instance names is textured
    assert call(colors=None) == BADARG                                       # instances 1 and 2 name the untextured mesh 1
    assert call(colors=None, mesh=i32(0, 0, 0), nbytes=0) == WORKSPACE       # every check passed but the last
    assert call(colors=None, mesh=i32(0, 0, 0), th=i32(0, 0), tw=i32(0, 0), toff=i64(0, 0, 0)) == BADARG
    assert call(colors=None, th=i32(5, 1), tw=i32(3, 1), toff=i64(0, 15, 16), nbytes=0) == WORKSPACE
    # what pvnet_render_color rejects
    assert call(rgb=None) == BADARG and call(bg=None) == BADARG
    for shading in (-1, 3):
        assert call(shading=shading) == BADARG, shading
    for ambient in (float("nan"), -0.5, float("inf")):
        assert call(ambient=ambient) == BADARG, ambient
    assert call(shading=2) == BADARG   # Phong without normals
    for far in (0.0, -1.0, float("nan")):
        assert call(far=far) == BADARG, far
    refuses_the_pvnet_render_list(call, ws_n, _abi.TEXTURE_MAX_MESHES, _abi.TEXTURE_MAX_INSTANCES, _abi.TEXTURE_MAX_IMAGE_SIDE,
                                  _abi.TEXTURE_MAX_IMAGES)
    big = _abi.TEXTURE_MAX_FACES + 1
    assert call(M=1, voff=i32(0, 20), foff=i32(0, big), T=big, mesh=i32(0, 0, 0), toff=i64(0, 15)) == UNSUPPORTED


# ---- 6. TexturedMeshes -------------------------------------------------------------------------------------------------------------------
def test_textured_meshes_validation_and_packing():
    rng = np.random.default_rng(6)
    v, f = render.icosphere(1, 0.1)
    P = len(v)
    col, uv = smooth_colors(v), spherical_uv(v)
    rgb = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (5, 3, 1), dtype=np.uint8)], 2)
    assert np.array_equal(texture.pack_texels(rgb), texture.pack_texels(rgba)) and texture.pack_texels(rgb).dtype == np.uint32
    words = texture.pack_texels(rgb)
    assert words.shape == (5, 3) and int(words[1, 2]) == int(rgb[1, 2, 0]) | int(rgb[1, 2, 1]) << 8 | int(rgb[1, 2, 2]) << 16
    assert (words >> 24 == 0).all()
    one, big = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    box = render.box_mesh(0.1, 0.2, 0.3)
    table = texture.TexturedMeshes([(v, f, col, None, uv, one), (v, f, None, None, uv, rgba), (*box, np.full((8, 3), 200), None, None, None),
                                    (v, f, col, None, uv.astype(np.float32), big)])
    assert isinstance(table, shade.ColorMeshes) and table.count == 4 and table.total_vertices == 3 * P + 8
    assert table.tex_offset.tolist() == [0, 1, 16, 16, 16 + 4096] and table.tex_offset.dtype == np.int64
    assert table.tex_h.tolist() == [1, 5, 0, 64] and table.tex_w.tolist() == [1, 3, 0, 64] and table.tex_h.dtype == np.int32
    assert list(table._c_toff) == table.tex_offset.tolist() and list(table._c_th) == [1, 5, 0, 64] and list(table._c_tw) == [1, 3, 0, 64]
    assert table.texels.dtype == np.uint32 and table.texels.shape == (16 + 4096,)
    assert np.array_equal(table.texels[1:16].reshape(5, 3), words) and np.array_equal(table.texels[16:].reshape(64, 64), texture.pack_texels(big))
    assert table.uv.dtype == np.float32 and table.uv.shape == (3 * P + 8, 2) and np.array_equal(table.uv[:P], uv.astype(np.float32))
    assert not table.uv[2 * P:2 * P + 8].any()
    assert not table.colors[P:2 * P].any() and np.array_equal(table.colors[:P], col)   # textured and no colours: zeros
    mv, mf, mc, mn, muv, mtex = table.mesh(1)
    assert np.array_equal(mtex, rgb) and mtex.dtype == np.uint8 and np.array_equal(muv, uv.astype(np.float32)) and len(mf) == len(f)
    assert table.mesh(2)[5] is None and np.array_equal(table.mesh(3)[5], big[..., :3])
    wild = uv.copy()
    wild[0], wild[1], wild[2] = (np.nan, 2.0), (np.inf, -np.inf), (-3.0, 1e30)
    assert np.isnan(texture.TexturedMeshes([(v, f, None, None, wild, rgb)]).uv[0, 0])   # uv is taken as it is, finite or not
    for bad in ([(v, f, col, None, None, rgb)],                      # a texture without uv
                [(v, f, None, None, None, None)],                    # neither colours nor a texture
                [(v, f, None, None, uv, None)],                      # uv alone is no texture
                [(v, f, col, None, uv, rgb.astype(np.float32))],     # not uint8
                [(v, f, col, None, uv, rgb.astype(np.int32))],
                [(v, f, col, None, uv, rgb[..., :2])], [(v, f, col, None, uv, rgb[0])], [(v, f, col, None, uv, rgb[:0])],
                [(v, f, col, None, uv[:-1], rgb)], [(v, f, col, None, uv.T, rgb)],
                [(v, f, col, None)], [(v, f, col)],
                [(v, f, col, None, uv, np.zeros((1, _abi.TEXTURE_MAX_SIDE + 1, 3), np.uint8))]):
        with pytest.raises(ValueError):
            texture.TexturedMeshes(bad)


# ---- 7. read_textured_ply ----------------------------------------------------------------------------------------------------------------
def write_ply(path, v, f, binary, uv=None, names=("texture_u", "texture_v"), colors=None):
    cols = [("x", "<f4", v[:, 0]), ("y", "<f4", v[:, 1]), ("z", "<f4", v[:, 2])]
    if colors is not None:
        cols += [("red", "u1", colors[:, 0]), ("green", "u1", colors[:, 1]), ("blue", "u1", colors[:, 2])]
    if uv is not None:
        cols += [(names[0], "<f4", uv[:, 0]), (names[1], "<f4", uv[:, 1])]
    kinds = {"<f4": "float", "u1": "uchar"}
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(v)] + \
        ["property %s %s" % (kinds[t], n) for n, t, _ in cols] + ["element face %d" % len(f), "property list uchar int vertex_indices",
                                                                  "end_header"]
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
                fh.write((" ".join(repr(float(val[i])) if t == "<f4" else str(int(val[i])) for _, t, val in cols) + "\n").encode())
            for face in f:
                fh.write(("3 %d %d %d\n" % tuple(face)).encode())


@pytest.mark.parametrize("binary", [False, True])
def test_read_textured_ply_round_trips(tmp_path, binary):
    v, f = render.icosphere(1, 0.1)
    v32, col = v.astype(np.float32), smooth_colors(v)
    uv = spherical_uv(v).astype(np.float32)
    for names in (("texture_u", "texture_v"), ("u", "v"), ("s", "t")):
        path = str(tmp_path / ("%s.ply" % names[0]))
        write_ply(path, v32, f, binary, uv, names, col)
        got = texture.read_textured_ply(path)
        assert got["uv"].dtype == np.float32 and got["uv"].shape == (len(v), 2) and np.array_equal(got["uv"], uv)
        plain = shade.read_ply(path)   # ... which returns what it returned before: no new key, the same arrays
        assert set(plain) == {"vertices", "faces", "normals", "colors"} and set(got) == set(plain) | {"uv"}
        for key in plain:
            assert (plain[key] is None and got[key] is None) or np.array_equal(plain[key], got[key]), key
        assert np.array_equal(plain["vertices"], v32.astype(np.float64)) and np.array_equal(plain["faces"], f)
        assert np.array_equal(plain["colors"], col) and plain["normals"] is None
        texture.TexturedMeshes([(got["vertices"], got["faces"], got["colors"], got["normals"], got["uv"], np.zeros((2, 2, 3), np.uint8))])
    bare = str(tmp_path / "bare.ply")
    write_ply(bare, v32, f, binary)
    got = texture.read_textured_ply(bare)
    assert got["uv"] is None and got["colors"] is None and np.array_equal(got["faces"], f)
    half = str(tmp_path / "half.ply")   # texture_u without texture_v is no uv; the reference's spelling wins over the others
    write_ply(half, v32, f, binary, uv, ("texture_u", "t"))
    assert texture.read_textured_ply(half)["uv"] is None
    # shade.read_ply on the shade tests' own files, through the helper both readers share
    full = str(tmp_path / "full.ply")
    TS.write_ply(full, v32, f, col, shade.vertex_normals(v, f), binary=binary, extra=True)
    plain, got = shade.read_ply(full), texture.read_textured_ply(full)
    assert got["uv"] is None and np.array_equal(plain["normals"], shade.vertex_normals(v, f)) and np.array_equal(got["normals"], plain["normals"])
    with pytest.raises(ValueError):
        texture.read_textured_ply(__file__)


# ---- 8. a known answer ------------------------------------------------------------------------------------------------------------------
QUAD_K = np.array([[64.0, 0.0, 31.5], [0.0, 64.0, 23.5], [0.0, 0.0, 1.0]])
QUAD_V = np.array([[-0.25, -0.25, 1.0], [0.25, -0.25, 1.0], [0.25, 0.25, 1.0], [-0.25, 0.25, 1.0]])   # image y points down:
QUAD_UV = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0], [0.0, 0.0]])                                     # top left, top right, bottom right, bottom left
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
BG = (12, 200, 77)


def quad_mesh(tex):
    return (QUAD_V, QUAD_F, np.zeros((4, 3), np.uint8), None, QUAD_UV, tex)


def test_known_answer_every_texel_is_a_four_by_four_block():
    """Every operand is a dyadic rational: the screen quad is exactly [15.5, 47.5] x [7.5, 39.5], the barycentrics of a pixel centre
    are multiples of 1 / 64, z = 1, so u = (px - 15.5) / 32 and v = 1 - (py - 7.5) / 32 exactly.  An 8 x 8 texture is then magnified
    four times with no pixel on a texel boundary.  This pins the flip, the axis order and the texel centres without the code under
    test."""
    tex = np.random.default_rng(8).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    rgb, depth, label, visible, status = TR.render([quad_mesh(tex)], [(0, EYE, QUAD_K, 0, 5)], 1, H, W, shading="none",
                                                   filter="nearest", background=BG)
    want = np.empty((H, W, 3), np.uint8)
    want[:] = BG
    want[8:40, 16:48] = np.kron(tex, np.ones((4, 4, 1), np.uint8))
    assert np.array_equal(rgb[0], want)
    assert visible.tolist() == [32 * 32] and status.tolist() == [0] and (label[0, 8:40, 16:48] == 5).all() and int((label != 0).sum()) == 1024
    assert (depth[0, 8:40, 16:48] == 1.0).all()
    # flat shading at ambient 1 saturates the light: the same image; the four corners name the four corner texels
    lit, _, _, _, _ = TR.render([quad_mesh(tex)], [(0, EYE, QUAD_K, 0, 5)], 1, H, W, shading="flat", ambient=1.0, background=BG)
    assert np.array_equal(lit, rgb)
    assert np.array_equal(rgb[0, 8, 16], tex[0, 0]) and np.array_equal(rgb[0, 8, 47], tex[0, 7])
    assert np.array_equal(rgb[0, 39, 16], tex[7, 0]) and np.array_equal(rgb[0, 39, 47], tex[7, 7])
    # bilinear: a pixel centre is 1/8 or 3/8 of a texel from the nearest texel centre; the answer in exact arithmetic, from the image
    pad = np.pad(tex.astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="edge")   # clamp to edge
    ys, xs = np.mgrid[8:40, 16:48]
    ty, tx = (ys - 7.5) / 4.0 - 0.5, (xs - 15.5) / 4.0 - 0.5     # in texel units from the top-left texel's centre
    j0, i0 = np.floor(ty).astype(int), np.floor(tx).astype(int)
    fy, fx = (ty - j0)[..., None], (tx - i0)[..., None]
    exact = (1 - fy) * ((1 - fx) * pad[j0 + 1, i0 + 1] + fx * pad[j0 + 1, i0 + 2]) + fy * ((1 - fx) * pad[j0 + 2, i0 + 1] + fx * pad[j0 + 2, i0 + 2])
    soft, _, _, _, _ = TR.render([quad_mesh(tex)], [(0, EYE, QUAD_K, 0, 5)], 1, H, W, shading="none", filter="bilinear", background=BG)
    assert np.array_equal(soft[0, 8:40, 16:48], np.floor(exact + 0.5).astype(np.uint8))   # (weights of k / 8: every product is exact)
    assert (soft[0][label[0] == 0] == BG).all()


# ---- 9. perspective ----------------------------------------------------------------------------------------------------------------------
def test_perspective_and_affine_interpolation_differ_on_a_turned_quad():
    checker = np.zeros((16, 16, 3), np.uint8)
    checker[(np.add.outer(np.arange(16), np.arange(16)) % 2) == 0] = (250, 240, 230)
    p = pose((0, 1, 0), np.pi / 3, (0.0, 0.0, 0.6))   # the quad about its own centre: its near edge at z = 0.38, its far one at 0.82
    centred = (QUAD_V - (0.0, 0.0, 1.0),) + quad_mesh(checker)[1:]
    inst = [(0, p, QUAD_K, 0, 1)]
    layers = {}
    persp, _, label, _, status = TR.render([centred], inst, 1, H, W, shading="none", layers=layers)
    affine, _, label2, _, _ = TR.render([centred], inst, 1, H, W, shading="none", layers=layers, affine=True)
    differing = int((persp != affine).any(-1).sum())
    print(f"perspective against affine uv: {differing} of {int((label != 0).sum())} covered pixels differ")
    assert status.tolist() == [0] and np.array_equal(label, label2) and int((label != 0).sum()) > 200
    assert not np.array_equal(persp, affine) and differing > 0
    assert np.array_equal(persp[label == 0], affine[label == 0])
    # seen head on both are the same image: z is the same at the three vertices
    flat = [(0, EYE, QUAD_K, 0, 1)]
    assert np.array_equal(TR.render([quad_mesh(checker)], flat, 1, H, W, shading="none")[0],
                          TR.render([quad_mesh(checker)], flat, 1, H, W, shading="none", affine=True)[0])


# ---- 10. the independent ray caster ------------------------------------------------------------------------------------------------------
def atlas_box(sx, sy, sz):
    """render.box_mesh with four vertices of its own per side and a cell of a 3 x 2 atlas per side (inset by 1/16 of a cell): the same
    twelve triangles in the same order, so coverage and face indices are box_mesh's"""
    v, f = render.box_mesh(sx, sy, sz)
    vs, fs, uvs = [], [], []
    corner = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    for side in range(6):
        (a, b, c), (a2, c2, d) = f[2 * side], f[2 * side + 1]
        assert a == a2 and c == c2
        base = len(vs)
        vs += [v[a], v[b], v[c], v[d]]
        fs += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
        cell = np.array([side % 3, side // 3], np.float64)
        uvs += list((cell + 1 / 16 + corner * 7 / 8) / (3.0, 2.0))
    return np.asarray(vs), np.asarray(fs, np.int32), np.asarray(uvs)


def gl_bilinear(tex, u, v):
    """bilinear sampling with clamp to edge as OpenGL states it, on the image FLIPPED IN MEMORY (row 0 at the bottom, as the reference
    uploads it): written from that description, not from pvnet_texture.h, whose row formula folds the flip in"""
    t = np.flipud(np.asarray(tex)[..., :3]).astype(np.float64)
    th, tw = t.shape[:2]
    x, y = np.clip(u, 0, 1) * tw - 0.5, np.clip(v, 0, 1) * th - 0.5
    i0, j0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = (x - i0)[:, None], (y - j0)[:, None]
    ia, ib, ja, jb = np.clip(i0, 0, tw - 1), np.clip(i0 + 1, 0, tw - 1), np.clip(j0, 0, th - 1), np.clip(j0 + 1, 0, th - 1)
    return (1 - fy) * ((1 - fx) * t[ja, ia] + fx * t[ja, ib]) + fy * ((1 - fx) * t[jb, ia] + fx * t[jb, ib])


TEXTURE64 = smooth_texture()
# the texture's largest step between two neighbouring texels, along a row or a column, any channel
TEXEL_STEP = float(max(np.abs(np.diff(TEXTURE64.astype(np.float64), axis=0)).max(), np.abs(np.diff(TEXTURE64.astype(np.float64), axis=1)).max()))
# MEASURED (the docstring below): the largest |du| tw and |dv| th between the restatement and the ray caster, per scene, rounded up
MEASURED_SHIFT = {"sphere": 5.0e-5, "box": 3.0e-6}


def oracle_bar(name):
    """0.5 for the rounding to uint8, what the measured shift of (u, v) can move a bilinear texel value, and 0.01"""
    return 0.5 + MEASURED_SHIFT[name] * TEXEL_STEP + 0.01


@pytest.fixture(scope="module")
def textured_oracle():
    """per scene, computed once: the mesh with its uv, the restatement's winning faces, the ray caster's hits and interior pixels"""
    out = {}
    (sv, sf, scol, snrm), sp = TS.ORACLE_SCENES["sphere"]
    bv, bf, buv = atlas_box(0.3, 0.22, 0.26)
    scenes = {"sphere": ((sv, sf, snrm, spherical_uv(sv)), sp), "box": ((bv, bf, shade.vertex_normals(bv, bf), buv), TS.ORACLE_SCENES["box"][1])}
    for name, ((v, f, nrm, uv), p) in scenes.items():
        _, owner, status = SR.instance_layers(v, f, p, TS.ORACLE_K, TS.ORACLE_H, TS.ORACLE_W)
        assert status == 0
        hits = TS.ray_hits(v, f, p, TS.ORACLE_K, TS.ORACLE_H, TS.ORACLE_W)
        out[name] = ((v, f, nrm, uv), p, owner, hits, TS.interior_pixels(hits[0]))
    return out


@pytest.mark.parametrize("shading", ["none", "flat", "phong"])
@pytest.mark.parametrize("name", ["box", "sphere"])
def test_restatement_against_the_ray_caster(textured_oracle, name, shading):
    """The ray caster of tests/test_shade_cpu.py (Moeller-Trumbore in camera space) gives the TRUE object-space barycentrics of every
    hit; (u, v) is their combination of the vertices' uv, the texel the bilinear formula on the image flipped in memory, in float64,
    unrounded; the light is 1 (shading "none") or that ray caster's own with its two named terms switched off (flat, Phong: the
    definition's light, see that file).  Against it the restatement's uint8, bilinear filter, a smooth 64 x 64 texture whose largest
    texel-to-texel step is TEXEL_STEP = 9 grey levels, 240 x 320, interior pixels only (20 947 of 21 607 covered pixels on the sphere,
    20 943 of 21 629 on the box: 3.1 / 3.2 % left out, at most 10 % allowed).

    MEASURED, largest over the interior pixels (the same for the three shadings and both ambients):
                     |du| tw      |dv| th      |difference|, grey levels (mean)
        sphere       4.133e-05    1.087e-05    0.500 (0.249)
        box          1.820e-06    2.812e-06    0.500 (0.249)
    (the sphere's spherical uv has a seam: a face across it spans the whole texture, so the float32 rounding of a screen vertex moves
    u by more there; a cell of the box's atlas spans a third of it).  MEASURED_SHIFT rounds the larger of each row up: 5e-5 and 3e-6
    texels.  The bar is 0.5 (the rounding to uint8) + MEASURED_SHIFT x TEXEL_STEP + 0.01: 0.51045 on the sphere, 0.51003 on the box.
    profiles/texture_probe.txt records the same."""
    (v, f, nrm, uv), p, owner, hits, interior = textured_oracle[name]
    covered, kept = int(hits[0].sum()), int(interior.sum())
    assert covered > 10000 and covered - kept <= 0.10 * covered, (covered, kept)
    assert (owner[interior] >= 0).all()   # the restatement covers every interior pixel
    ys, xs = np.nonzero(interior)
    _, hit, bary = hits
    corners = np.asarray(f, np.int64)[hit[ys, xs]]
    true_uv = (np.asarray(uv, np.float32).astype(np.float64)[corners] * bary[ys, xs][..., None]).sum(1)
    texel = gl_bilinear(TEXTURE64, true_uv[:, 0], true_uv[:, 1])
    white = np.full((len(v), 3), 255, np.uint8)
    if shading == "none":
        lights = {ambient: np.ones(len(ys)) for ambient in TS.ORACLE_AMBIENTS}
    else:   # the light alone: that ray caster on a white mesh, its two named terms off
        lit = TS.glsl_shade(hits, v, f, white, nrm, p, TS.ORACLE_K, shading, TS.ORACLE_AMBIENTS, vertex_light=False, normal_w=False)
        lights = {ambient: lit[ambient][ys, xs, 0] / 255.0 for ambient in TS.ORACLE_AMBIENTS}
    worst = 0.0
    for ambient in TS.ORACLE_AMBIENTS:
        args = (v, f, white, nrm, uv, TEXTURE64, p, TS.ORACLE_K, owner[ys, xs], xs, ys, TR.SHADING[shading], ambient)
        got = TR.shade_pixels(*args, filter=TR.BILINEAR).astype(np.float64)
        _, got_uv = TR.shade_pixels(*args, filter=TR.BILINEAR, rounded=False)
        shift = np.abs(got_uv - true_uv) * (TEXTURE64.shape[1], TEXTURE64.shape[0])
        diff = np.abs(got - lights[ambient][:, None] * texel)
        print(f"textured ray caster, {name}, {shading}, ambient {ambient}: largest |du| tw {shift[:, 0].max():.3e}, |dv| th {shift[:, 1].max():.3e}; "
              f"largest difference {diff.max():.3f} grey levels, mean {diff.mean():.3f}, over {kept} of {covered} covered pixels; bar "
              f"{oracle_bar(name):.3f} (texel step {TEXEL_STEP:.0f})")
        assert got.max() > 100 and shift.max() <= MEASURED_SHIFT[name], (name, shift.max(0))
        worst = max(worst, float(diff.max()))
    assert worst <= oracle_bar(name), worst


# ---- 11. against the depth and shade restatements ----------------------------------------------------------------------------------------
def test_restated_geometry_is_the_depth_restatements_and_untextured_colour_the_shade_restatements():
    K = camera(H, W)
    rng = np.random.default_rng(20261019)
    tex = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    plain = TS.MESHES   # (vertices, faces, colours, normals)
    mixed = [(*m, spherical_uv(m[0]), tex if k % 2 == 0 else None) for k, m in enumerate(plain)]
    bare = [(*m, None, None) for m in plain]
    scenes = []
    for _ in range(2):   # three instances per image, two images, overlapping
        inst = []
        for img in range(2):
            for m in rng.choice(4, 3, replace=False):
                t = (rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05), rng.uniform(0.4, 0.7))
                inst.append((int(m), pose(rng.normal(size=3), rng.uniform(0, np.pi), t), K, img, int(rng.integers(1, 256))))
        scenes.append(inst)
    p = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))
    scenes.append([(1, p, K, 0, 3), (0, p.copy(), K, 0, 7)])
    for inst in scenes:
        layers = {}
        for far in (np.inf, 0.55):
            wd, wl, wv, wst = DR.render([m[:2] for m in plain], inst, 2, H, W, far)
            for filt in ("nearest", "bilinear"):
                rgb, depth, label, visible, status = TR.render(mixed, inst, 2, H, W, far=far, shading="flat", background=(9, 8, 7), filter=filt,
                                                               layers=layers)
                assert np.array_equal(depth.view(np.uint32), wd.view(np.uint32)) and np.array_equal(label, wl)
                assert np.array_equal(visible, wv) and np.array_equal(status, wst) and label.any()
                assert (rgb[label == 0] == (9, 8, 7)).all() and rgb.dtype == np.uint8 and rgb.shape == (2, H, W, 3)
            for shading in ("none", "flat", "phong"):
                want = SR.render(plain, inst, 2, H, W, far=far, shading=shading, ambient=0.3, background=(9, 8, 7), layers=layers)
                got = TR.render(bare, inst, 2, H, W, far=far, shading=shading, ambient=0.3, background=(9, 8, 7), filter="bilinear", layers=layers)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), shading
                # ... and a textured mesh's pixels differ from its vertex colours' while every other pixel is the shade restatement's
                tex_rgb = TR.render(mixed, inst, 2, H, W, far=far, shading=shading, ambient=0.3, background=(9, 8, 7), layers=layers)[0]
                textured = np.isin(want[2], [ins[4] for ins in inst if mixed[ins[0]][5] is not None])
                assert np.array_equal(tex_rgb[~textured], want[0][~textured]) and (tex_rgb[textured] != want[0][textured]).any()
    # a texture of one colour is that colour under shading "none", whatever uv, pose and filter
    one = np.tile(np.array([[[10, 128, 250]]], np.uint8), (2, 2, 1))
    v, f, _, n = plain[3]
    wild = spherical_uv(v) * 3 - 1
    wild[0], wild[1] = (np.nan, np.inf), (-np.inf, 0.5)
    for filt in ("nearest", "bilinear"):
        rgb, _, label, _, _ = TR.render([(v, f, None, n, wild, one)], [(0, p, K, 0, 1)], 1, H, W, shading="none", filter=filt)
        assert label.any() and (rgb[label != 0] == (10, 128, 250)).all()
