"""CPU-only checks of the mesh rasteriser (include/pvnet_raster.h, libpvnet_raster.so, pvnet_amd/render.py): the numpy restatement
(tests/raster_restatement.py) against what the reference's own function recorded (tests/golden/raster.npz), the fixture's power to
tell a contracted predicate from the defined one, the library's exports and header constants against pvnet_amd/_abi.py, every bad
argument rejected before any HIP call, the register rule, the absence of fused float32 arithmetic in the kernels, and DeviceMeshes'
validation.
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
from tests import raster_restatement as RS
from tests.render_cases import BADARG, UNSUPPORTED, WORKSPACE, i32, refuses_the_pvnet_render_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_raster.h")).read()
EXPORTS = {"pvnet_raster_abi_version", "pvnet_raster_workspace_bytes", "pvnet_raster_triangles", "pvnet_render"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "raster.npz"))


@pytest.fixture(scope="module")
def lib():
    build.build_side("raster")
    return _abi.load_raster_library()


def triangle_cases(G, group=None):
    for name in G["triangle_cases"]:
        if group is None or str(G[f"t.{name}.group"]) == group:
            h, w = (int(x) for x in G[f"t.{name}.size"])
            yield str(name), G[f"t.{name}.tri"], h, w, G[f"t.{name}.mask"]


def test_restatement_equals_every_recorded_reference_mask(golden):
    G = golden
    groups = {}
    for name, tri, h, w, ref in triangle_cases(G):
        mask, status = RS.rasterize(tri, h, w)
        assert status == 0 and np.array_equal(mask, ref), name
        groups[str(G[f"t.{name}.group"])] = groups.get(str(G[f"t.{name}.group"]), 0) + 1
    assert groups["soup"] == 40 and groups["contract"] >= 20 and groups["degenerate"] >= 6
    assert len(G["render_cases"]) >= 24
    for name in G["render_cases"]:
        h, w = (int(x) for x in G[f"r.{name}.size"])
        mask, status = RS.rasterize(G[f"r.{name}.tri"], h, w)
        assert status == 0 and np.array_equal(mask, G[f"r.{name}.mask"]), name
        assert mask.any() and not mask.all()


def test_the_consequences_the_definition_names(golden):
    G = golden
    count = {name: int(ref.sum()) for name, _, _, _, ref in triangle_cases(G, "degenerate")}
    assert count["point"] == 4 and count["collinear"] == 100 and count["outside_corner"] == 1 and count["denormal_products"] == 1
    assert G["t.outside_corner.mask"][0, 0] == 1 and G["t.denormal_products.mask"][0, 0] == 1
    last = G["t.point_last_column_row.mask"]   # column w - 1 and row h - 1 are reached through the `+ 1`
    assert last[-1, -1] == 1 and last.sum() == 4
    # flushing the denormal products to zero would set four pixels: the restatement keeps them
    tri = G["t.denormal_products.tri"]
    assert 0 < abs(float(tri[0, 1, 0])) and np.float32(tri[0, 1, 0]) * np.float32(tri[0, 2, 1]) != 0
    # deviations: non-finite triangles cover nothing and say so; a triangle at +-1e30 covers nothing
    for bad in (np.nan, np.inf, -np.inf):
        mask, status = RS.rasterize(np.array([[(1, 1), (5, bad), (3, 7)]], np.float32), 12, 12)
        assert status == RS.S_NONFINITE and not mask.any()
    for far in (1e30, -1e30):
        mask, status = RS.rasterize(np.array([[(far, 1), (far, 5), (far, 3)]], np.float32), 12, 12)
        assert status == 0 and not mask.any()


def test_projection_within_one_ulp_of_the_recorded_triangles(golden):
    G = golden
    for name in G["render_cases"]:
        mesh = str(G[f"r.{name}.mesh"])
        tri, status = RS.project_triangles(G[f"mesh.{mesh}.vertices"], G[f"mesh.{mesh}.faces"], G[f"r.{name}.pose"], G[f"r.{name}.K"])
        ref = G[f"r.{name}.tri"]
        assert status == 0 and tri.dtype == np.float32 and tri.shape == ref.shape
        assert (np.abs(tri - ref) <= np.spacing(np.abs(ref))).all(), name


def test_the_fixture_tells_a_contracted_predicate_apart(golden):
    differing = 0
    for name, tri, h, w, ref in triangle_cases(golden, "contract"):
        fused, _ = RS.rasterize(tri, h, w, contracted=True)
        differing += int(not np.array_equal(fused, ref))
    assert differing >= 20


def test_header_exports_constants_and_prototypes():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS
    decl = re.search(r"^int pvnet_render\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.RASTER_PROTOTYPES["pvnet_render"][1]
    for k, (word, typ) in {2: ("vertex_offset", _abi._i32p), 8: ("mesh_id", _abi._i32p), 12: ("image_id", _abi._i32p), 13: ("label", _abi._i32p),
                           14: ("order", C.c_void_p), 22: ("ws_bytes", C.c_size_t), 23: ("stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_RASTER_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.RASTER_ABI_VERSION == 1
    consts.pop("WS_COOP_COUNT_OFFSET")
    assert len(consts) == 8
    for name, value in consts.items():
        assert getattr(_abi, "RASTER_" + name) == value, name


def test_library_is_built_with_its_exports(lib):
    assert lib.pvnet_raster_abi_version() == 1
    blob = open(_abi.RASTER_LIB_PATH, "rb").read()
    assert b"triangle_kernel" in blob and b"expand_kernel" in blob
    assert build.SIDE_LIBRARIES["raster"][:2] == (["raster.hip"], "pvnet_raster.h")
    assert not hasattr(C.CDLL(_abi.RASTER_LIB_PATH), "pvnet_vote_v3")
    for path in (_abi.LIB_PATH, _abi.DEV_LIB_PATH):   # the vote library holds nothing of it
        if os.path.exists(path):
            assert b"triangle_kernel" not in open(path, "rb").read()


def test_workspace_bytes_is_monotone_and_rejects_bad_sizes(lib):
    f = lib.pvnet_raster_workspace_bytes
    base = dict(q=4, P=100, T=200, b=2, h=60, w=80)
    assert f(*base.values()) > 0 and f(*base.values()) % 16 == 0
    for name in base:
        prev = 0
        for step in (0, 1, 2, 7, 64, 1000):
            n = f(*{**base, name: base[name] + step}.values())
            assert n >= prev > -1, name
            prev = n
    assert f(4, 100, 200, 2, 61, 80) > f(4, 100, 200, 2, 60, 80) and f(5, 100, 200, 2, 60, 80) > f(4, 100, 200, 2, 60, 80)
    assert f(4, 100, 200, 2, 60, 97) > f(4, 100, 200, 2, 60, 96)
    for bad in (dict(h=1), dict(w=1), dict(h=0), dict(w=-5), dict(q=-1), dict(P=-1), dict(T=-1), dict(b=-1), dict(h=40000)):
        assert f(*{**base, **bad}.values()) == 0, bad
    assert f(0, 0, 0, 0, 2, 2) == 16


def test_bad_arguments_are_rejected_without_a_device(lib):
    p = C.c_void_p(0x1000)   # never dereferenced: validation returns before any HIP call
    ws_n = lib.pvnet_raster_workspace_bytes(3, 0, 10, 3, 20, 24)

    def tri(t=p, n=3, tn=10, h=20, w=24, out=p, status=p, ws=p, nbytes=ws_n):
        return lib.pvnet_raster_triangles(t, n, tn, h, w, out, status, ws, nbytes, None)

    assert tri(h=1) == BADARG and tri(w=1) == BADARG and tri(h=0) == BADARG and tri(w=-2) == BADARG
    assert tri(t=None) == BADARG and tri(out=None) == BADARG and tri(ws=None) == BADARG
    assert tri(n=-1) == BADARG and tri(tn=-1) == BADARG
    assert tri(ws=C.c_void_p(0x1008)) == BADARG                      # misaligned
    assert tri(nbytes=ws_n - 1) == WORKSPACE and tri(nbytes=0) == WORKSPACE
    assert tri(n=_abi.RASTER_MAX_IMAGES + 1) == UNSUPPORTED and tri(h=_abi.RASTER_MAX_SIDE + 1) == UNSUPPORTED
    assert tri(n=0) == 0                                              # nothing to do, nothing enqueued

    voff, foff = i32(0, 12, 20), i32(0, 20, 32)
    ws_r = lib.pvnet_raster_workspace_bytes(3, 20, 32, 2, 20, 24)

    def render(vertices=p, faces=p, voff=voff, foff=foff, M=2, P=20, T=32, q=3, mesh=i32(0, 1, 1), poses=p, K=p, kper=0,
               image=i32(0, 0, 1), label=i32(1, 2, 3), order=None, b=2, h=20, w=24, out=p, tri_out=None, status=None, ws=p, nbytes=ws_r):
        return lib.pvnet_render(vertices, faces, voff, foff, M, P, T, q, mesh, poses, K, kper, image, label, order, b, h, w, out, tri_out,
                                status, ws, nbytes, None)

    assert render(out=None) == BADARG                                # neither an image nor triangles asked for
    refuses_the_pvnet_render_list(render, ws_r, _abi.RASTER_MAX_MESHES, _abi.RASTER_MAX_INSTANCES, _abi.RASTER_MAX_SIDE,
                                  _abi.RASTER_MAX_IMAGES)


def test_register_rule_and_no_fused_float32_arithmetic():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--raster"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "checked 4 kernels, 0 without" in r.stdout
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as CK
    (_, asm), = CK.side_assembly("raster")
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())
    # the predicate has no division: ANY fused float32 multiply-add in this translation unit would be a contraction
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)(mk|ak)?_f32\b", code)
    assert "v_mul_f32" in code and "v_add_f32" in code and "v_mul_f64" in code
    # float32 denormals kept in every kernel
    modes = re.findall(r"\.amdhsa_float_denorm_mode_32 (\d)", asm)
    assert len(modes) == 4 and set(modes) == {"3"}
    for banned in ("printf", "__assert_fail"):
        assert banned not in asm


def test_device_meshes_validate_on_the_host():
    from pvnet_amd import render
    v, f = render.icosphere(1)
    assert v.shape == (42, 3) and f.shape == (80, 3) and render.icosphere(3)[1].shape == (1280, 3)
    assert render.box_mesh()[1].shape == (12, 3) and render.l_prism_mesh()[1].shape == (20, 3)
    for mv, mf in (render.icosphere(2), render.box_mesh(), render.l_prism_mesh()):   # closed: every edge in exactly two faces
        edges = {}
        for a, b, c in mf:
            for e in ((a, b), (b, c), (c, a)):
                edges[tuple(sorted(e))] = edges.get(tuple(sorted(e)), 0) + 1
        assert set(edges.values()) == {2}
    m = render.DeviceMeshes([(v, f), render.box_mesh()])
    assert m.count == 2 and m.total_vertices == 50 and m.total_faces == 92
    assert list(m.vertex_offset) == [0, 42, 50] and list(m.face_offset) == [0, 80, 92] and m.faces.dtype == np.int32
    bad = f.copy()
    bad[5, 1] = 42
    with pytest.raises(ValueError):
        render.DeviceMeshes([(v, bad)])
    bad[5, 1] = -1
    with pytest.raises(ValueError):
        render.DeviceMeshes([(v, bad)])
    with pytest.raises(ValueError):   # an index valid in the table but not in its own mesh
        render.DeviceMeshes([render.box_mesh(), (v[:8], np.array([[0, 1, 9]]))])
    with pytest.raises(ValueError):
        render.DeviceMeshes([])
