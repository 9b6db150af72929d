"""CPU-only checks of the z-buffered mesh renderer (include/pvnet_depth.h, libpvnet_depth.so, pvnet_amd/depth.py): the registry row,
the header's constants against pvnet_amd/_abi.py, every bad argument rejected before any HIP call, the kernels' assembly (one 64-bit
atomic minimum, nothing contracted, the register rule), the numpy restatement (tests/depth_restatement.py) against the silhouette
restatement, against an independent ray-plane oracle and against what the reference's own ``get_mask_of_all_objects`` recorded
(tests/golden/depth.npz).
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build, render
from tests import depth_restatement as DR
from tests import raster_restatement as RS
from tests.render_cases import BADARG, camera, i32, refuses_the_pvnet_render_list, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_depth.h")).read()
EXPORTS = {"pvnet_depth_abi_version", "pvnet_depth_workspace_bytes", "pvnet_render_depth"}
H, W = 48, 64


@pytest.fixture(scope="module")
def lib():
    build.build_side("depth")
    return _abi.load_depth_library()


def test_registry_row():
    assert build.SIDE_LIBRARIES["depth"][:2] == (["depth.hip"], "pvnet_depth.h")
    shared, zbuffer = os.path.join(build.CSRC, "mesh_core.h"), os.path.join(build.CSRC, "zbuffer_core.h")
    assert build.SIDE_LIBRARIES["depth"][2] == [zbuffer] and build.SIDE_LIBRARIES["raster"][2] == [shared]
    # the projection and the coverage predicate rebuild the silhouette library and the three that render through the z-buffer
    assert {n for n in build.SIDE_LIBRARIES if shared in build._side(n)[1]} == {"raster", "depth", "shade", "texture"}
    assert {n for n in build.SIDE_LIBRARIES if zbuffer in build._side(n)[1]} == {"depth", "shade", "texture"}
    assert _abi.SIDE_LIBRARIES["depth"] == (_abi.DEPTH_LIB_PATH, _abi.DEPTH_ABI_VERSION, _abi.DEPTH_PROTOTYPES)
    assert _abi.load_depth_library.args == ("depth",)


def test_abi_version_and_constants_are_mirrored():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS == set(_abi.DEPTH_PROTOTYPES)
    decl = re.search(r"^int pvnet_render_depth\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.DEPTH_PROTOTYPES["pvnet_render_depth"][1]
    assert len(decl) == len(args) == 25
    for k, (word, typ) in {2: ("vertex_offset", _abi._i32p), 8: ("mesh_id", _abi._i32p), 12: ("image_id", _abi._i32p), 13: ("label", _abi._i32p),
                           17: ("float far", C.c_float), 18: ("depth_out", C.c_void_p), 19: ("label_out", C.c_void_p),
                           20: ("visible_out", C.c_void_p), 21: ("status_out", C.c_void_p), 23: ("ws_bytes", C.c_size_t),
                           24: ("stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_DEPTH_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.DEPTH_ABI_VERSION == 1
    consts.pop("WS_COOP_COUNT_OFFSET")
    assert len(consts) == 8
    for name, value in consts.items():
        assert getattr(_abi, "DEPTH_" + name) == value, name
        assert getattr(_abi, "RASTER_" + name) == value, name   # the limits and bits of pvnet_render under this header's names
    assert (DR.S_NONFINITE, DR.S_BEHIND, DR.S_BADFACE) == (_abi.DEPTH_S_NONFINITE, _abi.DEPTH_S_BEHIND, _abi.DEPTH_S_BADFACE)


def test_library_is_built_with_its_exports_and_leaves_the_raster_library_alone(lib):
    assert lib.pvnet_depth_abi_version() == 1
    blob = open(_abi.DEPTH_LIB_PATH, "rb").read()
    for kernel in (b"depth_setup_kernel", b"depth_clear_kernel", b"depth_tri_kernel", b"depth_resolve_kernel"):
        assert kernel in blob
    assert b"triangle_kernel" not in blob and b"expand_kernel" not in blob
    raw = C.CDLL(_abi.DEPTH_LIB_PATH)
    assert not hasattr(raw, "pvnet_render") and not hasattr(raw, "pvnet_vote_v3")


def test_workspace_bytes_is_monotone_and_rejects_bad_sizes(lib):
    f = lib.pvnet_depth_workspace_bytes
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
    ws_n = lib.pvnet_depth_workspace_bytes(3, 20, 32, 2, 20, 24)

    def call(vertices=p, faces=p, voff=voff, foff=foff, M=2, P=20, T=32, q=3, mesh=i32(0, 1, 1), poses=p, K=p, kper=0,
             image=i32(0, 0, 1), label=i32(1, 2, 3), b=2, h=20, w=24, far=float("inf"), depth=p, labels=p, visible=None, status=None,
             ws=p, nbytes=ws_n):
        return lib.pvnet_render_depth(vertices, faces, voff, foff, M, P, T, q, mesh, poses, K, kper, image, label, b, h, w, far, depth,
                                      labels, visible, status, ws, nbytes, None)

    for far in (0.0, -0.0, -1.0, float("-inf"), float("nan")):
        assert call(far=far) == BADARG, far
    assert call(depth=None, labels=None) == BADARG                 # no image output
    assert call(depth=None, labels=None, visible=p, status=p) == BADARG
    refuses_the_pvnet_render_list(call, ws_n, _abi.DEPTH_MAX_MESHES, _abi.DEPTH_MAX_INSTANCES, _abi.DEPTH_MAX_SIDE, _abi.DEPTH_MAX_IMAGES)


def test_assembly_one_atomic_minimum_nothing_contracted_and_the_register_rule():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--depth"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "checked 4 kernels, 0 without" in r.stdout
    assert all("scratch   0 B" in line for line in r.stdout.splitlines() if " allocates " in line)   # no spills
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as CK
    (_, asm), = CK.side_assembly("depth")
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())
    # the 64-bit unsigned minimum is one global atomic, not a compare-and-swap loop
    assert len(re.findall(r"\bglobal_atomic_umin_x2\b", code)) == 2 and "cmpswap" not in code
    # the predicate has no division: any fused float32 multiply-add would be a contraction
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)(mk|ak)?_f32\b", code)
    # float64: the only fused operations are those of the divisions' own expansion (five per division with this compiler: the
    # projection's six, 1/z three, b and c, and 1/inv on each of the two paths)
    divisions = len(re.findall(r"\bv_div_fixup_f64\b", code))
    assert divisions == 13 and len(re.findall(r"\bv_(fma|fmac)_f64(_e32|_e64)?\b", code)) == 5 * divisions
    assert "v_mul_f64" in code and "v_add_f64" in code and "v_mul_f32" in code
    modes = re.findall(r"\.amdhsa_float_denorm_mode_32 (\d)", asm) + re.findall(r"\.amdhsa_float_denorm_mode_16_64 (\d)", asm)
    assert len(modes) == 8 and set(modes) == {"3"}   # denormals kept in every kernel
    for banned in ("printf", "__assert_fail"):
        assert banned not in asm


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
MESHES = {"box": render.box_mesh(0.15, 0.1, 0.2), "lprism": render.l_prism_mesh(0.2, 0.08), "ico1": render.icosphere(1, 0.1),
          "ico2": render.icosphere(2, 0.1)}


def oracle_depth(vertices, faces, pose, K, h, w):
    """independent of the definition's formula: the ray through the pixel, K^-1 (px, py, 1), against the triangle's plane in camera
    space, in float64; the same coverage and clamp; the minimum over triangles.  -> float64 [h,w], +inf where nothing covers"""
    u, v, z = RS.project_points(vertices, pose, K)
    cam = np.asarray(vertices, np.float64) @ pose[:, :3].T + pose[:, 3]
    Kinv = np.linalg.inv(K)
    out = np.full((h, w), np.inf)
    for face in np.asarray(faces, np.int64):
        t = np.stack([u[face], v[face]], -1).astype(np.float32)
        box = DR.triangle_box(t, h, w)
        if box is None:
            continue
        begx, endx, begy, endy = box
        ys, xs = np.mgrid[begy:endy + 1, begx:endx + 1]
        ok = DR.triangle_coverage(t, xs.astype(np.float32), ys.astype(np.float32))
        c0, c1, c2 = cam[face]
        n = np.cross(c1 - c0, c2 - c0)
        rays = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64) @ Kinv.T
        with np.errstate(all="ignore"):
            d = (n @ c0) / (rays @ n) * rays[..., 2]
        zmin, zmax = z[face].min(), z[face].max()
        d = np.where(d >= zmin, d, zmin)
        d = np.where(d > zmax, zmax, d)
        view = out[begy:endy + 1, begx:endx + 1]
        np.minimum(view, np.where(ok, d, np.inf), out=view)
    return out


@pytest.fixture(scope="module")
def cases():
    """[(mesh name, pose, restated depth, restated status)]: six random poses per mesh at z in 0.4 .. 0.8, computed once"""
    rng = np.random.default_rng(20261019)
    K = camera(H, W)
    out = []
    for name, (v, f) in MESHES.items():
        for _ in range(6):
            t = (rng.uniform(-0.12, 0.12), rng.uniform(-0.09, 0.09), rng.uniform(0.4, 0.8))
            pose = np.concatenate([rotation(rng.normal(size=3), rng.uniform(0, np.pi)), np.asarray(t).reshape(3, 1)], 1)
            depth, status = DR.instance_depth(v, f, pose, K, H, W)
            out.append((name, pose, depth, status))
    return K, out


def test_restated_depth_covers_the_silhouette_and_stays_within_the_mesh(cases):
    K, out = cases
    covered = 0
    for name, pose, depth, status in out:
        v, f = MESHES[name]
        tri, st = RS.project_triangles(v, f, pose, K)
        mask, st2 = RS.rasterize(tri, H, W)
        assert status == 0 and st == 0 and st2 == 0
        assert depth.dtype == np.float32 and np.array_equal(depth != 0, mask != 0), name
        z = RS.project_points(v, pose, K)[2]
        inside = depth[depth != 0]
        assert inside.size and inside.min() >= np.float32(z.min()) and inside.max() <= np.float32(z.max()), name
        covered += inside.size
    assert covered > 5000


def test_a_face_parallel_to_the_image_plane_has_exactly_its_depth():
    v, f = render.box_mesh(0.15, 0.1, 0.2)
    K = camera(H, W)
    sides = 0
    for angle, t in ((0.0, (0.0, 0.0, 0.5)), (0.4, (0.03, -0.02, 0.7)), (1.1, (-0.05, 0.04, 0.45))):
        pose = np.concatenate([rotation((0, 0, 1), angle), np.asarray(t, np.float64).reshape(3, 1)], 1)
        depth, status = DR.instance_depth(v, f, pose, K, H, W)
        z = RS.project_points(v, pose, K)[2]
        front = [face for face in f if np.all(z[face] == z.min())]
        assert status == 0 and len(front) == 2
        tri, _ = RS.project_triangles(v, np.asarray(front), pose, K)
        mask, _ = RS.rasterize(tri, H, W)
        assert mask.sum() > 100 and (depth[mask != 0] == np.float32(z.min())).all()
        assert (depth[depth != 0] >= np.float32(z.min())).all()
        sides += int((depth[depth != 0] > np.float32(z.min())).sum())
    assert sides > 0   # off the axis the side faces are seen too, and lie deeper


def test_restated_depth_against_the_ray_plane_oracle(cases):
    """MEASURED with this seed (24 poses, 48 x 64): identical coverage; the largest absolute difference to the float64 ray-plane oracle
    is 7.6e-7 over 10 075 covered pixels (box 7.6e-7, lprism 5.6e-7, ico1 1.9e-7, ico2 4.1e-7).  That is the float32 rounding of u and
    v: half a float32 ulp of a coordinate near 32 is 1.9e-6 pixels, and a face seen nearly edge-on (the box's and the prism's sides)
    changes its depth by tenths of a metre per pixel; the rounding of the result itself is 3.0e-8 at 0.8.  The bar is four times the
    measured value, the margin being for other seeds, and no pixel is excluded.  profiles/depth_probe.txt records the same."""
    K, out = cases
    worst, pixels = {}, 0
    for name, pose, depth, _ in out:
        v, f = MESHES[name]
        want = oracle_depth(v, f, pose, K, H, W)
        assert np.array_equal(np.isfinite(want), depth != 0), name
        on = depth != 0
        worst[name] = max(worst.get(name, 0.0), float(np.abs(depth[on].astype(np.float64) - want[on]).max()))
        pixels += int(on.sum())
    print("ray-plane oracle: largest absolute difference per mesh", {k: f"{x:.3e}" for k, x in worst.items()}, "over", pixels, "pixels")
    assert max(worst.values()) <= ORACLE_BAR, worst


ORACLE_BAR = 4 * 7.6e-7   # four times the measured largest difference


def test_composition_equals_the_reference_at_far_10():
    G = np.load(os.path.join(ROOT, "tests", "golden", "depth.npz"))
    h, w = (int(x) for x in G["size"])
    far = float(G["far"])
    assert (h, w, far) == (480, 640, 10.0)
    names = [str(n) for n in G["instances"]]
    meshes = [(G[f"mesh.{m}.vertices"], G[f"mesh.{m}.faces"]) for m in G["instance_mesh"]]
    depths = []
    for k in range(len(names)):
        d, status = DR.instance_depth(*meshes[k], G["poses"][k], G["K"], h, w)
        assert status == 0
        depths.append(d)
    assert DR.checksum(depths) == str(G["depth_sha256"])   # the depth images the reference was handed
    by = dict(zip(names, depths))
    # what the fixture contains: depths beyond 10 (a wall wholly, a ball in part) and an exact tie
    assert by["wall"][by["wall"] != 0].min() > far and (by["ball"] > far).any() and ((by["ball"] != 0) & (by["ball"] < far)).any()
    assert np.array_equal(by["tie1"], by["tie2"]) and (by["tie1"] != 0).sum() > 1000
    labels = [int(x) for x in G["instance_label"]]
    seen = []
    for order, ref in zip(G["orders"], G["labels_ref"]):
        depth, lab, visible = DR.compose([depths[i] for i in order], [0] * len(order), [labels[i] for i in order], 1, far)
        assert np.array_equal(lab[0], ref)
        assert (depth[0][lab[0] == 0] == 0).all() and (depth[0][lab[0] != 0] < far).all() and (depth[0][lab[0] != 0] > 0).all()
        assert visible.sum() == (ref != 0).sum()
        for pos, i in enumerate(order):
            assert visible[pos] == (ref == labels[i]).sum()
        assert visible[list(order).index(names.index("wall"))] == 0
        seen.append(set(np.unique(ref)))
    assert seen == [{0, 1, 2, 3, 5}, {0, 1, 2, 4, 5}]   # the tie goes to whichever comes first
    # the two bars interpenetrate: neither painter's order gives the reference's image where they alone are seen
    ref = G["labels_ref"][0]
    bars = [(0, G["poses"][0], G["K"], 0, 1), (0, G["poses"][1], G["K"], 0, 2)]
    for order in ([0, 1], [1, 0]):
        painted, _, _ = RS.render([meshes[0]], bars, 1, h, w, order=order)
        assert ((painted[0] != np.where(ref <= 2, ref, 0)) & (ref <= 2)).sum() > 100
