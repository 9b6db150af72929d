"""Regenerates tests/golden/depth.npz: what the REFERENCE's own ``OcclusionLineModDB.get_mask_of_all_objects``
(lib/utils/data_utils.py:788-826) returns for one scene of low-polygon meshes whose depth images come from
tests/depth_restatement.py.

    python tests/golden/make_depth_golden.py <root of a zju3dv/pvnet checkout>

CPU only.  The reference's module is imported unchanged (tools/refshim.py serves the third-party packages it names).  An
``OcclusionLineModDB`` is made with ``object.__new__`` and given the three things its method reads: ``class_type_to_number`` (the
instance list: dict order is composition order), a ``read_blender_pose`` that returns the scene's pose of the current class, and an
``opengl_renderer`` whose ``render`` returns the restatement's depth image of that class (the reference's own depth images come from an
OpenGL backend; the COMPOSITION is what is recorded here).  The reference hard-codes 480 x 640.

The scene holds, in list order: two boxes that interpenetrate (checked here: neither painter's order of
tests/raster_restatement.py gives the reference's image), the same prism twice under one pose (an exact tie on every pixel; the
reference is run under both list orders and both images are recorded), a sphere that the reference's starting depth of 10 cuts
through, and a wall wholly beyond 10.

The file written holds data only: meshes made HERE, poses, K, labels, the two list orders with the reference's label image for each,
and a checksum of the depth images handed to the reference (7 MB raw: the test regenerates them and holds them to the checksum, so a
change to the restatement cannot silently move the fixture).
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "depth.npz")
H, W, FAR = 480, 640, 10.0


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose(axis, angle, t):
    return np.concatenate([rotation(axis, angle), np.asarray(t, np.float64).reshape(3, 1)], 1)


def camera(h, w):
    return np.array([[0.95 * w, 0.0, w / 2.0 + 0.37], [0.0, 0.97 * w, h / 2.0 - 0.21], [0.0, 0.0, 1.0]])


def scene():
    """-> meshes {name: (vertices, faces)}, instances [(name, mesh, pose, label)] in list order"""
    from pvnet_amd import render
    meshes = {"bar": render.box_mesh(0.5, 0.12, 0.1), "prism": render.l_prism_mesh(0.2, 0.08), "ball": render.icosphere(1, 1.5),
              "wall": render.box_mesh(4.0, 3.0, 0.2)}
    tie = pose((1, 2, 3), 0.8, (0.25, 0.12, 0.9))
    instances = [("bara", "bar", pose((0, 1, 0), 0.5, (-0.15, -0.1, 1.0)), 1),     # the left end nearer
                 ("barb", "bar", pose((0.1, 1, 0), -0.4, (-0.14, -0.09, 1.01)), 2),   # the right end nearer: they cross
                 ("tie1", "prism", tie, 3),
                 ("tie2", "prism", tie.copy(), 4),
                 ("ball", "ball", pose((1, 0, 1), 0.3, (-3.5, 2.4, 10.2)), 5),      # cut by the depth of 10
                 ("wall", "wall", pose((0, 0, 1), 0.1, (2.5, -1.5, 12.0)), 6)]      # wholly beyond 10
    return meshes, instances


def main(reference_root):
    import refshim
    refshim.install(reference_root)
    refshim.pin_overlay(reference_root)
    cwd = os.getcwd()
    os.chdir(reference_root)   # lib/utils/config.py opens its files relatively
    try:
        data_utils = importlib.import_module("lib.utils.data_utils")
    finally:
        os.chdir(cwd)
    assert os.path.abspath(data_utils.__file__).startswith(os.path.abspath(reference_root) + os.sep), data_utils.__file__
    from tests import depth_restatement as DR
    from tests import raster_restatement as RS

    meshes, instances = scene()
    K = camera(H, W)
    depth = {name: DR.instance_depth(*meshes[mesh], p, K, H, W) for name, mesh, p, _ in instances}
    assert all(status == 0 for _, status in depth.values())
    depth = {name: d for name, (d, _) in depth.items()}
    # what the fixture must contain
    assert (depth["wall"] != 0).any() and depth["wall"][depth["wall"] != 0].min() > FAR                      # wholly beyond 10
    ball = depth["ball"][depth["ball"] != 0]
    assert (ball < FAR).any() and (ball > FAR).any()                                                          # cut by 10
    assert np.array_equal(depth["tie1"], depth["tie2"]) and (depth["tie1"] != 0).sum() > 1000               # an exact tie

    class Renderer:
        def render(self, class_type, pose, camera_type=None):
            assert camera_type == "linemod" and np.array_equal(pose, poses[class_type])
            return depth[class_type].copy()

    poses = {name: p for name, _, p, _ in instances}
    labels = {name: lab for name, _, _, lab in instances}

    def reference(order):
        db = object.__new__(data_utils.OcclusionLineModDB)
        db.class_type_to_number = {instances[i][0]: str(labels[instances[i][0]]) for i in order}   # the reference's values are strings
        db.read_blender_pose = lambda index: poses[db.class_type]
        db.opengl_renderer = Renderer()
        out = db.get_mask_of_all_objects(0)
        assert out.dtype == np.uint8 and out.shape == (H, W)
        return out

    orders = np.array([[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]])   # the second: every pair the other way round, the tie too
    recorded = np.stack([reference(list(o)) for o in orders])
    assert set(np.unique(recorded[0])) == {0, 1, 2, 3, 5} and set(np.unique(recorded[1])) == {0, 1, 2, 4, 5}
    assert np.array_equal(recorded[0] == 3, recorded[1] == 4)
    assert np.array_equal(np.where(recorded[0] == 3, 4, recorded[0]), recorded[1])   # nothing else depends on the order
    # the restatement's own composition agrees (the CPU test asserts this from the file)
    for o, ref in zip(orders, recorded):
        inst = [(0, None, None, 0, labels[instances[i][0]]) for i in o]
        _, lab, _ = DR.compose([depth[instances[i][0]] for i in o], [0] * 6, [x[4] for x in inst], 1, FAR)
        print("order", list(o), "restatement equals the reference:", np.array_equal(lab[0], ref))
    # the two bars: no painter's order gives the reference's image
    bars = [(0, instances[0][2], K, 0, 1), (0, instances[1][2], K, 0, 2)]
    only_bars = np.where(recorded[0] <= 2, recorded[0], 0)
    for order in ([0, 1], [1, 0]):
        painted, _, _ = RS.render([meshes["bar"]], bars, 1, H, W, order=order)
        hidden = (recorded[0] > 2)   # pixels another object of the scene took
        differ = int(((painted[0] != only_bars) & ~hidden).sum())
        print("painter's order", order, "differs from the reference in", differ, "pixels")
        assert differ > 100

    arrays = {"size": np.array([H, W]), "far": np.float32(FAR), "K": K, "orders": orders, "labels_ref": recorded,
              "instances": np.array([name for name, _, _, _ in instances]), "instance_mesh": np.array([m for _, m, _, _ in instances]),
              "instance_label": np.array([lab for _, _, _, lab in instances], np.int32),
              "poses": np.stack([p for _, _, p, _ in instances]),
              "depth_sha256": np.array(DR.checksum([depth[name] for name, _, _, _ in instances]))}
    for name, (v, f) in meshes.items():
        arrays[f"mesh.{name}.vertices"], arrays[f"mesh.{name}.faces"] = v, f
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
