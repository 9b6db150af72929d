"""CPU-only checks of what the front ends of the four mesh renderers share (pvnet_amd/_mesh.py): the split of a batch into library
calls, the head of arguments every ``pvnet_render*`` entry point opens with against the prototypes of pvnet_amd/_abi.py, that the
shared pieces are written once, and the public signatures and refusal texts against what was recorded before the plumbing was shared
(tests/golden/mesh_front_parent.json, written by tests/golden/make_mesh_front_golden.py)."""
import ast
import glob
import importlib.util
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pvnet_amd import _abi, _mesh, render  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_front_parent.json")
FRONT_ENDS = ("render", "depth", "shade", "texture")
MODULES = FRONT_ENDS + ("_mesh",)


def source(name):
    with open(os.path.join(ROOT, "pvnet_amd", name + ".py")) as fh:
        return fh.read()


def test_image_stretches_known_answers():
    assert _mesh.image_stretches(5, 3, 7) == [(0, 2), (2, 4), (4, 5)]
    assert _mesh.image_stretches(3, 0, 768) == [(0, 3)]
    assert _mesh.image_stretches(0, 2, 768) == []
    assert _mesh.image_stretches(4, 3, 3) == [(0, 1), (1, 2), (2, 3), (3, 4)]   # one image per stretch


def test_the_argument_head_fits_the_four_prototypes():
    b, m, h, w, far = 2, 3, 20, 24, 7.5
    meshes = render.DeviceMeshes([render.box_mesh(), render.icosphere(0)])
    mesh_ids, labels = [0, 1, 1], [1, 2, 255]
    poses = torch.arange(b * m * 12, dtype=torch.float64).view(b, m, 3, 4)
    K, per = _mesh.check_camera(np.arange(b * m * 9, dtype=np.float64).reshape(b, m, 3, 3), poses.device, (b, m))
    assert per and tuple(K.shape) == (b * m, 3, 3)
    heads = list(_mesh.stretch_heads(meshes, mesh_ids, labels, poses, K, per, h, w, far, limit=m))   # split at one image per call
    assert [(i0, s, nb) for i0, s, nb, _ in heads] == [(0, 0, 1), (1, m, 1)]
    z_buffer = (_abi.DEPTH_PROTOTYPES["pvnet_render_depth"], _abi.SHADE_PROTOTYPES["pvnet_render_color"],
                _abi.TEXTURE_PROTOTYPES["pvnet_render_textured"])
    for _, _, _, head in heads:
        assert len(head) == 18 and head[17] == far and head[14:17] == (1, h, w)
        for _, argtypes in z_buffer:
            for value, argtype in zip(head, argtypes[:18]):
                argtype.from_param(value)
        for value, argtype in zip(head[:14], _abi.RASTER_PROTOTYPES["pvnet_render"][1][:14]):
            argtype.from_param(value)
        vertices, faces, _ = meshes.on(poses.device)
        assert (head[0].value, head[1].value) == (vertices.data_ptr(), faces.data_ptr())
        assert (list(head[2]), list(head[3])) == ([0, 8, 20], [0, 12, 32]) and head[4:8] == (2, 20, 32, m) and head[11] == 1
    second = heads[1][3]   # the second stretch is the second image: its poses and K, image ids from 0 on
    assert (list(second[8]), list(second[12]), list(second[13])) == (mesh_ids, [0, 0, 0], labels)
    assert second[9].value == poses[1].data_ptr() and second[10].value == K[m:].data_ptr()
    # pvnet_render's head is the first fourteen, from the same builder; one K for all: no stride
    head = _mesh.argument_head(meshes, poses.device, mesh_ids * b, poses.view(-1, 3, 4), K[0], False, [0, 0, 0, 1, 1, 1], labels * b)
    assert len(head) == 14 and head[7] == b * m and head[11] == 0 and list(head[12]) == [0, 0, 0, 1, 1, 1]
    for value, argtype in zip(head, _abi.RASTER_PROTOTYPES["pvnet_render"][1][:14]):
        argtype.from_param(value)
    # no instance: arrays of one element behind n = 0, no poses
    empty = _mesh.argument_head(meshes, poses.device, [], poses.view(-1, 3, 4)[:0], K[0], False, [], [], 1, h, w, far)
    assert len(empty) == 18 and empty[7] == 0 and empty[9] is None and len(empty[8]) == 1


def test_the_shared_pieces_are_written_once():
    texts = {name: source(name) for name in MODULES}
    for what in (r"_c_voff", r"labels must lie in 1 \.\. 255", r"pvnet_[\w{}]*_workspace_bytes"):   # (the last: the library call)
        assert sum(1 for text in texts.values() if re.search(what, text)) == 1, what
    assert re.search(r"pvnet_[\w{}]*_workspace_bytes", texts["_mesh"]) and "_c_voff" in texts["render"]
    # no front end takes an underscore name from another front end: not by import, not through the module
    for name in FRONT_ENDS:
        for node in ast.walk(ast.parse(texts[name])):
            if isinstance(node, ast.ImportFrom) and node.module in FRONT_ENDS:
                assert [a.name for a in node.names if a.name.startswith("_")] == [], (name, node.module)
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in FRONT_ENDS:
                assert not node.attr.startswith("_"), (name, node.value.id, node.attr)
    # the packing of the instance table, host side: one file of csrc/
    packing = [p for p in sorted(glob.glob(os.path.join(ROOT, "pvnet_amd", "csrc", "*")))
               if re.search(r"tab(\.|->)inst\[i\] =", open(p, errors="replace").read())]
    assert [os.path.basename(p) for p in packing] == ["mesh_core.h"]


def matches(template, text):
    """whether ``text`` is ``template`` with something in the place of every ``{}``"""
    return re.fullmatch(".*".join(re.escape(part) for part in template.split("{}")), text, re.S) is not None


def test_public_signatures_and_refusal_texts_are_the_recorded_ones():
    spec = importlib.util.spec_from_file_location("make_mesh_front_golden", os.path.join(ROOT, "tests", "golden", "make_mesh_front_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = maker.signatures()
    assert len(want["signatures"]) == 24 and {k: got.get(k) for k in want["signatures"]} == want["signatures"]
    # the one public name since: the PLY parser, which texture.py takes from shade.py under a public name
    assert set(got) - set(want["signatures"]) == {"shade.parse_ply"}
    # every recorded text is still raised and nothing else is: word for word, or as an instance of a template that has a placeholder
    # where the front ends differed (the library's name in the workspace refusal, the table's class, the spelling of a dtype)
    now, then = maker.raise_texts(MODULES), want["raises"]
    assert len(then) == 50
    assert [t for t in then if not any(matches(n, t) for n in now)] == []
    assert [n for n in now if not any(matches(n, t) for t in then)] == []
    new = [n for n in now if n not in then]
    assert new == ["{}_workspace_bytes: arguments out of range ({}; h, w >= 2)"] and len([t for t in then if t not in now]) == 6
