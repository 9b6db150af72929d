"""CPU-only checks of the augmentation on the device (include/pvnet_augment.h, libpvnet_augment.so): the header's exports against the
prototype table of pvnet_amd/_abi.py, the built library, every bad argument rejected with the documented code before any HIP call,
the register rule for the new kernels, the configuration's defaults against the reference's JSON, and the float64 restatement
(tests/augment_restatement.py) against what the reference's own ``augmentation`` returned (tests/golden/augment.npz), bit for bit.
What holds for every side library alike (header against table, the built library's symbols, the register tool's selection, the loud
failure without it) is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from pvnet_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_augment.h")).read()
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
EXPORTS = {"pvnet_augment_abi_version", "pvnet_augment_workspace_bytes", "pvnet_augment", "pvnet_normalize"}
KERNELS = ("augment_plan_kernel", "augment_warp_kernel")
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment.npz")
CFG_JSON = os.path.join(ROOT, "tests", "golden", "default_linemod_cfg.json")
IMPLEMENTED = ("mask", "min_mask", "max_mask", "rotation", "rot_ang_min", "rot_ang_max", "crop", "overlap_ratio", "resize_hmin",
               "resize_hmax", "resize_wmin", "resize_wmax", "flip", "use_mask_out")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_augment_library()


def test_header_declares_the_exports_and_every_one_has_a_prototype():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS
    decl = re.search(r"^int pvnet_augment\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.AUGMENT_PROTOTYPES["pvnet_augment"][1]
    assert "size_t workspace_bytes" in decl[-2] and args[-2] is C.c_size_t
    assert "uint64_t seed" in decl[14] and args[14] is C.c_uint64
    # every constant of the header is mirrored by value
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_AUGMENT_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.AUGMENT_ABI_VERSION == 1
    assert len(consts) == 13
    for name, value in consts.items():
        assert getattr(_abi, "AUGMENT_" + name) == value, name
    # the configuration struct: the same fields in the same order
    body = re.search(r"typedef struct PvnetAugmentConfig \{(.*?)\} PvnetAugmentConfig;", HDR, re.S).group(1)
    fields = [f.strip().split("[")[0] for line in re.sub(r"/\*.*?\*/", "", body).split(";") if line.strip()
              for f in line.strip().split(None, 1)[1].split(",")]
    assert fields == [n for n, _ in _abi.AugmentConfigStruct._fields_]
    assert C.sizeof(_abi.AugmentConfigStruct) == 8 + 7 * 8 + 6 * 4


def test_library_is_built_for_gfx950_and_exports_the_symbols(lib):
    blob = open(_abi.AUGMENT_LIB_PATH, "rb").read()
    assert all(k.encode() in blob for k in KERNELS)
    assert build.SIDE_LIBRARIES["augment"][:2] == (["augment.hip"], "pvnet_augment.h")
    # the other libraries' shapes have not moved
    assert [build.SIDE_LIBRARIES[n][0] for n in ("head", "train", "targets")] == [["head_metrics.hip"], ["head_grad.hip"], ["head_targets.hip"]]
    assert lib.pvnet_augment_workspace_bytes(0) == 0 and lib.pvnet_augment_workspace_bytes(65536) == 0
    assert lib.pvnet_augment_workspace_bytes(-1) == 0
    assert 0 < lib.pvnet_augment_workspace_bytes(1) and lib.pvnet_augment_workspace_bytes(32) == 32 * lib.pvnet_augment_workspace_bytes(1)


def test_bad_arguments_are_rejected_without_a_device(lib):
    from pvnet_amd.augment import AugmentConfig
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    s3 = (C.c_int64 * 3)(1, 1, 1)
    good = AugmentConfig().struct()
    U8, I16, I32, I64, F32 = 0, 1, 2, 3, 4

    def cfg(**kw):
        s = AugmentConfig().struct()
        for k, v in kw.items():
            if k in ("mean", "std"):
                getattr(s, k)[:] = v
            else:
                setattr(s, k, v)
        return s

    def aug(rgb=p, rs=s3, mask=p, mdt=U8, ms=s3, hc=p, un=p, b=4, h=48, w=64, vn=9, height=32, width=40, c=good, seed=1, image=p, idt=0,
            mo=p, modt=U8, hco=p, status=p, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_augment_workspace_bytes(max(b, 1))
        return lib.pvnet_augment(rgb, rs, mask, mdt, ms, hc, un, b, h, w, vn, height, width, None if c is None else C.byref(c), seed, image,
                                 idt, mo, modt, hco, status, ws, wsb, None)

    for name in ("rgb", "rs", "mask", "ms", "hc", "un", "c", "image", "mo", "hco", "status"):
        assert aug(**{name: None}) == BADARG, name
    assert aug(b=-1) == BADARG and aug(h=0) == BADARG and aug(w=0) == BADARG and aug(vn=0) == BADARG
    assert aug(height=0) == BADARG and aug(width=-3) == BADARG
    assert aug(idt=3) == BADARG and aug(idt=-1) == BADARG
    assert aug(mdt=99) == BADARG and aug(mdt=-1) == BADARG and aug(mdt=I16) == UNSUPPORTED and aug(mdt=F32) == UNSUPPORTED
    assert aug(modt=I32) == BADARG and aug(modt=F32) == BADARG
    assert aug(c=cfg(flags=32)) == BADARG and aug(c=cfg(reserved=1)) == BADARG
    assert aug(c=cfg(std=(0.2, 0.0, 0.2))) == BADARG and aug(c=cfg(mean=(float("nan"), 0.0, 0.0))) == BADARG
    assert aug(c=cfg(min_mask=-0.1)) == BADARG and aug(c=cfg(min_mask=0.5, max_mask=0.4)) == BADARG
    assert aug(c=cfg(overlap_ratio=1.5)) == BADARG and aug(c=cfg(overlap_ratio=float("nan"))) == BADARG
    assert aug(c=cfg(resize_hmin=0.0)) == BADARG and aug(c=cfg(resize_wmin=140.0)) == BADARG
    assert aug(c=cfg(flags=_abi.AUGMENT_F_FLIP)) == BADARG           # without the crop the output is the source's size
    assert aug(c=cfg(flags=_abi.AUGMENT_F_FLIP), height=48, width=64, b=0) == 0
    assert aug(b=65536) == UNSUPPORTED and aug(h=32769) == UNSUPPORTED and aug(h=32768, w=32768, b=0) == 0
    assert aug(h=32768, w=32768 + 1) == UNSUPPORTED and aug(height=40000) == UNSUPPORTED
    assert aug(ws=None) == WORKSPACE and aug(wsb=lib.pvnet_augment_workspace_bytes(4) - 1) == WORKSPACE
    assert aug(ws=C.c_void_p(0x2004)) == BADARG                     # misaligned workspace
    for mdt in (U8, I32, I64):
        for modt in (U8, I64):
            for idt in (0, 1, 2):
                assert aug(mdt=mdt, modt=modt, idt=idt, b=0, ws=None, wsb=0) == 0   # nothing to do, nothing enqueued

    def norm(rgb=p, rs=s3, b=4, h=48, w=64, c=good, image=p, idt=0):
        return lib.pvnet_normalize(rgb, rs, b, h, w, None if c is None else C.byref(c), image, idt, None)

    for name in ("rgb", "rs", "c", "image"):
        assert norm(**{name: None}) == BADARG, name
    assert norm(b=-1) == BADARG and norm(h=0) == BADARG and norm(idt=7) == BADARG and norm(c=cfg(std=(1.0, 1.0, -1.0))) == BADARG
    assert norm(b=65536) == UNSUPPORTED and norm(w=40000) == UNSUPPORTED
    assert norm(b=0) == 0 and norm(b=0, idt=1) == 0 and norm(b=0, idt=2) == 0


def test_register_check_covers_the_new_translation_unit(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as chk
    (src, text), = chk.side_assembly("augment")
    assert src.endswith("augment.hip")
    ks = chk.kernels(text)
    assert len(ks) == 7 and all(any(k in name for name, _, _, _ in ks) for k in KERNELS)   # the plan, 3 element types x 2 store paths
    assert not any("head_" in chk.short(name) or "vertex_targets" in chk.short(name) for name, _, _, _ in ks)
    for name, nfv, vmax, scratch in ks:
        assert nfv - (vmax + 1) >= chk.SLACK and scratch == 0, name
    # the vector path stores 16 bytes at a time
    assert "global_store_dwordx4" in text


def test_config_defaults_are_the_references():
    from pvnet_amd.augment import AugmentConfig
    ref = json.load(open(CFG_JSON))
    cfg = AugmentConfig()
    for key in IMPLEMENTED:
        assert getattr(cfg, key) == ref[key] and type(getattr(cfg, key)) is type(ref[key]) or \
            (not isinstance(ref[key], bool) and float(getattr(cfg, key)) == float(ref[key])), key
    assert ref["use_old"] is False and cfg.use_old is False
    for key in ("use_old", "blur", "jitter"):
        with pytest.raises(NotImplementedError):
            AugmentConfig(**{key: True})
    with pytest.raises(NotImplementedError):      # the reference's file asks for blur and jitter
        AugmentConfig.from_reference(ref)
    got = AugmentConfig.from_reference(ref, blur=False, jitter=False)
    assert got == cfg
    s = cfg.struct()
    assert s.flags == _abi.AUGMENT_F_MASK | _abi.AUGMENT_F_ROTATION | _abi.AUGMENT_F_CROP | _abi.AUGMENT_F_FLIP and s.reserved == 0
    assert (s.min_mask, s.max_mask, s.overlap_ratio) == (0.1, 0.4, 0.5)
    assert (s.resize_hmin, s.resize_hmax, s.resize_wmin, s.resize_wmax) == (20.0, 130.0, 20.0, 130.0)
    assert list(s.mean) == [np.float32(v) for v in (0.485, 0.456, 0.406)] and list(s.std) == [np.float32(v) for v in (0.229, 0.224, 0.225)]
    assert AugmentConfig.identity().flags() == 0
    from tests.augment_restatement import DEFAULTS
    assert DEFAULTS == {k: ref[k] for k in IMPLEMENTED}


def test_python_entries_refuse_host_tensors_and_bad_uniforms():
    import torch
    from pvnet_amd import augment as A
    rgb = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.augment_batch(rgb, torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 2, 3), dtype=torch.float64), 8, 8, A.AugmentConfig(),
                        A.draw_uniforms(1), 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.normalize_batch(rgb)
    g = torch.Generator().manual_seed(5)
    u = A.draw_uniforms(3, g)
    assert u.shape == (3, 12) and u.dtype == torch.float64 and bool(((u >= 0) & (u < 1)).all())
    assert torch.equal(u, A.draw_uniforms(3, torch.Generator().manual_seed(5)))
    packed = A.pack_uniforms(u, A.AugmentConfig(), "cpu")
    assert packed.shape == (3, 14) and torch.equal(packed[:, :12], u)
    from tests.augment_restatement import DEFAULTS, trig
    for i in range(3):
        assert tuple(packed[i, 12:].tolist()) == trig(float(u[i, 5]), DEFAULTS)
    with pytest.raises(RuntimeError):
        A.pack_uniforms(torch.ones((1, 12), dtype=torch.float64), A.AugmentConfig(), "cpu")
    with pytest.raises(RuntimeError):
        A.pack_uniforms(u.float(), A.AugmentConfig(), "cpu")


def test_restatement_equals_the_reference_bit_for_bit():
    """tests/augment_restatement.py against what the reference's own augmentation returned for the fixture's inputs: the float64
    key-points ``==`` in every case; the image and the mask ``==`` in the cases without rotation and resize, where the reference is
    pure numpy (flip, crop, pad, mask-out)."""
    from tests import augment_restatement as RS
    g = np.load(GOLDEN)
    names = [str(n) for n in g["cases"]]
    assert os.path.getsize(GOLDEN) < 200 * 1024 and len(names) >= 10
    seen = dict(rotated=False, resized=False, padded=False, pad_after_resize=False, flipped=False, unflipped=False, masked=False,
                negative_start=False, empty=False, images=0, odd=False, moved=False)
    for n in names:
        rgb, mask, hc, u = g[n + ".rgb"], g[n + ".mask"], g[n + ".hcoords"], g[n + ".uniforms"]
        assert rgb.shape == (48, 64, 3) and rgb.dtype == np.uint8 and hc.dtype == np.float64
        height, width = (int(v) for v in g[n + ".size"])
        cfg = json.loads(str(g[n + ".cfg"]))
        image, m, out, status, plan = RS.augment_one(rgb, mask, hc, height, width, cfg, u, int(g[n + ".seed"]))
        ref = g[n + ".ref_hcoords"]
        assert ref.dtype == np.float64 and np.array_equal(out, ref), n
        assert status & ~RS.S_NO_FOREGROUND == 0, n                  # the reference ran: none of the definition's extensions
        if n + ".ref_image" in g:
            assert not plan["rotated"] and not plan["resized"]
            want = (g[n + ".ref_image"].astype(np.float32) / np.float32(255.0) - RS.MEAN) / RS.STD
            assert np.array_equal(image, want.transpose(2, 0, 1)), n
            assert np.array_equal(m, g[n + ".ref_mask"].astype(np.int64)), n
            seen["images"] += 1
        seen["rotated"] |= plan["rotated"]
        seen["resized"] |= plan["resized"]
        seen["padded"] |= plan["hoff"] > 0 and plan["woff"] > 0
        seen["pad_after_resize"] |= plan["resized"] and plan["hoff"] > 0
        seen["flipped"] |= plan["flip"]
        seen["unflipped"] |= not plan["flip"]
        seen["moved"] |= plan["hbeg"] > 0 and plan["wbeg"] > 0
        seen["empty"] |= bool(status & RS.S_NO_FOREGROUND)
        seen["odd"] |= width % 8 != 0
        gate = (RS.DEFAULTS | cfg)["mask"] and u[0] < 0.5 and mask.any()
        seen["masked"] |= bool(gate and n + ".ref_image" in g and (g[n + ".ref_mask"].sum() < mask.sum()))
        seen["negative_start"] |= n == "negative_start" and bool(gate) and int(g[n + ".ref_mask"].sum()) == int(m.sum()) > 0
    assert all(seen.values()) and seen["images"] >= 5, seen
    # the negative start: the gate was open and nothing was masked out (the rectangle is empty, as the reference's slice is)
    n = "negative_start"
    _, m, _, _, plan = RS.augment_one(g[n + ".rgb"], g[n + ".mask"], g[n + ".hcoords"], 48, 64, dict(rotation=False, crop=False, flip=False),
                                      g[n + ".uniforms"], 1)
    assert np.array_equal(m, g[n + ".mask"].astype(np.int64))


def test_restatement_extensions():
    """what the definition adds where the reference raises: hi <= lo, a mask that mask-out empties, a bbox without extent"""
    from tests import augment_restatement as RS
    rgb = np.full((48, 64, 3), 200, np.uint8)
    hc = np.array([[10.0, 12.0, 1.0]])
    u = np.full(12, 0.9)
    one = np.zeros((48, 64), np.uint8)
    one[20, 30] = 1                                       # a single pixel: bbox without extent
    u1 = u.copy()
    u1[6] = 0.1
    _, m, out, status, plan = RS.augment_one(rgb, one, hc, 32, 40, {}, u1, 3)
    assert status & RS.S_DEGENERATE and not plan["resized"] and m.sum() == 1
    u2 = u.copy()
    u2[0] = 0.1
    _, _, _, status, _ = RS.augment_one(rgb, one, hc, 32, 40, {}, u2, 3)
    assert status & RS.S_RANGE                             # randint(xmin, xmax) with xmax == xmin
    small = np.zeros((48, 64), np.uint8)
    small[20:23, 30:33] = 1                                # 3 x 3: with sides of 1 the rectangle can cover all that the bbox start leaves
    cfgm = dict(min_mask=1.0, max_mask=1.0, rotation=False)
    u3 = u.copy()
    u3[0], u3[3], u3[4] = 0.1, 0.6, 0.6
    img, m, out, status, plan = RS.augment_one(rgb, small, hc, 32, 40, cfgm, u3, 3)
    assert plan["inst"] and m.sum() > 0 and m.sum() < 9    # partly masked out
    u4 = u.copy()
    u4[0], u4[3], u4[4] = 0.1, 0.99, 0.99                  # sides floor(2 * 2 / 2) = 2 about (31, 21): columns 29 .. 32, rows 19 .. 22
    _, m, out, status, plan = RS.augment_one(rgb, small, hc, 32, 40, dict(min_mask=2.0, max_mask=2.0), u4, 3)
    assert status & RS.S_EMPTIED and not plan["inst"] and not plan["rotated"] and m.sum() == 0
    assert np.array_equal(out, hc)                         # the no-foreground path leaves the key-points alone
