"""CPU-only checks of the augmentation on the device (include/pvnet_augment.h, libpvnet_augment.so): the header's exports against the
prototype table of pvnet_amd/_abi.py, the built library, every bad argument rejected with the documented code before any HIP call,
the register rule for the new kernels, the configuration's defaults against the reference's JSON, and the float64 restatement
(tests/augment_restatement.py) against what the reference's own ``augmentation`` returned (tests/golden/augment.npz), bit for bit.
The warp's image and mask for rotated and resized samples are held by two oracles that do not descend from the header: the closed
form of a ramp source under the inverse of the composed forward maps (tests/augment_cases.py), and the reference's own chain over
stand-in samplers, recorded in the fixture.
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
    key-points ``==`` in every case; the mask ``==`` in every case (rotated and resized ones too: the header's mask is the chain of
    integer maps, so one pass equals the reference's two); the image ``==`` in the cases without rotation and resize, where the
    reference is pure numpy (flip, crop, pad, mask-out).  For the rotated and resized cases the recorded image is the reference's
    chain over the stand-in samplers, interpolated and rounded twice:

    * ramp pictures: ``|v - ref_image| <= 1`` in integers wherever the source point is 2 px inside the source and the canvas point
      inside the canvas.  Against the exact ramp two passes are off by at most 0.5 (the warp's rint) + 0.5 (the resize's rint, after
      a convex combination of the first error), one pass by at most 0.5: a difference below 2, between integers at most 1.
    * the noisy pictures: the largest difference is printed and nothing asserted; it is the deviation the header names (79, 81, 77,
      93 grey levels on all_open, odd_target, resized_smaller_than_target, same_size; 0 on all_closed, which is only rotated)."""
    from tests import augment_cases as AC
    from tests import augment_restatement as RS
    g = np.load(GOLDEN)
    names = [str(n) for n in g["cases"]]
    ramps = [str(n) for n in g["ramp_cases"]]
    assert os.path.getsize(GOLDEN) < 200 * 1024 and len(names) >= 10 and len(ramps) == 5 and set(ramps) < set(names)
    seen = dict(rotated=False, resized=False, padded=False, pad_after_resize=False, flipped=False, unflipped=False, masked=False,
                negative_start=False, empty=False, images=0, odd=False, moved=False)
    ramp_seen = dict(only_rotated=False, grow=False, shrink_padded=False, resized_flip=False, resized_odd=False)
    ramp_pixels = 0
    for n in names:
        rgb, mask, hc, u = AC.golden_rgb(g, n), g[n + ".mask"], g[n + ".hcoords"], g[n + ".uniforms"]
        assert rgb.shape == (48, 64, 3) and rgb.dtype == np.uint8 and hc.dtype == np.float64
        height, width = (int(v) for v in g[n + ".size"])
        cfg = json.loads(str(g[n + ".cfg"]))
        image, m, out, status, plan = RS.augment_one(rgb, mask, hc, height, width, cfg, u, int(g[n + ".seed"]))
        ref = g[n + ".ref_hcoords"]
        assert ref.dtype == np.float64 and np.array_equal(out, ref), n
        assert status & ~RS.S_NO_FOREGROUND == 0, n                  # the reference ran: none of the definition's extensions
        assert g[n + ".ref_image"].dtype == np.uint8 and g[n + ".ref_image"].shape == (height, width, 3)
        assert np.array_equal(m, g[n + ".ref_mask"].astype(np.int64)), n
        integer_only = not plan["rotated"] and not plan["resized"]
        if integer_only:
            want = (g[n + ".ref_image"].astype(np.float32) / np.float32(255.0) - RS.MEAN) / RS.STD
            assert np.array_equal(image, want.transpose(2, 0, 1)), n
            seen["images"] += 1
        else:
            worst, pixels, anywhere = AC.two_pass_difference(AC.recover_uint8(image), g[n + ".ref_image"], plan, 48, 64)
            print(f"{n}: one pass against the reference's two: at most {worst} on {pixels} pixels 2 px inside, {anywhere} anywhere")
            if n in ramps:
                assert worst <= 1 and pixels >= 200 and m.sum() > 0, (n, worst, pixels)
                ramp_pixels += pixels
                ramp_seen["only_rotated"] |= not plan["resized"]
                ramp_seen["grow"] |= plan["resized"] and plan["ratio"] > 1
                ramp_seen["shrink_padded"] |= plan["resized"] and plan["ratio"] < 1 and plan["hoff"] > 0 and plan["woff"] > 0
                ramp_seen["resized_flip"] |= plan["resized"] and plan["flip"]
                ramp_seen["resized_odd"] |= plan["resized"] and width % 8 != 0
        assert (n in ramps) == (n + ".rgb" not in g) and (n not in ramps or (plan["rotated"] and u[0] >= 0.5))
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
        seen["masked"] |= bool(gate and integer_only and (g[n + ".ref_mask"].sum() < mask.sum()))
        seen["negative_start"] |= n == "negative_start" and bool(gate) and int(g[n + ".ref_mask"].sum()) == int(m.sum()) > 0
    assert all(seen.values()) and seen["images"] >= 5, seen
    assert all(ramp_seen.values()) and ramp_pixels >= 4000, (ramp_seen, ramp_pixels)
    # the negative start: the gate was open and nothing was masked out (the rectangle is empty, as the reference's slice is)
    n = "negative_start"
    _, m, _, _, plan = RS.augment_one(g[n + ".rgb"], g[n + ".mask"], g[n + ".hcoords"], 48, 64, dict(rotation=False, crop=False, flip=False),
                                      g[n + ".uniforms"], 1)
    assert np.array_equal(m, g[n + ".mask"].astype(np.int64))


def test_fixture_keeps_its_earlier_arrays():
    """the 100 arrays the fixture held before the reference's chain was recorded for every case and the ramp cases were appended:
    the same names in the same order, the same bytes (a digest over key, type, shape and data, taken from the earlier file)"""
    import hashlib
    g = np.load(GOLDEN)
    earlier = ["all_open", "all_closed", "odd_target", "resized_smaller_than_target", "flip_crop_only", "maskout_crop", "pad_both",
               "pad_rows_crop_columns", "negative_start", "empty_mask", "same_size"]
    assert [str(n) for n in g["cases"]][:11] == earlier
    pure = earlier[4:10]   # their image and mask were recorded already
    digest, count = hashlib.sha256(), 0
    for n in earlier:
        fields = ["rgb", "mask", "hcoords", "uniforms", "size", "seed", "cfg", "ref_hcoords"] + (["ref_image", "ref_mask"] if n in pure else [])
        for key in sorted(f"{n}.{f}" for f in fields):
            a = g[key]
            for part in (key.encode(), str(a.dtype).encode(), str(a.shape).encode(), np.ascontiguousarray(a).tobytes()):
                digest.update(part)
            count += 1
    assert count == 100 and digest.hexdigest() == "51a78897fb410a596ffbfe87718f96f64487e6304a8ac3ced07ba24cf343ce2e"


def test_ramp_closed_form_holds_for_the_restatement():
    """The restatement's image against ``rint(I(sx, sy))`` of a ramp source, the source point taken from the inverse of the composed
    FORWARD maps (tests/augment_cases.py), over the seeded set: 300 samples of status 0, 503 372 interior pixels, the worst
    ``|v - I(sx, sy)|`` 0.49999985 against the bar 0.5 + 1e-6.  The set's conditions are asserted from the restatement's plans."""
    from tests import augment_cases as AC
    groups = AC.ramp_set()
    assert len(groups) == 12 and {g["size"] for g in groups} == set(AC.TARGETS) and all(not g["maskout"] for g in groups)
    worst, counts = 0.0, []
    for g in groups:
        assert g["rgb"].shape[1:] == (48, 64, 3) and bool((g["want"][3] == 0).all()) and bool((g["U"][:, 0] >= 0.5).all())
        w, c, left = AC.ramp_check(g["want"][0], g)
        assert w <= AC.RAMP_BAR, (g["name"], w)
        assert sum(left) == 0
        worst, counts = max(worst, w), counts + c
    print(f"ramp closed form, restatement: worst |v - I(sx, sy)| = {worst:.8f} on {sum(counts)} interior pixels of {len(counts)} samples, "
          f"fewest per sample {min(counts)}")
    assert len(counts) >= 250 and sum(counts) >= AC.RAMP_MIN_INTERIOR_TOTAL and min(counts) >= AC.RAMP_MIN_INTERIOR_PER_SAMPLE
    features = AC.feature_counts(groups)
    assert set(features) == {"rotated", "grow", "shrink", "row_pad", "column_pad", "hbeg", "wbeg", "flip"}
    assert min(features.values()) >= 20, features


def test_ramp_bar_tells_a_defect():
    """Each of four mistakes a definition could share with its restatement and kernel, planted into a copy of the oracle's map, breaks
    the ramp check against the (unchanged) restatement -- so the same mistake in the restatement or the kernel breaks it against
    the (unchanged) oracle: the resize without its two half-pixel terms, ``width - X`` for the flip, ``b -> -b`` in the rotation,
    ``hoff`` and ``hbeg`` swapped.  Every one fails in at least 20 samples, and by whole grey levels."""
    from tests import augment_cases as AC
    groups = AC.ramp_set()
    for defect in AC.DEFECTS:
        failing, worst = 0, 0.0
        for g in groups:
            v = AC.recover_uint8(g["want"][0])
            for i, plan in enumerate(g["want"][4]):
                err = AC.ramp_errors(v[i], plan, 48, 64, defect)[0]
                if err.size and err.max() > AC.RAMP_BAR:
                    failing, worst = failing + 1, max(worst, float(err.max()))
        assert failing >= 20 and worst > 1.0, (defect, failing, worst)
    # and a map off by a hundredth of a pixel is seen: about 4 delta of the pixels of a slope-4 channel leave the bar
    g = groups[0]
    shifted = [dict(p, R=p["R"] + np.array([[0.0, 0.0, 0.01], [0.0, 0.0, 0.0]])) for p in g["want"][4]]
    v = AC.recover_uint8(g["want"][0])
    over = sum(int((AC.ramp_errors(v[i], p, 48, 64)[0] > AC.RAMP_BAR).sum()) for i, p in enumerate(shifted))
    assert over >= 100, over


def test_ramp_with_the_mask_out_gate_open_and_an_odd_source():
    """The gate open: pixels with a tap inside the rectangle carry the random fill and are left out; they are present, and with them
    in, the check fails.  A 37 x 53 source (w no multiple of 8) under slopes of its own."""
    from tests import augment_cases as AC
    from tests import augment_restatement as RS
    g = AC.ramp_maskout_case()
    assert g["maskout"] and bool((g["U"][:, 0] < 0.5).all()) and bool((g["want"][3] == 0).all())
    worst, counts, left = AC.ramp_check(g["want"][0], g)
    assert worst <= AC.RAMP_BAR and min(left) > 0 and sum(left) >= 500 and min(counts) >= 500, (worst, counts, left)
    v = AC.recover_uint8(g["want"][0])
    assert all(AC.ramp_errors(v[i], p, 48, 64)[0].max() > 1.0 for i, p in enumerate(g["want"][4]))   # without the exclusion
    # the rectangle the oracle leaves out is the one the restatement filled: without geometry the mask loses exactly its pixels
    for i in range(len(g["mask"])):
        rows, cols = AC.maskout_rectangle(g["mask"][i], g["cfg"], g["U"][i])
        m = RS.augment_one(g["rgb"][i], g["mask"][i], g["hc"][i], 48, 64, dict(g["cfg"], rotation=False, crop=False, flip=False), g["U"][i],
                           g["seed"], i)[1]
        want = g["mask"][i].astype(np.int64)
        want[np.ix_(rows, cols)] = 0
        assert len(rows) and len(cols) and np.array_equal(m, want) and want.sum() < g["mask"][i].sum()
    odd = AC.ramp_odd_source()
    assert [o["size"] for o in odd] == [(32, 40), (31, 37)]
    for o in odd:
        assert o["rgb"].shape[1:] == (37, 53, 3) and bool((o["want"][3] == 0).all())
        worst, counts, _ = AC.ramp_check(o["want"][0], o)
        assert worst <= AC.RAMP_BAR and min(counts) >= 500, (worst, counts)


def test_sweep_walks_every_branch():
    """what the device sweep (tests/test_augment_device.py) covers, asserted here from the restatement's plans and status, so that the
    GPU test cannot pass by leaving a branch out"""
    from tests import augment_cases as AC
    calls = AC.sweep_calls()
    cover = AC.sweep_coverage(calls)
    assert cover["samples"] >= 192 and all(32 <= len(c["rgb"]) <= 64 for c in calls)
    assert all(cover[f"status_{b}"] >= 1 for b in (1, 2, 4, 8)), cover
    for key in ("rotated", "resized", "flip", "maskmul"):
        assert cover[key] >= 10 and cover["not_" + key] >= 10, (key, cover)
    assert min(cover["row_pad"], cover["column_pad"], cover["row_crop"], cover["column_crop"]) >= 10, cover
    assert {c["rgb"].shape[1:3] for c in calls} == {(48, 64), (37, 53)}
    assert {c["size"] for c in calls} == {(32, 40), (31, 37), (56, 72), (48, 64), (56, 40)}
    assert {tuple(sorted((k, v) for k, v in c["cfg"].items() if k.startswith("resize_"))) for c in calls} == \
        {tuple(sorted(r.items())) for r in AC.RANGES.values()}
    assert {c["out_dtype"] for c in calls} == {"float32", "bfloat16", "float16"} and {c["mask_in"] for c in calls} == {"uint8", "int32", "int64"}
    assert {bool(c["cfg"].get("use_mask_out")) for c in calls} == {True, False} and sum(c["pad_strides"] for c in calls) == 1
    U = np.concatenate([c["U"] for c in calls])
    assert U.shape[1] == 12 and U.min() >= 0 and U.max() < 1 and bool(((U < 0.1).any(0) & (U > 0.9).any(0)).all())
    masks = [m for c in calls for m in c["mask"]]
    rows = lambda m: np.flatnonzero(m.any(1))   # noqa: E731
    cols = lambda m: np.flatnonzero(m.any(0))   # noqa: E731
    assert sum(not m.any() for m in masks) >= 5
    assert sum(m.any() and len(rows(m)) == 1 and len(cols(m)) > 1 for m in masks) >= 5
    assert sum(m.any() and len(cols(m)) == 1 and len(rows(m)) > 1 for m in masks) >= 5
    assert sum(bool(m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any()) for m in masks) >= 5


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
