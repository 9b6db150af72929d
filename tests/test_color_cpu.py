"""CPU-only checks of the colour jitter on the device (include/pvnet_color.h, libpvnet_color.so): the header's exports against the
prototype table of pvnet_amd/_abi.py, the built library, every bad argument rejected with the documented code before any HIP call,
the register rule for the new kernels, the configuration's defaults against the reference's JSON, the reference's configuration
loading as it stands, the properties of the numpy restatement (tests/color_restatement.py) that follow from the definition, and that
restatement against Pillow itself (tests/pillow_jitter_oracle.py, where Pillow is importable) and against the bytes recorded from it
(tests/golden/color_pillow.npz, always).
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
from tests import color_restatement as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_color.h")).read()
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
EXPORTS = {"pvnet_color_abi_version", "pvnet_color_workspace_bytes", "pvnet_color_jitter", "pvnet_augment_jitter"}
KERNELS = ("color_zero_kernel", "color_stats_kernel", "color_apply_kernel", "color_plan_kernel", "color_warp_kernel")
CFG_JSON = os.path.join(ROOT, "tests", "golden", "default_linemod_cfg.json")
ZERO = dict(brightness=0, contrast=0, saturation=0, hue=0)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _abi.load_color_library()


def test_header_declares_the_exports_and_every_one_has_a_prototype():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS
    decl = re.search(r"^int pvnet_augment_jitter\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.COLOR_PROTOTYPES["pvnet_augment_jitter"][1]
    assert "size_t workspace_bytes" in decl[-2] and args[-2] is C.c_size_t
    assert "uint64_t seed" in decl[14] and args[14] is C.c_uint64
    assert "PvnetColorConfig* jitter" in decl[15] and "jitter_uniforms" in decl[16]
    # what is left of it without the two added arguments is pvnet_augment's prototype
    assert args[:15] + args[17:] == _abi.AUGMENT_PROTOTYPES["pvnet_augment"][1]
    decl = re.search(r"^int pvnet_color_jitter\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    assert "size_t workspace_bytes" in decl[-2] and _abi.COLOR_PROTOTYPES["pvnet_color_jitter"][1][-2] is C.c_size_t
    # every constant of the header is mirrored by value
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_COLOR_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.COLOR_ABI_VERSION == 1
    assert len(consts) == 5
    for name, value in consts.items():
        assert getattr(_abi, "COLOR_" + name) == value, name
    assert (RS.B, RS.C, RS.S, RS.H) == (_abi.COLOR_STEP_B, _abi.COLOR_STEP_C, _abi.COLOR_STEP_S, _abi.COLOR_STEP_H)
    # the configuration struct: the same fields in the same order
    body = re.search(r"typedef struct PvnetColorConfig \{(.*?)\} PvnetColorConfig;", HDR, re.S).group(1)
    fields = [f.strip().split("[")[0] for line in re.sub(r"/\*.*?\*/", "", body).split(";") if line.strip()
              for f in line.strip().split(None, 1)[1].split(",")]
    assert fields == [n for n, _ in _abi.ColorConfigStruct._fields_]
    assert C.sizeof(_abi.ColorConfigStruct) == 4 * 8 + 6 * 4
    # the header says whose text it is, that it is held to Pillow byte for byte (the version, the record), and what blur is
    assert "THIS PROJECT'S" in HDR and "Pillow byte for byte" in HDR and "Pillow 12.2.0" in HDR and "tests/golden/color_pillow.npz" in HDR
    assert "may differ" not in HDR and "Nothing was recorded" not in HDR
    assert "linemod_dataset.py:232" in HDR and "augmentation.py:204-205" in HDR


def test_library_is_built_for_gfx950_and_exports_the_symbols(lib):
    blob = open(_abi.COLOR_LIB_PATH, "rb").read()
    assert all(k.encode() in blob for k in KERNELS)
    assert build.SIDE_LIBRARIES["color"][:2] == (["color_jitter.hip"], "pvnet_color.h")
    # the augment library still holds its own kernels under their names, and none of this library's
    aug = open(_abi.AUGMENT_LIB_PATH, "rb").read()
    assert b"augment_plan_kernel" in aug and b"augment_warp_kernel" in aug and not any(k.encode() in aug for k in KERNELS)
    ws = lib.pvnet_color_workspace_bytes
    assert ws(0, 0, 0) == 0 and ws(65536, 0, 0) == 0 and ws(-1, 0, 0) == 0 and ws(1, -1, 4) == 0 and ws(1, 0, 4) == 0
    assert ws(1, 0, 0) == 16 and ws(3, 0, 0) == 32                       # S_L: 8 bytes per image, rounded up to 16
    assert ws(4, 32, 48) == 32 + 4 * 112 + 4 * 32 * 48 * 3              # S_L, the plans, 3 bytes per output pixel
    assert ws(1, 32769, 8) == 0


def test_bad_arguments_are_rejected_without_a_device(lib):
    from pvnet_amd.augment import AugmentConfig
    from pvnet_amd.color import ColorJitterConfig
    # fake (never dereferenced) non-null pointers: validation must return before any HIP call
    p = C.c_void_p(0x1000)
    s3 = (C.c_int64 * 3)(1, 1, 1)
    good, jgood = AugmentConfig().struct(), ColorJitterConfig().struct()
    U8, I16, I32, I64, F32 = 0, 1, 2, 3, 4

    def jcfg(**kw):
        s = ColorJitterConfig().struct()
        for k, v in kw.items():
            if k in ("mean", "std"):
                getattr(s, k)[:] = v
            else:
                setattr(s, k, v)
        return s

    def jit(rgb=p, rs=s3, un=p, b=4, h=48, w=64, c=jgood, mask=None, mdt=U8, ms=None, mul=None, image=p, idt=0, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_color_workspace_bytes(max(b, 1), 0, 0)
        return lib.pvnet_color_jitter(rgb, rs, un, b, h, w, None if c is None else C.byref(c), mask, mdt, ms, mul, image, idt, ws, wsb, None)

    for name in ("rgb", "rs", "un", "c", "image"):
        assert jit(**{name: None}) == BADARG, name
    assert jit(b=-1) == BADARG and jit(h=0) == BADARG and jit(w=0) == BADARG and jit(idt=3) == BADARG and jit(idt=-1) == BADARG
    for key in ("brightness", "contrast", "saturation", "hue"):
        assert jit(c=jcfg(**{key: -0.1})) == BADARG and jit(c=jcfg(**{key: float("nan")})) == BADARG, key
        assert jit(c=jcfg(**{key: float("inf")})) == BADARG, key
    assert jit(c=jcfg(hue=0.51)) == BADARG and jit(c=jcfg(hue=0.5), b=0) == 0 and jit(c=jcfg(brightness=2e6)) == BADARG
    assert jit(c=jcfg(std=(0.2, 0.0, 0.2))) == BADARG and jit(c=jcfg(mean=(float("nan"), 0.0, 0.0))) == BADARG
    assert jit(mask=p) == BADARG and jit(mul=p) == BADARG and jit(mask=p, mul=p) == BADARG        # both or neither; strides with them
    assert jit(mask=p, mul=p, ms=s3, mdt=99) == BADARG and jit(mask=p, mul=p, ms=s3, mdt=I16) == UNSUPPORTED
    assert jit(mask=p, mul=p, ms=s3, mdt=F32) == UNSUPPORTED
    assert jit(b=65536) == UNSUPPORTED and jit(h=32769) == UNSUPPORTED and jit(h=32768, w=32768 + 1) == UNSUPPORTED
    assert jit(ws=None) == WORKSPACE and jit(wsb=lib.pvnet_color_workspace_bytes(4, 0, 0) - 1) == WORKSPACE
    assert jit(ws=C.c_void_p(0x2004)) == BADARG                     # misaligned workspace
    for idt in (0, 1, 2):
        assert jit(b=0, idt=idt, ws=None, wsb=0) == 0               # nothing to do, nothing enqueued
        for mdt in (U8, I32, I64):
            assert jit(b=0, idt=idt, mask=p, mul=p, ms=s3, mdt=mdt, ws=None, wsb=0) == 0

    def aug(rgb=p, rs=s3, mask=p, mdt=U8, ms=s3, hc=p, un=p, b=4, h=48, w=64, vn=9, height=32, width=40, c=good, seed=1, j=jgood, jun=p,
            image=p, idt=0, mo=p, modt=U8, hco=p, status=p, ws=C.c_void_p(0x2000), wsb=None):
        if wsb is None:
            wsb = lib.pvnet_color_workspace_bytes(max(b, 1), max(height, 1), max(width, 1))
        return lib.pvnet_augment_jitter(rgb, rs, mask, mdt, ms, hc, un, b, h, w, vn, height, width, None if c is None else C.byref(c), seed,
                                        None if j is None else C.byref(j), jun, image, idt, mo, modt, hco, status, ws, wsb, None)

    def cfg(**kw):
        s = AugmentConfig().struct()
        for k, v in kw.items():
            if k in ("mean", "std"):
                getattr(s, k)[:] = v
            else:
                setattr(s, k, v)
        return s

    # pvnet_augment's own checks, with its codes
    for name in ("rgb", "rs", "mask", "ms", "hc", "un", "c", "image", "mo", "hco", "status", "j", "jun"):
        assert aug(**{name: None}) == BADARG, name
    assert aug(b=-1) == BADARG and aug(h=0) == BADARG and aug(w=0) == BADARG and aug(vn=0) == BADARG
    assert aug(height=0) == BADARG and aug(width=-3) == BADARG and aug(idt=3) == BADARG
    assert aug(mdt=99) == BADARG and aug(mdt=I16) == UNSUPPORTED and aug(mdt=F32) == UNSUPPORTED
    assert aug(modt=I32) == BADARG and aug(modt=F32) == BADARG
    assert aug(c=cfg(flags=32)) == BADARG and aug(c=cfg(reserved=1)) == BADARG and aug(c=cfg(std=(0.2, 0.0, 0.2))) == BADARG
    assert aug(c=cfg(min_mask=-0.1)) == BADARG and aug(c=cfg(overlap_ratio=1.5)) == BADARG and aug(c=cfg(resize_hmin=0.0)) == BADARG
    assert aug(c=cfg(flags=_abi.AUGMENT_F_FLIP)) == BADARG           # without the crop the output is the source's size
    assert aug(c=cfg(flags=_abi.AUGMENT_F_FLIP), height=48, width=64, b=0) == 0
    assert aug(b=65536) == UNSUPPORTED and aug(h=32769) == UNSUPPORTED and aug(height=40000) == UNSUPPORTED
    # the jitter's
    assert aug(j=jcfg(contrast=-1.0)) == BADARG and aug(j=jcfg(hue=0.6)) == BADARG and aug(j=jcfg(saturation=float("nan"))) == BADARG
    assert aug(j=jcfg(std=(0.0, 0.0, 0.0)), b=0) == 0                # its mean and std are not read
    assert aug(ws=None) == WORKSPACE and aug(wsb=lib.pvnet_color_workspace_bytes(4, 32, 40) - 1) == WORKSPACE
    assert aug(wsb=lib.pvnet_color_workspace_bytes(4, 0, 0)) == WORKSPACE
    assert aug(ws=C.c_void_p(0x2008)) == BADARG                     # the workspace is 16-byte aligned
    for mdt in (U8, I32, I64):
        for modt in (U8, I64):
            for idt in (0, 1, 2):
                assert aug(mdt=mdt, modt=modt, idt=idt, b=0, ws=None, wsb=0) == 0


def test_register_check_covers_the_new_translation_unit(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as chk
    (src, text), = chk.side_assembly("color")
    assert src.endswith("color_jitter.hip")
    ks = chk.kernels(text)
    # the zeroing, the statistics, 3 element types x 2 store paths of the apply, the plan, 2 store paths of the warp
    assert len(ks) == 11 and all(any(k in name for name, _, _, _ in ks) for k in KERNELS)
    assert not any("head_" in chk.short(name) or "augment_" in chk.short(name) for name, _, _, _ in ks)
    for name, nfv, vmax, scratch in ks:
        assert nfv - (vmax + 1) >= chk.SLACK and scratch == 0, name
    # the vector path stores 16 bytes at a time
    assert "global_store_dwordx4" in text


def test_config_defaults_are_the_references_and_its_file_loads_as_it_stands():
    from pvnet_amd.augment import AugmentConfig
    from pvnet_amd.color import ColorJitterConfig, training_configs_from_reference
    ref = json.load(open(CFG_JSON))
    assert ref["jitter"] is True and ref["blur"] is True
    jc = ColorJitterConfig()
    for key in ("brightness", "contrast", "saturation", "hue"):
        assert getattr(jc, key) == ref[key] == RS.DEFAULTS[key], key
    with pytest.raises(NotImplementedError):      # the augment library's own class still refuses the file
        AugmentConfig.from_reference(ref)
    aug, jit = training_configs_from_reference(ref)
    assert aug == AugmentConfig() and jit == ColorJitterConfig() and type(jit) is ColorJitterConfig
    assert training_configs_from_reference(dict(ref, jitter=False)) == (AugmentConfig(), None)
    assert training_configs_from_reference(dict(ref, blur=False))[1] == jit
    aug, jit = training_configs_from_reference(dict(ref, hue=0.25, use_mask_out=True, flip=False))
    assert jit == ColorJitterConfig(hue=0.25) and aug == AugmentConfig(use_mask_out=True, flip=False)
    assert training_configs_from_reference(ref, rotation=False)[0] == AugmentConfig(rotation=False)
    with pytest.raises(NotImplementedError):
        training_configs_from_reference(dict(ref, use_old=True))
    s = jc.struct()
    assert (s.brightness, s.contrast, s.saturation, s.hue) == (0.1, 0.1, 0.1, 0.1)
    assert list(s.mean) == [np.float32(v) for v in (0.485, 0.456, 0.406)] and list(s.std) == [np.float32(v) for v in (0.229, 0.224, 0.225)]
    assert list(s.mean) == list(RS.MEAN) and list(s.std) == list(RS.STD)
    for bad in (dict(brightness=-0.1), dict(hue=0.6), dict(contrast=float("nan"))):
        with pytest.raises(ValueError):
            ColorJitterConfig(**bad)
    ColorJitterConfig(**ZERO)


def test_python_entries_refuse_host_tensors_and_bad_uniforms():
    import torch
    from pvnet_amd import color as K
    from pvnet_amd.augment import AugmentConfig, draw_uniforms
    rgb = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        K.jitter_batch(rgb, K.ColorJitterConfig(), K.draw_jitter_uniforms(1))
    with pytest.raises(RuntimeError, match="CUDA"):
        K.augment_jitter_batch(rgb, torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 2, 3), dtype=torch.float64), 8, 8,
                               AugmentConfig(), K.ColorJitterConfig(), draw_uniforms(1), K.draw_jitter_uniforms(1), 0)
    u = K.draw_jitter_uniforms(3, torch.Generator().manual_seed(5))
    assert u.shape == (3, 5) and u.dtype == torch.float64 and bool(((u >= 0) & (u < 1)).all())
    assert torch.equal(u, K.draw_jitter_uniforms(3, torch.Generator().manual_seed(5)))
    assert torch.equal(K._device_jitter_uniforms(u, 3, torch.device("cpu")), u)
    for bad in (torch.ones((3, 5), dtype=torch.float64), u.float(), u[:2], u[:, :4]):
        with pytest.raises(RuntimeError):
            K._device_jitter_uniforms(bad, 3, torch.device("cpu"))


# ---- the restatement's properties ----------------------------------------------------------------------------------------------------

def image(seed=0, h=16, w=24):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def u_for(range_, factor):
    """the uniform that gives `factor` under range(range_, u) (exactly, for the values used here)"""
    lo, hi = max(0.0, 1.0 - range_), 1.0 + range_
    return (factor - lo) / (hi - lo)


def test_restatement_all_ranges_zero_is_the_plain_normalisation():
    rgb = image(1)
    for u4 in (0.0, 0.37, 0.999):
        got = RS.jitter_one(rgb, ZERO, np.array([0.1, 0.9, 0.3, 0.7, u4]))
        want = ((rgb.astype(np.float32) / np.float32(255.0) - RS.MEAN) / RS.STD).transpose(2, 0, 1)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert RS.chain(ZERO, np.array([0.1, 0.9, 0.3, 0.7, u4]))[4] == []
    # use_mask_out: the multiply after the normalisation, only where maskmul says so
    mask = (np.arange(16 * 24).reshape(16, 24) % 3).astype(np.uint8)
    u = np.array([0.1, 0.9, 0.3, 0.7, 0.5])
    assert np.array_equal(RS.jitter_one(rgb, ZERO, u, mask, 1), RS.jitter_one(rgb, ZERO, u) * mask.astype(np.float32)[None])
    assert np.array_equal(RS.jitter_one(rgb, ZERO, u, mask, 0), RS.jitter_one(rgb, ZERO, u))


def test_restatement_unit_factors_are_identities_and_grey_is_fixed():
    rgb = image(2)
    half = u_for(0.5, 1.0)
    assert RS.range_factor(0.5, half) == np.float32(1.0) and RS.range_factor(2.0, u_for(2.0, 1.0)) == np.float32(1.0)
    for key, slot in (("brightness", 0), ("contrast", 1), ("saturation", 2)):
        u = np.array([0.3, 0.3, 0.3, 0.3, 0.0])
        u[slot] = half
        out, trace = RS.jitter_uint8(rgb, dict(ZERO, **{key: 0.5}), u)
        assert [s for s, _ in trace] == [{"brightness": RS.B, "contrast": RS.C, "saturation": RS.S}[key]]
        assert np.array_equal(out, rgb), key
    # a grey image is unchanged by S, whatever the factor; H maps grey and black pixels to themselves, whatever the shift
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    for u2 in (0.0, 0.4, 0.999):
        assert np.array_equal(RS.jitter_uint8(grey, dict(ZERO, saturation=0.9), np.array([0, 0, u2, 0, 0.0]))[0], grey)
    for u3 in (0.0, 0.2, 0.5, 0.999):
        assert np.array_equal(RS.jitter_uint8(grey, dict(ZERO, hue=0.5), np.array([0, 0, 0, u3, 0.0]))[0], grey)
    assert int(grey[0, 0].sum()) == 0                       # the ramp begins at black


def test_restatement_orders_mean_clip_and_hue_wrap():
    # the 24 orders are distinct permutations, lexicographic, reached by u4 = (k + 0.5) / 24; u4 -> 1 stays at 23
    orders = [tuple(RS.chain({}, np.array([0.5, 0.5, 0.5, 0.5, (k + 0.5) / 24]))[4]) for k in range(24)]
    assert len(set(orders)) == 24 and all(sorted(o) == [0, 1, 2, 3] for o in orders) and orders == sorted(orders)
    assert orders[0] == (RS.B, RS.C, RS.S, RS.H) and orders[1] == (RS.B, RS.C, RS.H, RS.S) and orders[23] == (RS.H, RS.S, RS.C, RS.B)
    assert tuple(RS.chain({}, np.array([0.5, 0.5, 0.5, 0.5, 1.0 - 2.0 ** -53]))[4]) == orders[23]
    # absent steps are dropped from the chosen permutation
    assert RS.chain(dict(contrast=0, hue=0), np.array([0.5, 0.5, 0.5, 0.5, 23.5 / 24]))[4] == [RS.S, RS.B]
    # the order matters: the chains give different images
    rgb = image(3)
    outs = {RS.jitter_uint8(rgb, dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.2), np.array([0.9, 0.1, 0.8, 0.3, (k + 0.5) / 24]))[0]
            .tobytes() for k in range(24)}
    assert len(outs) > 12
    # m rounds halves up: lumas 10 and 11 over two pixels give (2 * 21 + 2) // 4 = 11; 10, 10, 10, 11 give 10
    two = np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)
    assert list(RS.luma(two)[0]) == [10, 11] and RS.mean_luma(two) == 11
    four = np.array([[[10, 10, 10]] * 3 + [[11, 11, 11]]], np.uint8)
    assert RS.mean_luma(four) == 10
    assert RS.luma(np.array([255, 255, 255])) == 255 and RS.luma(np.array([0, 0, 0])) == 0
    # C blends with m of the image as it stands when the step is reached: B before C changes m
    u = np.array([0.999, 0.0, 0.5, 0.5, 0.0])
    _, trace = RS.jitter_uint8(rgb, dict(ZERO, brightness=0.5, contrast=0.5), u)                 # B C
    _, trace2 = RS.jitter_uint8(rgb, dict(ZERO, brightness=0.5, contrast=0.5), np.array([0.999, 0.0, 0.5, 0.5, 6.5 / 24]))   # C B
    assert [s for s, _ in trace] == [RS.B, RS.C] and [s for s, _ in trace2] == [RS.C, RS.B]
    assert trace2[0][1] == RS.mean_luma(rgb) and trace[1][1] > trace2[0][1]
    # the clip branch: fb > 1 on pixels of 250 and above gives 255; the blend truncates
    bright = np.full((4, 8, 3), 250, np.uint8)
    bright[1] = 253
    bright[2] = 255
    out, _ = RS.jitter_uint8(bright, dict(ZERO, brightness=0.5), np.array([0.9, 0, 0, 0, 0.0]))
    assert RS.range_factor(0.5, 0.9) > 1.02 and bool((out == 255).all())
    assert int(RS.blend(0, np.array([7]), np.float32(0.7))[0]) == 4                          # 4.9 truncates
    assert int(RS.blend(100, np.array([0]), np.float32(1.5))[0]) == 0                        # -50 clips
    # a negative fh wraps the hue: red shifted by -1/6 of the circle is magenta-ish, by +1/3 green
    red = np.zeros((2, 8, 3), np.uint8)
    red[..., 0] = 200
    neg = RS.hue_factor(0.5, 1.0 / 3.0)
    assert neg < 0 and int(np.float32(neg) * np.float32(255)) % 256 > 128                    # the shift wrapped
    out, _ = RS.jitter_uint8(red, dict(ZERO, hue=0.5), np.array([0, 0, 0, 1.0 / 3.0, 0.0]))
    assert out[0, 0, 0] == 200 and out[0, 0, 1] == 0 and out[0, 0, 2] > 150
    out, _ = RS.jitter_uint8(red, dict(ZERO, hue=0.5), np.array([0, 0, 0, 5.0 / 6.0, 0.0]))
    assert out[0, 0, 1] == 200 and out[0, 0, 2] == 0 and out[0, 0, 0] < 10


# ---- the restatement against Pillow (tests/pillow_jitter_oracle.py) and against what was recorded from it --------------------------------

from tests import pillow_jitter_oracle as PO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "color_pillow.npz")
KEYS = ("brightness", "contrast", "saturation", "hue")


def pil():
    """' (Pillow x.y.z)' for the assertion messages; skips without Pillow"""
    return f" (Pillow {pytest.importorskip('PIL').__version__})"


def slabs():
    """all 2^24 colours as 16 images [4096,256,3] uint8"""
    for r0 in range(0, 256, 16):
        r, g, b = np.meshgrid(np.arange(r0, r0 + 16), np.arange(256), np.arange(256), indexing="ij")
        yield np.stack([r, g, b], -1).reshape(16 * 256, 256, 3).astype(np.uint8)


@pytest.fixture(scope="module")
def forward_pass():
    """the forward conversion over all 2^24 colours, once: (mismatches with Pillow per plane, the distinct (s, v) pairs, the number
    of colours on which the float32-only hue differs per maxc branch)"""
    tag = pil()
    bad, pairs, hard = np.zeros(3, np.int64), set(), np.zeros(3, np.int64)
    for img in slabs():
        h, s, v = RS.rgb_to_hsv(img)
        for k, (got, want) in enumerate(zip((h, s, v), PO.rgb_to_hsv(img))):
            bad[k] += int((got != want).sum())
        pairs.update(np.unique(s * 256 + v).tolist())
        d = RS.rgb_to_hsv(img, float32_only=True)[0] != h
        m = img.max(-1)
        branch = np.where(img[..., 0] == m, 0, np.where(img[..., 1] == m, 1, 2))
        hard += np.bincount(branch[d], minlength=3)
    return bad, np.array(sorted(pairs)), hard, tag


def test_forward_hsv_equals_pillow_on_every_colour(forward_pass):
    bad, pairs, hard, tag = forward_pass
    print(f"forward conversion over 2^24 colours{tag}: mismatches in h, s, v {bad.tolist()}; {len(pairs)} distinct (s, v); the float32-only "
          f"hue differs on {hard.tolist()} colours of the r, g, b branches")
    assert bad.tolist() == [0, 0, 0], f"h, s, v mismatches {bad.tolist()}{tag}"
    # the float32-only hue is another one: on no colour of the r branch (float32 there by definition), on many of the others
    assert hard[0] > 0 and hard[1] > 0 and hard[2] > 0 and int(hard.sum()) == 72036, f"{hard.tolist()}{tag}"


def test_back_conversion_equals_pillow_on_every_triple_that_occurs(forward_pass):
    """every (s, v) that the forward pass produces x all 256 h: every (h, s, v) that occurs, under every shift"""
    _, pairs, _, tag = forward_pass
    s, v = pairs // 256, pairs % 256
    shape = (len(pairs), 256)
    h = np.broadcast_to(np.arange(256)[None, :], shape)
    s, v = np.broadcast_to(s[:, None], shape), np.broadcast_to(v[:, None], shape)
    got, want = RS.hsv_to_rgb(h, s, v), PO.hsv_to_rgb(h, s, v)
    bad = np.argwhere(got != want)
    print(f"back conversion over {len(pairs)} x 256 (h, s, v){tag}: {len(bad)} mismatching bytes")
    assert len(bad) == 0, f"{len(bad)} bytes, first (s, v, h, channel) {(int(s[bad[0][0], 0]), int(v[bad[0][0], 0]), *bad[0][1:].tolist())}{tag}"
    assert len(pairs) > 30000 and (199 * 256 + 206) in set(pairs.tolist())   # where x - floor(x) of a float32 x misses Pillow's byte


def half_image():
    """a 4 x 4 image of random colours whose luma sum puts (2 S_L + N) / (2 N) exactly on a half"""
    for seed in range(1000):
        img = np.random.default_rng(seed).integers(0, 256, (4, 4, 3), dtype=np.uint8)
        if int(RS.luma(img).sum()) % 16 == 8:
            return img
    raise AssertionError("no such image")


def test_steps_b_s_c_equal_pillow():
    tag = pil()
    half = half_image()
    assert (2 * int(RS.luma(half).sum())) % (2 * 16) == 16 and RS.mean_luma(half) == int(RS.luma(half).sum()) // 16 + 1
    images = {"48 x 64": image(20, 48, 64), "1 x 1": np.array([[[200, 17, 90]]], np.uint8), "half": half,
              "two greys": np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)}
    for name, rgb in images.items():
        for factor in (0.0, 0.9, 1.1, 2.0, 1e6):
            f = np.float32(factor)
            for s, fn in ((RS.B, PO.adjust_brightness), (RS.S, PO.adjust_saturation), (RS.C, PO.adjust_contrast)):
                got = RS.step(rgb.astype(np.int64), s, f)[0]
                want = np.asarray(fn(PO.to_pil(rgb), float(f)))
                assert np.array_equal(got, want), f"step {s}, factor {factor}, image {name}: {int((got != want).sum())} bytes differ{tag}"


def all_chains():
    """(cfg, uniforms) of all 24 orders x the 16 subsets of present steps, wide ranges, hue factors of both signs"""
    wide = dict(brightness=0.6, contrast=0.7, saturation=0.8, hue=0.5)
    rng = np.random.default_rng(21)
    for k in range(24):
        for subset in range(16):
            cfg = {key: (wide[key] if subset >> j & 1 else 0) for j, key in enumerate(KEYS)}
            u = rng.uniform(0.0, 1.0, 5)
            u[3] = rng.uniform(0.02, 0.48) + 0.5 * ((k + subset) & 1)
            u[4] = (k + 0.5) / 24
            yield cfg, u


def test_chain_equals_pillow_for_every_order_and_subset():
    tag = pil()
    rgb = np.load(GOLDEN)["image"]
    signs = set()
    for cfg, u in all_chains():
        got = RS.jitter_uint8(rgb, cfg, u)[0]
        want = PO.jitter_uint8(rgb, cfg, u)
        assert np.array_equal(got, want), f"{cfg}, {u.tolist()}: {int((got != want).sum())} bytes differ{tag}"
        signs.add((cfg["hue"] != 0, bool(RS.hue_factor(0.5, u[3]) < 0)))
    assert signs == {(a, b) for a in (False, True) for b in (False, True)}


def check_chain_against_fixture():
    z = np.load(GOLDEN)
    rgb, ranges, U, want = z["image"], z["ranges"], z["uniforms"], z["want"]
    version = str(z["pil_version"])
    assert rgb.shape == (32, 40, 3) and rgb.dtype == np.uint8 and want.shape == (48, 2, 32, 40, 3) and want.dtype == np.uint8
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "head_metrics.npz"))
    # half of the image: colours on which the float32-only hue differs, of all three maxc branches
    top = rgb[:16].reshape(-1, 3)
    assert bool((RS.rgb_to_hsv(top)[0] != RS.rgb_to_hsv(top, float32_only=True)[0]).all())
    m = top.max(1)
    assert min(int((top[:, 0] == m).sum()), int(((top[:, 0] != m) & (top[:, 1] == m)).sum()), int(((top[:, 0] != m) & (top[:, 1] != m)).sum())) >= 200
    orders = []
    for c in range(48):
        cfg = dict(zip(KEYS, ranges[c]))
        for j in range(2):
            got = RS.jitter_uint8(rgb, cfg, U[c, j])[0]
            assert np.array_equal(got, want[c, j]), f"case {c}.{j}: {int((got != want[c, j]).sum())} bytes differ (recorded from Pillow {version})"
        assert cfg["hue"] == 0 or RS.hue_factor(cfg["hue"], U[c, 0, 3]) < 0 < RS.hue_factor(cfg["hue"], U[c, 1, 3])
        orders.append((RS.ORDERS.index(tuple(RS.chain({}, U[c, 0])[4])), int((ranges[c] == 0).sum())))
    # each of the 24 orders twice: all four steps, and one absent, rotating through the four
    assert orders == [(k, copy) for k in range(24) for copy in (0, 1)]
    assert [int(np.argmin(ranges[2 * k + 1])) for k in range(24)] == [k % 4 for k in range(24)]
    return version


def test_chain_equals_the_bytes_recorded_from_pillow():
    assert check_chain_against_fixture() == "12.2.0"


def test_fixture_needs_no_pillow(monkeypatch):
    """with PIL unimportable the comparison with the recorded bytes runs all the same"""
    for name in [n for n in sys.modules if n == "PIL" or n.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError):
        import PIL  # noqa: F401
    check_chain_against_fixture()


def test_fixture_is_what_its_maker_writes():
    tag = pil()
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_color_golden as maker
    rng = np.random.default_rng(20240)
    z = np.load(GOLDEN)
    img, n_hard = maker.make_image(rng)
    ranges, uniforms = maker.make_cases(rng)
    assert np.array_equal(img, z["image"]) and np.array_equal(ranges, z["ranges"]) and np.array_equal(uniforms, z["uniforms"]), tag
    assert n_hard == int(z["hard_colours"]) == 72036


def test_hue_shift_equals_torchvisions_near_every_step():
    """float32 factors within 4 ulp of n / 255, n = -127 .. 127: the definition's float32 product against the oracle's double one"""
    tag = pil()
    count = 0
    for n in range(-127, 128):
        c = np.float32(n / 255)
        vals, lo, hi = [c], c, c
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1))
            vals += [lo, hi]
        for f in vals:
            assert abs(float(f)) <= 0.5
            got, want = RS.hue_shift(f), PO.hue_shift(f)
            assert got == want == int(np.uint8(np.int64(float(f) * 255))), f"fh = {float(f)!r}: {got} against {want}{tag}"
            count += 1
    assert count == 255 * 9
