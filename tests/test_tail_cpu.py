"""CPU-only checks of the fused network tail (include/pvnet_tail.h, libpvnet_tail.so, pvnet_amd/tail.py): the registry rows and their
place, the header's constants against pvnet_amd/_abi.py, every bad argument rejected before any HIP call, ``TailParams``' folding of the
BatchNorm against torch's own and its refusals, both attribute spellings of the tail (the network class: tests/test_net_cpu.py), and
the restatement (tests/tail_restatement.py): against fixture G9, against torch's float64 interpolation, against a known
answer that needs no code to state, and against planted mistakes, each of which the stage bars must catch.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

from pvnet_amd import _abi, build  # noqa: E402
from pvnet_amd import tail as T  # noqa: E402
from tests import tail_cases as TC  # noqa: E402
from tests import tail_restatement as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_tail.h")).read()
BADARG, UNSUPPORTED = -1, -3


# ---- 1. the registry rows and the ABI mirror -------------------------------------------------------------------------------------------
def test_registry_rows_and_their_place():
    assert build.SIDE_LIBRARIES["tail"] == (["tail.hip"], "pvnet_tail.h", [])
    for table in (build.SIDE_LIBRARIES, _abi.SIDE_LIBRARIES):
        names = list(table)
        assert names.index("tail") == names.index("texture") - 1 == len(names) - 2   # before texture, which stays the last row
    assert _abi.SIDE_LIBRARIES["tail"] == (_abi.TAIL_LIB_PATH, _abi.TAIL_ABI_VERSION, _abi.TAIL_PROTOTYPES)
    assert _abi.load_tail_library.args == ("tail",)
    # it compiles none of the shared cores: the sets of libraries that do stay as they are
    deps = build._side("tail")[1]
    assert not {os.path.basename(d) for d in deps} & {"mesh_core.h", "zbuffer_core.h", "depth_core.h", "pixel_color.h", "augment_warp.h"}
    assert "_abi.load_tail_library()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import pvnet_amd
    for name in ("TailParams", "fused_tail", "FusedTailNet"):
        assert getattr(pvnet_amd, name) is getattr(T, name) and name in pvnet_amd.__all__


def test_abi_version_and_constants_are_mirrored():
    defines = dict(re.findall(r"^#define\s+PVNET_TAIL_(\w+)\s+(\d+)u?\b", HDR, re.M))
    assert {k: int(v) for k, v in defines.items()} == dict(
        ABI_VERSION=_abi.TAIL_ABI_VERSION, WIDTH=_abi.TAIL_WIDTH, MAX_COUT=_abi.TAIL_MAX_COUT, T_F32=_abi.TAIL_T_F32, T_F16=_abi.TAIL_T_F16,
        T_BF16=_abi.TAIL_T_BF16, BF16=_abi.TAIL_BF16, F32=_abi.TAIL_F32, F_RAW=_abi.TAIL_F_RAW)
    decl = re.search(r"^int pvnet_tail_forward\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.TAIL_PROTOTYPES["pvnet_tail_forward"][1]
    assert len(decl) == len(args) == 23
    for k, (word, typ) in {0: ("const void* fm", C.c_void_p), 2: ("fm_strides[4]", _abi._i64p), 5: ("image_strides[4]", _abi._i64p),
                           6: ("const float* w1", C.c_void_p), 10: ("int b", C.c_int), 17: ("int cout", C.c_int),
                           18: ("int precision", C.c_int), 19: ("uint32_t flags", C.c_uint32), 20: ("void* out", C.c_void_p),
                           21: ("int out_type", C.c_int), 22: ("void* stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)


# ---- 2. bad arguments: every one rejected before any HIP call (there is no device here to answer one) ------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build_side("tail")
    return _abi.load_tail_library()


def test_library_holds_the_two_kernels(lib):
    blob = open(_abi.TAIL_LIB_PATH, "rb").read()
    assert b"tail_bf16_kernel" in blob and b"tail_f32_kernel" in blob
    asm = subprocess.run([build.hipcc_path()] + [f for f in build.flags() if f not in ("-shared", "-fPIC")] +
                         ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", os.path.join(build.CSRC, "tail.hip"), "-o", "-"],
                         capture_output=True, text=True, check=True).stdout

    def body(kernel):
        name = re.search(r"^(\S*%s\S*):" % kernel, asm, re.M).group(1)
        start = asm.index("\n" + name + ":")
        return asm[start:asm.index(".Lfunc_end", start)]

    # 18 + 2 k-steps of the 3 x 3 convolution and 2 of the 1 x 1 per 32 pixels, once in the code; the float32 tier has no matrix instruction
    assert len(re.findall(r"^\s*v_mfma_f32_32x32x16_bf16", body("tail_bf16_kernel"), re.M)) == 22
    assert "v_mfma" not in body("tail_f32_kernel") and re.search(r"v_fma(c)?_f32", body("tail_f32_kernel"))


def call(lib, **over):
    """pvnet_tail_forward on host buffers that a rejected call never touches"""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    s4 = (C.c_int64 * 4)(1, 1, 1, 1)
    a = dict(fm=p, fm_type=0, fm_strides=s4, image=p, image_type=0, image_strides=s4, w1=p, b1=p, w2=p, b2=p, b=1, hin=4, win=6, h=8, w=12,
             feat=32, raw=32, cout=20, precision=0, flags=0, out=p, out_type=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.pvnet_tail_forward(*a.values())


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    for name in ("fm", "fm_strides", "image", "image_strides", "w1", "b1", "w2", "b2", "out"):
        assert call(lib, **{name: None}) == BADARG, name
    for over in (dict(cout=0), dict(cout=33), dict(cout=-1), dict(b=0), dict(hin=0), dict(win=0), dict(h=0), dict(w=0), dict(feat=0), dict(raw=0),
                 dict(h=9), dict(h=7), dict(w=13), dict(w=6), dict(hin=8, h=8), dict(flags=2), dict(flags=0x80000000), dict(precision=2),
                 dict(precision=-1), dict(fm_type=3), dict(image_type=-1), dict(out_type=3), dict(flags=1, out_type=2), dict(flags=1, out_type=1)):
        assert call(lib, **over) == BADARG, over
    for over in (dict(feat=64), dict(raw=64), dict(feat=16), dict(raw=33), dict(b=65536), dict(hin=16385, h=32770), dict(win=16385, w=32770)):
        assert call(lib, **over) == UNSUPPORTED, over


# ---- 3. TailParams -----------------------------------------------------------------------------------------------------------------------
def modules(seed=0, cout=20, bias3=False, bias1=True, cin=35, width=32, slope=0.1):
    torch.manual_seed(seed)
    conv3, bn, act, conv1 = nn.Conv2d(cin, width, 3, 1, 1, bias=bias3), nn.BatchNorm2d(width), nn.LeakyReLU(slope, True), nn.Conv2d(width, cout, 1, 1, bias=bias1)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.3, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    return conv3, bn.eval(), act, conv1


def test_folding_against_torchs_own_eval_batchnorm_in_float64():
    conv3, bn, act, conv1 = modules()
    P = T.TailParams.from_modules(conv3, bn, conv1, act=act)
    assert P.cout == 20 and all(t.dtype == torch.float32 and t.is_contiguous() for t in (P.w1, P.b1, P.w2, P.b2))
    assert torch.equal(P.w2, conv1.weight.detach().view(20, 32)) and torch.equal(P.b2, conv1.bias.detach())
    x = torch.randn(2, 35, 9, 11, dtype=torch.float64)
    with torch.no_grad():
        want = bn.double()(conv3.double()(x))
        got = torch.nn.functional.conv2d(x, P.w1.double(), P.b1.double(), padding=1)
        # w1 and b1 are float64 values rounded once to float32: 2^-24 of every term
        lim = 2.0 ** -24 * (torch.nn.functional.conv2d(x.abs(), P.w1.double().abs(), P.b1.double().abs(), padding=1)) + 1e-14
    assert ((got - want).abs() <= lim).all()
    assert float((got - want).abs().max()) > 0   # (it IS rounded: not the float64 fold itself)


def test_refusals():
    conv3, bn, act, conv1 = modules()
    with pytest.raises(ValueError, match="eval"):
        T.TailParams.from_modules(conv3, modules()[1].train(), conv1)
    with pytest.raises(ValueError, match="LeakyReLU"):
        T.TailParams.from_modules(conv3, bn, conv1, act=nn.LeakyReLU(0.01))
    with pytest.raises(ValueError, match="LeakyReLU"):
        T.TailParams.from_modules(conv3, bn, conv1, act=nn.ReLU())
    with pytest.raises(ValueError, match="bias"):
        T.TailParams.from_modules(modules(bias3=True)[0], bn, conv1)
    with pytest.raises(ValueError, match="bias"):
        T.TailParams.from_modules(conv3, bn, modules(bias1=False)[3])
    c64 = modules(cin=67, width=64)
    with pytest.raises(ValueError, match="widths"):
        T.TailParams.from_modules(c64[0], c64[1], c64[3])
    with pytest.raises(ValueError, match="cout"):
        T.TailParams.from_modules(conv3, bn, modules(cout=33)[3])
    with pytest.raises(ValueError):
        T.TailParams.from_modules(nn.Conv2d(35, 32, 3, 1, 1, dilation=2, bias=False), bn, conv1)
    with pytest.raises(ValueError):
        T.TailParams(torch.zeros(64, 67, 3, 3), torch.zeros(64), torch.zeros(20, 64), torch.zeros(20))
    net, _ = TC.standin()
    with pytest.raises(ValueError, match="eval"):
        T.TailParams.from_network(net.train())
    with pytest.raises(RuntimeError):   # no CPU fallback
        T.fused_tail(torch.zeros(1, 32, 4, 4), torch.zeros(1, 3, 8, 8), T.TailParams.from_network(net.eval()))


class FlatTail(nn.Module):
    """the reference's spelling of the tail: `convraw` a flat Sequential of four"""

    def __init__(self, conv3, bn, act, conv1):
        super().__init__()
        self.convraw = nn.Sequential(conv3, bn, act, conv1)


def test_from_network_takes_both_spellings():
    conv3, bn, act, conv1 = modules(seed=3)
    flat = T.TailParams.from_network(FlatTail(conv3, bn, act, conv1))
    direct = T.TailParams.from_modules(conv3, bn, conv1, act=act)
    assert all(torch.equal(a, b) for a, b in zip((flat.w1, flat.b1, flat.w2, flat.b2), (direct.w1, direct.b1, direct.w2, direct.b2)))
    net, _ = TC.standin()
    nested = T.TailParams.from_network(net)
    body, last = net.convraw[0], net.convraw[1]
    direct = T.TailParams.from_modules(body[0], body[1], last, act=body[2])
    assert all(torch.equal(a, b) for a, b in zip((nested.w1, nested.b1, nested.w2, nested.b2), (direct.w1, direct.b1, direct.w2, direct.b2)))
    with pytest.raises(ValueError):
        T.TailParams.from_network(nn.Sequential())


# ---- 4. the restatement --------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_fixture_g9_under_the_fixtures_bar():
    fm, x, params, seg, ver = TC.g9()
    E = TR.forward_exact(fm, x, *params, "f32")
    y = torch.from_numpy(E["y"]).float()
    assert torch.allclose(y[:, :2], torch.from_numpy(seg), atol=1e-5, rtol=1e-5) and torch.allclose(y[:, 2:], torch.from_numpy(ver), atol=1e-5, rtol=1e-5)
    ref = np.concatenate([seg, ver], 1)
    assert np.abs(E["y"] - ref).max() < 1e-6
    # a simulation of the bfloat16 tier (its operands, float64 sums) stays under the a-priori bound
    bound, y32 = TR.bf16_bound(fm, x, *params)
    assert np.array_equal(y32, E["y"])
    sim = TR.forward_exact(fm, x, *params, "bf16")["y"]
    ratio = np.abs(sim - ref) / (bound + 1e-5 + 1e-5 * np.abs(ref))
    assert ratio.max() < 1 and ratio.max() > 0.01   # (not vacuous: the simulation uses a tenth of it)


def test_bf16_round_is_round_to_nearest_even():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 37
    x = torch.cat([x, torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, 256.0, 257.0, 3.0e38])])   # ties both ways among them
    assert np.array_equal(TR.bf16_round(x.numpy()), x.to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_restatements_upsample_against_torchs_float64_interpolation(shape):
    b, h, w = shape
    hin, win = h // 2, w // 2
    # a smooth positive field: the interpolated value has its operands' magnitude, so "4 ulps of the value" is a bar on the arithmetic
    yy, xx = torch.meshgrid(torch.arange(hin).double(), torch.arange(win).double(), indexing="ij")
    c = torch.arange(32).double()[:, None, None]
    fm = (4.0 + torch.sin(0.11 * xx + 0.3 * c) * torch.cos(0.07 * yy - 0.2 * c))[None].expand(b, 32, hin, win).float().contiguous()
    want = torch.nn.functional.interpolate(fm.double(), scale_factor=2, mode="bilinear", align_corners=True).numpy()
    got = TR.upsample(fm)
    assert got.shape == want.shape == (b, 32, h, w)
    assert (np.abs(got.astype(np.float64) - want) <= 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all()


def test_ramp_known_answer():
    for b, h, w in TC.SHAPES:
        fm, closed = TC.ramp(b, h // 2, w // 2)
        E = TR.forward_exact(fm, torch.zeros(b, 3, h, w), *TC.identity_weights(), "f32")
        assert (closed >= 0).all() and (np.abs(E["X"] - closed) <= 8 * TR.U32 * closed).all(), (b, h, w)
        assert np.array_equal(E["X"], TR.upsample(fm).astype(np.float64))   # identity weights: the raw output IS the upsampled operand


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_planted_mistakes_fail_the_stage_bars(precision):
    fm, image, (w1, b1, w2, b2) = TC.seeded(2, 40, 56, 20, seed=70)
    E = TR.forward_exact(fm, image, w1, b1, w2, b2, precision)
    lim1 = TR.bar1(E["A1"])
    # the bar can be met: the same operands summed in float32 by torch's own convolution
    In32, w32 = torch.from_numpy(E["In"]).float(), torch.from_numpy(E["w1"]).float()
    X32 = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(In32, w32, b1, padding=1), TR.SLOPE).double().numpy()
    assert (np.abs(X32 - E["X"]) <= lim1).all()
    for mistake in ("align_corners_false", "image_first", "taps_transposed", "slope_0.01", "pad_before_upsample"):
        Xm = TR.mistaken_raw(fm, image, w1, b1, precision, mistake)
        assert Xm.shape == E["X"].shape and (np.abs(Xm - E["X"]) > lim1).any(), mistake
    # the natural instead of the permuted k order of W2's fragment leaves stage 1 alone: it is stage 2's bar that must catch it
    y, A2 = TR.out_exact(E["Xq"], E["w2"], b2)
    ym, _ = TR.out_exact(E["Xq"], TR.swap_k_order(E["w2"]), b2)
    assert not np.array_equal(TR.swap_k_order(E["w2"]), E["w2"]) and np.array_equal(TR.swap_k_order(TR.swap_k_order(E["w2"])), E["w2"])
    assert (np.abs(ym - y) > TR.bar2(A2, y, torch.float32)).mean() > 0.9   # almost every output is wrong
    # ... and on the integer data it is not hidden either
    fi, ii, (wi1, bi1, wi2, bi2) = TC.integers(1, 32, 48, 20, seed=12, positive=True)
    Ei = TR.forward_exact(fi, ii, wi1, bi1, wi2, bi2, precision)
    assert (TR.out_exact(Ei["Xq"], TR.swap_k_order(Ei["w2"]), bi2)[0] != Ei["y"]).mean() > 0.9
