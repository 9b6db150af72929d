"""CPU-only checks of the fused trunk convolution (include/pvnet_trunk.h, libpvnet_trunk.so, pvnet_amd/trunk.py): the registry rows,
the header's constants against pvnet_amd/_abi.py, every bad argument rejected before any HIP call, ``ConvParams``' folding
of the BatchNorm against torch's own, its packing of the weights against the header's formula and its refusals, both attribute spellings
of a block (the reference's own class: tests/test_net_cpu.py), and the restatement (tests/trunk_restatement.py): against torch's
float64 ``F.conv2d``, against the reference's recorded trunk (tests/golden/trunk.npz), against one-hot weights, and against planted
mistakes, each of which the device tests' bar must catch.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from pvnet_amd import _abi, build  # noqa: E402
from pvnet_amd import trunk as T  # noqa: E402
from tests import trunk_cases as TC  # noqa: E402
from tests import trunk_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_trunk.h")).read()
FIXTURE = os.path.join(ROOT, "tests", "golden", "trunk.npz")
BADARG, UNSUPPORTED = -1, -3


# ---- 1. the registry rows and the ABI mirror -------------------------------------------------------------------------------------------
def test_registry_rows():
    assert build.SIDE_LIBRARIES["trunk"] == (["trunk.hip"], "pvnet_trunk.h", [])
    assert _abi.SIDE_LIBRARIES["trunk"] == (_abi.TRUNK_LIB_PATH, _abi.TRUNK_ABI_VERSION, _abi.TRUNK_PROTOTYPES)
    assert _abi.load_trunk_library.args == ("trunk",)
    deps = build._side("trunk")[1]
    assert not {os.path.basename(d) for d in deps} & {"mesh_core.h", "zbuffer_core.h", "depth_core.h", "pixel_color.h", "augment_warp.h"}
    assert "_abi.load_trunk_library()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import pvnet_amd
    for name in ("ConvParams", "fused_conv3x3", "FusedBasicBlock", "FusedTrunkNet"):
        assert getattr(pvnet_amd, name) is getattr(T, name) and name in pvnet_amd.__all__


def test_abi_version_and_constants_are_mirrored():
    defines = dict(re.findall(r"^#define\s+PVNET_TRUNK_(\w+)\s+(\d+)u?\b", HDR, re.M))
    assert {k: int(v) for k, v in defines.items()} == dict(
        ABI_VERSION=_abi.TRUNK_ABI_VERSION, MAX_WIDTH=_abi.TRUNK_MAX_WIDTH, CO_GROUP=_abi.TRUNK_CO_GROUP, T_F32=_abi.TRUNK_T_F32,
        T_F16=_abi.TRUNK_T_F16, T_BF16=_abi.TRUNK_T_BF16, ACT_NONE=_abi.TRUNK_ACT_NONE, ACT_RELU=_abi.TRUNK_ACT_RELU,
        ACT_LEAKY=_abi.TRUNK_ACT_LEAKY)
    assert (_abi.TRUNK_T_F32, _abi.TRUNK_T_F16, _abi.TRUNK_T_BF16) == (_abi.DECODER_T_F32, _abi.DECODER_T_F16, _abi.DECODER_T_BF16)
    assert list(_abi.TRUNK_GEOMETRIES) == TC.GEOMETRIES and T.ACTS == dict(none=0, relu=1, leaky=2) and tuple(T.ACTS) == R.ACTS
    decl = re.search(r"^int pvnet_conv3x3_fused\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.TRUNK_PROTOTYPES["pvnet_conv3x3_fused"][1]
    assert len(decl) == len(args) == 23
    for k, (word, typ) in {0: ("const void* src1", C.c_void_p), 1: ("int src1_type", C.c_int), 2: ("src1_strides[4]", _abi._i64p),
                           3: ("const void* src2", C.c_void_p), 5: ("src2_strides[4]", _abi._i64p), 6: ("const void* res", C.c_void_p),
                           8: ("res_strides[4]", _abi._i64p), 9: ("const void* w", C.c_void_p), 10: ("const float* bias", C.c_void_p),
                           11: ("int b", C.c_int), 14: ("int c1", C.c_int), 15: ("int c2", C.c_int), 16: ("int co", C.c_int),
                           17: ("int stride", C.c_int), 18: ("int dilation", C.c_int), 19: ("int act", C.c_int),
                           20: ("void* out", C.c_void_p), 21: ("int out_type", C.c_int), 22: ("void* stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)


# ---- 2. the library and its bad arguments: every one rejected before any HIP call (there is no device here to answer one) -----------------
@pytest.fixture(scope="module")
def lib():
    build.build_side("trunk")
    return _abi.load_trunk_library()


def test_library_holds_a_kernel_per_geometry(lib):
    assert lib.pvnet_trunk_abi_version() == _abi.TRUNK_ABI_VERSION
    asm = subprocess.run([build.hipcc_path()] + [f for f in build.flags() if f not in ("-shared", "-fPIC")] +
                         ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", os.path.join(build.CSRC, "trunk.hip"), "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S*conv3x3_kernel\S*)", asm, re.M)
    assert sorted(re.search(r"ILi(\d)ELi(\d)E", k).groups() for k in kernels) == sorted((str(s), str(d)) for s, d in TC.GEOMETRIES)
    for name in kernels:
        start = asm.index("\n" + name + ":")
        body = asm[start:asm.index(".Lfunc_end", start)]
        s, d = map(int, re.search(r"ILi(\d)ELi(\d)E", name).groups())
        # a row of taps is six k-steps x eight pixel rows of the tile, and the loop over the three rows is not unrolled
        assert len(re.findall(r"^\s*v_mfma_f32_32x32x16_bf16", body, re.M)) == 48, name
        assert "v_mfma_f32_32x32x2" not in body and not re.search(r"^\s*(scratch_|buffer_(load|store).*offen)", body, re.M), name
        desc = asm[asm.index(".amdhsa_kernel " + name):]
        field = (31 * s + 2 * d + 1) * (7 * s + 2 * d + 1) * 80   # the header's receptive field in 80-byte records
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) == field <= 160 * 1024 // (1 if s == 2 else 2)


def call(lib, **over):
    """pvnet_conv3x3_fused on host buffers that a rejected call never touches"""
    buf = (C.c_char * 64)()
    p = C.c_void_p(C.addressof(buf) + 16 - C.addressof(buf) % 16)
    s4 = (C.c_int64 * 4)(1, 1, 1, 1)
    a = dict(src1=p, src1_type=0, src1_strides=s4, src2=None, src2_type=0, src2_strides=None, res=None, res_type=0, res_strides=None, w=p,
             bias=p, b=1, h=4, w_=6, c1=64, c2=0, co=32, stride=1, dilation=1, act=0, out=p, out_type=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.pvnet_conv3x3_fused(*a.values()), p, s4


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    _, p, s4 = call(lib, b=0)
    for name in ("src1", "src1_strides", "w", "bias", "out"):
        assert call(lib, **{name: None})[0] == BADARG, name
    for over in (dict(b=0), dict(h=0), dict(w_=0), dict(c1=0), dict(c2=-32), dict(co=0), dict(co=-32), dict(stride=0), dict(dilation=0),
                 dict(dilation=-1), dict(act=3), dict(act=-1), dict(src1_type=3), dict(out_type=-1),
                 dict(c2=32), dict(src2=p, src2_strides=s4), dict(src2=p, c2=32), dict(src2=p, src2_strides=s4, c2=32, src2_type=3),
                 dict(res=p), dict(res=p, res_strides=s4, res_type=5)):
        assert call(lib, **over)[0] == BADARG, over
    assert call(lib, w=C.c_void_p(p.value + 2))[0] == BADARG   # the fragments are taken with 16-byte loads
    # widths that are no multiples of 32 or beyond 512 (the Bottleneck's), and every other stride and dilation
    for over in (dict(c1=48), dict(c1=544), dict(co=48), dict(co=1024), dict(co=2048), dict(c1=512, c2=32, src2=p, src2_strides=s4),
                 dict(c1=32, c2=16, src2=p, src2_strides=s4), dict(stride=2, dilation=2), dict(stride=3), dict(dilation=3), dict(dilation=8),
                 dict(stride=2, dilation=4), dict(b=65536), dict(h=32769), dict(w_=32769)):
        assert call(lib, **over)[0] == UNSUPPORTED, over


# ---- 3. ConvParams ---------------------------------------------------------------------------------------------------------------------------
def modules(seed=0, cin=64, cout=96, stride=1, dilation=2, bias=False, act=None, **conv):
    torch.manual_seed(seed)
    kw = dict(kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=bias)
    kw.update(conv)
    c, bn = nn.Conv2d(cin, cout, **kw), nn.BatchNorm2d(cout)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.2)
    bn.eval()
    return c, bn, act


@pytest.mark.parametrize("geometry", TC.GEOMETRIES)
def test_folding_against_torchs_own_eval_batchnorm_in_float64(geometry):
    s, d = geometry
    conv, bn, _ = modules(seed=3, stride=s, dilation=d)
    P = T.ConvParams.from_modules(conv, bn, nn.ReLU())
    assert (P.cin, P.co, P.stride, P.dilation, P.act) == (64, 96, s, d, "relu") and P.w.dtype == P.bias.dtype == torch.float32
    x = torch.randn(2, 64, 11, 13, dtype=torch.float64)
    with torch.no_grad():
        want = torch.relu(bn.double()(conv.double()(x)))
        got = torch.relu(F.conv2d(x, P.w.double(), P.bias.double(), s, d, d))
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-6)    # the folded weights are float32 roundings of the float64 ones
    assert T.ConvParams.from_modules(conv, bn).act == "none" and T.ConvParams.from_modules(conv, bn, nn.LeakyReLU(0.1)).act == "leaky"


@pytest.mark.parametrize("triple", [(32, 0, 32), (64, 32, 96)])
def test_packed_weights_are_the_headers_fragment_order(triple):
    c1, c2, co = triple
    cin = c1 + c2
    w = torch.randn(co, cin, 3, 3, generator=torch.Generator().manual_seed(9))
    P = T.ConvParams(w, torch.zeros(co))
    flat, wq = P.packed.reshape(-1), w.to(torch.bfloat16)
    assert P.packed.dtype == torch.bfloat16 and flat.numel() == co * cin * 9 and tuple(P.packed.shape) == (cin // 32, 9, 2, co // 32, 64, 8)
    # the header's formula, element by element
    idx = torch.arange(flat.numel())
    j, lane, m = idx % 8, idx // 8 % 64, idx // 512 % (co // 32)
    rest = idx // (512 * (co // 32))
    half, tap, chunk = rest % 2, rest // 2 % 9, rest // 18
    want = wq[32 * m + (lane & 31), 32 * chunk + 16 * half + 8 * (lane >> 5) + j, tap // 3, tap % 3]
    assert torch.equal(flat, want)


def test_refusals():
    ok = modules()
    T.ConvParams.from_modules(*ok)
    conv, bn, _ = modules()
    bn.train()
    with pytest.raises(ValueError, match="eval"):
        T.ConvParams.from_modules(conv, bn)
    for kw, match in ((dict(bias=True), "no bias"), (dict(kernel_size=1, padding=0, dilation=1), "expected Conv2d"),
                      (dict(kernel_size=5, padding=2, dilation=1), "expected Conv2d"), (dict(padding=1), "padding must be the dilation"),
                      (dict(groups=2), "expected Conv2d"), (dict(padding_mode="reflect"), "expected Conv2d"),
                      (dict(stride=(1, 2)), "padding must be the dilation"), (dict(stride=2), "stride, dilation"),
                      (dict(dilation=3, padding=3), "stride, dilation")):
        conv, bn, _ = modules(**kw)
        with pytest.raises(ValueError, match=match):
            T.ConvParams.from_modules(conv, bn)
    for cin, cout in ((48, 64), (64, 48), (1024, 64), (64, 2048)):
        conv, bn, _ = modules(cin=cin, cout=cout)
        with pytest.raises(ValueError, match="multiples of 32"):
            T.ConvParams.from_modules(conv, bn)
    conv, bn, _ = modules()
    for act in (nn.LeakyReLU(0.01), nn.Sigmoid(), "gelu"):
        with pytest.raises(ValueError, match="LeakyReLU|activation"):
            T.ConvParams.from_modules(conv, bn, act)
    with pytest.raises(ValueError):
        T.ConvParams(torch.zeros(32, 32, 3, 3), torch.zeros(31))
    with pytest.raises(RuntimeError):   # no CPU fallback
        T.fused_conv3x3(torch.zeros(1, 64, 4, 4), T.ConvParams.from_modules(*ok[:2]))


# ---- 4. the two spellings of a block (the network class: tests/test_net_cpu.py) ------------------------------------------------------------
def test_fused_basic_block_reads_both_spellings_and_refuses_the_rest():
    net = TC.standin()
    blk = T.FusedBasicBlock(net.l2[0])   # the stand-in's: c1, b1, c2, b2, down
    assert (blk.conv1.cin, blk.conv1.co, blk.conv1.stride, blk.conv1.act) == (64, 128, 2, "relu") and blk.down is not None
    assert (blk.conv2.cin, blk.conv2.co, blk.conv2.stride, blk.conv2.act) == (128, 128, 1, "relu")

    class Ref(nn.Module):                # the reference's: conv1, bn1, conv2, bn2, downsample
        def __init__(self, b):
            super().__init__()
            self.conv1, self.bn1, self.conv2, self.bn2, self.downsample, self.relu = b.c1, b.b1, b.c2, b.b2, b.down, nn.ReLU()

    other = T.FusedBasicBlock(Ref(net.l2[0]))
    assert torch.equal(other.conv1.packed, blk.conv1.packed) and torch.equal(other.conv2.w, blk.conv2.w) and torch.equal(other.down[0], blk.down[0])
    # the folded downsample is the module's own, in float64 up to float32's rounding of the folded weights
    x = torch.relu(torch.randn(1, 64, 9, 12))
    with torch.no_grad():
        want = _downsample64(net.l2[0].down, x.double())
    assert torch.allclose(blk.residual(x).double(), want, atol=1e-5, rtol=1e-5) and blk.residual(x).shape == (1, 128, 5, 6)
    plain = T.FusedBasicBlock(net.l4[1])
    assert plain.down is None and plain.residual(x) is x and plain.conv1.dilation == plain.conv2.dilation == 4
    with pytest.raises(ValueError, match="neither"):
        T.FusedBasicBlock(nn.Sequential())
    bottleneck = Ref(net.l1[0])
    bottleneck.conv3 = nn.Conv2d(64, 256, 1)
    with pytest.raises(ValueError, match="neither"):
        T.FusedBasicBlock(bottleneck)


# ---- 5. the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", TC.GEOMETRIES, ids=[f"s{s}d{d}" for s, d in TC.GEOMETRIES])
def test_restatement_against_torchs_float64_conv2d_at_every_geometry_and_shape(geometry):
    s, d = geometry
    for k, shape in enumerate(TC.SHAPES):
        for triple, act in zip(TC.SMALL_TRIPLES, R.ACTS):
            src1, src2, res, (w, bias) = TC.seeded(*shape, triple, s, seed=60 + k, even=shape[0] == 3)
            src1, w = src1.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()       # the operands rounded to bfloat16 first
            src2 = None if src2 is None else src2.to(torch.bfloat16).float()
            res = res - 0.5
            In = src1 if src2 is None else torch.cat([src1, src2], 1)
            with torch.no_grad():
                pre = F.conv2d(In.double(), w.double(), bias.double(), stride=s, padding=d, dilation=d) + res.double()
                want = {"none": pre, "relu": torch.relu(pre), "leaky": F.leaky_relu(pre, R.SLOPE)}[act].numpy()
            E = R.conv_exact(src1, w, bias, s, d, act, src2=src2, res=res)
            assert E["out"].shape == want.shape == (shape[0], triple[2], shape[1], shape[2])
            assert np.allclose(E["out"], want, atol=1e-12, rtol=1e-12), (shape, triple)
            assert np.array_equal(E["In"], In.double().numpy()) and (E["A"] >= np.abs(E["pre"]) - 1e-12).all()
            # unrounded operands: the same function of the operands as given
            assert np.array_equal(R.conv_exact(src1, w, bias, s, d, act, src2=src2, res=res, rounded=False)["out"], E["out"])


def test_restatement_under_one_hot_weights_is_the_shifted_rounded_operand():
    for s, d in TC.GEOMETRIES:
        for triple in TC.SMALL_TRIPLES[:2]:
            taps, w, bias = TC.onehot(triple, seed=5)
            for k, shape in enumerate(TC.SHAPES):
                src1, src2, _, _ = TC.seeded(*shape, triple, s, seed=100 + k, even=shape[0] == 3)
                src1 = src1 - 0.3
                want = R.onehot_expected(R.bf16_round(R.concat(src1, src2)), taps, s, d)
                assert np.array_equal(R.conv_exact(src1, w, bias, s, d, "none", src2=src2)["out"], want.astype(np.float64))


def test_integer_data_is_integral_with_every_partial_sum_exact():
    for s, d in TC.GEOMETRIES:
        src1, src2, res, (w, bias) = TC.integers(*TC.SHAPES[2], TC.SMALL_TRIPLES[1], s, seed=20)
        E = R.conv_exact(src1, w, bias, s, d, "relu", src2=src2, res=res)
        assert np.array_equal(E["In"], R.concat(src1, src2)) and np.array_equal(E["w"], w.numpy())   # bfloat16 holds them
        assert np.array_equal(E["out"], np.round(E["out"])) and (E["pre"] > 0).all() and E["A"].max() < 2 ** 22


def _downsample64(seq, x):
    """the 1 x 1 downsample (Conv2d, BatchNorm2d in eval()) of a block in float64"""
    conv, bn = seq
    y = F.conv2d(x, conv.weight.double(), None, conv.stride)
    g = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return y * g[None, :, None, None] + (bn.bias.double() - bn.running_mean.double() * g)[None, :, None, None]


def _layer64(blocks, x):
    """a layer of the stand-in through the UNROUNDED restatement, block by block: float64 numpy in, float64 numpy out"""
    for blk in blocks:
        f = T.FusedBasicBlock(blk)
        p1, p2 = f.conv1, f.conv2
        with torch.no_grad():
            res = x if blk.down is None else _downsample64(blk.down, torch.from_numpy(x)).numpy()
        y = R.conv_exact(x, p1.w, p1.bias, p1.stride, p1.dilation, "relu", rounded=False)["out"]
        x = R.conv_exact(y, p2.w, p2.bias, 1, p2.dilation, "relu", res=res, rounded=False)["out"]
    return x


def test_unrounded_restatement_meets_the_references_recorded_trunk():
    """tests/golden/trunk.npz: the reference's own Resnet18_8s with the seeded stand-in's weights.  Every piece, fed the RECORDED input
    of that piece, meets its recorded output within the stem fixture's 1e-5 -- the restatement's strides, dilations, residuals, the
    order of conv8s' two sources and the folding are the reference's."""
    g = np.load(FIXTURE)
    net = TC.standin()
    f64 = lambda k: g[k].astype(np.float64)   # noqa: E731
    assert g["pooled"].shape == (1, 64, 16, 22) and g["x32s"].shape == (1, 512, 8, 11) and g["pooled"].dtype == np.float32
    for k, (layer, src, dst) in enumerate(((net.l1, "pooled", "x4s"), (net.l2, "x4s", "x8s"), (net.l3, "x8s", "x16s"), (net.l4, "x16s", "x32s"))):
        got = _layer64(layer, f64(src))
        assert got.shape == g[dst].shape and np.allclose(got, g[dst], atol=1e-5, rtol=1e-5), dst
    P = T.ConvParams.from_modules(*net.fc)
    got = R.conv_exact(f64("x32s"), P.w, P.bias, 1, 1, P.act, rounded=False)["out"]
    assert P.act == "relu" and np.allclose(got, g["xfc"], atol=1e-5, rtol=1e-5)
    P = T.ConvParams.from_modules(*net.conv8s)
    got = R.conv_exact(f64("xfc"), P.w, P.bias, 1, 1, P.act, src2=f64("x8s"), rounded=False)["out"]
    assert P.act == "leaky" and (g["conv8s"] < 0).any() and np.allclose(got, g["conv8s"], atol=1e-5, rtol=1e-5)
    # ... and the other order of the two sources does not
    swapped = R.conv_exact(f64("xfc"), P.w[:, list(range(256, 384)) + list(range(256))], P.bias, 1, 1, P.act, src2=f64("x8s"), rounded=False)
    assert not np.allclose(swapped["out"], g["conv8s"], atol=1e-3, rtol=1e-3)


# (mistake, geometry, activation): each at a geometry where it is a mistake at all
PLANTED = [("dilation_on_padding_only", (1, 2), "relu"), ("dilation_on_padding_only", (1, 4), "relu"), ("origin_2Y", (2, 1), "relu"),
           ("residual_after_act", (1, 1), "relu"), ("taps_transposed", (1, 2), "none"), ("src2_first", (1, 1), "leaky"),
           ("relu_for_leaky", (1, 4), "leaky")]


@pytest.mark.parametrize("mistake,geometry,act", PLANTED, ids=[f"{m}-s{g[0]}d{g[1]}" for m, g, _ in PLANTED])
def test_planted_mistakes_fail_the_device_tests_bar(mistake, geometry, act):
    assert {m for m, _, _ in PLANTED} == set(R.MISTAKES) and len(R.MISTAKES) == 6
    s, d = geometry
    triple = (32, 32, 160) if mistake == "src2_first" else TC.SMALL_TRIPLES[1]   # (equal widths: the swapped concatenation has In's shape)
    for k, shape in enumerate((TC.SHAPES[2], TC.SHAPES[3])):
        src1, src2, res, (w, bias) = TC.seeded(*shape, triple, s, seed=80 + k)
        res = res - 0.5
        E = R.conv_exact(src1, w, bias, s, d, act, src2=src2, res=res)
        got = R.mistaken(src1, w, bias, s, d, act, mistake, src2=src2, res=res)
        lim = R.bar(E["A"], triple[0] + triple[1], E["out"], torch.bfloat16)   # the widest bar the device tests apply
        assert got.shape == E["out"].shape and (np.abs(got - E["out"]) > lim).any(), (mistake, shape)
    # and without the mistake the same route is the restatement
    assert mistake in R.MISTAKES
