"""CPU-only checks of the fused decoder stages (include/pvnet_decoder.h, libpvnet_decoder.so, pvnet_amd/decoder.py): the registry rows
and their place, the header's constants against pvnet_amd/_abi.py, every bad argument rejected before any HIP call, ``StageParams``'
folding of the BatchNorm against torch's own, its packing of the weights against the header's formula and its refusals (the network
class: tests/test_net_cpu.py), and the restatement (tests/decoder_restatement.py): against torch's float64 composition of the real
modules, against one-hot weights, and against planted mistakes, each of which the comparison's bar must catch.
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
from pvnet_amd import decoder as D  # noqa: E402
from tests import decoder_cases as DC  # noqa: E402
from tests import decoder_restatement as DR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_decoder.h")).read()
BADARG, UNSUPPORTED = -1, -3


# ---- 1. the registry rows and the ABI mirror -------------------------------------------------------------------------------------------
def test_registry_rows_and_their_place():
    assert build.SIDE_LIBRARIES["decoder"] == (["decoder.hip"], "pvnet_decoder.h", [])
    for table in (build.SIDE_LIBRARIES, _abi.SIDE_LIBRARIES):
        names = list(table)
        assert names.index("decoder") == names.index("tail") - 1   # beside the tail, the same position in both
    assert _abi.SIDE_LIBRARIES["decoder"] == (_abi.DECODER_LIB_PATH, _abi.DECODER_ABI_VERSION, _abi.DECODER_PROTOTYPES)
    assert _abi.load_decoder_library.args == ("decoder",)
    deps = build._side("decoder")[1]
    assert not {os.path.basename(d) for d in deps} & {"mesh_core.h", "zbuffer_core.h", "depth_core.h", "pixel_color.h", "augment_warp.h"}
    assert "_abi.load_decoder_library()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import pvnet_amd
    for name in ("StageParams", "fused_stage", "FusedDecoderNet"):
        assert getattr(pvnet_amd, name) is getattr(D, name) and name in pvnet_amd.__all__


def test_abi_version_and_constants_are_mirrored():
    defines = dict(re.findall(r"^#define\s+PVNET_DECODER_(\w+)\s+(\d+)u?\b", HDR, re.M))
    assert {k: int(v) for k, v in defines.items()} == dict(
        ABI_VERSION=_abi.DECODER_ABI_VERSION, SKIP=_abi.DECODER_SKIP, T_F32=_abi.DECODER_T_F32, T_F16=_abi.DECODER_T_F16,
        T_BF16=_abi.DECODER_T_BF16, F_PACKED=_abi.DECODER_F_PACKED)
    assert (_abi.DECODER_T_F32, _abi.DECODER_T_F16, _abi.DECODER_T_BF16) == (_abi.TAIL_T_F32, _abi.TAIL_T_F16, _abi.TAIL_T_BF16)
    assert list(_abi.DECODER_SHAPES) == DC.TRIPLES and all(cs == _abi.DECODER_SKIP for _, cs, _ in DC.TRIPLES)
    decl = re.search(r"^int pvnet_decoder_stage\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.DECODER_PROTOTYPES["pvnet_decoder_stage"][1]
    assert len(decl) == len(args) == 20
    for k, (word, typ) in {0: ("const void* lo", C.c_void_p), 1: ("int lo_type", C.c_int), 2: ("lo_strides[4]", _abi._i64p),
                           3: ("const void* skip", C.c_void_p), 5: ("skip_strides[4]", _abi._i64p), 6: ("const float* w", C.c_void_p),
                           7: ("const float* bias", C.c_void_p), 8: ("int b", C.c_int), 13: ("int cl", C.c_int), 15: ("int co", C.c_int),
                           16: ("uint32_t flags", C.c_uint32), 17: ("void* out", C.c_void_p), 18: ("int out_type", C.c_int),
                           19: ("void* stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)


# ---- 2. the library and its bad arguments: every one rejected before any HIP call (there is no device here to answer one) -----------------
@pytest.fixture(scope="module")
def lib():
    build.build_side("decoder")
    return _abi.load_decoder_library()


def test_library_holds_a_kernel_per_shape_and_weight_layout(lib):
    blob = open(_abi.DECODER_LIB_PATH, "rb").read()
    assert b"decoder_stage_kernel" in blob
    asm = subprocess.run([build.hipcc_path()] + [f for f in build.flags() if f not in ("-shared", "-fPIC")] +
                         ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", os.path.join(build.CSRC, "decoder.hip"), "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S*decoder_stage_kernel\S*)", asm, re.M)
    assert len(kernels) == 4 == len(set(kernels))   # (64, 32) and (128, 64), packed weights or float32
    for name in kernels:
        start = asm.index("\n" + name + ":")
        body = asm[start:asm.index(".Lfunc_end", start)]
        co, packed = int(re.search(r"ILi\d+ELi(\d+)ELb([01])", name).group(1)), "ELb1E" in name
        # a k-step is co / 32 row blocks x 2 column blocks; the packed kernels unroll a chunk's eighteen, the others loop over them
        assert len(re.findall(r"^\s*v_mfma_f32_32x32x16_bf16", body, re.M)) == (18 if packed else 1) * 2 * co // 32, name
        assert "v_mfma_f32_32x32x2" not in body and not re.search(r"^\s*(scratch_|buffer_(load|store).*offen)", body, re.M), name
        desc = asm[asm.index(".amdhsa_kernel " + name):]
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) <= 64 * 1024   # static LDS


def call(lib, **over):
    """pvnet_decoder_stage on host buffers that a rejected call never touches"""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    s4 = (C.c_int64 * 4)(1, 1, 1, 1)
    a = dict(lo=p, lo_type=0, lo_strides=s4, skip=p, skip_type=0, skip_strides=s4, w=p, bias=p, b=1, hin=4, win=6, h=8, w_=12, cl=64, cs=64, co=32,
             flags=0, out=p, out_type=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.pvnet_decoder_stage(*a.values())


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    for name in ("lo", "lo_strides", "skip", "skip_strides", "w", "bias", "out"):
        assert call(lib, **{name: None}) == BADARG, name
    for over in (dict(b=0), dict(hin=0), dict(win=0), dict(h=0), dict(w_=0), dict(cl=0), dict(cs=0), dict(co=0), dict(co=-32), dict(h=9), dict(h=7),
                 dict(w_=13), dict(w_=6), dict(hin=8, h=8), dict(flags=2), dict(flags=3), dict(flags=0x80000000), dict(lo_type=3), dict(skip_type=-1),
                 dict(out_type=3), dict(cl=128, co=64, h=9)):
        assert call(lib, **over) == BADARG, over
    buf = (C.c_char * 64)()
    odd = C.c_void_p(C.addressof(buf) + 16 - C.addressof(buf) % 16 + 2)   # packed weights are taken with 16-byte loads
    assert call(lib, flags=1, w=odd) == BADARG
    # the two triples only: the Resnet50_8s widths and every mixture of the two supported ones
    for over in (dict(cl=128), dict(co=64), dict(cs=32), dict(cl=64, cs=64, co=64), dict(cl=128, cs=64, co=32), dict(cl=256, cs=256, co=128),
                 dict(cl=512, cs=128, co=256), dict(cl=32, co=32), dict(b=65536), dict(hin=16385, h=32770), dict(win=16385, w_=32770),
                 dict(cl=128, co=64, b=65536)):
        assert call(lib, **over) == UNSUPPORTED, over


# ---- 3. StageParams ----------------------------------------------------------------------------------------------------------------------
def modules(seed=0, cin=128, cout=32, bias=False, slope=0.1, **conv):
    torch.manual_seed(seed)
    conv3 = nn.Conv2d(cin, cout, 3, bias=bias, **{**dict(stride=1, padding=1), **conv})
    bn, act = nn.BatchNorm2d(cout), nn.LeakyReLU(slope, True)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.3, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    return conv3, bn.eval(), act


@pytest.mark.parametrize("triple", DC.TRIPLES)
def test_folding_against_torchs_own_eval_batchnorm_in_float64(triple):
    cl, cs, co = triple
    conv3, bn, act = modules(cin=cl + cs, cout=co)
    P = D.StageParams.from_modules(conv3, bn, act=act)
    assert (P.cl, P.cs, P.co) == triple and all(t.dtype == torch.float32 and t.is_contiguous() for t in (P.w, P.bias))
    x = torch.randn(2, cl + cs, 9, 11, dtype=torch.float64)
    with torch.no_grad():
        want = bn.double()(conv3.double()(x))
        got = torch.nn.functional.conv2d(x, P.w.double(), P.bias.double(), padding=1)
        # w and bias are float64 values rounded once to float32: 2^-24 of every term
        lim = 2.0 ** -24 * (torch.nn.functional.conv2d(x.abs(), P.w.double().abs(), P.bias.double().abs(), padding=1)) + 1e-14
    assert ((got - want).abs() <= lim).all()
    assert float((got - want).abs().max()) > 0   # (it IS rounded: not the float64 fold itself)


@pytest.mark.parametrize("triple", DC.TRIPLES)
def test_packed_weights_are_the_headers_fragment_order(triple):
    cl, cs, co = triple
    w = DC.seeded(1, 2, 2, triple, seed=5)[2][0]
    P = D.StageParams(w, torch.zeros(co))
    pk = P.packed
    assert pk.dtype == torch.bfloat16 and pk.is_contiguous() and pk.numel() == w.numel()
    assert tuple(pk.shape) == ((cl + cs) // 32, 9, 2, co // 32, 64, 8)
    # the header's formula, element by element, in numpy
    chunk, tap, half, m, lane, j = np.meshgrid(*[np.arange(n) for n in pk.shape], indexing="ij")
    want = DR.bf16_round(w.numpy())[32 * m + (lane & 31), 32 * chunk + 16 * half + 8 * (lane >> 5) + j, tap // 3, tap % 3]
    assert np.array_equal(pk.float().numpy(), want)
    flat = ((((chunk * 9 + tap) * 2 + half) * (co // 32) + m) * 64 + lane) * 8 + j
    assert np.array_equal(flat.ravel(), np.arange(pk.numel()))   # and that IS the contiguous order


def test_refusals():
    conv3, bn, act = modules()
    with pytest.raises(ValueError, match="eval"):
        D.StageParams.from_modules(conv3, modules()[1].train())
    nostats = nn.BatchNorm2d(32, track_running_stats=False).eval()
    with pytest.raises(ValueError, match="running statistics"):
        D.StageParams.from_modules(conv3, nostats)
    with pytest.raises(ValueError, match="LeakyReLU"):
        D.StageParams.from_modules(conv3, bn, act=nn.LeakyReLU(0.01))
    with pytest.raises(ValueError, match="LeakyReLU"):
        D.StageParams.from_modules(conv3, bn, act=nn.ReLU())
    with pytest.raises(ValueError, match="bias"):
        D.StageParams.from_modules(modules(bias=True)[0], bn)
    for cin, cout in ((128, 64), (192, 32), (512 + 128, 256), (35, 32), (96, 32)):   # mixtures, Resnet50_8s, the tail's
        c, n, _ = modules(cin=cin, cout=cout)
        with pytest.raises(ValueError, match="widths"):
            D.StageParams.from_modules(c, n)
    for odd in (dict(dilation=2), dict(stride=2), dict(groups=2), dict(padding_mode="reflect")):
        with pytest.raises(ValueError):
            D.StageParams.from_modules(modules(**odd)[0], bn)
    with pytest.raises(ValueError):
        D.StageParams(torch.zeros(64, 128, 3, 3), torch.zeros(64))
    with pytest.raises(ValueError):
        D.StageParams(torch.zeros(32, 128, 3, 3), torch.zeros(31))
    with pytest.raises(ValueError):
        D.StageParams(torch.zeros(32, 128, 1, 1), torch.zeros(32))
    net, _ = DC.standin()
    with pytest.raises(ValueError, match="eval"):
        D.StageParams.from_network(net.train(), "conv2s")
    net.eval()
    with pytest.raises(ValueError, match="stage"):
        D.StageParams.from_network(net, "conv8s")
    with pytest.raises(ValueError):
        D.StageParams.from_network(nn.Sequential(), "conv2s")
    with pytest.raises(RuntimeError):   # no CPU fallback
        D.fused_stage(torch.zeros(1, 64, 4, 4), torch.zeros(1, 64, 8, 8), D.StageParams.from_network(net, "conv2s"))


def test_from_network_reads_the_reference_attribute_names():
    net, _ = DC.standin()
    for triple in DC.TRIPLES:
        stage = DC.STAGE_OF[triple]
        P = D.StageParams.from_network(net, stage)
        seq = getattr(net, stage)
        Q = D.StageParams.from_modules(seq[0], seq[1], act=seq[2])
        assert (P.cl, P.cs, P.co) == triple and torch.equal(P.w, Q.w) and torch.equal(P.bias, Q.bias) and torch.equal(P.packed, Q.packed)


# ---- 4. the restatement --------------------------------------------------------------------------------------------------------------------
def composition(lo, skip, w, bias):
    """torch's float64 composition of the REAL modules on the given operands: nn.UpsamplingBilinear2d, torch.cat, F.conv2d, LeakyReLU ->
    (the output, the concatenated In, what the float32 upsample may differ from the float64 one by, per upsampled element)"""
    up = nn.UpsamplingBilinear2d(scale_factor=2)
    with torch.no_grad():
        In = torch.cat([up(lo.double()), skip.double()], 1)
        pre = torch.nn.functional.conv2d(In, w.double(), bias.double(), padding=1)
        # the header's float32 source coordinate fl(Y * fl(r)) is off by at most 2 u32 n (n = max(hin, win) bounds it), which moves the
        # value by that times a difference of neighbours (<= 2 max |lo[c]|), in each direction; the six roundings of the products and
        # sums add at most 8 u32 of the largest neighbour
        n = max(lo.shape[2:])
        f32_slack = (8 + 8 * n) * DR.U32 * lo.double().abs().amax((2, 3), keepdim=True).expand_as(In[:, :lo.shape[1]])
        return nn.LeakyReLU(0.1)(pre).numpy(), In.numpy(), f32_slack.numpy()


def composition_bar(In64, f32_slack, w, cl):
    """What separates the restatement from that composition when lo, skip and w are bfloat16 values already: the float32 arithmetic of
    the upsample (see `composition`) and then the one rounding of every UPSAMPLED operand to bfloat16 (at most 2^-8 of it).  skip's and
    the weights' roundings change nothing, and the sums are float64 on both sides."""
    per_operand = DR.U_BF16 * np.abs(In64[:, :cl]) + (1 + DR.U_BF16) * f32_slack
    return torch.nn.functional.conv2d(torch.from_numpy(per_operand), torch.from_numpy(np.abs(w[:, :cl])), padding=1).numpy() + 1e-12


@pytest.mark.parametrize("triple", DC.TRIPLES)
def test_restatement_against_torchs_float64_composition_and_planted_mistakes(triple):
    cl, cs, co = triple
    lo, skip, (w, bias) = DC.seeded(2, 40, 56, triple, seed=70)
    lo, skip, w = (t.to(torch.bfloat16).float() for t in (lo, skip, w))   # the operands rounded to bfloat16 first
    want, In64, slack = composition(lo, skip, w, bias)
    E = DR.stage_exact(lo, skip, w, bias)
    lim = composition_bar(In64, slack, w.double().numpy(), cl)
    err = np.abs(E["out"] - want)
    assert E["out"].shape == want.shape == (2, co, 40, 56) and (err <= lim).all()
    assert err.max() > 0 and (E["out"] < 0).any() and (E["out"] > 0).any()   # (the rounding of the upsampled operands IS there)
    # the upsampled channels first, unrounded: against the real modules' float64 concatenation
    In32 = DR.concat(lo, skip)
    assert np.array_equal(In32[:, cl:], skip.numpy()) and (np.abs(In32[:, :cl] - In64[:, :cl]) <= slack).all()
    for mistake in DR.MISTAKES:
        got = DR.mistaken(lo, skip, w, bias, mistake)
        assert got.shape == want.shape and (np.abs(got - want) > lim).any(), mistake
        # ... and the device tests' own bar, against the restatement, catches it too
        assert (np.abs(got - E["out"]) > DR.bar(E["A"], DR.terms(cl, cs))).any(), mistake


@pytest.mark.parametrize("triple", DC.TRIPLES)
def test_restatement_under_one_hot_weights_is_the_shifted_rounded_operand(triple):
    for b, h, w in DC.SHAPES:
        lo, skip, _ = DC.seeded(b, h, w, triple, seed=71)
        taps, wt, bias = DC.onehot(triple, seed=72)
        E = DR.stage_exact(lo, skip, wt, bias)
        want = DR.onehot_expected(E["In"], taps)
        assert want.shape == E["out"].shape and (want < 0).any() and (want > 0).any() and (want == 0).any()
        assert np.array_equal(E["out"][want >= 0], want[want >= 0].astype(np.float64))
        assert (np.abs(E["out"] - want) <= DR.U32 * np.abs(want)).all()   # a negative value: the float32 rounding of x * 0.1f


def test_integer_data_is_integral_with_every_partial_sum_exact():
    assert 1728 * DC.INT_W * DC.INT_X < 2 ** 20 == DC.INT_BIAS
    for triple in DC.TRIPLES:
        lo, skip, (w, bias) = DC.integers(1, 32, 48, triple, seed=12)
        E = DR.stage_exact(lo, skip, w, bias)
        assert np.array_equal(E["In"], np.rint(E["In"])) and np.abs(E["In"]).max() <= DC.INT_X and np.abs(E["w"]).max() <= DC.INT_W
        assert np.array_equal(E["w"], w.double().numpy()) and E["A"].max() + float(bias.max()) < 2 ** 24
        assert (E["pre"] > 0).all() and np.array_equal(E["out"], np.rint(E["pre"])) and len(np.unique(E["out"])) > 1000
