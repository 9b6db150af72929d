"""CPU-only checks of the fused stem (include/pvnet_stem.h, libpvnet_stem.so, pvnet_amd/stem.py): the registry rows and their place, the
header's constants against pvnet_amd/_abi.py, every bad argument rejected before any HIP call, ``StemParams``' folding of the BatchNorm
against torch's own and its refusals (the network class: tests/test_net_cpu.py), and the restatement (tests/stem_restatement.py):
against torch's float64 composition, against the fixture recorded from the reference's own stem, against one-hot weights, and against planted mistakes, each of which the device tests' bars must catch.
What holds for every side library alike is in tests/test_side_libraries_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pvnet_amd import _abi, build  # noqa: E402
from pvnet_amd import stem as S  # noqa: E402
from tests import stem_cases as SC  # noqa: E402
from tests import stem_restatement as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_stem.h")).read()
BADARG, UNSUPPORTED = -1, -3
shapes = pytest.mark.parametrize("shape", SC.SHAPES, ids=["x".join(map(str, s)) for s in SC.SHAPES])


# ---- 1. the registry rows and the ABI mirror -------------------------------------------------------------------------------------------
def test_registry_rows_and_their_place():
    assert build.SIDE_LIBRARIES["stem"] == (["stem.hip"], "pvnet_stem.h", [])
    for table in (build.SIDE_LIBRARIES, _abi.SIDE_LIBRARIES):
        names = list(table)
        assert names.index("stem") == names.index("decoder") - 1   # in the network's order: stem, decoder, tail; the same in both
    assert _abi.SIDE_LIBRARIES["stem"] == (_abi.STEM_LIB_PATH, _abi.STEM_ABI_VERSION, _abi.STEM_PROTOTYPES)
    assert _abi.load_stem_library.args == ("stem",)
    deps = build._side("stem")[1]
    assert not {os.path.basename(d) for d in deps} & {"mesh_core.h", "zbuffer_core.h", "depth_core.h", "pixel_color.h", "augment_warp.h"}
    assert "_abi.load_stem_library()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import pvnet_amd
    for name in ("StemParams", "fused_stem", "FusedStemNet"):
        assert getattr(pvnet_amd, name) is getattr(S, name) and name in pvnet_amd.__all__
    for doc in ("README.md", "INTEGRATION.md"):
        assert "include/pvnet_stem.h" in open(os.path.join(ROOT, doc)).read(), doc


def test_abi_version_and_constants_are_mirrored():
    defines = dict(re.findall(r"^#define\s+PVNET_STEM_(\w+)\s+(\d+)u?\b", HDR, re.M))
    assert {k: int(v) for k, v in defines.items()} == dict(
        ABI_VERSION=_abi.STEM_ABI_VERSION, CIN=_abi.STEM_CIN, COUT=_abi.STEM_COUT, T_F32=_abi.STEM_T_F32, T_F16=_abi.STEM_T_F16,
        T_BF16=_abi.STEM_T_BF16)
    assert (_abi.STEM_T_F32, _abi.STEM_T_F16, _abi.STEM_T_BF16) == (_abi.DECODER_T_F32, _abi.DECODER_T_F16, _abi.DECODER_T_BF16)
    assert _abi.STEM_COUT == _abi.DECODER_SKIP   # x2s is conv2s' skip input
    decl = re.search(r"^int pvnet_stem_forward\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.STEM_PROTOTYPES["pvnet_stem_forward"][1]
    assert len(decl) == len(args) == 12
    for k, (word, typ) in {0: ("const void* image", C.c_void_p), 1: ("int image_type", C.c_int), 2: ("image_strides[4]", _abi._i64p),
                           3: ("const float* w", C.c_void_p), 4: ("const float* bias", C.c_void_p), 5: ("int b", C.c_int),
                           6: ("int h", C.c_int), 7: ("int w_", C.c_int), 8: ("void* x2s", C.c_void_p), 9: ("void* pooled", C.c_void_p),
                           10: ("int out_type", C.c_int), 11: ("void* stream", C.c_void_p)}.items():
        assert word in decl[k] and args[k] is typ, (k, word)


# ---- 2. the library and its bad arguments: every one rejected before any HIP call (there is no device here to answer one) -----------------
@pytest.fixture(scope="module")
def lib():
    build.build_side("stem")
    return _abi.load_stem_library()


def test_library_holds_a_kernel_per_output_type_on_the_matrix_pipe(lib):
    assert b"stem_kernel" in open(_abi.STEM_LIB_PATH, "rb").read()
    asm = subprocess.run([build.hipcc_path()] + [f for f in build.flags() if f not in ("-shared", "-fPIC")] +
                         ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", os.path.join(build.CSRC, "stem.hip"), "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S*stem_kernel\S*)", asm, re.M)
    assert len(kernels) == 3 == len(set(kernels))   # float32, float16, bfloat16 out
    for name in kernels:
        start = asm.index("\n" + name + ":")
        body = asm[start:asm.index(".Lfunc_end", start)]
        assert len(re.findall(r"^\s*v_mfma_f32_32x32x16_bf16", body, re.M)) == 11, name   # a job's eleven k-steps, one row block
        assert "v_mfma_f32_32x32x2" not in body and not re.search(r"^\s*(scratch_|buffer_(load|store).*offen)", body, re.M), name
        assert "atomic" not in body
        desc = asm[asm.index(".amdhsa_kernel " + name):]
        # static LDS: two workgroups fit a compute unit's 160 KB
        assert 2 * int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) <= 160 * 1024


def call(lib, **over):
    """pvnet_stem_forward on host buffers that a rejected call never touches"""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    s4 = (C.c_int64 * 4)(1, 1, 1, 1)
    a = dict(image=p, image_type=0, image_strides=s4, w=p, bias=p, b=1, h=8, w_=12, x2s=p, pooled=p, out_type=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.pvnet_stem_forward(*a.values())


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    for name in ("image", "image_strides", "w", "bias", "x2s"):
        assert call(lib, **{name: None}) == BADARG, name
        assert call(lib, **{name: None}, pooled=None) == BADARG, name
    for over in (dict(b=0), dict(h=0), dict(w_=0), dict(b=-1), dict(h=-8), dict(image_type=3), dict(image_type=-1), dict(out_type=3),
                 dict(out_type=-1), dict(b=0, h=40000), dict(image_type=5, b=70000)):
        assert call(lib, **over) == BADARG, over
    for over in (dict(b=65536), dict(h=32769), dict(w_=32769), dict(b=65536, pooled=None), dict(h=1 << 30, w_=1 << 30)):
        assert call(lib, **over) == UNSUPPORTED, over


# ---- 3. StemParams ----------------------------------------------------------------------------------------------------------------------
def modules(seed=0, cin=3, cout=64, k=7, bias=False, **conv):
    torch.manual_seed(seed)
    conv1 = nn.Conv2d(cin, cout, k, bias=bias, **{**dict(stride=2, padding=3), **conv})
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.3, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    return conv1, bn.eval(), nn.ReLU(True), nn.MaxPool2d(3, 2, 1)


def test_folding_against_torchs_own_eval_batchnorm_in_float64():
    conv1, bn, act, pool = modules()
    P = S.StemParams.from_modules(conv1, bn, act=act, pool=pool)
    assert tuple(P.w.shape) == (64, 3, 7, 7) and all(t.dtype == torch.float32 and t.is_contiguous() for t in (P.w, P.bias))
    x = torch.randn(2, 3, 21, 27, dtype=torch.float64)
    with torch.no_grad():
        want = bn.double()(conv1.double()(x))
        got = F.conv2d(x, P.w.double(), P.bias.double(), stride=2, padding=3)
        # w and bias are float64 values rounded once to float32: 2^-24 of every term
        lim = 2.0 ** -24 * F.conv2d(x.abs(), P.w.double().abs(), P.bias.double().abs(), stride=2, padding=3) + 1e-14
    assert ((got - want).abs() <= lim).all()
    assert float((got - want).abs().max()) > 0   # (it IS rounded: not the float64 fold itself)
    # the fold is StageParams.from_modules': the same float64 operations on the same statistics
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    assert torch.equal(P.w, (conv1.weight.double() * s[:, None, None, None]).float())
    assert torch.equal(P.bias, (bn.bias.double() - bn.running_mean.double() * s).float())


def test_refusals():
    conv1, bn, act, pool = modules()
    with pytest.raises(ValueError, match="eval"):
        S.StemParams.from_modules(conv1, modules()[1].train())
    with pytest.raises(ValueError, match="running statistics"):
        S.StemParams.from_modules(conv1, nn.BatchNorm2d(64, track_running_stats=False).eval())
    for odd in (dict(bias=True), dict(cin=4), dict(cout=32), dict(k=5), dict(stride=1), dict(padding=2), dict(dilation=2),
                dict(padding_mode="reflect"), dict(cin=6, cout=64, groups=2)):
        c, n, _, _ = modules(**odd)
        with pytest.raises(ValueError):
            S.StemParams.from_modules(c, n)
    with pytest.raises(ValueError, match="Conv2d"):
        S.StemParams.from_modules(modules(stride=1)[0], bn)
    with pytest.raises(ValueError, match="bias"):
        S.StemParams.from_modules(modules(bias=True)[0], bn)
    with pytest.raises(ValueError, match="widths"):
        S.StemParams.from_modules(*modules(cout=32)[:2])
    for wrong in (nn.LeakyReLU(0.1), nn.ReLU6(), nn.Identity()):
        with pytest.raises(ValueError, match="ReLU"):
            S.StemParams.from_modules(conv1, bn, act=wrong)
    for wrong in (nn.MaxPool2d(2, 2), nn.MaxPool2d(3, 2, 0), nn.MaxPool2d(3, 1, 1), nn.MaxPool2d(3, 2, 1, dilation=2),
                  nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.AvgPool2d(3, 2, 1)):
        with pytest.raises(ValueError, match="MaxPool2d"):
            S.StemParams.from_modules(conv1, bn, act=act, pool=wrong)
    S.StemParams.from_modules(conv1, bn, act=act, pool=nn.MaxPool2d((3, 3), (2, 2), (1, 1)))   # the same pool spelled with pairs
    with pytest.raises(ValueError):
        S.StemParams(torch.zeros(64, 3, 3, 3), torch.zeros(64))
    with pytest.raises(ValueError):
        S.StemParams(torch.zeros(64, 3, 7, 7), torch.zeros(63))
    net, _ = SC.standin()
    with pytest.raises(ValueError, match="eval"):
        S.StemParams.from_network(net.train())
    net.eval()
    with pytest.raises(ValueError, match="neither"):
        S.StemParams.from_network(nn.Sequential())
    P = S.StemParams.from_network(net)
    with pytest.raises(RuntimeError):   # no CPU fallback
        S.fused_stem(torch.zeros(1, 3, 8, 8), P)
    with pytest.raises(RuntimeError):
        S.fused_stem(torch.zeros(1, 3, 8, 8), (P.w, P.bias))


def test_from_network_reads_the_standins_attribute_names():
    net, _ = SC.standin()
    P = S.StemParams.from_network(net)
    Q = S.StemParams.from_modules(net.stem[0], net.stem[1], act=net.stem[2], pool=net.pool)
    assert torch.equal(P.w, Q.w) and torch.equal(P.bias, Q.bias)
    assert P.on("cpu") is P.on(torch.device("cpu")) and torch.equal(P.on("cpu")[0], P.w)   # the device copies are kept


# ---- 4. the restatement --------------------------------------------------------------------------------------------------------------------
def composition(image, w, bias):
    """torch's float64 composition on the given operands: F.conv2d(stride 2, padding 3), relu, F.max_pool2d(3, 2, 1)"""
    with torch.no_grad():
        x2s = torch.relu(F.conv2d(image.double(), w.double(), bias.double(), stride=2, padding=3))
        return x2s.numpy(), F.max_pool2d(x2s, 3, 2, 1).numpy()


@shapes
def test_restatement_against_torchs_float64_composition(shape):
    b, h, w = shape
    image, (wt, bias) = SC.seeded(b, h, w, seed=70 + h)
    image, wt = image.to(torch.bfloat16).float(), wt.to(torch.bfloat16).float()   # the operands rounded to bfloat16 first
    want, want_pooled = composition(image, wt, bias)
    E = SR.stem_exact(image, wt, bias)
    assert np.array_equal(E["In"], image.double().numpy()) and np.array_equal(E["w"], wt.double().numpy())   # rounding changed nothing
    ho, wo, hp, wp = SC.out_sizes(h, w)
    assert E["x2s"].shape == want.shape == (b, 64, ho, wo) and E["pooled"].shape == want_pooled.shape == (b, 64, hp, wp)
    lim = SR.bar(E["A"])   # the device tests' bar: two float64 sums of the same terms differ by far less
    assert (np.abs(E["x2s"] - want) <= lim).all() and (np.abs(E["x2s"] - want) <= 1e-12 * (1 + E["A"])).all()
    assert (np.abs(E["pooled"] - want_pooled) <= SR.pool(lim)).all()
    assert np.array_equal(E["pooled"], F.max_pool2d(torch.from_numpy(E["x2s"]), 3, 2, 1).numpy())   # the pool alone: torch's own, exactly
    if h > 1:
        assert (E["x2s"] == 0).any() and (E["x2s"] > 0).any() and (E["pre"] < 0).any()


def test_unrounded_restatement_against_the_fixture_of_the_references_own_stem():
    g = np.load(SC.FIXTURE)
    assert g["x2s"].shape == (1, 64, 19, 27) and g["pooled"].shape == (1, 64, 10, 14) and g["x2s"].dtype == g["pooled"].dtype == np.float32
    assert os.path.getsize(SC.FIXTURE) < 200 * 1024
    net, _ = SC.standin()
    P = S.StemParams.from_network(net)
    x = SC.fixture_input()
    assert tuple(x.shape) == SC.FIXTURE_SHAPE
    E = SR.stem_exact(x, P.w, P.bias, rounded=False)
    for name in ("x2s", "pooled"):
        assert (np.abs(E[name] - g[name]) <= 1e-5 + 1e-5 * np.abs(g[name])).all(), name   # fixture G9's bar
    assert (g["x2s"] == 0).any() and (g["x2s"] > 0).any()
    # the rounded operands are a different function: the fixture's bar tells them apart
    R = SR.stem_exact(x, P.w, P.bias)
    assert (np.abs(R["x2s"] - g["x2s"]) > 1e-5 + 1e-5 * np.abs(g["x2s"])).any()


@pytest.mark.parametrize("mistake", SR.MISTAKES)
def test_planted_mistakes_fail_the_device_tests_bars(mistake):
    for b, h, w in (SC.SHAPES[1], SC.SHAPES[3]):
        image, (wt, bias) = SC.seeded(b, h, w, seed=75)
        E = SR.stem_exact(image, wt, bias)
        x2s, pooled = SR.mistaken(image, wt, bias, mistake)
        lim = SR.bar(E["A"])
        assert x2s.shape == E["x2s"].shape and pooled.shape == E["pooled"].shape
        if mistake.startswith("pool"):   # the convolution is right, the pool is not
            assert np.array_equal(x2s, E["x2s"])
            assert (np.abs(pooled - E["pooled"]) > SR.pool(lim)).any(), mistake
            # ... and it is no longer torch's pool of its own x2s, which the device tests demand bit for bit
            assert not np.array_equal(pooled, F.max_pool2d(torch.from_numpy(x2s), 3, 2, 1).numpy())
        else:
            assert (np.abs(x2s - E["x2s"]) > lim).any(), mistake
            assert (np.abs(pooled - E["pooled"]) > SR.pool(lim)).any(), mistake
            for dt in (torch.float16, torch.bfloat16):   # the half types' wider bars too
                assert (np.abs(x2s - E["x2s"]) > SR.bar(E["A"], E["x2s"], dt)).any(), (mistake, dt)


@shapes
def test_restatement_under_one_hot_weights_is_the_shifted_rounded_operand(shape):
    b, h, w = shape
    image, _ = SC.seeded(b, h, w, seed=71)
    seen = set()
    for k in range(SC.ONEHOT_SETS):
        taps, wt, bias = SC.onehot(k)
        seen |= set(taps)
        E = SR.stem_exact(image, wt, bias)
        want = SR.onehot_expected(E["In"], taps)
        assert np.array_equal(E["x2s"], want.astype(np.float64))
        if h > 1:
            assert (want > 0).any() and (want == 0).any()
    assert seen == {(c, ky, kx) for c in range(3) for ky in range(7) for kx in range(7)}   # each of the 147 taps occurs


def test_integer_data_is_integral_with_every_partial_sum_exact():
    assert 147 * SC.INT_W * SC.INT_X == 75264 and 75264 + SC.INT_BIAS < 2 ** 24
    image, (wt, bias) = SC.integers(2, 37, 53, seed=12)
    E = SR.stem_exact(image, wt, bias)
    assert np.array_equal(E["In"], image.double().numpy()) and np.array_equal(E["w"], wt.double().numpy())   # bfloat16 holds them
    assert np.abs(E["In"]).max() == SC.INT_X and np.abs(E["w"]).max() == SC.INT_W and E["A"].max() + SC.INT_BIAS < 2 ** 24
    assert np.array_equal(E["x2s"], np.rint(E["x2s"])) and (E["pre"] < 0).any() and (E["pre"] > 0).any()   # both signs of pre-activation
    assert len(np.unique(E["x2s"])) > 1000
