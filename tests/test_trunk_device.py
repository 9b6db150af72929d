"""GPU tests of the fused trunk convolution (pvnet_amd/trunk.py, pvnet_amd/csrc/trunk.hip, libpvnet_trunk.so) against the restatement
of include/pvnet_trunk.h (tests/trunk_restatement.py).

No tolerance here is measured on the device code.  One-hot weights of +-1 must give the shifted, rounded operand itself
(``torch.equal``): that pins the stride, the dilation, the padding, every tap and the order of the two sources through the one tier
the library has.  Exact integer data must come out as THE integers, residual included.  Seeded real data at a trained trunk's scales is
held, every element, to the a-priori bar of tests/trunk_restatement.py.  The network tests compare with eager PyTorch, never with the
code under test."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import trunk_cases as TC  # noqa: E402
from tests import trunk_restatement as R  # noqa: E402

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
geometries = pytest.mark.parametrize("geometry", TC.GEOMETRIES, ids=[f"s{s}d{d}" for s, d in TC.GEOMETRIES])
triples = pytest.mark.parametrize("triple", TC.SMALL_TRIPLES, ids=["-".join(map(str, t)) for t in TC.SMALL_TRIPLES])
_exact = {}


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import trunk
    return trunk


def dev():
    return torch.device("cuda:0")


def up(t):
    return None if t is None else t.to(dev())


def exact(shape, triple, geometry, act, seed, dtypes=(torch.float32,) * 3, even=False):
    """the seeded case and its restatement, computed once and left unchanged; dtypes: of src1, src2 and res (the restatement widens
    them exactly, as the kernel does)"""
    key = (shape, triple, geometry, act, seed, dtypes, even)
    if key not in _exact:
        s, d = geometry
        src1, src2, res, (w, bias) = TC.seeded(*shape, triple, s, seed, even=even)
        src1, res = src1.to(dtypes[0]), res.to(dtypes[2])
        src2 = None if src2 is None else src2.to(dtypes[1])
        _exact[key] = (src1, src2, res, (w, bias), R.conv_exact(src1, w, bias, s, d, act, src2=src2, res=res))
    return _exact[key]


def hold(T, case, triple, geometry, act, out_dtypes=(torch.float32,), devs=None, misaligned=False, what=""):
    """the bar, every element; `devs`: the device tensors (src1, src2, res) the kernel reads instead of plain copies"""
    src1, src2, res, (w, bias), E = case
    s, d = geometry
    P = T.ConvParams(w, bias, s, d, act)
    d1, d2, dr = devs if devs is not None else (up(src1), up(src2), up(res))
    shape = E["out"].shape
    for dt in out_dtypes:
        kw = dict(out_dtype=dt)
        if misaligned:   # starts one element past an aligned address
            kw["out"] = torch.empty(int(np.prod(shape)) + 1, dtype=dt, device=dev())[1:].view(shape)
        out = T.fused_conv3x3(d1, P, src2=d2, residual=dr, **kw)
        torch.cuda.synchronize()
        assert out.dtype == dt and tuple(out.shape) == shape and out.is_contiguous()
        lim = R.bar(E["A"], triple[0] + triple[1], E["out"], dt)
        err = np.abs(out.cpu().double().numpy() - E["out"])
        print(f"trunk {what} s{s} d{d} {triple} {shape} {dt}: worst ratio to the bar {float((err / np.maximum(lim, 1e-300)).max()):.3f}")
        assert (err <= lim).all(), dt


# ---- one-hot weights: the geometry and the operand definition, bit for bit ------------------------------------------------------------
@geometries
@triples
def test_one_hot_weights_give_the_shifted_rounded_operand_itself(T, geometry, triple):
    s, d = geometry
    taps, w, bias = TC.onehot(triple, seed=5)
    P = T.ConvParams(w, bias, s, d, "none")
    for k, shape in enumerate(TC.SHAPES):
        src1, src2, _, _ = TC.seeded(*shape, triple, s, seed=100 + k, even=shape[0] == 3)
        src1 = src1 - 0.3                     # both signs: nothing is activated here
        want = torch.from_numpy(R.onehot_expected(R.bf16_round(R.concat(src1, src2)), taps, s, d))
        out = T.fused_conv3x3(up(src1), P, src2=up(src2), out_dtype=torch.float32).cpu()
        assert torch.equal(out, want), shape
        # the other order of the sources is another result
        if src2 is not None and triple[0] == triple[1]:
            assert not torch.equal(T.fused_conv3x3(up(src2), P, src2=up(src1), out_dtype=torch.float32).cpu(), want), shape


@geometries
def test_one_hot_weights_with_a_residual_and_relu(T, geometry):
    s, d = geometry
    triple, shape = TC.SMALL_TRIPLES[1], TC.SHAPES[3]
    taps, w, bias = TC.onehot(triple, seed=6)
    P = T.ConvParams(w, bias, s, d, "relu")
    src1, src2, res, _ = TC.seeded(*shape, triple, s, seed=111, even=True)
    src1, res = src1 - 0.3, res - 0.5
    x = torch.from_numpy(R.onehot_expected(R.bf16_round(R.concat(src1, src2)), taps, s, d))
    v = x + res                                       # one float32 addition
    want32 = torch.where(v <= 0, torch.zeros_like(v), v)
    assert (want32 == 0).any() and (want32 > 0).any()
    for dt in DTYPES:
        out = T.fused_conv3x3(up(src1), P, src2=up(src2), residual=up(res), out_dtype=dt).cpu()
        assert torch.equal(out, want32.to(dt)), dt   # rounded once


# ---- exact integer data ---------------------------------------------------------------------------------------------------------------------
@geometries
@triples
def test_integer_data_comes_out_as_the_integers(T, geometry, triple):
    s, d = geometry
    for k, shape in enumerate((TC.SHAPES[2], TC.SHAPES[3])):
        src1, src2, res, (w, bias) = TC.integers(*shape, triple, s, seed=20 + k)
        E = R.conv_exact(src1, w, bias, s, d, "relu", src2=src2, res=res)
        assert (E["pre"] > 0).all() and np.array_equal(E["out"], np.round(E["out"])) and np.abs(E["out"]).max() < 2 ** 24
        out = T.fused_conv3x3(up(src1), T.ConvParams(w, bias, s, d, "relu"), src2=up(src2), residual=up(res), out_dtype=torch.float32)
        assert np.array_equal(out.cpu().double().numpy(), E["out"]), shape


# ---- the a-priori bar on seeded data ----------------------------------------------------------------------------------------------------------
@geometries
@pytest.mark.parametrize("k", range(len(TC.SHAPES)), ids=["x".join(map(str, s)) for s in TC.SHAPES])
def test_bar_at_every_geometry_and_shape(T, geometry, k):
    shape = TC.SHAPES[k]
    for triple, act in zip(TC.SMALL_TRIPLES, ("relu", "leaky", "none")):
        hold(T, exact(shape, triple, geometry, act, seed=30 + k, even=shape[0] == 3), triple, geometry, act, what="shape")


@pytest.mark.parametrize("src_dtype", DTYPES)
def test_bar_with_the_types_crossed(T, src_dtype):
    triple, geometry, shape = TC.SMALL_TRIPLES[1], (1, 2), TC.SHAPES[2]
    for k, (t2, tr) in enumerate(((torch.float32, torch.bfloat16), (torch.float16, torch.float32), (torch.bfloat16, torch.float16))):
        case = exact(shape, triple, geometry, "leaky", seed=40, dtypes=(src_dtype, t2, tr))
        hold(T, case, triple, geometry, "leaky", out_dtypes=DTYPES, what=f"types {src_dtype} {t2} {tr}")


@pytest.mark.parametrize("layout", ["channels_last", "slice", "misaligned_out"])
@pytest.mark.parametrize("geometry", [(1, 1), (2, 1)], ids=["s1d1", "s2d1"])
def test_bar_with_strided_inputs_and_a_misaligned_out(T, geometry, layout):
    triple, shape = TC.SMALL_TRIPLES[1], TC.SHAPES[3]
    case = exact(shape, triple, geometry, "relu", seed=41, dtypes=(torch.bfloat16, torch.float16, torch.bfloat16), even=True)
    src1, src2, res = case[:3]
    devs = None
    if layout == "channels_last":
        devs = tuple(up(t).contiguous(memory_format=torch.channels_last) for t in (src1, src2, res))
        assert not devs[0].is_contiguous()
    elif layout == "slice":   # every tensor a window of a larger one, in all four dimensions
        def window(t):
            big = torch.full((t.shape[0] + 1, t.shape[1] + 3, t.shape[2] + 2, t.shape[3] + 5), float("nan"), dtype=t.dtype, device=dev())
            view = big[1:, 2:2 + t.shape[1], 1:1 + t.shape[2], 3:3 + t.shape[3]]
            view.copy_(t)
            return view
        devs = tuple(window(t) for t in (src1, src2, res))
    hold(T, case, triple, geometry, "relu", out_dtypes=(torch.bfloat16, torch.float32), devs=devs, misaligned=layout == "misaligned_out",
         what=layout)


@pytest.mark.parametrize("triple", TC.FULL_TRIPLES, ids=["-".join(map(str, t)) for t in TC.FULL_TRIPLES])
def test_bar_at_the_full_widths(T, triple):
    geometry = (1, 4) if triple[1] == 0 else (1, 1)   # layer4's and conv8s' own
    act = "relu" if triple[1] == 0 else "leaky"
    hold(T, exact(TC.TINY, triple, geometry, act, seed=42), triple, geometry, act, out_dtypes=(torch.bfloat16,), what="full width")


def test_a_negative_stride_through_the_c_abi_takes_the_wide_addresses(T):
    """torch has no negative strides, the C ABI has: src1 handed over mirrored in x, with its last column's address and stride -1, is
    the mirrored tensor -- the staging path with a 64-bit address per load"""
    from pvnet_amd import _abi
    triple, geometry, shape = TC.SMALL_TRIPLES[0], (1, 2), TC.SHAPES[2]
    src1, _, res, (w, bias), E = exact(shape, triple, geometry, "relu", seed=43)
    P = T.ConvParams(w, bias, 1, 2, "relu")
    mirrored = up(src1.flip(3).contiguous())
    b, c, h, wd = src1.shape
    st = mirrored.stride()
    out = torch.empty(E["out"].shape, dtype=torch.float32, device=dev())
    bias_d, wpk = P.on(dev())
    r = up(res)
    rc = _abi.load_trunk_library().pvnet_conv3x3_fused(
        C.c_void_p(mirrored.data_ptr() + 4 * (wd - 1)), _abi.TRUNK_T_F32, (C.c_int64 * 4)(st[0], st[1], st[2], -1), None, 0, None,
        C.c_void_p(r.data_ptr()), _abi.TRUNK_T_F32, (C.c_int64 * 4)(*r.stride()), C.c_void_p(wpk.data_ptr()), C.c_void_p(bias_d.data_ptr()),
        b, h, wd, c, 0, triple[2], 1, 2, _abi.TRUNK_ACT_RELU, C.c_void_p(out.data_ptr()), _abi.TRUNK_T_F32,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(out, T.fused_conv3x3(up(src1), P, residual=r, out_dtype=torch.float32))   # the same arithmetic, bit for bit
    assert (np.abs(out.cpu().double().numpy() - E["out"]) <= R.bar(E["A"], triple[0])).all()


# ---- non-finite values ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_and_an_inf_reach_exactly_the_windows_that_contain_them(T):
    triple, (s, d), shape = TC.SMALL_TRIPLES[1], (1, 4), TC.SHAPES[2]
    src1, src2, res, (w, bias), _ = exact(shape, triple, (s, d), "relu", seed=44)
    src1, src2 = src1.clone(), src2.clone()
    b, ho, wo = shape
    spots = [(src1, 0, 7, 0, 0, float("nan")), (src2, 0, 31, 9, 13, float("inf")), (src1, 0, 63, ho - 1, wo - 1, float("-inf"))]
    want = torch.zeros(b, ho, wo, dtype=torch.bool)
    for t, bi, c, y, x, val in spots:
        t[bi, c, y, x] = val
        for ky in range(3):
            for kx in range(3):
                Y, X = y - d * (ky - 1), x - d * (kx - 1)    # the output pixels whose tap (ky, kx) is (y, x)
                if 0 <= Y < ho and 0 <= X < wo:
                    want[bi, Y, X] = True
    assert (w != 0).all() and int(want.sum()) == 4 + 9 + 4      # the three spots' windows do not meet
    # without an activation: an infinity times a non-zero weight, or a NaN, in every output channel of exactly those pixels
    out = T.fused_conv3x3(up(src1), T.ConvParams(w, bias, s, d, "none"), src2=up(src2), residual=up(res), out_dtype=torch.float32).cpu()
    assert torch.equal(~out.isfinite(), want[:, None].expand_as(out))
    # the ReLU keeps a NaN (its comparison is false), so the NaN's four windows stay NaN in every channel, and nothing else is
    out = T.fused_conv3x3(up(src1), T.ConvParams(w, bias, s, d, "relu"), src2=up(src2), residual=up(res), out_dtype=torch.bfloat16).cpu()
    nan_spot = torch.zeros_like(want)
    nan_spot[0, 0:5:4, 0:5:4] = True
    assert torch.equal(out.isnan(), nan_spot[:, None].expand_as(out))
    assert torch.equal((~out.isfinite()).any(1) | want, want) and (out[out.isfinite()] >= 0).all()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(T):
    triple, geometry, shape = TC.SMALL_TRIPLES[1], (1, 4), TC.SHAPES[3]
    src1, src2, res, (w, bias), _ = exact(shape, triple, geometry, "relu", seed=45)
    other = TC.seeded(*shape, triple, 1, seed=46)[0]
    P = T.ConvParams(w, bias, 1, 4, "relu")
    d1, d2, dr = up(src1), up(src2), up(res)
    want1 = T.fused_conv3x3(d1, P, src2=d2, residual=dr, out_dtype=torch.bfloat16).clone()   # (also uploads the weights before the capture)
    want2 = T.fused_conv3x3(up(other), P, src2=d2, residual=dr, out_dtype=torch.bfloat16).clone()
    assert not torch.equal(want1, want2)
    out = torch.zeros_like(want1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            T.fused_conv3x3(d1, P, src2=d2, residual=dr, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        if k == 2:   # the input replaced in place
            d1.copy_(other.to(dev()))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want2 if k == 2 else want1), k


# ---- the network -----------------------------------------------------------------------------------------------------------------------------
def _eager_block_exact(blk, x, residual):
    """the block in float64 on the operands the two launches multiply, launch by launch: (y1 exact from x, the bar of launch 1; then,
    from the DEVICE's y1, out exact and the bar of launch 2)"""
    p1, p2 = blk.conv1, blk.conv2
    E1 = R.conv_exact(x, p1.w, p1.bias, p1.stride, p1.dilation, "relu")
    return E1, lambda y1: R.conv_exact(y1, p2.w, p2.bias, 1, p2.dilation, "relu", res=residual)


@pytest.mark.parametrize("kind", ["plain_d2", "downsample_s2"])
def test_fused_basic_block_against_the_eager_block(T, kind):
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import e2e_amd
    torch.manual_seed(7)
    eager = e2e_amd.block(64, 64, 1, 2) if kind == "plain_d2" else e2e_amd.block(32, 64, 2, 1)
    with torch.no_grad():
        for bn in (m for m in eager.modules() if isinstance(m, torch.nn.BatchNorm2d)):   # a trained BatchNorm's statistics
            bn.running_mean.normal_(0, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.2)
    eager = eager.eval().to(dev())
    blk = T.FusedBasicBlock(eager)
    x = torch.relu(torch.randn(2, eager.c1.in_channels, 19, 27)).to(torch.bfloat16)
    xd = x.to(dev())
    out = blk(xd)
    y1 = T.fused_conv3x3(xd, blk.conv1)
    res = blk.residual(xd)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and (res is xd) == (kind == "plain_d2")
    # launch by launch, under the bar: launch 2 judged on the device's own (rounded) y1 and residual
    E1, second = _eager_block_exact(blk, x, res.cpu())
    assert (np.abs(y1.cpu().double().numpy() - E1["out"]) <= R.bar(E1["A"], blk.conv1.cin, E1["out"], torch.bfloat16)).all()
    E2 = second(y1.cpu())
    assert (np.abs(out.cpu().double().numpy() - E2["out"]) <= R.bar(E2["A"], blk.conv2.cin, E2["out"], torch.bfloat16)).all()
    # and the whole against the eager MODULE in float64 on the same input -- the folded BatchNorms are the module's, the downsample's
    # too.  What separates them, propagated: the weights' rounding (u A per launch, u = 2^-8), y1's rounding and launch 1's bar through
    # |w2| (the ReLU does not stretch a difference), the output's rounding, and float32's share of the folding
    with torch.no_grad():
        ref = eager.double()(x.double().to(dev())).cpu().numpy()
    u = R.U_BF16
    d1 = u * E1["A"] + R.bar(E1["A"], blk.conv1.cin, E1["out"], torch.bfloat16)
    lim = R.conv3(d1, np.abs(E2["w"]), 1, blk.conv2.dilation) + u * E2["A"] + R.bar(E2["A"], blk.conv2.cin, E2["out"], torch.bfloat16)
    if kind == "downsample_s2":
        # the residual is PyTorch's bfloat16 1 x 1 convolution of the folded downsample, and enters the output once (the addition,
        # then the ReLU).  With Ad = |bias| + sum |w| |x| of that convolution: its weights' and bias' rounding to bfloat16 (u Ad), a
        # float32 sum of cin terms in any order, doubled as in the bar, its result's rounding and the rounding of the bias' addition,
        # which torch makes as an operation of its own (u Ad each), and float32's share of the folding
        wd, bd = (t.double().numpy() for t in blk.down)
        s = blk.conv1.stride
        Ad = np.einsum("oc,bchw->bohw", np.abs(wd[:, :, 0, 0]), np.abs(x.double().numpy()[:, :, ::s, ::s])) + np.abs(bd)[None, :, None, None]
        lim = lim + (3 * u + 2 * (blk.conv1.cin + 4) * R.U32 + 1e-6) * Ad
    worst = float((np.abs(out.cpu().double().numpy() - ref) / (lim + 1e-6 * E2["A"])).max())
    print(f"FusedBasicBlock {kind} against the eager float64 module: worst ratio to the bar {worst:.3f}")
    assert (np.abs(out.cpu().double().numpy() - ref) <= lim + 1e-6 * E2["A"]).all()
