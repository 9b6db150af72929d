"""GPU tests of the fused stem (pvnet_amd/stem.py, pvnet_amd/csrc/stem.hip, libpvnet_stem.so) against the restatement of
include/pvnet_stem.h (tests/stem_restatement.py).

No tolerance here is measured on the device code.  One-hot weights must give the shifted, rounded, activated operand itself
(``torch.equal``): that pins the window's origin, the stride, the taps' and the channels' order and the padding through the one tier the
library has.  Exact integer data must come out as THE integers' ReLU.  Seeded real data at a trained stem's scales is held, every element,
to the a-priori bar of the tail's first stage, and the pooled tensor must be torch's own max-pool of the device's x2s, bit for bit.  The
network test compares with eager PyTorch, never with the code under test."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

from tests import stem_cases as SC  # noqa: E402
from tests import stem_restatement as SR  # noqa: E402

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
shapes = pytest.mark.parametrize("shape", SC.SHAPES, ids=["x".join(map(str, s)) for s in SC.SHAPES])
_exact = {}


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import stem
    return stem


def dev():
    return torch.device("cuda:0")


def exact(shape, seed, dtype=torch.float32):
    """the seeded case and its restatement, computed once and left unchanged"""
    key = (shape, seed, dtype)
    if key not in _exact:
        image, params = SC.seeded(*shape, seed=seed)
        image = image.to(dtype)   # the restatement widens it exactly, as the kernel does
        _exact[key] = (image, params, SR.stem_exact(image, *params))
    return _exact[key]


def run(S, image, params, **kw):
    """fused_stem on a device copy (or on the given device tensor) -> the results on the CPU"""
    P = params if isinstance(params, S.StemParams) else S.StemParams(*params)
    x2s, pooled = S.fused_stem(image if image.is_cuda else image.to(dev()), P, **kw)
    torch.cuda.synchronize()
    return x2s.cpu(), None if pooled is None else pooled.cpu()


def torch_pool(x2s):
    """nn.MaxPool2d(3, 2, 1) on a CPU tensor of any of the three types, in float32 (which holds them exactly)"""
    return F.max_pool2d(x2s.float(), 3, 2, 1)


def same(a, b):
    """bit for bit where neither is NaN, NaN where the other is"""
    a, b = a.float(), b.float()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0))


def hold(S, image, params, E, out_dtypes=(torch.float32,), image_dev=None, misaligned=False, what=""):
    """the bars, every element; `image` is the CPU tensor the restatement read, image_dev what the device reads instead"""
    b, _, h, w = image.shape
    ho, wo, hp, wp = SC.out_sizes(h, w)
    P = S.StemParams(*params)
    for dt in out_dtypes:
        kw = dict(out_dtype=dt)
        if misaligned:   # both start one element past an aligned address
            kw["out"] = (torch.empty(b * 64 * ho * wo + 1, dtype=dt, device=dev())[1:].view(b, 64, ho, wo),
                         torch.empty(b * 64 * hp * wp + 1, dtype=dt, device=dev())[1:].view(b, 64, hp, wp))
        x2s, pooled = run(S, image if image_dev is None else image_dev, P, **kw)
        assert x2s.dtype == pooled.dtype == dt and tuple(x2s.shape) == (b, 64, ho, wo) and tuple(pooled.shape) == (b, 64, hp, wp)
        assert x2s.is_contiguous() and pooled.is_contiguous()
        lim = SR.bar(E["A"], E["x2s"], dt)
        err, perr = np.abs(x2s.double().numpy() - E["x2s"]), np.abs(pooled.double().numpy() - E["pooled"])
        print(f"stem {what} {dt}: worst ratio to the bar, x2s {float((err / np.maximum(lim, 1e-300)).max()):.3f}, "
              f"pooled {float((perr / np.maximum(SR.pool(lim), 1e-300)).max()):.3f}")
        assert (err <= lim).all(), dt
        assert (perr <= SR.pool(lim)).all(), dt
        assert torch.equal(pooled.float(), torch_pool(x2s)), dt   # independently: torch's pool of the device's own x2s


# ---- one-hot weights: the geometry and the operand definition, bit for bit ------------------------------------------------------------
@shapes
def test_one_hot_weights_give_the_shifted_rounded_operand_itself(S, shape):
    b, h, w = shape
    image, _ = SC.seeded(b, h, w, seed=80)
    assert (image < 0).any() and (image > 0).any()
    image_d = image.to(dev())
    In = SR.bf16_round(image.numpy())
    for k in range(SC.ONEHOT_SETS):
        taps, wt, bias = SC.onehot(k)
        want = torch.from_numpy(SR.onehot_expected(In, taps))
        x2s, pooled = run(S, image_d, (wt, bias), out_dtype=torch.float32)
        assert torch.equal(x2s, want), k
        assert torch.equal(pooled, torch_pool(want)), k
    if shape == SC.SHAPES[1]:   # the half types in are widened exactly
        taps, wt, bias = SC.onehot(1)
        for dt in (torch.float16, torch.bfloat16):
            x2s, _ = run(S, image.to(dt), (wt, bias), out_dtype=torch.float32)
            assert torch.equal(x2s, torch.from_numpy(SR.onehot_expected(SR.bf16_round(image.to(dt).float().numpy()), taps))), dt


# ---- exact integer data --------------------------------------------------------------------------------------------------------------
@shapes
def test_integer_data_comes_out_as_the_integers(S, shape):
    b, h, w = shape
    image, params = SC.integers(b, h, w, seed=11)
    E = SR.stem_exact(image, *params)
    assert np.array_equal(E["x2s"], np.rint(E["x2s"])) and E["A"].max() + SC.INT_BIAS < 2 ** 24
    if h > 1:
        assert (E["pre"] < 0).any() and (E["pre"] > 0).any()   # both signs of pre-activation
    want, want_pooled = torch.from_numpy(E["x2s"]).float(), torch.from_numpy(E["pooled"]).float()
    x2s, pooled = run(S, image, params, out_dtype=torch.float32)
    assert torch.equal(x2s, want) and torch.equal(pooled, want_pooled)
    for dt in (torch.float16, torch.bfloat16):   # one rounding of the exact value
        x2s, pooled = run(S, image, params, out_dtype=dt)
        assert x2s.dtype == pooled.dtype == dt and torch.equal(x2s, want.to(dt)) and torch.equal(pooled, want_pooled.to(dt)), dt


# ---- seeded real data: the a-priori bar ------------------------------------------------------------------------------------------------
@shapes
def test_bar_at_every_shape(S, shape):
    image, params, E = exact(shape, seed=20 + shape[1])
    hold(S, image, params, E, out_dtypes=(torch.float32, torch.bfloat16), what="x".join(map(str, shape)))


@pytest.mark.parametrize("image_dtype", DTYPES)
def test_bar_with_the_types_crossed(S, image_dtype):
    image, params, E = exact(SC.SHAPES[1], seed=31, dtype=image_dtype)
    hold(S, image, params, E, out_dtypes=DTYPES, what=f"{image_dtype} in")


@pytest.mark.parametrize("layout", ["channels_last", "slice", "misaligned_out"])
def test_bar_with_a_strided_image_and_misaligned_outputs(S, layout):
    shape = SC.SHAPES[3]
    image, params, E = exact(shape, seed=32)
    b, h, w = shape
    image_d = image.to(dev())
    if layout == "channels_last":
        image_d = image_d.contiguous(memory_format=torch.channels_last)
        assert not image_d.is_contiguous()
    elif layout == "slice":   # a channel slice of a wider tensor and a window of a larger plane; NaN around it
        wide = torch.full((b, 5, h + 3, w + 7), float("nan"), device=dev())
        wide[:, 1:4, 2:2 + h, 3:3 + w] = image_d
        image_d = wide[:, 1:4, 2:2 + h, 3:3 + w]
    hold(S, image, params, E, out_dtypes=DTYPES, image_dev=image_d, misaligned=layout == "misaligned_out", what=layout)


# ---- NaN and Inf --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SC.SHAPES[1], SC.SHAPES[3]], ids=["2x37x53", "3x18x262"])
def test_a_nan_and_an_inf_reach_exactly_the_windows_that_contain_them(S, shape):
    b, h, w = shape
    image, params, _ = exact(shape, seed=40)
    assert (params[0].to(torch.bfloat16) != 0).all()   # all weights non-zero
    # the NaN where its windows cross a tile boundary in both directions (x2s column 64 | row 4), the Inf in another image, near a corner
    ny, nx = 8, min(128, w - 9)
    bad = image.clone()
    bad[b - 1, 1, ny, nx] = float("nan")
    bad[0, 2, 1, 2] = float("inf")
    with np.errstate(invalid="ignore"):
        E = SR.stem_exact(bad, *params)
    touched = SR.window_sum(torch.isfinite(bad).logical_not().double().numpy(), np.ones((64, 3, 7, 7))) > 0   # windows with the NaN or the Inf
    nan = np.isnan(E["x2s"])
    assert 64 * 9 <= nan.sum() <= 64 * 16 and (touched & ~nan).sum() >= 64 * 4 and np.isinf(E["x2s"]).any()
    for dt in (torch.float32, torch.bfloat16):
        clean, clean_pooled = run(S, image, params, out_dtype=dt)
        x2s, pooled = run(S, bad, params, out_dtype=dt)
        assert torch.equal(x2s.isnan(), torch.from_numpy(nan)), dt
        outside = torch.from_numpy(~touched)
        assert torch.equal(x2s[outside].view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                           clean[outside].view(torch.int16 if dt == torch.bfloat16 else torch.int32)), dt   # bits
        # a window with the Inf alone holds one infinite product: +Inf, or -Inf and so +0
        inf_only = torch.from_numpy(touched & ~nan)
        assert torch.equal(x2s[inf_only].float(), torch.from_numpy(E["x2s"])[inf_only].float()), dt
        # pooled: NaN exactly over the windows with a NaN, the pool of the stored values elsewhere
        assert torch.equal(pooled.isnan(), torch.from_numpy(SR.pool(nan.astype(np.float64)) > 0)), dt
        assert torch.equal(pooled.isnan(), torch.from_numpy(np.isnan(E["pooled"]))), dt
        assert same(pooled, torch_pool(x2s)), dt
        pool_outside = torch.from_numpy(SR.pool(touched.astype(np.float64)) == 0)
        assert torch.equal(pooled[pool_outside].float(), clean_pooled[pool_outside].float()), dt


# ---- the launch ---------------------------------------------------------------------------------------------------------------------------
def test_without_the_pool_x2s_has_the_same_bits_and_out_is_returned(S):
    shape = SC.SHAPES[3]
    image, params, _ = exact(shape, seed=50)
    b, h, w = shape
    ho, wo, hp, wp = SC.out_sizes(h, w)
    P = S.StemParams(*params)
    image_d = image.to(dev())
    for dt in (torch.bfloat16, torch.float32):
        a, ap = S.fused_stem(image_d, P, out_dtype=dt)
        only, none = S.fused_stem(image_d, P, out_dtype=dt, pool=False)
        assert none is None and only.dtype == dt and torch.equal(only.float(), a.float())
        out = (torch.full((b, 64, ho, wo), float("nan"), dtype=dt, device=dev()), torch.full((b, 64, hp, wp), float("nan"), dtype=dt, device=dev()))
        x2s, pooled = S.fused_stem(image_d, P, out=out)
        assert x2s is out[0] and pooled is out[1] and torch.equal(x2s.float(), a.float()) and torch.equal(pooled.float(), ap.float())
        alone = torch.full((b, 64, ho, wo), float("nan"), dtype=dt, device=dev())
        x2s, pooled = S.fused_stem(image_d, P, out=alone, pool=False)
        assert x2s is alone and pooled is None and torch.equal(alone.float(), a.float())   # (a NaN left behind would show)
    # a pixel's arithmetic does not depend on the launch's shape: one image of the batch alone
    one, onep = S.fused_stem(image_d[1:2], P, out_dtype=torch.float32)
    a, ap = S.fused_stem(image_d, P, out_dtype=torch.float32)
    assert torch.equal(one, a[1:2]) and torch.equal(onep, ap[1:2])
    with pytest.raises(RuntimeError):
        S.fused_stem(image_d, P, out=(a, ap), out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        S.fused_stem(image_d, P, out=(a, ap[:, :, :-1]))
    with pytest.raises(RuntimeError):
        S.fused_stem(image_d, P, out=(a, ap), pool=False)
    with pytest.raises(RuntimeError):
        S.fused_stem(image_d, P, out=a)
    with pytest.raises(RuntimeError):
        S.fused_stem(image_d[:, :2], P)
    with pytest.raises(RuntimeError):
        S.fused_stem(image, P)   # a CPU tensor
    with pytest.raises(RuntimeError):
        S.fused_stem(image_d.double(), P)


def test_graph_capture_and_replay(S):
    shape = SC.SHAPES[1]
    image, params, _ = exact(shape, seed=51)
    image2, _ = SC.seeded(*shape, seed=52)
    P = S.StemParams(*params)
    s_im = image.to(dev())
    want1 = tuple(t.clone() for t in S.fused_stem(s_im, P, out_dtype=torch.bfloat16))   # (also uploads the weights before the capture)
    want2 = tuple(t.clone() for t in S.fused_stem(image2.to(dev()), P, out_dtype=torch.bfloat16))
    assert not torch.equal(want1[0], want2[0])
    out = tuple(torch.zeros_like(t) for t in want1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            S.fused_stem(s_im, P, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        if k == 2:   # the image replaced in place
            s_im.copy_(image2.to(dev()))
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, want2 if k == 2 else want1):
            assert torch.equal(got, want), k
