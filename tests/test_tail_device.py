"""GPU tests of the fused network tail (pvnet_amd/tail.py, pvnet_amd/csrc/tail.hip, libpvnet_tail.so) against the restatement of
include/pvnet_tail.h (tests/tail_restatement.py).

No tolerance here is measured on the device code.  Exact integer data must come out as THE integers (``torch.equal``) in both tiers,
raw and final -- the test for a swapped C/D map or a mis-ordered k of the accumulator-as-operand step.  Seeded real data is held stage
by stage to the restatement's bars, every element: stage 1 on the raw output, stage 2 on the output given the device's own raw values.
The float32 tier's raw output under centre-tap identity weights IS the restatement's float32 upsample, bit for bit; the ramp's closed
form holds within 8 u32 of its magnitude; fixture G9 holds the float32 tier to the reference's outputs under the fixture's own bar and
the bfloat16 tier under its a-priori bound."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import tail_cases as TC  # noqa: E402
from tests import tail_restatement as TR  # noqa: E402

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
PRECISIONS = ("bf16", "f32")


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import tail
    return tail


def dev():
    return torch.device("cuda:0")


def run(T, fm, image, params, **kw):
    """fused_tail on device copies (or on the given device tensors) -> the result on the CPU"""
    P = params if isinstance(params, T.TailParams) else T.TailParams(*params)
    fm = fm if fm.is_cuda else fm.to(dev())
    image = image if image.is_cuda else image.to(dev())
    out = T.fused_tail(fm, image, P, **kw)
    torch.cuda.synchronize()
    return out.cpu()


def hold_stages(T, fm, image, params, precision, out_dtypes=(torch.float32,), fm_dev=None, image_dev=None, misaligned=False):
    """both bars, every element; fm / image are the CPU tensors the restatement reads, *_dev what the device reads instead"""
    w1, b1, w2, b2 = params
    E = TR.forward_exact(fm, image, w1, b1, w2, b2, precision)
    fm_d = fm.to(dev()) if fm_dev is None else fm_dev
    im_d = image.to(dev()) if image_dev is None else image_dev
    b, h, w = image.shape[0], image.shape[2], image.shape[3]

    def given(shape, dtype):
        if not misaligned:
            return {}
        n = int(np.prod(shape))
        return dict(out=torch.empty(n + 1, dtype=dtype, device=dev())[1:].view(shape))   # starts one element past an aligned address

    X = run(T, fm_d, im_d, params, precision=precision, raw=True, **given((b, 32, h, w), torch.float32))
    assert X.dtype == torch.float32 and tuple(X.shape) == (b, 32, h, w)
    err1, lim1 = np.abs(X.double().numpy() - E["X"]), TR.bar1(E["A1"])
    print(f"stage 1 {precision}: worst ratio to the bar {float((err1 / np.maximum(lim1, 1e-300)).max()):.3f}")
    assert (err1 <= lim1).all()
    Xq = TR.stage2_input(X, precision)
    y_want, A2 = TR.out_exact(Xq, E["w2"], b2)
    for dt in out_dtypes:
        y = run(T, fm_d, im_d, params, precision=precision, out_dtype=dt, **given((b, w2.shape[0], h, w), dt))
        assert y.dtype == dt and tuple(y.shape) == (b, w2.shape[0], h, w) and y.is_contiguous()
        err2, lim2 = np.abs(y.double().numpy() - y_want), TR.bar2(A2, y_want, dt)
        print(f"stage 2 {precision} {dt}: worst ratio to the bar {float((err2 / np.maximum(lim2, 1e-300)).max()):.3f}")
        assert (err2 <= lim2).all(), dt


# ---- exact integer data --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cout", TC.COUTS)
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_integer_data_comes_out_as_the_integers(T, shape, cout, precision):
    b, h, w = shape
    # raw: both branches of the activation
    fm, image, params = TC.integers(b, h, w, cout, seed=11, positive=False)
    E = TR.forward_exact(fm, image, *params, precision)
    assert np.array_equal(E["In"], np.rint(E["In"])) and E["A1"].max() < 2 ** 24   # integral operands, exact partial sums
    assert (E["X"] < 0).any() and (E["X"] > 0).any()
    X = run(T, fm, image, params, precision=precision, raw=True)
    assert torch.equal(X, torch.from_numpy(E["X"].astype(np.float32)))   # (a negative value is the one rounding of v * 0.1f)
    # final: no negative pre-activation, so the raw values are integers and so is everything stage 2 adds up
    fm, image, params = TC.integers(b, h, w, cout, seed=12, positive=True)
    E = TR.forward_exact(fm, image, *params, precision)
    assert (E["X"] > 0).all() and np.array_equal(E["X"], np.rint(E["X"])) and E["A1"].max() < 2 ** 24 and E["A2"].max() < 2 ** 24
    assert np.array_equal(E["y"], np.rint(E["y"]))
    y = run(T, fm, image, params, precision=precision, out_dtype=torch.float32)
    assert torch.equal(y, torch.from_numpy(E["y"].astype(np.float32)))
    y16 = run(T, fm, image, params, precision=precision, out_dtype=torch.bfloat16)
    assert torch.equal(y16, torch.from_numpy(E["y"].astype(np.float32)).to(torch.bfloat16))   # one rounding of the exact value


# ---- seeded real data: the stage bars --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", range(len(TC.SHAPES)))
def test_stage_bars_at_every_shape(T, k, precision):
    b, h, w = TC.SHAPES[k]
    fm, image, params = TC.seeded(b, h, w, TC.COUTS[k % 4], seed=20 + k)
    hold_stages(T, fm, image, params, precision)


@pytest.mark.parametrize("image_dtype", DTYPES)
@pytest.mark.parametrize("fm_dtype", DTYPES)
def test_stage_bars_with_the_types_crossed(T, fm_dtype, image_dtype):
    fm, image, params = TC.seeded(2, 40, 56, 20, seed=31)
    fm, image = fm.to(fm_dtype), image.to(image_dtype)   # the restatement widens them exactly, as the kernel does
    for precision in PRECISIONS:
        hold_stages(T, fm, image, params, precision, out_dtypes=DTYPES)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", ["channels_last", "slices", "misaligned_out"])
def test_stage_bars_with_strided_inputs_and_a_misaligned_output(T, layout, precision):
    fm, image, params = TC.seeded(2, 40, 56, 18, seed=32)
    fm, image = fm.to(torch.bfloat16), image.to(torch.bfloat16)
    fm_d, im_d = fm.to(dev()), image.to(dev())
    if layout == "channels_last":
        fm_d, im_d = fm_d.contiguous(memory_format=torch.channels_last), im_d.contiguous(memory_format=torch.channels_last)
        assert not fm_d.is_contiguous() and not im_d.is_contiguous()
    elif layout == "slices":
        wide = torch.full((2, 40, 23, 33), float("nan"), dtype=torch.bfloat16, device=dev())
        wide[:, 3:35, 1:21, 2:30] = fm_d
        fm_d = wide[:, 3:35, 1:21, 2:30]
        wide_i = torch.full((2, 3, 40, 70), float("nan"), dtype=torch.bfloat16, device=dev())
        wide_i[:, :, :, 5:61] = im_d
        im_d = wide_i[:, :, :, 5:61]
    hold_stages(T, fm, image, params, precision, out_dtypes=(torch.float32, torch.bfloat16), fm_dev=fm_d, image_dev=im_d,
                misaligned=layout == "misaligned_out")


# ---- the geometry: the operand definition bit for bit, and a known answer ------------------------------------------------------------
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_f32_raw_under_identity_weights_is_the_float32_upsample_bit_for_bit(T, shape):
    b, h, w = shape
    fm = TC.seeded(b, h, w, 20, seed=40)[0]
    image = torch.randn(b, 3, h, w, generator=torch.Generator().manual_seed(41))
    for dt in DTYPES:   # every type is widened exactly
        f = fm.to(dt)
        up = TR.upsample(f)
        want = np.where(up > 0, up, up * np.float32(0.1))
        assert want.dtype == np.float32
        X = run(T, f, image, TC.identity_weights(), precision="f32", raw=True)
        assert torch.equal(X, torch.from_numpy(want)), dt


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ramp_known_answer(T, precision):
    for b, h, w in TC.SHAPES:
        fm, closed = TC.ramp(b, h // 2, w // 2)
        X = run(T, fm, torch.zeros(b, 3, h, w), TC.identity_weights(), precision=precision, raw=True).double().numpy()
        # (the bfloat16 tier rounds the operand once: at most 2^-8 of the value on top)
        lim = 8 * TR.U32 * closed + (TR.U_BF16 * (1 + 8 * TR.U32) * closed if precision == "bf16" else 0.0)
        assert (np.abs(X - closed) <= lim).all(), (b, h, w)


# ---- fixture G9: the reference's own outputs ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G9():
    fm, x, params, seg, ver = TC.g9()
    bound, y32 = TR.bf16_bound(fm, x, *params)
    return dict(fm=fm, x=x, params=params, ref=torch.from_numpy(np.concatenate([seg, ver], 1)), bound=bound, y32=y32)


def test_g9_f32_tier_under_the_fixtures_bar(T, G9):
    y = run(T, G9["fm"], G9["x"], G9["params"], precision="f32")
    assert tuple(y.shape) == (1, 20, 32, 48)
    assert torch.allclose(y, G9["ref"], atol=1e-5, rtol=1e-5)


def test_g9_bf16_tier_under_its_a_priori_bound(T, G9):
    y = run(T, G9["fm"], G9["x"], G9["params"], precision="bf16", out_dtype=torch.float32)
    ref = G9["ref"].double().numpy()
    # the bound is against the exact float32-operand tier; the fixture is pinned to that tier by its own bar, which comes on top
    lim = G9["bound"] + 1e-5 + 1e-5 * np.abs(ref)
    err = np.abs(y.double().numpy() - ref)
    print(f"G9 bf16: worst ratio to the a-priori bound {float((err / lim).max()):.3f}")
    assert (err <= lim).all()
    clear = np.abs(ref[:, 0] - ref[:, 1]) > 2 * np.maximum(lim[:, 0], lim[:, 1])
    assert clear.mean() > 0.5
    assert np.array_equal(y[:, :2].argmax(1).numpy()[clear], ref[:, :2].argmax(1)[clear])


# ---- the launch ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_and_out_is_returned(T):
    fm, image, params = TC.seeded(3, 34, 66, 20, seed=50)
    P = T.TailParams(*params)
    fm_d, im_d = fm.to(dev()).bfloat16(), image.to(dev()).bfloat16()
    for precision in PRECISIONS:
        a = T.fused_tail(fm_d, im_d, P, precision=precision)
        out = torch.full((3, 20, 34, 66), float("nan"), dtype=torch.bfloat16, device=dev())
        b_ = T.fused_tail(fm_d, im_d, P, precision=precision, out=out)
        assert b_ is out and a.dtype == torch.bfloat16
        assert torch.equal(a.view(torch.int16), out.view(torch.int16))   # bits, so that a NaN left behind would show
    with pytest.raises(RuntimeError):
        T.fused_tail(fm_d, im_d, P, out=torch.empty((3, 20, 34, 66), dtype=torch.float16, device=dev()), out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        T.fused_tail(fm_d, im_d[:, :, :-2], P)
    with pytest.raises(RuntimeError):
        T.fused_tail(fm_d, image.bfloat16(), P)   # a CPU tensor


def test_graph_capture_and_replay(T):
    fm, image, params = TC.seeded(2, 40, 56, 20, seed=51)
    fm2, image2, _ = TC.seeded(2, 40, 56, 20, seed=52)
    P = T.TailParams(*params)
    s_fm, s_im = fm.to(dev()).bfloat16(), image.to(dev()).bfloat16()
    want1 = T.fused_tail(s_fm, s_im, P).clone()   # (also uploads the weights before the capture)
    want2 = T.fused_tail(fm2.to(dev()).bfloat16(), image2.to(dev()).bfloat16(), P).clone()
    out = torch.zeros_like(want1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            T.fused_tail(s_fm, s_im, P, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        if k == 2:   # the inputs replaced in place
            s_fm.copy_(fm2.to(dev()))
            s_im.copy_(image2.to(dev()))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want2 if k == 2 else want1), k
