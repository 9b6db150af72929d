"""GPU tests of the fused decoder stages (pvnet_amd/decoder.py, pvnet_amd/csrc/decoder.hip, libpvnet_decoder.so) against the restatement
of include/pvnet_decoder.h (tests/decoder_restatement.py).

No tolerance here is measured on the device code.  One-hot weights must give the shifted, rounded, activated operand itself
(``torch.equal``): that pins the upsample bit for bit, the concatenation's order, the taps and the padding through the one tier the
library has.  Exact integer data must come out as THE integers.  Seeded real data at a trained decoder's scales is held, every element,
to the a-priori bar of the tail's first stage.  The network test compares with eager PyTorch, never with the code under test."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import decoder_cases as DC  # noqa: E402
from tests import decoder_restatement as DR  # noqa: E402

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
CASES = [(shape, triple) for triple in DC.TRIPLES for shape in DC.SHAPES]
case_ids = [f"{DC.STAGE_OF[t]}-{b}x{h}x{w}" for (b, h, w), t in CASES]


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import decoder
    return decoder


def dev():
    return torch.device("cuda:0")


def run(D, lo, skip, params, **kw):
    """fused_stage on device copies (or on the given device tensors) -> the result on the CPU"""
    P = params if isinstance(params, D.StageParams) else D.StageParams(*params)
    lo = lo if lo.is_cuda else lo.to(dev())
    skip = skip if skip.is_cuda else skip.to(dev())
    out = D.fused_stage(lo, skip, P, **kw)
    torch.cuda.synchronize()
    return out.cpu()


def hold(D, lo, skip, params, triple, out_dtypes=(torch.float32,), lo_dev=None, skip_dev=None, misaligned=False, what=""):
    """the bar, every element; lo / skip are the CPU tensors the restatement reads, *_dev what the device reads instead"""
    cl, cs, co = triple
    E = DR.stage_exact(lo, skip, *params)
    b, h, w = skip.shape[0], skip.shape[2], skip.shape[3]
    P = D.StageParams(*params)
    for dt in out_dtypes:
        kw = dict(out_dtype=dt)
        if misaligned:   # starts one element past an aligned address
            kw["out"] = torch.empty(b * co * h * w + 1, dtype=dt, device=dev())[1:].view(b, co, h, w)
        y = run(D, lo if lo_dev is None else lo_dev, skip if skip_dev is None else skip_dev, P, **kw)
        assert y.dtype == dt and tuple(y.shape) == (b, co, h, w) and y.is_contiguous()
        err, lim = np.abs(y.double().numpy() - E["out"]), DR.bar(E["A"], DR.terms(cl, cs), E["out"], dt)
        print(f"{DC.STAGE_OF[triple]} {what} {dt}: worst ratio to the bar {float((err / np.maximum(lim, 1e-300)).max()):.3f}")
        assert (err <= lim).all(), dt


# ---- one-hot weights: the geometry and the operand definition, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("shape,triple", CASES, ids=case_ids)
def test_one_hot_weights_give_the_shifted_rounded_operand_itself(D, shape, triple):
    b, h, w = shape
    lo, skip, _ = DC.seeded(b, h, w, triple, seed=80)
    taps, wt, bias = DC.onehot(triple, seed=81 + h)
    want = DR.onehot_expected(DR.bf16_round(DR.concat(lo, skip)), taps)
    assert (want < 0).any() and (want > 0).any()
    y = run(D, lo, skip, (wt, bias), out_dtype=torch.float32)
    assert torch.equal(y, torch.from_numpy(want))
    if shape == DC.SHAPES[2]:   # the half types in are widened exactly
        for dt in (torch.float16, torch.bfloat16):
            l, s = lo.to(dt), skip.to(dt)
            y = run(D, l, s, (wt, bias), out_dtype=torch.float32)
            assert torch.equal(y, torch.from_numpy(DR.onehot_expected(DR.bf16_round(DR.concat(l, s)), taps))), dt


# ---- exact integer data --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,triple", CASES, ids=case_ids)
def test_integer_data_comes_out_as_the_integers(D, shape, triple):
    b, h, w = shape
    cl, cs, co = triple
    assert 9 * (cl + cs) * DC.INT_W * DC.INT_X <= 1728 * 128 * 4 < 2 ** 20
    lo, skip, params = DC.integers(b, h, w, triple, seed=11)
    E = DR.stage_exact(lo, skip, *params)
    # integral operands, no negative pre-activation, and every partial sum in any order below 2^24
    assert np.array_equal(E["In"], np.rint(E["In"])) and (E["pre"] > 0).all() and E["A"].max() + float(params[1].max()) < 2 ** 24
    assert np.array_equal(E["out"], np.rint(E["out"]))
    y = run(D, lo, skip, params, out_dtype=torch.float32)
    assert torch.equal(y, torch.from_numpy(E["out"].astype(np.float32)))
    y16 = run(D, lo, skip, params, out_dtype=torch.bfloat16)
    assert torch.equal(y16, torch.from_numpy(E["out"].astype(np.float32)).to(torch.bfloat16))   # one rounding of the exact value


# ---- seeded real data: the a-priori bar ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,triple", CASES, ids=case_ids)
def test_bar_at_every_shape(D, shape, triple):
    b, h, w = shape
    lo, skip, params = DC.seeded(b, h, w, triple, seed=20 + h)
    hold(D, lo, skip, params, triple, what=f"{b}x{h}x{w}")


@pytest.mark.parametrize("skip_dtype", DTYPES)
@pytest.mark.parametrize("lo_dtype", DTYPES)
def test_bar_with_the_types_crossed(D, lo_dtype, skip_dtype):
    for triple in DC.TRIPLES:
        lo, skip, params = DC.seeded(2, 40, 56, triple, seed=31)
        lo, skip = lo.to(lo_dtype), skip.to(skip_dtype)   # the restatement widens them exactly, as the kernel does
        hold(D, lo, skip, params, triple, out_dtypes=DTYPES, what=f"{lo_dtype} x {skip_dtype}")


@pytest.mark.parametrize("triple", DC.TRIPLES, ids=list(DC.STAGE_OF.values()))
@pytest.mark.parametrize("layout", ["channels_last", "slices", "misaligned_out"])
def test_bar_with_strided_inputs_and_a_misaligned_output(D, layout, triple):
    cl, cs, _ = triple
    lo, skip, params = DC.seeded(2, 40, 56, triple, seed=32)
    lo, skip = lo.to(torch.bfloat16), skip.to(torch.bfloat16)
    lo_d, sk_d = lo.to(dev()), skip.to(dev())
    if layout == "channels_last":
        lo_d, sk_d = lo_d.contiguous(memory_format=torch.channels_last), sk_d.contiguous(memory_format=torch.channels_last)
        assert not lo_d.is_contiguous() and not sk_d.is_contiguous()
    elif layout == "slices":   # a channel slice of a wider tensor, and a window of a larger plane; NaN around both
        wide = torch.full((2, cl + 8, 23, 33), float("nan"), dtype=torch.bfloat16, device=dev())
        wide[:, 3:3 + cl, 1:21, 2:30] = lo_d
        lo_d = wide[:, 3:3 + cl, 1:21, 2:30]
        wide_s = torch.full((2, cs + 5, 40, 70), float("nan"), dtype=torch.bfloat16, device=dev())
        wide_s[:, 5:, :, 5:61] = sk_d
        sk_d = wide_s[:, 5:, :, 5:61]
    hold(D, lo, skip, params, triple, out_dtypes=DTYPES, lo_dev=lo_d, skip_dev=sk_d, misaligned=layout == "misaligned_out", what=layout)


# ---- the launch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", DC.TRIPLES, ids=list(DC.STAGE_OF.values()))
def test_calls_are_bitwise_equal_whatever_the_weights_layout_and_out_is_returned(D, triple):
    _, _, co = triple
    lo, skip, params = DC.seeded(3, 34, 66, triple, seed=50)
    P = D.StageParams(*params)
    lo_d, sk_d = lo.to(dev()).bfloat16(), skip.to(dev()).bfloat16()
    a = D.fused_stage(lo_d, sk_d, P)
    out = torch.full((3, co, 34, 66), float("nan"), dtype=torch.bfloat16, device=dev())
    b_ = D.fused_stage(lo_d, sk_d, P, out=out)
    assert b_ is out and a.dtype == torch.bfloat16
    assert torch.equal(a.view(torch.int16), out.view(torch.int16))   # bits, so that a NaN left behind would show
    # the float32 weights, gathered and rounded by the kernel: the same operands in the same order, so the same bits
    c = D.fused_stage(lo_d, sk_d, P, packed=False, out_dtype=torch.float32)
    assert torch.equal(c, D.fused_stage(lo_d, sk_d, P, out_dtype=torch.float32))
    # a pixel's arithmetic does not depend on the launch's shape: one image of the batch alone, and a window's interior
    one = D.fused_stage(lo_d[1:2], sk_d[1:2], P)
    assert torch.equal(one.view(torch.int16), a[1:2].view(torch.int16))
    with pytest.raises(RuntimeError):
        D.fused_stage(lo_d, sk_d, P, out=torch.empty((3, co, 34, 66), dtype=torch.float16, device=dev()), out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        D.fused_stage(lo_d, sk_d[:, :, :-2], P)
    with pytest.raises(RuntimeError):
        D.fused_stage(lo_d, sk_d[:, :-1], P)
    with pytest.raises(RuntimeError):
        D.fused_stage(lo_d, skip.bfloat16(), P)   # a CPU tensor
    with pytest.raises(RuntimeError):
        D.fused_stage(lo_d, sk_d, D.StageParams(*DC.seeded(1, 2, 2, DC.TRIPLES[triple == DC.TRIPLES[0]], seed=1)[2]))   # the other stage's


def test_graph_capture_and_replay(D):
    triple = DC.TRIPLES[1]
    lo, skip, params = DC.seeded(2, 40, 56, triple, seed=51)
    lo2, skip2, _ = DC.seeded(2, 40, 56, triple, seed=52)
    P = D.StageParams(*params)
    s_lo, s_sk = lo.to(dev()).bfloat16(), skip.to(dev()).bfloat16()
    want1 = D.fused_stage(s_lo, s_sk, P).clone()   # (also uploads the weights before the capture)
    want2 = D.fused_stage(lo2.to(dev()).bfloat16(), skip2.to(dev()).bfloat16(), P).clone()
    assert not torch.equal(want1, want2)
    out = torch.zeros_like(want1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            D.fused_stage(s_lo, s_sk, P, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        if k == 2:   # the inputs replaced in place
            s_lo.copy_(lo2.to(dev()))
            s_sk.copy_(skip2.to(dev()))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want2 if k == 2 else want1), k
