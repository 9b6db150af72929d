"""GPU tests of the head losses' backward on the device (pvnet_amd/validation.py, pvnet_amd/csrc/head_grad.hip).

Oracle 1: the float64 restatement (tests/head_grad_restatement.py), on the inputs as stored (``tensor.float()`` of half-precision
predictions).  Per element |device - f64| <= ulp of the output type at the value -- relative 2^-23 (float32), 2^-10 (float16), 2^-7
(bfloat16), or one subnormal step of the type where the value is that small.  Derived, not tuned: one correct rounding of the float64
value is half of it; the other half covers a float64 exp / division / sum order that lands the device's float64 value on the other
side of a rounding tie (the float64 values themselves agree to ~1e-15).  Exact zeros where the restatement has zeros, NaN exactly
where it has NaN, status equal.

Oracle 2: the reference's own float32 autograd recorded in tests/golden/head_grad.npz: |device - ref32| <= |ref32 - f64| + ulp(f64)
per element, the reference's own rounding distance read from the fixture.
"""
import os

import numpy as np
import pytest
import torch

from pvnet_amd import validation as V
from tests.head_grad_restatement import head_grad_f64, ulp
from tests.test_head_metrics_device import dev, host, random_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "head_grad.npz"))
CASES = [str(n) for n in GOLDEN["cases"]]
TYPE = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}


def upstream_for(b, d):
    """non-uniform per image, as a loss that weighs its images differently would send"""
    us, uv = np.linspace(0.5, 1.5, b), np.linspace(2.0, 0.25, b)
    return us, uv, torch.from_numpy(np.stack([us, uv], 1)).to(d)


def as_f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def compare(got, want, dtype, what):
    """one gradient tensor of the device (numpy float64 of the stored values) against the restatement's"""
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs"
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), f"{what}: a zero of the restatement is not zero"
    ok = ~nan
    err = np.abs(got[ok] - want[ok])
    bar = ulp(want[ok], TYPE[dtype])
    print(f"{what}: {ok.sum()} elements, max |device - f64| / ulp {float((err / bar).max()) if err.size else 0.0:.3f}")
    assert np.all(err <= bar), (what, float((err / bar).max()))


def check(inputs, sigma=1.0, what="", upstream=None, **kw):
    """device against the restatement on the same (stored) values; returns the device's (grad_seg, grad_vertex, status)"""
    seg, vp, mask, vt, vw = inputs
    b = seg.shape[0]
    us, uv, up = upstream_for(b, seg.device) if upstream is None else upstream
    gs, gv, status = V.head_grad_device(seg, vp, mask, vt, vw, up, sigma=sigma, **kw)
    torch.cuda.synchronize()
    ws, wv, wstatus = head_grad_f64(host(seg), host(vp), host(mask), host(vt), host(vw), us, uv, sigma)
    assert gs.dtype == seg.dtype and gv.dtype == vp.dtype and gs.shape == seg.shape and gv.shape == vp.shape
    compare(as_f64(gs), ws, seg.dtype, what + " grad_seg")
    compare(as_f64(gv), wv, vp.dtype, what + " grad_vertex")
    assert np.array_equal(status.cpu().numpy(), wstatus), what
    return gs, gv, status


def golden_inputs(name, d):
    g = GOLDEN
    return (torch.from_numpy(g[name + ".seg_pred"].astype(np.float32)).to(d), torch.from_numpy(g[name + ".vertex_pred"].astype(np.float32)).to(d),
            torch.from_numpy(g[name + ".mask"].astype(np.int64)).to(d), torch.from_numpy(g[name + ".vertex"].astype(np.float32)).to(d),
            torch.from_numpy(g[name + ".vertex_weights"].astype(np.float32)).to(d))


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_against_the_restatement_and_the_reference(name):
    d = dev()
    g = GOLDEN
    sigma = float(g[name + ".sigma"])
    us, uv = g[name + ".upstream_seg"], g[name + ".upstream_vertex"]
    up = torch.from_numpy(np.stack([us, uv], 1)).to(d)
    gs, gv, _ = check(golden_inputs(name, d), sigma, name, upstream=(us, uv, up))
    for got, key in ((gs, "grad_seg"), (gv, "grad_vertex")):
        got = as_f64(got)
        f64, ref32 = g[f"{name}.f64_{key}"], g[f"{name}.ref32_{key}"].astype(np.float64)
        # the reference's own float32 gradients: the only allowance is its own recorded rounding distance
        bound = np.abs(ref32 - f64) + ulp(f64, "float32")
        print(f"{name} {key}: |device - ref32| / bound max {np.max(np.abs(got - ref32) / bound):.3f}")
        assert np.all(np.abs(got - ref32) <= bound), (name, key)


def test_benchmark_size():
    check(random_inputs(2, 480, 640, 9, dev(), seed=1), 1.0, "480x640 vn=9 b=2")


@pytest.mark.parametrize("h,w", [(37, 53), (1, 1), (31, 33), (32, 33), (3, 1024), (65, 127)])
def test_odd_sizes(h, w):
    """h w not a multiple of the 1 024-pixel segment, of 8 or of 4"""
    check(random_inputs(3, h, w, 3, dev(), seed=h * w), 1.0, f"{h}x{w}")
    check(random_inputs(2, h, w, 2, dev(), seed=h + w, C=3), 2.0, f"{h}x{w} C=3 sigma=2")


def test_three_classes_on_the_fast_path():
    check(random_inputs(3, 48, 64, 2, dev(), seed=2, C=3), 1.0, "48x64 C=3")
    check(random_inputs(2, 40, 56, 3, dev(), seed=6, C=5), 0.7, "40x56 C=5 sigma=0.7")


def test_permuted_sliced_and_padded_inputs_and_outputs():
    d = dev()
    seg, vp, mask, vt, vw = random_inputs(2, 40, 56, 4, d, seed=5)
    us, uv, up = upstream_for(2, d)
    base = check((seg, vp, mask, vt, vw), 1.0, "contiguous")
    # channels-last predictions (a permuted view): empty_like keeps the layout, the gradients come channels-last
    seg_cl = seg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    vp_cl = vp.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wide = torch.zeros((2, 8, 48, 72), device=d)
    wide[:, :, 3:43, 9:65] = vt
    vt_cut = wide[:, :, 3:43, 9:65]
    mask_wide = torch.zeros((2, 40, 112), dtype=torch.int64, device=d)
    mask_wide[:, :, ::2] = mask
    mask_step = mask_wide[:, :, ::2]
    assert not seg_cl.is_contiguous() and not vt_cut.is_contiguous() and mask_step.stride(2) == 2
    got = check((seg_cl, vp_cl, mask_step, vt_cut, vw), 1.0, "permuted / sliced")
    assert got[0].stride() == seg_cl.stride() and got[1].stride() == vp_cl.stride()
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])   # per element the same float64 operations: bit for bit
    # contiguous inputs, gradients written into a window of a wider image and into channels-last storage
    out_wide = torch.full((2, 8, 48, 72), -7.0, device=d)
    out_cl = torch.full((2, 40, 56, 2), -7.0, device=d).permute(0, 3, 1, 2)
    V.head_grad_device(seg, vp, mask, vt, vw, up, out=(out_cl, out_wide[:, :, 3:43, 9:65]))
    torch.cuda.synchronize()
    assert torch.equal(out_cl, base[0]) and torch.equal(out_wide[:, :, 3:43, 9:65], base[1])
    frame = out_wide.clone()
    frame[:, :, 3:43, 9:65] = -7.0
    assert (frame == -7.0).all()   # nothing outside the window was written
    # every second image of a larger batch; weights expanded from one image (stride 0)
    big = [t.repeat_interleave(2, 0) for t in (seg, vp, mask, vt)]
    check((big[0][::2], big[1][::2], big[2][::2], big[3][::2], vw[:1].expand(2, -1, -1, -1)), 1.0, "batch stride / expanded weights")
    # a pixel count the fast path takes, planes that start 8 elements apart from where a dense tensor would put them: inputs and outputs
    pad = torch.zeros((2, 8, 40 * 56 + 8), device=d)
    pad[:, :, :40 * 56] = vp.reshape(2, 8, -1)
    vp_pad = pad[:, :, :40 * 56].view(2, 8, 40, 56)
    out_pad = torch.full((2, 8, 40 * 56 + 8), -7.0, device=d)
    gv_pad = out_pad[:, :, :40 * 56].view(2, 8, 40, 56)
    assert vp_pad.stride(1) == 40 * 56 + 8
    got = check((seg, vp_pad, mask, vt, vw), 1.0, "padded planes", out=(None, gv_pad))
    assert got[1] is gv_pad and torch.equal(gv_pad, base[1]) and torch.equal(got[0], base[0])
    assert (out_pad[:, :, 40 * 56:] == -7.0).all()


def test_misaligned_bases():
    """tensors that start at an address that is not a multiple of 16 bytes: the general path accesses element by element"""
    d = dev()
    seg, vp, mask, vt, vw = random_inputs(2, 24, 40, 3, d, seed=9, mask_dtype=torch.uint8)

    def shifted(t, k=1):
        flat = torch.zeros(t.numel() + k, dtype=t.dtype, device=d)
        flat[k:] = t.reshape(-1)
        out = flat[k:].view(t.shape)
        assert out.data_ptr() % 16 != 0
        return out

    base = check((seg, vp, mask, vt, vw), 1.0, "aligned")
    got = check((shifted(seg), shifted(vp), shifted(mask, 3), shifted(vt), shifted(vw)), 1.0, "misaligned")
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    for which in range(5):   # one misaligned tensor is enough to leave the fast path; the result stays right
        ts = [seg, vp, mask, vt, vw]
        ts[which] = shifted(ts[which], 3 if which == 2 else 1)
        check(tuple(ts), 1.0, f"misaligned tensor {which}")
    # aligned inputs, misaligned outputs
    us, uv, up = upstream_for(2, d)
    out = (shifted(torch.zeros_like(seg)), shifted(torch.zeros_like(vp)))
    V.head_grad_device(seg, vp, mask, vt, vw, up, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.bool, torch.int32, torch.int64])
@pytest.mark.parametrize("h,w", [(48, 64), (37, 53)])
def test_every_mask_dtype(mask_dtype, h, w):
    check(random_inputs(2, h, w, 3, dev(), seed=3, mask_dtype=mask_dtype), 1.0, f"{mask_dtype} {h}x{w}")
    if mask_dtype != torch.bool:
        check(random_inputs(3, h, w, 2, dev(), seed=4, C=3, mask_dtype=mask_dtype), 1.0, f"{mask_dtype} {h}x{w} C=3")


@pytest.mark.parametrize("pred_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("h,w", [(48, 64), (37, 53)])
def test_half_precision_predictions(pred_dtype, h, w):
    """read in place, gradients in that type; the value is the float32 call's float64 gradient x rounded once.  Against the float32
    call's STORED gradient g32 = x (1 + delta), |delta| <= 2^-24, the half-precision result RN(x) lies within half an ulp of the half
    type plus 2^-24 |x|: at most ulp(g32) (1/2 + 2^-13) for both types (2^-24 / 2^-10 = 2^-14 for float16, less for bfloat16, and
    the factor 1 + 2^-24 between |x| and |g32|); a subnormal step where the value is that small."""
    d = dev()
    seg, vp, mask, vt, vw = random_inputs(2, h, w, 4, d, seed=11, pred_dtype=pred_dtype)
    us, uv, up = upstream_for(2, d)
    gs, gv, _ = check((seg, vp, mask, vt, vw), 1.0, f"{pred_dtype} {h}x{w}")
    assert gs.dtype == pred_dtype and gv.dtype == pred_dtype
    check((seg.float(), vp, mask, vt, vw), 1.5, f"{pred_dtype} field, float32 logits")
    check((seg, vp.float(), mask, vt, vw), 0.5, f"{pred_dtype} logits, float32 field")
    gs32, gv32, _ = V.head_grad_device(seg.float(), vp.float(), mask, vt, vw, up)
    torch.cuda.synchronize()
    for half, full, what in ((gs, gs32, "grad_seg"), (gv, gv32, "grad_vertex")):
        half, full = as_f64(half), as_f64(full)
        bar = ulp(full, TYPE[pred_dtype]) * (0.5 + 2.0 ** -13)
        print(f"{pred_dtype} {what}: |half - float32| / (ulp / 2) max {float((np.abs(half - full) / bar).max()):.4f}; "
              f"equal to the float32 gradient rounded again in {float((half == as_f64(torch.from_numpy(full).to(pred_dtype))).mean()):.6f} of the elements")
        assert np.all(np.abs(half - full) <= bar), what


def test_nan_and_bad_labels():
    d = dev()
    for h, w in ((48, 64), (37, 53)):   # fast and general path
        seg, vp, mask, vt, vw = random_inputs(4, h, w, 2, d, seed=13)
        seg[0, 1, 5, 7] = float("nan")     # a NaN logit: both gradients of the pixel NaN
        vp[1, 2, 4, 4] = float("nan")      # a NaN in the field: takes the second branch, that element NaN
        vw[1, 0, 4, 4] = 1.0
        vt[1, 3, 6, 6] = float("nan")      # a NaN target under weight 0: 0 * NaN is NaN, as written
        mask[2, 3, 3] = 2                  # labels outside 0..1
        mask[2, 8, 9] = -1
        gs, gv, status = check((seg, vp, mask, vt, vw), 1.0, f"NaN / bad labels {h}x{w}")
        assert torch.isnan(gs[0, :, 5, 7]).all() and int(torch.isnan(gs[0]).sum()) == 2
        assert torch.isnan(gv[1, 2, 4, 4]) and torch.isnan(gv[1, 3, 6, 6]) and int(torch.isnan(gv).sum()) == 2
        assert torch.isnan(gs[2, :, 3, 3]).all() and torch.isnan(gs[2, :, 8, 9]).all() and int(torch.isnan(gs[2]).sum()) == 4
        assert status.tolist() == [0, 0, V.HEAD_S_BAD_LABEL, 0]
        assert torch.isfinite(gs[3]).all() and torch.isfinite(gv[3]).all()
        m8 = mask.clamp(min=0).to(torch.uint8)   # uint8 labels above C-1
        m8[3, 0, 0] = 255
        _, _, status = check((seg, vp, m8, vt, vw), 1.0, "uint8 bad labels")
        assert status.tolist() == [0, 0, 1, 1]
        # zero upstream gradients: zeros, except where the definition gives NaN
        zero = (np.zeros(4), np.zeros(4), torch.zeros((4, 2), dtype=torch.float64, device=d))
        gs, gv, _ = check((seg, vp, mask, vt, vw), 1.0, "zero upstream", upstream=zero)
        assert (gs[3] == 0).all() and (gv[3] == 0).all()


def test_garbage_workspace_two_calls_bitwise_equal_out_tensors_and_need():
    d = dev()
    inputs = random_inputs(3, 96, 128, 9, d, seed=17)
    us, uv, up = upstream_for(3, d)
    n = V.head_grad_workspace_bytes(3, 96, 128)
    results = []
    for fill in (0xFF, 0x7F):   # NaN patterns / set flags if anything of the workspace were read before it is written
        ws = torch.full((n,), fill, dtype=torch.uint8, device=d)
        out = (torch.full_like(inputs[0], -1.0), torch.full_like(inputs[1], -1.0))
        got = V.head_grad_device(*inputs, up, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert got[0] is out[0] and got[1] is out[1]
        results.append([t.clone() for t in got])
    assert all(torch.equal(a, b) for a, b in zip(*results))
    fresh = check(inputs, 1.0, "96x128 vn=9")
    assert all(torch.equal(a, b) for a, b in zip(fresh, results[0]))
    assert (results[0][2] == 0).all()
    # the measurement aids change which accesses are non-temporal, nothing else
    for flags in (V.HEAD_F_NT_NONE, V.HEAD_F_NT_ALL):
        other = V.head_grad_device(*inputs, up, flags=flags)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(other, results[0]))
    # one half only: the other tensor is not touched, the half that runs gives the same bits
    for need in ((True, False), (False, True)):
        out = (torch.full_like(inputs[0], -3.0), torch.full_like(inputs[1], -3.0))
        got = V.head_grad_device(*inputs, up, need=need, out=out)
        torch.cuda.synchronize()
        k = 0 if need[0] else 1
        assert got[k] is out[k] and got[1 - k] is None and torch.equal(out[k], results[0][k])
        assert (out[1 - k] == -3.0).all()
        alone = V.head_grad_device(*inputs, up, need=need)
        torch.cuda.synchronize()
        assert alone[1 - k] is None and torch.equal(alone[k], results[0][k]) and (alone[2] == 0).all()
    with pytest.raises(RuntimeError, match="need"):
        V.head_grad_device(*inputs, up, need=(False, False))
    with pytest.raises(RuntimeError, match="PVNET_E_WORKSPACE"):
        V.head_grad_device(*inputs, up, workspace=torch.empty(n - 256, dtype=torch.uint8, device=d))
    with pytest.raises(RuntimeError, match="out\\[1\\]"):
        V.head_grad_device(*inputs, up, out=(None, torch.empty_like(inputs[1], dtype=torch.float16)))
    with pytest.raises(RuntimeError, match="upstream"):
        V.head_grad_device(*inputs, up.float())
    empty = V.head_grad_device(*[t[:0] for t in inputs], up[:0])
    assert empty[0].shape == (0, 2, 96, 128) and empty[1].shape == (0, 18, 96, 128) and empty[2].shape == (0,)


def test_call_leaves_the_stream_unsynchronised():
    """the call only enqueues: behind a long-running kernel on the same stream it returns while that kernel still runs"""
    d = dev()
    inputs = random_inputs(2, 96, 128, 4, d, seed=19)
    us, uv, up = upstream_for(2, d)
    V.head_grad_device(*inputs, up)   # (library loaded, allocator warm)
    torch.cuda.synchronize()
    out = (torch.empty_like(inputs[0]), torch.empty_like(inputs[1]))
    ws = torch.empty(V.head_grad_workspace_bytes(2, 96, 128), dtype=torch.uint8, device=d)
    torch.cuda._sleep(50_000_000)   # a spin kernel of tens of milliseconds at the least: the call below takes well under one
    done = torch.cuda.Event()
    V.head_grad_device(*inputs, up, out=out, workspace=ws)
    done.record()
    assert not done.query(), "head_grad_device waited for the stream"
    torch.cuda.synchronize()
    assert done.query()


def torch_losses(seg_pred, vertex_pred, mask, vertex, vertex_weights, sigma):
    """the reference's formula (tools/train_linemod.py:87-89, net_utils.py:66-74) in torch, in the dtype of its arguments"""
    b = seg_pred.shape[0]
    loss_seg = torch.nn.functional.cross_entropy(seg_pred, mask, reduction="none").view(b, -1).mean(1)
    s2 = sigma * sigma
    diff = vertex_weights * (vertex_pred - vertex)
    a = diff.abs()
    near = (a < 1.0 / s2).detach().to(diff.dtype)
    in_loss = diff.pow(2) * (s2 / 2.0) * near + (a - 0.5 / s2) * (1.0 - near)
    loss_vertex = in_loss.view(b, -1).sum(1) / (vertex_pred.shape[1] * vertex_weights.view(b, -1).sum(1) + 1e-3)
    return loss_seg, loss_vertex


def test_module_values_are_those_of_head_metrics_and_only_the_losses_are_differentiable():
    d = dev()
    inputs = random_inputs(3, 48, 64, 9, d, seed=23)
    seg, vp = inputs[0].clone().requires_grad_(True), inputs[1].clone().requires_grad_(True)
    got = V.HeadLoss(sigma=2.0)(seg, vp, *inputs[2:])
    want = V.HeadMetrics(sigma=2.0)(*inputs)
    torch.cuda.synchronize()
    assert len(got) == 4
    for k, (a, c) in enumerate(zip(got, want)):
        assert a.dtype == torch.float32 and tuple(a.shape) == (3,) and torch.equal(a, c), k
    assert got[0].grad_fn is not None and got[1].grad_fn is not None and got[0].requires_grad and got[1].requires_grad
    assert not got[2].requires_grad and not got[3].requires_grad and got[2].grad_fn is None and got[3].grad_fn is None
    plain = V.HeadLoss()(*inputs)   # nothing asks for a gradient: nothing is recorded
    assert all(not t.requires_grad for t in plain)
    with pytest.raises(RuntimeError):   # once-differentiable: no double backward
        g, = torch.autograd.grad(got[0].sum(), seg, create_graph=True)
        g.sum().backward()


@pytest.mark.parametrize("sigma", [1.0, 0.6])
def test_backward_equals_the_function_and_torchs_own_autograd(sigma):
    """``mean(loss_seg) + 0.5 mean(loss_vertex)``: its backward through HeadLoss IS head_grad_device with upstream (1/b, 0.5/b), and
    agrees with torch's own autograd of the same formula in float64 on the device within the bar of the restatement.  torch's
    cross-entropy backward forms softmax - 1 for the label's class, whose float64 rounding error 2^-53 is e^margin 2^-53 of the value;
    the logits here are scaled to margins below 8, which keeps that below 1e-5 of a float32 ulp."""
    d = dev()
    b = 4
    inputs = list(random_inputs(b, 48, 64, 4, d, seed=29))
    inputs[0] = inputs[0] * 0.25
    seg, vp = inputs[0].clone().requires_grad_(True), inputs[1].clone().requires_grad_(True)
    loss_seg, loss_vertex, _, _ = V.HeadLoss(sigma=sigma)(seg, vp, *inputs[2:])
    (loss_seg.mean() + 0.5 * loss_vertex.mean()).backward()
    up = torch.tensor([[1.0 / b, 0.5 / b]] * b, dtype=torch.float32, device=d).to(torch.float64)   # what autograd sends, in float32
    gs, gv, _ = V.head_grad_device(*inputs, up, sigma=sigma)
    torch.cuda.synchronize()
    assert torch.equal(seg.grad, gs) and torch.equal(vp.grad, gv)
    s64, p64 = inputs[0].double().requires_grad_(True), inputs[1].double().requires_grad_(True)
    ls, lv = torch_losses(s64, p64, inputs[2], inputs[3].double(), inputs[4].double(), sigma)
    ((ls * up[:, 0]).sum() + (lv * up[:, 1]).sum()).backward()
    margin = float((inputs[0][:, 0] - inputs[0][:, 1]).abs().max())
    assert margin < 8.0
    compare(as_f64(seg.grad), s64.grad.cpu().numpy(), torch.float32, f"sigma={sigma} torch float64 autograd, grad_seg")
    compare(as_f64(vp.grad), p64.grad.cpu().numpy(), torch.float32, f"sigma={sigma} torch float64 autograd, grad_vertex")
    # only one of the two inputs asks for a gradient: that half runs, with the same bits
    seg2 = inputs[0].clone().requires_grad_(True)
    loss_seg, loss_vertex, _, _ = V.HeadLoss(sigma=sigma)(seg2, inputs[1], *inputs[2:])
    (loss_seg.mean() + 0.5 * loss_vertex.mean()).backward()
    assert torch.equal(seg2.grad, gs)
    vp2 = inputs[1].clone().requires_grad_(True)
    loss_seg, loss_vertex, _, _ = V.HeadLoss(sigma=sigma)(inputs[0], vp2, *inputs[2:])
    loss_vertex.mean().mul(0.5).backward()   # loss_seg takes no part: its incoming gradient is zeros
    assert torch.equal(vp2.grad, gv)


@pytest.mark.parametrize("pred_dtype", [torch.float32, torch.bfloat16])
def test_packed_equals_the_two_tensor_entry_and_its_gradient_arrives_in_the_parent(pred_dtype):
    d = dev()
    b, C = 2, 2
    seg, vp, mask, vt, vw = random_inputs(b, 48, 64, 4, d, seed=31, pred_dtype=pred_dtype)
    head_out = torch.cat([seg, vp], 1).requires_grad_(True)
    loss = V.HeadLoss(sigma=1.0)
    got = loss.packed(head_out, C, mask, vt, vw)
    (got[0].mean() + 0.5 * got[1].mean()).backward()
    parent = head_out.detach().clone().requires_grad_(True)
    two = loss(parent[:, :C], parent[:, C:], mask, vt, vw)   # the reference's slices: torch's slice backward pads and adds
    (two[0].mean() + 0.5 * two[1].mean()).backward()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(got, two))
    assert head_out.grad is not None and head_out.grad.shape == head_out.shape and head_out.grad.dtype == pred_dtype
    assert torch.equal(head_out.grad, parent.grad)
    up = torch.tensor([[1.0 / b, 0.5 / b]] * b, dtype=torch.float32, device=d).to(torch.float64)
    gs, gv, _ = V.head_grad_device(seg, vp, mask, vt, vw, up)
    torch.cuda.synchronize()
    assert torch.equal(head_out.grad[:, :C], gs) and torch.equal(head_out.grad[:, C:], gv)
    with pytest.raises(RuntimeError, match="seg_dim"):
        loss.packed(head_out, 1, mask, vt, vw)


def test_graph_of_forward_and_backward_replays_bitwise_eager():
    """PyTorch's rules for capturing a backward hold (torch.cuda.graph, "whole network capture"): a warm-up step on a side stream, and
    no autograd graph from outside the capture alive when it begins -- the leaf's gradient accumulator belongs to the stream it was
    created on, and one left over from an eager step would pull the default stream into the capture.  So ``step`` hands out detached
    tensors only: its graph dies with it."""
    d = dev()
    b = 4
    seg, vp, mask, vt, vw = random_inputs(b, 96, 128, 9, d, seed=37)
    head_out = torch.cat([seg, vp], 1).requires_grad_(True)
    loss = V.HeadLoss()

    def step():
        head_out.grad = None
        ls, lv, pr, rc = loss.packed(head_out, 2, mask, vt, vw)
        total = ls.mean() + 0.5 * lv.mean()
        total.backward()
        return [t.detach() for t in (total, ls, lv, pr, rc, head_out.grad)]   # (views of the same storage)

    eager = []
    for _ in range(2):
        out = step()
        torch.cuda.synchronize()
        eager.append([t.clone() for t in out])
    del out
    assert all(torch.equal(a, c) for a, c in zip(*eager))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    head_out.grad = None
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, a, c in zip(("total", "loss_seg", "loss_vertex", "precision", "recall", "gradient"), captured, eager[0]):
        assert torch.equal(a, c), name
    assert torch.isfinite(captured[5]).all() and float(captured[5].abs().max()) > 0.0
