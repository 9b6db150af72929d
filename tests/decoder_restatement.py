"""A numpy / torch-CPU restatement of include/pvnet_decoder.h, written from the header: the float32 upsample operation for operation
(the tail's, word for word: tests/tail_restatement.py holds it and is held to torch's own interpolation there), the concatenation with
the upsampled channels first, the one rounding of every operand to bfloat16, the convolution's sum in float64 (the sums are defined up
to their order, so float64 stands for "any order"), the activation, and the absolute-value sum the tests' bar is made of.  Nothing here
is measured on the device code.

Bar (u32 = 2^-24, K = 9 (cl + cs) terms of an output element):
    |out_dev - out_exact| <= 2 (K + 3) u32 A  (+ u_out |out| for a half-type out)        A = sum |w| |in| over the rounded operands
(K + 3) u is the bound of a float32 sum of K terms in any order plus the bias and the activation's product; the factor 2 stands for the
matrix pipe's partial sums, whose rounding is not documented -- the bar tests/tail_restatement.py states for the tail's first stage.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.tail_restatement import SLOPE, U32, U_BF16, U_OUT, bf16_round, f32, upsample  # noqa: F401  (re-exported for the tests)

MISTAKES = ("align_corners_false", "skip_first", "taps_transposed", "slope_0.01", "pad_before_upsample")


def terms(cl, cs):
    return 9 * (cl + cs)


def concat(lo, skip):
    """In [b,cl+cs,h,w] float32: the upsampled channels FIRST, then skip's"""
    return np.concatenate([upsample(lo), f32(skip)], 1)


def _conv3(In, w):   # float64, zero padding of 1 on In
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(In)), torch.from_numpy(np.ascontiguousarray(w)), padding=1).numpy()


def activate(pre, slope=SLOPE):
    return np.where(pre > 0, pre, pre * slope)


def stage_exact(lo, skip, w, bias, slope=SLOPE):
    """the stage in float64 on the operands the kernel multiplies: dict(In, w: the rounded operands as float64; pre; out: after the
    activation; A: sum |w| |in|)"""
    In = bf16_round(concat(lo, skip)).astype(np.float64)
    wq = bf16_round(f32(w)).astype(np.float64)
    pre = _conv3(In, wq) + f32(bias).astype(np.float64)[None, :, None, None]
    return dict(In=In, w=wq, pre=pre, out=activate(pre, slope), A=_conv3(np.abs(In), np.abs(wq)))


def bar(A, K, out=None, out_dtype=torch.float32):
    """the a-priori bar of every output element; a half-type out adds that type's one rounding of the value"""
    lim = 2 * (K + 3) * U32 * A
    return lim if out_dtype == torch.float32 else lim + U_OUT[out_dtype] * np.abs(out)


def onehot_expected(In, taps):
    """With w[o][c][ky][kx] = 1 for the one (c, ky, kx) = taps[o] of every output channel, bias 0: out[o](Y, X) =
    act(In[c](Y + ky - 1, X + kx - 1)), In (already rounded) zero outside the image -- as float32, bit for bit (the one product 1 * x
    and the sum with zeros are exact; a negative value takes the one rounding of v * 0.1f)."""
    In = np.asarray(In, dtype=np.float32)
    b, _, h, w = In.shape
    ring = np.pad(In, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.stack([ring[:, c, ky:ky + h, kx:kx + w] for c, ky, kx in taps], 1)
    res = np.where(out > 0, out, out * np.float32(0.1))
    assert res.dtype == np.float32
    return res


# ---- planted mistakes: what a wrong kernel would compute, for the tests that show the bars catch it -------------------------------------
def mistaken(lo, skip, w, bias, mistake):
    """the stage in float64 with one planted mistake: "align_corners_false", "skip_first" (the concatenation's halves in the wrong
    order), "taps_transposed", "slope_0.01", or "pad_before_upsample" (the zero ring lies around the half-resolution features: an output
    pixel outside the image is half way between the edge and that ring, so it holds half the edge's upsampled value instead of 0; the
    skip part stays 0)"""
    assert mistake in MISTAKES
    up, sk, w = upsample(lo), f32(skip), f32(w)
    cl = up.shape[1]
    slope = float(np.float32(0.01)) if mistake == "slope_0.01" else SLOPE
    if mistake == "align_corners_false":
        up = F.interpolate(torch.from_numpy(f32(lo)), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    In = np.concatenate([sk, up] if mistake == "skip_first" else [up, sk], 1)
    if mistake == "taps_transposed":
        w = np.ascontiguousarray(np.swapaxes(w, -1, -2))
    In, wq = bf16_round(In).astype(np.float64), bf16_round(w).astype(np.float64)
    b_ = f32(bias).astype(np.float64)[None, :, None, None]
    if mistake == "pad_before_upsample":
        ring = np.pad(In, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge") * 0.5
        ring[:, cl:] = 0.0
        ring[:, :, 1:-1, 1:-1] = In
        return activate(F.conv2d(torch.from_numpy(ring), torch.from_numpy(wq)).numpy() + b_, slope)
    return activate(_conv3(In, wq) + b_, slope)
