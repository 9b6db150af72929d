"""A numpy restatement of include/pvnet_trunk.h, written from the header: the concatenation with src1 first, the one rounding of every
operand to bfloat16, the strided, dilated 3 x 3 sum tap by tap in float64 (the sums are defined up to their order, so float64 stands for
"any order"), the residual, the activation, and the magnitude the tests' bar is made of.  Nothing here is measured on the device code;
tests/test_trunk_cpu.py holds it to torch's own float64 ``F.conv2d``.

Bar (u32 = 2^-24, K = 9 cin terms of an output element):
    |out_dev - out_exact| <= 2 (K + 4) u32 A  (+ u_out |out| for a half-type out)        A = |bias| + sum |w| |in| + |res|
(K + 4) u is the bound of a float32 sum of K terms in any order plus the bias, the residual's addition and the activation's product;
the factor 2 stands for the matrix pipe's partial sums, whose rounding is not documented -- the decoder's bar
(tests/decoder_restatement.py) with one more term for the residual.
"""
import numpy as np
import torch

from tests.tail_restatement import SLOPE, U32, U_BF16, U_OUT, bf16_round, f32  # noqa: F401  (re-exported for the tests)

ACTS = ("none", "relu", "leaky")
MISTAKES = ("dilation_on_padding_only", "origin_2Y", "residual_after_act", "taps_transposed", "src2_first", "relu_for_leaky")


def out_sizes(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def wide(t):
    """a tensor or array of one of the three types widened exactly to float32; a float64 array (the unrounded route's own intermediate
    results) stays as it is"""
    return t if isinstance(t, np.ndarray) and t.dtype == np.float64 else f32(t)


def concat(src1, src2=None):
    """In [b,c1+c2,h,w]: src1's channels FIRST, then src2's"""
    return wide(src1) if src2 is None else np.concatenate([wide(src1), wide(src2)], 1)


def conv3(In, w, s, d, tap_step=None, origin=None):
    """sum over c, ky, kx of w[o][c][ky][kx] In[c](s Y + origin + tap_step ky, s X + origin + tap_step kx) in float64, In zero outside
    the image.  The header's convolution has tap_step = d and origin = -d; the planted mistakes pass others."""
    tap_step = d if tap_step is None else tap_step
    origin = -d if origin is None else origin
    In, w = np.asarray(In, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b, _, h, wd = In.shape
    ho, wo = out_sizes(h, wd, s)
    pad = 2 * d + 2
    ring = np.pad(In, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((b, w.shape[0], ho, wo))
    for ky in range(3):
        for kx in range(3):
            y0, x0 = pad + origin + tap_step * ky, pad + origin + tap_step * kx
            win = ring[:, :, y0:y0 + s * (ho - 1) + 1:s, x0:x0 + s * (wo - 1) + 1:s]
            out += np.einsum("oc,bchw->bohw", w[:, :, ky, kx], win)
    return out


def activate(v, act):
    assert act in ACTS
    if act == "relu":
        return np.where(v <= 0, 0.0, v)    # the header's wording: a NaN compares false and stays
    if act == "leaky":
        return np.where(v > 0, v, v * SLOPE)
    return v


def conv_exact(src1, w, bias, s, d, act, src2=None, res=None, rounded=True):
    """the launch in float64 on the operands the kernel multiplies (``rounded=False``: on the operands as given -- the network's own
    float32 arithmetic up to its rounding): dict(In, w: the operands as float64; pre: before the activation; out; A: |bias| +
    sum |w| |in| + |res|)"""
    In, wq = concat(src1, src2), f32(w)
    if rounded:
        In, wq = bf16_round(In), bf16_round(wq)
    In, wq = In.astype(np.float64), wq.astype(np.float64)
    b_ = f32(bias).astype(np.float64)[None, :, None, None]
    pre = conv3(In, wq, s, d) + b_
    A = conv3(np.abs(In), np.abs(wq), s, d) + np.abs(b_)
    if res is not None:
        r = wide(res).astype(np.float64)
        pre, A = pre + r, A + np.abs(r)
    return dict(In=In, w=wq, pre=pre, out=activate(pre, act), A=A)


def terms(cin):
    return 9 * cin


def bar(A, cin, out=None, out_dtype=torch.float32):
    """the a-priori bar of every output element; a half-type out adds that type's one rounding of the value"""
    lim = 2 * (terms(cin) + 4) * U32 * A
    return lim if out_dtype == torch.float32 else lim + U_OUT[out_dtype] * np.abs(out)


def onehot_expected(In, taps, s, d):
    """With w[o][c][ky][kx] = sign for the one (c, ky, kx, sign) = taps[o] of every output channel, bias 0 and no activation: out[o](Y, X)
    = sign * In[c](s Y + d (ky - 1), s X + d (kx - 1)), In (already rounded) zero outside the image -- as float32, bit for bit (the one
    product and the sum with zeros are exact)."""
    In = np.asarray(In, dtype=np.float32)
    b, _, h, w = In.shape
    ho, wo = out_sizes(h, w, s)
    ring = np.pad(In, ((0, 0), (0, 0), (d, d), (d, d)))
    out = np.stack([np.float32(sg) * ring[:, c, d * ky:d * ky + s * (ho - 1) + 1:s, d * kx:d * kx + s * (wo - 1) + 1:s]
                    for c, ky, kx, sg in taps], 1)
    assert out.dtype == np.float32 and out.shape == (b, len(taps), ho, wo)
    return out + np.float32(0)   # (-0 of a negative sign times a zero: the sum with the other products' +0 is +0)


# ---- planted mistakes: what a wrong kernel would compute, for the tests that show the bars catch it -------------------------------------
def mistaken(src1, w, bias, s, d, act, mistake, src2=None, res=None):
    """the launch in float64 with one planted mistake: "dilation_on_padding_only" (the ring is d wide but the taps are one pixel apart,
    around the centre), "origin_2Y" (the window starts at s Y, not s Y - d), "residual_after_act", "taps_transposed", "src2_first" (the
    concatenation's halves in the wrong order) or "relu_for_leaky" """
    assert mistake in MISTAKES
    a, c = f32(src1), None if src2 is None else f32(src2)
    In = concat(c, a) if (mistake == "src2_first" and c is not None) else concat(a, c)
    wq = f32(w)
    if mistake == "taps_transposed":
        wq = np.ascontiguousarray(np.swapaxes(wq, -1, -2))
    In, wq = bf16_round(In).astype(np.float64), bf16_round(wq).astype(np.float64)
    b_ = f32(bias).astype(np.float64)[None, :, None, None]
    if mistake == "dilation_on_padding_only":
        pre = conv3(In, wq, s, d, tap_step=1, origin=-1) + b_
    elif mistake == "origin_2Y":
        pre = conv3(In, wq, s, d, origin=0) + b_
    else:
        pre = conv3(In, wq, s, d) + b_
    r = 0.0 if res is None else f32(res).astype(np.float64)
    if mistake == "relu_for_leaky":
        act = "relu"
    if mistake == "residual_after_act":
        return activate(pre, act) + r
    return activate(pre + r, act)
