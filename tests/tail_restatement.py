"""A numpy / torch-CPU restatement of include/pvnet_tail.h, written from the header: the float32 upsample operation for operation, the
concatenation, the roundings to bfloat16, the two convolutions' sums in float64 (``exact``: the sums are defined up to their order, so
float64 stands for "any order"), and the absolute-value sums the tests' bars are made of.  Nothing here is measured on the device
code.

Bars (u32 = 2^-24, K1 = 315 terms of a raw element, K2 = 32 of an output element):
    stage 1   |X_dev - X_exact| <= 2 (K1 + 3) u32 A1        A1 = sum |w1| |in| + |b1|
    stage 2   |y_dev - y_exact| <= 2 (K2 + 2) u32 A2 + u_out |y|      A2 = sum |w2| |Xq| + |b2|, Xq the device's own X as stage 2 takes it
(K + 3) u is the bound of a float32 sum of K terms in any order plus the bias and the activation's product; the factor 2 stands for
the matrix pipe's partial sums, whose rounding is not documented.  Operands are those the path under test uses: rounded to bfloat16
for "bf16", as they are for "f32".
"""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8     # unit roundoff of bfloat16 (8 significant bits): half an ulp of a value is at most this share of it
U_OPERAND = 2.0 ** -9  # the per-operand figure the a-priori bound of the bfloat16 tier is built from (see bf16_bound)
K1, K2 = 315, 32
SLOPE = float(np.float32(0.1))   # the activation multiplies by the float32 0.1f
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def f32(t):
    """a tensor (any float type) or array widened exactly to a float32 numpy array"""
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().float().numpy()
    return np.asarray(t, dtype=np.float32)


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def source_coordinates(n_in, n_out):
    """the header's (i0, i1, lambda, 1 - lambda) of every output index, float32"""
    f = np.float32
    r = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    s = np.arange(n_out, dtype=f) * r
    i0 = s.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    lam = s - i0.astype(f)
    return i0, i1, lam, f(1) - lam


def upsample(fm):
    """[b,c,hin,win] -> [b,c,2 hin,2 win], align_corners=True, every product and sum a float32 operation of its own, in the header's
    order: my * (mx * v00 + lx * v01) + ly * (mx * v10 + lx * v11)"""
    fm = f32(fm)
    hin, win = fm.shape[-2:]
    y0, y1, ly, my = source_coordinates(hin, 2 * hin)
    x0, x1, lx, mx = source_coordinates(win, 2 * win)
    v00, v01 = fm[..., y0[:, None], x0[None, :]], fm[..., y0[:, None], x1[None, :]]
    v10, v11 = fm[..., y1[:, None], x0[None, :]], fm[..., y1[:, None], x1[None, :]]
    top = mx * v00 + lx * v01
    bot = mx * v10 + lx * v11
    out = my[:, None] * top + ly[:, None] * bot
    assert out.dtype == np.float32
    return out


def concat(fm, image):
    """In [b,35,h,w] float32: the upsampled channels, then the image's"""
    return np.concatenate([upsample(fm), f32(image)], 1)


def operands(In, w1, w2, precision):
    """(In, w1, w2) as float64 arrays holding the values the path multiplies"""
    In, w1, w2 = f32(In), f32(w1), f32(w2)
    if precision == "bf16":
        In, w1, w2 = bf16_round(In), bf16_round(w1), bf16_round(w2)
    else:
        assert precision == "f32"
    return In.astype(np.float64), w1.astype(np.float64), w2.astype(np.float64)


def _conv3(In, w1):   # float64, zero padding of 1 on In
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(In)), torch.from_numpy(np.ascontiguousarray(w1)), padding=1).numpy()


def raw_exact(In, w1, b1, slope=SLOPE):
    """stage 1 in float64 from the operands as given: (X after the activation, A1)"""
    b1 = f32(b1).astype(np.float64)[None, :, None, None]
    pre = _conv3(In, w1) + b1
    A1 = _conv3(np.abs(In), np.abs(w1)) + np.abs(b1)
    return np.where(pre > 0, pre, pre * slope), A1


def out_exact(Xq, w2, b2):
    """stage 2 in float64 from the raw values as stage 2 takes them: (y, A2)"""
    Xq = np.asarray(Xq, dtype=np.float64)
    b2 = f32(b2).astype(np.float64)[None, :, None, None]
    y = np.einsum("qo,bohw->bqhw", w2, Xq) + b2
    A2 = np.einsum("qo,bohw->bqhw", np.abs(w2), np.abs(Xq)) + np.abs(b2)
    return y, A2


def bar1(A1):
    return 2 * (K1 + 3) * U32 * A1


def bar2(A2, y, out_dtype):
    return 2 * (K2 + 2) * U32 * A2 + U_OUT[out_dtype] * np.abs(y)


def stage2_input(X_dev, precision):
    """the device's own raw output (float32) as its second convolution takes it"""
    X = f32(X_dev)
    return (bf16_round(X) if precision == "bf16" else X).astype(np.float64)


def forward_exact(fm, image, w1, b1, w2, b2, precision):
    """both stages in float64 on the path's operands: dict(In, w1, w2, X, A1, Xq, y, A2); Xq is X rounded as the path rounds it"""
    In, w1_, w2_ = operands(concat(fm, image), w1, w2, precision)
    X, A1 = raw_exact(In, w1_, b1)
    Xq = bf16_round(X.astype(np.float32)).astype(np.float64) if precision == "bf16" else X
    y, A2 = out_exact(Xq, w2_, b2)
    return dict(In=In, w1=w1_, w2=w2_, X=X, A1=A1, Xq=Xq, y=y, A2=A2)


def bf16_bound(fm, image, w1, b1, w2, b2, out_dtype=torch.float32):
    """A-priori bound of |y_bf16 - y_f32| per output element, y_f32 the exact tier on the unrounded operands, from u = 2^-9 per
    operand rounding (U_OPERAND: half of bfloat16's worst case 2^-8, which a value just above a power of two reaches and an average one
    does not; the bound is a sanity line -- a simulation of the tier uses a tenth of it -- and the stage bars, not this, pin the tier):
      a product of two rounded operands is off by at most ((1 + u)^2 - 1) |w| |in|, so the pre-activation by e1 = ((1 + u)^2 - 1) A1
      (plus the stage-1 bar for the float32 sum); the activation does not expand it (slopes 1 and 0.1);
      rounding the activated value adds u |X~| <= u (|X| + e1):  e2 = e1 + u (|X| + e1);
      |w2~ Xq - w2 X| <= (1 + u) |w2| e2 + u |w2| |X|, summed over the 32 raw channels, plus the stage-2 bar for the float32 sum and
      the output's rounding.
    Returns (bound, y_f32)."""
    u = U_OPERAND
    In, w1_, w2_ = operands(concat(fm, image), w1, w2, "f32")
    X, A1 = raw_exact(In, w1_, b1)
    e1 = ((1 + u) ** 2 - 1) * A1 + bar1(A1)
    e2 = e1 + u * (np.abs(X) + e1)
    y, A2 = out_exact(X, w2_, b2)
    spread = np.einsum("qo,bohw->bqhw", np.abs(w2_), (1 + u) * e2 + u * np.abs(X))
    return spread + bar2(A2 + spread, np.abs(y) + spread, out_dtype), y


# ---- planted mistakes: what a wrong kernel would compute, for the tests that show the bars catch it -------------------------------------
def swap_k_order(w2):
    """w2 as the 1 x 1 convolution would apply it with its A fragment in the NATURAL k order against the accumulator's permuted one:
    element j of lane half h multiplies row 16 s + 8 (j >> 2) + 4 h + (j & 3) but holds column 16 s + 8 h + j, so bits 2 and 3 of the
    column index change places"""
    k = np.arange(32)
    perm = (k & ~0xC) | ((k & 4) << 1) | ((k & 8) >> 1)
    return np.asarray(w2)[:, perm]


def mistaken_raw(fm, image, w1, b1, precision, mistake):
    """stage 1 in float64 with one planted mistake: "align_corners_false", "image_first", "taps_transposed", "slope_0.01", or
    "pad_before_upsample" (the zero ring lies around the half-resolution features: an output pixel outside the image is half way
    between the edge and that ring, so it holds half the edge's upsampled value instead of 0; the image part stays 0)"""
    up, img = upsample(fm), f32(image)
    w1 = f32(w1)
    slope = SLOPE
    if mistake == "align_corners_false":
        up = F.interpolate(torch.from_numpy(f32(fm)), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    In = np.concatenate([img, up] if mistake == "image_first" else [up, img], 1)
    if mistake == "taps_transposed":
        w1 = np.ascontiguousarray(np.swapaxes(w1, -1, -2))
    if mistake == "slope_0.01":
        slope = float(np.float32(0.01))
    In_, w1_, _ = operands(In, w1, np.zeros((1, 32), np.float32), precision)
    if mistake == "pad_before_upsample":
        ring = np.pad(In_, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge") * 0.5
        ring[:, 32:] = 0.0
        ring[:, :, 1:-1, 1:-1] = In_
        b1_ = f32(b1).astype(np.float64)[None, :, None, None]
        pre = F.conv2d(torch.from_numpy(ring), torch.from_numpy(np.ascontiguousarray(w1_))).numpy() + b1_
        return np.where(pre > 0, pre, pre * slope)
    return raw_exact(In_, w1_, b1, slope)[0]
