"""A numpy restatement of include/pvnet_stem.h, written from the header: the one rounding of every operand to bfloat16 (a switch leaves
them unrounded), the 147 products of the 7 x 7 stride-2 window summed in float64 (the sums are defined up to their order, so float64
stands for "any order"), the ReLU, the one rounding to the output type, the 3 x 3 stride-2 maximum over the positions inside the image,
and the absolute-value sum the tests' bar is made of.  Nothing here is measured on the device code.

Bar (u32 = 2^-24, K = 147 terms of an output element):
    |x2s_dev - x2s_exact| <= 2 (K + 3) u32 A  (+ u_out |x2s| for a half-type out)        A = sum |w| |in| over the rounded operands
(K + 3) u is the bound of a float32 sum of K terms in any order plus the bias; the factor 2 stands for the matrix pipe's partial sums,
whose rounding is not documented -- the bar tests/tail_restatement.py states for the tail's first stage.  A maximum moves by no more
than its arguments do, so pooled is held to the 3 x 3 stride-2 maximum of those bars.
"""
import numpy as np

from tests.tail_restatement import U32, U_OUT, bf16_round, f32  # noqa: F401  (re-exported for the tests)

K = 147
MISTAKES = ("padding_2", "taps_transposed", "channels_reversed", "phase_shifted", "pool_padding_0", "pool_window_2")


def out_sizes(h, w):
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return ho, wo, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


def window_sum(In, w, origin=-3):
    """sum over c, ky, kx of w[o][c][ky][kx] * In[c](2 Y + ky + origin, 2 X + kx + origin) for Y < Ho, X < Wo, In zero outside the image;
    float64.  (origin = -3 is the header's; the planted mistakes move it.)"""
    In, w = np.asarray(In, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b, _, h, wd = In.shape
    ho, wo, _, _ = out_sizes(h, wd)
    lo, hi = max(0, -origin), 7 + max(0, origin)   # a ring wide enough for every index 2 Y + ky + origin
    ring = np.pad(In, ((0, 0), (0, 0), (lo, hi + 2), (lo, hi + 2)))
    out = np.zeros((b, w.shape[0], ho, wo))
    for c in range(w.shape[1]):
        for ky in range(7):
            for kx in range(7):
                y0, x0 = ky + origin + lo, kx + origin + lo
                out += w[None, :, c, ky, kx, None, None] * ring[:, c, None, y0:y0 + 2 * ho:2, x0:x0 + 2 * wo:2]
    return out


def relu(v):
    """a NaN stays, negative values and -0 become +0"""
    return np.where(v <= 0, 0.0, v)


def pool(x, pad=1, window=3):
    """pooled(Yp, Xp) = the maximum of x(2 Yp + ky - pad, 2 Xp + kx - pad), ky, kx < window, over the positions inside the image; NaN if
    any of them is NaN.  (pad = 1, window = 3 are the header's.)"""
    x = np.asarray(x)
    ho, wo = x.shape[-2:]
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    ring = np.pad(x, ((0, 0), (0, 0), (pad, window + 1), (pad, window + 1)), constant_values=-np.inf)
    out = np.full(x.shape[:2] + (hp, wp), -np.inf, dtype=x.dtype)
    for ky in range(window):
        for kx in range(window):
            out = np.maximum(out, ring[:, :, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2])   # np.maximum hands a NaN on
    return out


def round_to(v, out_dtype):
    """float64 -> the nearest value of the output type, as float64 (float32: unrounded, as the bar compares the accumulators)"""
    import torch
    if out_dtype == torch.float32:
        return v
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.float32).to(out_dtype).double().numpy()


def stem_exact(image, w, bias, rounded=True):
    """the stem in float64 on the operands the kernel multiplies (``rounded=False``: on the operands as given): dict(In, w: the operands
    as float64; pre; x2s: after the ReLU; pooled; A: sum |w| |in|)"""
    In, wq = f32(image), f32(w)
    if rounded:
        In, wq = bf16_round(In), bf16_round(wq)
    In, wq = In.astype(np.float64), wq.astype(np.float64)
    with np.errstate(invalid="ignore"):
        pre = window_sum(In, wq) + f32(bias).astype(np.float64)[None, :, None, None]
        x2s = relu(pre)
        return dict(In=In, w=wq, pre=pre, x2s=x2s, pooled=pool(x2s), A=window_sum(np.abs(In), np.abs(wq)))


def bar(A, x2s=None, out_dtype=None):
    """the a-priori bar of every x2s element; a half-type out adds that type's one rounding of the value"""
    import torch
    lim = 2 * (K + 3) * U32 * A
    return lim if out_dtype in (None, torch.float32) else lim + U_OUT[out_dtype] * np.abs(x2s)


def onehot_expected(In, taps):
    """With w[o][c][ky][kx] = +1 (even o) or -1 (odd o) for the one (c, ky, kx) = taps[o] of every output channel, bias 0:
    x2s[o](Y, X) = relu(+-In[c](2 Y + ky - 3, 2 X + kx - 3)), In (already rounded) zero outside the image -- as float32, bit for bit (the
    one product and the sum with zeros are exact)"""
    In = np.asarray(In, dtype=np.float32)
    b, _, h, w = In.shape
    ho, wo, _, _ = out_sizes(h, w)
    ring = np.pad(In, ((0, 0), (0, 0), (3, 5), (3, 5)))
    out = np.stack([ring[:, c, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] * np.float32(1 if o % 2 == 0 else -1) for o, (c, ky, kx) in enumerate(taps)], 1)
    res = np.where(out <= 0, np.float32(0), out)
    assert res.dtype == np.float32 and res.shape == (b, len(taps), ho, wo)
    return res


# ---- planted mistakes: what a wrong kernel would compute, for the tests that show the bars catch it -------------------------------------
def mistaken(image, w, bias, mistake):
    """(x2s, pooled) in float64 on the rounded operands with one planted mistake: "padding_2" (the window starts at 2 Y - 2),
    "taps_transposed" (ky <-> kx), "channels_reversed", "phase_shifted" (the stride's phase off by one: the window starts at 2 Y - 4),
    "pool_padding_0" (the pool's window starts at 2 Yp), "pool_window_2" (ky, kx < 2)"""
    assert mistake in MISTAKES
    In, wq = bf16_round(f32(image)).astype(np.float64), bf16_round(f32(w)).astype(np.float64)
    if mistake == "taps_transposed":
        wq = np.ascontiguousarray(np.swapaxes(wq, -1, -2))
    if mistake == "channels_reversed":
        In = np.ascontiguousarray(In[:, ::-1])
    origin = {"padding_2": -2, "phase_shifted": -4}.get(mistake, -3)
    x2s = relu(window_sum(In, wq, origin) + f32(bias).astype(np.float64)[None, :, None, None])
    return x2s, pool(x2s, pad=0 if mistake == "pool_padding_0" else 1, window=2 if mistake == "pool_window_2" else 3)
