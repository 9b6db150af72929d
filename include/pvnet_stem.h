/* pvnet_stem.h -- C ABI of libpvnet_stem.so: the network's STEM in one launch -- 7 x 7 stride-2 convolution (BatchNorm folded in), ReLU
 * and the 3 x 3 stride-2 max-pool behind it.  Inference only.
 *
 * Path replaced (reference tree, lib/networks/resnet.py:138-142, 200-204; ResNet.forward):
 *     x2s = relu(bn1(conv1(x)))        Conv2d(3, 64, 7, 2, 3, bias=False), BatchNorm2d(64), ReLU      [b,3,h,w] -> [b,64,Ho,Wo]
 *     x   = maxpool(x2s)               MaxPool2d(3, 2, 1)                                             -> [b,64,Hp,Wp]
 * four eager kernels (and a conversion of the float32 image under autocast), which write x2s, read and rewrite it for the BatchNorm and
 * for the ReLU and read it again for the pool.  Here the image is read once and x2s -- the decoder's conv2s stage takes it as its skip
 * input (pvnet_decoder.h) -- and the pooled tensor that layer1 takes are written once each.
 *
 * DEFINITION.  The operand values are defined bit for bit, the sums up to their order.
 *
 *   Sizes (integer division):  Ho = (h - 1) / 2 + 1,  Wo = (w_ - 1) / 2 + 1;   Hp = (Ho - 1) / 2 + 1,  Wp = (Wo - 1) / 2 + 1.
 *
 *   Operands: there is ONE tier, bfloat16.  Every image value and every element of w is rounded ONCE to bfloat16, round to nearest even.
 *   Products of two bfloat16 values are exact in float32; they are accumulated in float32 on the matrix pipe
 *   (v_mfma_f32_32x32x16_bf16), starting from bias[o]:
 *       x2s[o](Y, X) = relu(bias[o] + sum over c < 3, ky < 7, kx < 7 of w[o][c][ky][kx] * In[c](2 Y + ky - 3, 2 X + kx - 3))
 *   In is 0 outside the h x w_ image (the convolution's padding of 3).  w and bias hold the eval() BatchNorm already: w = W * s,
 *   bias = beta - mean * s with s = gamma / sqrt(var + eps).
 *       relu(v): a NaN stays a NaN, negative values and -0 become +0, everything else stays.
 *   The activated value is rounded once to out_type; a float32 x2s receives it unrounded.
 *
 *   Pool: pooled[o](Yp, Xp) = the maximum of the STORED x2s[o](2 Yp + ky - 1, 2 Xp + kx - 1) over ky, kx < 3; only positions inside
 *   Ho x Wo count (the centre always is), and the result is NaN if any of them is NaN: nn.MaxPool2d(3, 2, 1) on the stored values.
 *
 *   A pixel outside an output's 7 x 7 window has no influence on that output, whatever its value: K = 147 is padded to 176 for the
 *   matrix instruction, and the pad positions of BOTH operands are zero bits -- no image value, which might be an Inf or a NaN, is ever
 *   multiplied by a pad weight (0 * Inf is NaN).
 *
 * ARGUMENTS.  image [b,3,h,w_]: float32 / float16 / bfloat16 (PVNET_STEM_T_*), any ELEMENT strides (four; channels-last is one).
 * w [64,3,7,7] and bias [64]: float32, contiguous.  x2s [b,64,Ho,Wo] and pooled [b,64,Hp,Wp]: contiguous, of out_type, any element
 * alignment.  pooled may be null: then only x2s is written (with the same bits).  The widths are fixed at 3 -> 64, which are ResNet-50's
 * too.  There is one weights format: every workgroup rounds and arranges the 9 408 weights itself, once, before it loops over its tiles.
 *
 * ONE launch on `stream`: no workspace, no atomics, no allocation, no synchronisation; capturable in a graph; bitwise reproducible (a
 * pixel's arithmetic does not depend on the launch's shape: a pixel is one column of the matrix product, its k order fixed).  All
 * arguments are checked before any HIP call.  Return value: 0, a positive hipError_t, PVNET_E_BADARG (-1: a null pointer other than
 * pooled, a size < 1, an unknown type) or PVNET_E_UNSUPPORTED (-3: b > 65535, h or w_ > 32768).
 *
 * KERNEL SHAPE.  A grid of at most two workgroups per compute unit, four waves each, walks tiles of 64 x 4 x2s pixels.  A workgroup first
 * writes the weights into LDS in fragment order (22 KB).  K is ordered so that a lane's eight k values are consecutive columns of one
 * (c, ky) input row: 21 groups of 7 taps + 1 zero, and a 22nd group of zeros, 11 k-steps.  Per tile the workgroup
 *   1. stages the (2 * 65 + 5) x (2 * 5 + 5) x 3 input patch into LDS as bfloat16 (12 KB), zero outside the image: the tile's pixels and,
 *      for the pool, the x2s row above them and the x2s column to their left, which are RECOMPUTED, not exchanged (tile origins are
 *      even, so a pool window never reaches below or right of its tile; the convolution is cheap and a second pass is not).  The loads
 *      are issued one tile ahead, all of them unconditional (clamped into the image, zeroed afterwards);
 *   2. per half of the output channels (32: one row block of the matrix instruction) runs 11 jobs over its waves -- 5 rows x 2 column
 *      blocks of 32 pixels, and one block whose columns are the five pixels of the left halo column --, a job 11 k-steps with the weights'
 *      fragment (ds_read_b128) and the pixels' (16 bytes of a patch row at a 4-byte aligned address, its eighth value masked) from LDS;
 *      the activated values, rounded, go into a 32 x 5 x 65 LDS image as out_type's bits (at most 45 KB), +0 outside Ho x Wo, from which
 *   3. x2s is stored, eight consecutive pixels of a channel plane per lane -- one 16-byte store (two for float32) wherever the row's
 *      address allows it, element by element otherwise -- and
 *   4. the 32 x 2 x 32 pooled values of that half are taken as the unsigned maxima of nine values' bits (nothing stored is below +0, so
 *      the bits order as the values do, and a NaN's bits are above every number's) and stored.
 * The barriers between these steps wait for LDS operations only, not for the global stores behind them.
 * Without pooled, the halo row, the halo column and step 4 are left out.
 */
#ifndef PVNET_STEM_H_
#define PVNET_STEM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_STEM_ABI_VERSION 1
#define PVNET_STEM_CIN  3     /* channels of image */
#define PVNET_STEM_COUT 64    /* channels of x2s and pooled */
/* element types of image, x2s and pooled */
#define PVNET_STEM_T_F32  0
#define PVNET_STEM_T_F16  1
#define PVNET_STEM_T_BF16 2

int pvnet_stem_abi_version(void);

int pvnet_stem_forward(const void* image, int image_type, const int64_t image_strides[4],
                       const float* w, const float* bias, int b, int h, int w_,
                       void* x2s, void* pooled, int out_type, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_STEM_H_ */
