/* pvnet_tail.h -- C ABI of libpvnet_tail.so: the network's TAIL in one launch -- bilinear 2x upsample, concatenation with the image,
 * 3 x 3 convolution (BatchNorm folded in), LeakyReLU and 1 x 1 convolution.  Inference only.
 *
 * Path replaced (reference tree, lib/networks/model_repository.py:51-58, 74-78; Resnet18_8s):
 *     fm = up2storaw(fm)                  UpsamplingBilinear2d(scale_factor=2): [b,32,hin,win] -> [b,32,h,w]
 *     x  = convraw(cat([fm, image], 1))   Conv2d(35,32,3,1,1,bias=False) + BatchNorm2d(32) + LeakyReLU(0.1) + Conv2d(32,cout,1)
 * `out[:, :2]` / `out[:, 2:]` are the reference's seg_pred / ver_pred; the voting library's `_logits` entries read them in place.
 *
 * DEFINITION.  The operand values are defined bit for bit, the sums up to their order.
 *
 *   Upsample (align_corners = True).  With ry = (float)(hin - 1) / (float)(h - 1) (0 when h == 1) and rx likewise from win and w, both
 *   float32 quotients, output row Y takes
 *       sy = (float)Y * ry,   y0 = (int)sy,   y1 = y0 + (y0 < hin - 1),   ly = sy - (float)y0,   my = 1 - ly
 *   and column X the same with rx, x0, x1, lx, mx.  The value of channel c is
 *       my * (mx * v00 + lx * v01) + ly * (mx * v10 + lx * v11)            vij = (float)fm[c][yi][xj], widened exactly
 *   in float32 with ONE ROUNDING PER OPERATION in exactly that order: seven products, three sums, the two subtractions above, none
 *   contracted into a fused multiply-add (the translation unit is compiled under `#pragma clang fp contract(off)`; HIP's __fmul_rn /
 *   __fadd_rn are plain operators that the compiler may contract, so the pragma, not they, is what holds it).
 *
 *   Concatenation: In[0..31] = the upsampled channels, In[32..34] = (float)image[0..2], as cat([fm, image], 1).  The convolution's zero
 *   padding of 1 applies to In: outside the h x w image all 35 channels are 0.
 *
 *   Raw (stage 1):   X[o](Y, X) = act(b1[o] + sum over c < 35, ky < 3, kx < 3 of w1[o][c][ky][kx] * In[c](Y + ky - 1, X + kx - 1))
 *                    act(v) = v > 0 ? v : 0.1f * v        (one float32 product)
 *   Output (stage 2): out[q] = b2[q] + sum over o < 32 of w2[q][o] * X[o]
 *   w1 and b1 hold the eval() BatchNorm already: w1 = W * s, b1 = beta - mean * s with s = gamma / sqrt(var + eps).
 *
 *   PVNET_TAIL_BF16: every operand is rounded ONCE to bfloat16, round to nearest even -- every In value (the upsampled ones after the
 *   float32 arithmetic above), every w1 and w2 element, every X[o] (after the activation).  Products of two bfloat16 values are exact in
 *   float32; they are accumulated in float32 on the matrix pipe (v_mfma_f32_32x32x16_bf16), b1 and b2 enter in float32 (as the
 *   accumulators' initial values).
 *   PVNET_TAIL_F32: the operands are the float32 values, nothing is rounded to bfloat16; the sums are chains of float32 fused
 *   multiply-adds (fmaf) that start from b1 / b2.  No matrix instruction.  This tier pins the geometry.
 *   Either way the result is rounded once to the type of `out`.
 *
 *   PVNET_TAIL_F_RAW: `out` is [b,32,h,w] FLOAT32 and receives X, after the activation and before any rounding to bfloat16; the 1 x 1
 *   convolution is skipped (w2, b2 and cout are still checked).  A feature map to look at, and the handle by which the tests hold each
 *   stage to its own bound.
 *
 * ARGUMENTS.  fm [b,feat,hin,win] and image [b,3,h,w]: float32 / float16 / bfloat16 (PVNET_TAIL_T_*), any ELEMENT strides (four
 * each).  h == 2 hin and w == 2 win, anything else is PVNET_E_BADARG (the reference's cat fails there too).  w1 [raw,feat+3,3,3],
 * b1 [raw], w2 [cout,raw], b2 [cout]: float32, contiguous, 1 <= cout <= 32.  feat and raw must both be 32 (PVNET_TAIL_WIDTH; the
 * reference's Resnet50_8s has 64): other positive widths are PVNET_E_UNSUPPORTED.  out [b,cout,h,w] of out_type, contiguous, any
 * element alignment.
 *
 * ONE launch on `stream`: no workspace, no atomics, no allocation, no synchronisation; capturable in a graph; bitwise reproducible
 * (a pixel's arithmetic does not depend on the launch's shape).  All arguments are checked before any HIP call.  Return value: 0, a
 * positive hipError_t, PVNET_E_BADARG (-1: a null pointer, a size < 1, cout outside 1 .. 32, an unknown type, precision or flag,
 * h != 2 hin, w != 2 win, PVNET_TAIL_F_RAW with an out_type other than float32) or PVNET_E_UNSUPPORTED (-3: widths other than 32,
 * b > 65535, h or w > 32768).
 *
 * KERNEL SHAPE.  A workgroup of four waves walks tiles of 64 x 4 output pixels.  It stages the tile's In with a one-pixel halo into
 * LDS once -- upsampled, concatenated, a pixel's channels contiguous (40 bfloat16 = 80 bytes: that stride keeps the sixteen lanes of
 * a ds_read_b128 group on sixteen different 16-byte slots) -- then every wave owns one row: X = W1 * In per 32 pixels as 18 k-steps
 * (9 taps x 2 halves of the 32 feature channels, one ds_read_b128 per lane each) + 2 k-steps (the 27 (tap, image channel) terms,
 * padded to 32), W1's fragments in 80 registers for the whole launch; the accumulator tile is then the B operand of Y = W2 * X with no
 * lane movement (its k order inside a step is row 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), and W2's fragment is laid out to
 * match).  Pixels are on the lanes, so a store instruction writes 32 consecutive pixels of two channel planes.  The float32 tier
 * stages the same tile in float32 and gives a lane one pixel.
 */
#ifndef PVNET_TAIL_H_
#define PVNET_TAIL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_TAIL_ABI_VERSION 1
#define PVNET_TAIL_WIDTH 32      /* feature channels of fm, and channels after the 3 x 3 convolution */
#define PVNET_TAIL_MAX_COUT 32
/* element types of fm, image and out */
#define PVNET_TAIL_T_F32  0
#define PVNET_TAIL_T_F16  1
#define PVNET_TAIL_T_BF16 2
/* precision */
#define PVNET_TAIL_BF16 0        /* operands rounded to bfloat16, float32 accumulation on the matrix pipe: the hot path */
#define PVNET_TAIL_F32  1        /* float32 operands, float32 fused multiply-adds */
/* flags */
#define PVNET_TAIL_F_RAW 1u      /* out [b,32,h,w] float32 = the activated output of the 3 x 3 convolution */

int pvnet_tail_abi_version(void);

int pvnet_tail_forward(const void* fm, int fm_type, const int64_t fm_strides[4],
                       const void* image, int image_type, const int64_t image_strides[4],
                       const float* w1, const float* b1, const float* w2, const float* b2,
                       int b, int hin, int win, int h, int w, int feat, int raw, int cout,
                       int precision, uint32_t flags, void* out, int out_type, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_TAIL_H_ */
