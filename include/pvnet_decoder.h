/* pvnet_decoder.h -- C ABI of libpvnet_decoder.so: one DECODER STAGE in one launch -- bilinear 2x upsample, concatenation with the skip
 * features, 3 x 3 convolution (BatchNorm folded in) and LeakyReLU.  Inference only.
 *
 * Path replaced (reference tree, lib/networks/model_repository.py:29-50, 67-73; Resnet18_8s), twice:
 *     fm = conv4s(cat([up8sto4s(fm), x4s], 1))    up 2x of [b,128,h/8,w/8], skip [b,64,h/4,w/4] -> [b,64,h/4,w/4]
 *     fm = conv2s(cat([up4sto2s(fm), x2s], 1))    up 2x of [b, 64,h/4,w/4], skip [b,64,h/2,w/2] -> [b,32,h/2,w/2]
 * each UpsamplingBilinear2d(2), cat, Conv2d(cin, cout, 3, 1, 1, bias=False), BatchNorm2d, LeakyReLU(0.1).  (conv2s' output is what
 * pvnet_tail_forward of pvnet_tail.h takes as `fm`.)
 *
 * DEFINITION.  The operand values are defined bit for bit, the sums up to their order.
 *
 *   Upsample (align_corners = True), word for word that of pvnet_tail.h.  With ry = (float)(hin - 1) / (float)(h - 1) (0 when h == 1)
 *   and rx likewise from win and w, both float32 quotients, output row Y takes
 *       sy = (float)Y * ry,   y0 = (int)sy,   y1 = y0 + (y0 < hin - 1),   ly = sy - (float)y0,   my = 1 - ly
 *   and column X the same with rx, x0, x1, lx, mx.  The value of channel c is
 *       my * (mx * v00 + lx * v01) + ly * (mx * v10 + lx * v11)            vij = (float)lo[c][yi][xj], widened exactly
 *   in float32 with ONE ROUNDING PER OPERATION in exactly that order, none contracted into a fused multiply-add (the translation unit
 *   is compiled under `#pragma clang fp contract(off)`).
 *
 *   Concatenation: In[0..cl-1] = the upsampled channels of `lo`, In[cl..cl+cs-1] = (float)skip[0..cs-1]: the upsampled channels come
 *   FIRST, as cat([fm, x], 1).  The convolution's zero padding of 1 applies to In: outside the h x w image every channel is 0.
 *
 *   Operands: there is ONE tier, bfloat16.  Every In value (the upsampled ones after the float32 arithmetic above) and every element of
 *   w is rounded ONCE to bfloat16, round to nearest even.  Products of two bfloat16 values are exact in float32; they are accumulated
 *   in float32 on the matrix pipe (v_mfma_f32_32x32x16_bf16), starting from bias[o]:
 *       out[o](Y, X) = act(bias[o] + sum over c < cl + cs, ky < 3, kx < 3 of w[o][c][ky][kx] * In[c](Y + ky - 1, X + kx - 1))
 *       act(v) = v > 0 ? v : 0.1f * v        (one float32 product)
 *   w and bias hold the eval() BatchNorm already: w = W * s, bias = beta - mean * s with s = gamma / sqrt(var + eps).
 *   The result is rounded once to the type of `out`: a float32 `out` receives the activated accumulators unrounded.
 *   There is no float32 tier: one-hot weights pin the geometry through the bfloat16 tier itself.
 *
 * ARGUMENTS.  lo [b,cl,hin,win] and skip [b,cs,h,w_]: float32 / float16 / bfloat16 (PVNET_DECODER_T_*), any ELEMENT strides (four
 * each).  h == 2 hin and w_ == 2 win, anything else is PVNET_E_BADARG (the reference's cat fails there too).  w [co,cl+cs,3,3] and
 * bias [co]: float32, contiguous.  With PVNET_DECODER_F_PACKED, `w` points instead at the same weights already rounded to bfloat16 and
 * laid out in the order the kernel's matrix fragments take them (co * (cl + cs) * 9 bfloat16, 16-byte aligned):
 *     element ((((chunk * 9 + tap) * 2 + half) * (co / 32) + m) * 64 + lane) * 8 + j
 *         = bf16(w[32 m + (lane & 31)][32 chunk + 16 half + 8 (lane >> 5) + j][tap / 3][tap % 3])
 * which a front end makes once per parameter set; the values, and so the results, are the same bit for bit, and the kernel then takes
 * a fragment with one 16-byte load where it otherwise gathers and rounds eight float32 values (several times slower: that path is the
 * definition's, for a caller with nothing but the float32 weights).  (cl, cs, co) must be (64, 64, 32) or (128, 64, 64) -- conv2s and
 * conv4s of Resnet18_8s; the reference's Resnet50_8s is wider --: other positive widths are PVNET_E_UNSUPPORTED.
 * out [b,co,h,w_] of out_type, contiguous, any element alignment.
 *
 * ONE launch on `stream`: no workspace, no atomics, no allocation, no synchronisation; capturable in a graph; bitwise reproducible (a
 * pixel's arithmetic does not depend on the launch's shape).  All arguments are checked before any HIP call.  Return value: 0, a
 * positive hipError_t, PVNET_E_BADARG (-1: a null pointer, a size < 1, an unknown type or flag, h != 2 hin, w_ != 2 win) or
 * PVNET_E_UNSUPPORTED (-3: widths other than the two triples, b > 65535, h or w_ > 32768).
 *
 * KERNEL SHAPE.  A workgroup of four waves walks tiles of 64 x 4 output pixels and, per tile, the chunks of 32 channels of In.  It
 * stages a chunk of the tile with a one-pixel halo into LDS -- upsampled or copied, a pixel's 32 channels contiguous in a record of 80
 * bytes (that stride keeps the sixteen lanes of a ds_read_b128 group on sixteen different 16-byte slots) -- then every wave owns one
 * row: 18 k-steps per chunk (9 taps x 2 halves of the chunk), the B operand one ds_read_b128 per lane and column block of 32 pixels,
 * the A operand the weights' fragment from global memory (221 KB at most: resident in L2), each used for both column blocks; co / 32
 * row blocks x 2 column blocks of accumulators persist across the chunks.  Pixels are on the lanes, so a store instruction writes 32
 * consecutive pixels of a channel plane.
 */
#ifndef PVNET_DECODER_H_
#define PVNET_DECODER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_DECODER_ABI_VERSION 1
#define PVNET_DECODER_SKIP 64    /* channels of skip, at both supported shapes */
/* element types of lo, skip and out */
#define PVNET_DECODER_T_F32  0
#define PVNET_DECODER_T_F16  1
#define PVNET_DECODER_T_BF16 2
/* flags */
#define PVNET_DECODER_F_PACKED 1u   /* w is the bfloat16 fragment-order image of the weights (see ARGUMENTS) */

int pvnet_decoder_abi_version(void);

int pvnet_decoder_stage(const void* lo, int lo_type, const int64_t lo_strides[4],
                        const void* skip, int skip_type, const int64_t skip_strides[4],
                        const float* w, const float* bias,
                        int b, int hin, int win, int h, int w_, int cl, int cs, int co,
                        uint32_t flags, void* out, int out_type, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_DECODER_H_ */
