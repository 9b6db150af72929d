/* pvnet_trunk.h -- C ABI of libpvnet_trunk.so: one 3 x 3 CONVOLUTION OF THE RESIDUAL TRUNK in one launch -- the convolution over one
 * or two concatenated inputs with the eval() BatchNorm folded in, the residual addition and the activation applied to its own
 * accumulators.  Inference only.
 *
 * Path replaced (reference tree): every 3 x 3 convolution between the stem and the decoder of Resnet18_8s --
 *     BasicBlock.forward (lib/networks/resnet.py:54-70), twice per block and eight blocks in layer1 .. layer4:
 *         out = relu(bn1(conv1(x)))                        (s, d) = (1,1), (2,1) once in layer2[0], (1,2) in layer3, (1,4) in layer4
 *         out = relu(bn2(conv2(out)) + residual)           residual = x, or downsample(x)
 *     fc     = Conv2d(512, fcdim, 3, 1, 1), BatchNorm2d, ReLU                      (lib/networks/model_repository.py:17-27)
 *     conv8s = Conv2d(128 + fcdim, s8dim, 3, 1, 1), BatchNorm2d, LeakyReLU(0.1) on cat([xfc, x8s], 1)              (:29-33, 67)
 * -- eighteen convolutions, each followed in eager mode by up to five elementwise kernels over its output.
 *
 * DEFINITION.  There is ONE tier.  The operand values are defined bit for bit, the sums up to their order.
 *
 *   Concatenation: In[0..c1-1] = (float)src1[0..c1-1], In[c1..c1+c2-1] = (float)src2[0..c2-1]: src1 comes FIRST, as cat([src1, src2], 1).
 *   The convolution's zero padding of d applies to In: outside the h x w image every channel is 0.
 *
 *   Operands: every In value and every weight is rounded ONCE to bfloat16, round to nearest even.  Products of two bfloat16 values are
 *   exact in float32; they are accumulated in float32 on the matrix pipe (v_mfma_f32_32x32x16_bf16), starting from bias[o]:
 *       acc[o](Y, X) = bias[o] + sum over c < c1 + c2, ky < 3, kx < 3 of w[o][c][ky][kx] * In[c](s Y + d (ky - 1), s X + d (kx - 1))
 *   for Y < ho = (h - 1) / s + 1 and X < wo = (w_ - 1) / s + 1 (integer divisions).  Then
 *       v = acc + (float)res[o](Y, X)          ONE float32 addition, res widened exactly; only where res is given
 *       PVNET_TRUNK_ACT_NONE   out = v
 *       PVNET_TRUNK_ACT_RELU   out = v <= 0 ? +0 : v            (the stem's wording: a NaN compares false and stays, -0 becomes +0)
 *       PVNET_TRUNK_ACT_LEAKY  out = v > 0 ? v : v * 0.1f       (one float32 product, the decoder's wording)
 *   and out is rounded once to the type of `out`: a float32 `out` receives v unrounded.
 *   w and bias hold the eval() BatchNorm already: w = W * g, bias = beta - mean * g with g = gamma / sqrt(var + eps).
 *   There is no float32 tier: one-hot weights pin the geometry through the bfloat16 tier itself.
 *
 * ARGUMENTS.  src1 [b,c1,h,w_], src2 [b,c2,h,w_] or NULL with c2 == 0, res [b,co,ho,wo] or NULL: float32 / float16 / bfloat16
 * (PVNET_TRUNK_T_*, each its own), any ELEMENT strides (four each; the strides and type of a NULL tensor are not read).
 * c1 and c2 (where src2 is given) are positive multiples of 32 with c1 + c2 <= 512, co a multiple of 32 up to 512, and
 * (stride, dilation) one of (1,1), (2,1), (1,2), (1,4): anything else in positive sizes is PVNET_E_UNSUPPORTED (the ResNet-50
 * Bottleneck's widths are).  bias [co]: float32, contiguous.  out [b,co,ho,wo] of out_type, contiguous, any element alignment.
 * `w` is ALWAYS PACKED: the weights rounded to bfloat16 and laid out in the order the kernel's matrix fragments take them
 * (co * (c1 + c2) * 9 bfloat16, 16-byte aligned) -- the layout of PVNET_DECODER_F_PACKED of pvnet_decoder.h:
 *     element ((((chunk * 9 + tap) * 2 + half) * (co / 32) + m) * 64 + lane) * 8 + j
 *         = bf16(w[32 m + (lane & 31)][32 chunk + 16 half + 8 (lane >> 5) + j][tap / 3][tap % 3])
 * which a front end makes once per parameter set.  There is no unpacked path.
 *
 * ONE launch on `stream`: no workspace, no atomics, no allocation, no synchronisation; capturable in a graph; bitwise reproducible (a
 * pixel's arithmetic does not depend on the launch's shape).  All arguments are checked before any HIP call.  Return value: 0, a
 * positive hipError_t, PVNET_E_BADARG (-1: a null pointer other than src2 / res, src2 given without c2 or c2 without src2, a size < 1,
 * an unknown type or activation code, w not 16-byte aligned) or PVNET_E_UNSUPPORTED (-3: widths, stride or dilation outside the ranges
 * above, b > 65535, h or w_ > 32768).
 *
 * KERNEL SHAPE.  A workgroup of four waves takes a tile of 32 x 8 output pixels and a GROUP OF 128 OUTPUT CHANNELS
 * (PVNET_TRUNK_CO_GROUP): wave v owns the 32 channels 128 group + 32 v (a wave whose channels are beyond co only helps staging) and all
 * 256 pixels, eight accumulator blocks of 32 channels x 32 pixels.  Work items (group, tile) are walked group slowest, so the
 * workgroups in flight read the same at most 1.2 MB of weights (L2).  Per item the workgroup walks the chunks of 32 channels of In:
 * it stages the chunk of the tile's receptive field -- (31 s + 2 d + 1) x (7 s + 2 d + 1) pixels, 40 x 16 at d = 4 -- into LDS, rounded
 * to bfloat16, a pixel's 32 channels contiguous in a record of 80 bytes (the decoder's stride: the sixteen lanes of a ds_read_b128
 * group on sixteen different 16-byte slots at s = 1), zero outside the image; then 18 k-steps per chunk (9 taps x 2 halves of the
 * chunk): the A operand is the wave's weight fragment, ONE 16-byte load per lane from the packed image, used for all eight pixel
 * blocks, the B operand one ds_read_b128 per lane and pixel block -- one LDS read and one eighth of a global load per MFMA, and no
 * weight fragment is loaded twice by a workgroup.  Pixels are on the lanes, so a store instruction writes 32 consecutive pixels of a
 * channel plane.  The stride-2 geometry runs the same loop over a 65 x 17 field (its LDS reads are two-way conflicted: it occurs once
 * per network).  The staging has TWO ADDRESSING PATHS, chosen per source on the host: where no stride of the source is negative and one
 * image of it spans less than 2^31 bytes -- every tensor torch can hand over short of a 2 GB image -- a load's address is a scalar base
 * and a 32-bit offset and five staging items of a lane are in flight; otherwise (a negative stride, which only a caller of this C ABI
 * can pass, or a larger image) every load has a 64-bit address of its own and two items are in flight, which is all that fits beside the
 * 128 accumulator registers.  Both compute the same bits; the second path's speed has not been measured.
 */
#ifndef PVNET_TRUNK_H_
#define PVNET_TRUNK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_TRUNK_ABI_VERSION 1
#define PVNET_TRUNK_MAX_WIDTH 512   /* c1 + c2 and co, at most; each a multiple of 32 */
#define PVNET_TRUNK_CO_GROUP 128    /* output channels of a workgroup (see KERNEL SHAPE) */
/* element types of src1, src2, res and out */
#define PVNET_TRUNK_T_F32  0
#define PVNET_TRUNK_T_F16  1
#define PVNET_TRUNK_T_BF16 2
/* activations */
#define PVNET_TRUNK_ACT_NONE  0
#define PVNET_TRUNK_ACT_RELU  1
#define PVNET_TRUNK_ACT_LEAKY 2     /* LeakyReLU(0.1) */

int pvnet_trunk_abi_version(void);

int pvnet_conv3x3_fused(const void* src1, int src1_type, const int64_t src1_strides[4],
                        const void* src2, int src2_type, const int64_t src2_strides[4],
                        const void* res, int res_type, const int64_t res_strides[4],
                        const void* w, const float* bias,
                        int b, int h, int w_, int c1, int c2, int co, int stride, int dilation, int act,
                        void* out, int out_type, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_TRUNK_H_ */
