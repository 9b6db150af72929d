/* pvnet_color.h -- C ABI of libpvnet_color.so: the colour jitter of a training batch on the device, alone (pvnet_color_jitter) or
 * fused behind the geometric augmentation (pvnet_augment_jitter).
 *
 * Every training sample of the reference passes through transforms.ColorJitter(brightness, contrast, saturation, hue)
 * (lib/datasets/linemod_dataset.py:185-190, applied at :233-234) between the geometric augmentation and ToTensor + Normalize.  Its
 * arithmetic lives in torchvision 0.2.1 and Pillow, which are not part of the reference tree: adjust_brightness, adjust_contrast and
 * adjust_saturation are ImageEnhance.Brightness, .Contrast and .Color, adjust_hue is convert('HSV'), a wrapped uint8 add on H and
 * convert('RGB').  THE DEFINITION below is THIS PROJECT'S OWN TEXT of that arithmetic, one IEEE operation per step, and it is held to
 * Pillow byte for byte.  Checked against Pillow 12.2.0 (tests/test_color_cpu.py, through tests/pillow_jitter_oracle.py, which
 * restates torchvision's four functions with Pillow calls alone):
 *   - steps B, S and C (the mean luma m included) equal ImageEnhance's result in every byte of the images and factors tested;
 *   - step H's forward conversion equals convert('HSV') on all 2^24 colours, and its back conversion equals convert('RGB') on
 *     every (h, s, v) that the forward conversion produces, under every shift of h;
 *   - the float32 product of the shift lands on the integer of torchvision's double product for every factor tested;
 *   - the whole chain equals torchvision's for all 24 orders and every subset of absent steps.
 * tests/golden/color_pillow.npz is the record: Pillow's bytes for 48 chains over an image of the colours on which a float32-only
 * hue differs from Pillow's, which the kernels (pvnet_amd/csrc/color_jitter.hip) reproduce on the device.  The header, its numpy
 * restatement (tests/color_restatement.py) and the kernels are held to each other bit for bit.
 *
 * The values of step H changed without a change of PVNET_COLOR_ABI_VERSION (no signature or layout changed; this text is the
 * record).  Before, H's forward hue was computed in float32 throughout, which gives another h than Pillow on 72 036 of the 2^24
 * colours (one step of h, up to 6 grey levels after the back conversion), and the back conversion's f was x - floor(x) of the
 * float32 x = ((float)h 6f) / 255f, which gives another byte than Pillow on two (h, s, v).
 *
 * `blur` needs no kernel: the reference calls blur_image(rgb, k) at linemod_dataset.py:232 and discards what it returns
 * (augmentation.py:204-205 returns a new array), so `blur: true` changes no pixel.
 *
 * Randomness is an input: `uniforms [b,5]` float64 holds per image five independent U[0,1) numbers u0..u4.
 *
 * THE DEFINITION, per image of N = height width RGB uint8 pixels.  float32 arithmetic is not contracted: one IEEE operation per
 * step, in the order written; (float) converts an integer exactly; trunc, floor and rint (half to even) give integers.
 *
 *   Factors, each computed in float64 (one operation per step, in the order written) and then rounded once to float32:
 *     range(x, u) = lo + (hi - lo) u   with lo = max(0, 1 - x), hi = 1 + x
 *     fb = range(brightness, u0),  fc = range(contrast, u1),  fs = range(saturation, u2),  fh = -hue + (2 hue) u3
 *   Skipped steps: a step whose configured range (brightness, contrast, saturation, hue) is 0 is absent from the chain, as
 *   torchvision omits it; its uniform is ignored.
 *   Order: k = min(floor(24 u4), 23) indexes the 24 permutations of (B, C, S, H) in lexicographic order (k = 0: B C S H, k = 1:
 *   B C H S, ..., k = 23: H S C B); absent steps are dropped from the chosen permutation.
 *
 *   L(r,g,b) = (19595 r + 38470 g + 7471 b + 32768) >> 16                                     (integers)
 *   blend(d, x, f) = trunc(clip(d + f (x - d), 0, 255)):  x - d in integers, then (float)(x - d), one float32 multiply by f, one
 *   float32 add to (float)d, the clip, the truncation.
 *
 *   B  c <- blend(0, c, fb) per channel.
 *   S  c <- blend(L(r,g,b), c, fs) per channel, L of the pixel before the step.
 *   C  S_L = the integer sum of L over all N pixels of the image as it stands when the step is reached,
 *      m = (2 S_L + N) / (2 N) by integer division (the mean luma, halves rounded up),  c <- blend(m, c, fc) per channel.
 *   H  to HSV:  maxc, minc of (r,g,b), v = maxc.  minc == maxc: h = s = 0.  Otherwise cr = maxc - minc,
 *        s = trunc((255f (float)cr) / (float)maxc),
 *        rc = (float)(maxc - r) / (float)cr, gc and bc likewise,
 *        t = bc - gc in float32 if r == maxc; else (2.0 + (double)rc) - (double)bc if g == maxc, else (4.0 + (double)gc) -
 *        (double)rc: two float64 operations, the result rounded once to float32          (Pillow's C: double literals, float variables)
 *        x = (double)t / 6.0 + 1.0 in float64 (a true division, no reciprocal, not contracted),
 *        hf = x - floor(x) in float64, rounded once to float32,  h = trunc((double)hf 255.0).
 *      the shift:  h <- (h + (trunc(fh 255f) mod 256)) mod 256        (mod with a non-negative result)
 *      back to RGB:  s == 0: r = g = b = v.  Otherwise
 *        i = (6 h) / 255 by integer division (0 .. 6),  f = (float)(6 h - 255 i) / 255f  (for each of the 256 h the float32 that
 *        Pillow's (float)((float)h 6.0 / 255.0 - i) is),  sg = (float)s / 255f,  fv = (float)v,
 *        p  = clip(rint(fv (1f - sg)), 0, 255),
 *        q  = clip(rint(fv (1f - sg f)), 0, 255),
 *        t' = clip(rint(fv (1f - sg (1f - f))), 0, 255),
 *      (r,g,b) = (v,t',p), (q,v,p), (p,v,t'), (p,q,v), (t',p,v), (v,p,q) for i mod 6 = 0 .. 5.
 *      (Pillow forms p, q and t' with float64 products and round(); with this f the float32 products and rint give the same
 *      bytes on all 2^24 (h, s, v).)
 *   Normalise:  ((float)c / 255f - mean_c) / std_c  in float32, rounded once to the output type: the last line of
 *   include/pvnet_augment.h.  Where a mask is given and maskmul of the image is not 0, the float32 value is multiplied by
 *   (float)mask before that rounding (the reference's use_mask_out, applied after its transforms: linemod_dataset.py:237-238).
 *
 * S_L is an integer sum: whatever the order of its reduction, two calls agree bit for bit.
 */
#ifndef PVNET_COLOR_H
#define PVNET_COLOR_H

#include <stddef.h>
#include <stdint.h>

#include "pvnet_augment.h" /* PvnetAugmentConfig, PVNET_AUGMENT_OUT_*; through it PVNET_E_*, PVNET_MASK_* */

#define PVNET_COLOR_ABI_VERSION 1

#define PVNET_COLOR_UNIFORMS 5 /* doubles per image in the jitter's `uniforms` */

/* the steps, as the permutations of `Order` number them */
#define PVNET_COLOR_STEP_B 0
#define PVNET_COLOR_STEP_C 1
#define PVNET_COLOR_STEP_S 2
#define PVNET_COLOR_STEP_H 3

typedef struct PvnetColorConfig {
    double brightness, contrast, saturation, hue; /* the arguments of the reference's ColorJitter; 0: the step is absent */
    float mean[3], std[3];
} PvnetColorConfig;

#ifdef __cplusplus
extern "C" {
#endif

int pvnet_color_abi_version(void);

/* Bytes of workspace pvnet_augment_jitter needs for b images of height x width output pixels: the plans, 8 bytes per image for S_L and
 * the warped uint8 image, 3 bytes per pixel.  With height == 0 and width == 0: what pvnet_color_jitter needs (S_L alone).  0 for b
 * outside 1 .. 65535 or a negative size.  The workspace may hold anything on entry: the calls zero what they add into, on the stream. */
size_t pvnet_color_workspace_bytes(int b, int height, int width);

/* Enqueues the jitter and the normalisation of b images on `stream`: a small launch that zeroes S_L (a kernel, not a memset: see
 * pvnet_amd/csrc/color_jitter.hip) and two more (the statistics kernel runs the steps before C and reduces S_L per image; the apply
 * kernel runs the whole chain and normalises), or the apply kernel alone where contrast == 0.  No allocation, no synchronisation, capturable.  Arguments are checked before any HIP call.  All pointers but
 * `cfg`, `stream` and the stride arrays are device pointers; strides are in elements.
 *
 *   rgb       [b,h,w,3] uint8, strides rgb_strides (b, h, w); the channel stride is 1
 *   uniforms  [b,5] float64, contiguous
 *   mask      NULL, or [b,h,w] of mask_dtype PVNET_MASK_U8 / _I32 / _I64, strides mask_strides
 *   maskmul   NULL, or [b] int32: the images whose normalised value is multiplied by (float)mask.  Both or neither.
 *   image     [b,3,h,w] contiguous, image_dtype PVNET_AUGMENT_OUT_*
 *
 * Each lane of the apply kernel owns eight consecutive pixels of a row and stores 16 bytes at a time where w is a multiple of 8 and
 * `image` is 16-byte aligned; element by element otherwise.
 *
 * Returns 0, PVNET_E_BADARG (a range that is negative, not finite or above 1e6, hue above 0.5, ...), PVNET_E_WORKSPACE,
 * PVNET_E_UNSUPPORTED (b > 65535, a side above 32768, h w above 2^30, other mask types) or a hipError_t.  b == 0 returns 0 and
 * enqueues nothing. */
int pvnet_color_jitter(const uint8_t* rgb, const int64_t rgb_strides[3], const double* uniforms, int b, int h, int w,
                       const PvnetColorConfig* cfg, const void* mask, int mask_dtype, const int64_t mask_strides[3], const int32_t* maskmul,
                       void* image, int image_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* pvnet_augment (include/pvnet_augment.h: the same arguments, checks and results) with the jitter between its warp and its
 * normalisation.  Five launches: the plan; the warp, which writes the warped uint8 image into the workspace, and `mask_out`; the
 * two kernels above reading it (`mask_out` and the plan's use_mask_out draw are their mask and maskmul).  The plan and the per-pixel
 * part of the warp are the code pvnet_augment runs (pvnet_amd/csrc/augment_warp.h): `mask_out`, `hcoords_out` and `status` are what
 * pvnet_augment writes, and with all four ranges 0 so is `image`, with one restriction: the use_mask_out multiply reads `mask_out`,
 * that is the mask as mask_out_dtype holds it, where pvnet_augment multiplies by the source's value.  The two differ only where a
 * PVNET_MASK_I32 / _I64 source mask holds values outside 0 .. 255 and mask_out_dtype is PVNET_MASK_U8 (which keeps the low 8 bits);
 * ask for PVNET_MASK_I64 there.
 *
 *   jitter          brightness, contrast, saturation, hue; its mean and std are not read (`cfg`'s are)
 *   jitter_uniforms [b,5] float64, contiguous
 *   workspace       pvnet_color_workspace_bytes(b, height, width) bytes, 16-byte aligned */
int pvnet_augment_jitter(const uint8_t* rgb, const int64_t rgb_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3],
                         const double* hcoords, const double* uniforms, int b, int h, int w, int vn, int height, int width,
                         const PvnetAugmentConfig* cfg, uint64_t seed, const PvnetColorConfig* jitter, const double* jitter_uniforms,
                         void* image, int image_dtype, void* mask_out, int mask_out_dtype, double* hcoords_out, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PVNET_COLOR_H */
