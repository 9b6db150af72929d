/* pvnet_augment.h -- C ABI of libpvnet_augment.so: the geometric augmentation of a training batch on the device.
 *
 * The reference augments on the host, per sample (LineModDatasetRealAug.augmentation, lib/datasets/linemod_dataset.py:254-290, and
 * lib/datasets/augmentation.py), then ToTensor + Normalize, and ships a float32 image and an int64 mask: 20 bytes per pixel.  Since the
 * targets are made from the key-points (include/pvnet_targets.h) a sample's supervision is a mask and `hcoords [vn,3]`, so the same
 * augmentation is: warp a uint8 image and a mask, push 3 vn numbers through a few affine updates.  pvnet_augment does that for a batch
 * from the decoded uint8 sample; pvnet_normalize is the identity plan (the reference's test_img_transforms).
 *
 * Randomness is an input: `uniforms [b,14]` float64 holds per image twelve independent U[0,1) numbers u0..u11 and, at 12 and 13,
 * cos and sin of the rotation angle  (rot_ang_min + (rot_ang_max - rot_ang_min) u5) pi / 180  computed on the host (the only
 * transcendental values of the definition).  The fill of the masked-out rectangle is counter based (pvnet_rng.h, PVNET_TAG_AUG).
 *
 * THE DEFINITION, per image.  All arithmetic is float64, not contracted, one IEEE operation per step in the order written (fma where
 * fma is written); integers come from floor; `fg` means mask != 0.
 *
 *   uniform(lo,hi,u) = lo + (hi - lo) u
 *   randint(lo,hi,u) = min(floor(lo + u (hi - lo)), hi - 1);  where hi <= lo (the reference raises): lo, and PVNET_AUGMENT_S_RANGE
 *
 *   0  n0 = number of fg pixels.  n0 == 0: PVNET_AUGMENT_S_NO_FOREGROUND and the no-foreground path (step 4b).
 *   1  mask-out (mask_out_instance), if `mask` and n0 > 0 and u0 < 0.5:  (xmin,xmax,ymin,ymax) the bbox of fg;
 *        x_side = floor((xmax - xmin) uniform(min_mask,max_mask,u1) / 2),  y_side likewise with u2,
 *        x_loc = randint(xmin,xmax,u3),  y_loc = randint(ymin,ymax,u4);
 *      the rectangle is rows [y_loc - y_side, y_loc + y_side) and columns [x_loc - x_side, x_loc + x_side) under numpy's slice rule,
 *      as the reference indexes it: a stop is clipped at h (w); a negative start s counts from the end, max(s + h, 0), which makes
 *      the rectangle empty whenever 2 side <= h (always for max_mask <= 1).  Inside it every source image tap reads
 *        pvnet_rng_below(pvnet_rng_u32(seed, PVNET_TAG_AUG, image, (y w + x) 3 + c), 255)
 *      and every source mask tap reads 0.  n1 = fg pixels left.  n1 == 0 < n0: PVNET_AUGMENT_S_EMPTIED and the no-foreground path.
 *   2  rotation (rotate_instance), if `rotation`:  (cx, cy) = (sum x / n1, sum y / n1) over the fg pixels left (integer sums),
 *        a = cos, b = sin;  R = [[a, b, (1 - a) cx - b cy], [-b, a, b cx + (1 - a) cy]]     (getRotationMatrix2D, scale 1)
 *      on the canvas w x h; outside the source is 0.  The inverse map of a canvas point (X, Y) is
 *        sx = a (X - R02) - b (Y - R12),   sy = b (X - R02) + a (Y - R12)
 *      and canvas pixel (X, Y) of the rotated MASK is the source mask at (floor(sx + 0.5), floor(sy + 0.5)): a nearest warp.
 *      Without rotation a = 1, b = 0, R02 = R12 = 0, which makes the map exact.
 *   3  resize (crop_resize_instance_v2), if `crop` and u6 < 0.8:  (xmin..ymax) the bbox of the rotated mask (none:
 *      PVNET_AUGMENT_S_DEGENERATE, no resize, step 4b),  xlen = xmax - xmin, ylen = ymax - ymin,
 *        rmin = max(resize_wmin / xlen, resize_hmin / ylen),  rmax = min(resize_wmax / xlen, resize_hmax / ylen),
 *        ratio = uniform(rmin,rmax,u7),  h2 = floor(h ratio),  w2 = floor(w ratio),  s_w = w / w2,  s_h = h / h2.
 *      Image: resized column X reads canvas abscissa clamp((X + 0.5) s_w - 0.5, 0, w - 1), rows likewise.  Mask: resized pixel (X, Y)
 *      is canvas pixel (min(floor(X s_w), w - 1), min(floor(Y s_h), h - 1)).  xlen or ylen 0, a size outside 1 .. 2^24 - 1 or a resized
 *      mask without fg: PVNET_AUGMENT_S_DEGENERATE and no resize (the reference divides by zero or raises).
 *   4a crop or pad to height x width (crop_or_padding_to_fixed_size_instance), if `crop`:  (h2, w2) the current size, (hmin..wmax)
 *      the bbox of the current (resized) mask, fh = hmax - hmin, fw = wmax - wmin, hpad = height >= h2, wpad = width >= w2,
 *        hrmax = trunc(min(hmin + overlap_ratio fh, h2 - height)),  hrmin = trunc(max(hmin + overlap_ratio fh - height, 0)),
 *        hbeg = hpad ? 0 : randint(hrmin,hrmax,u8);   the same for the columns with u9;
 *      output row Y is current row Y - hoff + hbeg with hoff = hpad ? (height - h2) / 2 : 0, columns likewise; what falls outside the
 *      current image is 0.  Without `crop` nothing moves and (height, width) must be (h, w).
 *   4b the no-foreground path (crop_or_padding_to_fixed_size, whatever `crop` says):  hbeg = hpad ? 0 : randint(0, h - height, u8),
 *      wbeg likewise with u9, placed as in 4a; the key-points are NOT moved (the reference does not pass them).
 *   5  flip, if `flip` and u10 < 0.5:  output column X is column width - 1 - X.
 *   6  use_mask_out, if `use_mask_out` and u11 < 0.1:  the normalised image is multiplied by (float)(output mask), in float32.
 *
 *   Key-points, in this order, each line one step of the reference:
 *     2  x' = fma(z, R02, fma(y, b, x a)),  y' = fma(z, R12, fma(y, a, x (-b))),  z' = fma(z, 1, fma(y, 0, x 0))
 *        (hcoords @ [R; 0 0 1]^T as a three-term dot product accumulated by fused multiply-adds: what the FMA dgemm kernel behind
 *        np.matmul computed on the machine that recorded tests/golden/augment.npz; a BLAS that accumulates otherwise may differ from
 *        this definition in the last bit)
 *     3  x *= ratio, y *= ratio        4a  x -= wbeg z, y -= hbeg z; if hpad or wpad: x += woff z, y += hoff z
 *     5  x -= (width / 2) z;  x = -x;  x += (width / 2) z
 *
 *   Pixels are produced in ONE pass through the composed inverse map (5, 4, 3, 2 backwards), where the reference interpolates twice
 *   (warpAffine, then resize): a stated deviation.  At the source point (sx, sy): x0 = floor(sx), fx = sx - x0, likewise y; the taps
 *   v00 = (x0, y0), v01 = (x0 + 1, y0), v10 = (x0, y0 + 1), v11 = (x0 + 1, y0 + 1), 0 outside the source;
 *     top = v00 (1 - fx) + v01 fx,  bot = v10 (1 - fx) + v11 fx,  v = rint(top (1 - fy) + bot fy)        (half to even, 0 .. 255)
 *   then  ((float)v / 255f - mean_c) / std_c  in float32, rounded once to the output type.  The output mask is the source mask at the
 *   nearest pixel of the composed map (the mask chain of steps 4, 3, 2).
 *
 * No atomics, integer reductions, fixed orders: two calls agree bit for bit.
 */
#ifndef PVNET_AUGMENT_H
#define PVNET_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#include "pvnet_vote.h" /* PVNET_E_*, PVNET_MASK_U8 / _I32 / _I64 */

#define PVNET_AUGMENT_ABI_VERSION 1

/* PvnetAugmentConfig.flags: the reference's configuration switches of the same names */
#define PVNET_AUGMENT_F_MASK 1
#define PVNET_AUGMENT_F_ROTATION 2
#define PVNET_AUGMENT_F_CROP 4
#define PVNET_AUGMENT_F_FLIP 8
#define PVNET_AUGMENT_F_USE_MASK_OUT 16

/* element type of the image written */
#define PVNET_AUGMENT_OUT_F32 0
#define PVNET_AUGMENT_OUT_BF16 1
#define PVNET_AUGMENT_OUT_F16 2

/* status bits, per image */
#define PVNET_AUGMENT_S_RANGE 1         /* a randint with hi <= lo took lo */
#define PVNET_AUGMENT_S_EMPTIED 2       /* mask-out left no foreground: the no-foreground path was taken */
#define PVNET_AUGMENT_S_DEGENERATE 4    /* the resize was skipped (see step 3) */
#define PVNET_AUGMENT_S_NO_FOREGROUND 8 /* the mask had no foreground */

#define PVNET_AUGMENT_UNIFORMS 14 /* doubles per image in `uniforms` */

typedef struct PvnetAugmentConfig {
    uint32_t flags;
    uint32_t reserved; /* 0 */
    double min_mask, max_mask, overlap_ratio, resize_hmin, resize_hmax, resize_wmin, resize_wmax;
    float mean[3], std[3];
} PvnetAugmentConfig;

#ifdef __cplusplus
extern "C" {
#endif

int pvnet_augment_abi_version(void);

/* bytes of workspace a call for b images needs (0 for b outside 1 .. 65535); it may hold anything on entry */
size_t pvnet_augment_workspace_bytes(int b);

/* Enqueues the augmentation of b images on `stream`: two launches, no allocation, no synchronisation, capturable.  Arguments are
 * checked before any HIP call.  All pointers but `cfg`, `stream` and the stride arrays are device pointers; strides are in elements.
 *
 *   rgb         [b,h,w,3] uint8, strides rgb_strides (b, h, w); the channel stride is 1
 *   mask        [b,h,w], mask_dtype PVNET_MASK_U8 / _I32 / _I64, strides mask_strides
 *   hcoords     [b,vn,3] float64, contiguous;  uniforms [b,14] float64, contiguous (see above)
 *   image       [b,3,height,width] contiguous, image_dtype PVNET_AUGMENT_OUT_*
 *   mask_out    [b,height,width] contiguous, mask_out_dtype PVNET_MASK_U8 or PVNET_MASK_I64
 *   hcoords_out [b,vn,3] float64, contiguous (may be `hcoords` itself);  status [b] int32
 *
 * Each lane of the warp kernel owns eight consecutive pixels of an output row and stores 16 bytes at a time where width is a
 * multiple of 8 and `image` and `mask_out` are 16-byte aligned; element by element otherwise.
 *
 * Returns 0, PVNET_E_BADARG, PVNET_E_WORKSPACE, PVNET_E_UNSUPPORTED (b > 65535, a side above 32768, h w or height width above 2^30,
 * other mask types) or a hipError_t.  b == 0 returns 0 and enqueues nothing. */
int pvnet_augment(const uint8_t* rgb, const int64_t rgb_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3],
                  const double* hcoords, const double* uniforms, int b, int h, int w, int vn, int height, int width,
                  const PvnetAugmentConfig* cfg, uint64_t seed, void* image, int image_dtype, void* mask_out, int mask_out_dtype,
                  double* hcoords_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The identity plan: image [b,3,h,w] = ((float)rgb / 255f - mean) / std, rounded once to image_dtype.  Only `mean` and `std` of
 * `cfg` are read.  One launch, no workspace.  Same returns. */
int pvnet_normalize(const uint8_t* rgb, const int64_t rgb_strides[3], int b, int h, int w, const PvnetAugmentConfig* cfg, void* image,
                    int image_dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PVNET_AUGMENT_H */
