/* pvnet_classes.h -- C ABI of libpvnet_classes.so: the first kernel of the voting layer for a mask of CLASS LABELS.
 *
 * The reference's ransac_voting_layer_v2 (lib/ransac_voting_gpu_layer/ransac_voting_gpu.py:99-215) votes once per class
 * k + 1 = 1 .. class_num - 1 on the pixels `mask[bi] == k + 1` of one shared vector field.  Here a class of an image is a VIRTUAL
 * IMAGE of the voting library: virtual image v = i * (num_classes - 1) + k is (image i, label k + 1), and after its first kernel
 * the voting library (include/pvnet_vote.h) reads the mask never again.  pvnet_class_split is that first kernel for all
 * B = b * (num_classes - 1) virtual images at once: it reads every label ONCE and writes, for every v, exactly what the mask
 * kernel of pvnet_vote_v3 writes for the mask `labels[i] == k + 1` into a workspace laid out for B images:
 *   bits   uint64 [B][words]                 one bit per pixel (words = ceil(h w / 64)); every word is written, zero words too
 *   seg0   int32  [B][nseg]                  pixels of the class in every 4096-pixel segment (nseg = ceil(words / 64))
 *   cum    uint16 [B][nseg][1536]            where max_num < h w: the cumulative histogram of the thinning bins (pvnet_thin_bin of
 *                                            pvnet_rng.h) of every (class, segment) that HAS pixels, drawn with the key
 *                                            pvnet_rng_key(seed, PVNET_TAG_SUB, image_base + v) at the pixel's own index y w + x;
 *                                            rows of segments without pixels of the class are not written (nothing reads them)
 * i.e. PvnetVoteLayout's off_bits, the second array behind off_seg and the histograms behind both; pvnet_vote_v3_prepared with
 * src_div = num_classes - 1 then runs the rest of the layer on them.
 *
 * Labels are compared on their FULL integer value, as `mask[bi] == k + 1` does (not on their low byte): label 0, negative labels
 * and labels >= num_classes belong to no class.  mask_dtype is a PVNET_MASK_* code of pvnet_vote.h (U8 .. F32; U8 reads unsigned
 * bytes, I16 / I32 / I64 signed integers; a float32 label belongs to class c when it EQUALS c).
 *
 * pvnet_class_split_logits: the same on the backbone's class logits seg_pred [b,C,h,w] (element strides seg_strides[4], element
 * type logits_type), num_classes = C; a pixel's label is its arg-max over the C planes with torch's rules: the first maximum wins, a
 * NaN counts as the maximum.
 *
 * Both only enqueue ONE launch on `stream`: no allocation, no synchronisation, capturable in a graph.  Arguments are checked before
 * any HIP call.  Return value: 0, a positive hipError_t, or PVNET_E_BADARG (-1: a null pointer, a size < 1, num_classes outside
 * 2 .. PVNET_CLASSES_MAX, an unknown type code, max_num < 0, max_num < h w without `cum`, a misaligned output) / PVNET_E_UNSUPPORTED
 * (-3: h w > 2^30 or more than 65535 virtual images).
 */
#ifndef PVNET_CLASSES_H_
#define PVNET_CLASSES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_CLASSES_ABI_VERSION 1
/* classes INCLUDING the background (label 0).  The bit words of a segment's num_classes - 1 classes collect in the workgroup's
 * LDS, 512 bytes per class, beside the 6 KB thinning histogram: 63 classes are 31.5 KB, so four workgroups (every wave slot of a
 * compute unit) still fit its 160 KB.  Occlusion LINEMOD needs 9, the "fuse" images 14, 21 objects 22. */
#define PVNET_CLASSES_MAX 64
/* element types of seg_pred */
#define PVNET_CLASSES_LOGITS_F32  0
#define PVNET_CLASSES_LOGITS_F16  1
#define PVNET_CLASSES_LOGITS_BF16 2

int pvnet_classes_abi_version(void);

int pvnet_class_split(const void* labels, int mask_dtype, const int64_t mask_strides[3], int num_classes,
                      int b, int h, int w, int max_num, uint64_t seed, int image_base,
                      uint64_t* bits, int32_t* seg0, uint16_t* cum, void* stream);

int pvnet_class_split_logits(const void* seg_pred, int logits_type, const int64_t seg_strides[4], int num_classes,
                             int b, int h, int w, int max_num, uint64_t seed, int image_base,
                             uint64_t* bits, int32_t* seg0, uint16_t* cum, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_CLASSES_H_ */
