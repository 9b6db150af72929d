// augment.hip -- the geometric augmentation of a training batch on the device.  The whole of libpvnet_augment.so; C ABI and THE
// DEFINITION: include/pvnet_augment.h (every step named below is a step of that definition; the reference is
// LineModDatasetRealAug.augmentation, lib/datasets/linemod_dataset.py:254-290, and lib/datasets/augmentation.py).  The plan's body, the
// per-pixel part of the warp and the stores live in augment_warp.h, which color_jitter.hip (libpvnet_color.so) includes too.
//
//   augment_plan_kernel      grid (images), 512 threads.  Up to four passes over the image's mask, each an integer block reduction
//                            (sums, minima, maxima: no atomics, no floating reduction): the bbox and the count of the foreground; the
//                            count and the coordinate sums outside the masked-out rectangle; the bbox of the rotated mask through
//                            the inverse map; where the image is resized, the bbox of the foreground pixels that the resize's
//                            nearest map hits (the bbox of the resized mask follows from it, the map being monotone per axis).
//                            Every thread derives the plan from the reduced values (the same arithmetic on the same numbers);
//                            thread 0 writes the plan and the status, threads k < vn the key-points.
//   augment_warp_kernel<T,V> grid (lanes of 8 pixels / 256, images), output stationary.  A lane owns eight consecutive pixels of
//                            an output row: composed inverse map in float64, four uint8 taps per channel (the source is 0.9 MB per
//                            image at 480 x 640 and stays in L2), bilinear, rounded to 0 .. 255, normalised in float32, and the
//                            mask at the nearest source pixel.  V: 16 bytes per store and plane (width a multiple of 8, aligned
//                            outputs); else element by element.  The plan is read at a block-uniform address.  No LDS.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "augment_warp.h"   // the plan's body, the per-pixel part of the warp and the stores: shared with color_jitter.hip
#include "pvnet_augment.h"
#include "vote_common.h"   // PVNET_SPARE_VGPRS

// no contraction: every product and sum rounds as the float64 restatement's separate operations do (fma only where written)
#pragma clang fp contract(off)

namespace {

// the spare-VGPR granule of each kernel (tools/check_kernel_resources.py --augment holds them to it)
#define AUG_PLAN_SPARE 95
#define AUG_WARP_SPARE 127

struct WarpArgs {
    Source S;
    float mean[3], std[3];
    int height, width, mask_out_dtype;
    void* image;
    void* mask_out;   // NULL: pvnet_normalize
};

__global__ __launch_bounds__(PLAN_T) void augment_plan_kernel(PlanArgs A, const double* __restrict__ uniforms, const double* hcoords) {
    PVNET_SPARE_VGPRS(AUG_PLAN_SPARE);
    __shared__ long long sh[PLAN_SH];
    augment_plan_body(A, uniforms, hcoords, sh);
}

// OUT: PVNET_AUGMENT_OUT_*;  VEC: 16 bytes per store (width % 8 == 0, aligned outputs)
template <int OUT, bool VEC>
__global__ __launch_bounds__(WARP_T) void augment_warp_kernel(WarpArgs A, const Plan* __restrict__ plans) {
    PVNET_SPARE_VGPRS(AUG_WARP_SPARE);
    const Source& S = A.S;
    const int bi = blockIdx.y, width = A.width, height = A.height;
    const int lanes_per_row = (width + PPL - 1) / PPL;
    const long long lane = (long long)blockIdx.x * WARP_T + threadIdx.x;
    const int Y = (int)(lane / lanes_per_row);
    if (Y >= height) return;
    const int X0 = (int)(lane - (long long)Y * lanes_per_row) * PPL;
    Plan P;
    if (plans) P = plans[bi];
    else identity_plan(S, P);
    const uint8_t* __restrict__ img = S.rgb + (int64_t)bi * S.rs[0];
    const uint32_t key = pvnet_rng_key(S.seed, PVNET_TAG_AUG, (uint32_t)bi);
    float o[3][PPL];
    long long mo[PPL];
    const int yc = Y - P.hoff, y2 = yc + P.hbeg;
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
        double val[3];
        long long m;
        warp_pixel(S, P, img, key, bi, X0 + i, yc, y2, width, val, m);
        mo[i] = m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f = ((float)val[c] / 255.0f - A.mean[c]) / A.std[c];
            if (P.maskmul) f = f * (float)m;
            o[c][i] = f;
        }
    }
    // ---- stores
    const size_t plane = (size_t)height * width, row = (size_t)Y * width + X0;
    store_planes<OUT, VEC>(A.image, bi, plane, row, X0, width, o);
    if (A.mask_out) store_mask<VEC>(A.mask_out, A.mask_out_dtype, bi, plane, row, X0, width, mo);
}

int launch_warp(const WarpArgs& A, int b, int image_dtype, const Plan* plans, hipStream_t s) {
    const bool vec = A.width % PPL == 0 && aligned16(A.image) && (!A.mask_out || aligned16(A.mask_out));
    const long long lanes = (long long)((A.width + PPL - 1) / PPL) * A.height;
    const dim3 grid((unsigned)((lanes + WARP_T - 1) / WARP_T), (unsigned)b), block(WARP_T);
#define AUG_LAUNCH(OUT)                                                                        \
    do {                                                                                       \
        if (vec) hipLaunchKernelGGL((augment_warp_kernel<OUT, true>), grid, block, 0, s, A, plans); \
        else hipLaunchKernelGGL((augment_warp_kernel<OUT, false>), grid, block, 0, s, A, plans);    \
    } while (0)
    if (image_dtype == PVNET_AUGMENT_OUT_F32) AUG_LAUNCH(PVNET_AUGMENT_OUT_F32);
    else if (image_dtype == PVNET_AUGMENT_OUT_BF16) AUG_LAUNCH(PVNET_AUGMENT_OUT_BF16);
    else AUG_LAUNCH(PVNET_AUGMENT_OUT_F16);
#undef AUG_LAUNCH
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int pvnet_augment_abi_version(void) { return PVNET_AUGMENT_ABI_VERSION; }

size_t pvnet_augment_workspace_bytes(int b) { return b > 0 && b <= MAX_B ? (size_t)b * sizeof(Plan) : 0; }

int pvnet_augment(const uint8_t* rgb, const int64_t rgb_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3],
                  const double* hcoords, const double* uniforms, int b, int h, int w, int vn, int height, int width,
                  const PvnetAugmentConfig* cfg, uint64_t seed, void* image, int image_dtype, void* mask_out, int mask_out_dtype,
                  double* hcoords_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_augment(rgb, rgb_strides, mask, mask_dtype, mask_strides, hcoords, uniforms, b, h, w, vn, height, width, cfg, image,
                                     image_dtype, mask_out, mask_out_dtype, hcoords_out, status))
        return rc;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_augment_workspace_bytes(b)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PlanArgs PA;
    PA.S = make_source(rgb, rgb_strides, mask, mask_dtype, mask_strides, h, w, seed);
    PA.cfg = *cfg;
    PA.vn = vn;
    PA.height = height;
    PA.width = width;
    PA.hc_out = hcoords_out;
    PA.status = status;
    PA.plans = static_cast<Plan*>(workspace);
    hipLaunchKernelGGL(augment_plan_kernel, dim3((unsigned)b), dim3(PLAN_T), 0, s, PA, uniforms, hcoords);
    WarpArgs WA;
    WA.S = PA.S;
    for (int c = 0; c < 3; ++c) WA.mean[c] = cfg->mean[c], WA.std[c] = cfg->std[c];
    WA.height = height;
    WA.width = width;
    WA.mask_out_dtype = mask_out_dtype;
    WA.image = image;
    WA.mask_out = mask_out;
    return launch_warp(WA, b, image_dtype, PA.plans, s);
}

int pvnet_normalize(const uint8_t* rgb, const int64_t rgb_strides[3], int b, int h, int w, const PvnetAugmentConfig* cfg, void* image,
                    int image_dtype, void* stream) {
    if (!cfg) return PVNET_E_BADARG;
    if (const int rc = check_source(rgb, rgb_strides, b, h, w)) return rc;
    if (const int rc = check_image(image, image_dtype)) return rc;
    if (!config_ok(cfg->mean, cfg->std)) return PVNET_E_BADARG;
    if (b == 0) return 0;
    WarpArgs WA;
    WA.S = make_source(rgb, rgb_strides, nullptr, PVNET_MASK_U8, nullptr, h, w, 0);
    for (int c = 0; c < 3; ++c) WA.mean[c] = cfg->mean[c], WA.std[c] = cfg->std[c];
    WA.height = h;
    WA.width = w;
    WA.mask_out_dtype = PVNET_MASK_U8;
    WA.image = image;
    WA.mask_out = nullptr;
    return launch_warp(WA, b, image_dtype, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"
