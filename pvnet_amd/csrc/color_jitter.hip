// color_jitter.hip -- the colour jitter of a training batch on the device.  The whole of libpvnet_color.so; C ABI and THE DEFINITION:
// include/pvnet_color.h (every step named below is a step of that definition; the reference is transforms.ColorJitter at
// lib/datasets/linemod_dataset.py:185-190, applied at :233-234).
//
//   color_stats_kernel        grid (lanes of 8 pixels / 256, images).  Runs the steps of the image's chain that come before C and adds
//                             the integer luma of its pixels into the image's S_L: a wave reduction, one LDS round, one 64-bit integer
//                             atomic per block (an integer sum: the same value in any order).  Not launched where contrast == 0.
//   color_zero_kernel         zeroes the b sums before it: a kernel, not a memset.  With hipMemsetAsync in its place the captured call
//                             gave a wrong image at the second replay of its graph (profiles/color_memset_graph.txt has the run; the
//                             cause inside the runtime is not established), with this kernel it does not.
//   color_apply_kernel<T,V>   the same grid, output stationary.  A lane owns eight consecutive pixels of a row: 24 bytes in (six dword
//                             loads where the pixels are packed and aligned, bytes otherwise), the whole chain in registers, the
//                             normalisation, the optional multiply by the mask, and the stores of augment.hip's warp (16 bytes per
//                             store and plane where V).  The chain's factors and order are derived per thread from the image's five
//                             uniforms at a block-uniform address.  No LDS.
//   color_plan_kernel,        pvnet_augment_jitter: the plan and the per-pixel part of the warp of pvnet_augment (augment_warp.h, the
//   color_warp_kernel<V>      one copy both libraries compile), the warp writing the rounded uint8 pixel, 3 bytes, into the workspace
//                             instead of normalising it.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "augment_warp.h"
#include "pvnet_color.h"
#include "vote_common.h"   // PVNET_SPARE_VGPRS

// no contraction: every float32 product and sum rounds as the numpy restatement's separate operations do
#pragma clang fp contract(off)

namespace {

// the spare-VGPR granule of each kernel (tools/check_kernel_resources.py --color holds them to it)
#define COLOR_PLAN_SPARE 95
#define COLOR_WARP_SPARE 127
#define COLOR_STATS_SPARE 87
#define COLOR_APPLY_SPARE 79
#define COLOR_ZERO_SPARE 15

constexpr int COLOR_T = WARP_T;
constexpr double MAX_RANGE = 1e6;

struct ColorArgs {
    const uint8_t* rgb;
    int64_t rs[3];
    const void* mask;         // NULL: no multiply
    int64_t ms[3];
    int mask_dtype;
    const int32_t* maskmul;   // element bi * maskmul_stride: multiply image bi by its mask
    int maskmul_stride;
    const double* uniforms;   // [b,5]
    double brightness, contrast, saturation, hue;
    float mean[3], std[3];
    int h, w;
    unsigned long long* sums;   // S_L per image
    void* image;
};

// an image's chain: the float32 factors, the hue shift and the present steps in order, one nibble each from bit 0
struct Chain {
    float fb, fc, fs;
    int hshift;
    uint32_t order;
    int n;
};

__device__ __forceinline__ float range_factor(double x, double u) {
    const double a = 1.0 - x, lo = a > 0.0 ? a : 0.0, hi = 1.0 + x;
    const double d = hi - lo, p = d * u;
    return (float)(lo + p);
}

__device__ __forceinline__ Chain make_chain(const ColorArgs& A, int bi) {
    const double* __restrict__ u = A.uniforms + (size_t)bi * PVNET_COLOR_UNIFORMS;
    Chain ch;
    ch.fb = range_factor(A.brightness, u[0]);
    ch.fc = range_factor(A.contrast, u[1]);
    ch.fs = range_factor(A.saturation, u[2]);
    const double h2 = 2.0 * A.hue, hp = h2 * u[3];
    const float fh = (float)(-A.hue + hp);
    ch.hshift = (int)(fh * 255.0f) & 255;
    const double t = 24.0 * u[4];
    int k = t >= 0.0 && t < 24.0 ? (int)t : (t >= 24.0 ? 23 : 0);
    // the k-th permutation of (B, C, S, H) in lexicographic order: the factorial digits of k pick from what is left
    uint32_t left = 0x3210u;
    const bool present[4] = {A.brightness != 0.0, A.contrast != 0.0, A.saturation != 0.0, A.hue != 0.0};
    ch.order = 0;
    ch.n = 0;
    const int radix[4] = {6, 2, 1, 1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = k / radix[j];
        k -= d * radix[j];
        const uint32_t step = (left >> (4 * d)) & 15u;
        left = (left & ((1u << (4 * d)) - 1u)) | ((left >> (4 * d + 4)) << (4 * d));
        const bool on = step == PVNET_COLOR_STEP_B ? present[0] : (step == PVNET_COLOR_STEP_C ? present[1] : (step == PVNET_COLOR_STEP_S ? present[2] : present[3]));
        if (on) {
            ch.order |= step << (4 * ch.n);
            ++ch.n;
        }
    }
    return ch;
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__device__ __forceinline__ int blend(int d, int x, float f) {
    const float t = f * (float)(x - d);
    float r = (float)d + t;
    r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
    return (int)r;
}

__device__ __forceinline__ int clip_rint(float x) {
    const float r = rintf(x);
    return (int)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

// step H of one pixel
__device__ __forceinline__ void hue_step(int& r, int& g, int& b, int hshift) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b), minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    const int v = maxc;
    int h = 0, s = 0;
    if (minc != maxc) {
        const int cr = maxc - minc;
        const float fcr = (float)cr;
        s = (int)((255.0f * fcr) / (float)maxc);
        const float rc = (float)(maxc - r) / fcr, gc = (float)(maxc - g) / fcr, bc = (float)(maxc - b) / fcr;
        // Pillow writes the hue with double literals and float variables: the sums of the g and b branches, the division by 6 and
        // the fractional part are float64 operations (uncontracted, a true division), each result rounded once to float32
        // One pair of float64 operations for the three branches: the operands are selected first, and the r branch adds 0.0.  Its
        // float64 sum and difference are exact (two float32 quotients in 0 .. 1), so the one rounding gives the float32 bc - gc.
        const bool rmax = r == maxc, gmax = g == maxc;
        const float ta = rmax ? bc : (gmax ? rc : gc), tb = rmax ? gc : (gmax ? bc : rc);
        const double base = rmax ? 0.0 : (gmax ? 2.0 : 4.0);
        const float t = (float)((base + (double)ta) - (double)tb);
        const double x = (double)t / 6.0 + 1.0;
        const float hf = (float)(x - floor(x));
        h = (int)((double)hf * 255.0);
    }
    h = (h + hshift) & 255;
    if (s == 0) {
        r = g = b = v;
        return;
    }
    int i = (6 * h) / 255;   // 0 .. 6
    const float f = (float)(6 * h - 255 * i) / 255.0f;
    const float sg = (float)s / 255.0f, fv = (float)v;
    const float a1 = 1.0f - sg;
    const int p = clip_rint(fv * a1);
    const float sf = sg * f, a2 = 1.0f - sf;
    const int q = clip_rint(fv * a2);
    const float g1 = 1.0f - f, sg1 = sg * g1, a3 = 1.0f - sg1;
    const int t2 = clip_rint(fv * a3);
    i = i >= 6 ? i - 6 : i;
    r = i == 0 || i == 5 ? v : (i == 1 ? q : (i == 4 ? t2 : p));
    g = i == 1 || i == 2 ? v : (i == 0 ? t2 : (i == 3 ? q : p));
    b = i == 3 || i == 4 ? v : (i == 2 ? t2 : (i == 5 ? q : p));
}

// step `op` (block-uniform) of a lane's eight pixels; m: the mean luma of step C
__device__ __forceinline__ void run_step(uint32_t op, const Chain& ch, int m, int (&px)[PPL][3]) {
    if (op == PVNET_COLOR_STEP_B) {
#pragma unroll
        for (int i = 0; i < PPL; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i][c] = blend(0, px[i][c], ch.fb);
    } else if (op == PVNET_COLOR_STEP_C) {
#pragma unroll
        for (int i = 0; i < PPL; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i][c] = blend(m, px[i][c], ch.fc);
    } else if (op == PVNET_COLOR_STEP_S) {
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
            const int l = luma(px[i][0], px[i][1], px[i][2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i][c] = blend(l, px[i][c], ch.fs);
        }
    } else {
#pragma unroll
        for (int i = 0; i < PPL; ++i) hue_step(px[i][0], px[i][1], px[i][2], ch.hshift);
    }
}

// a lane's eight pixels of row Y from column X0 (pixels at or beyond w read as 0)
__device__ __forceinline__ void load_pixels(const ColorArgs& A, int bi, int Y, int X0, int (&px)[PPL][3]) {
    const uint8_t* __restrict__ src = A.rgb + (int64_t)bi * A.rs[0] + (int64_t)Y * A.rs[1] + (int64_t)X0 * A.rs[2];
    if (A.rs[2] == 3 && X0 + PPL <= A.w && (reinterpret_cast<uintptr_t>(src) & 3u) == 0) {   // 24 packed bytes, dword aligned
        const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(src);
        uint32_t d[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = q[k];
#pragma unroll
        for (int i = 0; i < PPL; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int byte = 3 * i + c;
                px[i][c] = (int)((d[byte >> 2] >> (8 * (byte & 3))) & 0xFFu);
            }
    } else {
#pragma unroll
        for (int i = 0; i < PPL; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i][c] = X0 + i < A.w ? (int)src[(int64_t)i * A.rs[2] + c] : 0;
    }
}

__device__ __forceinline__ bool lane_position(int h, int w, int& Y, int& X0) {
    const int lanes_per_row = (w + PPL - 1) / PPL;
    const long long lane = (long long)blockIdx.x * COLOR_T + threadIdx.x;
    Y = (int)(lane / lanes_per_row);
    X0 = (int)(lane - (long long)Y * lanes_per_row) * PPL;
    return Y < h;
}

__global__ __launch_bounds__(COLOR_T) void color_zero_kernel(unsigned long long* sums, int b) {
    PVNET_SPARE_VGPRS(COLOR_ZERO_SPARE);
    const int i = blockIdx.x * COLOR_T + threadIdx.x;
    if (i < b) sums[i] = 0;
}

__global__ __launch_bounds__(COLOR_T) void color_stats_kernel(ColorArgs A) {
    PVNET_SPARE_VGPRS(COLOR_STATS_SPARE);
    __shared__ unsigned long long sh[COLOR_T / 64];
    const int bi = blockIdx.y;
    int Y, X0;
    unsigned long long sum = 0;
    if (lane_position(A.h, A.w, Y, X0)) {   // (no early return: every thread reaches the barrier)
        const Chain ch = make_chain(A, bi);
        int px[PPL][3];
        load_pixels(A, bi, Y, X0, px);
        for (int j = 0; j < ch.n; ++j) {
            const uint32_t op = (ch.order >> (4 * j)) & 15u;
            if (op == PVNET_COLOR_STEP_C) break;
            run_step(op, ch, 0, px);
        }
#pragma unroll
        for (int i = 0; i < PPL; ++i)
            if (X0 + i < A.w) sum += (unsigned)luma(px[i][0], px[i][1], px[i][2]);
    }
    for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < COLOR_T / 64; ++k) t += sh[k];
        atomicAdd(A.sums + bi, t);
    }
}

__device__ __forceinline__ long long load_mask_at(const void* mask, int mask_dtype, int64_t off) {
    if (mask_dtype == PVNET_MASK_U8) return reinterpret_cast<const uint8_t*>(mask)[off];
    if (mask_dtype == PVNET_MASK_I32) return reinterpret_cast<const int32_t*>(mask)[off];
    return reinterpret_cast<const long long*>(mask)[off];
}

// OUT: PVNET_AUGMENT_OUT_*;  VEC: 16 bytes per store (w % 8 == 0, an aligned image)
template <int OUT, bool VEC>
__global__ __launch_bounds__(COLOR_T) void color_apply_kernel(ColorArgs A) {
    PVNET_SPARE_VGPRS(COLOR_APPLY_SPARE);
    const int bi = blockIdx.y;
    int Y, X0;
    if (!lane_position(A.h, A.w, Y, X0)) return;
    const Chain ch = make_chain(A, bi);
    int px[PPL][3];
    load_pixels(A, bi, Y, X0, px);
    for (int j = 0; j < ch.n; ++j) {
        const uint32_t op = (ch.order >> (4 * j)) & 15u;
        int m = 0;
        if (op == PVNET_COLOR_STEP_C) {
            const unsigned long long n = (unsigned long long)A.h * (unsigned long long)A.w;
            m = (int)((2ull * A.sums[bi] + n) / (2ull * n));
        }
        run_step(op, ch, m, px);
    }
    float o[3][PPL];
#pragma unroll
    for (int i = 0; i < PPL; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c][i] = ((float)px[i][c] / 255.0f - A.mean[c]) / A.std[c];
    if (A.mask && A.maskmul[(size_t)bi * A.maskmul_stride] != 0) {
        const int64_t base = (int64_t)bi * A.ms[0] + (int64_t)Y * A.ms[1] + (int64_t)X0 * A.ms[2];
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
            const float fm = X0 + i < A.w ? (float)load_mask_at(A.mask, A.mask_dtype, base + (int64_t)i * A.ms[2]) : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c][i] = o[c][i] * fm;
        }
    }
    const size_t plane = (size_t)A.h * A.w, row = (size_t)Y * A.w + X0;
    store_planes<OUT, VEC>(A.image, bi, plane, row, X0, A.w, o);
}

__global__ __launch_bounds__(PLAN_T) void color_plan_kernel(PlanArgs A, const double* __restrict__ uniforms, const double* hcoords) {
    PVNET_SPARE_VGPRS(COLOR_PLAN_SPARE);
    __shared__ long long sh[PLAN_SH];
    augment_plan_body(A, uniforms, hcoords, sh);
}

struct WarpU8Args {
    Source S;
    int height, width, mask_out_dtype;
    uint8_t* warped;   // [b,height,width,3]
    void* mask_out;
};

// pvnet_augment's warp up to its rounded pixel: that pixel, 3 bytes, into `warped`, and the mask.  VEC: 8 bytes per store of the
// pixels (24 bytes a lane), the mask's vector stores (width % 8 == 0, aligned outputs)
template <bool VEC>
__global__ __launch_bounds__(WARP_T) void color_warp_kernel(WarpU8Args A, const Plan* __restrict__ plans) {
    PVNET_SPARE_VGPRS(COLOR_WARP_SPARE);
    const Source& S = A.S;
    const int bi = blockIdx.y, width = A.width, height = A.height;
    const int lanes_per_row = (width + PPL - 1) / PPL;
    const long long lane = (long long)blockIdx.x * WARP_T + threadIdx.x;
    const int Y = (int)(lane / lanes_per_row);
    if (Y >= height) return;
    const int X0 = (int)(lane - (long long)Y * lanes_per_row) * PPL;
    const Plan P = plans[bi];
    const uint8_t* __restrict__ img = S.rgb + (int64_t)bi * S.rs[0];
    const uint32_t key = pvnet_rng_key(S.seed, PVNET_TAG_AUG, (uint32_t)bi);
    uint32_t d[6] = {0u, 0u, 0u, 0u, 0u, 0u};
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
            const int byte = 3 * i + c;
            d[byte >> 2] |= ((uint32_t)(int)val[c] & 0xFFu) << (8 * (byte & 3));
        }
    }
    const size_t plane = (size_t)height * width, row = (size_t)Y * width + X0;
    uint8_t* dst = A.warped + ((size_t)bi * plane + row) * 3;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x2 q = {d[2 * k], d[2 * k + 1]};
            *reinterpret_cast<u32x2*>(dst + 8 * k) = q;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PPL; ++i)
            if (X0 + i < width)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int byte = 3 * i + c;
                    dst[byte] = (uint8_t)(d[byte >> 2] >> (8 * (byte & 3)));
                }
    }
    store_mask<VEC>(A.mask_out, A.mask_out_dtype, bi, plane, row, X0, width, mo);
}

inline size_t align16(size_t n) { return (n + 15u) & ~(size_t)15u; }

bool range_ok(double x, double hi) { return x >= 0.0 && x <= hi; }   // (false for a NaN)

int check_color_config(const PvnetColorConfig* cfg) {
    if (!range_ok(cfg->brightness, MAX_RANGE) || !range_ok(cfg->contrast, MAX_RANGE) || !range_ok(cfg->saturation, MAX_RANGE) ||
        !range_ok(cfg->hue, 0.5))
        return PVNET_E_BADARG;
    return 0;
}

// the zeroing of S_L, the statistics kernel (both only where C is present) and the apply kernel
int launch_jitter(const ColorArgs& A, int b, int image_dtype, hipStream_t s) {
    const long long lanes = (long long)((A.w + PPL - 1) / PPL) * A.h;
    const dim3 grid((unsigned)((lanes + COLOR_T - 1) / COLOR_T), (unsigned)b), block(COLOR_T);
    if (A.contrast != 0.0) {
        hipLaunchKernelGGL(color_zero_kernel, dim3((unsigned)((b + COLOR_T - 1) / COLOR_T)), block, 0, s, A.sums, b);
        hipLaunchKernelGGL(color_stats_kernel, grid, block, 0, s, A);
    }
    const bool vec = A.w % PPL == 0 && aligned16(A.image);
#define COLOR_LAUNCH(OUT)                                                                   \
    do {                                                                                    \
        if (vec) hipLaunchKernelGGL((color_apply_kernel<OUT, true>), grid, block, 0, s, A);  \
        else hipLaunchKernelGGL((color_apply_kernel<OUT, false>), grid, block, 0, s, A);     \
    } while (0)
    if (image_dtype == PVNET_AUGMENT_OUT_F32) COLOR_LAUNCH(PVNET_AUGMENT_OUT_F32);
    else if (image_dtype == PVNET_AUGMENT_OUT_BF16) COLOR_LAUNCH(PVNET_AUGMENT_OUT_BF16);
    else COLOR_LAUNCH(PVNET_AUGMENT_OUT_F16);
#undef COLOR_LAUNCH
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

void set_config(ColorArgs& A, const PvnetColorConfig* cfg, const float* mean, const float* std) {
    A.brightness = cfg->brightness, A.contrast = cfg->contrast, A.saturation = cfg->saturation, A.hue = cfg->hue;
    for (int c = 0; c < 3; ++c) A.mean[c] = mean[c], A.std[c] = std[c];
}

}  // namespace

extern "C" {

int pvnet_color_abi_version(void) { return PVNET_COLOR_ABI_VERSION; }

size_t pvnet_color_workspace_bytes(int b, int height, int width) {
    if (b <= 0 || b > MAX_B || height < 0 || width < 0 || height > MAX_SIDE || width > MAX_SIDE || (long long)height * width > MAX_PIXELS) return 0;
    const size_t sums = align16((size_t)b * sizeof(unsigned long long));
    if (height == 0 && width == 0) return sums;
    if (height == 0 || width == 0) return 0;
    return sums + (size_t)b * sizeof(Plan) + (size_t)b * height * width * 3;
}

int pvnet_color_jitter(const uint8_t* rgb, const int64_t rgb_strides[3], const double* uniforms, int b, int h, int w,
                       const PvnetColorConfig* cfg, const void* mask, int mask_dtype, const int64_t mask_strides[3], const int32_t* maskmul,
                       void* image, int image_dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!uniforms || !cfg) return PVNET_E_BADARG;
    if (const int rc = check_source(rgb, rgb_strides, b, h, w)) return rc;
    if (const int rc = check_image(image, image_dtype)) return rc;
    if (const int rc = check_color_config(cfg)) return rc;
    if (!config_ok(cfg->mean, cfg->std)) return PVNET_E_BADARG;
    if ((mask != nullptr) != (maskmul != nullptr) || (mask && !mask_strides)) return PVNET_E_BADARG;
    if (mask) {
        if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
        if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    }
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_color_workspace_bytes(b, 0, 0)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    ColorArgs A;
    A.rgb = rgb;
    for (int i = 0; i < 3; ++i) A.rs[i] = rgb_strides[i], A.ms[i] = mask ? mask_strides[i] : 0;
    A.mask = mask;
    A.mask_dtype = mask_dtype;
    A.maskmul = maskmul;
    A.maskmul_stride = 1;
    A.uniforms = uniforms;
    set_config(A, cfg, cfg->mean, cfg->std);
    A.h = h;
    A.w = w;
    A.sums = static_cast<unsigned long long*>(workspace);
    A.image = image;
    return launch_jitter(A, b, image_dtype, static_cast<hipStream_t>(stream));
}

int pvnet_augment_jitter(const uint8_t* rgb, const int64_t rgb_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3],
                         const double* hcoords, const double* uniforms, int b, int h, int w, int vn, int height, int width,
                         const PvnetAugmentConfig* cfg, uint64_t seed, const PvnetColorConfig* jitter, const double* jitter_uniforms,
                         void* image, int image_dtype, void* mask_out, int mask_out_dtype, double* hcoords_out, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!jitter || !jitter_uniforms) return PVNET_E_BADARG;
    if (const int rc = check_augment(rgb, rgb_strides, mask, mask_dtype, mask_strides, hcoords, uniforms, b, h, w, vn, height, width, cfg, image,
                                     image_dtype, mask_out, mask_out_dtype, hcoords_out, status))
        return rc;
    if (const int rc = check_color_config(jitter)) return rc;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_color_workspace_bytes(b, height, width)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return PVNET_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const size_t sums_bytes = align16((size_t)b * sizeof(unsigned long long));
    Plan* plans = reinterpret_cast<Plan*>(ws + sums_bytes);
    uint8_t* warped = ws + sums_bytes + (size_t)b * sizeof(Plan);
    PlanArgs PA;
    PA.S = make_source(rgb, rgb_strides, mask, mask_dtype, mask_strides, h, w, seed);
    PA.cfg = *cfg;
    PA.vn = vn;
    PA.height = height;
    PA.width = width;
    PA.hc_out = hcoords_out;
    PA.status = status;
    PA.plans = plans;
    hipLaunchKernelGGL(color_plan_kernel, dim3((unsigned)b), dim3(PLAN_T), 0, s, PA, uniforms, hcoords);
    WarpU8Args WA;
    WA.S = PA.S;
    WA.height = height;
    WA.width = width;
    WA.mask_out_dtype = mask_out_dtype;
    WA.warped = warped;
    WA.mask_out = mask_out;
    {
        const bool vec = width % PPL == 0 && aligned16(mask_out);   // (`warped` is 16-byte aligned, its rows multiples of 24 bytes then)
        const long long lanes = (long long)((width + PPL - 1) / PPL) * height;
        const dim3 grid((unsigned)((lanes + WARP_T - 1) / WARP_T), (unsigned)b), block(WARP_T);
        if (vec) hipLaunchKernelGGL((color_warp_kernel<true>), grid, block, 0, s, WA, plans);
        else hipLaunchKernelGGL((color_warp_kernel<false>), grid, block, 0, s, WA, plans);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    ColorArgs A;
    A.rgb = warped;
    A.rs[0] = (int64_t)height * width * 3, A.rs[1] = (int64_t)width * 3, A.rs[2] = 3;
    A.mask = mask_out;
    A.ms[0] = (int64_t)height * width, A.ms[1] = width, A.ms[2] = 1;
    A.mask_dtype = mask_out_dtype;
    A.maskmul = &plans[0].maskmul;
    A.maskmul_stride = (int)(sizeof(Plan) / sizeof(int32_t));
    A.uniforms = jitter_uniforms;
    set_config(A, jitter, cfg->mean, cfg->std);
    A.h = height;
    A.w = width;
    A.sums = reinterpret_cast<unsigned long long*>(ws);
    A.image = image;
    return launch_jitter(A, b, image_dtype, s);
}

}  // extern "C"
