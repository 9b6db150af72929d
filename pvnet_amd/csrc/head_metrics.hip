// head_metrics.hip -- the network-head metrics of a validation step, on the device: per-image cross-entropy of the class logits,
// weighted smooth-L1 loss of the vector field, segmentation precision and recall, for a batch in one call.  The whole of
// libpvnet_head.so; C ABI: pvnet_head_metrics in include/pvnet_head.h.
//
// Restates what the reference's NetWrapper.forward computes after the backbone (tools/train_linemod.py:85-91 with
// lib/utils/net_utils.py:54-79 and :329-348), term for term in float64 on the inputs as stored.  Its oracle is the float64
// restatement of tests/test_head_metrics_device.py and the reference's own recorded outputs (tests/golden/head_metrics.npz).
//
//   head_partial_kernel   grid (segments of 1 024 pixels, images).  A workgroup streams its run of pixels through every plane -- the
//     (fast path)         class logits, the 2 vn predicted and 2 vn target planes, the weights, the mask -- eight consecutive pixels
//                         per lane, 16 bytes per load wherever the element is 2 bytes or wider: 164 bytes per pixel with float32
//                         predictions and int64 masks, each read once.  The planes must be contiguous in the pixels and 16-byte
//                         aligned, h * w a multiple of 8 (what a backbone and a dataset deliver).  The targets, the weights and
//                         the mask are loaded non-temporally -- nobody reads them again --, the predictions plainly: the vote reads
//                         them next (profiles/head_metrics_probe.txt holds the A/B).
//   head_partial_general_kernel   the same record from any element strides, any alignment, any h * w: a pixel per lane and load
//                         (mirrors the mask_linear split of k1_mask.hip).
//   head_final_kernel     a workgroup per image: sums the image's records in a fixed order, finalises, writes the outputs.
//
// No atomics; every sum has a fixed order (lane-sequential, then an xor butterfly over the wave, then the waves in order), so two
// calls on the same inputs agree bit for bit.  float64 throughout: at 164 bytes per pixel the float64 vector rate is far above
// what the memory system can feed, the kernel is bound by HBM reads.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "pvnet_head.h"
#include "vote_common.h"   // ld_elem / ld_elem_rt (VT_*), PVNET_SPARE_VGPRS

// no contraction: the sums round as the float64 restatement's separate multiplies and adds do
#pragma clang fp contract(off)

namespace {

using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;

constexpr int HM_T = 128;                // lanes of a pass-1 workgroup
constexpr int HM_PPL = 8;                // consecutive pixels per lane (fast path)
constexpr int HM_SEG = HM_T * HM_PPL;    // pixels per workgroup = per partial record
constexpr int HM_FT = 256;               // lanes of the final workgroup
constexpr int HM_MAX_B = 65535;
constexpr int HM_MAX_PIXELS = 1 << 30;
// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define HM_FAST_SPARE 119
#define HM_GENERAL_SPARE 87
#define HM_FINAL_SPARE 71

enum { NT_NONE = 0, NT_TARGETS = 1, NT_ALL = 2 };

struct HeadPartial {   // 32 bytes
    double ce, sl1, wsum;
    unsigned long long packed;   // tp | fp << 16 | fn << 32 | bad << 48: each at most HM_SEG
};
static_assert(sizeof(HeadPartial) == 32 && HM_SEG < (1 << 16), "a record's four counts share one 64-bit word");

struct HeadArgs {
    const void* seg;
    const void* vp;
    const float* vt;
    const float* vw;
    const void* mask;
    int64_t ss[4], vs[4], ts[4], ws[3], ms[3];
    int seg_type, vp_type, mask_dtype, num_classes, planes;
    int h, w, npix, nseg;
    double hs, inv, half;   // sigma^2 / 2, 1 / sigma^2, 0.5 / sigma^2
    double* losses;
    int64_t* counts;
    int32_t* status;
    HeadPartial* partial;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <bool NT, typename V>
__device__ __forceinline__ V ldv(const void* p) {
    return NT ? __builtin_nontemporal_load(reinterpret_cast<const V*>(p)) : *reinterpret_cast<const V*>(p);
}

// eight consecutive elements at element offset `off` (a multiple of 8 from a 16-byte aligned base), widened to float32
template <int VT, bool NT>
__device__ __forceinline__ void load8(const void* base, int64_t off, float* o) {
    if (VT == VT_F32) {
        const float* p = reinterpret_cast<const float*>(base) + off;
        const f32x4 a = ldv<NT, f32x4>(p), b = ldv<NT, f32x4>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = a[i];
            o[4 + i] = b[i];
        }
    } else if (VT == VT_F16) {
        const f16x8 a = ldv<NT, f16x8>(reinterpret_cast<const _Float16*>(base) + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (float)a[i];
    } else {
        const u32x4 a = ldv<NT, u32x4>(reinterpret_cast<const uint16_t*>(base) + off);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[2 * i] = __uint_as_float(a[i] << 16);
            o[2 * i + 1] = __uint_as_float(a[i] & 0xFFFF0000u);
        }
    }
}
template <bool NT>
__device__ __forceinline__ void load8_rt(int vt, const void* base, int64_t off, float* o) {   // workgroup-uniform type
    if (vt == VT_F16) load8<VT_F16, NT>(base, off, o);
    else if (vt == VT_BF16) load8<VT_BF16, NT>(base, off, o);
    else load8<VT_F32, NT>(base, off, o);
}

// a label as the kernels use it: 0 .. C-1, or -1 for a value outside (which is still "not background")
__device__ __forceinline__ int label_of(long long v, int C) { return (v < 0 || v >= C) ? -1 : (int)v; }

template <bool NT>
__device__ __forceinline__ void load8_labels(int dt, const void* base, int64_t off, int C, int* lab) {
    if (dt == PVNET_MASK_U8) {
        const u32x2 a = ldv<NT, u32x2>(reinterpret_cast<const uint8_t*>(base) + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) lab[i] = label_of((a[i >> 2] >> (8 * (i & 3))) & 0xFFu, C);
    } else if (dt == PVNET_MASK_I32) {
        const int32_t* p = reinterpret_cast<const int32_t*>(base) + off;
        const u32x4 a = ldv<NT, u32x4>(p), b = ldv<NT, u32x4>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lab[i] = label_of((int32_t)a[i], C);
            lab[4 + i] = label_of((int32_t)b[i], C);
        }
    } else {
        const long long* p = reinterpret_cast<const long long*>(base) + off;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const i64x2 a = ldv<NT, i64x2>(p + 2 * i);
            lab[2 * i] = label_of(a.x, C);
            lab[2 * i + 1] = label_of(a.y, C);
        }
    }
}

__device__ __forceinline__ long long load_label_rt(int dt, const void* base, int64_t off) {
    if (dt == PVNET_MASK_U8) return reinterpret_cast<const uint8_t*>(base)[off];
    if (dt == PVNET_MASK_I32) return reinterpret_cast<const int32_t*>(base)[off];
    return reinterpret_cast<const long long*>(base)[off];
}

// torch.argmax's rule (k1_mask.hip:69-80): the first maximum wins and a NaN counts as the maximum -- a NaN replaces a number, a
// later NaN never an earlier one
__device__ __forceinline__ bool takes_over(float best, float x) { return (best == best) & !(x <= best); }

// one smooth-L1 term (net_utils.py:66-71): d = w (p - t); d^2 sigma^2 / 2 where |d| < 1 / sigma^2, else |d| - 0.5 / sigma^2.  A NaN
// fails the comparison, takes the second branch and stays NaN.
__device__ __forceinline__ double smooth_l1(const HeadArgs& A, double w, float p, float t) {
    const double d = w * ((double)p - (double)t);
    const double a = fabs(d);
    return a < A.inv ? d * d * A.hs : a - A.half;
}

// log(sum_c exp(s_c - m)) - (s_label - m): the cross-entropy of one pixel with the maximum m subtracted first, as log_softmax does
__device__ __forceinline__ double cross_entropy(double sum, float s_label, float m) {
    return log(sum) - ((double)s_label - (double)m);
}

struct Acc {
    double ce = 0.0, sl1 = 0.0, wsum = 0.0;
    unsigned long long packed = 0;
};
constexpr unsigned long long ONE_TP = 1ull, ONE_FP = 1ull << 16, ONE_FN = 1ull << 32, ONE_BAD = 1ull << 48;

__device__ __forceinline__ unsigned long long confusion(bool pred_fg, int lab) {
    const bool fg = lab != 0;
    return (pred_fg && fg ? ONE_TP : 0) | (pred_fg && !fg ? ONE_FP : 0) | (!pred_fg && fg ? ONE_FN : 0) | (lab < 0 ? ONE_BAD : 0);
}

__device__ __forceinline__ double wave_sum(double v) {   // xor butterfly: every lane ends with the same, order-fixed sum
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// the workgroup's record: waves reduced by butterfly, then added in wave order by lane 0
template <int T>
__device__ __forceinline__ bool block_reduce(Acc& a) {
    constexpr int NW = T / 64;
    __shared__ double s_d[NW][3];
    __shared__ unsigned long long s_p[NW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double ce = wave_sum(a.ce), sl1 = wave_sum(a.sl1), wsum = wave_sum(a.wsum);
    const unsigned long long packed = wave_sum(a.packed);
    if (lane == 0) {
        s_d[wave][0] = ce;
        s_d[wave][1] = sl1;
        s_d[wave][2] = wsum;
        s_p[wave] = packed;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    a.ce = s_d[0][0];
    a.sl1 = s_d[0][1];
    a.wsum = s_d[0][2];
    a.packed = s_p[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) {
        a.ce = a.ce + s_d[i][0];
        a.sl1 = a.sl1 + s_d[i][1];
        a.wsum = a.wsum + s_d[i][2];
        a.packed = a.packed + s_p[i];
    }
    return true;
}

__device__ __forceinline__ void store_partial(const HeadArgs& A, const Acc& a) {
    HeadPartial* r = A.partial + (size_t)blockIdx.y * A.nseg + blockIdx.x;
    r->ce = a.ce;
    r->sl1 = a.sl1;
    r->wsum = a.wsum;
    r->packed = a.packed;
}

template <int VT, int NT>
__global__ __launch_bounds__(HM_T) void head_partial_kernel(HeadArgs A) {
    PVNET_SPARE_VGPRS(HM_FAST_SPARE);
    constexpr bool NT_P = NT == NT_ALL, NT_T = NT != NT_NONE;   // predictions, targets / weights / mask
    const int bi = blockIdx.y;
    const int p0 = blockIdx.x * HM_SEG + (int)threadIdx.x * HM_PPL;
    Acc acc;
    if (p0 < A.npix) {   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
        int lab[HM_PPL];
        load8_labels<NT_T>(A.mask_dtype, A.mask, (int64_t)bi * A.ms[0] + p0, A.num_classes, lab);
        // ---- class logits: maximum and arg-max in one pass, then sum exp(s - max) in a second (the planes are in cache) -------------
        const int64_t soff = (int64_t)bi * A.ss[0] + p0;
        float best[HM_PPL], sl[HM_PPL], s[HM_PPL];
        bool pfg[HM_PPL];
        load8_rt<NT_P>(A.seg_type, A.seg, soff, best);
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) {
            pfg[i] = false;
            sl[i] = best[i];   // label 0, or a bad label (not used then)
        }
        for (int c = 1; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HM_PPL; ++i) {
                const bool take = takes_over(best[i], s[i]);
                best[i] = take ? s[i] : best[i];
                pfg[i] = take ? true : pfg[i];
                sl[i] = lab[i] == c ? s[i] : sl[i];
            }
        }
        double sum[HM_PPL];
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) sum[i] = 0.0;
        for (int c = 0; c < A.num_classes; ++c) {
            load8_rt<NT_P>(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1], s);
#pragma unroll
            for (int i = 0; i < HM_PPL; ++i) sum[i] = sum[i] + exp((double)s[i] - (double)best[i]);
        }
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) {
            if (lab[i] >= 0) acc.ce = acc.ce + cross_entropy(sum[i], sl[i], best[i]);
            acc.packed += confusion(pfg[i], lab[i]);
        }
        // ---- the field: 2 vn planes of prediction and target under one plane of weights ---------------------------------------------
        float wf[HM_PPL];
        double wd[HM_PPL];
        load8<VT_F32, NT_T>(A.vw, (int64_t)bi * A.ws[0] + p0, wf);
#pragma unroll
        for (int i = 0; i < HM_PPL; ++i) {
            wd[i] = (double)wf[i];
            acc.wsum = acc.wsum + wd[i];
        }
        const int64_t poff = (int64_t)bi * A.vs[0] + p0, toff = (int64_t)bi * A.ts[0] + p0;
#pragma unroll 2
        for (int k = 0; k < A.planes; ++k) {
            float p[HM_PPL], t[HM_PPL];
            load8<VT, NT_P>(A.vp, poff + (int64_t)k * A.vs[1], p);
            load8<VT_F32, NT_T>(A.vt, toff + (int64_t)k * A.ts[1], t);
#pragma unroll
            for (int i = 0; i < HM_PPL; ++i) acc.sl1 = acc.sl1 + smooth_l1(A, wd[i], p[i], t[i]);
        }
    }
    if (block_reduce<HM_T>(acc)) store_partial(A, acc);
}

__global__ __launch_bounds__(HM_T) void head_partial_general_kernel(HeadArgs A) {
    PVNET_SPARE_VGPRS(HM_GENERAL_SPARE);
    const int bi = blockIdx.y;
    Acc acc;
    for (int j = 0; j < HM_PPL; ++j) {
        const int p = blockIdx.x * HM_SEG + j * HM_T + (int)threadIdx.x;
        if (p >= A.npix) break;
        const int y = p / A.w, x = p - y * A.w;
        const int lab = label_of(load_label_rt(A.mask_dtype, A.mask, (int64_t)bi * A.ms[0] + (int64_t)y * A.ms[1] + (int64_t)x * A.ms[2]),
                                 A.num_classes);
        const int64_t soff = (int64_t)bi * A.ss[0] + (int64_t)y * A.ss[2] + (int64_t)x * A.ss[3];
        float best = pvd::ld_elem_rt(A.seg_type, A.seg, soff);
        float sl = best;
        bool pfg = false;
        for (int c = 1; c < A.num_classes; ++c) {
            const float s = pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]);
            const bool take = takes_over(best, s);
            best = take ? s : best;
            pfg = take ? true : pfg;
            sl = lab == c ? s : sl;
        }
        double sum = 0.0;
        for (int c = 0; c < A.num_classes; ++c)
            sum = sum + exp((double)pvd::ld_elem_rt(A.seg_type, A.seg, soff + (int64_t)c * A.ss[1]) - (double)best);
        if (lab >= 0) acc.ce = acc.ce + cross_entropy(sum, sl, best);
        acc.packed += confusion(pfg, lab);
        const double wd = (double)A.vw[(int64_t)bi * A.ws[0] + (int64_t)y * A.ws[1] + (int64_t)x * A.ws[2]];
        acc.wsum = acc.wsum + wd;
        const int64_t poff = (int64_t)bi * A.vs[0] + (int64_t)y * A.vs[2] + (int64_t)x * A.vs[3];
        const int64_t toff = (int64_t)bi * A.ts[0] + (int64_t)y * A.ts[2] + (int64_t)x * A.ts[3];
        for (int k = 0; k < A.planes; ++k)
            acc.sl1 = acc.sl1 + smooth_l1(A, wd, pvd::ld_elem_rt(A.vp_type, A.vp, poff + (int64_t)k * A.vs[1]),
                                          A.vt[toff + (int64_t)k * A.ts[1]]);
    }
    if (block_reduce<HM_T>(acc)) store_partial(A, acc);
}

__global__ __launch_bounds__(HM_FT) void head_final_kernel(HeadArgs A) {
    PVNET_SPARE_VGPRS(HM_FINAL_SPARE);
    const int bi = blockIdx.x;
    Acc acc;
    long long tp = 0, fp = 0, fn = 0, bad = 0;   // a record's packed counts are unpacked before they are added: no field overflows
    const HeadPartial* rec = A.partial + (size_t)bi * A.nseg;
    for (int k = threadIdx.x; k < A.nseg; k += HM_FT) {   // lane t: records t, t + 256, ... in order
        acc.ce = acc.ce + rec[k].ce;
        acc.sl1 = acc.sl1 + rec[k].sl1;
        acc.wsum = acc.wsum + rec[k].wsum;
        const unsigned long long q = rec[k].packed;
        tp += (long long)(q & 0xFFFFu);
        fp += (long long)((q >> 16) & 0xFFFFu);
        fn += (long long)((q >> 32) & 0xFFFFu);
        bad += (long long)(q >> 48);
    }
    __shared__ long long s_cnt[HM_FT / 64][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    tp = (long long)wave_sum((unsigned long long)tp);
    fp = (long long)wave_sum((unsigned long long)fp);
    fn = (long long)wave_sum((unsigned long long)fn);
    bad = (long long)wave_sum((unsigned long long)bad);
    if (lane == 0) {
        s_cnt[wave][0] = tp;
        s_cnt[wave][1] = fp;
        s_cnt[wave][2] = fn;
        s_cnt[wave][3] = bad;
    }
    if (!block_reduce<HM_FT>(acc)) return;   // (its barrier also orders s_cnt)
    tp = fp = fn = bad = 0;
#pragma unroll
    for (int i = 0; i < HM_FT / 64; ++i) {
        tp += s_cnt[i][0];
        fp += s_cnt[i][1];
        fn += s_cnt[i][2];
        bad += s_cnt[i][3];
    }
    double* out = A.losses + (size_t)bi * 4;
    out[0] = bad ? __builtin_nan("") : acc.ce / (double)A.npix;
    out[1] = acc.sl1 / ((double)A.planes * acc.wsum + 1e-3);   // net_utils.py:74
    out[2] = ((double)tp + 1.0) / ((double)tp + (double)fp + 1.0);
    out[3] = ((double)tp + 1.0) / ((double)tp + (double)fn + 1.0);
    int64_t* cnt = A.counts + (size_t)bi * 3;
    cnt[0] = tp;
    cnt[1] = fp;
    cnt[2] = fn;
    if (A.status) A.status[bi] = bad ? PVNET_HEAD_S_BAD_LABEL : 0;
}

// a tensor's planes can be read eight pixels at a time: pixels contiguous, base and every plane / image start on 16 bytes
bool plane_linear(const void* base, int b, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int w) {
    return sw == 1 && sh == w && (b == 1 || sb % 8 == 0) && sc % 8 == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
}

int type_of(uint32_t flags, uint32_t f16, uint32_t bf16) { return (flags & f16) ? VT_F16 : (flags & bf16) ? VT_BF16 : VT_F32; }

template <int VT>
void launch_fast(int nt, dim3 grid, hipStream_t s, const HeadArgs& A) {
    if (nt == NT_NONE) hipLaunchKernelGGL((head_partial_kernel<VT, NT_NONE>), grid, dim3(HM_T), 0, s, A);
    else if (nt == NT_ALL) hipLaunchKernelGGL((head_partial_kernel<VT, NT_ALL>), grid, dim3(HM_T), 0, s, A);
    else hipLaunchKernelGGL((head_partial_kernel<VT, NT_TARGETS>), grid, dim3(HM_T), 0, s, A);
}

}  // namespace

extern "C" {

int pvnet_head_abi_version(void) { return PVNET_HEAD_ABI_VERSION; }

size_t pvnet_head_metrics_workspace_bytes(int b, int h, int w) {
    if (b <= 0 || h <= 0 || w <= 0 || b > HM_MAX_B || (long long)h * w > HM_MAX_PIXELS) return 0;
    const size_t nseg = ((size_t)h * w + HM_SEG - 1) / HM_SEG;
    return ((size_t)b * nseg * sizeof(HeadPartial) + 255) / 256 * 256;
}

int pvnet_head_metrics(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4],
                       const float* vertex_weights, const int64_t w_strides[3], const void* mask, int mask_dtype,
                       const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags, double* losses,
                       int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    constexpr uint32_t KNOWN = PVNET_HEAD_F_VERTEX_F16 | PVNET_HEAD_F_VERTEX_BF16 | PVNET_HEAD_F_LOGITS_F16 | PVNET_HEAD_F_LOGITS_BF16 |
                               PVNET_HEAD_F_NT_NONE | PVNET_HEAD_F_NT_ALL;
    if (!seg_pred || !seg_strides || !vertex_pred || !vp_strides || !vertex_target || !vt_strides || !vertex_weights || !w_strides ||
        !mask || !mask_strides || !losses || !counts)
        return PVNET_E_BADARG;
    if (b < 0 || h <= 0 || w <= 0 || vn <= 0 || num_classes < 2 || !(sigma > 0.0) || !isfinite(sigma) || (flags & ~KNOWN) != 0)
        return PVNET_E_BADARG;
    if (((flags & PVNET_HEAD_F_VERTEX_F16) && (flags & PVNET_HEAD_F_VERTEX_BF16)) ||
        ((flags & PVNET_HEAD_F_LOGITS_F16) && (flags & PVNET_HEAD_F_LOGITS_BF16)) ||
        ((flags & PVNET_HEAD_F_NT_NONE) && (flags & PVNET_HEAD_F_NT_ALL)))
        return PVNET_E_BADARG;
    if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
    if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (b > HM_MAX_B || (long long)h * w > HM_MAX_PIXELS || vn > (1 << 20)) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_head_metrics_workspace_bytes(b, h, w)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    HeadArgs A;
    A.seg = seg_pred;
    A.vp = vertex_pred;
    A.vt = vertex_target;
    A.vw = vertex_weights;
    A.mask = mask;
    for (int i = 0; i < 4; ++i) {
        A.ss[i] = seg_strides[i];
        A.vs[i] = vp_strides[i];
        A.ts[i] = vt_strides[i];
    }
    for (int i = 0; i < 3; ++i) {
        A.ws[i] = w_strides[i];
        A.ms[i] = mask_strides[i];
    }
    A.seg_type = type_of(flags, PVNET_HEAD_F_LOGITS_F16, PVNET_HEAD_F_LOGITS_BF16);
    A.vp_type = type_of(flags, PVNET_HEAD_F_VERTEX_F16, PVNET_HEAD_F_VERTEX_BF16);
    A.mask_dtype = mask_dtype;
    A.num_classes = num_classes;
    A.planes = 2 * vn;
    A.h = h;
    A.w = w;
    A.npix = h * w;
    A.nseg = (A.npix + HM_SEG - 1) / HM_SEG;
    const double s2 = sigma * sigma;
    A.hs = s2 / 2.0;
    A.inv = 1.0 / s2;
    A.half = 0.5 / s2;
    A.losses = losses;
    A.counts = counts;
    A.status = status;
    A.partial = static_cast<HeadPartial*>(workspace);
    const bool fast = A.npix % HM_PPL == 0 && plane_linear(seg_pred, b, A.ss[0], A.ss[1], A.ss[2], A.ss[3], w) &&
                      plane_linear(vertex_pred, b, A.vs[0], A.vs[1], A.vs[2], A.vs[3], w) &&
                      plane_linear(vertex_target, b, A.ts[0], A.ts[1], A.ts[2], A.ts[3], w) &&
                      plane_linear(vertex_weights, b, A.ws[0], 0, A.ws[1], A.ws[2], w) &&
                      plane_linear(mask, b, A.ms[0], 0, A.ms[1], A.ms[2], w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (fast) {
        const int nt = (flags & PVNET_HEAD_F_NT_NONE) ? NT_NONE : (flags & PVNET_HEAD_F_NT_ALL) ? NT_ALL : NT_TARGETS;
        if (A.vp_type == VT_F16) launch_fast<VT_F16>(nt, grid, s, A);
        else if (A.vp_type == VT_BF16) launch_fast<VT_BF16>(nt, grid, s, A);
        else launch_fast<VT_F32>(nt, grid, s, A);
    } else {
        hipLaunchKernelGGL(head_partial_general_kernel, grid, dim3(HM_T), 0, s, A);
    }
    hipLaunchKernelGGL(head_final_kernel, dim3((unsigned)b), dim3(HM_FT), 0, s, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"
