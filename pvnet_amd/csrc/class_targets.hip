// class_targets.hip -- the training targets of the vector field for images of several objects, made on the device from a label image
// and one set of key-points per class, and the network head's forward and backward fused with them.  The whole of
// libpvnet_class_targets.so; C ABI: include/pvnet_class_targets.h (the definition is stated there).
//
// This file holds the third target source of head_common.h's per-pixel bodies, ClassKpSource -- KpSource of head_targets.hip with
// the key-points picked by the pixel's label --, the one kernel that writes the targets out, and the head's kernels instantiated on
// that source.  It holds none of the head's arithmetic (the bodies are head_common.h's, the same source text the three other head
// libraries instantiate) and none of the target's: kp_target is kp_target.h's, the one copy head_targets.hip compiles too.
//
//   vertex_targets_classes_kernel<FAST>  grid (segments of 1 024 pixels, images).  Reads the labels, writes the 2 vn target planes and
//                                        the weights.  Fast path: eight consecutive pixels per lane, 16 bytes per store; else a pixel
//                                        per lane and store, any strides.
//   head_partial_ckp_kernel<VT, NT>      the forward (head_partial8 / head_partial1 / head_final_image).  Same grid, segments, records
//   head_partial_ckp_general_kernel      and summation order as on loaded targets.
//   head_final_ckp_kernel
//   head_grad_ckp_wsum_kernel<FAST>      the backward (head_grad_wsum / head_grad_final_image / head_grad8 / head_grad1 /
//   head_grad_ckp_final_kernel           head_grad_status_image).  The labels are read whichever half is asked for.
//   head_grad_ckp_kernel<VT, NT>
//   head_grad_ckp_general_kernel
//   head_grad_ckp_status_kernel
//
// The key-points are no longer wave-uniform: they depend on the lane's labels, so SGPRs cannot hold them as in head_targets.hip.  Each
// workgroup stages its image's table in LDS once -- nk weights (float32, 1.0f without a scale) and nk * vn * 3 doubles, from the
// kernel's own noalias argument -- behind one barrier, then per lane of eight pixels:
//   no pixel with a label 1 .. nk          no float64 work, as in head_targets.hip; a wave of such lanes branches over it
//   all such pixels of ONE class           the common case inside an object: the key-point's three doubles are read once per
//                                          key-point, and lanes of the same class read the same address (a broadcast)
//   mixed                                  read per pixel
// The LDS is dynamic, sized by the call's table (256 + nk * vn * 24 bytes: 2.6 KiB for 13 classes of 9 key-points), so the occupancy
// is the registers' to decide.  The predictions are still read at every pixel.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "head_common.h"
#include "kp_target.h"
#include "pvnet_class_targets.h"
#include "pvnet_classes.h"

static_assert(PVNET_CLASS_TARGETS_MAX_CLASSES == PVNET_CLASSES_MAX, "one limit of the class count for the vote and the targets");

// no contraction (kp_target.h and head_common.h say why)
#pragma clang fp contract(off)

namespace {

using namespace pvh;

// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define CKP_TARGETS_FAST_SPARE 103    // four waves per SIMD where vertex_targets_kernel has five: the packed classes and both loops
#define CKP_TARGETS_GENERAL_SPARE 39
#define CKP_HEAD_FAST_SPARE 127       // float32 predictions: four waves per SIMD, as head_partial_kp_kernel
#define CKP_HEAD_FAST16_SPARE 135     // float16 / bfloat16: as head_partial_kp_kernel's
#define CKP_HEAD_GENERAL_SPARE 95
#define CKP_HEAD_FINAL_SPARE 71
#define CKP_GRAD_FAST_SPARE 143       // three waves per SIMD, as head_grad_kp_kernel
#define CKP_GRAD_GENERAL_SPARE 87
#define CKP_GRAD_WSUM_SPARE 39
#define CKP_GRAD_FINAL_SPARE 31
#define CKP_GRAD_STATUS_SPARE 23

constexpr int CK_WEIGHT_SLOTS = 64;                  // floats in front of the table: nk <= 63 weights, and the doubles stay aligned
constexpr int CK_POINTS_AT = CK_WEIGHT_SLOTS / 2;    // where the key-points start, in doubles
static_assert(PVNET_CLASS_TARGETS_MAX_CLASSES - 1 <= CK_WEIGHT_SLOTS && PVNET_CLASS_TARGETS_MAX_CLASSES - 1 <= HC_T,
              "a workgroup's first lanes stage a weight each");

// the workgroup's table: [CK_WEIGHT_SLOTS] float32 weights, then [nk][vn][3] float64 key-points (dynamic LDS, sized by the host)
__device__ __forceinline__ double* ck_lds() {
    extern __shared__ double ck_table[];
    return ck_table;
}

// ---- the class key-point source: where the labels are, and the target source made of them (the interface is stated at MemSource) --
struct ClassKpSource {
    const void* mask;
    const float* __restrict__ wscale;   // NULL or [b][nk]
    int64_t ms[3];
    int mask_dtype, vn, nk, motion;
    int w, npix, nseg;

    __device__ __forceinline__ const float* weights() const { return reinterpret_cast<const float*>(ck_lds()); }
    __device__ __forceinline__ const double* points() const { return ck_lds() + CK_POINTS_AT; }

    // a workgroup of HC_T lanes stages its image's table; hcoords NULL: the weights alone (the kernels that make no target)
    __device__ __forceinline__ void stage(const double* __restrict__ hcoords) const {
        const int bi = blockIdx.y, t = threadIdx.x;
        if (t < nk) reinterpret_cast<float*>(ck_lds())[t] = wscale ? wscale[(size_t)bi * nk + t] : 1.0f;
        if (hcoords) {
            const int n = nk * vn * 3;
            const double* __restrict__ src = hcoords + (size_t)bi * n;
            double* dst = ck_lds() + CK_POINTS_AT;
            for (int i = t; i < n; i += HC_T) dst[i] = src[i];
        }
        __syncthreads();
    }

    __device__ __forceinline__ long long mask_at(int bi, int x, int y) const {
        return load_label_rt(mask_dtype, mask, (int64_t)bi * ms[0] + (int64_t)y * ms[1] + (int64_t)x * ms[2]);
    }
    // the class of a label value: 1 .. nk, or 0 for every value that gets no target (0, negative, >= class_num)
    __device__ __forceinline__ int class_of(long long m) const { return (m >= 1 && m <= nk) ? (int)m : 0; }

    // -- as a target source: the labels are read whether or not they are asked for (the weights and the targets depend on them)
    struct Lane8 {
        float wf[HC_PPL];
        unsigned long long cls = 0;   // byte i: the class of pixel i, 0 without a target
        int one = 0;                  // the one class of the lane's target pixels; 0: it has none, -1: they are of several classes
    };
    struct Image {};
    struct Pixel {
        long long m;
    };

    template <bool NT>
    __device__ __forceinline__ void pixels8(int bi, int p0, int C, bool, int* lab, Lane8& L) const {
        long long mv[HC_PPL];
        load8_mask<NT>(mask_dtype, mask, (int64_t)bi * ms[0] + p0, mv);
        const float* wt = weights();
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) {
            lab[i] = label_of(mv[i], C);
            const int c = class_of(mv[i]);
            L.wf[i] = c ? wt[c - 1] : 0.0f;
            L.cls |= (unsigned long long)c << (8 * i);
            if (c) L.one = L.one == 0 || L.one == c ? c : -1;
        }
    }
    template <bool NT>
    __device__ __forceinline__ void weights8(int, int, const Lane8& L, double* wd) const {
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) wd[i] = (double)L.wf[i];
    }

    // the targets of key-point k for a lane's eight consecutive pixels from (x0, y0) on
    __device__ __forceinline__ void targets8(int k, int x0, int y0, const Lane8& L, float* tx, float* ty) const {
#pragma unroll
        for (int i = 0; i < HC_PPL; ++i) tx[i] = ty[i] = 0.0f;
        if (L.one == 0) return;
        const double* pts = points() + 3 * k;
        int x = x0, y = y0;
        if (L.one > 0) {
            const double* hc = pts + (L.one - 1) * vn * 3;
            const double hx = hc[0], hy = hc[1], hz = hc[2];
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) {
                float ax, ay;
                kp_target(hx, hy, hz, x, y, motion != 0, ax, ay);
                const bool on = ((L.cls >> (8 * i)) & 0xFFu) != 0;
                tx[i] = on ? ax : 0.0f;
                ty[i] = on ? ay : 0.0f;
                if (++x == w) {
                    x = 0;
                    ++y;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < HC_PPL; ++i) {
                const int c = (int)((L.cls >> (8 * i)) & 0xFFu);
                const double* hc = pts + (c ? c - 1 : 0) * vn * 3;   // (a pixel without a target: any class's, the result is dropped)
                float ax, ay;
                kp_target(hc[0], hc[1], hc[2], x, y, motion != 0, ax, ay);
                tx[i] = c ? ax : 0.0f;
                ty[i] = c ? ay : 0.0f;
                if (++x == w) {
                    x = 0;
                    ++y;
                }
            }
        }
    }

    // the x and the y plane of a key-point per step; BOTH as in KpSource
    template <bool NT, bool BOTH, typename LOAD, typename USE>
    __device__ __forceinline__ void planes8(const double* __restrict__, int, int p0, int, const Lane8& L, LOAD load, USE use) const {
        const int y0 = p0 / w, x0 = p0 - y0 * w;
        for (int k = 0; k < vn; ++k) {
            float p[HC_PPL], q[HC_PPL], tx[HC_PPL], ty[HC_PPL];
            if (BOTH) {
                load(2 * k, p);
                load(2 * k + 1, q);
            }
            targets8(k, x0, y0, L, tx, ty);
            if (!BOTH) load(2 * k, p);
            use(2 * k, p, tx);
            if (!BOTH) load(2 * k + 1, q);
            use(2 * k + 1, q, ty);
        }
    }

    __device__ __forceinline__ Image image(int) const { return Image(); }
    __device__ __forceinline__ Pixel pixel1(int bi, int x, int y) const { return Pixel{mask_at(bi, x, y)}; }
    __device__ __forceinline__ int label1(int, int, int, int C, const Pixel& P) const { return label_of(P.m, C); }
    __device__ __forceinline__ float weight_of(long long m) const {
        const int c = class_of(m);
        return c ? weights()[c - 1] : 0.0f;
    }
    __device__ __forceinline__ double weight1(const Image&, int, int, int, const Pixel& P) const { return (double)weight_of(P.m); }
    __device__ __forceinline__ void target1(long long m, int k, int x, int y, float& tx, float& ty) const {
        tx = ty = 0.0f;
        const int c = class_of(m);
        if (c) {
            const double* hc = points() + ((c - 1) * vn + k) * 3;
            kp_target(hc[0], hc[1], hc[2], x, y, motion != 0, tx, ty);
        }
    }
    template <typename USE>
    __device__ __forceinline__ void planes1(const double* __restrict__, int, int x, int y, int, const Pixel& P, USE use) const {
        for (int k = 0; k < vn; ++k) {
            float tx, ty;
            target1(P.m, k, x, y, tx, ty);
            use(2 * k, tx);
            use(2 * k + 1, ty);
        }
    }
};

struct ClassTargetArgs {
    ClassKpSource K;
    float* vt;   // NULL: not asked for
    float* vw;   // NULL: not asked for
    int64_t ts[4], ws[3];
};

typedef HeadArgs<ClassKpSource> CkpHeadArgs;
typedef GradArgs<ClassKpSource> CkpGradArgs;

__device__ __forceinline__ void st8(float* base, int64_t off, const float* v) {
    f32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = v[i];
        b[i] = v[4 + i];
    }
    stv<false, f32x4>(base + off, a);
    stv<false, f32x4>(base + off + 4, b);
}

// ---- the materialising kernel ------------------------------------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(HC_T) void vertex_targets_classes_kernel(ClassTargetArgs A, const double* __restrict__ hcoords) {
    const ClassKpSource& K = A.K;
    const int bi = blockIdx.y;
    K.stage(A.vt ? hcoords : nullptr);   // (every lane of the workgroup: the barrier is in front of any return)
    if (FAST) {
        PVNET_SPARE_VGPRS(CKP_TARGETS_FAST_SPARE);
        const int p0 = blockIdx.x * HC_SEG + (int)threadIdx.x * HC_PPL;
        if (p0 >= K.npix) return;   // (npix is a multiple of 8 here: the lane's eight pixels are all inside)
        int lab[HC_PPL];
        ClassKpSource::Lane8 L;
        K.pixels8<false>(bi, p0, K.nk + 1, true, lab, L);
        if (A.vw) st8(A.vw, (int64_t)bi * A.ws[0] + p0, L.wf);
        if (!A.vt) return;
        const int y0 = p0 / K.w, x0 = p0 - y0 * K.w;
        const int64_t toff = (int64_t)bi * A.ts[0] + p0;
        for (int k = 0; k < K.vn; ++k) {
            float tx[HC_PPL], ty[HC_PPL];
            K.targets8(k, x0, y0, L, tx, ty);
            st8(A.vt, toff + (int64_t)(2 * k) * A.ts[1], tx);
            st8(A.vt, toff + (int64_t)(2 * k + 1) * A.ts[1], ty);
        }
    } else {
        PVNET_SPARE_VGPRS(CKP_TARGETS_GENERAL_SPARE);
        for (int j = 0; j < HC_PPL; ++j) {
            const int p = blockIdx.x * HC_SEG + j * HC_T + (int)threadIdx.x;
            if (p >= K.npix) break;
            const int y = p / K.w, x = p - y * K.w;
            const long long m = K.mask_at(bi, x, y);
            if (A.vw) A.vw[(int64_t)bi * A.ws[0] + (int64_t)y * A.ws[1] + (int64_t)x * A.ws[2]] = K.weight_of(m);
            if (!A.vt) continue;
            const int64_t toff = (int64_t)bi * A.ts[0] + (int64_t)y * A.ts[2] + (int64_t)x * A.ts[3];
            for (int k = 0; k < K.vn; ++k) {
                float tx, ty;
                K.target1(m, k, x, y, tx, ty);
                A.vt[toff + (int64_t)(2 * k) * A.ts[1]] = tx;
                A.vt[toff + (int64_t)(2 * k + 1) * A.ts[1]] = ty;
            }
        }
    }
}

// ---- the head on the class key-point source: the staging, head_common.h's bodies, the spare-VGPR constants, nothing else ---------
template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_partial_ckp_kernel(CkpHeadArgs A, const double* __restrict__ hcoords) {
    if (VT == VT_F32) PVNET_SPARE_VGPRS(CKP_HEAD_FAST_SPARE);
    else PVNET_SPARE_VGPRS(CKP_HEAD_FAST16_SPARE);
    A.T.stage(hcoords);
    head_partial8<VT, NT>(A, nullptr);
}

__global__ __launch_bounds__(HC_T) void head_partial_ckp_general_kernel(CkpHeadArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(CKP_HEAD_GENERAL_SPARE);
    A.T.stage(hcoords);
    head_partial1(A, nullptr);
}

__global__ __launch_bounds__(HC_FT) void head_final_ckp_kernel(CkpHeadArgs A) {
    PVNET_SPARE_VGPRS(CKP_HEAD_FINAL_SPARE);
    head_final_image(A);
}

template <bool FAST>
__global__ __launch_bounds__(HC_T) void head_grad_ckp_wsum_kernel(CkpGradArgs A) {
    PVNET_SPARE_VGPRS(CKP_GRAD_WSUM_SPARE);
    A.T.stage(nullptr);
    head_grad_wsum<FAST>(A);
}

__global__ __launch_bounds__(HC_FT) void head_grad_ckp_final_kernel(CkpGradArgs A) {
    PVNET_SPARE_VGPRS(CKP_GRAD_FINAL_SPARE);
    head_grad_final_image(A);
}

template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_grad_ckp_kernel(CkpGradArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(CKP_GRAD_FAST_SPARE);
    A.T.stage(A.gv ? hcoords : nullptr);
    head_grad8<VT, NT>(A, nullptr);
}

__global__ __launch_bounds__(HC_T) void head_grad_ckp_general_kernel(CkpGradArgs A, const double* __restrict__ hcoords) {
    PVNET_SPARE_VGPRS(CKP_GRAD_GENERAL_SPARE);
    A.T.stage(A.gv ? hcoords : nullptr);
    head_grad1(A, nullptr);
}

__global__ __launch_bounds__(HC_FT) void head_grad_ckp_status_kernel(CkpGradArgs A) {
    PVNET_SPARE_VGPRS(CKP_GRAD_STATUS_SPARE);
    head_grad_status_image(A);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// the class count's checks, behind head_common.h's: 0 or the code to return
int check_classes(int class_num, int vn) {
    if ((long long)(class_num - 1) * vn > PVNET_CLASS_TARGETS_MAX_TABLE) return PVNET_E_UNSUPPORTED;
    return 0;
}

ClassKpSource make_source(const void* mask, int mask_dtype, const int64_t* mask_strides, const float* weight_scale, int class_num,
                          int h, int w, int vn, uint32_t flags) {
    ClassKpSource K;
    K.mask = mask;
    K.wscale = weight_scale;
    for (int i = 0; i < 3; ++i) K.ms[i] = mask_strides[i];
    K.mask_dtype = mask_dtype;
    K.vn = vn;
    K.nk = class_num - 1;
    K.motion = (flags & PVNET_TARGETS_F_MOTION) ? 1 : 0;
    K.w = w;
    K.npix = h * w;
    K.nseg = (int)segments((size_t)K.npix);
    return K;
}

// the dynamic LDS of a workgroup: the weights' slots, and the key-points where the kernel makes targets
unsigned lds_bytes(const ClassKpSource& K, bool points) {
    return (unsigned)(CK_WEIGHT_SLOTS * sizeof(float) + (points ? (size_t)K.nk * K.vn * 3 * sizeof(double) : 0));
}

}  // namespace

extern "C" {

int pvnet_class_targets_abi_version(void) { return PVNET_CLASS_TARGETS_ABI_VERSION; }

int pvnet_vertex_targets_classes(const void* mask, int mask_dtype, const int64_t mask_strides[3], const double* hcoords,
                                 const float* weight_scale, int class_num, int b, int h, int w, int vn, uint32_t flags, float* vertex,
                                 const int64_t v_strides[4], float* vertex_weights, const int64_t w_strides[3], void* stream) {
    const bool pointers = mask && mask_strides && hcoords && (vertex || vertex_weights) && (!vertex || v_strides) &&
                          (!vertex_weights || w_strides);
    if (class_num > PVNET_CLASS_TARGETS_MAX_CLASSES) return PVNET_E_BADARG;
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, class_num, 1.0, flags, PVNET_TARGETS_F_MOTION)) return rc;
    if (const int rc = check_classes(class_num, vn)) return rc;
    if (b == 0) return 0;
    ClassTargetArgs A;
    A.K = make_source(mask, mask_dtype, mask_strides, weight_scale, class_num, h, w, vn, flags);
    A.vt = vertex;
    A.vw = vertex_weights;
    for (int i = 0; i < 4; ++i) A.ts[i] = vertex ? v_strides[i] : 0;
    for (int i = 0; i < 3; ++i) A.ws[i] = vertex_weights ? w_strides[i] : 0;
    const bool fast = A.K.npix % HC_PPL == 0 && linear3(mask, b, A.K.ms, w) && (!vertex || linear4(vertex, b, A.ts, w)) &&
                      (!vertex_weights || linear3(vertex_weights, b, A.ws, w));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.K.nseg, (unsigned)b);
    const unsigned lds = lds_bytes(A.K, vertex != nullptr);
    if (fast) hipLaunchKernelGGL(vertex_targets_classes_kernel<true>, grid, dim3(HC_T), lds, s, A, hcoords);
    else hipLaunchKernelGGL(vertex_targets_classes_kernel<false>, grid, dim3(HC_T), lds, s, A, hcoords);
    return launched();
}

size_t pvnet_head_metrics_ckp_workspace_bytes(int b, int h, int w) { return head_workspace_bytes(b, h, w); }

int pvnet_head_metrics_ckp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                           const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                           int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                           double* losses, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const bool pointers = seg_pred && seg_strides && vertex_pred && vp_strides && hcoords && mask && mask_strides && losses && counts;
    if (num_classes > PVNET_CLASS_TARGETS_MAX_CLASSES) return PVNET_E_BADARG;
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, num_classes, sigma, flags, HEAD_FLAGS | PVNET_TARGETS_F_MOTION)) return rc;
    if (const int rc = check_classes(num_classes, vn)) return rc;
    if (b == 0) return 0;
    if (const int rc = check_workspace(workspace, workspace_bytes, head_workspace_bytes(b, h, w))) return rc;
    CkpHeadArgs A;
    A.T = make_source(mask, mask_dtype, mask_strides, weight_scale, num_classes, h, w, vn, flags);
    fill_inputs(A, seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, h, w, vn, sigma, flags);
    fill_head(A, losses, counts, status, workspace);
    const bool fast = A.npix % HC_PPL == 0 && linear4(seg_pred, b, A.ss, w) && linear4(vertex_pred, b, A.vs, w) && linear3(mask, b, A.T.ms, w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    const unsigned lds = lds_bytes(A.T, true);
    if (fast)
        launch_fast(A.vp_type, flags, [&](auto vt, auto nt) {
            hipLaunchKernelGGL((head_partial_ckp_kernel<decltype(vt)::value, decltype(nt)::value>), grid, dim3(HC_T), lds, s, A, hcoords);
        });
    else
        hipLaunchKernelGGL(head_partial_ckp_general_kernel, grid, dim3(HC_T), lds, s, A, hcoords);
    hipLaunchKernelGGL(head_final_ckp_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    return launched();
}

size_t pvnet_head_grad_ckp_workspace_bytes(int b, int h, int w) { return grad_workspace_bytes(b, h, w); }

int pvnet_head_grad_ckp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                        const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                        int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                        const double* upstream, void* grad_seg, const int64_t gs_strides[4], void* grad_vertex,
                        const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const bool pointers = seg_pred && seg_strides && vertex_pred && vp_strides && hcoords && mask && mask_strides && upstream &&
                          (grad_seg || grad_vertex) && (!grad_seg || gs_strides) && (!grad_vertex || gv_strides);
    if (num_classes > PVNET_CLASS_TARGETS_MAX_CLASSES) return PVNET_E_BADARG;
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, num_classes, sigma, flags, HEAD_FLAGS | PVNET_TARGETS_F_MOTION)) return rc;
    if (const int rc = check_classes(num_classes, vn)) return rc;
    if (b == 0) return 0;
    if (const int rc = check_workspace(workspace, workspace_bytes, grad_workspace_bytes(b, h, w))) return rc;
    CkpGradArgs A;
    A.T = make_source(mask, mask_dtype, mask_strides, weight_scale, num_classes, h, w, vn, flags);
    fill_inputs(A, seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, h, w, vn, sigma, flags);
    fill_grad(A, b, upstream, grad_seg, gs_strides, grad_vertex, gv_strides, status, workspace);
    // the labels are read by either half; each half asks the fast path's shape of its own tensors beyond them
    const bool lin_m = linear3(mask, b, A.T.ms, w);
    const bool fast = A.npix % HC_PPL == 0 && lin_m && (!grad_seg || (linear4(seg_pred, b, A.ss, w) && linear4(grad_seg, b, A.gss, w))) &&
                      (!grad_vertex || (linear4(vertex_pred, b, A.vs, w) && linear4(grad_vertex, b, A.gvs, w)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    const unsigned lds = lds_bytes(A.T, grad_vertex != nullptr);
    if (grad_vertex) {
        if (A.npix % HC_PPL == 0 && lin_m) hipLaunchKernelGGL(head_grad_ckp_wsum_kernel<true>, grid, dim3(HC_T), lds_bytes(A.T, false), s, A);
        else hipLaunchKernelGGL(head_grad_ckp_wsum_kernel<false>, grid, dim3(HC_T), lds_bytes(A.T, false), s, A);
    }
    hipLaunchKernelGGL(head_grad_ckp_final_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    if (fast)
        launch_fast(A.vp_type, flags, [&](auto vt, auto nt) {
            hipLaunchKernelGGL((head_grad_ckp_kernel<decltype(vt)::value, decltype(nt)::value>), grid, dim3(HC_T), lds, s, A, hcoords);
        });
    else
        hipLaunchKernelGGL(head_grad_ckp_general_kernel, grid, dim3(HC_T), lds, s, A, hcoords);
    if (status) hipLaunchKernelGGL(head_grad_ckp_status_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    return launched();
}

}  // extern "C"
