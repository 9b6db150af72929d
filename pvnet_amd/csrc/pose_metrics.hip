// pose_metrics.hip -- the pose metrics after the pose solve, on the device: ADD / ADD-S, the 2-D projection error (plain or
// symmetric) and 5cm5deg for a batch of images in one call.  C ABI: pvnet_pose_metrics in include/pvnet_vote.h.
//
// Restates the host Evaluator's per-image metrics (pvnet_amd/evaluation.py: add_error, projection_2d_error, pnp.cm_degree_error,
// the recorder thresholds of Evaluator._record), which is this file's oracle (tests/test_pose_metrics_device.py).  Three kernels:
//
//   metrics_points_kernel  grid (point tiles, images).  Every lane transforms one model point by the predicted and the target pose
//                          and projects both, in float64 with the host's formulas term by term (model @ R^T + t, then p @ K^T and
//                          xy / z, the general 3x3 K); each workgroup writes the sums of its tile's 3-D and 2-D distances (a
//                          fixed-order tree).  For images of a symmetric class it also sets the packed nearest-neighbour word of
//                          every query to "none".
//   metrics_search_kernel  grid (query tiles, reference slices, images x searches).  The ADD-S / symmetric-projection search of
//                          find_nearest_point_distance(pred, target): queries = target points, reference cloud = predicted points,
//                          both the float32 roundings of the float64 clouds -- what the host feeds pvnet_nn.  The layout is
//                          pvnet_nn.hip's: the reference slice streams through LDS in tiles of 256 points read back by broadcast,
//                          float32 squared distance in the reference's order, strict `<` (the first index wins ties), slices
//                          combined with a 64-bit atomicMin on (distance bits, index).  The clouds are computed here, not stored:
//                          a tile's transform is ~60 float64 operations per lane against 256 x 11 float32 ones of its search.
//                          One kernel serves 2-D and 3-D: a 2-D point stored with z = 0 gives the bitwise-same squared distance,
//                          (dx^2 + dy^2) + 0 * 0 being exact.  Blocks of non-symmetric images return at once.
//   metrics_final_kernel   a workgroup per image.  Reduces the tile sums in a fixed order (bitwise reproducible), or, for
//                          symmetric images, recomputes |pred[idx] - target| in float64 with the same device functions and
//                          reduces it the same way; 5cm5deg as pnp.cm_degree_error; errors, pass flags and status.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pvnet_vote.h"

// no contraction anywhere in this file: the clouds must round as the host's numpy expressions do (the float32 roundings feed a
// search whose ties are decided bit for bit), and the search's squared distance as the reference's float32 expression does
#pragma clang fp contract(off)

namespace {

// one unused VGPR granule beyond what a kernel uses: see PVNET_SPARE_VGPRS in vote_common.h
#define PVNET_SPARE_VGPRS_(r) asm volatile("" ::: "v" #r)
#define PVNET_SPARE_VGPRS(r) PVNET_SPARE_VGPRS_(r)

constexpr int PM_T = 256;  // lanes per workgroup = model points per tile = queries per search workgroup
constexpr unsigned long long PM_NONE = ((unsigned long long)0x7F7FFFFFu << 32) | 0xFFFFFFFFull;  // (FLT_MAX, no index)
constexpr int PM_MAX_POINTS = 1 << 24;

struct MetricArgs {
    const double* pose_pred;    // [n,3,4]
    const void* pose_target;    // [n,3,4] f32 or f64
    int target_f64;
    const double* model;        // [total,3]
    const int32_t* offsets;     // [num_classes+1]
    const double* diameters;    // [num_classes]
    const uint8_t* symmetric;   // [num_classes]
    int num_classes, max_points, tiles, searches, slice;
    const int32_t* class_ids;   // [n] or null
    const double* K;            // [3,3] or [n,3,3]
    int k_per_image;
    double th_proj, th_add, th_cm, th_deg;
    double* errors;             // [n,4]
    uint8_t* passed;            // [n,3]
    int32_t* status;            // [n] or null
    unsigned long long* best;   // workspace: [n, searches, max_points] packed (distance bits, index)
    double* partial;            // workspace: [n, tiles, 2] tile sums of the 3-D and 2-D distances
};

struct ImageClass {
    int ok;        // 0, or the status: -1 class id out of range, -2 point count outside 1..max_points
    int cls, off, np, sym;
};

__device__ inline ImageClass image_class(const MetricArgs& A, int i) {
    ImageClass r{0, 0, 0, 0, 0};
    const int c = A.class_ids ? A.class_ids[i] : 0;
    if (c < 0 || c >= A.num_classes) {
        r.ok = -1;
        return r;
    }
    r.cls = c;
    r.off = A.offsets[c];
    r.np = A.offsets[c + 1] - r.off;
    if (r.np < 1 || r.np > A.max_points || r.off < 0) {
        r.ok = -2;
        return r;
    }
    r.sym = A.symmetric[c] != 0;
    return r;
}

__device__ inline void load_pred(const MetricArgs& A, int i, double* P) {
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = A.pose_pred[(size_t)i * 12 + k];
}
__device__ inline void load_target(const MetricArgs& A, int i, double* P) {
    if (A.target_f64) {
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = static_cast<const double*>(A.pose_target)[(size_t)i * 12 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = (double)static_cast<const float*>(A.pose_target)[(size_t)i * 12 + k];
    }
}
__device__ inline void load_K(const MetricArgs& A, int i, double* K) {
    const double* k = A.K + (A.k_per_image ? (size_t)i * 9 : 0);
#pragma unroll
    for (int j = 0; j < 9; ++j) K[j] = k[j];
}

// model @ R^T + t, element by element as numpy's dot rounds it without FMA: ((m0 R[r,0] + m1 R[r,1]) + m2 R[r,2]) + t[r]
__device__ inline void transform(const double* P, const double* m, double* a) {
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = m[0] * P[r * 4] + m[1] * P[r * 4 + 1] + m[2] * P[r * 4 + 2] + P[r * 4 + 3];
}
// pnp.project after the transform: p @ K^T, then xy / z
__device__ inline void project(const double* K, const double* a, double* x) {
    const double u = a[0] * K[0] + a[1] * K[1] + a[2] * K[2];
    const double v = a[0] * K[3] + a[1] * K[4] + a[2] * K[5];
    const double w = a[0] * K[6] + a[1] * K[7] + a[2] * K[8];
    x[0] = u / w;
    x[1] = v / w;
}
__device__ inline double dist3(const double* a, const double* b) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}
__device__ inline double dist2(const double* a, const double* b) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1];
    return sqrt(d0 * d0 + d1 * d1);
}

// the sum of every lane's value over the workgroup in a fixed tree order (all PM_T lanes must call it)
__device__ inline double block_sum(double v, double* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int h = PM_T / 2; h > 0; h >>= 1) {
        if (t < h) s[t] = s[t] + s[t + h];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(PM_T) void metrics_points_kernel(MetricArgs A) {
    PVNET_SPARE_VGPRS(79);
    __shared__ double s_sum[PM_T];
    const int i = blockIdx.y;
    const ImageClass c = image_class(A, i);
    const int j0 = blockIdx.x * PM_T;
    if (c.ok != 0 || j0 >= c.np) return;   // uniform over the workgroup
    const int j = j0 + (int)threadIdx.x;
    double d3 = 0.0, d2 = 0.0;
    if (j < c.np) {
        double Pp[12], Pt[12], K[9], m[3], a[3], b[3], xa[2], xb[2];
        load_pred(A, i, Pp);
        load_target(A, i, Pt);
        load_K(A, i, K);
        const double* mp = A.model + (size_t)(c.off + j) * 3;
        m[0] = mp[0];
        m[1] = mp[1];
        m[2] = mp[2];
        transform(Pp, m, a);
        transform(Pt, m, b);
        d3 = dist3(a, b);
        project(K, a, xa);
        project(K, b, xb);
        d2 = dist2(xa, xb);
        if (c.sym) {
            unsigned long long* w = A.best + (size_t)i * A.searches * A.max_points + j;
            for (int s = 0; s < A.searches; ++s) w[(size_t)s * A.max_points] = PM_NONE;
        }
    }
    const double t3 = block_sum(d3, s_sum);
    const double t2 = block_sum(d2, s_sum);
    if (threadIdx.x == 0) {
        double* p = A.partial + ((size_t)i * A.tiles + blockIdx.x) * 2;
        p[0] = t3;
        p[1] = t2;
    }
}

// the float32 point the search sees for model point m: the 3-D cloud (search 0) or the projected one with z = 0 (search 1)
__device__ inline float4 search_point(const double* P, const double* K, const double* m, int proj) {
    double a[3];
    transform(P, m, a);
    if (proj) {
        double x[2];
        project(K, a, x);
        return make_float4((float)x[0], (float)x[1], 0.f, 0.f);
    }
    return make_float4((float)a[0], (float)a[1], (float)a[2], 0.f);
}

__global__ __launch_bounds__(PM_T) void metrics_search_kernel(MetricArgs A) {
    PVNET_SPARE_VGPRS(95);
    __shared__ float4 s_ref[PM_T];
    const int i = blockIdx.z / A.searches;
    const int s = blockIdx.z - i * A.searches;
    const ImageClass c = image_class(A, i);
    const int r0 = blockIdx.y * A.slice;
    if (c.ok != 0 || !c.sym || (int)blockIdx.x * PM_T >= c.np || r0 >= c.np) return;   // uniform over the workgroup
    const int r1 = r0 + A.slice < c.np ? r0 + A.slice : c.np;
    const int q = blockIdx.x * PM_T + threadIdx.x;
    double Pp[12], Pt[12], K[9], m[3];
    load_pred(A, i, Pp);
    load_target(A, i, Pt);
    load_K(A, i, K);
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (q < c.np) {
        const double* mp = A.model + (size_t)(c.off + q) * 3;
        m[0] = mp[0];
        m[1] = mp[1];
        m[2] = mp[2];
        const float4 p = search_point(Pt, K, m, s);
        qx = p.x;
        qy = p.y;
        qz = p.z;
    }
    float min_dist = FLT_MAX;
    int min_idx = -1;
    for (int t0 = r0; t0 < r1; t0 += PM_T) {
        const int nt = r1 - t0 < PM_T ? r1 - t0 : PM_T;
        __syncthreads();  // the previous tile has been consumed
        if ((int)threadIdx.x < nt) {
            const double* mp = A.model + (size_t)(c.off + t0 + threadIdx.x) * 3;
            m[0] = mp[0];
            m[1] = mp[1];
            m[2] = mp[2];
            s_ref[threadIdx.x] = search_point(Pp, K, m, s);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < nt; ++j) {
            const float4 r = s_ref[j];
            const float dx = r.x - qx, dy = r.y - qy, dz = r.z - qz;
            const float dist = dx * dx + dy * dy + dz * dz;
            const bool lt = dist < min_dist;  // strict: the first index wins ties
            min_idx = lt ? t0 + j : min_idx;
            min_dist = lt ? dist : min_dist;
        }
    }
    if (q < c.np && min_idx >= 0) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(min_dist) << 32) | (uint32_t)min_idx;
        atomicMin(A.best + ((size_t)i * A.searches + s) * A.max_points + q, key);
    }
}

__global__ __launch_bounds__(PM_T) void metrics_final_kernel(MetricArgs A) {
    PVNET_SPARE_VGPRS(127);
    __shared__ double s_sum[PM_T];
    const int i = blockIdx.x;
    const int t = threadIdx.x;
    const ImageClass c = image_class(A, i);
    double* err = A.errors + (size_t)i * 4;
    uint8_t* ok = A.passed + (size_t)i * 3;
    if (c.ok != 0) {   // nothing of the class table is read past this point
        if (t < 4) err[t] = __builtin_nan("");
        if (t < 3) ok[t] = 0;
        if (t == 0 && A.status) A.status[i] = c.ok;
        return;
    }
    double Pp[12], Pt[12], K[9];
    load_pred(A, i, Pp);
    load_target(A, i, Pt);
    load_K(A, i, K);
    const int tiles = (c.np + PM_T - 1) / PM_T;
    // plain metrics: the tile sums of metrics_points_kernel, lane t summing tiles t, t + PM_T, ... then the tree
    double v3 = 0.0, v2 = 0.0;
    for (int k = t; k < tiles; k += PM_T) {
        const double* p = A.partial + ((size_t)i * A.tiles + k) * 2;
        v3 = v3 + p[0];
        v2 = v2 + p[1];
    }
    double add = block_sum(v3, s_sum);
    double proj = block_sum(v2, s_sum);
    if (c.sym) {
        // nearest-neighbour metrics: lane t sums queries t, t + PM_T, ... in order, then the tree
        const unsigned long long* w = A.best + (size_t)i * A.searches * A.max_points;
        for (int s = 0; s < A.searches; ++s) {
            double v = 0.0;
            for (int j = t; j < c.np; j += PM_T) {
                const unsigned long long key = w[(size_t)s * A.max_points + j];
                int idx = key == PM_NONE ? 0 : (int)(uint32_t)(key & 0xFFFFFFFFull);   // no finite hit: index 0, as pvnet_nn
                idx = idx < c.np ? idx : 0;
                const double* mq = A.model + (size_t)(c.off + j) * 3;
                const double* mr = A.model + (size_t)(c.off + idx) * 3;
                const double mqv[3] = {mq[0], mq[1], mq[2]}, mrv[3] = {mr[0], mr[1], mr[2]};
                double a[3], b[3];
                transform(Pp, mrv, a);
                transform(Pt, mqv, b);
                if (s == 0) {
                    v = v + dist3(a, b);
                } else {
                    double xa[2], xb[2];
                    project(K, a, xa);
                    project(K, b, xb);
                    v = v + dist2(xa, xb);
                }
            }
            const double sum = block_sum(v, s_sum);
            if (s == 0) add = sum;
            else proj = sum;
        }
    }
    if (t != 0) return;
    add = add / (double)c.np;
    proj = proj / (double)c.np;
    // pnp.cm_degree_error: |t_p - t_t| * 100 and arccos(clip((min(trace(R_p R_t^T), 3) - 1) / 2, -1, 1)) in degrees
    const double e0 = Pp[3] - Pt[3], e1 = Pp[7] - Pt[7], e2 = Pp[11] - Pt[11];
    const double cm = sqrt(e0 * e0 + e1 * e1 + e2 * e2) * 100.0;
    double tr = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) tr = tr + (Pp[r * 4] * Pt[r * 4] + Pp[r * 4 + 1] * Pt[r * 4 + 1] + Pp[r * 4 + 2] * Pt[r * 4 + 2]);
    const double cl = 3.0 < tr ? 3.0 : tr;   // Python's min(tr, 3.0): NaN stays NaN
    double x = (cl - 1.0) / 2.0;
    x = x > 1.0 ? 1.0 : (x < -1.0 ? -1.0 : x);   // np.clip: NaN stays NaN
    const double deg = acos(x) * (180.0 / M_PI);
    err[0] = proj;
    err[1] = add;
    err[2] = cm;
    err[3] = deg;
    ok[0] = proj < A.th_proj;
    ok[1] = add < A.diameters[c.cls] * A.th_add;
    ok[2] = cm < A.th_cm && deg < A.th_deg;
    if (A.status) A.status[i] = 0;
}

}  // namespace

extern "C" {

size_t pvnet_pose_metrics_workspace_bytes(int n, int max_points, int flags) {
    if (n <= 0 || max_points <= 0 || max_points > PM_MAX_POINTS) return 0;
    const size_t searches = (flags & PVNET_METRIC_SYM_PROJECTION) ? 2 : 1;
    const size_t tiles = ((size_t)max_points + PM_T - 1) / PM_T;
    const size_t bytes = (size_t)n * searches * max_points * sizeof(unsigned long long) + (size_t)n * tiles * 2 * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

int pvnet_pose_metrics(const double* pose_pred, const void* pose_target, int target_f64, const double* model_pts,
                       const int32_t* class_offsets, const double* diameters, const uint8_t* symmetric, int num_classes,
                       int max_points, const int32_t* class_ids, const double* K, int k_per_image, int n, int flags,
                       const double thresholds[4], double* errors, uint8_t* passed, int32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!pose_pred || !pose_target || !model_pts || !class_offsets || !diameters || !symmetric || !K || !thresholds || !errors ||
        !passed)
        return PVNET_E_BADARG;
    if (num_classes <= 0 || max_points <= 0 || n < 0 || (flags & ~PVNET_METRIC_SYM_PROJECTION) != 0) return PVNET_E_BADARG;
    if (max_points > PM_MAX_POINTS) return PVNET_E_UNSUPPORTED;
    const int searches = (flags & PVNET_METRIC_SYM_PROJECTION) ? 2 : 1;
    if (n > 65535 / searches) return PVNET_E_UNSUPPORTED;   // images x searches on the search grid's z
    if (n == 0) return 0;
    if (!workspace || workspace_bytes < pvnet_pose_metrics_workspace_bytes(n, max_points, flags)) return PVNET_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return PVNET_E_BADARG;
    MetricArgs A;
    A.pose_pred = pose_pred;
    A.pose_target = pose_target;
    A.target_f64 = target_f64 ? 1 : 0;
    A.model = model_pts;
    A.offsets = class_offsets;
    A.diameters = diameters;
    A.symmetric = symmetric;
    A.num_classes = num_classes;
    A.max_points = max_points;
    A.tiles = (max_points + PM_T - 1) / PM_T;
    A.searches = searches;
    A.class_ids = class_ids;
    A.K = K;
    A.k_per_image = k_per_image ? 1 : 0;
    A.th_proj = thresholds[0];
    A.th_add = thresholds[1];
    A.th_cm = thresholds[2];
    A.th_deg = thresholds[3];
    A.errors = errors;
    A.passed = passed;
    A.status = status;
    A.best = static_cast<unsigned long long*>(workspace);
    A.partial = reinterpret_cast<double*>(A.best + (size_t)n * searches * max_points);
    // the search: enough workgroups to fill the chip (~4 per CU) over all images and searches, never slices shorter than a tile;
    // the host cannot know which images are symmetric (class ids live on the device), so it sizes for all of them
    const long long per_slice = (long long)A.tiles * n * searches;
    const long long want = (1024 + per_slice - 1) / per_slice;
    int nslices = (int)(want < 1 ? 1 : (want > A.tiles ? A.tiles : want));
    if (nslices > 65535) nslices = 65535;
    A.slice = ((A.tiles + nslices - 1) / nslices) * PM_T;
    nslices = (max_points + A.slice - 1) / A.slice;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(metrics_points_kernel, dim3((unsigned)A.tiles, (unsigned)n), dim3(PM_T), 0, s, A);
    hipLaunchKernelGGL(metrics_search_kernel, dim3((unsigned)A.tiles, (unsigned)nslices, (unsigned)(n * searches)), dim3(PM_T), 0,
                       s, A);
    hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)n), dim3(PM_T), 0, s, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"
