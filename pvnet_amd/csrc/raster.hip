// raster.hip -- libpvnet_raster.so: silhouettes and label images of posed meshes (include/pvnet_raster.h holds THE DEFINITION).
//
// Path replaced (reference tree): mesh_binary_rasterization (lib/utils/extend_utils/src/mesh_rasterization.cpp:43-71), a serial loop
// over the triangles of one image on the host, and Projector.project_K in front of it (lib/utils/base_utils.py:290-294).
//
// An object mesh has tens of thousands of triangles of a few pixels each, so the work is TRIANGLE-parallel into bit planes (one
// [h, ceil(w/32)] uint32 plane per instance), not pixel-parallel over a triangle list:
//   setup_kernel        (pvnet_render only) one workgroup: the instance table (mesh_core.h), which arrives in the launch's arguments, becomes
//                       records in the workspace (mesh ranges, the prefix of the faces for tri_out); status and counters zeroed
//   clear_check_kernel  clears the planes with 16-byte stores; other workgroups of the same launch evaluate camera z of every vertex
//                       of every instance (PVNET_RASTER_S_BEHIND)
//   triangle_kernel     one lane per (instance, triangle): projects its three vertices (stage P: the same operations whichever
//                       triangle asks, so a shared vertex gets the same bits), computes the box; a box of at most
//                       PVNET_RASTER_LANE_PIXELS pixels the lane walks alone: per touched word it reads the plane, skips set bits and
//                       commits with one atomicOr; larger boxes are taken one after the other by the whole wave, lanes across 64
//                       pixels of a row, a ballot forming the two words, one atomicOr per non-zero word
//   expand_kernel       per target image: the planes of its instances in painter's order -> uint8 labels, 16 pixels per lane
// Bits are only ever OR-ed into planes that the call itself cleared: the result does not depend on the order of the atomics.
//
// The predicate and the projection are evaluated without contraction (FP_CONTRACT OFF below; tests/test_raster_cpu.py looks for
// fused float32 instructions in the assembly) and with float32 denormals kept (the compiler's default for gfx950).
#include <algorithm>

#include "vote_common.h"

#include "pvnet_raster.h"
#include "mesh_core.h"   // project, make_edge, same_side, inside: shared with depth.hip, shade.hip and texture.hip

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

constexpr int TPB = 256;   // lanes per workgroup of every kernel but setup_kernel

struct Inst {   // one instance, as the kernels read it
    int voff, vcnt, foff, fcnt, tri0, image, label, pad;
};
static_assert(sizeof(Inst) == 32, "workspace layout");

static_assert(PVNET_RASTER_MAX_INSTANCES == MAX_INSTANCES && PVNET_RASTER_MAX_MESHES == MAX_MESHES && PVNET_RASTER_MAX_IMAGES == MAX_IMAGES &&
                  PVNET_RASTER_MAX_SIDE == MAX_IMAGE_SIDE, "mesh_core.h's Table and checks are written in this public header's limits");

constexpr size_t WS_HEAD = 16;   // counters: [0] triangles that took the cooperative path

__global__ __launch_bounds__(1024) void setup_kernel(Table T, int q, Inst* recs, int32_t* status, uint32_t* counters) {
    PVNET_SPARE_VGPRS(31);
    __shared__ int s_scan[1024];
    const int t = threadIdx.x;
    Inst r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t < q) {
        const uint32_t e = T.inst[t];
        const int m = (int)(e & 63u);
        r.voff = T.voff[m];
        r.vcnt = T.voff[m + 1] - r.voff;
        r.foff = T.foff[m];
        r.fcnt = T.foff[m + 1] - r.foff;
        r.label = (int)((e >> 6) & 255u);
        r.image = (int)(e >> 14);
    }
    s_scan[t] = r.fcnt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // inclusive prefix of the face counts
        const int u = t >= o ? s_scan[t - o] : 0;
        __syncthreads();
        s_scan[t] += u;
        __syncthreads();
    }
    if (t < q) {
        r.tri0 = s_scan[t] - r.fcnt;
        recs[t] = r;
        if (status) status[t] = 0;
    }
    if (t < 4) counters[t] = 0u;
}

struct ClearParams {
    uint4* planes;
    size_t n16;          // 16-byte words of the planes
    int clear_blocks;    // the first workgroups of the launch clear; the others check vertices
    int zero_status_n;   // pvnet_raster_triangles: status[0 .. n) and the counters are zeroed here (no setup launch)
    int32_t* status;
    uint32_t* counters;
    const Inst* recs;
    int vblocks;         // workgroups per instance over its vertices
    const double* vertices;
    const double* poses;
};

__global__ __launch_bounds__(TPB) void clear_check_kernel(ClearParams P) {
    PVNET_SPARE_VGPRS(31);
    if ((int)blockIdx.x < P.clear_blocks) {
        const size_t gid = (size_t)blockIdx.x * TPB + threadIdx.x, stride = (size_t)P.clear_blocks * TPB;
        for (size_t i = gid; i < P.n16; i += stride) P.planes[i] = make_uint4(0u, 0u, 0u, 0u);
        if (P.zero_status_n) {
            if (P.status)
                for (size_t i = gid; i < (size_t)P.zero_status_n; i += stride) P.status[i] = 0;
            if (gid < 4) P.counters[gid] = 0u;
        }
        return;
    }
    const int bid = (int)blockIdx.x - P.clear_blocks;
    const int inst = bid / P.vblocks, v = (bid - inst * P.vblocks) * TPB + (int)threadIdx.x;
    const Inst r = P.recs[inst];
    bool behind = false;
    if (v < r.vcnt) {
        const double* X = P.vertices + (size_t)(r.voff + v) * 3;
        const double* pose = P.poses + (size_t)inst * 12;
        const double c2 = ((pose[8] * X[0] + pose[9] * X[1]) + pose[10] * X[2]) + pose[11];
        behind = c2 <= 0.0;
    }
    const unsigned long long any = __ballot(behind);
    if (any && (int)(threadIdx.x & 63) == __ffsll((long long)any) - 1) atomicOr(&P.status[inst], PVNET_RASTER_S_BEHIND);
}

struct TriParams {
    const float* tri;   // pvnet_raster_triangles: [n,tn,3,2]; NULL for pvnet_render
    int tn;
    const Inst* recs;
    const double* vertices;
    const int32_t* faces;
    const double* poses;
    const double* K;
    int k_stride;       // 0 or 9
    float* tri_out;
    int32_t* status;
    uint32_t* planes;   // NULL: project only
    uint32_t* counters;
    int h, w, w32;
};

__device__ __forceinline__ float bcast(float v, int src) { return __shfl(v, src, 64); }

__global__ __launch_bounds__(TPB) void triangle_kernel(TriParams P) {
    PVNET_SPARE_VGPRS(95);
    const int inst = blockIdx.y, lane = threadIdx.x & 63;
    const int f = (int)blockIdx.x * TPB + (int)threadIdx.x;
    Inst r = {0, 0, 0, P.tn, 0, 0, 0, 0};
    if (!P.tri) r = P.recs[inst];
    bool valid = f < r.fcnt;
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    int st = 0;
    if (valid) {
        if (P.tri) {
            const float2* t = reinterpret_cast<const float2*>(P.tri) + ((size_t)inst * P.tn + f) * 3;
            const float2 a = t[0], b = t[1], c = t[2];
            x0 = a.x; y0 = a.y; x1 = b.x; y1 = b.y; x2 = c.x; y2 = c.y;
        } else {
            const int32_t* fc = P.faces + (size_t)(r.foff + f) * 3;
            const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
            if ((unsigned)i0 >= (unsigned)r.vcnt || (unsigned)i1 >= (unsigned)r.vcnt || (unsigned)i2 >= (unsigned)r.vcnt) {
                st |= PVNET_RASTER_S_BADFACE;
                valid = false;
                x0 = y0 = x1 = y1 = x2 = y2 = __builtin_nanf("");
            } else {
                const double* pose = P.poses + (size_t)inst * 12;
                const double* K = P.K + (size_t)inst * P.k_stride;
                const double* V = P.vertices + (size_t)r.voff * 3;
                project(pose, K, V + (size_t)i0 * 3, x0, y0);
                project(pose, K, V + (size_t)i1 * 3, x1, y1);
                project(pose, K, V + (size_t)i2 * 3, x2, y2);
            }
            if (P.tri_out) {
                float2* o = reinterpret_cast<float2*>(P.tri_out) + ((size_t)r.tri0 + f) * 3;
                o[0] = make_float2(x0, y0);
                o[1] = make_float2(x1, y1);
                o[2] = make_float2(x2, y2);
            }
        }
    }
    if (!P.planes) return;   // block-uniform: project only
    if (valid && !(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) {
        st |= PVNET_RASTER_S_NONFINITE;
        valid = false;
    }
    if (st && P.status) atomicOr(&P.status[inst], st);

    int begx = 0, endx = -1, begy = 0, endy = -1;
    if (valid) {
        const float minx = fmaxf(0.f, fminf(fminf(x0, x1), x2)), maxx = fminf((float)(P.w - 2), fmaxf(fmaxf(x0, x1), x2));
        const float miny = fmaxf(0.f, fminf(fminf(y0, y1), y2)), maxy = fminf((float)(P.h - 2), fmaxf(fmaxf(y0, y1), y2));
        const float ex = maxx + 1.f, ey = maxy + 1.f;
        // the emptiness rule of the header, in float before any cast
        if (minx >= (float)P.w || ex <= -1.f || miny >= (float)P.h || ey <= -1.f) {
            valid = false;
        } else {
            begx = (int)minx; endx = (int)ex; begy = (int)miny; endy = (int)ey;
            // (what the clamps above already guarantee, stated for the stores below: no bit outside the plane)
            begx = max(begx, 0); begy = max(begy, 0); endx = min(endx, P.w - 1); endy = min(endy, P.h - 1);
            valid = begx <= endx && begy <= endy;
        }
    }
    const Edge e0 = make_edge(x0, y0, x1, y1, x2, y2), e1 = make_edge(x1, y1, x2, y2, x0, y0), e2 = make_edge(x2, y2, x0, y0, x1, y1);
    uint32_t* plane = P.planes + (size_t)inst * P.h * P.w32;
    const int area = valid ? (endx - begx + 1) * (endy - begy + 1) : 0;   // (at most 32768^2 = 2^30)
    const bool large = area > PVNET_RASTER_LANE_PIXELS;

    if (valid && !large) {   // the lane alone: at most PVNET_RASTER_LANE_PIXELS pixels
        for (int yi = begy; yi <= endy; ++yi) {
            const float py = (float)yi;
            uint32_t* row = plane + (size_t)yi * P.w32;
            for (int wi = begx >> 5; wi <= (endx >> 5); ++wi) {
                const int xl = max(begx, wi << 5), xh = min(endx, (wi << 5) + 31);
                const uint32_t have = __hip_atomic_load(row + wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                uint32_t add = 0u;
                for (int xi = xl; xi <= xh; ++xi) {
                    const uint32_t bit = 1u << (xi & 31);
                    if (have & bit) continue;   // the reference's early-out: the result is an OR
                    if (inside(e0, e1, e2, (float)xi, py)) add |= bit;
                }
                if (add) atomicOr(row + wi, add);
            }
        }
    }

    // the cooperative path: the wave takes its large triangles one after the other, lanes across 64 pixels of a row
    unsigned long long big = __ballot(large);
    if (big && lane == (int)(__ffsll((long long)big) - 1)) atomicAdd(&P.counters[0], (uint32_t)__popcll(big));
    while (big) {   // wave-uniform
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        Edge c0, c1, c2;
        c0.xa = bcast(e0.xa, src); c0.ya = bcast(e0.ya, src); c0.nx = bcast(e0.nx, src); c0.ny = bcast(e0.ny, src); c0.val0 = bcast(e0.val0, src);
        c1.xa = bcast(e1.xa, src); c1.ya = bcast(e1.ya, src); c1.nx = bcast(e1.nx, src); c1.ny = bcast(e1.ny, src); c1.val0 = bcast(e1.val0, src);
        c2.xa = bcast(e2.xa, src); c2.ya = bcast(e2.ya, src); c2.nx = bcast(e2.nx, src); c2.ny = bcast(e2.ny, src); c2.val0 = bcast(e2.val0, src);
        const int bx = __shfl(begx, src, 64), ex = __shfl(endx, src, 64), by = __shfl(begy, src, 64), ey = __shfl(endy, src, 64);
        for (int yi = by; yi <= ey; ++yi) {
            const float py = (float)yi;
            uint32_t* row = plane + (size_t)yi * P.w32;
            for (int xb = bx & ~63; xb <= ex; xb += 64) {
                const int xi = xb + lane;
                const bool in = xi >= bx && xi <= ex && inside(c0, c1, c2, (float)xi, py);
                const unsigned long long m = __ballot(in);
                // (a set bit lies at x <= ex <= w - 1: a non-zero word is a word of the row)
                if (lane == 0 && (uint32_t)m) atomicOr(row + (xb >> 5), (uint32_t)m);
                if (lane == 32 && (uint32_t)(m >> 32)) atomicOr(row + (xb >> 5) + 1, (uint32_t)(m >> 32));
            }
        }
    }
}

struct ExpandParams {
    const uint32_t* planes;
    const Inst* recs;      // NULL: instance i is image i with label 1 (pvnet_raster_triangles)
    const int32_t* order;  // NULL: list order
    int q, has_inst;       // has_inst 0: no instance at all, zeros
    int h, w, w32, groups; // groups: 16-pixel groups per row
    int vec;               // 16-byte stores possible
    uint8_t* out;
};

// 4 bits -> 4 bytes of 0xFF / 0x00
__device__ __forceinline__ uint32_t spread4(uint32_t b4) { return (((b4 & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu; }

__global__ __launch_bounds__(TPB) void expand_kernel(ExpandParams P) {
    PVNET_SPARE_VGPRS(39);
    __shared__ int s_sorted[PVNET_RASTER_MAX_INSTANCES];   // the image's instances in painter's order: index | label << 16
    __shared__ int s_range[2];
    const int img = blockIdx.y, t = threadIdx.x;
    int first = img, last = img + 1;
    if (P.recs) {
        if (t == 0) {   // the image's stretch of the (non-decreasing) list: two binary searches over at most 768 records
            int lo = 0, hi = P.q;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.recs[mid].image < img) lo = mid + 1; else hi = mid; }
            s_range[0] = lo;
            hi = P.q;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.recs[mid].image <= img) lo = mid + 1; else hi = mid; }
            s_range[1] = lo;
        }
        __syncthreads();
        first = s_range[0];
        last = s_range[1];
        const int m = last - first;
        for (int i = t; i < m; i += TPB) {   // rank by (order, list position)
            int pos = i;
            if (P.order) {
                const int mine = P.order[first + i];
                pos = 0;
                for (int j = 0; j < m; ++j) {
                    const int o = P.order[first + j];
                    pos += (o < mine || (o == mine && j < i)) ? 1 : 0;
                }
            }
            s_sorted[pos] = (first + i) | (P.recs[first + i].label << 16);
        }
        __syncthreads();
    } else if (!P.has_inst) {
        last = first;
    }
    const int g = (int)blockIdx.x * TPB + t;
    if (g >= P.h * P.groups) return;
    const int y = g / P.groups, xg = g - y * P.groups, x = xg * 16;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < last - first; ++k) {
        int idx = first + k;
        uint32_t lab = 1u;
        if (P.recs) {
            const int e = s_sorted[k];
            idx = e & 0xFFFF;
            lab = (uint32_t)e >> 16;
        }
        const uint32_t word = P.planes[((size_t)idx * P.h + y) * P.w32 + (x >> 5)];
        const uint32_t b16 = (word >> (x & 31)) & 0xFFFFu;
        if (!b16) continue;
        const uint32_t l4 = lab * 0x01010101u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t m = spread4(b16 >> (4 * j));
            o[j] = (o[j] & ~m) | (l4 & m);
        }
    }
    uint8_t* dst = P.out + ((size_t)img * P.h + y) * P.w + x;
    if (P.vec) {   // w is a multiple of 16 and `out` 16-byte aligned
        *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {       // byte by byte, and the tail of a row
        const int nb = min(16, P.w - x);
        for (int j = 0; j < nb; ++j) dst[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
    }
}

size_t plane_bytes(int q, int h, int w) {
    const size_t words = (size_t)q * (size_t)h * (size_t)((w + 31) / 32);
    return (words * 4 + 15) / 16 * 16;
}

int last_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int launch_expand(const uint32_t* planes, const Inst* recs, const int32_t* order, int q, int has_inst, int b, int h, int w,
                  uint8_t* out, hipStream_t s) {
    ExpandParams E;
    E.planes = planes; E.recs = recs; E.order = order; E.q = q; E.has_inst = has_inst;
    E.h = h; E.w = w; E.w32 = (w + 31) / 32; E.groups = (w + 15) / 16;
    E.vec = (w % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) ? 1 : 0;
    E.out = out;
    const long long groups = (long long)h * E.groups;
    hipLaunchKernelGGL(expand_kernel, dim3((unsigned)((groups + TPB - 1) / TPB), b), dim3(TPB), 0, s, E);
    return last_error();
}

int clear_blocks_for(size_t n16) { return (int)std::min<size_t>(std::max<size_t>((n16 + TPB - 1) / TPB, 1), 2048); }

}  // namespace
}  // namespace pvd

using namespace pvd;

extern "C" {

int pvnet_raster_abi_version(void) { return PVNET_RASTER_ABI_VERSION; }

size_t pvnet_raster_workspace_bytes(int q, int P, int T, int b, int h, int w) {
    if (q < 0 || P < 0 || T < 0 || b < 0 || h < 2 || w < 2 || h > PVNET_RASTER_MAX_SIDE || w > PVNET_RASTER_MAX_SIDE) return 0;
    return WS_HEAD + sizeof(Inst) * (size_t)q + plane_bytes(q, h, w);
}

int pvnet_raster_triangles(const float* tri, int n, int tn, int h, int w, uint8_t* mask_out, int32_t* status_out, void* ws,
                           size_t ws_bytes, void* stream) {
    int rc = 0;
    if (n < 0 || tn < 0) return PVNET_E_BADARG;
    if ((rc = check_sizes(h, w))) return rc;
    if (n > PVNET_RASTER_MAX_IMAGES) return PVNET_E_UNSUPPORTED;
    if (n == 0) return 0;
    if (!mask_out || !ws || (tn > 0 && !tri)) return PVNET_E_BADARG;
    if (reinterpret_cast<uintptr_t>(ws) & 15u) return PVNET_E_BADARG;
    if (ws_bytes < pvnet_raster_workspace_bytes(n, 0, tn, n, h, w)) return PVNET_E_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    uint32_t* counters = reinterpret_cast<uint32_t*>(base);
    uint32_t* planes = reinterpret_cast<uint32_t*>(base + WS_HEAD + sizeof(Inst) * (size_t)n);
    if (tn == 0) {   // nothing to rasterise: zeros (and a zero status) without touching the planes
        if (status_out) {
            ClearParams C = {nullptr, 0, 1, n, status_out, counters, nullptr, 0, nullptr, nullptr};
            hipLaunchKernelGGL(clear_check_kernel, dim3(1), dim3(TPB), 0, s, C);
            if ((rc = last_error())) return rc;
        }
        return launch_expand(planes, nullptr, nullptr, 0, 0, n, h, w, mask_out, s);
    }
    ClearParams C;
    C.planes = reinterpret_cast<uint4*>(planes);
    C.n16 = plane_bytes(n, h, w) / 16;
    C.clear_blocks = clear_blocks_for(C.n16);
    C.zero_status_n = n; C.status = status_out; C.counters = counters;
    C.recs = nullptr; C.vblocks = 0; C.vertices = nullptr; C.poses = nullptr;
    hipLaunchKernelGGL(clear_check_kernel, dim3(C.clear_blocks), dim3(TPB), 0, s, C);
    if ((rc = last_error())) return rc;
    TriParams Tp;
    Tp.tri = tri; Tp.tn = tn; Tp.recs = nullptr; Tp.vertices = nullptr; Tp.faces = nullptr; Tp.poses = nullptr; Tp.K = nullptr;
    Tp.k_stride = 0; Tp.tri_out = nullptr; Tp.status = status_out; Tp.planes = planes; Tp.counters = counters;
    Tp.h = h; Tp.w = w; Tp.w32 = (w + 31) / 32;
    hipLaunchKernelGGL(triangle_kernel, dim3((tn + TPB - 1) / TPB, n), dim3(TPB), 0, s, Tp);
    if ((rc = last_error())) return rc;
    return launch_expand(planes, nullptr, nullptr, n, 1, n, h, w, mask_out, s);
}

int pvnet_render(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M, int P,
                 int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                 const int32_t* image_id, const int32_t* label, const int32_t* order, int b, int h, int w, uint8_t* out,
                 float* tri_out, int32_t* status_out, void* ws, size_t ws_bytes, void* stream) {
    const Instances S = {vertices, faces, vertex_offset, face_offset, M, P, T, q, mesh_id, poses, K, k_per_instance, image_id, label, b, h, w};
    int rc = 0, max_v, max_f;
    Table tab;
    if ((rc = check_counts(S))) return rc;
    if ((rc = check_tables(S))) return rc;
    if (!out && !tri_out) return PVNET_E_BADARG;
    if ((rc = check_arrays(S))) return rc;
    if ((rc = check_instances(S, &tab, &max_f, &max_v))) return rc;
    if (b == 0) return 0;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return PVNET_E_BADARG;
    if (ws_bytes < pvnet_raster_workspace_bytes(q, P, T, b, h, w)) return PVNET_E_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    uint32_t* counters = reinterpret_cast<uint32_t*>(base);
    Inst* recs = reinterpret_cast<Inst*>(base + WS_HEAD);
    uint32_t* planes = reinterpret_cast<uint32_t*>(base + WS_HEAD + sizeof(Inst) * (size_t)q);
    if (q == 0) return out ? launch_expand(planes, nullptr, nullptr, 0, 0, b, h, w, out, s) : 0;
    hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(1024), 0, s, tab, q, recs, status_out, counters);
    if ((rc = last_error())) return rc;
    ClearParams C;
    C.planes = reinterpret_cast<uint4*>(planes);
    C.n16 = out ? plane_bytes(q, h, w) / 16 : 0;
    C.clear_blocks = out ? clear_blocks_for(C.n16) : 0;
    C.zero_status_n = 0; C.status = status_out; C.counters = counters;
    C.recs = recs; C.vblocks = status_out ? (max_v + TPB - 1) / TPB : 0; C.vertices = vertices; C.poses = poses;
    const long long nblocks = (long long)C.clear_blocks + (long long)q * C.vblocks;
    if (nblocks > 0x7FFFFFFFll) return PVNET_E_UNSUPPORTED;
    if (nblocks > 0) {
        hipLaunchKernelGGL(clear_check_kernel, dim3((unsigned)nblocks), dim3(TPB), 0, s, C);
        if ((rc = last_error())) return rc;
    }
    if (max_f > 0) {
        TriParams Tp;
        Tp.tri = nullptr; Tp.tn = 0; Tp.recs = recs; Tp.vertices = vertices; Tp.faces = faces; Tp.poses = poses; Tp.K = K;
        Tp.k_stride = k_per_instance ? 9 : 0; Tp.tri_out = tri_out; Tp.status = status_out; Tp.planes = out ? planes : nullptr;
        Tp.counters = counters; Tp.h = h; Tp.w = w; Tp.w32 = (w + 31) / 32;
        hipLaunchKernelGGL(triangle_kernel, dim3((max_f + TPB - 1) / TPB, q), dim3(TPB), 0, s, Tp);
        if ((rc = last_error())) return rc;
    }
    return out ? launch_expand(planes, recs, order, q, 1, b, h, w, out, s) : 0;
}

}  // extern "C"
