// depth.hip -- libpvnet_depth.so: depth images, occlusion-correct label images and visible pixel counts of posed meshes
// (include/pvnet_depth.h holds THE DEFINITION).
//
// Path replaced (reference tree): OcclusionLineModDB.get_mask_of_all_objects (lib/utils/data_utils.py:788-826), a loop over the objects
// of one image on the host around an OpenGL depth render, and render_mesh_depth (lib/utils/extend_utils/extend_utils.py:196-213), whose
// native body the reference does not have.
//
// A z-buffer of one 64-bit word per pixel: bits(float32 depth) << 32 | instance << 8 | label.  Depths are positive, so the words order
// like (depth, instance) and one unsigned 64-bit minimum per candidate takes the nearest surface and, at a tie, the earlier instance:
//   depth_setup_kernel    one workgroup: the instance table, which arrives in the launch's arguments, becomes records in the
//                         workspace; status, visible counts and counters zeroed
//   depth_clear_kernel    the z-buffer to bits(far) << 32 | 0xFFFFFFFF with 16-byte stores
//   depth_tri_kernel      one lane per (instance, triangle): stage P for its three vertices and the coverage predicate are the functions
//                         libpvnet_raster.so compiles (raster_common.h); the plane of inverse depth in float64 once per triangle, one
//                         float64 division per covered pixel.  A box of at most PVNET_DEPTH_LANE_PIXELS pixels the lane walks alone;
//                         larger boxes are taken one after the other by the whole wave, lanes across 64 pixels of a row (512 contiguous
//                         bytes of z-buffer).  Per covered pixel: a plain load of the word, nothing more when the candidate is not
//                         smaller (the stored word only ever decreases), else one 64-bit atomic minimum
//   depth_resolve_kernel  four pixels per lane: words -> float32 depth (16-byte stores) and label bytes (4-byte stores); the pixels each
//                         instance won are counted in LDS and leave the workgroup as one integer add per instance present
// Minima and integer sums do not depend on the order in which they land: the call is bitwise reproducible.
//
// Nothing is contracted (FP_CONTRACT OFF), float32 and float64 denormals are kept (the compiler's default for gfx950).
#include <algorithm>

#include "vote_common.h"

#include "pvnet_depth.h"
#include "raster_common.h"   // project, make_edge, same_side, inside: shared with raster.hip
#include "depth_plane.h"     // camera_z, make_plane, pixel_depth: shared with shade.hip

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

constexpr int TPB = 256;   // lanes per workgroup of every kernel but depth_setup_kernel
constexpr uint32_t NOBODY = 0xFFFFFFFFu;   // the low word of a pixel no kept candidate reached

struct Inst {   // one instance, as the kernels read it
    int voff, vcnt, foff, fcnt, image, label, pad0, pad1;
};
static_assert(sizeof(Inst) == 32, "workspace layout");

// the instance table as it travels in depth_setup_kernel's arguments: mesh (6 bits) | label (8) << 6 | image (18) << 14
struct Table {
    uint32_t inst[PVNET_DEPTH_MAX_INSTANCES];
    int32_t voff[PVNET_DEPTH_MAX_MESHES + 1], foff[PVNET_DEPTH_MAX_MESHES + 1];
};
static_assert(sizeof(Table) <= 3800, "kernel arguments: 4 KB with the rest");
static_assert(PVNET_DEPTH_MAX_MESHES <= 64 && PVNET_DEPTH_MAX_IMAGES < (1 << 18), "the packing of Table::inst");
static_assert(PVNET_DEPTH_MAX_INSTANCES <= (1 << 24) - 1, "instance << 8 | label in the low word, below NOBODY");

constexpr size_t WS_HEAD = 16;   // counters: [0] triangles that took the cooperative path

__global__ __launch_bounds__(1024) void depth_setup_kernel(Table T, int q, Inst* recs, int32_t* status, int32_t* visible,
                                                           uint32_t* counters) {
    PVNET_SPARE_VGPRS(31);
    const int t = threadIdx.x;
    if (t < q) {
        const uint32_t e = T.inst[t];
        const int m = (int)(e & 63u);
        Inst r;
        r.voff = T.voff[m];
        r.vcnt = T.voff[m + 1] - r.voff;
        r.foff = T.foff[m];
        r.fcnt = T.foff[m + 1] - r.foff;
        r.label = (int)((e >> 6) & 255u);
        r.image = (int)(e >> 14);
        r.pad0 = r.pad1 = 0;
        recs[t] = r;
        if (status) status[t] = 0;
        if (visible) visible[t] = 0;
    }
    if (t < 4) counters[t] = 0u;
}

__global__ __launch_bounds__(TPB) void depth_clear_kernel(uint4* zbuf, size_t n16, uint32_t far_bits) {
    PVNET_SPARE_VGPRS(31);
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n16; i += stride) zbuf[i] = make_uint4(NOBODY, far_bits, NOBODY, far_bits);
}

struct TriParams {
    const Inst* recs;
    const double* vertices;
    const int32_t* faces;
    const double* poses;
    const double* K;
    int k_stride;       // 0 or 9
    int32_t* status;
    unsigned long long* zbuf;
    uint32_t* counters;
    float far;
    int h, w;
};

// a candidate for one pixel: kept when depth < far; the stored word only ever decreases, so a plain load may rule the atomic out
__device__ __forceinline__ void commit(unsigned long long* word, float depth, float far, uint32_t low) {
    if (!(depth < far)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | low;
    const unsigned long long have = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (key < have) atomicMin(word, key);
}

__device__ __forceinline__ float bcast(float v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ double bcast(double v, int src) { return __shfl(v, src, 64); }

__global__ __launch_bounds__(TPB) void depth_tri_kernel(TriParams P) {
    PVNET_SPARE_VGPRS(103);
    const int inst = blockIdx.y, lane = threadIdx.x & 63;
    const int f = (int)blockIdx.x * TPB + (int)threadIdx.x;
    const Inst r = P.recs[inst];
    bool valid = f < r.fcnt;
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    double z0 = 1.0, z1 = 1.0, z2 = 1.0;
    int st = 0;
    if (valid) {
        const int32_t* fc = P.faces + (size_t)(r.foff + f) * 3;
        const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
        if ((unsigned)i0 >= (unsigned)r.vcnt || (unsigned)i1 >= (unsigned)r.vcnt || (unsigned)i2 >= (unsigned)r.vcnt) {
            st |= PVNET_DEPTH_S_BADFACE;
            valid = false;
        } else {
            const double* pose = P.poses + (size_t)inst * 12;
            const double* K = P.K + (size_t)inst * P.k_stride;
            const double* V = P.vertices + (size_t)r.voff * 3;
            project(pose, K, V + (size_t)i0 * 3, x0, y0);
            project(pose, K, V + (size_t)i1 * 3, x1, y1);
            project(pose, K, V + (size_t)i2 * 3, x2, y2);
            z0 = camera_z(pose, V + (size_t)i0 * 3);
            z1 = camera_z(pose, V + (size_t)i1 * 3);
            z2 = camera_z(pose, V + (size_t)i2 * 3);
            // each condition sets its own bit; either one means the triangle is not drawn
            if (!(isfinite(z0) && isfinite(z1) && isfinite(z2)) || (float)z0 <= 0.f || (float)z1 <= 0.f || (float)z2 <= 0.f)
                st |= PVNET_DEPTH_S_BEHIND;
            if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)))
                st |= PVNET_DEPTH_S_NONFINITE;
            if (st) valid = false;
        }
    }
    if (st && P.status) atomicOr(&P.status[inst], st);
    if (!valid) {   // (keeps the arithmetic below on finite numbers; nothing of it is used)
        x0 = y0 = x1 = y1 = x2 = y2 = 0.f;
        z0 = z1 = z2 = 1.0;
    }

    int begx = 0, endx = -1, begy = 0, endy = -1;
    if (valid) {   // the box of stage R
        const float minx = fmaxf(0.f, fminf(fminf(x0, x1), x2)), maxx = fminf((float)(P.w - 2), fmaxf(fmaxf(x0, x1), x2));
        const float miny = fmaxf(0.f, fminf(fminf(y0, y1), y2)), maxy = fminf((float)(P.h - 2), fmaxf(fmaxf(y0, y1), y2));
        const float ex = maxx + 1.f, ey = maxy + 1.f;
        // the emptiness rule of pvnet_raster.h, in float before any cast
        if (minx >= (float)P.w || ex <= -1.f || miny >= (float)P.h || ey <= -1.f) {
            valid = false;
        } else {
            begx = (int)minx; endx = (int)ex; begy = (int)miny; endy = (int)ey;
            // (what the clamps above already guarantee, stated for the atomics below: no word outside the image)
            begx = max(begx, 0); begy = max(begy, 0); endx = min(endx, P.w - 1); endy = min(endy, P.h - 1);
            valid = begx <= endx && begy <= endy;
        }
    }
    const Edge e0 = make_edge(x0, y0, x1, y1, x2, y2), e1 = make_edge(x1, y1, x2, y2, x0, y0), e2 = make_edge(x2, y2, x0, y0, x1, y1);
    const Plane pl = make_plane(x0, y0, x1, y1, x2, y2, z0, z1, z2);
    unsigned long long* img = P.zbuf + (size_t)r.image * P.h * P.w;
    const uint32_t low = ((uint32_t)inst << 8) | (uint32_t)r.label;
    const int area = valid ? (endx - begx + 1) * (endy - begy + 1) : 0;   // (at most 32768^2 = 2^30)
    const bool large = area > PVNET_DEPTH_LANE_PIXELS;

    if (valid && !large) {   // the lane alone: at most PVNET_DEPTH_LANE_PIXELS pixels
        for (int yi = begy; yi <= endy; ++yi) {
            const float py = (float)yi;
            unsigned long long* row = img + (size_t)yi * P.w;
            for (int xi = begx; xi <= endx; ++xi) {
                const float px = (float)xi;
                if (inside(e0, e1, e2, px, py)) commit(row + xi, pixel_depth(pl, px, py), P.far, low);
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
        Plane cp;
        cp.x0 = bcast(pl.x0, src); cp.y0 = bcast(pl.y0, src); cp.i0 = bcast(pl.i0, src); cp.b = bcast(pl.b, src); cp.c = bcast(pl.c, src);
        cp.zmin = bcast(pl.zmin, src); cp.zmax = bcast(pl.zmax, src); cp.flat = __shfl(pl.flat, src, 64);
        const int bx = __shfl(begx, src, 64), ex = __shfl(endx, src, 64), by = __shfl(begy, src, 64), ey = __shfl(endy, src, 64);
        for (int yi = by; yi <= ey; ++yi) {
            const float py = (float)yi;
            unsigned long long* row = img + (size_t)yi * P.w;
            for (int xb = bx & ~63; xb <= ex; xb += 64) {
                const int xi = xb + lane;
                // (xi <= ex <= w - 1: the word is a word of the row)
                if (xi >= bx && xi <= ex && inside(c0, c1, c2, (float)xi, py)) commit(row + xi, pixel_depth(cp, (float)xi, py), P.far, low);
            }
        }
    }
}

struct ResolveParams {
    const unsigned long long* zbuf;   // NULL: no instance at all, zeros
    size_t n;                         // pixels of the call: b h w
    int q;
    float* depth;
    uint8_t* label;
    int32_t* visible;
    int vec_depth, vec_label;         // 16-byte / 4-byte stores possible
};

__global__ __launch_bounds__(TPB) void depth_resolve_kernel(ResolveParams P) {
    PVNET_SPARE_VGPRS(31);
    __shared__ int s_count[PVNET_DEPTH_MAX_INSTANCES];   // pixels won inside this workgroup, per instance
    const int t = threadIdx.x;
    const bool counting = P.visible && P.zbuf;
    if (counting) {
        for (int i = t; i < P.q; i += TPB) s_count[i] = 0;
        __syncthreads();
    }
    const size_t p = ((size_t)blockIdx.x * TPB + t) * 4;
    if (p < P.n) {
        const int np = (int)std::min<size_t>(4, P.n - p);
        unsigned long long word[4] = {NOBODY, NOBODY, NOBODY, NOBODY};
        if (P.zbuf) {
            if (np == 4) {   // p is a multiple of 4 and the z-buffer 16-byte aligned
                const uint4 a = *reinterpret_cast<const uint4*>(P.zbuf + p), b = *reinterpret_cast<const uint4*>(P.zbuf + p + 2);
                word[0] = ((unsigned long long)a.y << 32) | a.x; word[1] = ((unsigned long long)a.w << 32) | a.z;
                word[2] = ((unsigned long long)b.y << 32) | b.x; word[3] = ((unsigned long long)b.w << 32) | b.z;
            } else {
                for (int j = 0; j < np; ++j) word[j] = P.zbuf[p + j];
            }
        }
        float d[4];
        uint32_t labels = 0u;
        int run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t low = (uint32_t)word[j];
            const bool won = low != NOBODY;
            d[j] = won ? __uint_as_float((uint32_t)(word[j] >> 32)) : 0.f;
            labels |= won ? (low & 255u) << (8 * j) : 0u;
            if (counting && won) {   // one LDS add per run of pixels with the same winner
                ++run;
                if (j == 3 || (uint32_t)word[j + 1 < 4 ? j + 1 : 3] != low) {
                    atomicAdd(&s_count[low >> 8], run);
                    run = 0;
                }
            }
        }
        if (P.depth) {
            if (P.vec_depth && np == 4) *reinterpret_cast<float4*>(P.depth + p) = make_float4(d[0], d[1], d[2], d[3]);
            else for (int j = 0; j < np; ++j) P.depth[p + j] = d[j];
        }
        if (P.label) {
            if (P.vec_label && np == 4) *reinterpret_cast<uint32_t*>(P.label + p) = labels;
            else for (int j = 0; j < np; ++j) P.label[p + j] = (uint8_t)(labels >> (8 * j));
        }
    }
    if (counting) {
        __syncthreads();
        for (int i = t; i < P.q; i += TPB) {
            const int c = s_count[i];
            if (c) atomicAdd(&P.visible[i], c);
        }
    }
}

bool sizes_ok(int h, int w, int* rc) {
    if (h < 2 || w < 2) { *rc = PVNET_E_BADARG; return false; }
    if (h > PVNET_DEPTH_MAX_SIDE || w > PVNET_DEPTH_MAX_SIDE) { *rc = PVNET_E_UNSUPPORTED; return false; }
    return true;
}

size_t zbuf_bytes(int b, int h, int w) { return ((size_t)b * (size_t)h * (size_t)w * 8 + 15) / 16 * 16; }

int last_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace
}  // namespace pvd

using namespace pvd;

extern "C" {

int pvnet_depth_abi_version(void) { return PVNET_DEPTH_ABI_VERSION; }

size_t pvnet_depth_workspace_bytes(int q, int P, int T, int b, int h, int w) {
    if (q < 0 || P < 0 || T < 0 || b < 0 || h < 2 || w < 2 || h > PVNET_DEPTH_MAX_SIDE || w > PVNET_DEPTH_MAX_SIDE) return 0;
    return WS_HEAD + sizeof(Inst) * (size_t)q + zbuf_bytes(b, h, w);
}

int pvnet_render_depth(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                       int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                       const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, float* depth_out,
                       uint8_t* label_out, int32_t* visible_out, int32_t* status_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = 0;
    if (M < 1 || P < 0 || T < 0 || q < 0 || b < 0) return PVNET_E_BADARG;
    if (!(far > 0.f)) return PVNET_E_BADARG;   // (NaN too)
    if (!sizes_ok(h, w, &rc)) return rc;
    if (M > PVNET_DEPTH_MAX_MESHES || q > PVNET_DEPTH_MAX_INSTANCES || b > PVNET_DEPTH_MAX_IMAGES) return PVNET_E_UNSUPPORTED;
    if (!vertex_offset || !face_offset) return PVNET_E_BADARG;
    if (vertex_offset[0] != 0 || face_offset[0] != 0 || vertex_offset[M] != P || face_offset[M] != T) return PVNET_E_BADARG;
    for (int m = 0; m < M; ++m)
        if (vertex_offset[m + 1] < vertex_offset[m] || face_offset[m + 1] < face_offset[m]) return PVNET_E_BADARG;
    if (!depth_out && !label_out) return PVNET_E_BADARG;
    if (q > 0 && (!mesh_id || !image_id || !label || !poses || !K)) return PVNET_E_BADARG;
    if ((P > 0 && !vertices) || (T > 0 && !faces)) return PVNET_E_BADARG;
    int max_f = 0;
    Table tab;
    for (int i = 0; i < q; ++i) {
        if (mesh_id[i] < 0 || mesh_id[i] >= M) return PVNET_E_BADARG;
        if (label[i] < 1 || label[i] > 255) return PVNET_E_BADARG;
        if (image_id[i] < 0 || image_id[i] >= b || (i > 0 && image_id[i] < image_id[i - 1])) return PVNET_E_BADARG;
        max_f = std::max(max_f, face_offset[mesh_id[i] + 1] - face_offset[mesh_id[i]]);
        tab.inst[i] = (uint32_t)mesh_id[i] | ((uint32_t)label[i] << 6) | ((uint32_t)image_id[i] << 14);
    }
    if (b == 0) return 0;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return PVNET_E_BADARG;
    if (ws_bytes < pvnet_depth_workspace_bytes(q, P, T, b, h, w)) return PVNET_E_WORKSPACE;
    const size_t n = (size_t)b * (size_t)h * (size_t)w;
    const size_t resolve_blocks = ((n + 3) / 4 + TPB - 1) / TPB;
    if (resolve_blocks > 0x7FFFFFFFull) return PVNET_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    uint32_t* counters = reinterpret_cast<uint32_t*>(base);
    Inst* recs = reinterpret_cast<Inst*>(base + WS_HEAD);
    unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(base + WS_HEAD + sizeof(Inst) * (size_t)q);
    ResolveParams R;
    R.zbuf = q > 0 ? zbuf : nullptr; R.n = n; R.q = q; R.depth = depth_out; R.label = label_out; R.visible = visible_out;
    R.vec_depth = (reinterpret_cast<uintptr_t>(depth_out) & 15u) == 0 ? 1 : 0;
    R.vec_label = (reinterpret_cast<uintptr_t>(label_out) & 3u) == 0 ? 1 : 0;
    if (q > 0) {
        for (int i = q; i < PVNET_DEPTH_MAX_INSTANCES; ++i) tab.inst[i] = 0u;
        for (int m = 0; m <= PVNET_DEPTH_MAX_MESHES; ++m) {
            tab.voff[m] = vertex_offset[std::min(m, M)];
            tab.foff[m] = face_offset[std::min(m, M)];
        }
        hipLaunchKernelGGL(depth_setup_kernel, dim3(1), dim3(1024), 0, s, tab, q, recs, status_out, visible_out, counters);
        if ((rc = last_error())) return rc;
        const size_t n16 = zbuf_bytes(b, h, w) / 16;
        const int clear_blocks = (int)std::min<size_t>(std::max<size_t>((n16 + TPB - 1) / TPB, 1), 4096);
        uint32_t far_bits;
        static_assert(sizeof(far_bits) == sizeof(far), "float32");
        __builtin_memcpy(&far_bits, &far, sizeof(far_bits));
        hipLaunchKernelGGL(depth_clear_kernel, dim3(clear_blocks), dim3(TPB), 0, s, reinterpret_cast<uint4*>(zbuf), n16, far_bits);
        if ((rc = last_error())) return rc;
        if (max_f > 0) {
            TriParams Tp;
            Tp.recs = recs; Tp.vertices = vertices; Tp.faces = faces; Tp.poses = poses; Tp.K = K; Tp.k_stride = k_per_instance ? 9 : 0;
            Tp.status = status_out; Tp.zbuf = zbuf; Tp.counters = counters; Tp.far = far; Tp.h = h; Tp.w = w;
            hipLaunchKernelGGL(depth_tri_kernel, dim3((max_f + TPB - 1) / TPB, q), dim3(TPB), 0, s, Tp);
            if ((rc = last_error())) return rc;
        }
    }
    hipLaunchKernelGGL(depth_resolve_kernel, dim3((unsigned)resolve_blocks), dim3(TPB), 0, s, R);
    return last_error();
}

}  // extern "C"
