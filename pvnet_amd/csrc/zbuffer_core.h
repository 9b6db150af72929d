// zbuffer_core.h -- the ONE copy of the z-buffer that depth.hip (libpvnet_depth.so), shade.hip (libpvnet_shade.so) and texture.hip
// (libpvnet_texture.so) render through: one 64-bit word per pixel, bits(float32 depth) << 32 | low word.  Depths are positive, so one
// unsigned 64-bit minimum per candidate takes the nearest surface and, at a tie, the smaller low word.  Here are the records and the
// setup body, the clear body, commit and the triangle walk, and the host side: the validation of the argument list the three entry
// points share, the workspace formula and the launch sequence.  (The resolve kernels are two: depth.hip's own, and the body that
// shade.hip and texture.hip share in pixel_color.h.)  The three translation units keep their __global__ wrappers (a kernel's name, __launch_bounds__ and PVNET_SPARE_VGPRS
// value), what is particular to them and their extern "C" functions; each includes its public header before this one (the PVNET_E_*
// codes) and states with PVNET_ZBUFFER_CONSTANTS_ARE that its header's limits and bits are the ones below.
//
// What differs between the libraries in the walk is the low word (LabelWord, FaceWord).
//
// Nothing here may be contracted into a fused multiply-add; float32 and float64 denormals are kept (the compiler's default for gfx950).
#ifndef PVNET_ZBUFFER_CORE_H_
#define PVNET_ZBUFFER_CORE_H_

#include <algorithm>

#include "vote_common.h"
#include "mesh_core.h"    // project, make_edge, same_side, inside: what libpvnet_raster.so compiles too
#include "depth_core.h"   // camera_z, make_plane, pixel_depth

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

// the limits and the status bits: equal in include/pvnet_depth.h, pvnet_shade.h and pvnet_texture.h under their own prefixes
constexpr int LANE_PIXELS = 64;   // (MAX_INSTANCES, MAX_MESHES, MAX_IMAGES, MAX_IMAGE_SIDE: mesh_core.h)
constexpr int S_NONFINITE = 1, S_BEHIND = 2, S_BADFACE = 4;
#define PVNET_ZBUFFER_CONSTANTS_ARE(PREFIX, SIDE)                                                                                       \
    static_assert(PREFIX##LANE_PIXELS == pvd::LANE_PIXELS && PREFIX##MAX_INSTANCES == pvd::MAX_INSTANCES &&                            \
                      PREFIX##MAX_MESHES == pvd::MAX_MESHES && PREFIX##MAX_IMAGES == pvd::MAX_IMAGES &&                                \
                      PREFIX##SIDE == pvd::MAX_IMAGE_SIDE && PREFIX##S_NONFINITE == pvd::S_NONFINITE &&                                \
                      PREFIX##S_BEHIND == pvd::S_BEHIND && PREFIX##S_BADFACE == pvd::S_BADFACE && PREFIX##WS_COOP_COUNT_OFFSET == 0,   \
                  "zbuffer_core.h is written in this public header's constants")

constexpr int TPB = 256;   // lanes per workgroup of every kernel but the setup kernels
constexpr uint32_t NOBODY = 0xFFFFFFFFu;   // the low word of a pixel no kept candidate reached
constexpr int FACE_BITS = 22;
constexpr uint32_t FACE_MASK = (1u << FACE_BITS) - 1u;
constexpr int MAX_FACES = 1 << FACE_BITS;   // of one mesh, where the low word names the face

struct Inst {   // one instance, as the kernels read it
    int voff, vcnt, foff, fcnt, image, label;
    int toff;        // the texture library's two words, zero elsewhere: first texel of its mesh's texture in the table (below 2^31)
    uint32_t dims;   // th << 16 | tw; 0: the mesh has no texture
};
static_assert(sizeof(Inst) == 32, "workspace layout: 16-byte aligned records");

constexpr size_t WS_HEAD = 16;   // counters: [0] triangles that took the cooperative path

// the low word.  LabelWord (depth): instance << 8 | label, the same for every triangle of an instance, so the words order like
// (depth, instance) and the resolve kernel reads the label from the word.  FaceWord (shade, texture): instance << 22 | face, the
// words order like (depth, instance, face), the winner of a pixel names the face to colour and the label comes from the record.
struct LabelWord {
    static constexpr bool PER_FACE = false;
    static __device__ __forceinline__ uint32_t make(int inst, const Inst& r, int) { return ((uint32_t)inst << 8) | (uint32_t)r.label; }
};
static_assert(MAX_INSTANCES <= (1 << 24) - 1, "instance << 8 | label in the low word, below NOBODY");
struct FaceWord {
    static constexpr bool PER_FACE = true;
    // (f < fcnt <= MAX_FACES, checked on the host: the face stays inside its 22 bits)
    static __device__ __forceinline__ uint32_t make(int inst, const Inst&, int f) {
        return ((uint32_t)inst << FACE_BITS) | ((uint32_t)f & FACE_MASK);
    }
    static __device__ __forceinline__ uint32_t instance(uint32_t low) { return low >> FACE_BITS; }
    static __device__ __forceinline__ bool same_instance(uint32_t a, uint32_t b) {   // (NOBODY names instance 1023: nobody)
        return (a >> FACE_BITS) == (b >> FACE_BITS);
    }
};
static_assert(MAX_INSTANCES < (1 << (32 - FACE_BITS)) - 1, "instance << 22 | face in the low word, below NOBODY");

struct NoTexture {   // the two spare words of a record where no mesh has a texture
    __device__ __forceinline__ void operator()(int, Inst& r) const {
        r.toff = 0;
        r.dims = 0u;
    }
};

// one workgroup of 1024: the instance table becomes records in the workspace; status, visible counts and counters zeroed.
// texture(m, r) fills the record's two spare words for mesh m.
template <class Texture>
__device__ __forceinline__ void setup_body(const Table& T, int q, Inst* recs, int32_t* status, int32_t* visible, uint32_t* counters,
                                           Texture texture) {
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
        texture(m, r);
        recs[t] = r;
        if (status) status[t] = 0;
        if (visible) visible[t] = 0;
    }
    if (t < 4) counters[t] = 0u;
}

// the z-buffer to bits(far) << 32 | 0xFFFFFFFF with 16-byte stores
__device__ __forceinline__ void clear_body(uint4* zbuf, size_t n16, uint32_t far_bits) {
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

// one lane per (instance, triangle): stage P for its three vertices and the coverage predicate of mesh_core.h, the plane of inverse
// depth of depth_core.h in float64 once per triangle, one float64 division per covered pixel.  A box of at most LANE_PIXELS pixels the
// lane walks alone; larger boxes are taken one after the other by the whole wave, lanes across 64 pixels of a row (512 contiguous
// bytes of z-buffer).  Per covered pixel: a plain load of the word, nothing more when the candidate is not smaller, else one 64-bit
// atomic minimum.  A low word that is the same for the whole wave (Word::PER_FACE false) is not broadcast.
template <class Word>
__device__ __forceinline__ void tri_body(const TriParams& P) {
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
            st |= S_BADFACE;
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
                st |= S_BEHIND;
            if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)))
                st |= S_NONFINITE;
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
    const uint32_t low = Word::make(inst, r, f);
    const int area = valid ? (endx - begx + 1) * (endy - begy + 1) : 0;   // (at most 32768^2 = 2^30)
    const bool large = area > LANE_PIXELS;

    if (valid && !large) {   // the lane alone: at most LANE_PIXELS pixels
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
        uint32_t clow = low;
        if constexpr (Word::PER_FACE) clow = (uint32_t)__shfl((int)low, src, 64);
        for (int yi = by; yi <= ey; ++yi) {
            const float py = (float)yi;
            unsigned long long* row = img + (size_t)yi * P.w;
            for (int xb = bx & ~63; xb <= ex; xb += 64) {
                const int xi = xb + lane;
                // (xi <= ex <= w - 1: the word is a word of the row)
                if (xi >= bx && xi <= ex && inside(c0, c1, c2, (float)xi, py)) commit(row + xi, pixel_depth(cp, (float)xi, py), P.far, clow);
            }
        }
    }
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------

struct Scene : Instances { float far; };   // the argument list the three entry points share

size_t zbuf_bytes(int b, int h, int w) { return ((size_t)b * (size_t)h * (size_t)w * 8 + 15) / 16 * 16; }

// one workspace formula: 0 for sizes no call accepts
size_t workspace_bytes(int q, int P, int T, int b, int h, int w) {
    if (q < 0 || P < 0 || T < 0 || b < 0 || h < 2 || w < 2 || h > MAX_IMAGE_SIDE || w > MAX_IMAGE_SIDE) return 0;
    return WS_HEAD + sizeof(Inst) * (size_t)q + zbuf_bytes(b, h, w);
}

int last_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// mesh_core.h's validation through the arrays, far in its place: 0 or the code.  A library's checks of its own scalars (all
// PVNET_E_BADARG) go before this call, those of its own arrays and outputs between this call and check_instances.
int check_scene(const Scene& S) {
    int rc;
    if ((rc = check_counts(S))) return rc;
    if (!(S.far > 0.f)) return PVNET_E_BADARG;   // (NaN too)
    if ((rc = check_tables(S))) return rc;
    return check_arrays(S);
}

// Last the workspace and the size of the resolve grid (b > 0): the workspace's parts
struct Workspace {
    uint32_t* counters;
    Inst* recs;
    unsigned long long* zbuf;
    unsigned resolve_blocks;
};

int check_workspace(const Scene& S, void* ws, size_t ws_bytes, Workspace* W) {
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return PVNET_E_BADARG;
    if (ws_bytes < workspace_bytes(S.q, S.P, S.T, S.b, S.h, S.w)) return PVNET_E_WORKSPACE;
    const size_t blocks = (((size_t)S.b * (size_t)S.h * (size_t)S.w + 3) / 4 + TPB - 1) / TPB;
    if (blocks > 0x7FFFFFFFull) return PVNET_E_UNSUPPORTED;
    char* base = static_cast<char*>(ws);
    W->counters = reinterpret_cast<uint32_t*>(base);
    W->recs = reinterpret_cast<Inst*>(base + WS_HEAD);
    W->zbuf = reinterpret_cast<unsigned long long*>(base + WS_HEAD + sizeof(Inst) * (size_t)S.q);
    W->resolve_blocks = (unsigned)blocks;
    return 0;
}

// the fields of a resolve kernel's arguments that every resolve kernel reads
template <class Params>
void resolve_outputs(Params& R, const Scene& S, const Workspace& W, float* depth_out, uint8_t* label_out, int32_t* visible_out) {
    R.zbuf = S.q > 0 ? W.zbuf : nullptr; R.n = (size_t)S.b * (size_t)S.h * (size_t)S.w; R.q = S.q;
    R.depth = depth_out; R.label = label_out; R.visible = visible_out;
    R.vec_depth = (reinterpret_cast<uintptr_t>(depth_out) & 15u) == 0 ? 1 : 0;
    R.vec_label = (reinterpret_cast<uintptr_t>(label_out) & 3u) == 0 ? 1 : 0;
}

// The launch sequence: setup, clear and the triangle walk when there is an instance, then the resolve kernel; all on `stream`
template <class SetupTable, class Params>
int launch(const Scene& S, const Workspace& W, int max_f, int32_t* status_out, int32_t* visible_out, void* stream,
           void (*setup)(SetupTable, int, Inst*, int32_t*, int32_t*, uint32_t*), const SetupTable& tab,
           void (*clear)(uint4*, size_t, uint32_t), void (*tri)(TriParams), void (*resolve)(Params), const Params& R) {
    int rc = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (S.q > 0) {
        hipLaunchKernelGGL(setup, dim3(1), dim3(1024), 0, s, tab, S.q, W.recs, status_out, visible_out, W.counters);
        if ((rc = last_error())) return rc;
        const size_t n16 = zbuf_bytes(S.b, S.h, S.w) / 16;
        const int clear_blocks = (int)std::min<size_t>(std::max<size_t>((n16 + TPB - 1) / TPB, 1), 4096);
        uint32_t far_bits;
        static_assert(sizeof(far_bits) == sizeof(S.far), "float32");
        __builtin_memcpy(&far_bits, &S.far, sizeof(far_bits));
        hipLaunchKernelGGL(clear, dim3(clear_blocks), dim3(TPB), 0, s, reinterpret_cast<uint4*>(W.zbuf), n16, far_bits);
        if ((rc = last_error())) return rc;
        if (max_f > 0) {
            TriParams Tp;
            Tp.recs = W.recs; Tp.vertices = S.vertices; Tp.faces = S.faces; Tp.poses = S.poses; Tp.K = S.K;
            Tp.k_stride = S.k_per_instance ? 9 : 0; Tp.status = status_out; Tp.zbuf = W.zbuf; Tp.counters = W.counters; Tp.far = S.far;
            Tp.h = S.h; Tp.w = S.w;
            hipLaunchKernelGGL(tri, dim3((max_f + TPB - 1) / TPB, S.q), dim3(TPB), 0, s, Tp);
            if ((rc = last_error())) return rc;
        }
    }
    hipLaunchKernelGGL(resolve, dim3(W.resolve_blocks), dim3(TPB), 0, s, R);
    return last_error();
}

}  // namespace
}  // namespace pvd
#endif  // PVNET_ZBUFFER_CORE_H_
