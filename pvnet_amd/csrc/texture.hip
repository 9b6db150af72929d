// texture.hip -- libpvnet_texture.so: the images of libpvnet_shade.so for meshes that may carry a texture image and per-vertex UV
// coordinates, with the depth, labels and visible pixel counts of libpvnet_depth.so from the same call (include/pvnet_texture.h holds
// THE DEFINITION).
//
// Path replaced (reference tree): the u_use_texture branch of the offline OpenGL renderer (lib/utils/opengl_render_backend.py:68-69,
// 95-96 the shaders' last line, 316-323 and 344-352 the texture and its coordinates).
//
// A COPY of shade.hip's four kernels under this library's names (that library's sources, exports and device code are pinned by its
// tests, and a mesh without a texture must come out of this library exactly as out of that one), with three additions: the setup
// kernel writes the texture of an instance's mesh into the two spare words of its record, the resolve kernel interpolates (u, v)
// with the weights it has and fetches one or four texels, and the host checks the texture table.
//   texture_setup_kernel    one workgroup: the instance table and the textures' sides, which arrive in the launch's arguments,
//                           become records in the workspace (a texture's first texel is the sum of the sizes before it); status,
//                           visible counts and counters zeroed
//   texture_clear_kernel    the z-buffer to bits(far) << 32 | 0xFFFFFFFF with 16-byte stores
//   texture_tri_kernel      the shade library's triangle walk, itself depth_tri_kernel's: a lane alone up to PVNET_TEXTURE_LANE_PIXELS pixels,
//                           the wave across a row beyond; coverage and depth are the functions the other three libraries compile
//                           (mesh_core.h, depth_core.h: the bodies behind mesh_stages.h and depth_plane.h)
//   texture_resolve_kernel  the shade library's resolve layout: four pixels per lane, twelve bytes of background and of colour, 16-byte
//                           depth stores, packed labels, visible counts in LDS with one integer add per workgroup and instance.  A
//                           covered pixel of a textured mesh: u and v by the attribute interpolation, one 4-byte load per texel, the
//                           blend in float64 in the header's order
// Minima and integer sums do not depend on the order in which they land: the call is bitwise reproducible.
//
// Nothing is contracted (FP_CONTRACT OFF), float32 and float64 denormals are kept (the compiler's default for gfx950).
#include <algorithm>
#include <cmath>

#include "vote_common.h"

#include "pvnet_texture.h"
#include "mesh_core.h"    // project, make_edge, same_side, inside: what the raster, depth and shade libraries compile
#include "depth_core.h"   // camera_z, make_plane, pixel_depth: what the depth and shade libraries compile

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

constexpr int TPB = 256;   // lanes per workgroup of every kernel but texture_setup_kernel
constexpr uint32_t NOBODY = 0xFFFFFFFFu;   // the low word of a pixel no kept candidate reached
constexpr int FACE_BITS = 22;
constexpr uint32_t FACE_MASK = (1u << FACE_BITS) - 1u;

struct Inst {   // one instance, as the kernels read it: the shade library's record with its two spare words in use
    int voff, vcnt, foff, fcnt, image, label;
    int toff;        // first texel of its mesh's texture in the table (below 2^31)
    uint32_t dims;   // th << 16 | tw; 0: the mesh has no texture
};
static_assert(sizeof(Inst) == 32, "workspace layout: 16-byte aligned records, the shade library's workspace formula");

// the instance table as it travels in texture_setup_kernel's arguments: mesh (6 bits) | label (8) << 6 | image (18) << 14; per mesh
// the sides of its texture, th << 16 | tw.  (The texel offsets do not travel: they are the running sum of th tw, which the host has
// checked against tex_offset.)
struct Table {
    uint32_t inst[PVNET_TEXTURE_MAX_INSTANCES];
    int32_t voff[PVNET_TEXTURE_MAX_MESHES + 1], foff[PVNET_TEXTURE_MAX_MESHES + 1];
    uint32_t dims[PVNET_TEXTURE_MAX_MESHES];
};
static_assert(sizeof(Table) + 48 <= 4096, "kernel arguments: 4 KB with the rest (an int and four pointers)");
static_assert(PVNET_TEXTURE_MAX_SIDE < (1 << 16), "th << 16 | tw");
static_assert(PVNET_TEXTURE_MAX_MESHES <= 64 && PVNET_TEXTURE_MAX_IMAGES < (1 << 18), "the packing of Table::inst");
static_assert(PVNET_TEXTURE_MAX_INSTANCES < (1 << (32 - FACE_BITS)) - 1, "instance << 22 | face in the low word, below NOBODY");
static_assert(PVNET_TEXTURE_MAX_FACES == (1 << FACE_BITS), "the face index of the low word");

constexpr size_t WS_HEAD = 16;   // counters: [0] triangles that took the cooperative path

__global__ __launch_bounds__(1024) void texture_setup_kernel(Table T, int q, Inst* recs, int32_t* status, int32_t* visible,
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
        r.dims = T.dims[m];
        uint32_t toff = 0u;   // (below 2^31 in all: checked on the host)
        for (int k = 0; k < m; ++k) toff += (T.dims[k] >> 16) * (T.dims[k] & 0xFFFFu);
        r.toff = (int)toff;
        recs[t] = r;
        if (status) status[t] = 0;
        if (visible) visible[t] = 0;
    }
    if (t < 4) counters[t] = 0u;
}

__global__ __launch_bounds__(TPB) void texture_clear_kernel(uint4* zbuf, size_t n16, uint32_t far_bits) {
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

__global__ __launch_bounds__(TPB) void texture_tri_kernel(TriParams P) {
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
            st |= PVNET_TEXTURE_S_BADFACE;
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
                st |= PVNET_TEXTURE_S_BEHIND;
            if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)))
                st |= PVNET_TEXTURE_S_NONFINITE;
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
    // (f < fcnt <= PVNET_TEXTURE_MAX_FACES, checked on the host: the face stays inside its 22 bits)
    const uint32_t low = ((uint32_t)inst << FACE_BITS) | ((uint32_t)f & FACE_MASK);
    const int area = valid ? (endx - begx + 1) * (endy - begy + 1) : 0;   // (at most 32768^2 = 2^30)
    const bool large = area > PVNET_TEXTURE_LANE_PIXELS;

    if (valid && !large) {   // the lane alone: at most PVNET_TEXTURE_LANE_PIXELS pixels
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
        const uint32_t clow = (uint32_t)__shfl((int)low, src, 64);
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

struct ResolveParams {
    const unsigned long long* zbuf;   // NULL: no instance at all, background and zeros
    size_t n;                         // pixels of the call: b h w
    uint32_t hw, w;                   // pixels of one image (at most 2^30), of one row
    unsigned long long hw_magic;      // floor((2^64 - 1) / hw): the high half of p * hw_magic is p / hw or one less
    int q;
    const Inst* recs;
    const double* vertices;
    const int32_t* faces;
    const uint8_t* colors;
    const double* normals;
    const float* uv;                  // [P,2]
    const uint32_t* texels;           // R | G << 8 | B << 16 per texel, the textures of the table one after the other
    const double* poses;
    const double* K;
    int k_stride;                     // 0 or 9
    int filter;
    int shading;
    float ambient;
    uint32_t bg[3];                   // twelve bytes: bg_color four times
    const uint8_t* bg_image;          // or NULL
    uint8_t* rgb;
    float* depth;
    uint8_t* label;
    int32_t* visible;
    int vec_rgb, vec_bg, vec_depth, vec_label;   // 4-byte / 4-byte / 16-byte / 4-byte accesses possible
};

// the camera-space vertex: the c_0, c_1, c_2 of stage P (the same expressions as in project(): the same bits)
__device__ __forceinline__ void camera_point(const double* pose, const double* X, double* c) {
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    c[0] = ((pose[0] * X0 + pose[1] * X1) + pose[2] * X2) + pose[3];
    c[1] = ((pose[4] * X0 + pose[5] * X1) + pose[6] * X2) + pose[7];
    c[2] = ((pose[8] * X0 + pose[9] * X1) + pose[10] * X2) + pose[11];
}

__device__ __forceinline__ double clamp01(double l) {
    if (!(l >= 0.0)) l = 0.0;
    if (l > 1.0) l = 1.0;
    return l;
}

struct Weights {
    double w0, w1, w2, s;
    bool degenerate;
};

__device__ __forceinline__ double attribute(const Weights& W, double a0, double a1, double a2) {
    const double t0 = W.w0 * a0, t1 = W.w1 * a1, t2 = W.w2 * a2;
    const double u = t0 + t1;
    const double v = u + t2;
    const double r = v / W.s;
    return W.degenerate ? a0 : r;
}

__device__ __forceinline__ double dot3(const double* u, const double* v) {
    const double a = u[0] * v[0], b = u[1] * v[1], c = u[2] * v[2];
    const double s = a + b;
    return s + c;
}

// THE DEFINITION's colour of pixel (px, py) under face `face` of instance `inst`: three bytes in the low 24 bits
__device__ __forceinline__ uint32_t textured_pixel(const ResolveParams& P, int inst, int face, int xi, int yi) {
    const Inst r = P.recs[inst];
    const int32_t* fc = P.faces + (size_t)(r.foff + face) * 3;
    const size_t i0 = (size_t)(r.voff + fc[0]), i1 = (size_t)(r.voff + fc[1]), i2 = (size_t)(r.voff + fc[2]);
    const double* pose = P.poses + (size_t)inst * 12;
    const double* K = P.K + (size_t)inst * P.k_stride;
    float fx0, fy0, fx1, fy1, fx2, fy2;
    project(pose, K, P.vertices + i0 * 3, fx0, fy0);
    project(pose, K, P.vertices + i1 * 3, fx1, fy1);
    project(pose, K, P.vertices + i2 * 3, fx2, fy2);
    double C0[3], C1[3], C2[3];
    camera_point(pose, P.vertices + i0 * 3, C0);
    camera_point(pose, P.vertices + i1 * 3, C1);
    camera_point(pose, P.vertices + i2 * 3, C2);
    const double x0 = (double)fx0, y0 = (double)fy0, x1 = (double)fx1, y1 = (double)fy1, x2 = (double)fx2, y2 = (double)fy2;
    const double px = (double)xi, py = (double)yi;
    // screen barycentrics
    const double dx1 = x1 - x0, dy1 = y1 - y0, dx2 = x2 - x0, dy2 = y2 - y0, ex = px - x0, ey = py - y0;
    const double a0 = dx1 * dy2, a1 = dx2 * dy1;
    const double area = a0 - a1;
    const double p0 = ex * dy2, p1 = dx2 * ey;
    const double q0 = dx1 * ey, q1 = ex * dy1;
    double l1 = (p0 - p1) / area;
    double l2 = (q0 - q1) / area;
    const double h0 = 1.0 - l1;
    double l0 = h0 - l2;
    l0 = clamp01(l0);
    l1 = clamp01(l1);
    l2 = clamp01(l2);
    // perspective weights
    Weights W;
    W.w0 = l0 / C0[2];
    W.w1 = l1 / C1[2];
    W.w2 = l2 / C2[2];
    const double s01 = W.w0 + W.w1;
    W.s = s01 + W.w2;
    W.degenerate = area == 0.0 || !(W.s > 0.0);
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = attribute(W, C0[k], C1[k], C2[k]);
    double col[3];
    if (r.dims) {   // a textured mesh: its vertex colours are not read
        const int th = (int)(r.dims >> 16), tw = (int)(r.dims & 0xFFFFu);
        const float *t0 = P.uv + i0 * 2, *t1 = P.uv + i1 * 2, *t2 = P.uv + i2 * 2;
        const double u = clamp01(attribute(W, (double)t0[0], (double)t1[0], (double)t2[0]));
        const double v = clamp01(attribute(W, (double)t0[1], (double)t1[1], (double)t2[1]));
        // (u and v lie in 0 .. 1 and are no NaN: every column below lies in 0 .. tw - 1 and every row in 0 .. th - 1, the texel inside
        // its texture, which the host has checked to lie inside the table; the outer clamps change no value and state that)
        const uint32_t* tex = P.texels + (size_t)r.toff;
        const double su = u * (double)tw, sv = v * (double)th;
        if (P.filter == PVNET_TEXTURE_NEAREST) {
            const int i = max(min((int)floor(su), tw - 1), 0), j = max(min((int)floor(sv), th - 1), 0);
            const uint32_t c = tex[(size_t)(th - 1 - j) * tw + i];
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = (double)((c >> (8 * k)) & 255u);
        } else {
            const double x = su - 0.5, y = sv - 0.5;
            const double fi = floor(x), fj = floor(y);
            const double fx = x - fi, fy = y - fj;
            const int i0t = (int)fi, j0t = (int)fj;
            const int ia = min(max(i0t, 0), tw - 1), ib = max(min(i0t + 1, tw - 1), 0);
            const int ja = min(max(j0t, 0), th - 1), jb = max(min(j0t + 1, th - 1), 0);
            const uint32_t* ra = tex + (size_t)(th - 1 - ja) * tw;
            const uint32_t* rb = tex + (size_t)(th - 1 - jb) * tw;
            const uint32_t caa = ra[ia], cab = ra[ib], cba = rb[ia], cbb = rb[ib];
            const double gx = 1.0 - fx, gy = 1.0 - fy;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double taa = (double)((caa >> (8 * k)) & 255u), tab = (double)((cab >> (8 * k)) & 255u);
                const double tba = (double)((cba >> (8 * k)) & 255u), tbb = (double)((cbb >> (8 * k)) & 255u);
                const double l0t = gx * taa, l1t = fx * tab, h0t = gx * tba, h1t = fx * tbb;
                const double lo = l0t + l1t, hi = h0t + h1t;
                const double m0 = gy * lo, m1 = fy * hi;
                col[k] = m0 + m1;
            }
        }
    } else {
        const uint8_t *k0 = P.colors + i0 * 3, *k1 = P.colors + i1 * 3, *k2 = P.colors + i2 * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = attribute(W, (double)k0[k], (double)k1[k], (double)k2[k]);
    }
    double light = 1.0;
    if (P.shading != PVNET_TEXTURE_SHADING_NONE) {
        const double le = sqrt(dot3(e, e));
        double diffuse;
        if (P.shading == PVNET_TEXTURE_SHADING_FLAT) {
            double a[3], b[3], g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a[k] = C1[k] - C0[k];
                b[k] = C2[k] - C0[k];
            }
            const double g00 = a[1] * b[2], g01 = a[2] * b[1], g10 = a[2] * b[0], g11 = a[0] * b[2], g20 = a[0] * b[1], g21 = a[1] * b[0];
            g[0] = g00 - g01;
            g[1] = g10 - g11;
            g[2] = g20 - g21;
            const double lg = sqrt(dot3(g, g));
            const double d = dot3(e, g);
            const double len = le * lg;
            diffuse = fabs(d) / len;
            if (le == 0.0 || lg == 0.0) diffuse = 0.0;
        } else {
            const double *n0 = P.normals + i0 * 3, *n1 = P.normals + i1 * 3, *n2 = P.normals + i2 * 3;
            double n[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double* R = pose + 4 * k;
                const double m0 = (R[0] * n0[0] + R[1] * n0[1]) + R[2] * n0[2];
                const double m1 = (R[0] * n1[0] + R[1] * n1[1]) + R[2] * n1[2];
                const double m2 = (R[0] * n2[0] + R[1] * n2[1]) + R[2] * n2[2];
                n[k] = attribute(W, m0, m1, m2);
            }
            const double ln = sqrt(dot3(n, n));
            const double d = dot3(e, n);
            const double len = le * ln;
            diffuse = (-d) / len;
            if (!(diffuse > 0.0)) diffuse = 0.0;
            if (le == 0.0 || ln == 0.0) diffuse = 0.0;
        }
        light = (double)P.ambient + diffuse;
        if (!(light < 1.0)) light = 1.0;
    }
    uint32_t out = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double m = light * col[k];
        double v = floor(m + 0.5);
        if (!(v >= 0.0)) v = 0.0;
        if (v > 255.0) v = 255.0;
        out |= (uint32_t)(int)v << (8 * k);
    }
    return out;
}

__global__ __launch_bounds__(TPB) void texture_resolve_kernel(ResolveParams P) {
    PVNET_SPARE_VGPRS(135);
    __shared__ int s_count[PVNET_TEXTURE_MAX_INSTANCES];   // pixels won inside this workgroup, per instance
    __shared__ int s_label[PVNET_TEXTURE_MAX_INSTANCES];   // the instances' labels
    const int t = threadIdx.x;
    const bool counting = P.visible && P.zbuf;
    const bool labelling = P.label && P.zbuf;
    if (counting || labelling) {
        for (int i = t; i < P.q; i += TPB) {
            s_count[i] = 0;
            s_label[i] = P.recs[i].label;
        }
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
        // the twelve bytes of these four pixels, background first: bytes 0 .. 7 in lo, 8 .. 11 in hi
        uint8_t* dst = P.rgb + p * 3;
        unsigned long long lo;
        uint32_t hi;
        if (P.bg_image) {
            const uint8_t* src = P.bg_image + p * 3;
            if (P.vec_bg && np == 4) {   // (p * 3 is a multiple of 12)
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
                lo = (unsigned long long)s4[0] | ((unsigned long long)s4[1] << 32);
                hi = s4[2];
            } else {
                lo = 0ull;
                hi = 0u;
                for (int k = 0; k < np * 3; ++k) {
                    if (k < 8) lo |= (unsigned long long)src[k] << (8 * k);
                    else hi |= (uint32_t)src[k] << (8 * (k - 8));
                }
            }
        } else {
            lo = (unsigned long long)P.bg[0] | ((unsigned long long)P.bg[1] << 32);
            hi = P.bg[2];
        }
        const bool any = (uint32_t)word[0] != NOBODY || (uint32_t)word[1] != NOBODY || (uint32_t)word[2] != NOBODY || (uint32_t)word[3] != NOBODY;
        if (any) {   // the pixel of p within its image; the four may cross a row or an image
            // (no 64-bit division: its expansion is float32 arithmetic with fused operations, which this library's assembly is
            // searched for)
            unsigned long long rest = p - __umul64hi(p, P.hw_magic) * P.hw;
            if (rest >= P.hw) rest -= P.hw;
            uint32_t rem = (uint32_t)rest;
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const uint32_t low = (uint32_t)word[j];
                if (low != NOBODY) {
                    const uint32_t yi = rem / P.w, xi = rem - yi * P.w;
                    const unsigned long long c = textured_pixel(P, (int)(low >> FACE_BITS), (int)(low & FACE_MASK), (int)xi, (int)yi);
                    const int bit = 24 * j;   // byte 3 j of twelve
                    if (j < 2) lo = (lo & ~(0xFFFFFFull << bit)) | (c << bit);
                    else if (j == 3) hi = (hi & 0xFFu) | ((uint32_t)c << 8);
                    else {   // j == 2: bytes 6, 7 in lo, byte 8 in hi
                        lo = (lo & 0x0000FFFFFFFFFFFFull) | (c << 48);
                        hi = (hi & 0xFFFFFF00u) | (uint32_t)(c >> 16);
                    }
                }
                if (++rem == P.hw) rem = 0u;
            }
        }
        if (P.vec_rgb && np == 4) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
            d4[0] = (uint32_t)lo;
            d4[1] = (uint32_t)(lo >> 32);
            d4[2] = hi;
        } else {
            for (int k = 0; k < np * 3; ++k) dst[k] = (uint8_t)(k < 8 ? lo >> (8 * k) : (unsigned long long)(hi >> (8 * (k - 8))));
        }
        float d[4];
        uint32_t labels = 0u;
        int run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t low = (uint32_t)word[j];
            const bool won = low != NOBODY;
            const uint32_t who = low >> FACE_BITS;
            d[j] = won ? __uint_as_float((uint32_t)(word[j] >> 32)) : 0.f;
            if (labelling && won) labels |= ((uint32_t)s_label[who] & 255u) << (8 * j);
            if (counting && won) {   // one LDS add per run of pixels with the same winner
                ++run;
                if (j == 3 || ((uint32_t)word[j + 1 < 4 ? j + 1 : 3] >> FACE_BITS) != who) {   // (NOBODY names instance 1023: nobody)
                    atomicAdd(&s_count[who], run);
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
    if (h > PVNET_TEXTURE_MAX_IMAGE_SIDE || w > PVNET_TEXTURE_MAX_IMAGE_SIDE) { *rc = PVNET_E_UNSUPPORTED; return false; }
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

int pvnet_texture_abi_version(void) { return PVNET_TEXTURE_ABI_VERSION; }

size_t pvnet_texture_workspace_bytes(int q, int P, int T, int b, int h, int w) {
    if (q < 0 || P < 0 || T < 0 || b < 0 || h < 2 || w < 2 || h > PVNET_TEXTURE_MAX_IMAGE_SIDE || w > PVNET_TEXTURE_MAX_IMAGE_SIDE) return 0;
    return WS_HEAD + sizeof(Inst) * (size_t)q + zbuf_bytes(b, h, w);
}

int pvnet_render_textured(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                          int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                          const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, const uint8_t* colors,
                          const double* normals, const float* uv, const uint32_t* texels, const int64_t* tex_offset,
                          const int32_t* tex_h, const int32_t* tex_w, int filter, int shading, float ambient, const uint8_t* bg_color,
                          const uint8_t* bg_image, uint8_t* rgb_out, float* depth_out, uint8_t* label_out, int32_t* visible_out,
                          int32_t* status_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = 0;
    if (M < 1 || P < 0 || T < 0 || q < 0 || b < 0) return PVNET_E_BADARG;
    if (!(far > 0.f)) return PVNET_E_BADARG;   // (NaN too)
    if (filter < PVNET_TEXTURE_NEAREST || filter > PVNET_TEXTURE_BILINEAR) return PVNET_E_BADARG;
    if (shading < PVNET_TEXTURE_SHADING_NONE || shading > PVNET_TEXTURE_SHADING_PHONG) return PVNET_E_BADARG;
    if (!(ambient >= 0.f) || !std::isfinite(ambient)) return PVNET_E_BADARG;   // (NaN too)
    if (!sizes_ok(h, w, &rc)) return rc;
    if (M > PVNET_TEXTURE_MAX_MESHES || q > PVNET_TEXTURE_MAX_INSTANCES || b > PVNET_TEXTURE_MAX_IMAGES) return PVNET_E_UNSUPPORTED;
    if (!vertex_offset || !face_offset) return PVNET_E_BADARG;
    if (vertex_offset[0] != 0 || face_offset[0] != 0 || vertex_offset[M] != P || face_offset[M] != T) return PVNET_E_BADARG;
    for (int m = 0; m < M; ++m)
        if (vertex_offset[m + 1] < vertex_offset[m] || face_offset[m + 1] < face_offset[m]) return PVNET_E_BADARG;
    if (!rgb_out || !bg_color) return PVNET_E_BADARG;
    if (q > 0 && (!mesh_id || !image_id || !label || !poses || !K)) return PVNET_E_BADARG;
    if ((P > 0 && !vertices) || (T > 0 && !faces)) return PVNET_E_BADARG;
    if (shading == PVNET_TEXTURE_SHADING_PHONG && P > 0 && !normals) return PVNET_E_BADARG;
    // the texture table: sides first (what is wrong before what is too large), then the offsets, which must be the running sum
    if (!tex_offset || !tex_h || !tex_w) return PVNET_E_BADARG;
    bool textured = false;
    for (int m = 0; m < M; ++m) {
        if (tex_h[m] < 0 || tex_w[m] < 0 || (tex_h[m] == 0) != (tex_w[m] == 0)) return PVNET_E_BADARG;
        textured = textured || tex_h[m] > 0;
    }
    if (textured && (!uv || !texels)) return PVNET_E_BADARG;
    for (int m = 0; m < M; ++m)
        if (tex_h[m] > PVNET_TEXTURE_MAX_SIDE || tex_w[m] > PVNET_TEXTURE_MAX_SIDE) return PVNET_E_UNSUPPORTED;
    if (tex_offset[0] != 0) return PVNET_E_BADARG;
    for (int m = 0; m < M; ++m)   // (a side is at most 2^14: the product at most 2^28, the sum over 64 meshes at most 2^34)
        if (tex_offset[m + 1] != tex_offset[m] + (int64_t)tex_h[m] * (int64_t)tex_w[m]) return PVNET_E_BADARG;
    if (tex_offset[M] >= (int64_t)1 << 31) return PVNET_E_UNSUPPORTED;
    int max_f = 0;
    Table tab;
    for (int i = 0; i < q; ++i) {
        if (mesh_id[i] < 0 || mesh_id[i] >= M) return PVNET_E_BADARG;
        if (!colors && P > 0 && tex_h[mesh_id[i]] == 0) return PVNET_E_BADARG;   // an untextured mesh is drawn: it needs its colours
        if (label[i] < 1 || label[i] > 255) return PVNET_E_BADARG;
        if (image_id[i] < 0 || image_id[i] >= b || (i > 0 && image_id[i] < image_id[i - 1])) return PVNET_E_BADARG;
        max_f = std::max(max_f, face_offset[mesh_id[i] + 1] - face_offset[mesh_id[i]]);
        tab.inst[i] = (uint32_t)mesh_id[i] | ((uint32_t)label[i] << 6) | ((uint32_t)image_id[i] << 14);
    }
    if (max_f > PVNET_TEXTURE_MAX_FACES) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return PVNET_E_BADARG;
    if (ws_bytes < pvnet_texture_workspace_bytes(q, P, T, b, h, w)) return PVNET_E_WORKSPACE;
    const size_t n = (size_t)b * (size_t)h * (size_t)w;
    const size_t resolve_blocks = ((n + 3) / 4 + TPB - 1) / TPB;
    if (resolve_blocks > 0x7FFFFFFFull) return PVNET_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    uint32_t* counters = reinterpret_cast<uint32_t*>(base);
    Inst* recs = reinterpret_cast<Inst*>(base + WS_HEAD);
    unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(base + WS_HEAD + sizeof(Inst) * (size_t)q);
    ResolveParams R;
    R.zbuf = q > 0 ? zbuf : nullptr; R.n = n; R.hw = (uint32_t)h * (uint32_t)w; R.hw_magic = ~0ull / R.hw; R.w = (uint32_t)w; R.q = q; R.recs = recs;
    R.vertices = vertices; R.faces = faces; R.colors = colors; R.normals = normals; R.uv = uv; R.texels = texels; R.poses = poses; R.K = K;
    R.k_stride = k_per_instance ? 9 : 0; R.filter = filter; R.shading = shading; R.ambient = ambient;
    const uint32_t cr = bg_color[0], cg = bg_color[1], cb = bg_color[2];
    R.bg[0] = cr | (cg << 8) | (cb << 16) | (cr << 24);
    R.bg[1] = cg | (cb << 8) | (cr << 16) | (cg << 24);
    R.bg[2] = cb | (cr << 8) | (cg << 16) | (cb << 24);
    R.bg_image = bg_image; R.rgb = rgb_out; R.depth = depth_out; R.label = label_out; R.visible = visible_out;
    R.vec_rgb = (reinterpret_cast<uintptr_t>(rgb_out) & 3u) == 0 ? 1 : 0;
    R.vec_bg = (reinterpret_cast<uintptr_t>(bg_image) & 3u) == 0 ? 1 : 0;
    R.vec_depth = (reinterpret_cast<uintptr_t>(depth_out) & 15u) == 0 ? 1 : 0;
    R.vec_label = (reinterpret_cast<uintptr_t>(label_out) & 3u) == 0 ? 1 : 0;
    if (q > 0) {
        for (int i = q; i < PVNET_TEXTURE_MAX_INSTANCES; ++i) tab.inst[i] = 0u;
        for (int m = 0; m <= PVNET_TEXTURE_MAX_MESHES; ++m) {
            tab.voff[m] = vertex_offset[std::min(m, M)];
            tab.foff[m] = face_offset[std::min(m, M)];
        }
        for (int m = 0; m < PVNET_TEXTURE_MAX_MESHES; ++m)
            tab.dims[m] = m < M ? ((uint32_t)tex_h[m] << 16) | (uint32_t)tex_w[m] : 0u;
        hipLaunchKernelGGL(texture_setup_kernel, dim3(1), dim3(1024), 0, s, tab, q, recs, status_out, visible_out, counters);
        if ((rc = last_error())) return rc;
        const size_t n16 = zbuf_bytes(b, h, w) / 16;
        const int clear_blocks = (int)std::min<size_t>(std::max<size_t>((n16 + TPB - 1) / TPB, 1), 4096);
        uint32_t far_bits;
        static_assert(sizeof(far_bits) == sizeof(far), "float32");
        __builtin_memcpy(&far_bits, &far, sizeof(far_bits));
        hipLaunchKernelGGL(texture_clear_kernel, dim3(clear_blocks), dim3(TPB), 0, s, reinterpret_cast<uint4*>(zbuf), n16, far_bits);
        if ((rc = last_error())) return rc;
        if (max_f > 0) {
            TriParams Tp;
            Tp.recs = recs; Tp.vertices = vertices; Tp.faces = faces; Tp.poses = poses; Tp.K = K; Tp.k_stride = k_per_instance ? 9 : 0;
            Tp.status = status_out; Tp.zbuf = zbuf; Tp.counters = counters; Tp.far = far; Tp.h = h; Tp.w = w;
            hipLaunchKernelGGL(texture_tri_kernel, dim3((max_f + TPB - 1) / TPB, q), dim3(TPB), 0, s, Tp);
            if ((rc = last_error())) return rc;
        }
    }
    hipLaunchKernelGGL(texture_resolve_kernel, dim3((unsigned)resolve_blocks), dim3(TPB), 0, s, R);
    return last_error();
}

}  // extern "C"
