// pixel_color.h -- the ONE copy of the colour of a covered pixel (include/pvnet_shade.h and include/pvnet_texture.h, THE DEFINITION) and
// of the resolve kernel that writes it, with the depth, labels and visible counts, compiled by shade.hip (libpvnet_shade.so) and texture.hip
// (libpvnet_texture.so): a mesh without a texture comes out of the texture library exactly as out of the shade library because both
// evaluate these functions.  The z-buffer they read is zbuffer_core.h's, with FaceWord as its low word.
//
// A covered word: the face's three vertices projected again (float32 screen vertices, float64 camera-space vertices), the definition
// evaluated in float64, three bytes.  The colour source of a textured mesh (u and v by the attribute interpolation, one 4-byte load per
// texel, the blend in float64 in the header's order) is compiled only where the kernel's arguments say TEXTURED.
//
// Params, the resolve kernel's arguments, stay with each library (the shade library's do not carry the texture's fields): beside the
// fields of zbuffer_core.h's resolve_outputs() those that color_arguments() fills, and, where TEXTURED, uv, texels and filter.
//
// Nothing here may be contracted into a fused multiply-add; float64 denormals are kept (the compiler's default for gfx950).
#ifndef PVNET_PIXEL_COLOR_H_
#define PVNET_PIXEL_COLOR_H_

#include <cmath>

#include "zbuffer_core.h"

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

// equal in include/pvnet_shade.h (PVNET_SHADE_NONE ...) and include/pvnet_texture.h (PVNET_TEXTURE_SHADING_NONE ...)
constexpr int SHADING_NONE = 0, SHADING_FLAT = 1, SHADING_PHONG = 2;
#define PVNET_SHADING_CONSTANTS_ARE(PREFIX)                                                                                       \
    static_assert(PREFIX##NONE == pvd::SHADING_NONE && PREFIX##FLAT == pvd::SHADING_FLAT && PREFIX##PHONG == pvd::SHADING_PHONG, \
                  "pixel_color.h is written in this public header's constants")
constexpr int FILTER_NEAREST = 0, FILTER_BILINEAR = 1;   // PVNET_TEXTURE_NEAREST, PVNET_TEXTURE_BILINEAR

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

// the colour source of a mesh without a texture: the interpolated vertex colours
template <class Params>
__device__ __forceinline__ void vertex_color(const Params& P, const Weights& W, size_t i0, size_t i1, size_t i2, double* col) {
    const uint8_t *k0 = P.colors + i0 * 3, *k1 = P.colors + i1 * 3, *k2 = P.colors + i2 * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k] = attribute(W, (double)k0[k], (double)k1[k], (double)k2[k]);
}

// the colour source of a textured mesh (r.dims != 0): its vertex colours are not read
template <class Params>
__device__ __forceinline__ void texel_color(const Params& P, const Inst& r, const Weights& W, size_t i0, size_t i1, size_t i2, double* col) {
    const int th = (int)(r.dims >> 16), tw = (int)(r.dims & 0xFFFFu);
    const float *t0 = P.uv + i0 * 2, *t1 = P.uv + i1 * 2, *t2 = P.uv + i2 * 2;
    const double u = clamp01(attribute(W, (double)t0[0], (double)t1[0], (double)t2[0]));
    const double v = clamp01(attribute(W, (double)t0[1], (double)t1[1], (double)t2[1]));
    // (u and v lie in 0 .. 1 and are no NaN: every column below lies in 0 .. tw - 1 and every row in 0 .. th - 1, the texel inside
    // its texture, which the host has checked to lie inside the table; the outer clamps change no value and state that)
    const uint32_t* tex = P.texels + (size_t)r.toff;
    const double su = u * (double)tw, sv = v * (double)th;
    if (P.filter == FILTER_NEAREST) {
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
}

// THE DEFINITION's colour of pixel (px, py) under face `face` of instance `inst`: three bytes in the low 24 bits
template <class Params>
__device__ __forceinline__ uint32_t pixel_color(const Params& P, int inst, int face, int xi, int yi) {
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
    if constexpr (Params::TEXTURED) {
        if (r.dims) texel_color(P, r, W, i0, i1, i2, col);
        else vertex_color(P, W, i0, i1, i2, col);
    } else {
        vertex_color(P, W, i0, i1, i2, col);
    }
    double light = 1.0;
    if (P.shading != SHADING_NONE) {
        const double le = sqrt(dot3(e, e));
        double diffuse;
        if (P.shading == SHADING_FLAT) {
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

// The twelve bytes of the four pixels from p on, of which np exist: the background, copied or constant, then the colour of every pixel
// whose word names a face.
template <class Params>
__device__ __forceinline__ void resolve_rgb(const Params& P, size_t p, int np, const unsigned long long* word) {
    // background first: bytes 0 .. 7 in lo, 8 .. 11 in hi
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
        // (no 64-bit division: its expansion is float32 arithmetic with fused operations, which these libraries' assembly is
        // searched for)
        unsigned long long rest = p - __umul64hi(p, P.hw_magic) * P.hw;
        if (rest >= P.hw) rest -= P.hw;
        uint32_t rem = (uint32_t)rest;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const uint32_t low = (uint32_t)word[j];
            if (low != NOBODY) {
                const uint32_t yi = rem / P.w, xi = rem - yi * P.w;
                const unsigned long long c = pixel_color(P, (int)(low >> FACE_BITS), (int)(low & FACE_MASK), (int)xi, (int)yi);
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
}

// The resolve kernel of the two colour libraries, four pixels per lane: the twelve bytes of resolve_rgb(), then, as in
// depth_resolve_kernel, words -> float32 depth (16-byte stores) and label bytes (4-byte stores, the labels from the records through LDS:
// the word names a face, not a label); the pixels each instance won are counted in LDS and leave the workgroup as one integer add per
// instance present.  P: the library's kernel arguments.
template <class Params>
__device__ __forceinline__ void resolve_body(const Params& P) {
    __shared__ int s_count[MAX_INSTANCES];   // pixels won inside this workgroup, per instance
    __shared__ int s_label[MAX_INSTANCES];   // the instances' labels
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
        resolve_rgb(P, p, np, word);
        float d[4];
        uint32_t labels = 0u;
        int run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t low = (uint32_t)word[j];
            const bool won = low != NOBODY;
            const uint32_t who = FaceWord::instance(low);
            d[j] = won ? __uint_as_float((uint32_t)(word[j] >> 32)) : 0.f;
            if (labelling && won) labels |= ((uint32_t)s_label[who] & 255u) << (8 * j);
            if (counting && won) {   // one LDS add per run of pixels with the same winner
                ++run;
                if (j == 3 || !FaceWord::same_instance((uint32_t)word[j + 1 < 4 ? j + 1 : 3], low)) {
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

// ---- the host side ----------------------------------------------------------------------------------------------------------------------

// the scalars of the shading, checked before zbuffer_core.h's check_scene()
int check_shading(int shading, float ambient) {
    if (shading < SHADING_NONE || shading > SHADING_PHONG) return PVNET_E_BADARG;
    if (!(ambient >= 0.f) || !std::isfinite(ambient)) return PVNET_E_BADARG;   // (NaN too)
    return 0;
}

// the fields of a resolve kernel's arguments that resolve_rgb() and pixel_color() read, but the texture's
template <class Params>
void color_arguments(Params& R, const Scene& S, const Workspace& W, const uint8_t* colors, const double* normals, int shading, float ambient,
                     const uint8_t* bg_color, const uint8_t* bg_image, uint8_t* rgb_out) {
    R.hw = (uint32_t)S.h * (uint32_t)S.w; R.hw_magic = ~0ull / R.hw; R.w = (uint32_t)S.w; R.recs = W.recs;
    R.vertices = S.vertices; R.faces = S.faces; R.colors = colors; R.normals = normals; R.poses = S.poses; R.K = S.K;
    R.k_stride = S.k_per_instance ? 9 : 0; R.shading = shading; R.ambient = ambient;
    const uint32_t cr = bg_color[0], cg = bg_color[1], cb = bg_color[2];
    R.bg[0] = cr | (cg << 8) | (cb << 16) | (cr << 24);
    R.bg[1] = cg | (cb << 8) | (cr << 16) | (cg << 24);
    R.bg[2] = cb | (cr << 8) | (cg << 16) | (cb << 24);
    R.bg_image = bg_image; R.rgb = rgb_out;
    R.vec_rgb = (reinterpret_cast<uintptr_t>(rgb_out) & 3u) == 0 ? 1 : 0;
    R.vec_bg = (reinterpret_cast<uintptr_t>(bg_image) & 3u) == 0 ? 1 : 0;
}

}  // namespace
}  // namespace pvd
#endif  // PVNET_PIXEL_COLOR_H_
