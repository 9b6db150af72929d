// augment_warp.h -- what augment.hip (libpvnet_augment.so) and color_jitter.hip (libpvnet_color.so) share of the geometric
// augmentation, so that both libraries run ONE copy of it: the plan of an image (the body of the plan kernel), the per-pixel part of
// the warp (the composed inverse map, the taps, the bilinear value and the mask of one output pixel), the stores of a lane's eight
// normalised pixels, and the argument checks of pvnet_augment.  THE DEFINITION: include/pvnet_augment.h (every step named below is a
// step of it).  Each translation unit wraps the bodies in kernels of its own names; everything here is internal to it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pvnet_augment.h"
#include "pvnet_rng.h"

// no contraction: every product and sum rounds as the restatements' separate operations do (fma only where written)
#pragma clang fp contract(off)

namespace {

constexpr int PLAN_T = 512, WARP_T = 256, PPL = 8;
constexpr int MAX_B = 65535, MAX_SIDE = 32768;
constexpr long long MAX_PIXELS = 1ll << 30;
constexpr uint32_t KNOWN_FLAGS = PVNET_AUGMENT_F_MASK | PVNET_AUGMENT_F_ROTATION | PVNET_AUGMENT_F_CROP | PVNET_AUGMENT_F_FLIP |
                                 PVNET_AUGMENT_F_USE_MASK_OUT;

// what the warp kernel needs of one image's augmentation
struct Plan {
    double a, b, r02, r12;   // the rotation (identity: 1, 0, 0, 0)
    double sw, sh;           // the resize's scales w / w2, h / h2
    int32_t rx0, rx1, ry0, ry1;   // the masked-out rectangle of the source (empty: rx0 >= rx1)
    int32_t resized, w2, h2, wbeg, hbeg, woff, hoff, flip, maskmul, pad_[3];
};
static_assert(sizeof(Plan) == 112, "Plan is 6 doubles and 16 ints");

struct Source {
    const uint8_t* rgb;
    const void* mask;   // NULL: pvnet_normalize
    int64_t rs[3], ms[3];
    int mask_dtype, h, w;
    uint64_t seed;
};

struct PlanArgs {
    Source S;
    PvnetAugmentConfig cfg;
    int vn, height, width;
    double* hc_out;
    int32_t* status;
    Plan* plans;
};

__device__ __forceinline__ long long load_mask(const Source& S, int bi, int x, int y) {
    const int64_t off = (int64_t)bi * S.ms[0] + (int64_t)y * S.ms[1] + (int64_t)x * S.ms[2];
    if (S.mask_dtype == PVNET_MASK_U8) return reinterpret_cast<const uint8_t*>(S.mask)[off];
    if (S.mask_dtype == PVNET_MASK_I32) return reinterpret_cast<const int32_t*>(S.mask)[off];
    return reinterpret_cast<const long long*>(S.mask)[off];
}

// the source mask after step 1: 0 outside the source and inside the rectangle
__device__ __forceinline__ long long mask_tap(const Source& S, int bi, int rx0, int rx1, int ry0, int ry1, int x, int y) {
    if (x < 0 || y < 0 || x >= S.w || y >= S.h) return 0;
    if (x >= rx0 && x < rx1 && y >= ry0 && y < ry1) return 0;
    return load_mask(S, bi, x, y);
}

// step 2's inverse map, nearest: the source pixel of canvas pixel (X, Y)
__device__ __forceinline__ void nearest_source(double a, double b, double r02, double r12, int X, int Y, int& x, int& y) {
    const double dx = (double)X - r02, dy = (double)Y - r12;
    const double sx = a * dx - b * dy, sy = b * dx + a * dy;
    // (a canvas point far outside maps outside: keep the conversion to int defined)
    x = sx > -2.0 && sx < 40000.0 ? (int)floor(sx + 0.5) : -1;
    y = sy > -2.0 && sy < 40000.0 ? (int)floor(sy + 0.5) : -1;
}

// step 3's nearest map of one axis: the canvas index of resized index X
__device__ __forceinline__ int resize_nearest(int X, double s, int n) {
    const int v = (int)floor((double)X * s);
    return v < n - 1 ? v : n - 1;
}

// is canvas index x1 the image of a resized index in [0, n2)?
__device__ __forceinline__ bool resize_hits(int x1, double s, int n2, int n) {
    const int X0 = (int)floor((double)x1 / s);
    bool hit = false;
#pragma unroll
    for (int d = -1; d <= 2; ++d) {
        const int X = X0 + d;
        hit |= X >= 0 && X < n2 && resize_nearest(X, s, n) == x1;
    }
    return hit;
}

// the first / the last resized index whose image is x1 (x1 is hit)
__device__ __forceinline__ int resize_first(int x1, double s, int n2, int n) {
    int X = (int)floor((double)x1 / s) - 1;
    X = X < 0 ? 0 : (X > n2 - 1 ? n2 - 1 : X);
    while (X < n2 - 1 && resize_nearest(X, s, n) < x1) ++X;
    while (X > 0 && resize_nearest(X - 1, s, n) >= x1) --X;
    return X;
}
__device__ __forceinline__ int resize_last(int x1, double s, int n2, int n) {
    int X = (int)floor((double)(x1 + 1) / s) + 1;
    X = X < 0 ? 0 : (X > n2 - 1 ? n2 - 1 : X);
    while (X > 0 && resize_nearest(X, s, n) > x1) --X;
    while (X < n2 - 1 && resize_nearest(X + 1, s, n) <= x1) ++X;
    return X;
}

__device__ __forceinline__ int randint(int lo, int hi, double u, int& status) {
    if (hi <= lo) {
        status |= PVNET_AUGMENT_S_RANGE;
        return lo;
    }
    const int v = (int)floor((double)lo + u * (double)(hi - lo));
    return v < hi - 1 ? v : hi - 1;
}

enum { R_SUM, R_MIN, R_MAX };
constexpr long long BIG = 1ll << 40;
constexpr int PLAN_SH = (PLAN_T / 64) * 5;   // long longs of LDS the plan body needs

// integer block reduction of K values; every thread gets the results.  `sh` holds (PLAN_T / 64) * K values.
template <int K>
__device__ __forceinline__ void block_reduce(long long (&v)[K], const int (&op)[K], long long* sh) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off; off >>= 1) {
            const long long o = __shfl_xor(v[k], off);
            v[k] = op[k] == R_SUM ? v[k] + o : (op[k] == R_MIN ? (o < v[k] ? o : v[k]) : (o > v[k] ? o : v[k]));
        }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();   // the previous reduction's readers are done with sh
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        long long r = sh[k];
        for (int wv = 1; wv < PLAN_T / 64; ++wv) {
            const long long o = sh[wv * K + k];
            r = op[k] == R_SUM ? r + o : (op[k] == R_MIN ? (o < r ? o : r) : (o > r ? o : r));
        }
        v[k] = r;
    }
}

// The plan of image blockIdx.x, by a block of PLAN_T threads.  Up to four passes over the image's mask, each an integer block
// reduction (sums, minima, maxima: no atomics, no floating reduction): the bbox and the count of the foreground; the count and the
// coordinate sums outside the masked-out rectangle; the bbox of the rotated mask through the inverse map; where the image is resized,
// the bbox of the foreground pixels that the resize's nearest map hits (the bbox of the resized mask follows from it, the map being
// monotone per axis).  Every thread derives the plan from the reduced values (the same arithmetic on the same numbers); thread 0
// writes the plan and the status, threads k < vn the key-points.  `sh`: PLAN_SH long longs of LDS.
// (hcoords carries no __restrict__: hcoords_out may be the same array -- each thread reads its key-point before it writes it)
__device__ __forceinline__ void augment_plan_body(const PlanArgs& A, const double* __restrict__ uniforms, const double* hcoords, long long* sh) {
    const Source& S = A.S;
    const PvnetAugmentConfig& cfg = A.cfg;
    const int bi = blockIdx.x, tid = threadIdx.x;
    const int h = S.h, w = S.w, npix = h * w;
    const double* __restrict__ u = uniforms + (size_t)bi * PVNET_AUGMENT_UNIFORMS;
    const int op5[5] = {R_SUM, R_MIN, R_MAX, R_MIN, R_MAX};
    int status = 0;
    Plan P;
    P.a = 1.0, P.b = 0.0, P.r02 = 0.0, P.r12 = 0.0, P.sw = 1.0, P.sh = 1.0;
    P.rx0 = P.rx1 = P.ry0 = P.ry1 = 0;
    P.resized = 0, P.w2 = w, P.h2 = h, P.wbeg = P.hbeg = P.woff = P.hoff = 0;
    P.pad_[0] = P.pad_[1] = P.pad_[2] = 0;

    // ---- step 0: the foreground's count and bbox
    long long v[5] = {0, BIG, -1, BIG, -1};
    for (int p = tid; p < npix; p += PLAN_T) {
        const int y = p / w, x = p - y * w;
        if (load_mask(S, bi, x, y) != 0) {
            ++v[0];
            v[1] = x < v[1] ? x : v[1], v[2] = x > v[2] ? x : v[2];
            v[3] = y < v[3] ? y : v[3], v[4] = y > v[4] ? y : v[4];
        }
    }
    block_reduce(v, op5, sh);
    const long long n0 = v[0];
    bool fg = n0 > 0;
    if (!fg) status |= PVNET_AUGMENT_S_NO_FOREGROUND;

    // ---- step 1: mask-out
    if ((cfg.flags & PVNET_AUGMENT_F_MASK) && fg && u[0] < 0.5) {
        const int xmin = (int)v[1], xmax = (int)v[2], ymin = (int)v[3], ymax = (int)v[4];
        const double fx = cfg.min_mask + (cfg.max_mask - cfg.min_mask) * u[1], fy = cfg.min_mask + (cfg.max_mask - cfg.min_mask) * u[2];
        const double xs = floor((double)(xmax - xmin) * fx / 2.0), ys = floor((double)(ymax - ymin) * fy / 2.0);
        const int x_side = xs > 0.0 && xs < (double)MAX_SIDE ? (int)xs : 0, y_side = ys > 0.0 && ys < (double)MAX_SIDE ? (int)ys : 0;
        const int x_loc = randint(xmin, xmax, u[3], status), y_loc = randint(ymin, ymax, u[4], status);
        // numpy's slice rule: a negative start counts from the end (and is empty unless it wraps below the stop), a stop is clipped
        int x0 = x_loc - x_side, y0 = y_loc - y_side;
        x0 = x0 < 0 ? (x0 + w > 0 ? x0 + w : 0) : x0;
        y0 = y0 < 0 ? (y0 + h > 0 ? y0 + h : 0) : y0;
        const int x1 = x_loc + x_side < w ? x_loc + x_side : w, y1 = y_loc + y_side < h ? y_loc + y_side : h;
        if (x0 < x1 && y0 < y1) P.rx0 = x0, P.rx1 = x1, P.ry0 = y0, P.ry1 = y1;
    }

    // ---- what is left: count and coordinate sums
    long long n1 = 0, sumx = 0, sumy = 0;
    if (fg) {
        long long q[3] = {0, 0, 0};
        const int op3[3] = {R_SUM, R_SUM, R_SUM};
        for (int p = tid; p < npix; p += PLAN_T) {
            const int y = p / w, x = p - y * w;
            if (mask_tap(S, bi, P.rx0, P.rx1, P.ry0, P.ry1, x, y) != 0) ++q[0], q[1] += x, q[2] += y;
        }
        block_reduce(q, op3, sh);
        n1 = q[0], sumx = q[1], sumy = q[2];
        if (n1 == 0) {
            status |= PVNET_AUGMENT_S_EMPTIED;
            fg = false;
        }
    }

    // ---- step 2: rotation about the centroid
    const bool rotated = fg && (cfg.flags & PVNET_AUGMENT_F_ROTATION);
    if (rotated) {
        P.a = u[12], P.b = u[13];
        const double cx = (double)sumx / (double)n1, cy = (double)sumy / (double)n1, t = 1.0 - P.a;
        P.r02 = t * cx - P.b * cy;
        P.r12 = P.b * cx + t * cy;
    }

    // ---- step 3: the rotated mask's bbox, the resize
    bool inst = false;   // step 4a (else 4b)
    double ratio = 1.0;
    int hmin = 0, hmax = 0, wmin = 0, wmax = 0;
    const bool crop = fg && (cfg.flags & PVNET_AUGMENT_F_CROP);
    if (crop) {
        long long r[5] = {0, BIG, -1, BIG, -1};
        for (int p = tid; p < npix; p += PLAN_T) {
            const int Y = p / w, X = p - Y * w;
            int x, y;
            nearest_source(P.a, P.b, P.r02, P.r12, X, Y, x, y);
            if (mask_tap(S, bi, P.rx0, P.rx1, P.ry0, P.ry1, x, y) != 0) {
                ++r[0];
                r[1] = X < r[1] ? X : r[1], r[2] = X > r[2] ? X : r[2];
                r[3] = Y < r[3] ? Y : r[3], r[4] = Y > r[4] ? Y : r[4];
            }
        }
        block_reduce(r, op5, sh);
        inst = r[0] > 0;
        if (!inst) status |= PVNET_AUGMENT_S_DEGENERATE;
        wmin = (int)r[1], wmax = (int)r[2], hmin = (int)r[3], hmax = (int)r[4];
        if (inst && u[6] < 0.8) {
            const int xlen = wmax - wmin, ylen = hmax - hmin;
            bool ok = xlen > 0 && ylen > 0;
            int w2 = w, h2 = h;
            if (ok) {
                double rmin = cfg.resize_wmin / (double)xlen, rmax = cfg.resize_wmax / (double)xlen;
                const double rh = cfg.resize_hmax / (double)ylen, rl = cfg.resize_hmin / (double)ylen;
                rmax = rh < rmax ? rh : rmax;
                rmin = rl > rmin ? rl : rmin;
                ratio = rmin + (rmax - rmin) * u[7];
                const double th = (double)h * ratio, tw = (double)w * ratio;
                ok = th >= 1.0 && tw >= 1.0 && th < 16777216.0 && tw < 16777216.0;
                if (ok) h2 = (int)th, w2 = (int)tw;
            }
            long long t[5] = {0, BIG, -1, BIG, -1};
            if (ok) {   // (block-uniform: every thread holds the same reduced values)
                const double sw = (double)w / (double)w2, shh = (double)h / (double)h2;
                for (int p = tid; p < npix; p += PLAN_T) {
                    const int Y = p / w, X = p - Y * w;
                    int x, y;
                    nearest_source(P.a, P.b, P.r02, P.r12, X, Y, x, y);
                    if (mask_tap(S, bi, P.rx0, P.rx1, P.ry0, P.ry1, x, y) != 0 && resize_hits(X, sw, w2, w) && resize_hits(Y, shh, h2, h)) {
                        ++t[0];
                        t[1] = X < t[1] ? X : t[1], t[2] = X > t[2] ? X : t[2];
                        t[3] = Y < t[3] ? Y : t[3], t[4] = Y > t[4] ? Y : t[4];
                    }
                }
                block_reduce(t, op5, sh);
                ok = t[0] > 0;
                if (ok) {
                    P.resized = 1, P.w2 = w2, P.h2 = h2, P.sw = sw, P.sh = shh;
                    wmin = resize_first((int)t[1], sw, w2, w), wmax = resize_last((int)t[2], sw, w2, w);
                    hmin = resize_first((int)t[3], shh, h2, h), hmax = resize_last((int)t[4], shh, h2, h);
                }
            }
            if (!ok) {
                status |= PVNET_AUGMENT_S_DEGENERATE;
                ratio = 1.0;
            }
        }
    }

    // ---- step 4: crop or pad
    const int height = A.height, width = A.width;
    const bool hpad = height >= P.h2, wpad = width >= P.w2;
    bool moved = false;   // the key-points follow the crop
    if (inst) {
        const double ah = (double)hmin + cfg.overlap_ratio * (double)(hmax - hmin), aw = (double)wmin + cfg.overlap_ratio * (double)(wmax - wmin);
        const double hd = (double)(P.h2 - height), wd = (double)(P.w2 - width);
        const int hrmax = (int)(ah < hd ? ah : hd), wrmax = (int)(aw < wd ? aw : wd);
        const double hl = ah - (double)height, wl = aw - (double)width;
        const int hrmin = (int)(hl > 0.0 ? hl : 0.0), wrmin = (int)(wl > 0.0 ? wl : 0.0);
        if (!hpad) P.hbeg = randint(hrmin, hrmax, u[8], status);
        if (!wpad) P.wbeg = randint(wrmin, wrmax, u[9], status);
        moved = true;
    } else if (!fg || crop) {
        if (!hpad) P.hbeg = randint(0, P.h2 - height, u[8], status);
        if (!wpad) P.wbeg = randint(0, P.w2 - width, u[9], status);
    }
    P.hoff = hpad ? (height - P.h2) / 2 : 0;
    P.woff = wpad ? (width - P.w2) / 2 : 0;
    P.flip = (cfg.flags & PVNET_AUGMENT_F_FLIP) && u[10] < 0.5 ? 1 : 0;
    P.maskmul = (cfg.flags & PVNET_AUGMENT_F_USE_MASK_OUT) && u[11] < 0.1 ? 1 : 0;

    if (tid == 0) {
        A.plans[bi] = P;
        A.status[bi] = status;
    }
    // ---- the key-points: the same steps, sequentially, as the reference writes them
    for (int k = tid; k < A.vn; k += PLAN_T) {
        const double* hc = hcoords + ((size_t)bi * A.vn + k) * 3;
        double x = hc[0], y = hc[1], z = hc[2];
        if (rotated) {
            const double nx = __builtin_fma(z, P.r02, __builtin_fma(y, P.b, x * P.a));
            const double ny = __builtin_fma(z, P.r12, __builtin_fma(y, P.a, x * -P.b));
            const double nz = __builtin_fma(z, 1.0, __builtin_fma(y, 0.0, x * 0.0));
            x = nx, y = ny, z = nz;
        }
        if (P.resized) x = x * ratio, y = y * ratio;
        if (moved) {
            x = x - (double)P.wbeg * z;
            y = y - (double)P.hbeg * z;
            if (hpad || wpad) {
                x = x + (double)P.woff * z;
                y = y + (double)P.hoff * z;
            }
        }
        if (P.flip) {
            const double half = (double)width / 2.0;
            x = x - half * z;
            x = -x;
            x = x + half * z;
        }
        double* o = A.hc_out + ((size_t)bi * A.vn + k) * 3;
        o[0] = x, o[1] = y, o[2] = z;
    }
}

// one source image tap of channel c after step 1: 0 outside, the counter-based fill inside the rectangle
__device__ __forceinline__ double image_tap(const Source& S, const Plan& P, const uint8_t* __restrict__ img, uint32_t key, int x, int y, int c) {
    if (x < 0 || y < 0 || x >= S.w || y >= S.h) return 0.0;
    if (x >= P.rx0 && x < P.rx1 && y >= P.ry0 && y < P.ry1)
        return (double)pvnet_rng_below(pvnet_rng_at(key, (uint32_t)(y * S.w + x) * 3u + (uint32_t)c), 255u);
    return (double)img[(int64_t)y * S.rs[1] + (int64_t)x * S.rs[2] + c];
}

__device__ __forceinline__ void identity_plan(const Source& S, Plan& P) {
    P.a = 1.0, P.b = 0.0, P.r02 = 0.0, P.r12 = 0.0, P.sw = 1.0, P.sh = 1.0;
    P.rx0 = P.rx1 = P.ry0 = P.ry1 = 0;
    P.resized = 0, P.w2 = S.w, P.h2 = S.h, P.wbeg = P.hbeg = P.woff = P.hoff = P.flip = P.maskmul = 0;
}

// The per-pixel part of the warp: output pixel (X, Y) of image bi, with yc = Y - P.hoff and y2 = yc + P.hbeg.  The composed inverse
// map in float64, four uint8 taps per channel, bilinear, rounded: val[c] is an integer 0 .. 255 held in a double; m is the source
// mask at the nearest pixel of the composed map.  X >= width (the tail of a lane) gives zeros.
__device__ __forceinline__ void warp_pixel(const Source& S, const Plan& P, const uint8_t* __restrict__ img, uint32_t key, int bi, int X, int yc,
                                           int y2, int width, double (&val)[3], long long& m) {
    const int Xf = P.flip ? width - 1 - X : X;
    const int xc = Xf - P.woff, x2 = xc + P.wbeg;
    val[0] = val[1] = val[2] = 0.0;
    m = 0;
    if (X < width && xc >= 0 && yc >= 0 && x2 < P.w2 && y2 < P.h2) {
        double cx = (double)x2, cy = (double)y2;
        int mx = x2, my = y2;
        if (P.resized) {
            cx = ((double)x2 + 0.5) * P.sw - 0.5;
            cy = ((double)y2 + 0.5) * P.sh - 0.5;
            cx = cx < 0.0 ? 0.0 : (cx > (double)(S.w - 1) ? (double)(S.w - 1) : cx);
            cy = cy < 0.0 ? 0.0 : (cy > (double)(S.h - 1) ? (double)(S.h - 1) : cy);
            mx = resize_nearest(x2, P.sw, S.w);
            my = resize_nearest(y2, P.sh, S.h);
        }
        if (S.mask) {
            int msx, msy;
            nearest_source(P.a, P.b, P.r02, P.r12, mx, my, msx, msy);
            m = mask_tap(S, bi, P.rx0, P.rx1, P.ry0, P.ry1, msx, msy);
        }
        const double dx = cx - P.r02, dy = cy - P.r12;
        const double sx = P.a * dx - P.b * dy, sy = P.b * dx + P.a * dy;
        if (sx > -1.0 && sx < (double)S.w && sy > -1.0 && sy < (double)S.h) {
            const double fx0 = floor(sx), fy0 = floor(sy);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const double fx = sx - fx0, fy = sy - fy0, gx = 1.0 - fx, gy = 1.0 - fy;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v00 = image_tap(S, P, img, key, x0, y0, c), v01 = image_tap(S, P, img, key, x0 + 1, y0, c);
                const double v10 = image_tap(S, P, img, key, x0, y0 + 1, c), v11 = image_tap(S, P, img, key, x0 + 1, y0 + 1, c);
                const double top = v00 * gx + v01 * fx, bot = v10 * gx + v11 * fx;
                val[c] = rint(top * gy + bot * fy);
            }
        }
    }
}

__device__ __forceinline__ uint16_t to_bf16(float f) {   // round to nearest even (finite values only here)
    const uint32_t x = __float_as_uint(f);
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ uint16_t to_f16(float f) {
    const _Float16 v = (_Float16)f;
    return __builtin_bit_cast(uint16_t, v);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// A lane's eight normalised pixels of the three planes of image bi, from column X0 of row `row / width`: `row` = Y width + X0.
// OUT: PVNET_AUGMENT_OUT_*;  VEC: 16 bytes per store (width % 8 == 0, an aligned image), else element by element.
template <int OUT, bool VEC>
__device__ __forceinline__ void store_planes(void* image, int bi, size_t plane, size_t row, int X0, int width, const float (&o)[3][PPL]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t off = ((size_t)bi * 3 + c) * plane + row;
        if (OUT == PVNET_AUGMENT_OUT_F32) {
            float* dst = reinterpret_cast<float*>(image) + off;
            if (VEC) {
                u32x4 q0, q1;
#pragma unroll
                for (int i = 0; i < 4; ++i) q0[i] = __float_as_uint(o[c][i]), q1[i] = __float_as_uint(o[c][4 + i]);
                *reinterpret_cast<u32x4*>(dst) = q0;
                *reinterpret_cast<u32x4*>(dst + 4) = q1;
            } else {
                for (int i = 0; i < PPL; ++i)
                    if (X0 + i < width) dst[i] = o[c][i];
            }
        } else {
            uint16_t* dst = reinterpret_cast<uint16_t*>(image) + off;
            uint16_t hv[PPL];
#pragma unroll
            for (int i = 0; i < PPL; ++i) hv[i] = OUT == PVNET_AUGMENT_OUT_BF16 ? to_bf16(o[c][i]) : to_f16(o[c][i]);
            if (VEC) {
                u32x4 q;
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = (uint32_t)hv[2 * i] | ((uint32_t)hv[2 * i + 1] << 16);
                *reinterpret_cast<u32x4*>(dst) = q;
            } else {
                for (int i = 0; i < PPL; ++i)
                    if (X0 + i < width) dst[i] = hv[i];
            }
        }
    }
}

// a lane's eight pixels of the output mask (PVNET_MASK_U8 or PVNET_MASK_I64), addressed as store_planes addresses a plane
template <bool VEC>
__device__ __forceinline__ void store_mask(void* mask_out, int mask_out_dtype, int bi, size_t plane, size_t row, int X0, int width,
                                           const long long (&mo)[PPL]) {
    const size_t off = (size_t)bi * plane + row;
    if (mask_out_dtype == PVNET_MASK_U8) {
        uint8_t* dst = reinterpret_cast<uint8_t*>(mask_out) + off;
        if (VEC) {
            u32x2 q = {0u, 0u};
#pragma unroll
            for (int i = 0; i < PPL; ++i) q[i >> 2] |= ((uint32_t)mo[i] & 0xFFu) << (8 * (i & 3));
            *reinterpret_cast<u32x2*>(dst) = q;
        } else {
            for (int i = 0; i < PPL; ++i)
                if (X0 + i < width) dst[i] = (uint8_t)mo[i];
        }
    } else {
        long long* dst = reinterpret_cast<long long*>(mask_out) + off;
        if (VEC) {
#pragma unroll
            for (int i = 0; i < PPL; i += 2) {
                u32x4 q = {(uint32_t)mo[i], (uint32_t)((unsigned long long)mo[i] >> 32), (uint32_t)mo[i + 1],
                           (uint32_t)((unsigned long long)mo[i + 1] >> 32)};
                *reinterpret_cast<u32x4*>(dst + i) = q;
            }
        } else {
            for (int i = 0; i < PPL; ++i)
                if (X0 + i < width) dst[i] = mo[i];
        }
    }
}

// ---- host: the argument checks, before any HIP call

inline int check_source(const void* rgb, const int64_t* rgb_strides, int b, int h, int w) {
    if (!rgb || !rgb_strides) return PVNET_E_BADARG;
    if (b < 0 || h <= 0 || w <= 0) return PVNET_E_BADARG;
    if (b > MAX_B || h > MAX_SIDE || w > MAX_SIDE || (long long)h * w > MAX_PIXELS) return PVNET_E_UNSUPPORTED;
    return 0;
}

inline int check_image(const void* image, int image_dtype) {
    if (!image) return PVNET_E_BADARG;
    if (image_dtype != PVNET_AUGMENT_OUT_F32 && image_dtype != PVNET_AUGMENT_OUT_BF16 && image_dtype != PVNET_AUGMENT_OUT_F16)
        return PVNET_E_BADARG;
    return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline Source make_source(const uint8_t* rgb, const int64_t* rs, const void* mask, int mask_dtype, const int64_t* ms, int h, int w, uint64_t seed) {
    Source S;
    S.rgb = rgb;
    S.mask = mask;
    for (int i = 0; i < 3; ++i) S.rs[i] = rs[i], S.ms[i] = ms ? ms[i] : 0;
    S.mask_dtype = mask_dtype;
    S.h = h;
    S.w = w;
    S.seed = seed;
    return S;
}

inline bool config_ok(const float* mean, const float* std) {
    for (int c = 0; c < 3; ++c)
        if (!(std[c] > 0.0f) || !(mean[c] == mean[c])) return false;
    return true;
}

// everything pvnet_augment checks but its workspace; 0 where the call may go on (b == 0 included: the caller returns 0 then)
inline int check_augment(const uint8_t* rgb, const int64_t* rgb_strides, const void* mask, int mask_dtype, const int64_t* mask_strides,
                         const double* hcoords, const double* uniforms, int b, int h, int w, int vn, int height, int width,
                         const PvnetAugmentConfig* cfg, const void* image, int image_dtype, const void* mask_out, int mask_out_dtype,
                         const double* hcoords_out, const int32_t* status) {
    if (!mask || !mask_strides || !hcoords || !uniforms || !cfg || !mask_out || !hcoords_out || !status) return PVNET_E_BADARG;
    if (const int rc = check_source(rgb, rgb_strides, b, h, w)) return rc;
    if (const int rc = check_image(image, image_dtype)) return rc;
    if (vn <= 0 || height <= 0 || width <= 0) return PVNET_E_BADARG;
    if ((cfg->flags & ~KNOWN_FLAGS) != 0 || cfg->reserved != 0 || !config_ok(cfg->mean, cfg->std)) return PVNET_E_BADARG;
    if (!(cfg->min_mask >= 0.0) || !(cfg->max_mask >= cfg->min_mask) || !(cfg->max_mask <= 2.0) || !(cfg->overlap_ratio >= 0.0) ||
        !(cfg->overlap_ratio <= 1.0) || !(cfg->resize_hmin > 0.0) || !(cfg->resize_hmax >= cfg->resize_hmin) || !(cfg->resize_wmin > 0.0) ||
        !(cfg->resize_wmax >= cfg->resize_wmin) || !(cfg->resize_hmax < 1e9) || !(cfg->resize_wmax < 1e9))
        return PVNET_E_BADARG;
    if (!(cfg->flags & PVNET_AUGMENT_F_CROP) && (height != h || width != w)) return PVNET_E_BADARG;
    if (mask_dtype == PVNET_MASK_I16 || mask_dtype == PVNET_MASK_F32 || mask_dtype == PVNET_MASK_LOGITS_F32) return PVNET_E_UNSUPPORTED;
    if (mask_dtype != PVNET_MASK_U8 && mask_dtype != PVNET_MASK_I32 && mask_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (mask_out_dtype != PVNET_MASK_U8 && mask_out_dtype != PVNET_MASK_I64) return PVNET_E_BADARG;
    if (height > MAX_SIDE || width > MAX_SIDE || (long long)height * width > MAX_PIXELS || vn > (1 << 20)) return PVNET_E_UNSUPPORTED;
    return 0;
}

}  // namespace
