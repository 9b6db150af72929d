// net_common.h -- what the four fused network libraries share (tail.hip, decoder.hip, stem.hip, trunk.hip): the leaves of their kernels
// and the host's argument checks and launch plan.  The staging pipelines, the MFMA schedules, the launch bounds and the register
// budgets are each file's own.  Nothing here changes the floating-point contraction mode of the file that includes it: the bodies that
// need one rounding per operation say so themselves.
#pragma once
#include "vote_common.h"

#include <type_traits>

namespace pvnc {

using pvd::f32x16;
using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;

// the type codes of a library's header (PVNET_<LIB>_T_*) are ld_elem_rt's
#define PVNET_NET_TYPE_CODES(LIB)                                                                                              \
    static_assert(PVNET_##LIB##_T_F32 == pvd::VT_F32 && PVNET_##LIB##_T_F16 == pvd::VT_F16 && PVNET_##LIB##_T_BF16 == pvd::VT_BF16, \
                  "the type codes of the library's header are ld_elem_rt's")

template <int VT>
struct elem {
    typedef typename std::conditional<VT == VT_F32, float, typename std::conditional<VT == VT_F16, _Float16, __bf16>::type>::type type;
};

// a lane's sixteen accumulator registers -> its pixel of the planes they are rows of (register g of lane half hh is row
// (g & 3) + 8 (g >> 2) + 4 hh), rows behind `rows` left out; `at` is the pixel's element in the block's plane 0.  One running pointer:
// a table of sixteen 64-bit plane offsets per lane is what the compiler otherwise keeps in registers across the whole kernel.
template <int VT>
__device__ __forceinline__ void store_rows(void* out, size_t at, size_t plane, const f32x16& v, int hh, int rows = 32) {
    typedef typename elem<VT>::type T;
    T* o = reinterpret_cast<T*>(out) + at + (size_t)(4 * hh) * plane;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        if ((g & 3) + 8 * (g >> 2) + 4 * hh < rows) *o = (T)v[g];   // one rounding to the output type
        o += (g & 3) == 3 ? 5 * plane : plane;
    }
}

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : v * 0.1f; }   // the LeakyReLU(0.1) of the reference's decoder

// tile `tile` of a batch cut into P.tiles_x x P.tiles_y tiles of TILE_W x ROWS pixels per image, x fastest: its image and top-left pixel
template <int TILE_W, int ROWS, class Args>
__device__ __forceinline__ void tile_of(const Args& P, int tile, int& bi, int& ty0, int& tx0) {
    const int tx = tile % P.tiles_x, rest = tile / P.tiles_x;
    const int ty = rest % P.tiles_y;
    bi = rest / P.tiles_y;
    ty0 = ty * ROWS;
    tx0 = tx * TILE_W;
}

// A staged pixel's record: 32 bfloat16 channels (the tail: 32 + 3 and a zero), padded from 64 to 80 bytes -- with that stride the
// sixteen lanes of a ds_read_b128 group are on sixteen different 16-byte slots.  A staging item is CPI channels of a pixel: 32 loads
// in flight per lane where they are upsampled, one 16-byte LDS store.
constexpr int REC = 80, CPI = 8;
__host__ __device__ constexpr int rec_slot(int p, int cg) { return p * REC + cg * (2 * CPI); }   // byte offset of item cg of pixel p

// The fragment-order weight image [cin/32, 9, 2, co/32, 64, 8] bfloat16, in units of a lane's eight values: k-step `step` = 18 chunk +
// 2 tap + half, row block m of mb, lane (r, hh) holds output channel 32 m + r, channel 32 chunk + 16 half + 8 hh + j of In at that tap.
template <class I>
__host__ __device__ constexpr I frag_at(I step, int mb, int m, int lane) { return (step * mb + m) * 64 + lane; }

// the four source pixels of output pixel (Y, X) of a bilinear 2x upsample with aligned corners and their weights: ry, rx are
// up_ratio's.  float32, one rounding per operation, as the headers define it.
struct Taps {
    int y0, y1, x0, x1;
    float ly, lx, my, mx;
    __device__ __forceinline__ Taps(int Y, int X, float ry, float rx, int hin, int win) {
#pragma clang fp contract(off)
        const float sy = (float)Y * ry, sx = (float)X * rx;
        y0 = min((int)sy, hin - 1), x0 = min((int)sx, win - 1);   // (the minimum never binds: sy <= hin - 1)
        y1 = y0 + (y0 < hin - 1), x1 = x0 + (x0 < win - 1);
        ly = sy - (float)y0, lx = sx - (float)x0;
        my = 1.f - ly, mx = 1.f - lx;
    }
    __device__ __forceinline__ float blend(float v00, float v01, float v10, float v11) const {
#pragma clang fp contract(off)
        const float top = mx * v00 + lx * v01, bot = mx * v10 + lx * v11;
        return my * top + ly * bot;
    }
};

// ---- the host's side of a launch
inline bool type_ok(int t) { return t == VT_F32 || t == VT_F16 || t == VT_BF16; }
inline bool sizes_ok(int b, int h, int w) { return b <= 65535 && h <= 32768 && w <= 32768; }   // beyond: PVNET_E_UNSUPPORTED
inline float up_ratio(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// P.tiles_x, P.tiles_y and P.ntiles of b images of h x w output pixels; returns the launch's work items, `groups` per tile, or -1
// where they pass 2^31 - 1 (PVNET_E_UNSUPPORTED)
template <int TILE_W, int ROWS, class Args>
inline long long plan_tiles(Args& P, int b, int h, int w, int groups = 1) {
    P.tiles_x = (w + TILE_W - 1) / TILE_W;
    P.tiles_y = (h + ROWS - 1) / ROWS;
    const long long ntiles = (long long)b * P.tiles_x * P.tiles_y, nitems = ntiles * groups;
    if (nitems > 0x7FFFFFFFll) return -1;
    P.ntiles = (int)ntiles;
    return nitems;
}

inline dim3 clamped_grid(int items, int max_grid) { return dim3(items < max_grid ? items : max_grid); }

inline int launch_status() {   // 0, or the launch's hipError_t
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace pvnc
