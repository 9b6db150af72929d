// tail.hip -- libpvnet_tail.so: the network's tail in one launch (include/pvnet_tail.h holds the definition): bilinear 2x upsample of
// the last decoder stage, concatenation with the image, 3 x 3 convolution with the eval() BatchNorm folded in, LeakyReLU(0.1) and the
// 1 x 1 convolution to the seg / vertex channels.
//
// Path replaced (reference tree): up2storaw + cat + convraw of Resnet18_8s.forward (lib/networks/model_repository.py:51-58, 74-78) --
// six eager kernels that write and re-read a 32-channel full-resolution tensor five times.  Here the half-resolution features and the
// image are read once and the output channels written once.
//
// A workgroup (four waves) walks tiles of TILE_W x ROWS output pixels, tile = blockIdx.x, += gridDim.x: the weights' fragments are
// loaded once per wave and stay in registers for every tile it takes.  Per tile
//   1. stage:   In with a one-pixel halo -> LDS, upsampled (float32, one rounding per operation: no contraction in this file) and
//               concatenated, a pixel's channels contiguous; zero outside the image (the convolution's padding).  bfloat16 records of
//               80 bytes (BF16 tier) or float32 records of 144 bytes (F32 tier); both strides keep the sixteen lanes of a
//               ds_read_b128 group on sixteen different 16-byte slots.
//   2. compute: BF16 tier -- wave v owns row v, 32 pixels per MFMA column block: X = W1 In as 18 + 2 v_mfma_f32_32x32x16_bf16 (raw
//               channels on the accumulator's rows, pixels on the lanes), then the accumulator tile IS the B operand of Y = W2 X: its
//               registers 8 s .. 8 s + 7, activated and rounded to bfloat16, are k-step s with the k order
//               16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), and W2's A fragment is loaded in that order.
//               F32 tier -- a lane owns a pixel: 32 accumulators, chains of fmaf; the workgroup brings one tap of w1 at a time into
//               LDS, [channel][raw channel], and every lane reads it by broadcast.
//   3. store:   pixels are on the lanes, so a store instruction writes 32 consecutive pixels of two channel planes (BF16 tier) or 64
//               of one (F32 tier); any alignment of `out`.  (No 16-byte store path: a lane holds ONE pixel of a plane, and bringing
//               eight to a lane would cost the lane movement the accumulator-as-operand layout avoids.)
#include "net_common.h"

#include "pvnet_tail.h"

// one rounding per operation: the header defines the upsample as separate float32 products and sums
#pragma clang fp contract(off)

namespace pvt {
namespace {

using pvd::bf16x8;
using pvd::f32x16;
using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;
using pvnc::CPI;
using pvnc::leaky;
using pvnc::rec_slot;

PVNET_NET_TYPE_CODES(TAIL);

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int WIDTH = PVNET_TAIL_WIDTH;   // feature channels, raw channels
constexpr int CIN = WIDTH + 3;            // channels of In
constexpr int W1_ROW = CIN * 9;           // w1 elements per raw channel
constexpr int TILE_W = 64, ROWS = 4;      // output pixels of a tile: a wave per row, two MFMA column blocks of 32
constexpr int THREADS = 64 * ROWS;
constexpr int HALO_W = TILE_W + 2, HALO_H = ROWS + 2, HALO_PIX = HALO_W * HALO_H;
constexpr int REC_BF = pvnc::REC;         // bytes of a pixel's record, BF16 tier: 32 + 3 channels + a zero, bfloat16
constexpr int REC_F = 144;                // F32 tier: 32 + 3 channels + 1 zero, float32
constexpr int FGROUPS = WIDTH / CPI, GROUPS = FGROUPS + 1;   // staging items per pixel: CPI feature channels each, then the image's three
constexpr int MAX_GRID = 768;             // workgroups of a launch: three per compute unit

struct TailArgs {
    const void* fm;
    const void* image;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    void* out;
    int64_t fs[4], is[4];
    int fm_type, image_type, out_type;
    int hin, win, h, w, cout, raw;
    int tiles_x, tiles_y, ntiles;
    float ry, rx;   // (float)(hin - 1) / (float)(h - 1), (float)(win - 1) / (float)(w - 1); 0 for h == 1 / w == 1
};

__device__ __forceinline__ void store_out(int vt, void* out, size_t idx, float v) {   // one rounding to the output type
    if (vt == VT_F16) reinterpret_cast<_Float16*>(out)[idx] = (_Float16)v;
    else if (vt == VT_BF16) reinterpret_cast<__bf16*>(out)[idx] = (__bf16)v;
    else reinterpret_cast<float*>(out)[idx] = v;
}

// In of the tile at (ty0, tx0) of image bi with its halo -> LDS.  An item is (group of CPI channels, pixel), pixels fastest: a wave's
// loads of a plane run along a row.
template <bool BF, int FT>
__device__ __forceinline__ void stage_tile_typed(const TailArgs& P, int bi, int ty0, int tx0, unsigned char* tile) {
    for (int it = threadIdx.x; it < GROUPS * HALO_PIX; it += THREADS) {
        const int cg = it / HALO_PIX, p = it - cg * HALO_PIX;
        const int py = p / HALO_W, px = p - py * HALO_W;
        const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
        float v[CPI];
#pragma unroll
        for (int c = 0; c < CPI; ++c) v[c] = 0.f;
        if (Y >= 0 && Y < P.h && X >= 0 && X < P.w) {
            if (cg < FGROUPS) {
                const pvnc::Taps t(Y, X, P.ry, P.rx, P.hin, P.win);
                const int y0 = t.y0, y1 = t.y1, x0 = t.x0, x1 = t.x1;
                const int64_t base = (int64_t)bi * P.fs[0] + (int64_t)(cg * CPI) * P.fs[1];
                const int64_t o00 = base + (int64_t)y0 * P.fs[2] + (int64_t)x0 * P.fs[3], o01 = base + (int64_t)y0 * P.fs[2] + (int64_t)x1 * P.fs[3];
                const int64_t o10 = base + (int64_t)y1 * P.fs[2] + (int64_t)x0 * P.fs[3], o11 = base + (int64_t)y1 * P.fs[2] + (int64_t)x1 * P.fs[3];
#pragma unroll
                for (int c = 0; c < CPI; ++c) {
                    const int64_t oc = (int64_t)c * P.fs[1];
                    const float v00 = pvd::ld_elem<FT>(P.fm, o00 + oc), v01 = pvd::ld_elem<FT>(P.fm, o01 + oc);
                    const float v10 = pvd::ld_elem<FT>(P.fm, o10 + oc), v11 = pvd::ld_elem<FT>(P.fm, o11 + oc);
                    v[c] = t.blend(v00, v01, v10, v11);
                }
            } else {
                const int64_t o = (int64_t)bi * P.is[0] + (int64_t)Y * P.is[2] + (int64_t)X * P.is[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = pvd::ld_elem_rt(P.image_type, P.image, o + (int64_t)c * P.is[1]);
            }
        }
        if (BF) {   // (the image's item writes channel 35, the zero the image's k-steps read, too)
            bf16x8 q;
#pragma unroll
            for (int c = 0; c < CPI; ++c) q[c] = (__bf16)v[c];
            *reinterpret_cast<bf16x8*>(tile + rec_slot(p, cg)) = q;
        } else {
            f32x4* dst = reinterpret_cast<f32x4*>(tile + p * REC_F + cg * (4 * CPI));
            dst[0] = f32x4{v[0], v[1], v[2], v[3]};
            if (cg < FGROUPS) dst[1] = f32x4{v[4], v[5], v[6], v[7]};   // (the image's item: channels 32 .. 35, the record ends there)
        }
    }
}

template <bool BF>
__device__ __forceinline__ void stage_tile(const TailArgs& P, int bi, int ty0, int tx0, unsigned char* tile) {   // (uniform branch)
    if (P.fm_type == VT_BF16) stage_tile_typed<BF, VT_BF16>(P, bi, ty0, tx0, tile);
    else if (P.fm_type == VT_F16) stage_tile_typed<BF, VT_F16>(P, bi, ty0, tx0, tile);
    else stage_tile_typed<BF, VT_F32>(P, bi, ty0, tx0, tile);
}

// byte offset, from the record of a block's top-left tap, of term k of the image's two k-steps: k = 3 tap + channel for k < 27, then
// one of the record's zeros (the weights' fragment holds zeros there too)
__host__ __device__ constexpr int image_term(int k) {
    return k < 27 ? ((k / 9) * HALO_W + (k / 3) % 3) * REC_BF + (WIDTH + k % 3) * 2 : CIN * 2;
}

// (amdgpu_num_vgpr: 160 usable of the 168 allocated -- the backend doubles the literal on this target, as for hypothesis_kernel --
// so three waves per SIMD, at the price of three spilled dwords)
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_num_vgpr(80))) void tail_bf16_kernel(TailArgs P) {
    PVNET_SPARE_VGPRS(167);
    __shared__ __attribute__((aligned(16))) unsigned char tile[HALO_PIX * REC_BF];
    __shared__ __attribute__((aligned(16))) float s_bias[2 * WIDTH];   // b1, then b2 with zeros behind cout
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    if (threadIdx.x < 2 * WIDTH)
        s_bias[threadIdx.x] = threadIdx.x < WIDTH ? P.b1[threadIdx.x] : (threadIdx.x - WIDTH < P.cout ? P.b2[threadIdx.x - WIDTH] : 0.f);
    // A fragments: lane (r, hh) holds row r, k = 8 hh + j of a k-step.  W1: k-step 2 tap + half is feature channel 16 half + k of that
    // tap; k-steps 18 and 19 are the image's 27 (tap, channel) terms, then zeros.  The workgroup rounds w1 to bfloat16 once, into the
    // LDS that holds the tiles afterwards, in fragment order; a wave then takes its twenty fragments with one ds_read_b128 each.
    static_assert(20 * 64 * 16 <= HALO_PIX * REC_BF, "W1's fragments pass through the tile's LDS");
    for (int i = threadIdx.x; i < 20 * 64 * 8; i += THREADS) {
        const int ks = i >> 9, fl = (i >> 3) & 63, j = i & 7;
        const int k = 8 * (fl >> 5) + j;   // within the k-step
        const float* w1r = P.w1 + (fl & 31) * W1_ROW;
        float wv;
        if (ks < 18) {
            wv = w1r[(16 * (ks & 1) + k) * 9 + (ks >> 1)];
        } else {
            const int ki = 16 * (ks - 18) + k;
            wv = ki < 27 ? w1r[(WIDTH + ki % 3) * 9 + ki / 3] : 0.f;
        }
        reinterpret_cast<__bf16*>(tile)[i] = (__bf16)wv;
    }
    __syncthreads();
    bf16x8 A1[20], A2[2];
#pragma unroll
    for (int ks = 0; ks < 20; ++ks) A1[ks] = reinterpret_cast<const bf16x8*>(tile)[ks * 64 + lane];
    // W2: k-step s in the accumulator's row order 16 s + 8 (j >> 2) + 4 hh + (j & 3); rows behind cout are zeros
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            A2[s][j] = (__bf16)(r < P.cout ? P.w2[r * WIDTH + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)] : 0.f);
    __syncthreads();   // the first tile overwrites the fragments' image
    const size_t plane = (size_t)P.h * P.w;

    for (int t_ = blockIdx.x; t_ < P.ntiles; t_ += gridDim.x) {
        int bi, ty0, tx0;
        pvnc::tile_of<TILE_W, ROWS>(P, t_, bi, ty0, tx0);
        stage_tile<true>(P, bi, ty0, tx0, tile);
        __syncthreads();
        const int Y = ty0 + wave;
        if (Y < P.h) {
#pragma unroll 1
            for (int q = 0; q < TILE_W / 32; ++q) {
                if (tx0 + 32 * q >= P.w) break;   // wave-uniform
                const int X = tx0 + 32 * q + r;
                const unsigned char* rec = tile + (wave * HALO_W + 32 * q + r) * REC_BF;   // the top-left tap of this lane's pixel
                f32x16 acc;
#pragma unroll
                for (int g = 0; g < 16; g += 4) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(s_bias + 2 * g + 4 * hh);   // rows 8 (g >> 2) + 4 hh + 0 .. 3
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[g + i] = bv[i];
                }
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int c16 = 0; c16 < 2; ++c16) {
                        const bf16x8 B = *reinterpret_cast<const bf16x8*>(rec + ((t / 3) * HALO_W + t % 3) * REC_BF + (16 * c16 + 8 * hh) * 2);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1[2 * t + c16], B, acc, 0, 0, 0);
                    }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4 raw;
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        const int o0 = hh ? image_term(16 * s + 8 + j) : image_term(16 * s + j);
                        const int o1 = hh ? image_term(16 * s + 9 + j) : image_term(16 * s + 1 + j);
                        raw[j >> 1] = (uint32_t)*reinterpret_cast<const uint16_t*>(rec + o0) |
                                      ((uint32_t)*reinterpret_cast<const uint16_t*>(rec + o1) << 16);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1[18 + s], __builtin_bit_cast(bf16x8, raw), acc, 0, 0, 0);
                }
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[g] = leaky(acc[g]);
                if (P.raw) {
                    if (X < P.w) pvnc::store_rows<VT_F32>(P.out, (size_t)bi * WIDTH * plane + (size_t)Y * P.w + X, plane, acc, hh, WIDTH);
                    continue;
                }
                bf16x8 B0, B1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    B0[j] = (__bf16)acc[j];
                    B1[j] = (__bf16)acc[8 + j];
                }
                f32x16 y;
#pragma unroll
                for (int g = 0; g < 16; g += 4) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(s_bias + WIDTH + 2 * g + 4 * hh);
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[g + i] = bv[i];
                }
                y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A2[0], B0, y, 0, 0, 0);
                y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A2[1], B1, y, 0, 0, 0);
                if (X < P.w) {
                    const size_t o = (size_t)bi * P.cout * plane + (size_t)Y * P.w + X;
                    if (P.out_type == VT_BF16) pvnc::store_rows<VT_BF16>(P.out, o, plane, y, hh, P.cout);
                    else if (P.out_type == VT_F16) pvnc::store_rows<VT_F16>(P.out, o, plane, y, hh, P.cout);
                    else pvnc::store_rows<VT_F32>(P.out, o, plane, y, hh, P.cout);
                }
            }
        }
        __syncthreads();   // the next tile overwrites the image
    }
}

__global__ __launch_bounds__(THREADS) void tail_f32_kernel(TailArgs P) {
    PVNET_SPARE_VGPRS(103);   // (89 in use)
    __shared__ __attribute__((aligned(16))) unsigned char tile[HALO_PIX * REC_F];
    __shared__ __attribute__((aligned(16))) float s_w[CIN * WIDTH];   // one tap of w1 at a time: with the image 61.5 KB of the 64 KB
    static_assert(sizeof(tile) + sizeof(s_w) <= 64 * 1024, "static LDS");
    const int row = threadIdx.x >> 6, col = threadIdx.x & 63;
    const size_t plane = (size_t)P.h * P.w;
    const float* __restrict__ w1 = P.w1;
    const float* __restrict__ w2 = P.w2;

    for (int t_ = blockIdx.x; t_ < P.ntiles; t_ += gridDim.x) {
        int bi, ty0, tx0;
        pvnc::tile_of<TILE_W, ROWS>(P, t_, bi, ty0, tx0);
        stage_tile<false>(P, bi, ty0, tx0, tile);
        __syncthreads();
        const int Y = ty0 + row, X = tx0 + col;
        const bool inside = Y < P.h && X < P.w;
        float x[WIDTH];
#pragma unroll
        for (int o = 0; o < WIDTH; ++o) x[o] = P.b1[o];
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            // the tap's weights, [channel of In][raw channel]: every lane reads the same address, one broadcast ds_read_b128 per four
            if (t > 0) __syncthreads();   // the previous tap's are read
            for (int i = threadIdx.x; i < CIN * WIDTH; i += THREADS) s_w[i] = w1[(i & (WIDTH - 1)) * W1_ROW + (i / WIDTH) * 9 + t];
            __syncthreads();
            if (!inside) continue;
            const unsigned char* rec = tile + ((row + t / 3) * HALO_W + col + t % 3) * REC_F;
#pragma unroll 1
            for (int c4 = 0; c4 < (CIN + 3) / 4; ++c4) {   // (channel 35 is the record's zero and has no weights: three terms in the last turn)
                const f32x4 in = *reinterpret_cast<const f32x4*>(rec + 16 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (4 * c4 + e >= CIN) break;
                    const f32x4* wv = reinterpret_cast<const f32x4*>(s_w + (4 * c4 + e) * WIDTH);
#pragma unroll
                    for (int o4 = 0; o4 < WIDTH / 4; ++o4) {
                        const f32x4 q = wv[o4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) x[4 * o4 + i] = fmaf(q[i], in[e], x[4 * o4 + i]);
                    }
                }
            }
        }
        if (inside) {
#pragma unroll
            for (int o = 0; o < WIDTH; ++o) x[o] = leaky(x[o]);
            if (P.raw) {
                float* o_ = reinterpret_cast<float*>(P.out) + (size_t)bi * WIDTH * plane + (size_t)Y * P.w + X;
#pragma unroll
                for (int o = 0; o < WIDTH; ++o) o_[(size_t)o * plane] = x[o];
            } else {
                const size_t o_ = (size_t)bi * P.cout * plane + (size_t)Y * P.w + X;
#pragma unroll 1
                for (int q = 0; q < P.cout; ++q) {
                    float y = P.b2[q];
#pragma unroll
                    for (int o = 0; o < WIDTH; ++o) y = fmaf(w2[q * WIDTH + o], x[o], y);
                    store_out(P.out_type, P.out, o_ + (size_t)q * plane, y);
                }
            }
        }
        __syncthreads();   // the next tile overwrites the image
    }
}

}  // namespace
}  // namespace pvt

using namespace pvt;

extern "C" {

int pvnet_tail_abi_version(void) { return PVNET_TAIL_ABI_VERSION; }

int pvnet_tail_forward(const void* fm, int fm_type, const int64_t fm_strides[4], const void* image, int image_type,
                       const int64_t image_strides[4], const float* w1, const float* b1, const float* w2, const float* b2, int b, int hin,
                       int win, int h, int w, int feat, int raw, int cout, int precision, uint32_t flags, void* out, int out_type,
                       void* stream) {
    if (!fm || !fm_strides || !image || !image_strides || !w1 || !b1 || !w2 || !b2 || !out) return PVNET_E_BADARG;
    if (b < 1 || hin < 1 || win < 1 || h < 1 || w < 1 || feat < 1 || raw < 1) return PVNET_E_BADARG;
    if (cout < 1 || cout > PVNET_TAIL_MAX_COUT) return PVNET_E_BADARG;
    if (!pvnc::type_ok(fm_type) || !pvnc::type_ok(image_type) || !pvnc::type_ok(out_type)) return PVNET_E_BADARG;
    if (precision != PVNET_TAIL_BF16 && precision != PVNET_TAIL_F32) return PVNET_E_BADARG;
    if ((flags & ~PVNET_TAIL_F_RAW) != 0) return PVNET_E_BADARG;
    if ((flags & PVNET_TAIL_F_RAW) && out_type != PVNET_TAIL_T_F32) return PVNET_E_BADARG;
    if ((long long)h != 2ll * hin || (long long)w != 2ll * win) return PVNET_E_BADARG;
    if (feat != PVNET_TAIL_WIDTH || raw != PVNET_TAIL_WIDTH) return PVNET_E_UNSUPPORTED;
    TailArgs P;
    if (!pvnc::sizes_ok(b, h, w) || pvnc::plan_tiles<TILE_W, ROWS>(P, b, h, w) < 0) return PVNET_E_UNSUPPORTED;
    P.fm = fm;
    P.image = image;
    P.w1 = w1;
    P.b1 = b1;
    P.w2 = w2;
    P.b2 = b2;
    P.out = out;
    for (int i = 0; i < 4; ++i) {
        P.fs[i] = fm_strides[i];
        P.is[i] = image_strides[i];
    }
    P.fm_type = fm_type;
    P.image_type = image_type;
    P.out_type = out_type;
    P.hin = hin;
    P.win = win;
    P.h = h;
    P.w = w;
    P.cout = cout;
    P.raw = (flags & PVNET_TAIL_F_RAW) ? 1 : 0;
    P.ry = pvnc::up_ratio(hin, h);
    P.rx = pvnc::up_ratio(win, w);
    const dim3 grid = pvnc::clamped_grid(P.ntiles, MAX_GRID), block(THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (precision == PVNET_TAIL_BF16) hipLaunchKernelGGL(tail_bf16_kernel, grid, block, 0, s, P);
    else hipLaunchKernelGGL(tail_f32_kernel, grid, block, 0, s, P);
    return pvnc::launch_status();
}

}  // extern "C"
