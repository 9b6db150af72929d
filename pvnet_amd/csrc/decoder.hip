// decoder.hip -- libpvnet_decoder.so: one decoder stage in one launch (include/pvnet_decoder.h holds the definition): bilinear 2x
// upsample of the previous stage, concatenation with the trunk's skip features, 3 x 3 convolution with the eval() BatchNorm folded in
// and LeakyReLU(0.1).
//
// Path replaced (reference tree): up8sto4s + cat + conv4s and up4sto2s + cat + conv2s of Resnet18_8s.forward
// (lib/networks/model_repository.py:29-50, 67-73) -- five eager kernels each, which write and re-read the upsampled tensor, the
// concatenated tensor and the convolution's output.  Here the two inputs are read once (with the tiles' halo) and the output written once.
//
// A workgroup (four waves) walks tiles of TILE_W x ROWS output pixels, tile = blockIdx.x, += gridDim.x.  The weights do not fit in
// registers (128 or 192 input channels against the tail's 35), so a tile is a loop over CHUNKS of 32 channels of In, the accumulators
// (CO / 32 row blocks x 2 column blocks of 32 pixels per wave) persisting across them.  Per chunk
//   1. stage:   the chunk of In with a one-pixel halo -> LDS: upsampled (float32, one rounding per operation: no contraction in this
//               file) for the channels of `lo`, copied for those of `skip`, rounded to bfloat16, a pixel's 32 channels contiguous in a
//               record of 80 bytes (the tail's stride: the sixteen lanes of a ds_read_b128 group on sixteen different 16-byte slots);
//               zero outside the image (the convolution's padding).
//   2. compute: wave v owns row v.  18 k-steps (9 taps x 2 halves of the chunk): B = one ds_read_b128 per lane and column block, A =
//               the weights' fragment, one 16-byte load per lane from the fragment-order image (PVNET_DECODER_F_PACKED; every wave of
//               the launch reads the same 74 / 221 KB: L2) or eight float32 loads rounded here.  An A fragment serves both column
//               blocks and a B fragment all row blocks: 1.5 (CO = 32) or 1 (CO = 64) fragment reads per MFMA.
// then, per tile, 3. store: pixels are on the lanes, so a store instruction writes 32 consecutive pixels of a channel plane; any
// alignment of `out`.
#include "net_common.h"

#include "pvnet_decoder.h"

// one rounding per operation: the header defines the upsample as separate float32 products and sums
#pragma clang fp contract(off)

namespace pvdec {
namespace {

using pvd::bf16x8;
using pvd::f32x16;
using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;
using pvnc::CPI;
using pvnc::REC;
using pvnc::rec_slot;

PVNET_NET_TYPE_CODES(DECODER);

constexpr int CS = PVNET_DECODER_SKIP;    // channels of skip
constexpr int CHUNK = 32;                 // channels of In staged at a time: two k-steps per tap
constexpr int TILE_W = 64, ROWS = 4;      // output pixels of a tile: a wave per row, two MFMA column blocks of 32
constexpr int NQ = TILE_W / 32;
constexpr int THREADS = 64 * ROWS;
constexpr int HALO_W = TILE_W + 2, HALO_H = ROWS + 2, HALO_PIX = HALO_W * HALO_H;
constexpr int GROUPS = CHUNK / CPI;       // staging items per pixel and chunk
constexpr int KSTEPS = 18;                // per chunk: 9 taps x 2 halves of 16 channels
constexpr int MAX_GRID_32 = 1024, MAX_GRID_64 = 768;   // workgroups of a launch: four (CO = 32) or three (CO = 64) per compute unit

struct StageArgs {
    const void* lo;
    const void* skip;
    const float* w;      // [co,cl+cs,3,3] float32, or the fragment-order bfloat16 image
    const float* bias;
    void* out;
    int64_t ls[4], ss[4];
    int lo_type, skip_type, out_type;
    int hin, win, h, w_;
    int tiles_x, tiles_y, ntiles;
    float ry, rx;   // (float)(hin - 1) / (float)(h - 1), (float)(win - 1) / (float)(w_ - 1); 0 for h == 1 / w_ == 1
};

// channels c0 .. c0 + 31 of In, upsampled from `lo`, of the tile at (ty0, tx0) of image bi with its halo -> LDS.  An item is (group of
// CPI channels, pixel), pixels fastest: a wave's loads of a plane run along a row.
template <int FT>
__device__ __forceinline__ void stage_lo(const StageArgs& P, int bi, int ty0, int tx0, int c0, unsigned char* tile) {
    for (int it = threadIdx.x; it < GROUPS * HALO_PIX; it += THREADS) {
        const int cg = it / HALO_PIX, p = it - cg * HALO_PIX;
        const int py = p / HALO_W, px = p - py * HALO_W;
        const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
        bf16x8 q;
#pragma unroll
        for (int c = 0; c < CPI; ++c) q[c] = (__bf16)0.f;
        if (Y >= 0 && Y < P.h && X >= 0 && X < P.w_) {
            const pvnc::Taps t(Y, X, P.ry, P.rx, P.hin, P.win);
            const int y0 = t.y0, y1 = t.y1, x0 = t.x0, x1 = t.x1;
            const int64_t base = (int64_t)bi * P.ls[0] + (int64_t)(c0 + cg * CPI) * P.ls[1];
            const int64_t o00 = base + (int64_t)y0 * P.ls[2] + (int64_t)x0 * P.ls[3], o01 = base + (int64_t)y0 * P.ls[2] + (int64_t)x1 * P.ls[3];
            const int64_t o10 = base + (int64_t)y1 * P.ls[2] + (int64_t)x0 * P.ls[3], o11 = base + (int64_t)y1 * P.ls[2] + (int64_t)x1 * P.ls[3];
#pragma unroll
            for (int c = 0; c < CPI; ++c) {
                const int64_t oc = (int64_t)c * P.ls[1];
                const float v00 = pvd::ld_elem<FT>(P.lo, o00 + oc), v01 = pvd::ld_elem<FT>(P.lo, o01 + oc);
                const float v10 = pvd::ld_elem<FT>(P.lo, o10 + oc), v11 = pvd::ld_elem<FT>(P.lo, o11 + oc);
                q[c] = (__bf16)t.blend(v00, v01, v10, v11);
            }
        }
        *reinterpret_cast<bf16x8*>(tile + rec_slot(p, cg)) = q;
    }
}

// channels c0 .. c0 + 31 of `skip` likewise
template <int FT>
__device__ __forceinline__ void stage_skip(const StageArgs& P, int bi, int ty0, int tx0, int c0, unsigned char* tile) {
    for (int it = threadIdx.x; it < GROUPS * HALO_PIX; it += THREADS) {
        const int cg = it / HALO_PIX, p = it - cg * HALO_PIX;
        const int py = p / HALO_W, px = p - py * HALO_W;
        const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
        bf16x8 q;
#pragma unroll
        for (int c = 0; c < CPI; ++c) q[c] = (__bf16)0.f;
        if (Y >= 0 && Y < P.h && X >= 0 && X < P.w_) {
            const int64_t o = (int64_t)bi * P.ss[0] + (int64_t)(c0 + cg * CPI) * P.ss[1] + (int64_t)Y * P.ss[2] + (int64_t)X * P.ss[3];
#pragma unroll
            for (int c = 0; c < CPI; ++c) q[c] = (__bf16)pvd::ld_elem<FT>(P.skip, o + (int64_t)c * P.ss[1]);
        }
        *reinterpret_cast<bf16x8*>(tile + rec_slot(p, cg)) = q;
    }
}

// chunk `chunk` of In (workgroup-uniform branches: the chunk and the types are the launch's)
template <int CL>
__device__ __forceinline__ void stage_chunk(const StageArgs& P, int bi, int ty0, int tx0, int chunk, unsigned char* tile) {
    if (chunk < CL / CHUNK) {
        if (P.lo_type == VT_BF16) stage_lo<VT_BF16>(P, bi, ty0, tx0, chunk * CHUNK, tile);
        else if (P.lo_type == VT_F16) stage_lo<VT_F16>(P, bi, ty0, tx0, chunk * CHUNK, tile);
        else stage_lo<VT_F32>(P, bi, ty0, tx0, chunk * CHUNK, tile);
    } else {
        const int c0 = chunk * CHUNK - CL;
        if (P.skip_type == VT_BF16) stage_skip<VT_BF16>(P, bi, ty0, tx0, c0, tile);
        else if (P.skip_type == VT_F16) stage_skip<VT_F16>(P, bi, ty0, tx0, c0, tile);
        else stage_skip<VT_F32>(P, bi, ty0, tx0, c0, tile);
    }
}

// the A fragment of (chunk, k-step ks = 2 tap + half, row block m): lane (r, hh) holds output channel 32 m + r, k = 8 hh + j, which is
// channel 32 chunk + 16 half + k of In at that tap
template <int CIN, int CO, bool PACKED>
__device__ __forceinline__ bf16x8 weights_fragment(const float* w, int chunk, int ks, int m, int lane) {
    if (PACKED) return reinterpret_cast<const bf16x8*>(w)[pvnc::frag_at(chunk * KSTEPS + ks, CO / 32, m, lane)];
    const float* wr = w + ((size_t)(32 * m + (lane & 31)) * CIN + CHUNK * chunk + 16 * (ks & 1) + 8 * (lane >> 5)) * 9 + (ks >> 1);
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (__bf16)wr[9 * j];
    return a;
}

// k-step ks = 2 tap + half of a chunk: CO / 32 weight fragments and the wave's two pixel fragments (`rec`: the record of the top-left
// tap of this lane's pixel of column block 0, at this lane half's eight channels), CO / 32 x 2 MFMAs
template <int CIN, int CO, bool PACKED>
__device__ __forceinline__ void k_step(const float* w, int chunk, int ks, int lane, const unsigned char* rec, f32x16 (&acc)[NQ][CO / 32]) {
    constexpr int MB = CO / 32;
    const int t = ks >> 1;
    bf16x8 A[MB], B[NQ];
#pragma unroll
    for (int m = 0; m < MB; ++m) A[m] = weights_fragment<CIN, CO, PACKED>(w, chunk, ks, m, lane);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        B[q] = *reinterpret_cast<const bf16x8*>(rec + ((t / 3) * HALO_W + t % 3 + 32 * q) * REC + 32 * (ks & 1));
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[q][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[m], B[q], acc[q][m], 0, 0, 0);
}

template <int CL, int CO, bool PACKED>
__global__ __launch_bounds__(THREADS) void decoder_stage_kernel(StageArgs P) {
    if constexpr (CO == 64) PVNET_SPARE_VGPRS(135);   // (122 in use: three workgroups per compute unit)
    else PVNET_SPARE_VGPRS(127);                      // (113 in use: four)
    constexpr int CIN = CL + CS, NCHUNK = CIN / CHUNK, MB = CO / 32;
    __shared__ __attribute__((aligned(16))) unsigned char tile[HALO_PIX * REC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const size_t plane = (size_t)P.h * P.w_;

    for (int t_ = blockIdx.x; t_ < P.ntiles; t_ += gridDim.x) {
        int bi, ty0, tx0;
        pvnc::tile_of<TILE_W, ROWS>(P, t_, bi, ty0, tx0);
        const int Y = ty0 + wave;
        f32x16 acc[NQ][MB];
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float bv = P.bias[32 * m + (g & 3) + 8 * (g >> 2) + 4 * hh];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q][m][g] = bv;
            }
#pragma unroll 1
        for (int chunk = 0; chunk < NCHUNK; ++chunk) {
            stage_chunk<CL>(P, bi, ty0, tx0, chunk, tile);
            __syncthreads();
            if (Y < P.h) {   // wave-uniform; the barriers are outside
                const unsigned char* rec = tile + (wave * HALO_W + r) * REC + 16 * hh;   // the top-left tap of this lane's pixel of block 0
                if constexpr (PACKED) {   // unrolled: the eighteen steps' fragment loads are in flight together
#pragma unroll
                    for (int ks = 0; ks < KSTEPS; ++ks) k_step<CIN, CO, PACKED>(P.w, chunk, ks, lane, rec, acc);
                } else {
#pragma unroll 1
                    for (int ks = 0; ks < KSTEPS; ++ks) k_step<CIN, CO, PACKED>(P.w, chunk, ks, lane, rec, acc);
                }
            }
            __syncthreads();   // the next chunk (or tile) overwrites the image
        }
        if (Y < P.h) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int X = tx0 + 32 * q + r;
                if (X >= P.w_) continue;
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    f32x16 v = acc[q][m];
#pragma unroll
                    for (int g = 0; g < 16; ++g) v[g] = pvnc::leaky(v[g]);
                    const size_t o = ((size_t)bi * CO + 32 * m) * plane + (size_t)Y * P.w_ + X;
                    if (P.out_type == VT_BF16) pvnc::store_rows<VT_BF16>(P.out, o, plane, v, hh);
                    else if (P.out_type == VT_F16) pvnc::store_rows<VT_F16>(P.out, o, plane, v, hh);
                    else pvnc::store_rows<VT_F32>(P.out, o, plane, v, hh);
                }
            }
        }
    }
}

template <int CL, int CO>
void launch(const StageArgs& P, bool packed, dim3 grid, hipStream_t s) {
    if (packed) hipLaunchKernelGGL((decoder_stage_kernel<CL, CO, true>), grid, dim3(THREADS), 0, s, P);
    else hipLaunchKernelGGL((decoder_stage_kernel<CL, CO, false>), grid, dim3(THREADS), 0, s, P);
}

}  // namespace
}  // namespace pvdec

using namespace pvdec;

extern "C" {

int pvnet_decoder_abi_version(void) { return PVNET_DECODER_ABI_VERSION; }

int pvnet_decoder_stage(const void* lo, int lo_type, const int64_t lo_strides[4], const void* skip, int skip_type,
                        const int64_t skip_strides[4], const float* w, const float* bias, int b, int hin, int win, int h, int w_, int cl,
                        int cs, int co, uint32_t flags, void* out, int out_type, void* stream) {
    if (!lo || !lo_strides || !skip || !skip_strides || !w || !bias || !out) return PVNET_E_BADARG;
    if (b < 1 || hin < 1 || win < 1 || h < 1 || w_ < 1 || cl < 1 || cs < 1 || co < 1) return PVNET_E_BADARG;
    if (!pvnc::type_ok(lo_type) || !pvnc::type_ok(skip_type) || !pvnc::type_ok(out_type)) return PVNET_E_BADARG;
    if ((flags & ~PVNET_DECODER_F_PACKED) != 0) return PVNET_E_BADARG;
    if ((flags & PVNET_DECODER_F_PACKED) && (reinterpret_cast<uintptr_t>(w) & 15) != 0) return PVNET_E_BADARG;   // 16-byte fragment loads
    if ((long long)h != 2ll * hin || (long long)w_ != 2ll * win) return PVNET_E_BADARG;
    const bool conv2s = cl == 64 && cs == CS && co == 32, conv4s = cl == 128 && cs == CS && co == 64;
    if (!conv2s && !conv4s) return PVNET_E_UNSUPPORTED;
    StageArgs P;
    if (!pvnc::sizes_ok(b, h, w_) || pvnc::plan_tiles<TILE_W, ROWS>(P, b, h, w_) < 0) return PVNET_E_UNSUPPORTED;
    P.lo = lo;
    P.skip = skip;
    P.w = w;
    P.bias = bias;
    P.out = out;
    for (int i = 0; i < 4; ++i) {
        P.ls[i] = lo_strides[i];
        P.ss[i] = skip_strides[i];
    }
    P.lo_type = lo_type;
    P.skip_type = skip_type;
    P.out_type = out_type;
    P.hin = hin;
    P.win = win;
    P.h = h;
    P.w_ = w_;
    P.ry = pvnc::up_ratio(hin, h);
    P.rx = pvnc::up_ratio(win, w_);
    const dim3 grid = pvnc::clamped_grid(P.ntiles, conv2s ? MAX_GRID_32 : MAX_GRID_64);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (flags & PVNET_DECODER_F_PACKED) != 0;
    if (conv2s) launch<64, 32>(P, packed, grid, s);
    else launch<128, 64>(P, packed, grid, s);
    return pvnc::launch_status();
}

}  // extern "C"
