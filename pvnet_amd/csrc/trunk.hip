// trunk.hip -- libpvnet_trunk.so: one 3 x 3 convolution of the residual trunk in one launch (include/pvnet_trunk.h holds the
// definition): the convolution over one or two concatenated inputs with the eval() BatchNorm folded in, stride 1 or 2, dilation 1, 2
// or 4, and the residual addition and the activation applied to its own accumulators.
//
// Path replaced (reference tree): conv1 + bn1 + relu and conv2 + bn2 + add + relu of BasicBlock.forward (lib/networks/resnet.py:54-70),
// fc and cat + conv8s of Resnet18_8s (lib/networks/model_repository.py:17-33, 67) -- a convolution and up to five elementwise kernels
// each, which write and re-read the convolution's output.  Here the inputs are read once per group of output channels (with the tiles'
// receptive field) and the output written once.
//
// A workgroup (four waves) walks work items (group of COG = 128 output channels, tile of TILE_W x ROWS output pixels), item =
// blockIdx.x, += gridDim.x, the group slowest.  The decoder's loop (decoder.hip) with the waves turned from the tile's rows to the
// output channels: wave v owns the 32 channels 128 group + 32 v and ALL pixels of the tile -- ROWS accumulator blocks of 32 channels x
// 32 pixels -- so a weight fragment is loaded by one wave only and serves ROWS MFMAs.  Per chunk of 32 channels of In
//   1. stage:   the chunk of the tile's receptive field -> LDS, rounded to bfloat16, a pixel's 32 channels contiguous in a record of 80
//               bytes; zero outside the image (the convolution's padding).  Pixel p of the field is input pixel
//               (S ty0 - D + p / HALO_W, S tx0 - D + p % HALO_W).
//   2. compute: 18 k-steps (9 taps x 2 halves of the chunk): A = the wave's weight fragment, one 16-byte load per lane from the
//               fragment-order image (the workgroups in flight read the same group's: L2), B = one ds_read_b128 per lane and row of
//               the tile: output pixel (y, r) reads field pixel (S y + D ky, S r + D kx).
// then, per item, 3. epilogue: residual (one float32 addition), activation, one rounding, store: pixels are on the lanes, so a store
// instruction writes 32 consecutive pixels of a channel plane; any alignment of `out`.
// Step 1 exists twice per source type and geometry (stage_src's NEAR and FAR): 32-bit offsets from a scalar base for every source whose
// strides are non-negative and whose image spans less than 2^31 bytes, a 64-bit address per load for the rest (a negative stride through
// the C ABI, an image over 2 GB).  The second is there for the header's "any element strides", computes the same bits, keeps fewer
// loads in flight and has not been timed.
#include "net_common.h"

#include "pvnet_trunk.h"

// one rounding per operation: the header defines the residual addition and LeakyReLU's product as separate float32 operations
#pragma clang fp contract(off)

namespace pvtrunk {
namespace {

using pvd::bf16x8;
using pvd::f32x16;
using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;
using pvnc::CPI;
using pvnc::REC;

PVNET_NET_TYPE_CODES(TRUNK);

constexpr int CHUNK = 32;                 // channels of In staged at a time: two k-steps per tap
constexpr int TILE_W = 32, ROWS = 8;      // output pixels of a tile: one MFMA column block wide, an accumulator block per row
constexpr int WAVES = 4, THREADS = 64 * WAVES;
constexpr int COG = PVNET_TRUNK_CO_GROUP; // output channels of a work item: 32 per wave
static_assert(COG == 32 * WAVES, "a wave owns one row block of 32 output channels");
constexpr int GROUPS = CHUNK / CPI;       // staging items per pixel and chunk
constexpr int BATCH_NEAR = 5, BATCH_FAR = 2;   // staging items of a lane whose loads are in flight together (see stage_src)
constexpr int MAX_GRID = 2048;            // workgroups of a launch

struct ConvArgs {
    const void* src[2];
    const void* res;     // or null
    const bf16x8* w;     // the fragment-order bfloat16 image
    const float* bias;
    void* out;
    int64_t ss[2][4], rs[4];
    int src_type[2], res_type, out_type, act;
    int near[2];         // the source takes stage_src's 32-bit offsets
    int c1, nchunk, mb;  // channels of src1, chunks of In, row blocks of 32 output channels
    int h, w_, ho, wo;
    int tiles_x, tiles_y, ntiles, nitems;   // tiles of the batch; items = tiles x groups
};

// element at BYTE offset `off` of a workgroup-uniform base: a scalar base and a 32-bit lane offset, one address register per load
template <int VT>
__device__ __forceinline__ float ld_near(const char* base, uint32_t off) {
    if (VT == VT_F16) return (float)*reinterpret_cast<const _Float16*>(base + off);
    if (VT == VT_BF16) return __uint_as_float((uint32_t)*reinterpret_cast<const uint16_t*>(base + off) << 16);
    return *reinterpret_cast<const float*>(base + off);
}

// channels c0 .. c0 + 31 of a source, of the receptive field whose top-left input pixel is (iy0, ix0) of image bi -> LDS.  An item is
// (group of CPI channels, pixel), pixels fastest: a wave's loads of a plane run along a row.
// BATCH items at a time, all their loads issued before the first is used: a loop that waits for an item's eight loads before it issues
// the next item's spends the memory latency once per item.  No branch around a load: an item beyond the count or a pixel outside the
// image loads the nearest pixel of the image and is zeroed afterwards.
// NEAR (the host's choice: no negative stride and an image of the source spans less than 2^31 bytes): the addresses are the image's
// chunk, a scalar, plus a 32-bit byte offset, and BATCH_NEAR items are in flight; otherwise every load has a 64-bit address of its own
// and BATCH_FAR items are -- more would spill beside the 128 accumulator registers.
template <int FT, bool NEAR, int HALO_W, int HALO_PIX>
__device__ __forceinline__ void stage_src(const void* src, const int64_t (&st)[4], int h, int w_, int bi, int iy0, int ix0, int c0,
                                          unsigned char* field) {
    constexpr int N = GROUPS * HALO_PIX, ITERS = (N + THREADS - 1) / THREADS, BATCH = NEAR ? BATCH_NEAR : BATCH_FAR;
    constexpr uint32_t ES = FT == VT_F32 ? 4 : 2;
    const char* near = reinterpret_cast<const char*>(src) + ((int64_t)bi * st[0] + (int64_t)c0 * st[1]) * (int64_t)ES;
    const uint32_t n1 = (uint32_t)st[1] * ES, n2 = (uint32_t)st[2] * ES, n3 = (uint32_t)st[3] * ES;
    const char* plane[CPI];   // scalars: an item's eight loads share one offset register
#pragma unroll
    for (int c = 0; c < CPI; ++c) plane[c] = near + (int64_t)c * st[1] * (int64_t)ES;
#pragma unroll 1   // (unrolled, the batches' loads are hoisted together and spill)
    for (int k0 = 0; k0 < ITERS; k0 += BATCH) {
        float v[BATCH][CPI];
        int at[BATCH];   // the item's LDS offset, or -1: no store; bit 30: zeros
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            if (k0 + k >= ITERS) continue;
            const int it = threadIdx.x + (k0 + k) * THREADS, itc = min(it, N - 1);
            const int cg = itc / HALO_PIX, p = itc - cg * HALO_PIX;
            const int py = p / HALO_W, px = p - py * HALO_W;
            const int Y = iy0 + py, X = ix0 + px;
            const bool inside = Y >= 0 && Y < h && X >= 0 && X < w_;
            at[k] = it < N ? pvnc::rec_slot(p, cg) | (inside ? 0 : 1 << 30) : -1;
            const int Yc = min(max(Y, 0), h - 1), Xc = min(max(X, 0), w_ - 1);
            if constexpr (NEAR) {
                const uint32_t o = (uint32_t)(cg * CPI) * n1 + (uint32_t)Yc * n2 + (uint32_t)Xc * n3;
#pragma unroll
                for (int c = 0; c < CPI; ++c) v[k][c] = ld_near<FT>(plane[c], o);
            } else {
                const int64_t o = (int64_t)bi * st[0] + (int64_t)(c0 + cg * CPI) * st[1] + (int64_t)Yc * st[2] + (int64_t)Xc * st[3];
#pragma unroll
                for (int c = 0; c < CPI; ++c) v[k][c] = pvd::ld_elem<FT>(src, o + (int64_t)c * st[1]);
            }
        }
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            if (k0 + k >= ITERS) continue;
            bf16x8 q;
#pragma unroll
            for (int c = 0; c < CPI; ++c) q[c] = (at[k] & (1 << 30)) ? (__bf16)0.f : (__bf16)v[k][c];
            if (at[k] >= 0) *reinterpret_cast<bf16x8*>(field + (at[k] & ~(1 << 30))) = q;
        }
    }
}

template <int FT, int HALO_W, int HALO_PIX>
__device__ __forceinline__ void stage_typed(const ConvArgs& P, int which, int bi, int iy0, int ix0, int c0, unsigned char* field) {
    if (P.near[which]) stage_src<FT, true, HALO_W, HALO_PIX>(P.src[which], P.ss[which], P.h, P.w_, bi, iy0, ix0, c0, field);
    else stage_src<FT, false, HALO_W, HALO_PIX>(P.src[which], P.ss[which], P.h, P.w_, bi, iy0, ix0, c0, field);
}

// chunk `chunk` of In (workgroup-uniform branches: the chunk and the types are the launch's)
template <int HALO_W, int HALO_PIX>
__device__ __forceinline__ void stage_chunk(const ConvArgs& P, int bi, int iy0, int ix0, int chunk, unsigned char* field) {
    const int which = chunk * CHUNK >= P.c1;
    const int c0 = chunk * CHUNK - (which ? P.c1 : 0);
    const int t = P.src_type[which];
    if (t == VT_BF16) stage_typed<VT_BF16, HALO_W, HALO_PIX>(P, which, bi, iy0, ix0, c0, field);
    else if (t == VT_F16) stage_typed<VT_F16, HALO_W, HALO_PIX>(P, which, bi, iy0, ix0, c0, field);
    else stage_typed<VT_F32, HALO_W, HALO_PIX>(P, which, bi, iy0, ix0, c0, field);
}

__device__ __forceinline__ float activate(float v, int act) {
    if (act == PVNET_TRUNK_ACT_RELU) return v <= 0.f ? 0.f : v;   // a NaN compares false and stays; -0 becomes +0
    if (act == PVNET_TRUNK_ACT_LEAKY) return pvnc::leaky(v);
    return v;
}

template <int S, int D>
__global__ __launch_bounds__(THREADS, S == 2 ? 1 : 2) void conv3x3_kernel(ConvArgs P) {
    if constexpr (S == 2) PVNET_SPARE_VGPRS(223);   // (216 in use; its 88 KB of LDS admit one workgroup per compute unit anyway)
    else PVNET_SPARE_VGPRS(239);                    // (231 in use at most, 240 allocated: two workgroups' waves per SIMD)
    constexpr int HALO_W = S * (TILE_W - 1) + 2 * D + 1, HALO_H = S * (ROWS - 1) + 2 * D + 1, HALO_PIX = HALO_W * HALO_H;
    __shared__ __attribute__((aligned(16))) unsigned char field[HALO_PIX * REC];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const size_t plane = (size_t)P.ho * P.wo;

    for (int item = blockIdx.x; item < P.nitems; item += gridDim.x) {
        const int group = item / P.ntiles, t_ = item - group * P.ntiles;
        int bi, ty0, tx0;
        pvnc::tile_of<TILE_W, ROWS>(P, t_, bi, ty0, tx0);
        const int m = group * WAVES + wave;   // this wave's row block of output channels
        const bool active = m < P.mb;         // wave-uniform; the barriers are outside
        f32x16 acc[ROWS];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const float bv = active ? P.bias[32 * m + (g & 3) + 8 * (g >> 2) + 4 * hh] : 0.f;
#pragma unroll
            for (int y = 0; y < ROWS; ++y) acc[y][g] = bv;
        }
        // The weights go a ROW OF TAPS at a time (six k-steps, ks = 2 tap + half; row `row` = 3 chunk + ky of the item's 3 nchunk): the
        // next row's six fragments are loaded behind this row's 48 MFMAs, the first row of the next chunk before that chunk is staged.
        // Not unrolled further: eighteen fragments beside the 128 accumulator registers would spill.
        const size_t kstride = pvnc::frag_at((size_t)1, P.mb, 0, 0);   // a k-step of the weights' image
        const bf16x8* wf = P.w + pvnc::frag_at((size_t)0, P.mb, active ? m : 0, lane);   // (a wave without channels loads row block 0's and uses nothing)
        const int last_row = 3 * P.nchunk - 1;
        bf16x8 A[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = wf[(size_t)k * kstride];
#pragma unroll 1
        for (int chunk = 0; chunk < P.nchunk; ++chunk) {
            stage_chunk<HALO_W, HALO_PIX>(P, bi, S * ty0 - D, S * tx0 - D, chunk, field);
            __syncthreads();
            if (active) {
                const unsigned char* rec = field + (S * r) * REC + 16 * hh;   // the top-left tap of this lane's pixel of row 0
#pragma unroll 1
                for (int ky = 0; ky < 3; ++ky) {
                    const int next = min(3 * chunk + ky + 1, last_row);   // (the last row loads itself again: no branch around the loads)
                    bf16x8 N[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) N[k] = wf[(size_t)(6 * next + k) * kstride];
                    const unsigned char* row = rec + (D * ky * HALO_W) * REC;
#pragma unroll
                    for (int k = 0; k < 6; ++k)
#pragma unroll
                        for (int y = 0; y < ROWS; ++y)
                            acc[y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                A[k], *reinterpret_cast<const bf16x8*>(row + (S * y * HALO_W + D * (k >> 1)) * REC + 32 * (k & 1)), acc[y], 0, 0, 0);
#pragma unroll
                    for (int k = 0; k < 6; ++k) A[k] = N[k];
                }
            }
            __syncthreads();   // the next chunk (or item) overwrites the field
        }
        const int X = tx0 + r;
        if (active && X < P.wo) {
#pragma unroll
            for (int y = 0; y < ROWS; ++y) {
                const int Y = ty0 + y;
                if (Y >= P.ho) break;
                f32x16 v = acc[y];
                if (P.res) {
                    const int64_t ro = (int64_t)bi * P.rs[0] + (int64_t)(32 * m + 4 * hh) * P.rs[1] + (int64_t)Y * P.rs[2] + (int64_t)X * P.rs[3];
#pragma unroll
                    for (int g = 0; g < 16; ++g)
                        v[g] = v[g] + pvd::ld_elem_rt(P.res_type, P.res, ro + (int64_t)((g & 3) + 8 * (g >> 2)) * P.rs[1]);
                }
#pragma unroll
                for (int g = 0; g < 16; ++g) v[g] = activate(v[g], P.act);
                const size_t o = ((size_t)bi * (32 * P.mb) + 32 * m) * plane + (size_t)Y * P.wo + X;
                if (P.out_type == VT_BF16) pvnc::store_rows<VT_BF16>(P.out, o, plane, v, hh);
                else if (P.out_type == VT_F16) pvnc::store_rows<VT_F16>(P.out, o, plane, v, hh);
                else pvnc::store_rows<VT_F32>(P.out, o, plane, v, hh);
            }
        }
    }
}

// whether the byte offsets inside one image of a [*, c, h, w] tensor are non-negative and below 2^31
inline int near_ok(const int64_t st[4], int type, int c, int h, int w) {
    if (st[1] < 0 || st[2] < 0 || st[3] < 0) return 0;
    const long double span = ((long double)(c - 1) * st[1] + (long double)(h - 1) * st[2] + (long double)(w - 1) * st[3] + 1) *
                             (type == PVNET_TRUNK_T_F32 ? 4 : 2);
    return span < 2147483648.0L;
}

}  // namespace
}  // namespace pvtrunk

using namespace pvtrunk;

extern "C" {

int pvnet_trunk_abi_version(void) { return PVNET_TRUNK_ABI_VERSION; }

int pvnet_conv3x3_fused(const void* src1, int src1_type, const int64_t src1_strides[4], const void* src2, int src2_type,
                        const int64_t src2_strides[4], const void* res, int res_type, const int64_t res_strides[4], const void* w,
                        const float* bias, int b, int h, int w_, int c1, int c2, int co, int stride, int dilation, int act, void* out,
                        int out_type, void* stream) {
    if (!src1 || !src1_strides || !w || !bias || !out) return PVNET_E_BADARG;
    if ((src2 != nullptr) != (c2 != 0) || (src2 && !src2_strides) || (res && !res_strides)) return PVNET_E_BADARG;
    if (b < 1 || h < 1 || w_ < 1 || c1 < 1 || c2 < 0 || co < 1 || stride < 1 || dilation < 1) return PVNET_E_BADARG;
    using pvnc::type_ok;
    if (!type_ok(src1_type) || (src2 && !type_ok(src2_type)) || (res && !type_ok(res_type)) || !type_ok(out_type)) return PVNET_E_BADARG;
    if (act != PVNET_TRUNK_ACT_NONE && act != PVNET_TRUNK_ACT_RELU && act != PVNET_TRUNK_ACT_LEAKY) return PVNET_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(w) & 15) != 0) return PVNET_E_BADARG;   // 16-byte fragment loads
    if (c1 % CHUNK || c2 % CHUNK || (long long)c1 + c2 > PVNET_TRUNK_MAX_WIDTH || co % 32 || co > PVNET_TRUNK_MAX_WIDTH)
        return PVNET_E_UNSUPPORTED;
    const int geometry = stride == 1 && dilation == 1 ? 0 : stride == 2 && dilation == 1 ? 1 : stride == 1 && dilation == 2 ? 2 :
                         stride == 1 && dilation == 4 ? 3 : -1;
    if (geometry < 0) return PVNET_E_UNSUPPORTED;
    if (!pvnc::sizes_ok(b, h, w_)) return PVNET_E_UNSUPPORTED;
    ConvArgs P;
    P.ho = (h - 1) / stride + 1;
    P.wo = (w_ - 1) / stride + 1;
    const long long nitems = pvnc::plan_tiles<TILE_W, ROWS>(P, b, P.ho, P.wo, (co + COG - 1) / COG);
    if (nitems < 0) return PVNET_E_UNSUPPORTED;
    P.nitems = (int)nitems;
    P.src[0] = src1;
    P.src[1] = src2;
    P.res = res;
    P.w = static_cast<const bf16x8*>(w);
    P.bias = bias;
    P.out = out;
    for (int i = 0; i < 4; ++i) {
        P.ss[0][i] = src1_strides[i];
        P.ss[1][i] = src2 ? src2_strides[i] : 0;
        P.rs[i] = res ? res_strides[i] : 0;
    }
    P.near[0] = near_ok(src1_strides, src1_type, c1, h, w_);
    P.near[1] = src2 ? near_ok(src2_strides, src2_type, c2, h, w_) : 0;
    P.src_type[0] = src1_type;
    P.src_type[1] = src2 ? src2_type : PVNET_TRUNK_T_F32;
    P.res_type = res ? res_type : PVNET_TRUNK_T_F32;
    P.out_type = out_type;
    P.act = act;
    P.c1 = c1;
    P.nchunk = (c1 + c2) / CHUNK;
    P.mb = co / 32;
    P.h = h;
    P.w_ = w_;
    const dim3 grid = pvnc::clamped_grid(P.nitems, MAX_GRID);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (geometry == 0) hipLaunchKernelGGL((conv3x3_kernel<1, 1>), grid, dim3(THREADS), 0, s, P);
    else if (geometry == 1) hipLaunchKernelGGL((conv3x3_kernel<2, 1>), grid, dim3(THREADS), 0, s, P);
    else if (geometry == 2) hipLaunchKernelGGL((conv3x3_kernel<1, 2>), grid, dim3(THREADS), 0, s, P);
    else hipLaunchKernelGGL((conv3x3_kernel<1, 4>), grid, dim3(THREADS), 0, s, P);
    return pvnc::launch_status();
}

}  // extern "C"
