// stem.hip -- libpvnet_stem.so: the network's stem in one launch (include/pvnet_stem.h holds the definition): 7 x 7 stride-2 convolution
// with the eval() BatchNorm folded in, ReLU, and the 3 x 3 stride-2 max-pool behind it.
//
// Path replaced (reference tree): conv1 + bn1 + relu + maxpool of ResNet.forward (lib/networks/resnet.py:138-142, 200-204) -- four
// eager kernels that write x2s, the largest activation of the trunk, and read it three more times.  Here the image is read once (with
// the tiles' halo) and x2s and the pooled tensor are written once.
//
// A workgroup (four waves) first writes the weights' fragments into LDS, then walks tiles of TILE_W x ROWS x2s pixels, tile =
// blockIdx.x, += gridDim.x.  The pool needs the x2s row above the tile and the column left of it: they are recomputed (CROWS x CCOLS
// computed pixels), bit for bit what their own tile stores, because a pixel is one column of the matrix product whatever lane it is on.
// Per tile
//   1. stage:   the input patch of the computed pixels -> LDS as bfloat16, [c][row][column], zero outside the image; its loads were
//               issued a tile earlier;
//   2. compute: per half m of the output channels, jobs over the waves: (row, column block of 32 pixels) and one block for the halo
//               column.  K = (c, ky) groups of 7 taps + 1 zero: a lane's B fragment is 16 bytes of a patch row from column 2 x (4-byte
//               aligned), its eighth value masked to zero bits; group 21 is zero in both operands.  The activated, rounded values go
//               into `pbuf` in the output type, +0 where the pixel is outside Ho x Wo;
//   3. store:   x2s from pbuf, eight pixels of a row per lane: 16-byte stores wherever the row's address allows them (storing from the
//               accumulators, a lane a pixel, took 2-byte stores: 512 store instructions per tile against 32);
//   4. pool:    the 3 x 3 maxima of pbuf's 32 channels -> pooled, as unsigned maxima of the values' bits (no value is below +0, so
//               the +0 of a position outside Ho x Wo never counts, and a NaN's bits are above every number's).
#include "net_common.h"

#include "pvnet_stem.h"

namespace pvstem {
namespace {

using pvd::bf16x8;
using pvd::f32x16;
using pvd::VT_BF16;
using pvd::VT_F16;
using pvd::VT_F32;

PVNET_NET_TYPE_CODES(STEM);

constexpr int CI = PVNET_STEM_CIN, CO = PVNET_STEM_COUT;
constexpr int TILE_W = 64, ROWS = 4;                  // x2s pixels of a tile; both even: a pool window never reaches below or right of it
constexpr int THREADS = 256;
constexpr int CROWS = ROWS + 1, CCOLS = TILE_W + 1;   // computed pixels: local row 0 is the row above the tile, local column 0 the one left of it
constexpr int PH = 2 * CROWS + 5;                     // rows of the input patch
constexpr int PWP = 2 * CCOLS + 6;                    // its columns, 2 * CCOLS + 5, and one more that only the masked eighth value reads
constexpr int GROUPS = CI * 7;                        // (c, ky) input rows of a window: 21, a k group of 8 each
constexpr int KSTEPS = (GROUPS + 2) / 2;              // of 16: 11, the 22nd group zero
constexpr int PB0 = 7, PBW = PB0 + CCOLS;             // a row of pbuf: local column 0 at PB0, so that every eight of the tile's own 64 are a 16-byte slot
constexpr int JOBS = 2 * CROWS + 1;                   // (row, column block) and the halo column's
constexpr int MAX_GRID = 512;                         // workgroups of a launch: two per compute unit (81 KB of LDS each at most)
static_assert(ROWS % 2 == 0 && TILE_W == 64 && CROWS <= 32 && PWP % 2 == 0 && PBW % 8 == 0, "the tile");

struct StemArgs {
    const void* image;
    const float* w;      // [64,3,7,7]
    const float* bias;
    void* x2s;
    void* pooled;        // or null
    int64_t is[4];
    int image_type;
    int h, w_, ho, wo, hp, wp;
    int tiles_x, tiles_y, ntiles;
};

// element (k group gi, tap 0) of a patch whose top-left element is the window's
__host__ __device__ constexpr int group_offset(int gi) { return ((gi / 7) * PH + gi % 7) * PWP; }

// sixteen bytes at a 4-byte aligned LDS address
struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t d[4];
};

// The patch of the tile whose computed pixels start at (cy0, cx0) of image bi: element (c, iy, ix) is In[c](2 cy0 - 3 + iy, 2 cx0 - 3 + ix).
// An item is two columns: a wave's loads run along an image row.  Staging is two steps, so that a tile's loads are in flight while the
// tile before it is computed: patch_load issues every load of a thread -- unconditional, from a position clamped into the image -- and
// patch_write rounds the values, zero outside the image, into LDS.
constexpr int STAGE_ITEMS = CI * PH * (PWP / 2), STAGE_ITERS = (STAGE_ITEMS + THREADS - 1) / THREADS;

template <int FT>
__device__ __forceinline__ void patch_load(const StemArgs& P, int bi, int cy0, int cx0, float (&v0)[STAGE_ITERS], float (&v1)[STAGE_ITERS]) {
    const int64_t base = (int64_t)bi * P.is[0];
#pragma unroll
    for (int k = 0; k < STAGE_ITERS; ++k) {
        const int it = min((int)threadIdx.x + k * THREADS, STAGE_ITEMS - 1);
        const int c = it / (PH * (PWP / 2)), rem = it - c * (PH * (PWP / 2));
        const int iy = rem / (PWP / 2), ix = 2 * (rem - iy * (PWP / 2));
        const int gy = 2 * cy0 - 3 + iy, gx = 2 * cx0 - 3 + ix;
        const int64_t row = base + (int64_t)c * P.is[1] + (int64_t)min(max(gy, 0), P.h - 1) * P.is[2];
        v0[k] = pvd::ld_elem<FT>(P.image, row + (int64_t)min(max(gx, 0), P.w_ - 1) * P.is[3]);
        v1[k] = pvd::ld_elem<FT>(P.image, row + (int64_t)min(max(gx + 1, 0), P.w_ - 1) * P.is[3]);
    }
}

__device__ __forceinline__ void patch_write(const StemArgs& P, int cy0, int cx0, const float (&v0)[STAGE_ITERS], const float (&v1)[STAGE_ITERS],
                                            __bf16* patch) {
#pragma unroll
    for (int k = 0; k < STAGE_ITERS; ++k) {
        const int it = (int)threadIdx.x + k * THREADS;
        if (it >= STAGE_ITEMS) break;
        const int c = it / (PH * (PWP / 2)), rem = it - c * (PH * (PWP / 2));
        const int iy = rem / (PWP / 2), ix = 2 * (rem - iy * (PWP / 2));
        const int gy = 2 * cy0 - 3 + iy, gx = 2 * cx0 - 3 + ix;
        const bool in_y = gy >= 0 && gy < P.h;
        pvd::bf16x2 q;
        q[0] = (__bf16)(in_y && gx >= 0 && gx < P.w_ ? v0[k] : 0.f);   // the one rounding of an image value; zero outside the image
        q[1] = (__bf16)(in_y && gx + 1 >= 0 && gx + 1 < P.w_ ? v1[k] : 0.f);
        *reinterpret_cast<pvd::bf16x2*>(patch + (c * PH + iy) * PWP + ix) = q;
    }
}

// the loads of tile t_ (workgroup-uniform branches: the type is the launch's)
__device__ __forceinline__ void tile_load(const StemArgs& P, int bi, int ty0, int tx0, float (&v0)[STAGE_ITERS], float (&v1)[STAGE_ITERS]) {
    if (P.image_type == VT_BF16) patch_load<VT_BF16>(P, bi, ty0 - 1, tx0 - 1, v0, v1);
    else if (P.image_type == VT_F16) patch_load<VT_F16>(P, bi, ty0 - 1, tx0 - 1, v0, v1);
    else patch_load<VT_F32>(P, bi, ty0 - 1, tx0 - 1, v0, v1);
}

// A barrier between phases that exchange data through LDS only: it waits for this wave's LDS operations, not for its global stores, which
// drain while the next phase runs (__syncthreads() would wait for them too).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
}

template <int OT>
__global__ __launch_bounds__(THREADS) void stem_kernel(StemArgs P) {
    PVNET_SPARE_VGPRS(247);   // (239 in use: the compiler spends what two waves per SIMD leave it; the LDS allows two workgroups per compute unit: two waves per SIMD, 256 registers each)
    typedef typename pvnc::elem<OT>::type T;
    __shared__ __attribute__((aligned(16))) __bf16 wfrag[2 * KSTEPS * 64 * 8];   // [m][k-step][lane][j]: the A fragments
    __shared__ __attribute__((aligned(16))) __bf16 patch[CI * PH * PWP];
    // the stored values' BITS, [channel of the half][local row][PB0 + local column]; +0 outside Ho x Wo.  Every value is +0 or above, or
    // a NaN, so the unsigned maximum of the bits is the maximum of the values, and a NaN (above every number's bits) wins it
    typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint16_t>::type U;
    typedef U ux8 __attribute__((ext_vector_type(8)));
    __shared__ __attribute__((aligned(32))) U pbuf[32 * CROWS * PBW];
    __shared__ float sbias[CO];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const bool pool = P.pooled != nullptr;
    const size_t plane = (size_t)P.ho * P.wo, pplane = (size_t)P.hp * P.wp;

    // the weights, rounded once, in fragment order: lane (r, hh) of k-step s holds output channel 32 m + r, k group 2 s + hh, taps 0 .. 6
    // and a zero; group 21 is zero.  (Loads unconditional and eleven in flight, as in stage_patch.)
    static_assert(2 * KSTEPS * 64 * 8 % (11 * THREADS) == 0, "the weights' loop");
#pragma unroll 1
    for (int i0 = threadIdx.x; i0 < 2 * KSTEPS * 64 * 8; i0 += 11 * THREADS) {
        float v[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const int i = i0 + k * THREADS;
            const int j = i & 7, l = (i >> 3) & 63, ms = i >> 9;
            const int gi = 2 * (ms % KSTEPS) + (l >> 5);
            v[k] = P.w[((32 * (ms / KSTEPS) + (l & 31)) * GROUPS + min(gi, GROUPS - 1)) * 7 + min(j, 6)];
        }
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const int i = i0 + k * THREADS;
            const int j = i & 7, l = (i >> 3) & 63, ms = i >> 9;
            const int gi = 2 * (ms % KSTEPS) + (l >> 5);
            wfrag[i] = (__bf16)(gi < GROUPS && j < 7 ? v[k] : 0.f);
        }
    }

    if (threadIdx.x < CO) sbias[threadIdx.x] = P.bias[threadIdx.x];

    float v0[STAGE_ITERS], v1[STAGE_ITERS];   // a tile's image values on their way into the patch
    if ((int)blockIdx.x < P.ntiles) {
        int bi, ty0, tx0;
        pvnc::tile_of<TILE_W, ROWS>(P, blockIdx.x, bi, ty0, tx0);
        tile_load(P, bi, ty0, tx0, v0, v1);
    }
    for (int t_ = blockIdx.x; t_ < P.ntiles; t_ += gridDim.x) {
        int bi, ty0, tx0;
        pvnc::tile_of<TILE_W, ROWS>(P, t_, bi, ty0, tx0);
        const int cy0 = ty0 - 1, cx0 = tx0 - 1;
        patch_write(P, cy0, cx0, v0, v1, patch);
        lds_barrier();   // (the first tile: the weights and the bias too)
        if (t_ + (int)gridDim.x < P.ntiles) {   // the next tile's loads, in flight while this one is computed
            int nb, ny0, nx0;
            pvnc::tile_of<TILE_W, ROWS>(P, t_ + gridDim.x, nb, ny0, nx0);
            tile_load(P, nb, ny0, nx0, v0, v1);
        }
#pragma unroll 1
        for (int m = 0; m < 2; ++m) {
#pragma unroll 1
            for (int job = (pool ? 0 : 2) + wave; job < (pool ? JOBS : JOBS - 1); job += 4) {   // wave-uniform; the barriers are outside
                const bool halo = job == JOBS - 1;
                const int yl = halo ? min(r, CROWS - 1) : job >> 1;
                const int xl = halo ? 0 : 1 + 32 * (job & 1) + r;
                const int Y = cy0 + yl, X = cx0 + xl;
                const bool outside = Y < 0 || Y >= P.ho || X < 0 || X >= P.wo;   // (an edge tile computes these too: pbuf is written whole)
                f32x16 acc;
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[g] = sbias[32 * m + (g & 3) + 8 * (g >> 2) + 4 * hh];
                const __bf16* win = patch + (2 * yl) * PWP + 2 * xl;   // the top-left element of this lane's window
                const __bf16* wf = wfrag + ((m * KSTEPS) * 64 + lane) * 8;
#pragma unroll
                for (int s = 0; s < KSTEPS; ++s) {
                    const bool zero = 2 * s + 1 >= GROUPS;   // the 22nd group: lane half 1 of the last step
                    const int off = hh && !zero ? group_offset(zero ? 0 : 2 * s + 1) : group_offset(2 * s);
                    Words4 raw = *reinterpret_cast<const Words4*>(win + off);
                    raw.d[3] &= 0xFFFFu;   // the eighth value is the next tap's column: zero bits, not an image value times a zero weight
                    if (zero && hh) raw.d[0] = raw.d[1] = raw.d[2] = raw.d[3] = 0u;
                    const bf16x8 B = __builtin_bit_cast(bf16x8, raw);
                    const bf16x8 A = *reinterpret_cast<const bf16x8*>(wf + s * 64 * 8);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc, 0, 0, 0);
                }
                if (!halo || r < CROWS) {
                    U* pb = pbuf + (4 * hh) * (CROWS * PBW) + yl * PBW + PB0 + xl;
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        const float v = acc[g];   // a NaN compares false and stays; -0 becomes +0; then the one rounding to the output type
                        pb[((g & 3) + 8 * (g >> 2)) * (CROWS * PBW)] = __builtin_bit_cast(U, (T)(v <= 0.f || outside ? 0.f : v));
                    }
                }
            }
            lds_barrier();
            // x2s, this half's 32 channels x ROWS x 64 pixels: an item is eight pixels of a row, one 16-byte store (two for float32)
            // where the row's address allows it -- a wave's stores cover eight whole rows of the tile
#pragma unroll 1
            for (int it = threadIdx.x; it < 32 * ROWS * (TILE_W / 8); it += THREADS) {
                const int cg = it & 7, row = (it >> 3) % ROWS, ch = it / (8 * ROWS);
                const int Y = ty0 + row, X0 = tx0 + 8 * cg;
                if (Y >= P.ho || X0 >= P.wo) continue;
                const ux8 q = *reinterpret_cast<const ux8*>(pbuf + (ch * CROWS + 1 + row) * PBW + PB0 + 1 + 8 * cg);
                U* o = reinterpret_cast<U*>(P.x2s) + ((size_t)bi * CO + 32 * m + ch) * plane + (size_t)Y * P.wo + X0;
                if (X0 + 8 <= P.wo && (reinterpret_cast<uintptr_t>(o) & (sizeof(ux8) - 1)) == 0) {
                    *reinterpret_cast<ux8*>(o) = q;
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (X0 + i < P.wo) o[i] = q[i];
                }
            }
            if (!pool) {
                lds_barrier();   // the next half (or tile) overwrites pbuf
                continue;
            }
            // the pooled pixels of this half: (channel, pooled row) pairs over the half waves, 32 consecutive pooled pixels per store
            const int xpl = threadIdx.x & 31, Xp = tx0 / 2 + xpl;
            if (Xp < P.wp) {
#pragma unroll 1
                for (int it = threadIdx.x >> 5; it < 32 * (ROWS / 2); it += THREADS / 32) {
                    const int ch = it / (ROWS / 2), ypl = it - ch * (ROWS / 2);
                    const int Yp = ty0 / 2 + ypl;
                    if (Yp >= P.hp) continue;
                    const U* pb = pbuf + ch * (CROWS * PBW) + (2 * ypl) * PBW + PB0 + 2 * xpl;   // the window's top-left
                    uint32_t best = 0;   // (+0: what a position outside Ho x Wo holds; the centre is always inside)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) best = max(best, (uint32_t)pb[ky * PBW + kx]);
                    reinterpret_cast<U*>(P.pooled)[((size_t)bi * CO + 32 * m + ch) * pplane + (size_t)Yp * P.wp + Xp] = (U)best;
                }
            }
            lds_barrier();   // the next half (or tile) overwrites pbuf
        }
    }
}

}  // namespace
}  // namespace pvstem

using namespace pvstem;

extern "C" {

int pvnet_stem_abi_version(void) { return PVNET_STEM_ABI_VERSION; }

int pvnet_stem_forward(const void* image, int image_type, const int64_t image_strides[4], const float* w, const float* bias, int b, int h,
                       int w_, void* x2s, void* pooled, int out_type, void* stream) {
    if (!image || !image_strides || !w || !bias || !x2s) return PVNET_E_BADARG;
    if (b < 1 || h < 1 || w_ < 1) return PVNET_E_BADARG;
    if (!pvnc::type_ok(image_type) || !pvnc::type_ok(out_type)) return PVNET_E_BADARG;
    if (!pvnc::sizes_ok(b, h, w_)) return PVNET_E_UNSUPPORTED;
    StemArgs P;
    P.h = h;
    P.w_ = w_;
    P.ho = (h - 1) / 2 + 1;
    P.wo = (w_ - 1) / 2 + 1;
    P.hp = (P.ho - 1) / 2 + 1;
    P.wp = (P.wo - 1) / 2 + 1;
    if (pvnc::plan_tiles<TILE_W, ROWS>(P, b, P.ho, P.wo) < 0) return PVNET_E_UNSUPPORTED;
    P.image = image;
    P.w = w;
    P.bias = bias;
    P.x2s = x2s;
    P.pooled = pooled;
    for (int i = 0; i < 4; ++i) P.is[i] = image_strides[i];
    P.image_type = image_type;
    const dim3 grid = pvnc::clamped_grid(P.ntiles, MAX_GRID);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (out_type == PVNET_STEM_T_BF16) hipLaunchKernelGGL((stem_kernel<VT_BF16>), grid, dim3(THREADS), 0, s, P);
    else if (out_type == PVNET_STEM_T_F16) hipLaunchKernelGGL((stem_kernel<VT_F16>), grid, dim3(THREADS), 0, s, P);
    else hipLaunchKernelGGL((stem_kernel<VT_F32>), grid, dim3(THREADS), 0, s, P);
    return pvnc::launch_status();
}

}  // extern "C"
