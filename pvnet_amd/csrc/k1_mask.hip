// k1_mask.hip -- K1: mask (any integer dtype / float32 / class logits, any strides) -> one bit per pixel, segment counts, thinning histograms
// (part of libpvnet_vote.so; the stage map is at the top of vote_host.hip, the shared definitions in vote_common.h)
#include "vote_common.h"

namespace pvd {
namespace {

// ------------------------------------------------------------------------------------------------------------
// K1: mask -> bit mask + foreground count                     (ransac_voting_gpu.py:527-528)
// ------------------------------------------------------------------------------------------------------------
// (the mask's elements through a generic pointer, or through one known to be global memory: scalar_ptr() below)
typedef const __attribute__((address_space(1))) char* gptr_t;
template <typename T> __device__ __forceinline__ const T* elems(const void* m) { return reinterpret_cast<const T*>(m); }
template <typename T> __device__ __forceinline__ const __attribute__((address_space(1))) T* elems(gptr_t m) {
    return (const __attribute__((address_space(1))) T*)m;
}
template <int DT, typename PTR>
__device__ __forceinline__ bool load_fg(PTR m, int64_t off) {
    if (DT == PVNET_MASK_U8) return elems<uint8_t>(m)[off] != 0;
    if (DT == PVNET_MASK_I16) return (elems<uint16_t>(m)[off] & 0xFFu) != 0;
    if (DT == PVNET_MASK_I32) return (elems<uint32_t>(m)[off] & 0xFFu) != 0;
    if (DT == PVNET_MASK_I64)  // read once, never again: non-temporal (keeps the 78 MB of a batch out of L2 / MALL)
        return ((uint32_t)__builtin_nontemporal_load(elems<uint64_t>(m) + off) & 0xFFu) != 0;
    const float v = elems<float>(m)[off];  // torch .byte() of a float: truncate, wrap
    return (static_cast<long long>(v) & 0xFF) != 0;
}

// wave 0 of a K1 workgroup: inclusive prefix over the segment's histogram of thinning bins -- cum[k - 1] = pixels kept at threshold k
__device__ __forceinline__ void thin_hist_prefix(const VoteParams& P, int bi, const int* s_hist, int lane) {
    constexpr int PER = THIN_BINS / 64;  // consecutive bins per lane
    int h[PER], mine = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        mine += s_hist[PER * lane + i];
        h[i] = mine;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    const int e = incl - mine;
    uint16_t* dst = P.cum + ((size_t)bi * P.nseg + blockIdx.x) * THIN_BINS + PER * lane;
#pragma unroll
    for (int i = 0; i < PER; i += 2)
        *reinterpret_cast<uint32_t*>(dst + i) = (uint32_t)(e + h[i]) | ((uint32_t)(e + h[i + 1]) << 16);
}

// A wave's loads of a FULL segment (every segment but an image's last, decided once per workgroup) leave from one scalar address
// per wave -- advanced by a constant per load -- plus one 32-bit vector offset, with no bound test: they are issued back to back and
// are in flight together.  (Round 13: a bound test per lane and load put every load into an exec-masked branch of its own with a
// 64-bit vector address rebuilt in front of it and a wait for it right behind -- 13 to 19 vector instructions per load.)
// The foreground test of a pixel is one 32-bit compare of the low byte whose result IS the ballot word (a scalar pair): no 0 / 1
// value is kept per pixel, and the thinning histogram takes its per-lane predicates back from the ballot words.
__device__ __forceinline__ gptr_t scalar_ptr(const char* base, uint32_t bytes) {   // base + bytes, both wave-uniform, as ONE scalar address:
    uint64_t a = reinterpret_cast<uint64_t>(base) + bytes;   // opaque, so that the constant cannot join the load's vector offset, where it
    asm("" : "+s"(a));                                       // costs a 64-bit vector add per load
    return reinterpret_cast<gptr_t>(a);
}
__device__ __forceinline__ bool lane_bit(unsigned long long m, int lane) { return ((m >> lane) & 1ull) != 0; }

template <int DT>
__global__ __launch_bounds__(64 * K1_WAVES) void mask_bits_kernel(VoteParams P) {
    PVNET_SPARE_VGPRS(39);
    small_stage_prio();
    const int bi = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // Round 5 (tools/ubench_hbm_read.hip, profiles/r05_ubench_mask_kernel.txt): load i of the workgroup's waves covers ONE contiguous
    // 512 * K1_WAVES bytes -- wave w takes the segment's words w, w + K1_WAVES, ... -- instead of every wave walking its own 4 KB
    // (-1.5 us), and the 64 bit words of the segment leave as one coalesced 512-byte store by wave 0 behind the barrier the count
    // needs anyway, instead of as 64 one-lane stores (-2 us).
    const int seg_word0 = blockIdx.x * SEG_WORDS;
    auto word_of = [&](int i) { return seg_word0 + wave + i * K1_WAVES; };
    constexpr int ESIZE = DT == PVNET_MASK_U8 ? 1 : DT == PVNET_MASK_I16 ? 2 : DT == PVNET_MASK_I64 ? 8 : 4;
    unsigned long long m[K1_WORDS_PER_WAVE];
    if (DT != PVNET_MASK_LOGITS_F32 && P.mask_linear && (seg_word0 + SEG_WORDS) * 64 <= P.npix) {   // workgroup-uniform: a full segment
        const char* wbase = reinterpret_cast<const char*>(P.mask) + ((int64_t)bi * P.ms0 + (int64_t)word_of(0) * 64) * ESIZE;
        bool f[K1_WORDS_PER_WAVE];
#pragma unroll
        for (int i = 0; i < K1_WORDS_PER_WAVE; ++i) f[i] = load_fg<DT>(scalar_ptr(wbase, i * (K1_WAVES * 64 * ESIZE)), (uint32_t)lane);
#pragma unroll
        for (int i = 0; i < K1_WORDS_PER_WAVE; ++i) m[i] = __ballot(f[i]);
    } else {
#pragma unroll
        for (int i = 0; i < K1_WORDS_PER_WAVE; ++i) {
            const int p = word_of(i) * 64 + lane;
            bool v = false;
            if (p < P.npix) {
                int64_t off;
                if (P.mask_linear) {
                    off = (int64_t)bi * P.ms0 + p;
                } else {
                    const int y = p / P.w, x = p - y * P.w;
                    off = (int64_t)bi * P.ms0 + (int64_t)y * P.ms1 + (int64_t)x * P.ms2;
                }
                if (DT == PVNET_MASK_LOGITS_F32) {  // fused torch.argmax(seg_pred, 1) (tools/demo.py:52): first maximum wins
                    // torch's rule for NaN: it counts as the maximum -- a NaN replaces a number, a later NaN never an earlier one.
                    // take = x > best || (x is NaN && best is not), as two compares and a select: `||` compiled to a branch per class
                    float best = ld_elem_rt(P.logits_type, P.mask, off);
                    int arg = 0;
                    for (int c = 1; c < P.num_classes; ++c) {
                        const float x = ld_elem_rt(P.logits_type, P.mask, off + (int64_t)c * P.ms_c);
                        const bool take = (best == best) & !(x <= best);
                        best = take ? x : best;
                        arg = take ? c : arg;
                    }
                    v = (arg & 0xFF) != 0;  // then .byte() != 0 (ransac_voting_gpu.py:527)
                } else {
                    v = load_fg<DT>(P.mask, off);
                }
            }
            m[i] = __ballot(v);
        }
    }
    int cnt = 0;
    __shared__ unsigned long long s_words[SEG_WORDS];
#pragma unroll
    for (int i = 0; i < K1_WORDS_PER_WAVE; ++i) cnt += __popcll(m[i]);
    __shared__ int s_cnt[K1_WAVES];
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < K1_WORDS_PER_WAVE; ++i) s_words[wave + i * K1_WAVES] = m[i];
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (wave == 0 && seg_word0 + lane < P.words) P.bits[(size_t)bi * P.words + seg_word0 + lane] = s_words[lane];
    if (P.cum == nullptr && wave != 0) return;  // (wave-uniform: without thinning tables only the segment count is left to write)
    int t = 0;
#pragma unroll
    for (int i = 0; i < K1_WAVES; ++i) t += s_cnt[i];
    if (threadIdx.x == 0) P.seg0[bi * P.nseg + blockIdx.x] = t;  // foreground pixels of this 4096-pixel segment (tn0 = their sum)

    // Thinning (ransac_voting_gpu.py:537-540) keeps a pixel when the bin of its random word (pvnet_thin_bin) is below
    // K = pvnet_thin_bins_kept(max_num, tn0) -- but tn0 is only known when every segment has been counted.  So a segment
    // WITH foreground (one in ten) also counts how many of its pixels EVERY possible k would keep (a cumulative histogram
    // of those bits, 2 KB), and the compaction kernel, which sums the segment counts anyway, picks its column: no separate
    // thinning launch.  Only when thinning can happen at all (max_num < h*w: P.cum is set).
    if (P.cum == nullptr || t == 0) return;  // block-uniform
    __shared__ int s_hist[THIN_BINS];
    for (int i = threadIdx.x; i < THIN_BINS; i += 64 * K1_WAVES) s_hist[i] = 0;
    __syncthreads();
    const uint32_t key = pvnet_rng_key(P.seed, PVNET_TAG_SUB, (uint32_t)(P.image_base + bi));
#pragma unroll
    for (int i = 0; i < K1_WORDS_PER_WAVE; ++i)
        if (lane_bit(m[i], lane)) atomicAdd(&s_hist[pvnet_thin_bin(pvnet_rng_at(key, (uint32_t)(word_of(i) * 64 + lane)))], 1);
    __syncthreads();
    if (wave == 0) thin_hist_prefix(P, bi, s_hist, lane);
}

// K1 for contiguous, 16-byte aligned int64 masks -- what torch.argmax delivers (tools/demo.py:52) and what the benchmark times: ONE
// 16-byte load brings two pixels per lane (a bare read of this size takes 15.4 us that way against 18.6 with 8-byte loads,
// profiles/r05_ubench_mask_kernel.txt).  A wave's ballots then hold the even and the odd pixels of a 128-pixel double word; wave 0
// interleaves them into the segment's 64 bit words behind the barrier and stores those as one coalesced 512 bytes.  Same outputs
// as mask_bits_kernel<PVNET_MASK_I64>: bit words, segment count, thinning histogram.
__device__ __forceinline__ uint32_t spread16(uint32_t x) {   // bit k of x (x < 65536) -> bit 2 k
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
__global__ __launch_bounds__(64 * K1_WAVES) void mask_bits_pair_kernel(VoteParams P) {
    PVNET_SPARE_VGPRS(39);
    small_stage_prio();
    constexpr int DW = SEG_WORDS / 2;     // double words (128 pixels) per segment
    constexpr int DPW = DW / K1_WAVES;    // per wave
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    const int bi = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int seg_word0 = blockIdx.x * SEG_WORDS;
    const uint64_t* image = reinterpret_cast<const uint64_t*>(P.mask) + (int64_t)bi * P.ms0;
    auto pixel_of = [&](int i) { return (blockIdx.x * DW + wave + i * K1_WAVES) * 128 + 2 * lane; };   // (load i of the waves: 1 KB * K1_WAVES contiguous)
    unsigned long long me[DPW], mo[DPW];   // the even / the odd pixels of the wave's double words: the ballots
    if ((seg_word0 + SEG_WORDS) * 64 <= P.npix) {   // workgroup-uniform: a full segment
        const char* wbase = reinterpret_cast<const char*>(image + (int64_t)(blockIdx.x * DW + wave) * 128);
        u64x2 v[DPW];
#pragma unroll
        for (int i = 0; i < DPW; ++i)
            v[i] = __builtin_nontemporal_load(elems<u64x2>(scalar_ptr(wbase, i * (K1_WAVES * 1024)) + (uint32_t)(lane * 16)));
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            me[i] = __ballot(((uint32_t)v[i].x & 0xFFu) != 0u);   // .byte() != 0 (ransac_voting_gpu.py:527)
            mo[i] = __ballot(((uint32_t)v[i].y & 0xFFu) != 0u);
        }
    } else {   // an image's last segment: the bound per lane
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            const int p = pixel_of(i);
            uint32_t lo = 0u, hi = 0u;
            if (p < P.npix) {   // (npix is even here: p + 1 < npix too)
                const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(image) + (p >> 1));
                lo = (uint32_t)v.x, hi = (uint32_t)v.y;
            }
            me[i] = __ballot((lo & 0xFFu) != 0u);
            mo[i] = __ballot((hi & 0xFFu) != 0u);
        }
    }
    int cnt = 0;
    __shared__ u64x2 s_eo[DW];   // (even, odd) per double word
#pragma unroll
    for (int i = 0; i < DPW; ++i) cnt += __popcll(me[i]) + __popcll(mo[i]);
    __shared__ int s_cnt[K1_WAVES];
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < DPW; ++i) s_eo[wave + i * K1_WAVES] = u64x2{me[i], mo[i]};
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (wave == 0 && seg_word0 + lane < P.words) {   // word `lane` of the segment: half of a double word, even and odd pixels interleaved
        const u64x2 eo = s_eo[lane >> 1];
        const uint32_t e32 = (lane & 1) ? (uint32_t)(eo.x >> 32) : (uint32_t)eo.x, o32 = (lane & 1) ? (uint32_t)(eo.y >> 32) : (uint32_t)eo.y;
        const uint32_t wlo = spread16(e32 & 0xFFFFu) | (spread16(o32 & 0xFFFFu) << 1), whi = spread16(e32 >> 16) | (spread16(o32 >> 16) << 1);
        P.bits[(size_t)bi * P.words + seg_word0 + lane] = (unsigned long long)wlo | ((unsigned long long)whi << 32);
    }
    if (P.cum == nullptr && wave != 0) return;  // (wave-uniform: without thinning tables only the segment count is left to write)
    int t = 0;
#pragma unroll
    for (int i = 0; i < K1_WAVES; ++i) t += s_cnt[i];
    if (threadIdx.x == 0) P.seg0[bi * P.nseg + blockIdx.x] = t;
    if (P.cum == nullptr || t == 0) return;  // block-uniform: the thinning histogram, as in mask_bits_kernel
    __shared__ int s_hist[THIN_BINS];
    for (int i = threadIdx.x; i < THIN_BINS; i += 64 * K1_WAVES) s_hist[i] = 0;
    __syncthreads();
    const uint32_t key = pvnet_rng_key(P.seed, PVNET_TAG_SUB, (uint32_t)(P.image_base + bi));
#pragma unroll
    for (int i = 0; i < DPW; ++i) {
        if (lane_bit(me[i], lane)) atomicAdd(&s_hist[pvnet_thin_bin(pvnet_rng_at(key, (uint32_t)pixel_of(i)))], 1);
        if (lane_bit(mo[i], lane)) atomicAdd(&s_hist[pvnet_thin_bin(pvnet_rng_at(key, (uint32_t)pixel_of(i) + 1u))], 1);
    }
    __syncthreads();
    if (wave == 0) thin_hist_prefix(P, bi, s_hist, lane);
}


}  // namespace

int launch_mask_bits(const VoteParams& P, hipStream_t s) {
    dim3 grid(P.nseg, P.b);
    switch (P.mask_dtype) {
        case PVNET_MASK_U8: hipLaunchKernelGGL(mask_bits_kernel<PVNET_MASK_U8>, grid, dim3(64 * K1_WAVES), 0, s, P); break;
        case PVNET_MASK_I16: hipLaunchKernelGGL(mask_bits_kernel<PVNET_MASK_I16>, grid, dim3(64 * K1_WAVES), 0, s, P); break;
        case PVNET_MASK_I32: hipLaunchKernelGGL(mask_bits_kernel<PVNET_MASK_I32>, grid, dim3(64 * K1_WAVES), 0, s, P); break;
        case PVNET_MASK_I64:
            // contiguous images at 16-byte aligned addresses, an even number of pixels: two pixels per 16-byte load
            if (P.mask_linear && (reinterpret_cast<uintptr_t>(P.mask) & 15u) == 0 && (P.ms0 & 1) == 0 && (P.npix & 1) == 0)
                hipLaunchKernelGGL(mask_bits_pair_kernel, grid, dim3(64 * K1_WAVES), 0, s, P);
            else
                hipLaunchKernelGGL(mask_bits_kernel<PVNET_MASK_I64>, grid, dim3(64 * K1_WAVES), 0, s, P);
            break;
        case PVNET_MASK_F32: hipLaunchKernelGGL(mask_bits_kernel<PVNET_MASK_F32>, grid, dim3(64 * K1_WAVES), 0, s, P); break;
        case PVNET_MASK_LOGITS_F32: hipLaunchKernelGGL(mask_bits_kernel<PVNET_MASK_LOGITS_F32>, grid, dim3(64 * K1_WAVES), 0, s, P); break;
        default: return PVNET_E_BADARG;
    }
    return 0;
}

}  // namespace pvd
