// class_split.hip -- libpvnet_classes.so: the voting layer's first kernel for a mask of class LABELS (include/pvnet_classes.h).
//
// Path replaced (reference tree): the `cur_mask = mask[bi] == k + 1` / torch.sum / uniform_ selection at the head of
// ransac_voting_layer_v2's class loop (lib/ransac_voting_gpu_layer/ransac_voting_gpu.py:116-131), for every class of every image at
// once.  A class of an image is a VIRTUAL IMAGE v = i * (num_classes - 1) + k of libpvnet_vote.so: this kernel writes what its mask
// kernel (k1_mask.hip) writes for the mask `labels[i] == k + 1` -- bit words, segment counts, thinning histograms -- and
// pvnet_vote_v3_prepared runs the rest of the layer on them.  Nothing here is linked from that library; vote_common.h and
// pvnet_rng.h give the one definition of the segment size, THIN_BINS, pvnet_thin_bin and the RNG key.
//
// One workgroup per 4096-pixel segment of a SOURCE image (the mask kernel's shape: K1_WAVES waves, load i of the waves covers one
// contiguous stretch), every label loaded exactly once.  Per 64-pixel word a wave peels off the classes present: the label of the
// first remaining lane (a scalar), one ballot of `label == c`, those lanes cleared -- as many ballots as the word has distinct
// classes, usually one or two.  The words of all classes collect in LDS ([num_classes - 1][64] u64, zeroed while the loads are in
// flight); behind the one barrier every class's 64 words leave as one coalesced 512-byte store, ZERO WORDS INCLUDED (nothing
// zero-fills the workspace), and their popcounts are the class's segment count.  The 6 KB thinning histogram is built and
// prefix-summed only for the classes that have pixels in this segment (a block-uniform loop): the compaction kernel reads `cum` only
// where the segment count is positive.
#include "vote_common.h"

#include "pvnet_classes.h"

namespace pvd {
namespace {

static_assert(PVNET_CLASSES_LOGITS_F32 == VT_F32 && PVNET_CLASSES_LOGITS_F16 == VT_F16 && PVNET_CLASSES_LOGITS_BF16 == VT_BF16,
              "the logits type codes of pvnet_classes.h are ld_elem_rt's");
static_assert((PVNET_CLASSES_MAX - 1) * SEG_WORDS * 8 + THIN_BINS * 4 + PVNET_CLASSES_MAX * 4 <= 40 * 1024,
              "four workgroups per compute unit: 40 KB of LDS each at most");

constexpr int CS_LOGITS = PVNET_MASK_F32 + 1;   // label source codes: PVNET_MASK_U8 .. PVNET_MASK_F32, then the class logits

struct ClassParams {
    const void* labels;
    int64_t ms0, ms1, ms2, ms_c;
    int linear, logits_type, num_classes;   // num_classes counts the background: labels 1 .. num_classes - 1 are classes
    int npix, w, words, nseg;
    uint64_t seed;
    int image_base;
    uint64_t* bits;
    int32_t* seg0;
    uint16_t* cum;   // NULL when max_num >= h * w: no call on this workspace thins
};

__device__ __forceinline__ int class_of(long long v, int nc) { return (v >= 1 && v < (long long)nc) ? (int)v : 0; }

// the class of the pixel at element offset `off`: 1 .. nc - 1, or 0 for "nobody's" (compared on the label's full value)
template <int DT>
__device__ __forceinline__ int load_class(const ClassParams& P, int64_t off) {
    const int nc = P.num_classes;
    if (DT == PVNET_MASK_U8) return class_of(reinterpret_cast<const uint8_t*>(P.labels)[off], nc);
    if (DT == PVNET_MASK_I16) return class_of(reinterpret_cast<const int16_t*>(P.labels)[off], nc);
    if (DT == PVNET_MASK_I32) return class_of(reinterpret_cast<const int32_t*>(P.labels)[off], nc);
    if (DT == PVNET_MASK_I64)   // read once, never again: non-temporal, as the mask kernel reads it
        return class_of(__builtin_nontemporal_load(reinterpret_cast<const long long*>(P.labels) + off), nc);
    if (DT == PVNET_MASK_F32) {   // `mask == k + 1` on a float mask: the value itself has to be the integer
        const float f = reinterpret_cast<const float*>(P.labels)[off];
        const int c = (f >= 1.f && f < (float)nc) ? (int)f : 0;
        return (float)c == f ? c : 0;
    }
    // torch.argmax(seg_pred, 1) with the first-maximum and NaN rule of k1_mask.hip: take = x > best || (x is NaN && best is not)
    float best = ld_elem_rt(P.logits_type, P.labels, off);
    int arg = 0;
    for (int c = 1; c < nc; ++c) {
        const float x = ld_elem_rt(P.logits_type, P.labels, off + (int64_t)c * P.ms_c);
        const bool take = (best == best) & !(x <= best);
        best = take ? x : best;
        arg = take ? c : arg;
    }
    return arg;
}

__device__ __forceinline__ unsigned long long spread_bits(uint32_t v) {   // bit k of v -> bit 2 k
    unsigned long long x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// wave 0: inclusive prefix over a segment's histogram of thinning bins -- dst[k - 1] = pixels kept at threshold k (what
// thin_hist_prefix of k1_mask.hip writes)
__device__ __forceinline__ void hist_prefix(uint16_t* dst, const int* s_hist, int lane) {
    constexpr int PER = THIN_BINS / 64;   // consecutive bins per lane
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
    dst += PER * lane;
#pragma unroll
    for (int i = 0; i < PER; i += 2)
        *reinterpret_cast<uint32_t*>(dst + i) = (uint32_t)(e + h[i]) | ((uint32_t)(e + h[i + 1]) << 16);
}

// PAIR: contiguous, 16-byte aligned int64 labels with an even number of pixels per image -- one 16-byte load brings two pixels per
// lane (mask_bits_pair_kernel's load); a wave's ballots then hold the even and the odd pixels of a 128-pixel double word, kept in
// the two halves of the class's 64 LDS slots and interleaved when the words are stored.
template <int DT, bool PAIR>
__global__ __launch_bounds__(64 * K1_WAVES) void class_split_kernel(ClassParams P) {
    PVNET_SPARE_VGPRS(63);   // (the histogram prefix holds 24 bins per lane: 53 in use; 64 still leave eight waves per SIMD)
    small_stage_prio();
    constexpr int NL = K1_WORDS_PER_WAVE;   // labels per lane: NL words of 64 pixels, or NL / 2 double words of 128
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    extern __shared__ unsigned long long s_words[];   // [num_classes - 1][SEG_WORDS]
    __shared__ int s_cnt[PVNET_CLASSES_MAX];
    __shared__ int s_hist[THIN_BINS];
    const int bi = blockIdx.y, nk = P.num_classes - 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int seg_word0 = blockIdx.x * SEG_WORDS;
    // label j of this lane: its pixel, and the LDS slot (of a class's 64) its ballot goes to
    auto pixel_of = [&](int j) {
        return PAIR ? (blockIdx.x * (SEG_WORDS / 2) + wave + (j >> 1) * K1_WAVES) * 128 + 2 * lane + (j & 1)
                    : (seg_word0 + wave + j * K1_WAVES) * 64 + lane;
    };
    auto slot_of = [&](int j) { return PAIR ? (j & 1) * (SEG_WORDS / 2) + wave + (j >> 1) * K1_WAVES : wave + j * K1_WAVES; };

    int lab[NL];
    if (PAIR) {
        const i64x2* base = reinterpret_cast<const i64x2*>(reinterpret_cast<const long long*>(P.labels) + (int64_t)bi * P.ms0);
#pragma unroll
        for (int j = 0; j < NL; j += 2) {
            const int p = pixel_of(j);
            lab[j] = lab[j + 1] = 0;
            if (p < P.npix) {   // (npix is even here: p + 1 < npix too)
                const i64x2 v = __builtin_nontemporal_load(base + (p >> 1));
                lab[j] = class_of(v.x, P.num_classes);
                lab[j + 1] = class_of(v.y, P.num_classes);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int p = pixel_of(j);
            lab[j] = 0;
            if (p < P.npix) {
                int64_t off;
                if (P.linear) {
                    off = (int64_t)bi * P.ms0 + p;
                } else {
                    const int y = p / P.w, x = p - y * P.w;
                    off = (int64_t)bi * P.ms0 + (int64_t)y * P.ms1 + (int64_t)x * P.ms2;
                }
                lab[j] = load_class<DT>(P, off);
            }
        }
    }
    for (int i = threadIdx.x; i < nk * SEG_WORDS; i += 64 * K1_WAVES) s_words[i] = 0ull;   // (the loads are in flight)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        unsigned long long rem = __ballot(lab[j] != 0);
        while (rem) {   // wave-uniform: one turn per distinct class among these 64 pixels
            const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
            const int c = __builtin_amdgcn_readlane(lab[j], first);
            const unsigned long long m = __ballot(lab[j] == c);
            if (lane == 0) s_words[(c - 1) * SEG_WORDS + slot_of(j)] = m;
            rem &= ~m;
        }
    }
    __syncthreads();
    for (int c = wave; c < nk; c += K1_WAVES) {   // class c + 1: its 64 words of this segment, one coalesced store
        unsigned long long wd;
        if (PAIR) {   // word `lane`: half of a double word, even and odd pixels interleaved
            const unsigned long long me = s_words[c * SEG_WORDS + (lane >> 1)], mo = s_words[c * SEG_WORDS + SEG_WORDS / 2 + (lane >> 1)];
            const uint32_t e32 = (lane & 1) ? (uint32_t)(me >> 32) : (uint32_t)me, o32 = (lane & 1) ? (uint32_t)(mo >> 32) : (uint32_t)mo;
            wd = spread_bits(e32) | (spread_bits(o32) << 1);
        } else {
            wd = s_words[c * SEG_WORDS + lane];
        }
        const size_t v = (size_t)bi * nk + c;
        if (seg_word0 + lane < P.words) P.bits[v * P.words + seg_word0 + lane] = wd;
        const int cnt = wave_reduce_add((int)__popcll(wd));
        if (lane == 0) {
            P.seg0[v * P.nseg + blockIdx.x] = cnt;
            s_cnt[c] = cnt;
        }
    }
    if (P.cum == nullptr) return;   // block-uniform
    __syncthreads();
    for (int c = 0; c < nk; ++c) {
        if (s_cnt[c] == 0) continue;   // block-uniform: most classes have no pixel in most segments
        for (int i = threadIdx.x; i < THIN_BINS; i += 64 * K1_WAVES) s_hist[i] = 0;
        __syncthreads();
        const size_t v = (size_t)bi * nk + c;
        const uint32_t key = pvnet_rng_key(P.seed, PVNET_TAG_SUB, (uint32_t)(P.image_base + (int)v));
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (lab[j] == c + 1) atomicAdd(&s_hist[pvnet_thin_bin(pvnet_rng_at(key, (uint32_t)pixel_of(j)))], 1);
        __syncthreads();
        if (wave == 0) hist_prefix(P.cum + (v * P.nseg + blockIdx.x) * THIN_BINS, s_hist, lane);
        __syncthreads();   // the next class zeroes the histogram
    }
}

int launch(const ClassParams& P, int dt, int b, hipStream_t s) {
    const dim3 grid(P.nseg, b), block(64 * K1_WAVES);
    const size_t lds = sizeof(unsigned long long) * SEG_WORDS * (size_t)(P.num_classes - 1);
    switch (dt) {
        case PVNET_MASK_U8: hipLaunchKernelGGL((class_split_kernel<PVNET_MASK_U8, false>), grid, block, lds, s, P); break;
        case PVNET_MASK_I16: hipLaunchKernelGGL((class_split_kernel<PVNET_MASK_I16, false>), grid, block, lds, s, P); break;
        case PVNET_MASK_I32: hipLaunchKernelGGL((class_split_kernel<PVNET_MASK_I32, false>), grid, block, lds, s, P); break;
        case PVNET_MASK_I64:
            // contiguous images at 16-byte aligned addresses, an even number of pixels: two pixels per 16-byte load
            if (P.linear && (reinterpret_cast<uintptr_t>(P.labels) & 15u) == 0 && (P.ms0 & 1) == 0 && (P.npix & 1) == 0)
                hipLaunchKernelGGL((class_split_kernel<PVNET_MASK_I64, true>), grid, block, lds, s, P);
            else
                hipLaunchKernelGGL((class_split_kernel<PVNET_MASK_I64, false>), grid, block, lds, s, P);
            break;
        case PVNET_MASK_F32: hipLaunchKernelGGL((class_split_kernel<PVNET_MASK_F32, false>), grid, block, lds, s, P); break;
        case CS_LOGITS: hipLaunchKernelGGL((class_split_kernel<CS_LOGITS, false>), grid, block, lds, s, P); break;
        default: return PVNET_E_BADARG;
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// everything both entries check and fill but the label source itself
int fill(ClassParams& P, const void* src, const int64_t* strides, int num_classes, int b, int h, int w, int max_num, uint64_t seed,
         int image_base, uint64_t* bits, int32_t* seg0, uint16_t* cum) {
    if (!src || !strides || !bits || !seg0) return PVNET_E_BADARG;
    if (num_classes < 2 || num_classes > PVNET_CLASSES_MAX) return PVNET_E_BADARG;
    if (b <= 0 || h <= 0 || w <= 0 || max_num < 0) return PVNET_E_BADARG;
    const long long npix = (long long)h * w;
    if (npix > (1ll << 30) || (long long)b * (num_classes - 1) > 65535) return PVNET_E_UNSUPPORTED;   // pvnet_vote_layout's limits
    if (max_num < npix && !cum) return PVNET_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(bits) & 7u) || (reinterpret_cast<uintptr_t>(seg0) & 3u) || (reinterpret_cast<uintptr_t>(cum) & 3u))
        return PVNET_E_BADARG;
    P.labels = src;
    P.num_classes = num_classes;
    P.logits_type = VT_F32;
    P.ms_c = 0;
    P.npix = (int)npix;
    P.w = w;
    P.words = (int)((npix + 63) / 64);
    P.nseg = (P.words + SEG_WORDS - 1) / SEG_WORDS;
    P.seed = seed;
    P.image_base = image_base;
    P.bits = bits;
    P.seg0 = seg0;
    P.cum = max_num < npix ? cum : nullptr;
    return 0;
}

}  // namespace
}  // namespace pvd

using namespace pvd;

extern "C" {

int pvnet_classes_abi_version(void) { return PVNET_CLASSES_ABI_VERSION; }

int pvnet_class_split(const void* labels, int mask_dtype, const int64_t mask_strides[3], int num_classes, int b, int h, int w,
                      int max_num, uint64_t seed, int image_base, uint64_t* bits, int32_t* seg0, uint16_t* cum, void* stream) {
    if (mask_dtype < PVNET_MASK_U8 || mask_dtype > PVNET_MASK_F32) return PVNET_E_BADARG;
    ClassParams P;
    const int rc = fill(P, labels, mask_strides, num_classes, b, h, w, max_num, seed, image_base, bits, seg0, cum);
    if (rc) return rc;
    P.ms0 = mask_strides[0]; P.ms1 = mask_strides[1]; P.ms2 = mask_strides[2];
    P.linear = (mask_strides[2] == 1 && mask_strides[1] == w) ? 1 : 0;
    return launch(P, mask_dtype, b, static_cast<hipStream_t>(stream));
}

int pvnet_class_split_logits(const void* seg_pred, int logits_type, const int64_t seg_strides[4], int num_classes, int b, int h,
                             int w, int max_num, uint64_t seed, int image_base, uint64_t* bits, int32_t* seg0, uint16_t* cum,
                             void* stream) {
    if (logits_type < PVNET_CLASSES_LOGITS_F32 || logits_type > PVNET_CLASSES_LOGITS_BF16) return PVNET_E_BADARG;
    ClassParams P;
    const int rc = fill(P, seg_pred, seg_strides, num_classes, b, h, w, max_num, seed, image_base, bits, seg0, cum);
    if (rc) return rc;
    P.ms0 = seg_strides[0]; P.ms_c = seg_strides[1]; P.ms1 = seg_strides[2]; P.ms2 = seg_strides[3];   // (b, y, x); the class stride apart
    P.linear = (seg_strides[3] == 1 && seg_strides[2] == w) ? 1 : 0;
    P.logits_type = logits_type;
    return launch(P, CS_LOGITS, b, static_cast<hipStream_t>(stream));
}

}  // extern "C"
