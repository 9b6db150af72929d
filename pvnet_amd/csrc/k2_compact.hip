// k2_compact.hip -- K2: thinning of the own segment (tn0 > max_num), order-preserving compaction, one float4 record per (pixel, key-point)
// (part of libpvnet_vote.so; the stage map is at the top of vote_host.hip, the shared definitions in vote_common.h)
#include "vote_common.h"

namespace pvd {
namespace {

// ------------------------------------------------------------------------------------------------------------
// The ORIGIN block: one extra block per image of an exact-mode launch (vn <= KP_MAX).  What K3's blocks need to know about their
// image -- per key-point the origin of the rounding band, the image's culling vote, band_rho(tn) -- depends on the image alone, and
// until round 12 every one of the 37 blocks per image of the hypothesis launch worked it out for itself (kp_preamble) so that no
// block had to wait for another.  This block works it out ONCE, before that launch starts, and it waits for nobody either: it
// reads only what K1 left (segment counts, bit words) and the field itself.
//   The estimate reads 17 slots of the image's pixel list (origin_slot(): eight fixed pairs + the median pixel).  An image that is
// not thinned keeps every foreground pixel in raster order, so slot t is the t-th set bit of the mask: its segment from a scan of
// the segment counts, its word from a scan of the segment's 64 popcounts, its bit by the popcount bisection of `locate` below.  The
// pixels' directions come straight from the field with compact_kernel's own addressing (ld_elem<VT>, vs*, bi / src_div): bit for
// bit the records the compaction blocks write beside this one -- exact-mode records keep the raw direction.  Then the arithmetic of
// kp_origin_vote() (vote_common.h), which is what kp_preamble runs.
//   A THINNED image (tn0 > max_num) keeps a random subset: its list is not the mask's.  The block clears OR_READY and K3's blocks
// of that image run kp_preamble as before.  Dead images (tn0 < min_num, tn = 0) get origin (0, 0) and vote 0, as kp_preamble gives.
// ------------------------------------------------------------------------------------------------------------
template <int VT>
__device__ __forceinline__ void origin_block(const VoteParams& P, int bi) {
    __shared__ KpShared S;
    __shared__ int s_sum[4];
    __shared__ int s_seg[ORIGIN_SLOTS], s_rank[ORIGIN_SLOTS], s_pixel[ORIGIN_SLOTS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t* sg = P.seg0 + bi * P.nseg;
    auto wave_scan = [&](int c) {   // inclusive, over the wave's lanes
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        return incl;
    };
    int tot = 0;
    for (int j = tid; j < P.nseg; j += 256) tot += sg[j];
    tot = wave_reduce_add(tot);
    if (lane == 0) s_sum[wave] = tot;
    __syncthreads();
    const int tn0 = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    int32_t* const ready = origin_ready_ptr(P, bi);
    if (tn0 > P.max_num) {   // block-uniform: thinned
        if (tid == 0) ready[OR_READY] = 0;
        return;
    }
    const int usable = P.cap - PAD;
    const int tn = tn0 < usable ? tn0 : usable;   // what the block of the last segment writes to C_TN
    const bool live = tn0 >= P.min_num && tn > 0;
    if (live) {   // block-uniform
        if (tid < ORIGIN_SLOTS) s_seg[tid] = s_rank[tid] = s_pixel[tid] = 0;   // (every slot below is found exactly once: tn <= the sum of the counts)
        // ---- the segment of every slot: thread = segment, 256 at a time; [excl, excl + c) are the list slots of its pixels
        int carry = 0;
        for (int j0 = 0; j0 < P.nseg; j0 += 256) {
            __syncthreads();   // (s_sum of the previous trip / of the total has been read)
            const int j = j0 + tid;
            const int c = j < P.nseg ? sg[j] : 0;
            const int incl = wave_scan(c);
            if (lane == 63) s_sum[wave] = incl;
            __syncthreads();
            int excl = carry + incl - c;
            for (int i = 0; i < wave; ++i) excl += s_sum[i];
            if (c > 0)
#pragma unroll 1   // (unrolled, the 17 slot ranks -- scalar values -- are kept across the whole block and scalar registers run out)
                for (int s = 0; s < ORIGIN_SLOTS; ++s) {
                    const int r = origin_slot(s, tn) - excl;
                    if ((unsigned)r < (unsigned)c) {
                        s_seg[s] = j;
                        s_rank[s] = r;
                    }
                }
            carry += s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        }
        __syncthreads();
        // ---- the pixel of every slot: a wave per slot, lane = word of the slot's segment
        const uint64_t* bw = P.bits + (size_t)bi * P.words;
        for (int s = wave; s < ORIGIN_SLOTS; s += 4) {
            const int wi = s_seg[s] * SEG_WORDS + lane;
            const unsigned long long wd = wi < P.words ? bw[wi] : 0ull;
            const int c = __popcll(wd);
            int r = s_rank[s] - (wave_scan(c) - c);
            if ((unsigned)r < (unsigned)c) {   // one lane: the bit of rank r in its word
                int bitpos = 0;
#pragma unroll
                for (int st = 32; st > 0; st >>= 1) {
                    const int cc = __popcll((wd >> bitpos) & ((1ull << st) - 1ull));
                    const int take = ~((r - cc) >> 31);  // r >= cc
                    bitpos += st & take;
                    r -= cc & take;
                }
                s_pixel[s] = wi * 64 + bitpos;
            }
        }
        __syncthreads();
    }
    // ---- candidate j of key-point kk: the records of slots j and NCAND + j, as the compaction blocks write them
    const int kk = tid / NCAND, j = tid % NCAND;
    const bool mine = tid < P.vn * NCAND;
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    int pm = 0;
    if (live) {
        pm = s_pixel[2 * NCAND];
        if (mine) {
            const int64_t vimg = (int64_t)(bi / P.src_div) * P.vs0 + (int64_t)kk * P.vs3;
            const int pa = s_pixel[j], pb = s_pixel[NCAND + j];
            const int ya = pa / P.w, xa = pa - ya * P.w;
            const int yb = pb / P.w, xb = pb - yb * P.w;
            const int64_t va = vimg + (int64_t)ya * P.vs1 + (int64_t)xa * P.vs2;
            const int64_t vb = vimg + (int64_t)yb * P.vs1 + (int64_t)xb * P.vs2;
            q0 = make_float4((float)xa, (float)ya, ld_elem<VT>(P.vertex, va), ld_elem<VT>(P.vertex, va + P.vs4));
            q1 = make_float4((float)xb, (float)yb, ld_elem<VT>(P.vertex, vb), ld_elem<VT>(P.vertex, vb + P.vs4));
        }
    }
    kp_origin_vote(P, tn, live, pm, mine, q0, q1, S);
    if (tid < P.vn) {
        int32_t* o = band_origin_ptr(P, (size_t)bi * P.vn + tid);
        o[0] = S.org[tid * 2];
        o[1] = S.org[tid * 2 + 1];
    }
    if (tid == 0) {
        ready[OR_VOTE] = (P.cull && live && image_culled(S, P.vn)) ? 1 : 0;
        P.ctrl[bi * CTRL_STRIDE + C_RHO] = (int)__float_as_uint(band_rho(tn));
        ready[OR_READY] = 1;
    }
}

// ------------------------------------------------------------------------------------------------------------
// K2: order-preserving compaction + direction gather          (ransac_voting_gpu.py:542-546)
// One block per (segment, image, group of K2_KG key-points); an exact-mode launch (compact_origin()) has one more block per image
// behind the segments', the origin block above.
// ------------------------------------------------------------------------------------------------------------
template <bool LITERAL, int K2_KG, int VT>  // K2_KG key-points per block: grid.z = ceil(vn / K2_KG); VT: field element type
__global__ __launch_bounds__(256) void compact_kernel(VoteParams P) {
    if (K2_KG == 1) PVNET_SPARE_VGPRS(39); else if (K2_KG <= 3) PVNET_SPARE_VGPRS(47); else PVNET_SPARE_VGPRS(87);
    small_stage_prio();
    const int bi = blockIdx.y;
    if (LITERAL && K2_KG == 3 && (int)blockIdx.x >= P.nseg) {   // block-uniform: the image's origin block (only launch_compact's exact-mode grid has it)
        if (blockIdx.z == 0) origin_block<VT>(P, bi);
        return;
    }
    const int w0 = blockIdx.x * K2_WORDS_PER_BLOCK;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t* bw = P.bits + (size_t)bi * P.words;

    __shared__ int s_red[4];
    __shared__ int s_tot[4];
    __shared__ int s_woff[K2_WORDS_PER_BLOCK];
    __shared__ uint64_t s_word[K2_WORDS_PER_BLOCK];
    __shared__ uint16_t s_piece[4 * K2_WORDS_PER_BLOCK];
    __shared__ int s_total;

    // the image's foreground count (tn0) and the pixels kept before this block = sums over the segment counts
    // (<= a few hundred ints)
    const int32_t* sg = P.seg0 + bi * P.nseg;
    const bool last = (int)blockIdx.x == P.nseg - 1;
    if (!last && sg[blockIdx.x] == 0) return;  // block-uniform: most of the image is background
    int part = 0, tot = 0;
    for (int j = threadIdx.x; j < P.nseg; j += 256) {
        const int c = sg[j];
        tot += c;
        part += j < (int)blockIdx.x ? c : 0;
    }
    part = wave_reduce_add(part);
    tot = wave_reduce_add(tot);
    if (lane == 0) {
        s_red[wave] = part;
        s_tot[wave] = tot;
    }
    auto scan_words = [&](unsigned long long wd) {  // wave 0: exclusive scan of this block's 64 word popcounts
        const int c = __popcll(wd);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        s_word[lane] = wd;
        s_woff[lane] = incl - c;
        if (lane == 63) s_total = incl;
    };
    if (wave == 0) scan_words((w0 + lane < P.words) ? bw[w0 + lane] : 0ull);
    __syncthreads();
    const int tn0 = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
    int base = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    if (tn0 > P.max_num) {
        // Thinning (block-uniform, rare: objects larger than max_num pixels, or the evaluation call site's max_num = 100):
        // keep a pixel when the bin of its random word is below k (oracle: subsample_threshold).  The pixels kept in
        // earlier segments are column k - 1 of their cumulative histograms (K1); this segment's words are filtered here,
        // 16 bits per thread.
        const int k = pvnet_thin_bins_kept(P.max_num, tn0);  // 0 .. PVNET_THIN_LAST + 1
        int part2 = 0;
        if (k > 0)
            for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256)
                if (sg[j] > 0) part2 += P.cum[((size_t)bi * P.nseg + j) * THIN_BINS + k - 1];
        part2 = wave_reduce_add(part2);
        const int q = threadIdx.x & 3;
        unsigned todo = (unsigned)(s_word[threadIdx.x >> 2] >> (16 * q)) & 0xFFFFu, kept = 0;
        const uint32_t key = pvnet_rng_key(P.seed, PVNET_TAG_SUB, (uint32_t)(P.image_base + bi));
        const uint32_t p0 = (uint32_t)((w0 + (threadIdx.x >> 2)) * 64 + 16 * q);
        while (todo) {
            const int bpos = __ffs((int)todo) - 1;
            todo &= todo - 1;
            if (pvnet_thin_bin(pvnet_rng_at(key, p0 + (uint32_t)bpos)) < k) kept |= 1u << bpos;
        }
        __syncthreads();  // every read of s_word / s_red above has been performed
        s_piece[threadIdx.x] = (uint16_t)kept;
        if (lane == 0) s_red[wave] = part2;
        __syncthreads();
        if (wave == 0)
            scan_words((unsigned long long)s_piece[4 * lane] | ((unsigned long long)s_piece[4 * lane + 1] << 16) |
                       ((unsigned long long)s_piece[4 * lane + 2] << 32) | ((unsigned long long)s_piece[4 * lane + 3] << 48));
        __syncthreads();
        base = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    }
    const int usable = P.cap - PAD;

    // One thread per KEPT pixel (not per mask bit): thread t of the segment finds the word holding its pixel by a
    // binary search over the 64 word offsets (LDS) and the bit by a popcount bisection, so every lane does useful
    // work and consecutive lanes gather consecutive (raster-adjacent) addresses.  blockIdx.z selects a group of
    // K2_KG key-points; two pixels per thread are in flight before the first use (the stage is latency-bound).
    const int k0 = blockIdx.z * K2_KG;
    const int T = s_total;
    auto locate = [&](int t, int& pos, int& p) {
        // branch-free: every decision is the sign bit of a difference turned into an all-ones / zero mask
        int lo = 0;
#pragma unroll
        for (int st = 32; st > 0; st >>= 1) lo += st & ~((t - s_woff[lo + st]) >> 31);  // s_woff[lo + st] <= t; lo + st <= 63
        const unsigned long long wd = s_word[lo];
        int r = t - s_woff[lo], bitpos = 0;
#pragma unroll
        for (int st = 32; st > 0; st >>= 1) {
            const int c = __popcll((wd >> bitpos) & ((1ull << st) - 1ull));
            const int take = ~((r - c) >> 31);  // r >= c
            bitpos += st & take;
            r -= c & take;
        }
        pos = base + t;
        p = (w0 + lo) * 64 + bitpos;
    };
    auto emit = [&](int pos, int x, int y, const float* ux, const float* uy) {
#pragma unroll
        for (int kk = 0; kk < K2_KG; ++kk) {
            if (k0 + kk >= P.vn) break;
            const size_t o = ((size_t)bi * P.vn + k0 + kk) * P.cap + pos;
            if (LITERAL) {
                P.rec[o] = make_float4((float)x, (float)y, ux[kk], uy[kk]);
            } else {
                const bool dead = norm1_literal(ux[kk], uy[kk]) <= kF1e6;  // never votes (:119-121): stored as a zero record
                P.rec[o] = make_float4((float)x, (float)y, dead ? 0.f : ux[kk], dead ? 0.f : uy[kk]);
            }
        }
    };
    const int64_t vimg = (int64_t)(bi / P.src_div) * P.vs0;  // the image's field (scalar; src_div = 1 unless the images are classes of one)
    for (int t0 = threadIdx.x; t0 < T; t0 += 512) {
        const int t1 = t0 + 256;
        const bool has1 = t1 < T;
        int pos0, p0, pos1 = 0, p1 = 0;
        locate(t0, pos0, p0);
        if (has1) locate(t1, pos1, p1);
        const int y0 = p0 / P.w, x0 = p0 - y0 * P.w;
        const int y1 = p1 / P.w, x1 = p1 - y1 * P.w;
        const int64_t v0 = vimg + (int64_t)y0 * P.vs1 + (int64_t)x0 * P.vs2;  // element offsets
        const int64_t v1 = vimg + (int64_t)y1 * P.vs1 + (int64_t)x1 * P.vs2;
        float ux0[K2_KG], uy0[K2_KG], ux1[K2_KG], uy1[K2_KG];
#pragma unroll
        for (int kk = 0; kk < K2_KG; ++kk) {
            const int k = (k0 + kk < P.vn) ? k0 + kk : P.vn - 1;  // clamp: loads stay in bounds, unconditional
            ux0[kk] = ld_elem<VT>(P.vertex, v0 + (int64_t)k * P.vs3);
            uy0[kk] = ld_elem<VT>(P.vertex, v0 + (int64_t)k * P.vs3 + P.vs4);
            ux1[kk] = ld_elem<VT>(P.vertex, v1 + (int64_t)k * P.vs3);  // (p1 = 0 when there is no second pixel: a valid address)
            uy1[kk] = ld_elem<VT>(P.vertex, v1 + (int64_t)k * P.vs3 + P.vs4);
        }
        if (pos0 < usable) {
            if (k0 == 0) P.pix[(size_t)bi * P.cap + pos0] = p0;
            emit(pos0, x0, y0, ux0, uy0);
        }
        if (has1 && pos1 < usable) {
            if (k0 == 0) P.pix[(size_t)bi * P.cap + pos1] = p1;
            emit(pos1, x1, y1, ux1, uy1);
        }
    }
    if (last) {  // the block that owns the last segment knows the total
        const int total = base + s_total;
        const int tn = total < usable ? total : usable;
        if (k0 == 0 && wave == 0) {  // nothing zero-fills ctrl: this block owns tn0 / tn / status of its image
            if (lane == 0) {
                P.ctrl[bi * CTRL_STRIDE + C_TN0] = tn0;
                P.ctrl[bi * CTRL_STRIDE + C_TN] = tn;
                P.ctrl[bi * CTRL_STRIDE + C_STATUS] = total > usable ? PVNET_S_OVERFLOW : 0;
                if (bi == 0) {   // the call's flags (vote_common.h): K3 sets / adds to them
                    int32_t* cf = call_flags_ptr(P);
                    const bool prev = P.ctrl[P.b * CTRL_STRIDE + 6] == P.layout_fp;   // a previous call of this layout left its votes here
                    cf[CF_BATCH_OK] = (!prev || 3 * cf[CF_VOTES_NOW] >= 2 * P.b) ? 1 : 0;
                    cf[CF_VOTES_NOW] = 0;
                    cf[CF_ANY_CULLED] = 0;
                }
            }
        }
        const int tpad = (tn + PAD - 1) / PAD * PAD;  // sentinel records: zero direction never votes
        const int kn = (k0 + K2_KG < P.vn ? k0 + K2_KG : P.vn) - k0;
        for (int i = threadIdx.x; i < (tpad - tn) * kn; i += 256) {
            const int kk = i / (tpad - tn), t = tn + i - kk * (tpad - tn);
            P.rec[((size_t)bi * P.vn + k0 + kk) * P.cap + t] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}


}  // namespace

int launch_compact(const VoteParams& P, hipStream_t s, bool literal, int kg) {
    dim3 grid(P.nseg, P.b, (P.vn + kg - 1) / kg);
    // the calls whose K3 blocks look for stored band origins (hypothesis_kernel's kp_origin) get the origin block: one more column of
    // blocks, of which the one at z = 0 works and the others leave at once
    const bool origin = !literal && P.mode && P.exact && P.vn <= KP_MAX;
    const dim3 g3(P.nseg + (origin ? 1 : 0), P.b, (P.vn + 2) / 3);
    (void)grid;
#ifdef PVNET_DEV
#define PV_K2(VT)                                                                                                  \
    do {                                                                                                           \
        if (literal || P.exact) hipLaunchKernelGGL((compact_kernel<true, 3, VT>), g3, dim3(256), 0, s, P);         \
        else if (kg == 1) hipLaunchKernelGGL((compact_kernel<false, 1, VT>), grid, dim3(256), 0, s, P);            \
        else if (kg == 9) hipLaunchKernelGGL((compact_kernel<false, 9, VT>), grid, dim3(256), 0, s, P);            \
        else hipLaunchKernelGGL((compact_kernel<false, 3, VT>), g3, dim3(256), 0, s, P);                           \
    } while (0)
#else   // release: three key-points per block (the PVNET_COMPACT_KG variants 1 and 9 are development builds only)
#define PV_K2(VT)                                                                                                  \
    do {                                                                                                           \
        if (literal || P.exact) hipLaunchKernelGGL((compact_kernel<true, 3, VT>), g3, dim3(256), 0, s, P);         \
        else hipLaunchKernelGGL((compact_kernel<false, 3, VT>), g3, dim3(256), 0, s, P);                           \
    } while (0)
#endif
    if (P.vertex_type == VT_F16) PV_K2(VT_F16);
    else if (P.vertex_type == VT_BF16) PV_K2(VT_BF16);
    else PV_K2(VT_F32);
#undef PV_K2
    return 0;
}

}  // namespace pvd
