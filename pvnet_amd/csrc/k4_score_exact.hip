// k4_score_exact.hip -- K4, exact mode (the default): the dense scoring kernels -- matrix-pipe scoring with the rounding-band epilogue, counts equal to kernel.cu:88-126
// (part of libpvnet_vote.so; the stage map is at the top of vote_host.hip, the shared definitions in vote_common.h)
#include "vote_common.h"
#include "k4_exact_body.h"

namespace pvd {
namespace {

// The register allocator fills whatever budget the occupancy target leaves (3 waves per SIMD: up to 168 VGPRs), the library needs
// the top granule of every allocation unused (PVNET_SPARE_VGPRS): amdgpu_num_vgpr -- a literal, hence one definition per
// instantiation -- caps what the code may use one granule below what PVNET_SPARE_VGPRS makes the kernel allocate (the
// backend doubles the attribute's value on targets with a unified VGPR / AGPR file, hence the / 2).
// Release builds hold the variants the library's defaults reach: 1 / 2 / 4 tiles per wave (small hypothesis counts; cells of one pixel
// tile, two accumulator pairs) and, at 8 tiles per wave, one accumulator pair with strided items (a batch alone) or contiguous runs
// (batches in flight), each also with the clock stamps of the profiling entry.  Cells of a whole work item (PVNET_EXACT_FOLD=0), two
// accumulator pairs at 8 tiles (PVNET_SCORE_ACC=2) and the stamped forms of the small shapes are development builds (-DPVNET_DEV).
// The set of built (MH, FOLD, TIMED, NACC, RUNS) variants with their register budgets is PV_SCORE_EXACT_SET, stated once: the kernels
// are defined from it and launch_score_exact dispatches over it, so a combination outside it is PVNET_E_UNSUPPORTED in that library.
#define PV_SCORE_EXACT4(X, MH_, NACC_, RUNS_, NVGPR_)                                                                    \
    X(MH_, 0, 0, NACC_, RUNS_, NVGPR_) X(MH_, 0, 1, NACC_, RUNS_, NVGPR_)                                                \
    X(MH_, 1, 0, NACC_, RUNS_, NVGPR_) X(MH_, 1, 1, NACC_, RUNS_, NVGPR_)
#ifdef PVNET_DEV
#define PV_SCORE_EXACT_SET(X)                                                                                            \
    PV_SCORE_EXACT4(X, 1, 2, 0, 104) PV_SCORE_EXACT4(X, 2, 2, 0, 104) PV_SCORE_EXACT4(X, 4, 2, 0, 136)                   \
    PV_SCORE_EXACT4(X, 8, 1, 0, 120) PV_SCORE_EXACT4(X, 8, 2, 0, 160)                                                    \
    PV_SCORE_EXACT4(X, 8, 1, 1, 128) PV_SCORE_EXACT4(X, 8, 2, 1, 160)
#else
#define PV_SCORE_EXACT_SET(X)                                                                                            \
    X(1, 1, 0, 2, 0, 104) X(2, 1, 0, 2, 0, 104) X(4, 1, 0, 2, 0, 136)                                                    \
    X(8, 1, 0, 1, 0, 120) X(8, 1, 1, 1, 0, 120)                                                                          \
    X(8, 1, 0, 1, 1, 128) X(8, 1, 1, 1, 1, 128)
#endif
#define PV_DEF_SCORE_EXACT(MH_, FOLD_, TIMED_, NACC_, RUNS_, NVGPR_)                                                     \
    __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8), amdgpu_num_vgpr(NVGPR_ / 2))) void       \
        score_exact_kernel_##MH_##_##FOLD_##_##TIMED_##_##NACC_##_##RUNS_(VoteParams P) {                                \
        score_exact_body<MH_, FOLD_, TIMED_ != 0, NACC_, RUNS_ != 0>(P);                                                 \
    }
PV_SCORE_EXACT_SET(PV_DEF_SCORE_EXACT)
#undef PV_DEF_SCORE_EXACT

}  // namespace

// one_acc / runs: one accumulator pair / contiguous item runs (8 tiles per wave only: fewer tiles have two pairs, strided items);
// cells: P.fold1
int launch_score_exact(const VoteParams& P, dim3 g, size_t lds, hipStream_t s, bool timed, bool one_acc, bool runs) {
    const int mh = P.wg_g * P.hpl / 2;
    const int fold = P.fold1 ? 1 : 0, nacc = (mh == 8 && one_acc) ? 1 : 2;
    const bool r = mh == 8 && runs;
#define PV_TRY_SCORE_EXACT(MH_, FOLD_, TIMED_, NACC_, RUNS_, NVGPR_)                                                     \
    if (mh == MH_ && fold == FOLD_ && timed == (TIMED_ != 0) && nacc == NACC_ && r == (RUNS_ != 0)) {                    \
        hipLaunchKernelGGL(score_exact_kernel_##MH_##_##FOLD_##_##TIMED_##_##NACC_##_##RUNS_, g, dim3(256), lds, s, P);  \
        return 0;                                                                                                        \
    }
    PV_SCORE_EXACT_SET(PV_TRY_SCORE_EXACT)
#undef PV_TRY_SCORE_EXACT
    return PVNET_E_UNSUPPORTED;   // not built in this library (release: a development variant), or no such tile count
}

}  // namespace pvd
