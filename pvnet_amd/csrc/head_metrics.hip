// head_metrics.hip -- the network-head metrics of a validation step, on the device: per-image cross-entropy of the class logits,
// weighted smooth-L1 loss of the vector field, segmentation precision and recall, for a batch in one call.  The whole of
// libpvnet_head.so; C ABI: pvnet_head_metrics in include/pvnet_head.h.
//
// Restates what the reference's NetWrapper.forward computes after the backbone (tools/train_linemod.py:85-91 with
// lib/utils/net_utils.py:54-79 and :329-348), term for term in float64 on the inputs as stored.  Its oracle is the float64
// restatement of tests/test_head_metrics_device.py and the reference's own recorded outputs (tests/golden/head_metrics.npz).
//
// The arithmetic is head_common.h's, shared with the backward and the key-point forms; this file instantiates the forward's bodies
// on the memory source (targets, weights and mask loaded) and holds the entry point:
//
//   head_partial_kernel   grid (segments of 1 024 pixels, images).  A workgroup streams its run of pixels through every plane -- the
//     (head_partial8)     class logits, the 2 vn predicted and 2 vn target planes, the weights, the mask -- eight consecutive pixels
//                         per lane, 16 bytes per load wherever the element is 2 bytes or wider: 164 bytes per pixel with float32
//                         predictions and int64 masks, each read once.  The planes must be contiguous in the pixels and 16-byte
//                         aligned, h * w a multiple of 8 (what a backbone and a dataset deliver).  The targets, the weights and
//                         the mask are loaded non-temporally -- nobody reads them again --, the predictions plainly: the vote reads
//                         them next (profiles/head_metrics_probe.txt holds the A/B).
//   head_partial_general_kernel   the same record from any element strides, any alignment, any h * w: a pixel per lane and load
//     (head_partial1)     (mirrors the mask_linear split of k1_mask.hip).
//   head_final_kernel     a workgroup per image: sums the image's records in a fixed order, finalises, writes the outputs.
//
// No atomics; every sum has a fixed order (lane-sequential, then an xor butterfly over the wave, then the waves in order), so two
// calls on the same inputs agree bit for bit.  float64 throughout: at 164 bytes per pixel the float64 vector rate is far above
// what the memory system can feed, the kernel is bound by HBM reads.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "head_common.h"
#include "pvnet_head.h"

namespace {

using namespace pvh;

// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define HEAD_FAST_SPARE 119      // float32 predictions
#define HEAD_FAST16_SPARE 127    // float16 / bfloat16: their conversions pass 111 VGPRs; still four waves per SIMD
#define HEAD_GENERAL_SPARE 87
#define HEAD_FINAL_SPARE 71

typedef HeadArgs<MemSource> Args;

template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_partial_kernel(Args A) {
    if (VT == VT_F32) PVNET_SPARE_VGPRS(HEAD_FAST_SPARE);
    else PVNET_SPARE_VGPRS(HEAD_FAST16_SPARE);
    head_partial8<VT, NT>(A, nullptr);
}

__global__ __launch_bounds__(HC_T) void head_partial_general_kernel(Args A) {
    PVNET_SPARE_VGPRS(HEAD_GENERAL_SPARE);
    head_partial1(A, nullptr);
}

__global__ __launch_bounds__(HC_FT) void head_final_kernel(Args A) {
    PVNET_SPARE_VGPRS(HEAD_FINAL_SPARE);
    head_final_image(A);
}

}  // namespace

extern "C" {

int pvnet_head_abi_version(void) { return PVNET_HEAD_ABI_VERSION; }

size_t pvnet_head_metrics_workspace_bytes(int b, int h, int w) { return head_workspace_bytes(b, h, w); }

int pvnet_head_metrics(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4],
                       const float* vertex_weights, const int64_t w_strides[3], const void* mask, int mask_dtype,
                       const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags, double* losses,
                       int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const bool pointers = seg_pred && seg_strides && vertex_pred && vp_strides && vertex_target && vt_strides && vertex_weights &&
                          w_strides && mask && mask_strides && losses && counts;
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, num_classes, sigma, flags, HEAD_FLAGS)) return rc;
    if (b == 0) return 0;
    if (const int rc = check_workspace(workspace, workspace_bytes, head_workspace_bytes(b, h, w))) return rc;
    Args A;
    A.T = make_mem_source(vertex_target, vt_strides, vertex_weights, w_strides, mask, mask_dtype, mask_strides);
    fill_inputs(A, seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, h, w, vn, sigma, flags);
    fill_head(A, losses, counts, status, workspace);
    const bool fast = A.npix % HC_PPL == 0 && linear4(seg_pred, b, A.ss, w) && linear4(vertex_pred, b, A.vs, w) &&
                      A.T.targets_linear(b, w) && linear3(mask, b, A.T.ms, w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (fast)
        launch_fast(A.vp_type, flags, [&](auto vt, auto nt) {
            hipLaunchKernelGGL((head_partial_kernel<decltype(vt)::value, decltype(nt)::value>), grid, dim3(HC_T), 0, s, A);
        });
    else
        hipLaunchKernelGGL(head_partial_general_kernel, grid, dim3(HC_T), 0, s, A);
    hipLaunchKernelGGL(head_final_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    return launched();
}

}  // extern "C"
