// head_grad.hip -- the backward of the network-head losses of a training step, on the device: the gradient of the per-image
// cross-entropy with respect to the class logits and of the weighted smooth-L1 loss with respect to the predicted field, for a batch
// in one call.  The whole of libpvnet_train.so; C ABI: pvnet_head_grad in include/pvnet_train.h (the formulas are stated there).
//
// The forward is pvnet_head_metrics (head_metrics.hip, libpvnet_head.so); the loss is the reference's (tools/train_linemod.py:85-91,
// lib/utils/net_utils.py:54-79).  Both gradients have a closed form per element, so nothing of the forward is saved: the kernels read
// the forward's inputs again and write the two gradient tensors.  Its oracle is the float64 restatement
// tests/head_grad_restatement.py and the reference's own autograd, recorded in tests/golden/head_grad.npz.
//
// The arithmetic is head_common.h's, shared with the forward and the key-point forms; this file instantiates the backward's bodies
// on the memory source (targets, weights and mask loaded) and holds the entry point:
//
//   head_grad_wsum_kernel<FAST>   grid (segments of 1 024 pixels, images): the segment's sum of the weights, in the forward's order
//     (head_grad_wsum)            (so D_i = 2vn sum w + 1e-3 is the forward's denominator bit for bit).  4 bytes per pixel, loaded
//                                 plainly: the gradient kernel reads them again.  Skipped without a field gradient.
//   head_grad_final_kernel        a workgroup per image: sums the records in a fixed order and writes the image's two coefficients
//                                 u_s / (h w) and u_v / D_i to the workspace.
//   head_grad_kernel<VT, NT>      grid (segments, images), the fast path: eight consecutive pixels per lane, 16 bytes per load and
//     (head_grad8)                store wherever the element is 2 bytes or wider.  Reads every input byte once -- targets, weights
//                                 and mask non-temporally, as the forward does --, writes every gradient byte once, plainly: the
//                                 backbone's backward reads them next.  244 bytes per pixel with float32 predictions, int64 masks,
//                                 C = 2 and vn = 9.  Needs what the forward's fast path needs, of the gradient tensors too.
//   head_grad_general_kernel      the same from any element strides, any alignment, any h * w: a pixel per lane and access.
//     (head_grad1)
//   head_grad_status_kernel       a workgroup per image: ORs the segments' bad-label flags into status (only when status is asked
//                                 for; 0 where the logits' half did not run).
//
// No atomics; every sum has a fixed order, every output element is a function of its own pixel and the image's two coefficients:
// two calls agree bit for bit.  float64 after the load; each element is rounded ONCE to its tensor's type (float16 / bfloat16 through
// a round-to-odd float32, which makes the second rounding exact).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "head_common.h"
#include "pvnet_train.h"

namespace {

using namespace pvh;

// the spare-VGPR granule of each kernel (PVNET_SPARE_VGPRS in vote_common.h; tools/check_kernel_resources.py holds them to it)
#define GRAD_FAST_SPARE 135
#define GRAD_GENERAL_SPARE 79
#define GRAD_WSUM_SPARE 31
#define GRAD_FINAL_SPARE 31
#define GRAD_STATUS_SPARE 23

typedef GradArgs<MemSource> Args;

template <bool FAST>
__global__ __launch_bounds__(HC_T) void head_grad_wsum_kernel(Args A) {
    PVNET_SPARE_VGPRS(GRAD_WSUM_SPARE);
    head_grad_wsum<FAST>(A);
}

__global__ __launch_bounds__(HC_FT) void head_grad_final_kernel(Args A) {
    PVNET_SPARE_VGPRS(GRAD_FINAL_SPARE);
    head_grad_final_image(A);
}

template <int VT, int NT>
__global__ __launch_bounds__(HC_T) void head_grad_kernel(Args A) {
    PVNET_SPARE_VGPRS(GRAD_FAST_SPARE);
    head_grad8<VT, NT>(A, nullptr);
}

__global__ __launch_bounds__(HC_T) void head_grad_general_kernel(Args A) {
    PVNET_SPARE_VGPRS(GRAD_GENERAL_SPARE);
    head_grad1(A, nullptr);
}

__global__ __launch_bounds__(HC_FT) void head_grad_status_kernel(Args A) {
    PVNET_SPARE_VGPRS(GRAD_STATUS_SPARE);
    head_grad_status_image(A);
}

}  // namespace

extern "C" {

int pvnet_train_abi_version(void) { return PVNET_TRAIN_ABI_VERSION; }

size_t pvnet_head_grad_workspace_bytes(int b, int h, int w) { return grad_workspace_bytes(b, h, w); }

int pvnet_head_grad(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                    const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4], const float* vertex_weights,
                    const int64_t w_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3], int b, int h, int w,
                    int vn, double sigma, uint32_t flags, const double* upstream, void* grad_seg, const int64_t gs_strides[4],
                    void* grad_vertex, const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream) {
    const bool pointers = seg_pred && seg_strides && vertex_pred && vp_strides && vertex_target && vt_strides && vertex_weights &&
                          w_strides && mask && mask_strides && upstream && (grad_seg || grad_vertex) && (!grad_seg || gs_strides) &&
                          (!grad_vertex || gv_strides);
    if (const int rc = check_args(pointers, mask_dtype, b, h, w, vn, num_classes, sigma, flags, HEAD_FLAGS)) return rc;
    if (b == 0) return 0;
    if (const int rc = check_workspace(workspace, workspace_bytes, grad_workspace_bytes(b, h, w))) return rc;
    Args A;
    A.T = make_mem_source(vertex_target, vt_strides, vertex_weights, w_strides, mask, mask_dtype, mask_strides);
    fill_inputs(A, seg_pred, seg_strides, num_classes, vertex_pred, vp_strides, h, w, vn, sigma, flags);
    fill_grad(A, b, upstream, grad_seg, gs_strides, grad_vertex, gv_strides, status, workspace);
    // each half asks the fast path's shape of its own tensors only: the other half's are not touched
    const bool lin_w = linear3(vertex_weights, b, A.T.ws, w);
    const bool fast = A.npix % HC_PPL == 0 &&
                      (!grad_seg || (linear4(seg_pred, b, A.ss, w) && linear3(mask, b, A.T.ms, w) && linear4(grad_seg, b, A.gss, w))) &&
                      (!grad_vertex || (linear4(vertex_pred, b, A.vs, w) && A.T.targets_linear(b, w) && linear4(grad_vertex, b, A.gvs, w)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)A.nseg, (unsigned)b);
    if (grad_vertex) {
        if (A.npix % HC_PPL == 0 && lin_w) hipLaunchKernelGGL(head_grad_wsum_kernel<true>, grid, dim3(HC_T), 0, s, A);
        else hipLaunchKernelGGL(head_grad_wsum_kernel<false>, grid, dim3(HC_T), 0, s, A);
    }
    hipLaunchKernelGGL(head_grad_final_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    if (fast)
        launch_fast(A.vp_type, flags, [&](auto vt, auto nt) {
            hipLaunchKernelGGL((head_grad_kernel<decltype(vt)::value, decltype(nt)::value>), grid, dim3(HC_T), 0, s, A);
        });
    else
        hipLaunchKernelGGL(head_grad_general_kernel, grid, dim3(HC_T), 0, s, A);
    if (status) hipLaunchKernelGGL(head_grad_status_kernel, dim3((unsigned)b), dim3(HC_FT), 0, s, A);
    return launched();
}

}  // extern "C"
