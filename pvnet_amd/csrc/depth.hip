// depth.hip -- libpvnet_depth.so: depth images, occlusion-correct label images and visible pixel counts of posed meshes
// (include/pvnet_depth.h holds THE DEFINITION).
//
// Path replaced (reference tree): OcclusionLineModDB.get_mask_of_all_objects (lib/utils/data_utils.py:788-826), a loop over the objects
// of one image on the host around an OpenGL depth render, and render_mesh_depth (lib/utils/extend_utils/extend_utils.py:196-213), whose
// native body the reference does not have.
//
// A z-buffer of one 64-bit word per pixel: bits(float32 depth) << 32 | instance << 8 | label.  Depths are positive, so the words order
// like (depth, instance) and one unsigned 64-bit minimum per candidate takes the nearest surface and, at a tie, the earlier instance.
// The one copy of the z-buffer lives in zbuffer_core.h (records, the setup, clear and triangle kernels' bodies, validation, workspace,
// launch sequence), which shade.hip and texture.hip compile too; here are the kernels' names and register allowances, this library's
// low word (LabelWord: the same for every triangle of an instance, so the cooperative path does not broadcast it), its resolve kernel,
// which reads the label from that word, and its entry points:
//   depth_setup_kernel    one workgroup: the instance table, which arrives in the launch's arguments, becomes records in the
//                         workspace; status, visible counts and counters zeroed
//   depth_clear_kernel    the z-buffer to bits(far) << 32 | 0xFFFFFFFF with 16-byte stores
//   depth_tri_kernel      one lane per (instance, triangle): stage P for its three vertices and the coverage predicate are the functions
//                         libpvnet_raster.so compiles (mesh_core.h); the plane of inverse depth in float64 once per triangle (depth_core.h),
//                         one float64 division per covered pixel.  A box of at most PVNET_DEPTH_LANE_PIXELS pixels the lane walks alone;
//                         larger boxes are taken one after the other by the whole wave, lanes across 64 pixels of a row
//   depth_resolve_kernel  four pixels per lane: words -> float32 depth (16-byte stores) and label bytes (4-byte stores); the pixels each
//                         instance won are counted in LDS and leave the workgroup as one integer add per instance present
// Minima and integer sums do not depend on the order in which they land: the call is bitwise reproducible.
//
// Nothing is contracted (FP_CONTRACT OFF), float32 and float64 denormals are kept (the compiler's default for gfx950).
#include "pvnet_depth.h"
#include "zbuffer_core.h"

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

PVNET_ZBUFFER_CONSTANTS_ARE(PVNET_DEPTH_, MAX_SIDE);

__global__ __launch_bounds__(1024) void depth_setup_kernel(Table T, int q, Inst* recs, int32_t* status, int32_t* visible,
                                                           uint32_t* counters) {
    PVNET_SPARE_VGPRS(31);
    setup_body(T, q, recs, status, visible, counters, NoTexture());
}

__global__ __launch_bounds__(TPB) void depth_clear_kernel(uint4* zbuf, size_t n16, uint32_t far_bits) {
    PVNET_SPARE_VGPRS(31);
    clear_body(zbuf, n16, far_bits);
}

__global__ __launch_bounds__(TPB) void depth_tri_kernel(TriParams P) {
    PVNET_SPARE_VGPRS(103);
    tri_body<LabelWord>(P);
}

struct ResolveParams {
    const unsigned long long* zbuf;   // NULL: no instance at all, zeros
    size_t n;                         // pixels of the call: b h w
    int q;
    float* depth;
    uint8_t* label;
    int32_t* visible;
    int vec_depth, vec_label;         // 16-byte / 4-byte stores possible
};

// Kept here, not in a shared body: this kernel reads the label from the word, needs no table of labels in LDS and has no colours to
// write, and as an instance of the colour libraries' resolve body it came out slower (profiles/zbuffer_core_probe.txt)
__global__ __launch_bounds__(TPB) void depth_resolve_kernel(ResolveParams P) {
    PVNET_SPARE_VGPRS(31);
    __shared__ int s_count[MAX_INSTANCES];   // pixels won inside this workgroup, per instance
    const int t = threadIdx.x;
    const bool counting = P.visible && P.zbuf;
    if (counting) {
        for (int i = t; i < P.q; i += TPB) s_count[i] = 0;
        __syncthreads();
    }
    const size_t p = ((size_t)blockIdx.x * TPB + t) * 4;
    if (p < P.n) {
        const int np = (int)std::min<size_t>(4, P.n - p);
        unsigned long long word[4] = {NOBODY, NOBODY, NOBODY, NOBODY};
        if (P.zbuf) {
            if (np == 4) {   // p is a multiple of 4 and the z-buffer 16-byte aligned
                const uint4 a = *reinterpret_cast<const uint4*>(P.zbuf + p), b = *reinterpret_cast<const uint4*>(P.zbuf + p + 2);
                word[0] = ((unsigned long long)a.y << 32) | a.x; word[1] = ((unsigned long long)a.w << 32) | a.z;
                word[2] = ((unsigned long long)b.y << 32) | b.x; word[3] = ((unsigned long long)b.w << 32) | b.z;
            } else {
                for (int j = 0; j < np; ++j) word[j] = P.zbuf[p + j];
            }
        }
        float d[4];
        uint32_t labels = 0u;
        int run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t low = (uint32_t)word[j];
            const bool won = low != NOBODY;
            d[j] = won ? __uint_as_float((uint32_t)(word[j] >> 32)) : 0.f;
            labels |= won ? (low & 255u) << (8 * j) : 0u;
            if (counting && won) {   // one LDS add per run of pixels with the same winner
                ++run;
                if (j == 3 || (uint32_t)word[j + 1 < 4 ? j + 1 : 3] != low) {
                    atomicAdd(&s_count[low >> 8], run);
                    run = 0;
                }
            }
        }
        if (P.depth) {
            if (P.vec_depth && np == 4) *reinterpret_cast<float4*>(P.depth + p) = make_float4(d[0], d[1], d[2], d[3]);
            else for (int j = 0; j < np; ++j) P.depth[p + j] = d[j];
        }
        if (P.label) {
            if (P.vec_label && np == 4) *reinterpret_cast<uint32_t*>(P.label + p) = labels;
            else for (int j = 0; j < np; ++j) P.label[p + j] = (uint8_t)(labels >> (8 * j));
        }
    }
    if (counting) {
        __syncthreads();
        for (int i = t; i < P.q; i += TPB) {
            const int c = s_count[i];
            if (c) atomicAdd(&P.visible[i], c);
        }
    }
}

}  // namespace
}  // namespace pvd

using namespace pvd;

extern "C" {

int pvnet_depth_abi_version(void) { return PVNET_DEPTH_ABI_VERSION; }

size_t pvnet_depth_workspace_bytes(int q, int P, int T, int b, int h, int w) { return workspace_bytes(q, P, T, b, h, w); }

int pvnet_render_depth(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                       int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                       const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, float* depth_out,
                       uint8_t* label_out, int32_t* visible_out, int32_t* status_out, void* ws, size_t ws_bytes, void* stream) {
    const Scene S = {{vertices, faces, vertex_offset, face_offset, M, P, T, q, mesh_id, poses, K, k_per_instance, image_id, label, b, h, w}, far};
    int rc, max_f;
    Table tab;
    Workspace W;
    if ((rc = check_scene(S))) return rc;
    if (!depth_out && !label_out) return PVNET_E_BADARG;
    if ((rc = check_instances(S, &tab, &max_f))) return rc;
    if (b == 0) return 0;
    if ((rc = check_workspace(S, ws, ws_bytes, &W))) return rc;
    ResolveParams R;
    resolve_outputs(R, S, W, depth_out, label_out, visible_out);
    return launch(S, W, max_f, status_out, visible_out, stream, depth_setup_kernel, tab, depth_clear_kernel, depth_tri_kernel, depth_resolve_kernel, R);
}

}  // extern "C"
