// shade.hip -- libpvnet_shade.so: shaded vertex-colour images of posed meshes over a background, with the depth, labels and visible
// pixel counts of libpvnet_depth.so from the same call (include/pvnet_shade.h holds THE DEFINITION).
//
// Path replaced (reference tree): the offline OpenGL renderer behind the rendered training images (lib/utils/opengl_render_backend.py:
// 19-102 the shaders, 203-264 the draw, 306-399 the entry point).
//
// The z-buffer of depth.hip with another low word: bits(float32 depth) << 32 | instance << 22 | face.  The words order like (depth,
// instance, face), so the winner of a pixel names the face to shade.  The one copy of the z-buffer lives in zbuffer_core.h (records,
// the setup, clear and triangle kernels' bodies, validation, workspace, launch sequence) and the one copy of a covered pixel's colour
// and of the colour libraries' resolve body in pixel_color.h, which texture.hip compiles too; here are the kernels' names and register
// allowances, the resolve kernel's arguments and the entry points:
//   shade_setup_kernel    one workgroup: the instance table, which arrives in the launch's arguments, becomes records in the
//                         workspace; status, visible counts and counters zeroed
//   shade_clear_kernel    the z-buffer to bits(far) << 32 | 0xFFFFFFFF with 16-byte stores
//   shade_tri_kernel      depth_tri_kernel's walk with FaceWord as its low word: a lane alone up to PVNET_SHADE_LANE_PIXELS pixels, the
//                         wave across a row beyond; coverage and depth are the functions libpvnet_raster.so and libpvnet_depth.so
//                         compile (mesh_core.h, depth_core.h)
//   shade_resolve_kernel  four pixels per lane.  Four untouched words: twelve bytes of background, copied or constant.  A covered word:
//                         the face's three vertices projected again (float32 screen vertices, float64 camera-space vertices), the
//                         definition evaluated in float64, three bytes.  Depth, label bytes and visible counts leave as in
//                         depth_resolve_kernel, the labels from the records: counts in LDS, one integer add per workgroup and instance
// Minima and integer sums do not depend on the order in which they land: the call is bitwise reproducible.
//
// Nothing is contracted (FP_CONTRACT OFF), float32 and float64 denormals are kept (the compiler's default for gfx950).
#include "pvnet_shade.h"
#include "pixel_color.h"

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

PVNET_ZBUFFER_CONSTANTS_ARE(PVNET_SHADE_, MAX_SIDE);
PVNET_SHADING_CONSTANTS_ARE(PVNET_SHADE_);
static_assert(PVNET_SHADE_MAX_FACES == MAX_FACES, "the face index of the low word");

__global__ __launch_bounds__(1024) void shade_setup_kernel(Table T, int q, Inst* recs, int32_t* status, int32_t* visible,
                                                           uint32_t* counters) {
    PVNET_SPARE_VGPRS(31);
    setup_body(T, q, recs, status, visible, counters, NoTexture());
}

__global__ __launch_bounds__(TPB) void shade_clear_kernel(uint4* zbuf, size_t n16, uint32_t far_bits) {
    PVNET_SPARE_VGPRS(31);
    clear_body(zbuf, n16, far_bits);
}

__global__ __launch_bounds__(TPB) void shade_tri_kernel(TriParams P) {
    PVNET_SPARE_VGPRS(103);
    tri_body<FaceWord>(P);
}

struct ResolveParams {
    static constexpr bool TEXTURED = false;
    const unsigned long long* zbuf;   // NULL: no instance at all, background and zeros
    size_t n;                         // pixels of the call: b h w
    uint32_t hw, w;                   // pixels of one image (at most 2^30), of one row
    unsigned long long hw_magic;      // floor((2^64 - 1) / hw): the high half of p * hw_magic is p / hw or one less
    int q;
    const Inst* recs;
    const double* vertices;
    const int32_t* faces;
    const uint8_t* colors;
    const double* normals;
    const double* poses;
    const double* K;
    int k_stride;                     // 0 or 9
    int shading;
    float ambient;
    uint32_t bg[3];                   // twelve bytes: bg_color four times
    const uint8_t* bg_image;          // or NULL
    uint8_t* rgb;
    float* depth;
    uint8_t* label;
    int32_t* visible;
    int vec_rgb, vec_bg, vec_depth, vec_label;   // 4-byte / 4-byte / 16-byte / 4-byte accesses possible
};

__global__ __launch_bounds__(TPB) void shade_resolve_kernel(ResolveParams P) {
    PVNET_SPARE_VGPRS(135);
    resolve_body(P);
}

}  // namespace
}  // namespace pvd

using namespace pvd;

extern "C" {

int pvnet_shade_abi_version(void) { return PVNET_SHADE_ABI_VERSION; }

size_t pvnet_shade_workspace_bytes(int q, int P, int T, int b, int h, int w) { return workspace_bytes(q, P, T, b, h, w); }

int pvnet_render_color(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                       int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                       const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, const uint8_t* colors,
                       const double* normals, int shading, float ambient, const uint8_t* bg_color, const uint8_t* bg_image,
                       uint8_t* rgb_out, float* depth_out, uint8_t* label_out, int32_t* visible_out, int32_t* status_out, void* ws,
                       size_t ws_bytes, void* stream) {
    const Scene S = {{vertices, faces, vertex_offset, face_offset, M, P, T, q, mesh_id, poses, K, k_per_instance, image_id, label, b, h, w}, far};
    int rc, max_f;
    Table tab;
    Workspace W;
    if ((rc = check_shading(shading, ambient))) return rc;
    if ((rc = check_scene(S))) return rc;
    if (!rgb_out || !bg_color) return PVNET_E_BADARG;
    if (P > 0 && !colors) return PVNET_E_BADARG;
    if (shading == SHADING_PHONG && P > 0 && !normals) return PVNET_E_BADARG;
    if ((rc = check_instances(S, &tab, &max_f))) return rc;
    if (max_f > MAX_FACES) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    if ((rc = check_workspace(S, ws, ws_bytes, &W))) return rc;
    ResolveParams R;
    resolve_outputs(R, S, W, depth_out, label_out, visible_out);
    color_arguments(R, S, W, colors, normals, shading, ambient, bg_color, bg_image, rgb_out);
    return launch(S, W, max_f, status_out, visible_out, stream, shade_setup_kernel, tab, shade_clear_kernel, shade_tri_kernel, shade_resolve_kernel, R);
}

}  // extern "C"
