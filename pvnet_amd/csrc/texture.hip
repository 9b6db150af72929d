// texture.hip -- libpvnet_texture.so: the images of libpvnet_shade.so for meshes that may carry a texture image and per-vertex UV
// coordinates, with the depth, labels and visible pixel counts of libpvnet_depth.so from the same call (include/pvnet_texture.h holds
// THE DEFINITION).
//
// Path replaced (reference tree): the u_use_texture branch of the offline OpenGL renderer (lib/utils/opengl_render_backend.py:68-69,
// 95-96 the shaders' last line, 316-323 and 344-352 the texture and its coordinates).
//
// The shade library's four kernels under this library's names: the one copy of the z-buffer lives in zbuffer_core.h and the one copy
// of a covered pixel's colour in pixel_color.h, which shade.hip compiles too, so a mesh without a texture comes out of this library
// exactly as out of that one.  Three additions: the setup kernel writes the texture of an instance's mesh into the two spare words of
// its record (here), the resolve kernel interpolates (u, v) with the weights it has and fetches one or four texels (pixel_color.h,
// compiled where the kernel's arguments say TEXTURED), and the host checks the texture table (here).
//   texture_setup_kernel    one workgroup: the instance table and the textures' sides, which arrive in the launch's arguments,
//                           become records in the workspace (a texture's first texel is the sum of the sizes before it); status,
//                           visible counts and counters zeroed
//   texture_clear_kernel    the z-buffer to bits(far) << 32 | 0xFFFFFFFF with 16-byte stores
//   texture_tri_kernel      the triangle walk with FaceWord as its low word: a lane alone up to PVNET_TEXTURE_LANE_PIXELS pixels, the
//                           wave across a row beyond; coverage and depth are the functions the other three libraries compile
//                           (mesh_core.h, depth_core.h)
//   texture_resolve_kernel  the shade library's resolve layout: four pixels per lane, twelve bytes of background and of colour, 16-byte
//                           depth stores, packed labels, visible counts in LDS with one integer add per workgroup and instance.  A
//                           covered pixel of a textured mesh: u and v by the attribute interpolation, one 4-byte load per texel, the
//                           blend in float64 in the header's order
// Minima and integer sums do not depend on the order in which they land: the call is bitwise reproducible.
//
// Nothing is contracted (FP_CONTRACT OFF), float32 and float64 denormals are kept (the compiler's default for gfx950).
#include "pvnet_texture.h"
#include "pixel_color.h"

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

PVNET_ZBUFFER_CONSTANTS_ARE(PVNET_TEXTURE_, MAX_IMAGE_SIDE);
PVNET_SHADING_CONSTANTS_ARE(PVNET_TEXTURE_SHADING_);
static_assert(PVNET_TEXTURE_MAX_FACES == MAX_FACES, "the face index of the low word");
static_assert(PVNET_TEXTURE_NEAREST == FILTER_NEAREST && PVNET_TEXTURE_BILINEAR == FILTER_BILINEAR, "pixel_color.h's filters");

// the instance table as it travels in texture_setup_kernel's arguments, with, per mesh, the sides of its texture, th << 16 | tw.  (The
// texel offsets do not travel: they are the running sum of th tw, which the host has checked against tex_offset.)
struct TexturedTable : Table {
    uint32_t dims[MAX_MESHES];
};
static_assert(sizeof(TexturedTable) + 48 <= 4096, "kernel arguments: 4 KB with the rest (an int and four pointers)");
static_assert(PVNET_TEXTURE_MAX_SIDE < (1 << 16), "th << 16 | tw");

struct TextureOf {   // the two spare words of a record: the texture of mesh m
    const TexturedTable& T;
    __device__ __forceinline__ void operator()(int m, Inst& r) const {
        r.dims = T.dims[m];
        uint32_t toff = 0u;   // (below 2^31 in all: checked on the host)
        for (int k = 0; k < m; ++k) toff += (T.dims[k] >> 16) * (T.dims[k] & 0xFFFFu);
        r.toff = (int)toff;
    }
};

__global__ __launch_bounds__(1024) void texture_setup_kernel(TexturedTable T, int q, Inst* recs, int32_t* status, int32_t* visible,
                                                             uint32_t* counters) {
    PVNET_SPARE_VGPRS(31);
    setup_body(T, q, recs, status, visible, counters, TextureOf{T});
}

__global__ __launch_bounds__(TPB) void texture_clear_kernel(uint4* zbuf, size_t n16, uint32_t far_bits) {
    PVNET_SPARE_VGPRS(31);
    clear_body(zbuf, n16, far_bits);
}

__global__ __launch_bounds__(TPB) void texture_tri_kernel(TriParams P) {
    PVNET_SPARE_VGPRS(103);
    tri_body<FaceWord>(P);
}

struct ResolveParams {   // the shade library's, with uv and texels behind normals and filter before shading
    static constexpr bool TEXTURED = true;
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
    const float* uv;                  // [P,2]
    const uint32_t* texels;           // R | G << 8 | B << 16 per texel, the textures of the table one after the other
    const double* poses;
    const double* K;
    int k_stride;                     // 0 or 9
    int filter;
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

__global__ __launch_bounds__(TPB) void texture_resolve_kernel(ResolveParams P) {
    PVNET_SPARE_VGPRS(135);
    resolve_body(P);
}

// the texture table: sides first (what is wrong before what is too large), then the offsets, which must be the running sum
int check_textures(int M, const float* uv, const uint32_t* texels, const int64_t* tex_offset, const int32_t* tex_h, const int32_t* tex_w) {
    if (!tex_offset || !tex_h || !tex_w) return PVNET_E_BADARG;
    bool textured = false;
    for (int m = 0; m < M; ++m) {
        if (tex_h[m] < 0 || tex_w[m] < 0 || (tex_h[m] == 0) != (tex_w[m] == 0)) return PVNET_E_BADARG;
        textured = textured || tex_h[m] > 0;
    }
    if (textured && (!uv || !texels)) return PVNET_E_BADARG;
    for (int m = 0; m < M; ++m)
        if (tex_h[m] > PVNET_TEXTURE_MAX_SIDE || tex_w[m] > PVNET_TEXTURE_MAX_SIDE) return PVNET_E_UNSUPPORTED;
    if (tex_offset[0] != 0) return PVNET_E_BADARG;
    for (int m = 0; m < M; ++m)   // (a side is at most 2^14: the product at most 2^28, the sum over 64 meshes at most 2^34)
        if (tex_offset[m + 1] != tex_offset[m] + (int64_t)tex_h[m] * (int64_t)tex_w[m]) return PVNET_E_BADARG;
    if (tex_offset[M] >= (int64_t)1 << 31) return PVNET_E_UNSUPPORTED;
    return 0;
}

}  // namespace
}  // namespace pvd

using namespace pvd;

extern "C" {

int pvnet_texture_abi_version(void) { return PVNET_TEXTURE_ABI_VERSION; }

size_t pvnet_texture_workspace_bytes(int q, int P, int T, int b, int h, int w) { return workspace_bytes(q, P, T, b, h, w); }

int pvnet_render_textured(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                          int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                          const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, const uint8_t* colors,
                          const double* normals, const float* uv, const uint32_t* texels, const int64_t* tex_offset,
                          const int32_t* tex_h, const int32_t* tex_w, int filter, int shading, float ambient, const uint8_t* bg_color,
                          const uint8_t* bg_image, uint8_t* rgb_out, float* depth_out, uint8_t* label_out, int32_t* visible_out,
                          int32_t* status_out, void* ws, size_t ws_bytes, void* stream) {
    const Scene S = {{vertices, faces, vertex_offset, face_offset, M, P, T, q, mesh_id, poses, K, k_per_instance, image_id, label, b, h, w}, far};
    int rc, max_f;
    TexturedTable tab;
    Workspace W;
    if (filter < FILTER_NEAREST || filter > FILTER_BILINEAR) return PVNET_E_BADARG;
    if ((rc = check_shading(shading, ambient))) return rc;
    if ((rc = check_scene(S))) return rc;
    if (!rgb_out || !bg_color) return PVNET_E_BADARG;
    if (shading == SHADING_PHONG && P > 0 && !normals) return PVNET_E_BADARG;
    if ((rc = check_textures(M, uv, texels, tex_offset, tex_h, tex_w))) return rc;
    if ((rc = check_instances(S, &tab, &max_f))) return rc;
    for (int i = 0; i < q; ++i)   // an untextured mesh is drawn: it needs its colours
        if (!colors && P > 0 && tex_h[mesh_id[i]] == 0) return PVNET_E_BADARG;
    if (max_f > MAX_FACES) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    if ((rc = check_workspace(S, ws, ws_bytes, &W))) return rc;
    for (int m = 0; m < MAX_MESHES; ++m) tab.dims[m] = m < M ? ((uint32_t)tex_h[m] << 16) | (uint32_t)tex_w[m] : 0u;
    ResolveParams R;
    resolve_outputs(R, S, W, depth_out, label_out, visible_out);
    color_arguments(R, S, W, colors, normals, shading, ambient, bg_color, bg_image, rgb_out);
    R.uv = uv; R.texels = texels; R.filter = filter;
    return launch(S, W, max_f, status_out, visible_out, stream, texture_setup_kernel, tab, texture_clear_kernel, texture_tri_kernel, texture_resolve_kernel,
                  R);
}

}  // extern "C"
