/* pvnet_texture.h -- C ABI of libpvnet_texture.so: pvnet_render_color (pvnet_shade.h) for meshes that may carry a texture image and
 * per-vertex UV coordinates.  A covered pixel of a textured mesh takes its colour from the texture instead of from the interpolated
 * vertex colours; everything else -- rgb over a background, depth, occlusion-correct labels, visible counts, status, the composition --
 * is pvnet_render_color's.  Meshes with and without a texture may be mixed in one call and in one image.
 *
 * Both of the reference's fragment shaders end in a branch on u_use_texture that replaces the vertex colour by the texture's sample at
 * the interpolated coordinate, times the light weight (lib/utils/opengl_render_backend.py:68-69, 95-96); its render() flips the texture image and binds model['texture_uv'] per vertex
 * (316-323, 344-352), which OpenGLRenderer.load_ply reads from the vertex properties texture_u / texture_v
 * (lib/utils/render_utils.py:424-427, 471-473).  A numpy restatement of this header: tests/texture_restatement.py.  The header, the
 * restatement and the kernels are held to each other bit for bit.
 *
 * WHAT IS THIS PROJECT'S OWN, AND WHAT IS BELIEVED BUT NOT CHECKED
 *   - the texel value of a pixel is THIS PROJECT'S OWN definition, stated below.  The reference's renderer needs an OpenGL context and
 *     the glumpy package, neither of which was available: no pixel of the reference could be recorded, and none is compared against;
 *   - nearest filtering with clamp-to-edge is, as far as can be told without glumpy, what the reference gets from glumpy's default
 *     Texture2D.  That is a belief, not a checked fact;
 *   - alpha is ignored: the reference multiplies the vec4 by light_w and keeps rgb (opengl_render_backend.py:260);
 *   - there are no mip levels and no repeat wrap;
 *   - the deviations of pvnet_shade.h from the shaders (the light vector from the pixel's eye point, normals as three-vectors, the flat
 *     normal facing the viewer) hold here unchanged.
 *
 * THE DEFINITION
 *
 * Unchanged, by reference:
 *   pvnet_depth.h   instances and coverage; the depth of a covered pixel under one triangle; `far`; the skipped triangles and the status
 *                   bits (the kernels compile the same functions: pvnet_amd/csrc/mesh_core.h, pvnet_amd/csrc/depth_core.h, and the
 *                   one z-buffer of pvnet_amd/csrc/zbuffer_core.h);
 *   pvnet_shade.h   the composition order (depth, then instance, then face); C_k, z_k and the float32 screen vertex (x_k, y_k); the
 *                   screen barycentrics l_k with their clamps; the perspective weights w_k = l_k / z_k, s, and the interpolation A(a)
 *                   with its fallback a0; the eye point e; the three light terms (none / flat / Phong); the final
 *                   v = floor(light c[ch] + 0.5) clamped to 0 .. 255; the background.
 * All arithmetic is float64, every operation rounded once, nothing contracted, in the order written.  Only the source of c[ch] changes,
 * and only for a textured mesh.
 *
 * Inputs beyond pvnet_render_color's, per mesh m of the table:
 *     uv          [P,2] float32, device: the per-vertex texture coordinates (the reference's a_texcoord), promoted to float64; any value,
 *                 NaN and infinities included.  Rows of untextured meshes are never read
 *     texels      one little-endian uint32 per texel, device: R | G << 8 | B << 16, top byte 0 (it is ignored).  Row-major, the TOP row
 *                 of the image first, exactly as the image was loaded: the reference's np.flipud and OpenGL's bottom-left origin are
 *                 folded into `row` below, nothing is flipped in memory.  The textures of the table are concatenated
 *     tex_offset  [M+1] int64, HOST: first texel of mesh m; tex_offset[0] == 0, tex_offset[m+1] == tex_offset[m] + tex_h[m] tex_w[m]
 *     tex_h, tex_w [M] int32, HOST: th x tw texels.  tex_h[m] == 0 (then tex_w[m] == 0 too) means UNTEXTURED: the pixel's colour is
 *                 c[ch] = A(colour_.[ch]) as in pvnet_render_color
 *     filter      PVNET_TEXTURE_NEAREST or PVNET_TEXTURE_BILINEAR, one for all meshes of the call
 * The host arrays are read before the call returns, like vertex_offset.
 *
 * Colour of a covered pixel of a mesh with th x tw texels t[row][column][ch], won by a face whose vertices carry (u_k, v_k):
 *     u = A(u_.),  v = A(v_.)                                  perspective-correct: the same A, the same weights as for colours
 *     if !(u >= 0): u = 0;  if u > 1: u = 1;  the same for v     clamp to edge; NaN becomes 0
 *   nearest:
 *     i = min((int) floor(u tw), tw - 1),  j = min((int) floor(v th), th - 1),  row = th - 1 - j
 *     c[ch] = (double) t[row][i][ch]
 *   bilinear:
 *     x = u tw - 0.5,  i0 = floor(x),  fx = x - i0,  ia = max(i0, 0),  ib = min(i0 + 1, tw - 1)
 *     y = v th - 0.5,  j0 = floor(y),  fy = y - j0,  ja = max(j0, 0),  jb = min(j0 + 1, th - 1)
 *     ra = th - 1 - ja,  rb = th - 1 - jb
 *     lo = (1 - fx) t[ra][ia][ch] + fx t[ra][ib][ch],   hi = (1 - fx) t[rb][ia][ch] + fx t[rb][ib][ch]
 *     c[ch] = (1 - fy) lo + fy hi
 * (v = 0 is the BOTTOM row of the image as loaded, v = 1 its top; texel centres are at (i + 0.5) / tw.)  c[ch] then enters
 * v = floor(light c[ch] + 0.5) of pvnet_shade.h.
 *
 * THE KERNELS (pvnet_amd/csrc/texture.hip): at most four launches per call, all on `stream`; no allocation, no synchronisation,
 * capturable in a graph, bitwise reproducible.  The z-buffer word is pvnet_shade.h's, bits(float32 depth) << 32 | instance << 22 | face;
 * the z-buffer and the counters are cleared inside every call: the workspace may hold anything on entry.  The resolve kernel
 * interpolates u and v with the weights it has and fetches one texel (nearest) or four (bilinear) with one 4-byte load each.
 */
#ifndef PVNET_TEXTURE_H_
#define PVNET_TEXTURE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_TEXTURE_ABI_VERSION 1

/* the error codes of pvnet_vote.h */
#ifndef PVNET_E_BADARG
#define PVNET_E_BADARG      (-1)
#define PVNET_E_WORKSPACE   (-2)
#define PVNET_E_UNSUPPORTED (-3)
#endif

/* the limits of pvnet_render_color, under this header's names (PVNET_TEXTURE_MAX_IMAGE_SIDE is its PVNET_SHADE_MAX_SIDE) */
#define PVNET_TEXTURE_LANE_PIXELS 64
#define PVNET_TEXTURE_MAX_INSTANCES 768
#define PVNET_TEXTURE_MAX_MESHES 64
#define PVNET_TEXTURE_MAX_IMAGES 65535
#define PVNET_TEXTURE_MAX_IMAGE_SIDE 32768
#define PVNET_TEXTURE_MAX_FACES 4194304
/* texels along one side of one texture; all textures of a table together hold fewer than 2^31 texels */
#define PVNET_TEXTURE_MAX_SIDE 16384

/* status bits per instance: those of pvnet_depth.h */
#define PVNET_TEXTURE_S_NONFINITE 1
#define PVNET_TEXTURE_S_BEHIND    2
#define PVNET_TEXTURE_S_BADFACE   4

/* shading: the values of pvnet_shade.h */
#define PVNET_TEXTURE_SHADING_NONE  0
#define PVNET_TEXTURE_SHADING_FLAT  1
#define PVNET_TEXTURE_SHADING_PHONG 2

/* filter */
#define PVNET_TEXTURE_NEAREST  0
#define PVNET_TEXTURE_BILINEAR 1

int pvnet_texture_abi_version(void);

/* The bytes pvnet_shade_workspace_bytes answers for the same arguments: 8 per pixel, 32 per instance, 16.  Textures need no
 * workspace.  0 for an argument out of range. */
size_t pvnet_texture_workspace_bytes(int q, int P, int T, int b, int h, int w);

/* pvnet_render_color's arguments (pvnet_shade.h) with uv, texels, tex_offset, tex_h, tex_w and filter (above) inserted after `normals`.
 *   colors      may be NULL when every mesh an instance names is textured (a textured mesh's colours are never read)
 *   uv, texels  may be NULL when no mesh of the table is textured
 *   ws          pvnet_texture_workspace_bytes(q, P, T, b, h, w) bytes, 16-byte aligned
 * At most four launches.  b == 0 returns 0 and enqueues nothing; q == 0 writes the background (and zeros).
 * Returns 0, a positive hipError_t, PVNET_E_BADARG (what pvnet_render_color rejects but for colors, see above; tex_offset, tex_h or tex_w
 * NULL; a textured mesh without uv or texels; tex_h or tex_w negative, or only one of them zero; tex_offset[0] != 0 or an offset that does
 * not increase by th tw; a filter outside 0 .. 1), PVNET_E_WORKSPACE or PVNET_E_UNSUPPORTED (pvnet_render_color's limits under the names
 * above; a texture side beyond PVNET_TEXTURE_MAX_SIDE; 2^31 texels or more in the table).  Bad arguments are rejected before any HIP
 * call. */
int pvnet_render_textured(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                          int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                          const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, const uint8_t* colors,
                          const double* normals, const float* uv, const uint32_t* texels, const int64_t* tex_offset,
                          const int32_t* tex_h, const int32_t* tex_w, int filter, int shading, float ambient, const uint8_t* bg_color,
                          const uint8_t* bg_image, uint8_t* rgb_out, float* depth_out, uint8_t* label_out, int32_t* visible_out,
                          int32_t* status_out, void* ws, size_t ws_bytes, void* stream);

/* Development aid: the triangles of the last call on this workspace that took the cooperative path, as the call left it in the
 * workspace's first word (a device address; copy it out after synchronising). */
#define PVNET_TEXTURE_WS_COOP_COUNT_OFFSET 0

#ifdef __cplusplus
}
#endif
#endif /* PVNET_TEXTURE_H_ */
