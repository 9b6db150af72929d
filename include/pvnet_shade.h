/* pvnet_shade.h -- C ABI of libpvnet_shade.so: shaded vertex-colour images of posed meshes over a background, with the depth,
 * occlusion-correct labels and visible pixel counts of pvnet_render_depth (pvnet_depth.h) from the same call.
 *
 * The reference renders its 10 000 synthetic training images per class offline with an OpenGL / Blender renderer
 * (lib/utils/opengl_render_backend.py:19-102 the shaders, 203-264 the draw, 306-399 the entry point): vertex colours, one light at the
 * camera, an ambient weight, flat or Phong shading.  That renderer needs an OpenGL context, so the value of a pixel is THIS PROJECT'S
 * OWN definition, stated here; it follows the structure of the reference's shaders.  A numpy restatement: tests/shade_restatement.py.
 * The header, the restatement and the kernels are held to each other bit for bit; an independent float64 ray caster of the GLSL
 * formulas checks the restatement (tests/test_shade_cpu.py).
 *
 * DIFFERENCES from the reference's shaders, all deliberate (measured by tests/test_shade_cpu.py on a sphere of 1 280 small faces and on
 * a box of 0.3 m seen from 0.7 m; profiles/shade_probe.txt):
 *   - textures (the shaders' u_use_texture) are NOT built: LINEMOD's meshes carry vertex colours;
 *   - the light vector: the shaders normalise `light - v_eye_pos` per VERTEX and interpolate it (v_L, line 43); here the direction is
 *     taken from the pixel's own eye point, the light being at the camera.  Nothing beyond the uint8 rounding on the sphere, up to 4.4
 *     grey levels (flat) and 5.2 (Phong) on the box;
 *   - the normal matrix: the shaders transform a normal as the four-vector (a_normal, 1) by inverse(model view)^T and normalise all
 *     four components (line 44), which shortens each vertex normal by 1 / sqrt(1 + (1 - t . R a_normal)^2) before interpolation; here
 *     R a_normal itself is interpolated.  0.2 grey levels on the sphere; up to 35.5 (mean 3.7 .. 5.5) on the box, whose corner normals
 *     point far apart.  Flat shading does not read the normals;
 *   - the flat normal faces the viewer whatever the winding (the shaders' derivative cross product does so for the reference's view).
 * With the second and third removed from a ray caster of the shaders, it and this definition agree within the rounding to uint8.
 *
 * THE DEFINITION
 *
 * Instances, coverage, the depth of a covered pixel under one triangle, `far`, the skipped triangles and the status bits: pvnet_depth.h,
 * unchanged (the kernels compile the same functions: pvnet_amd/csrc/mesh_core.h, pvnet_amd/csrc/depth_core.h).
 *
 * Composition.  A pixel takes the smallest kept depth over all triangles of all instances of its image; at equal float32 depth the
 * instance earlier in the list wins, and between two faces of one instance the lower face index (local to its mesh).  Depth, labels,
 * visible counts and status therefore equal pvnet_render_depth's on the same inputs.  The result does not depend on the order in which
 * triangles or atomics land.
 *
 * Colour of a covered pixel (px, py), won by face (i0, i1, i2) of an instance with pose [R|t].  All arithmetic is float64, every
 * operation rounded once (sqrt and the divisions correctly rounded), nothing contracted, in the order written; k = 0, 1, 2:
 *     C_k[r] = ((R[r][0] X_k[0] + R[r][1] X_k[1]) + R[r][2] X_k[2]) + t[r]          the camera-space vertex: stage P's c_0, c_1, c_2
 *     z_k    = C_k[2]
 *     (x_k, y_k): stage P's float32 screen vertex, promoted to float64
 *   screen barycentrics
 *     dx1 = x1-x0, dy1 = y1-y0, dx2 = x2-x0, dy2 = y2-y0, ex = px-x0, ey = py-y0
 *     area = dx1 dy2 - dx2 dy1                                                       (the area of pvnet_depth.h)
 *     l1 = (ex dy2 - dx2 ey) / area,   l2 = (dx1 ey - ex dy1) / area,   l0 = (1 - l1) - l2
 *     each l: if !(l >= 0): l = 0;  if l > 1: l = 1           (stage R covers some pixels outside the true triangle; NaN becomes 0)
 *   perspective weights
 *     w_k = l_k / z_k,   s = (w0 + w1) + w2
 *     an attribute with vertex values a0, a1, a2:   A(a) = ((w0 a0 + w1 a1) + w2 a2) / s;   if area == 0 or !(s > 0):  A(a) = a0
 *     e[r] = A(C_.[r])                     the eye point
 *     c[ch] = A(colour_.[ch])              the vertex colours as 0 .. 255
 *   diffuse term, |v| = sqrt((v0 v0 + v1 v1) + v2 v2), dot(u, v) = (u0 v0 + u1 v1) + u2 v2
 *     flat:   a = C_1 - C_0, b = C_2 - C_0, g = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
 *             diffuse = |dot(e, g)| / (|e| |g|);  0 when |e| == 0 or |g| == 0
 *             (the shaders' cross(dFdx(v_eye_pos), dFdy(v_eye_pos)) always faces the viewer; this is that, independent of winding)
 *     Phong:  m_k[r] = (R[r][0] N_k[0] + R[r][1] N_k[1]) + R[r][2] N_k[2],  n[r] = A(m_.[r])
 *             diffuse = (-dot(e, n)) / (|e| |n|);  if !(diffuse > 0): diffuse = 0;  0 when |e| == 0 or |n| == 0
 *   light
 *     none:   light = 1
 *     else:   light = (double) ambient + diffuse;  if !(light < 1): light = 1        (the shaders' light_w, the light at the camera)
 *   per channel
 *     v = floor(light c[ch] + 0.5);  if !(v >= 0): v = 0;  if v > 255: v = 255;  out = (uint8) v
 * A pixel no kept candidate reached takes the background: bg_image's pixel when bg_image is given, else bg_color.
 *
 * Outputs; rgb_out is required, the others optional (NULL); every byte of a given output is written:
 *     rgb_out     [b,h,w,3] uint8   the layout pvnet_augment reads
 *     depth_out   [b,h,w] float32,  label_out [b,h,w] uint8,  visible_out [q] int32,  status_out [q] int32: as pvnet_render_depth
 *
 * THE KERNELS (pvnet_amd/csrc/shade.hip): at most four launches per call, all on `stream`; no allocation, no synchronisation,
 * capturable in a graph, bitwise reproducible.  The z-buffer is one 64-bit word per pixel in the workspace,
 *     bits(float32 depth) << 32 | instance << 22 | face,
 * so one unsigned minimum orders by depth, then instance, then face; a pixel nobody reached keeps a low word of all ones, which no
 * instance below PVNET_SHADE_MAX_INSTANCES produces.  The resolve kernel finds (instance, face) in the word, projects the face's three
 * vertices again and evaluates the definition.  The z-buffer and the counters are cleared inside every call: the workspace may hold
 * anything on entry.
 */
#ifndef PVNET_SHADE_H_
#define PVNET_SHADE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_SHADE_ABI_VERSION 1

/* the error codes of pvnet_vote.h */
#ifndef PVNET_E_BADARG
#define PVNET_E_BADARG      (-1)
#define PVNET_E_WORKSPACE   (-2)
#define PVNET_E_UNSUPPORTED (-3)
#endif

/* the limits of pvnet_render_depth, under this header's names, and the faces of one mesh (the face index has 22 bits of the word) */
#define PVNET_SHADE_LANE_PIXELS 64
#define PVNET_SHADE_MAX_INSTANCES 768
#define PVNET_SHADE_MAX_MESHES 64
#define PVNET_SHADE_MAX_IMAGES 65535
#define PVNET_SHADE_MAX_SIDE 32768
#define PVNET_SHADE_MAX_FACES 4194304

/* status bits per instance: those of pvnet_depth.h */
#define PVNET_SHADE_S_NONFINITE 1
#define PVNET_SHADE_S_BEHIND    2
#define PVNET_SHADE_S_BADFACE   4

/* shading */
#define PVNET_SHADE_NONE  0 /* the interpolated vertex colour */
#define PVNET_SHADE_FLAT  1 /* the face normal */
#define PVNET_SHADE_PHONG 2 /* the interpolated vertex normals */

int pvnet_shade_abi_version(void);

/* Bytes of workspace for q instances composed into b images of h x w pixels: 8 per pixel, 32 per instance, 16.  P and T are part of
 * the signature and checked, but nothing is stored per vertex or face.  0 for an argument out of range. */
size_t pvnet_shade_workspace_bytes(int q, int P, int T, int b, int h, int w);

/* The arguments of pvnet_render_depth (pvnet_depth.h) through `far`, with the same meaning, then:
 *   colors      [P,3] uint8, device: the vertex colours of the mesh table
 *   normals     [P,3] float64, device: the vertex normals; read only when shading == PVNET_SHADE_PHONG, NULL otherwise allowed
 *   shading     PVNET_SHADE_NONE / _FLAT / _PHONG
 *   ambient     float32, finite, >= 0
 *   bg_color    [3] uint8, HOST, read before the call returns
 *   bg_image    [b,h,w,3] uint8, device, or NULL: bg_color everywhere
 *   rgb_out     [b,h,w,3] uint8, required;  depth_out, label_out, visible_out, status_out: optional, as pvnet_render_depth
 *   ws          pvnet_shade_workspace_bytes(q, P, T, b, h, w) bytes, 16-byte aligned
 * At most four launches.  b == 0 returns 0 and enqueues nothing; q == 0 writes the background (and zeros); an image with no instance
 * is its background.
 * Returns 0, a positive hipError_t, PVNET_E_BADARG (what pvnet_render_depth rejects but for its need of depth_out or label_out; no
 * rgb_out, colors or bg_color; shading outside 0 .. 2; Phong without normals; ambient negative or not finite), PVNET_E_WORKSPACE or
 * PVNET_E_UNSUPPORTED (the limits above; an instance's mesh with more than PVNET_SHADE_MAX_FACES faces).  Bad arguments are rejected
 * before any HIP call. */
int pvnet_render_color(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                       int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                       const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, const uint8_t* colors,
                       const double* normals, int shading, float ambient, const uint8_t* bg_color, const uint8_t* bg_image,
                       uint8_t* rgb_out, float* depth_out, uint8_t* label_out, int32_t* visible_out, int32_t* status_out, void* ws,
                       size_t ws_bytes, void* stream);

/* Development aid: the triangles of the last call on this workspace that took the cooperative path, as the call left it in the
 * workspace's first word (a device address; copy it out after synchronising). */
#define PVNET_SHADE_WS_COOP_COUNT_OFFSET 0

#ifdef __cplusplus
}
#endif
#endif /* PVNET_SHADE_H_ */
