/* pvnet_depth.h -- C ABI of libpvnet_depth.so: depth images, occlusion-correct label images and visible pixel counts of posed meshes.
 *
 * The reference makes Occlusion LINEMOD's label images from depth: OcclusionLineModDB.get_mask_of_all_objects
 * (lib/utils/data_utils.py:788-826) renders a depth image per object and keeps, per pixel, the label of the object with the smallest
 * depth (the depth map starts at 10, the comparison is a strict `<`, so the earlier object wins a tie).  Its depth images come from an
 * OpenGL renderer; the native render_mesh_depth it declares (lib/utils/extend_utils/extend_utils.py:196-213) has no body.  So the
 * depth of a pixel is THIS PROJECT'S OWN definition, stated here; the composition is the reference's.  libpvnet_raster.so composes in
 * painter's order, which no order makes equal to this for instances that interpenetrate or wrap around each other.
 * A numpy restatement: tests/depth_restatement.py.  The header, the restatement and the kernels are held to each other bit for bit.
 *
 * THE DEFINITION
 *
 * Instances: (mesh id, pose [3,4] float64, K, target image, label 1 .. 255), the instance table of pvnet_render (pvnet_raster.h).
 *
 * Coverage: stage P then stage R of pvnet_raster.h, unchanged (the kernels compile the same functions, pvnet_amd/csrc/mesh_core.h):
 * the vertices are projected in float64 in that header's operation order, u and v rounded to float32, and a pixel of the triangle's
 * inclusive box belongs to the triangle when the float32 same_side predicate holds for the three edges.  The depth image of one
 * instance alone (far = +inf) is therefore non-zero exactly where pvnet_render's mask is 1, whenever the instance's status is 0.
 *
 * Depth of a covered pixel (px, py) under one triangle.  z0, z1, z2: the camera-space z of its vertices, each the c_2 of stage P in
 * float64.  (x0,y0), (x1,y1), (x2,y2): its float32 screen vertices promoted to float64.  All arithmetic is float64, every operation
 * rounded once, nothing contracted, in the order written:
 *     i_k  = 1 / z_k
 *     zmin = min(z0, z1, z2),  zmax = max(z0, z1, z2)
 *     area = (x1-x0)(y2-y0) - (x2-x0)(y1-y0)
 *     b = ((i1-i0)(y2-y0) - (i2-i0)(y1-y0)) / area
 *     c = ((i2-i0)(x1-x0) - (i1-i0)(x2-x0)) / area                 per triangle, once
 *     inv = (i0 + b (px-x0)) + c (py-y0)
 *     d = 1 / inv                                                   per pixel
 *     if area == 0:    d = zmin
 *     if !(d >= zmin): d = zmin                                     (this also catches NaN and negative values)
 *     if d > zmax:     d = zmax
 *     depth = (float) d                                             one rounding to float32
 * Inverse depth is affine on the screen for a planar triangle under any K, so this is the exact plane depth up to the float32 rounding
 * of u and v.  Stage R's predicate covers some pixels outside the true triangle (its `>=`, its box `+ 1`, point triangles, collinear
 * triangles): the clamp makes the value defined and bounded there.
 *
 * DEVIATIONS from the silhouette library, which draws such triangles:
 *   - a triangle with a vertex at (float) z_k <= 0 or with a non-finite z_k is not drawn and sets PVNET_DEPTH_S_BEHIND on its instance
 *     (there is no depth to give it; pvnet_render reports the bit per mesh vertex and rasterises whatever stage P yields);
 *   - as there, a triangle with a non-finite screen coordinate is not drawn and sets PVNET_DEPTH_S_NONFINITE.
 * Each condition sets its own bit: a NaN pose sets both.
 *
 * Composition.  `far` is float32, > 0 and not NaN (+inf: keep everything).  A candidate is kept only when depth < far.  A pixel takes
 * the smallest kept depth over all triangles of all instances of its image; at equal float32 depth the instance earlier in the list
 * wins.  far = 10 reproduces the reference's get_mask_of_all_objects.  The result does not depend on the order in which triangles or
 * atomics land.
 *
 * Outputs, each optional (NULL) but at least one of depth_out / label_out is required; every byte of a given output is written:
 *     depth_out   [b,h,w] float32   the kept depth, 0 where nothing is kept (the background of the reference's `depth != 0`)
 *     label_out   [b,h,w] uint8     the label of the winning instance, 0 for background
 *     visible_out [q] int32         the pixels each instance wins
 *     status_out  [q] int32         PVNET_DEPTH_S_* bits
 *
 * THE KERNELS (pvnet_amd/csrc/depth.hip): at most four launches per call, all on `stream`; no allocation, no synchronisation,
 * capturable in a graph.  The z-buffer is one 64-bit word per pixel in the workspace: the float32 depth's bit pattern above the
 * instance's index in the call, so an unsigned minimum takes the nearest depth and, at a tie, the earlier instance.  It and the
 * counters are cleared inside every call: the workspace may hold anything on entry.
 */
#ifndef PVNET_DEPTH_H_
#define PVNET_DEPTH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_DEPTH_ABI_VERSION 1

/* the error codes of pvnet_vote.h */
#ifndef PVNET_E_BADARG
#define PVNET_E_BADARG      (-1)
#define PVNET_E_WORKSPACE   (-2)
#define PVNET_E_UNSUPPORTED (-3)
#endif

/* the limits of pvnet_render, under this header's names (one table serves only its own header's names) */
#define PVNET_DEPTH_LANE_PIXELS 64
#define PVNET_DEPTH_MAX_INSTANCES 768
#define PVNET_DEPTH_MAX_MESHES 64
#define PVNET_DEPTH_MAX_IMAGES 65535
#define PVNET_DEPTH_MAX_SIDE 32768

/* status bits per instance */
#define PVNET_DEPTH_S_NONFINITE 1 /* a triangle with a non-finite screen coordinate was skipped */
#define PVNET_DEPTH_S_BEHIND    2 /* a triangle with a vertex at camera z <= 0 (as float32), or a non-finite z, was skipped */
#define PVNET_DEPTH_S_BADFACE   4 /* a face names a vertex outside its mesh and was skipped (the host validates faces; this guards) */

int pvnet_depth_abi_version(void);

/* Bytes of workspace for q instances composed into b images of h x w pixels.  P and T, the vertices and faces of the mesh table, are
 * part of the signature and checked, but nothing is stored per vertex or face.  0 for an argument out of range. */
size_t pvnet_depth_workspace_bytes(int q, int P, int T, int b, int h, int w);

/* The mesh table and the instances are those of pvnet_render (pvnet_raster.h): HOST arrays, read before the call returns, are
 * vertex_offset, face_offset, mesh_id, image_id, label; everything else is device memory.
 *   vertices [P,3] float64, faces [T,3] int32 (local to their mesh), vertex_offset / face_offset [M+1] int32
 *   q instances: mesh_id [q], poses [q,3,4] float64, K [3,3] float64 (k_per_instance == 0) or [q,3,3], image_id [q] non-decreasing in
 *                0 .. b-1, label [q] in 1 .. 255
 *   far          float32, > 0, not NaN
 *   depth_out, label_out, visible_out, status_out: see Outputs above
 *   ws           pvnet_depth_workspace_bytes(q, P, T, b, h, w) bytes, 16-byte aligned
 * At most four launches.  b == 0 returns 0 and enqueues nothing; q == 0 writes zeros; an image with no instance is zeros.
 * Returns 0, a positive hipError_t, PVNET_E_BADARG (what pvnet_render rejects, far <= 0 or NaN, neither depth_out nor label_out),
 * PVNET_E_WORKSPACE or PVNET_E_UNSUPPORTED (q > PVNET_DEPTH_MAX_INSTANCES, M > PVNET_DEPTH_MAX_MESHES, b > PVNET_DEPTH_MAX_IMAGES, a
 * side above PVNET_DEPTH_MAX_SIDE).  Bad arguments are rejected before any HIP call. */
int pvnet_render_depth(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                       int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                       const int32_t* image_id, const int32_t* label, int b, int h, int w, float far, float* depth_out,
                       uint8_t* label_out, int32_t* visible_out, int32_t* status_out, void* ws, size_t ws_bytes, void* stream);

/* Development aid: the triangles of the last call on this workspace that took the cooperative path, as the call left it in the
 * workspace's first word (a device address; copy it out after synchronising). */
#define PVNET_DEPTH_WS_COOP_COUNT_OFFSET 0

#ifdef __cplusplus
}
#endif
#endif /* PVNET_DEPTH_H_ */
