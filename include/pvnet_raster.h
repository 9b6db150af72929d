/* pvnet_raster.h -- C ABI of libpvnet_raster.so: silhouettes and label images of posed meshes on the device.
 *
 * The reference's helper library has one native function that goes from a pose back to pixels: mesh_binary_rasterization
 * (lib/utils/extend_utils/src/mesh_rasterization.cpp:43-71, called through extend_utils.py:7-20), the triangle-coverage mask of a
 * projected mesh.  This library is that function for a batch (stage R), the projection its caller puts in front of it (stage P) and
 * the composition of several instances into one label image (stage C).  A numpy restatement: tests/raster_restatement.py.
 *
 * THE DEFINITION
 *
 * Stage R, triangles to mask, per image: tri [tn,3,2] float32 -> mask [h,w] uint8, 0 or 1.  All arithmetic is float32, one IEEE
 * rounding per operation, nothing contracted into a fused multiply-add, denormals kept.  For every triangle (x0,y0),(x1,y1),(x2,y2):
 *     minx = max(0, min(x0,x1,x2)),  maxx = min((float)(w - 2), max(x0,x1,x2));  miny, maxy likewise with h
 *     begx = (int)minx,  endx = (int)(maxx + 1.f);  begy, endy likewise               (truncation; both ends inclusive)
 *     the pixel (xi, yi) of that box is set when same_side holds for the three edges (0,1; third 2), (1,2; third 0), (2,0; third 1)
 *     same_side of the edge (xa,ya)-(xb,yb) with third vertex (tx,ty) and the pixel (px,py) = ((float)xi, (float)yi):
 *         dx = xb - xa,  dy = yb - ya,  nx = -dy,  ny = dx
 *         val0 = (tx - xa) nx + (ty - ya) ny,   val1 = (px - xa) nx + (py - ya) ny       (two products, one sum: three roundings)
 *         holds when val0 val1 >= 0
 * The mask is the OR over all triangles: the reference's `if(mask[...]) continue` is an early-out only, so neither the order of the
 * triangles nor the order in which the kernels' atomics land changes the result.  What the loop bounds and `>=` imply belongs to the
 * definition: a point triangle sets its 2 x 2 box, three collinear vertices set their whole box, column w - 1 and row h - 1 are
 * reached through the `+ 1`, and (0,0),(1e-14,0),(0,1e-14) sets exactly one pixel because its edge products are float32 denormals
 * of either sign.
 *
 * Where the reference's C is undefined this library defines the result (DEVIATIONS; never compared with the reference there):
 *   - a triangle with a non-finite coordinate covers nothing and sets PVNET_RASTER_S_NONFINITE on its instance;
 *   - the box is empty when minx >= (float)w or maxx + 1.f <= -1.f (and likewise in y), compared in float BEFORE any cast: a
 *     triangle at 1e30 or -1e30 covers nothing.  Wherever the reference's casts are defined these two comparisons decide exactly
 *     what its integer loop bounds decide (begx >= w > endx, or endx <= -1 < begx), so nothing else changes;
 *   - h, w >= 2 are required (the reference reads outside the image below that).
 *
 * Stage P, pose to triangles: the reference caller's Projector.project_K (lib/utils/base_utils.py:290-294) followed by
 * np.ascontiguousarray(..., np.float32) (extend_utils.py:13), in float64, every operation rounded once, in this order:
 *     c_r = ((R[r,0] X0 + R[r,1] X1) + R[r,2] X2) + t[r]          r = 0, 1, 2;  pose = [R | t], [3,4]
 *     p_r = (K[r,0] c0 + K[r,1] c1) + K[r,2] c2
 *     u = p0 / p2,  v = p1 / p2,  each then rounded to float32
 * (The reference multiplies with BLAS, whose summation order is not defined: P is held bit for bit to the restatement and within one
 * float32 ulp to the reference's recorded output.)  There is no near-plane clipping, as in the reference: an instance with any vertex
 * of its mesh at c2 <= 0 gets PVNET_RASTER_S_BEHIND and its triangles are rasterised from whatever P yields.
 *
 * Stage C, composition: an instance is (mesh id, pose, K, target image, label).  A target image starts at 0; a pixel takes the label
 * of the LAST instance, in painter's order, that covers it.  Painter's order is the order of the list, or, with `order`, ascending
 * order[i] among the instances of an image (ties: list order); the caller paints far to near.  `out` is overwritten, never OR-ed into.
 *
 * THE KERNELS (pvnet_amd/csrc/raster.hip): at most four launches per call, all on `stream`; no allocation, no synchronisation,
 * capturable in a graph.  The bit planes ([q,h,ceil(w/32)] uint32 in the workspace, one per instance) are cleared inside every call,
 * so a reused workspace leaks nothing.  One lane per (instance, triangle) walks its box alone while the box has at most
 * PVNET_RASTER_LANE_PIXELS pixels; every larger box takes the cooperative path, the 64 lanes of the wave across the pixels of a row.
 */
#ifndef PVNET_RASTER_H_
#define PVNET_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_RASTER_ABI_VERSION 1

/* the error codes of pvnet_vote.h */
#ifndef PVNET_E_BADARG
#define PVNET_E_BADARG      (-1)
#define PVNET_E_WORKSPACE   (-2)
#define PVNET_E_UNSUPPORTED (-3)
#endif

/* pixels of a triangle's box that a single lane walks by itself; a box with more takes the cooperative path */
#define PVNET_RASTER_LANE_PIXELS 64
/* instances per pvnet_render call (their table travels in the launch's arguments) and meshes per table */
#define PVNET_RASTER_MAX_INSTANCES 768
#define PVNET_RASTER_MAX_MESHES 64
/* images per call, the longer side of an image */
#define PVNET_RASTER_MAX_IMAGES 65535
#define PVNET_RASTER_MAX_SIDE 32768

/* status bits, per instance (pvnet_render) or per image (pvnet_raster_triangles) */
#define PVNET_RASTER_S_NONFINITE 1 /* a triangle with a non-finite coordinate was skipped */
#define PVNET_RASTER_S_BEHIND    2 /* a vertex of the instance's mesh lies at camera z <= 0 */
#define PVNET_RASTER_S_BADFACE   4 /* a face names a vertex outside its mesh and was skipped (the host validates faces; this guards) */

int pvnet_raster_abi_version(void);

/* Bytes of workspace for q instances (for pvnet_raster_triangles: q = n images) of h x w pixels.  P and T, the vertices and faces of
 * the mesh table, are part of the signature and checked, but the triangles are projected where they are rasterised and nothing is
 * stored per vertex or face.  0 for an argument out of range.  The workspace may hold anything on entry. */
size_t pvnet_raster_workspace_bytes(int q, int P, int T, int b, int h, int w);

/* Stage R for n images of tn triangles each.
 *   tri        [n,tn,3,2] float32, contiguous, device
 *   mask_out   [n,h,w] uint8, device; every byte is written (0 or 1)
 *   status_out NULL or [n] int32, device: PVNET_RASTER_S_NONFINITE or 0
 *   ws         pvnet_raster_workspace_bytes(n, 0, tn, n, h, w) bytes, 16-byte aligned, device
 * Three launches.  n == 0 returns 0 and enqueues nothing; tn == 0 writes zeros.
 * Returns 0, a positive hipError_t, PVNET_E_BADARG (a null pointer, n or tn < 0, h or w < 2, a misaligned workspace),
 * PVNET_E_WORKSPACE or PVNET_E_UNSUPPORTED (n > PVNET_RASTER_MAX_IMAGES, a side above PVNET_RASTER_MAX_SIDE). */
int pvnet_raster_triangles(const float* tri, int n, int tn, int h, int w, uint8_t* mask_out, int32_t* status_out,
                           void* ws, size_t ws_bytes, void* stream);

/* Stages P + R + C over a mesh table.  HOST arrays (read before the call returns): vertex_offset, face_offset, mesh_id, image_id,
 * label.  Everything else is device memory.
 *   vertices       [P,3] float64, the meshes' vertices one after the other
 *   faces          [T,3] int32, each index local to its mesh
 *   vertex_offset  [M+1] int32, host: mesh m owns vertices vertex_offset[m] .. vertex_offset[m+1]-1; [0] == 0, [M] == P
 *   face_offset    [M+1] int32, host, likewise with T
 *   q instances:   mesh_id [q] int32 host, poses [q,3,4] float64, K [3,3] float64 (k_per_instance == 0) or [q,3,3] (!= 0),
 *                  image_id [q] int32 host, non-decreasing, in 0 .. b-1;  label [q] int32 host, in 1 .. 255
 *   order          NULL or [q] int32, device: see stage C
 *   out            [b,h,w] uint8; every byte is written.  NULL: project only (tri_out is then required)
 *   tri_out        NULL or float32 [sum of the instances' faces,3,2]: the projected triangles, instance after instance
 *   status_out     NULL or [q] int32: PVNET_RASTER_S_* bits
 *   ws             pvnet_raster_workspace_bytes(q, P, T, b, h, w) bytes, 16-byte aligned
 * Four launches.  b == 0 returns 0 and enqueues nothing; q == 0 writes zeros.
 * Returns 0, a positive hipError_t, PVNET_E_BADARG (a null pointer, a negative size, h or w < 2, offsets that do not start at 0, decrease
 * or do not end at P / T, a mesh_id outside 0 .. M-1, a label outside 1 .. 255, an image_id outside 0 .. b-1 or below its
 * predecessor, a misaligned workspace), PVNET_E_WORKSPACE or PVNET_E_UNSUPPORTED (q > PVNET_RASTER_MAX_INSTANCES, M >
 * PVNET_RASTER_MAX_MESHES, b > PVNET_RASTER_MAX_IMAGES, a side above PVNET_RASTER_MAX_SIDE). */
int pvnet_render(const double* vertices, const int32_t* faces, const int32_t* vertex_offset, const int32_t* face_offset, int M,
                 int P, int T, int q, const int32_t* mesh_id, const double* poses, const double* K, int k_per_instance,
                 const int32_t* image_id, const int32_t* label, const int32_t* order, int b, int h, int w, uint8_t* out,
                 float* tri_out, int32_t* status_out, void* ws, size_t ws_bytes, void* stream);

/* Development aid: the triangles of the last call on this workspace that took the cooperative path, as the call left it in the
 * workspace's first word (a device address; copy it out after synchronising). */
#define PVNET_RASTER_WS_COOP_COUNT_OFFSET 0

#ifdef __cplusplus
}
#endif
#endif /* PVNET_RASTER_H_ */
