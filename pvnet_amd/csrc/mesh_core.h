// mesh_core.h -- the ONE copy of stage P (pose -> float32 screen vertex) and of stage R's coverage predicate (include/pvnet_raster.h,
// THE DEFINITION).  raster.hip (libpvnet_raster.so) includes it itself; depth.hip, shade.hip and texture.hip compile it with the
// z-buffer of zbuffer_core.h: a colour or textured image is covered exactly where the silhouette is set and the depth image non-zero
// because all four libraries evaluate these functions.  Below them the host side all four share: the instance table a setup kernel takes
// and the checks of the arguments every pvnet_render* entry point opens with (the PVNET_E_* codes: the public header, included first).
//
// Nothing here may be contracted into a fused multiply-add (tests/test_raster_cpu.py looks for fused float32 instructions in the
// assembly); float32 denormals are kept (the compiler's default for gfx950).
#ifndef PVNET_MESH_CORE_H_
#define PVNET_MESH_CORE_H_

#include <algorithm>

#include <hip/hip_runtime.h>

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

// stage P for one vertex
__device__ __forceinline__ void project(const double* pose, const double* K, const double* X, float& u, float& v) {
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const double c0 = ((pose[0] * X0 + pose[1] * X1) + pose[2] * X2) + pose[3];
    const double c1 = ((pose[4] * X0 + pose[5] * X1) + pose[6] * X2) + pose[7];
    const double c2 = ((pose[8] * X0 + pose[9] * X1) + pose[10] * X2) + pose[11];
    const double p0 = (K[0] * c0 + K[1] * c1) + K[2] * c2;
    const double p1 = (K[3] * c0 + K[4] * c1) + K[5] * c2;
    const double p2 = (K[6] * c0 + K[7] * c1) + K[8] * c2;
    u = (float)(p0 / p2);
    v = (float)(p1 / p2);
}

// one edge of same_side: what does not depend on the pixel
struct Edge {
    float xa, ya, nx, ny, val0;
};

__device__ __forceinline__ Edge make_edge(float xa, float ya, float xb, float yb, float tx, float ty) {
    Edge e;
    const float dx = xb - xa, dy = yb - ya;
    e.xa = xa;
    e.ya = ya;
    e.nx = -dy;
    e.ny = dx;
    const float dx0 = tx - xa, dy0 = ty - ya;
    const float a = dx0 * e.nx, b = dy0 * e.ny;
    e.val0 = a + b;
    return e;
}

__device__ __forceinline__ bool same_side(const Edge& e, float px, float py) {
    const float dx1 = px - e.xa, dy1 = py - e.ya;
    const float a = dx1 * e.nx, b = dy1 * e.ny;
    const float val1 = a + b;
    const float prod = e.val0 * val1;
    return prod >= 0.f;
}

__device__ __forceinline__ bool inside(const Edge& e0, const Edge& e1, const Edge& e2, float px, float py) {
    return same_side(e0, px, py) && same_side(e1, px, py) && same_side(e2, px, py);
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------

// the limits: equal in the four public headers under their own prefixes
constexpr int MAX_INSTANCES = 768, MAX_MESHES = 64, MAX_IMAGES = 65535, MAX_IMAGE_SIDE = 32768;

// the instance table as it travels in a setup kernel's arguments: mesh (6 bits) | label (8) << 6 | image (18) << 14
struct Table {
    uint32_t inst[MAX_INSTANCES];
    int32_t voff[MAX_MESHES + 1], foff[MAX_MESHES + 1];
};
static_assert(sizeof(Table) <= 3800, "kernel arguments: 4 KB with the rest");
static_assert(MAX_MESHES <= 64 && MAX_IMAGES < (1 << 18), "the packing of Table::inst");

struct Instances {   // the arguments the four entry points share
    const double* vertices;
    const int32_t *faces, *vertex_offset, *face_offset;
    int M, P, T, q;
    const int32_t* mesh_id;
    const double *poses, *K;
    int k_per_instance;
    const int32_t *image_id, *label;
    int b, h, w;
};

// The validation, in the order the entry points have always returned their codes in, cut where one has checks of its own in between:
// the counts, [far], the sizes, the limits and the mesh table, [pvnet_render's outputs], the arrays, [a library's own], the instances.
int check_counts(const Instances& S) { return S.M < 1 || S.P < 0 || S.T < 0 || S.q < 0 || S.b < 0 ? PVNET_E_BADARG : 0; }

int check_sizes(int h, int w) {
    if (h < 2 || w < 2) return PVNET_E_BADARG;
    return h > MAX_IMAGE_SIDE || w > MAX_IMAGE_SIDE ? PVNET_E_UNSUPPORTED : 0;
}

int check_tables(const Instances& S) {
    if (int rc = check_sizes(S.h, S.w)) return rc;
    if (S.M > MAX_MESHES || S.q > MAX_INSTANCES || S.b > MAX_IMAGES) return PVNET_E_UNSUPPORTED;
    if (!S.vertex_offset || !S.face_offset) return PVNET_E_BADARG;
    if (S.vertex_offset[0] != 0 || S.face_offset[0] != 0 || S.vertex_offset[S.M] != S.P || S.face_offset[S.M] != S.T) return PVNET_E_BADARG;
    for (int m = 0; m < S.M; ++m)
        if (S.vertex_offset[m + 1] < S.vertex_offset[m] || S.face_offset[m + 1] < S.face_offset[m]) return PVNET_E_BADARG;
    return 0;
}

int check_arrays(const Instances& S) {
    if (S.q > 0 && (!S.mesh_id || !S.image_id || !S.label || !S.poses || !S.K)) return PVNET_E_BADARG;
    if ((S.P > 0 && !S.vertices) || (S.T > 0 && !S.faces)) return PVNET_E_BADARG;
    return 0;
}

// the instances, packed into the table as they are checked; *max_f, *max_v: the most faces and vertices a mesh of an instance has
int check_instances(const Instances& S, Table* tab, int* max_f, int* max_v = nullptr) {
    int faces = 0, vertices = 0;
    for (int i = 0; i < S.q; ++i) {
        if (S.mesh_id[i] < 0 || S.mesh_id[i] >= S.M) return PVNET_E_BADARG;
        if (S.label[i] < 1 || S.label[i] > 255) return PVNET_E_BADARG;
        if (S.image_id[i] < 0 || S.image_id[i] >= S.b || (i > 0 && S.image_id[i] < S.image_id[i - 1])) return PVNET_E_BADARG;
        faces = std::max(faces, S.face_offset[S.mesh_id[i] + 1] - S.face_offset[S.mesh_id[i]]);
        vertices = std::max(vertices, S.vertex_offset[S.mesh_id[i] + 1] - S.vertex_offset[S.mesh_id[i]]);
        tab->inst[i] = (uint32_t)S.mesh_id[i] | ((uint32_t)S.label[i] << 6) | ((uint32_t)S.image_id[i] << 14);
    }
    for (int i = S.q; i < MAX_INSTANCES; ++i) tab->inst[i] = 0u;
    for (int m = 0; m <= MAX_MESHES; ++m) {
        tab->voff[m] = S.vertex_offset[std::min(m, S.M)];
        tab->foff[m] = S.face_offset[std::min(m, S.M)];
    }
    *max_f = faces;
    if (max_v) *max_v = vertices;
    return 0;
}

}  // namespace
}  // namespace pvd
#endif  // PVNET_MESH_CORE_H_
