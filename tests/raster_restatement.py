"""numpy restatement of include/pvnet_raster.h: stage P (pose -> float32 triangles), stage R (triangles -> mask) and stage C (painter's
composition), exactly as THE DEFINITION there states them.  float32 arithmetic with one rounding per operation (numpy's elementwise
operations on float32 arrays), float64 for the projection, no ``matmul`` anywhere.  ``contracted=True`` evaluates ``a*b + c*d`` of the
predicate as one fused multiply-add would (the first product exact): NOT the definition, only there to show that the fixtures tell the
two apart."""
import numpy as np

S_NONFINITE, S_BEHIND, S_BADFACE = 1, 2, 4
f32 = np.float32


def project_points(vertices, pose, K):
    """[P,3] float64 -> (u, v) float32 [P], camera z float64 [P]; every operation rounded once, in the header's order"""
    X = np.asarray(vertices, np.float64)
    R = np.asarray(pose, np.float64)
    K = np.asarray(K, np.float64)
    with np.errstate(all="ignore"):
        c = [((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + R[r, 3] for r in range(3)]
        p = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
        u = (p[0] / p[2]).astype(np.float32)
        v = (p[1] / p[2]).astype(np.float32)
    return u, v, c[2]


def project_triangles(vertices, faces, pose, K):
    """-> (tri [T,3,2] float32, status)"""
    u, v, z = project_points(vertices, pose, K)
    faces = np.asarray(faces, np.int64)
    tri = np.stack([u[faces], v[faces]], -1).astype(np.float32).reshape(len(faces), 3, 2)
    return tri, (S_BEHIND if bool((z <= 0).any()) else 0)


def _dot2(a, b, c, d, contracted):
    """a*b + c*d in float32: two products and a sum, three roundings; contracted: fma(a, b, fl(c*d))"""
    if not contracted:
        return a * b + c * d
    cd = (c * d).astype(np.float64)
    return (a.astype(np.float64) * b.astype(np.float64) + cd).astype(np.float32)


def _same_side(xa, ya, xb, yb, tx, ty, px, py, contracted):
    dx, dy = f32(xb - xa), f32(yb - ya)
    nx, ny = f32(-dy), dx
    one = np.ones(1, np.float32)
    val0 = _dot2(f32(tx - xa) * one, nx * one, f32(ty - ya) * one, ny * one, contracted)
    val1 = _dot2(px - xa, nx * np.ones_like(px), py - ya, ny * np.ones_like(py), contracted)
    return val0 * val1 >= 0


def rasterize(tri, h, w, contracted=False):
    """tri [tn,3,2] float32 -> (mask [h,w] uint8, status)"""
    assert h >= 2 and w >= 2
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 2)
    mask = np.zeros((h, w), np.uint8)
    status = 0
    with np.errstate(all="ignore"):
        for t in tri:
            if not np.isfinite(t).all():
                status |= S_NONFINITE
                continue
            (x0, y0), (x1, y1), (x2, y2) = t
            minx, maxx = max(f32(0), min(x0, x1, x2)), min(f32(w - 2), max(x0, x1, x2))
            miny, maxy = max(f32(0), min(y0, y1, y2)), min(f32(h - 2), max(y0, y1, y2))
            ex, ey = f32(maxx + f32(1)), f32(maxy + f32(1))
            if minx >= f32(w) or ex <= f32(-1) or miny >= f32(h) or ey <= f32(-1):
                continue
            begx, endx, begy, endy = int(minx), int(ex), int(miny), int(ey)   # truncation, both ends inclusive
            if begx > endx or begy > endy:
                continue
            ys, xs = np.mgrid[begy:endy + 1, begx:endx + 1]
            px, py = xs.astype(np.float32), ys.astype(np.float32)
            ok = _same_side(x0, y0, x1, y1, x2, y2, px, py, contracted) & _same_side(x1, y1, x2, y2, x0, y0, px, py, contracted) & \
                _same_side(x2, y2, x0, y0, x1, y1, px, py, contracted)
            mask[begy:endy + 1, begx:endx + 1] |= ok.astype(np.uint8)
    return mask, status


def painter_order(image_ids, order=None):
    """the instances' indices in the order they are painted: by image, then ascending order[i], ties in list order"""
    idx = np.arange(len(image_ids))
    key = np.zeros(len(image_ids), np.int64) if order is None else np.asarray(order, np.int64)
    return sorted(idx, key=lambda i: (image_ids[i], key[i], i))


def render(meshes, instances, b, h, w, order=None):
    """meshes: [(vertices, faces)]; instances: [(mesh_id, pose [3,4], K [3,3], image, label)] with non-decreasing image
    -> (out [b,h,w] uint8, status [q] int32, triangles per instance)"""
    out = np.zeros((b, h, w), np.uint8)
    status = np.zeros(len(instances), np.int32)
    masks, tris = [], []
    for i, (m, pose, K, _, _) in enumerate(instances):
        tri, st = project_triangles(meshes[m][0], meshes[m][1], pose, K)
        mask, st2 = rasterize(tri, h, w)
        status[i] = st | st2
        masks.append(mask)
        tris.append(tri)
    for i in painter_order([ins[3] for ins in instances], order):
        out[instances[i][3]][masks[i] != 0] = instances[i][4]
    return out, status, tris


def centroid_order(meshes, mesh_ids, poses):
    """far to near by the camera-space z of each mesh's centroid: poses [m,3,4] -> order[i] = position of instance i (stable)"""
    z = []
    for m, pose in zip(mesh_ids, poses):
        c = np.asarray(meshes[m][0], np.float64).mean(0)
        z.append(((pose[2, 0] * c[0] + pose[2, 1] * c[1]) + pose[2, 2] * c[2]) + pose[2, 3])
    perm = np.argsort(-np.asarray(z), kind="stable")
    rank = np.empty(len(perm), np.int64)
    rank[perm] = np.arange(len(perm))
    return rank
