"""numpy restatement of include/pvnet_depth.h: coverage (stages P and R of include/pvnet_raster.h, through tests/raster_restatement.py),
the depth of a covered pixel under one triangle, and the composition, exactly as THE DEFINITION there states them.  float64 arithmetic
with one rounding per operation (numpy's elementwise operations), one rounding to float32 at the end, no ``matmul`` anywhere."""
import numpy as np

from tests import raster_restatement as RS

S_NONFINITE, S_BEHIND, S_BADFACE = 1, 2, 4
f32 = np.float32


def triangle_box(t, h, w):
    """stage R's inclusive pixel box of one float32 triangle [3,2] -> (begx, endx, begy, endy) or None when it is empty"""
    (x0, y0), (x1, y1), (x2, y2) = t
    minx, maxx = max(f32(0), min(x0, x1, x2)), min(f32(w - 2), max(x0, x1, x2))
    miny, maxy = max(f32(0), min(y0, y1, y2)), min(f32(h - 2), max(y0, y1, y2))
    ex, ey = f32(maxx + f32(1)), f32(maxy + f32(1))
    if minx >= f32(w) or ex <= f32(-1) or miny >= f32(h) or ey <= f32(-1):
        return None
    begx, endx, begy, endy = int(minx), int(ex), int(miny), int(ey)   # truncation, both ends inclusive
    if begx > endx or begy > endy:
        return None
    return begx, endx, begy, endy


def triangle_coverage(t, px, py):
    """stage R's predicate for the float32 pixel coordinates px, py (arrays) -> bool array"""
    (x0, y0), (x1, y1), (x2, y2) = t
    return RS._same_side(x0, y0, x1, y1, x2, y2, px, py, False) & RS._same_side(x1, y1, x2, y2, x0, y0, px, py, False) & \
        RS._same_side(x2, y2, x0, y0, x1, y1, px, py, False)


def triangle_depth(t, z, px, py):
    """the depth of the pixels (px, py) (float32 arrays, integer values) under the triangle t [3,2] float32 with camera z [3] float64
    -> float32 array; every line one float64 operation per element, in the header's order"""
    x0, y0, x1, y1, x2, y2 = (np.float64(v) for v in (t[0][0], t[0][1], t[1][0], t[1][1], t[2][0], t[2][1]))
    z0, z1, z2 = (np.float64(v) for v in z)
    one = np.float64(1.0)
    i0, i1, i2 = one / z0, one / z1, one / z2
    zmin, zmax = min(z0, z1, z2), max(z0, z1, z2)
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    b = ((i1 - i0) * (y2 - y0) - (i2 - i0) * (y1 - y0)) / area
    c = ((i2 - i0) * (x1 - x0) - (i1 - i0) * (x2 - x0)) / area
    inv = (i0 + b * (px.astype(np.float64) - x0)) + c * (py.astype(np.float64) - y0)
    d = one / inv
    if area == 0:
        d = np.full_like(d, zmin)
    d = np.where(d >= zmin, d, zmin)   # !(d >= zmin): NaN and negative values too
    d = np.where(d > zmax, zmax, d)
    return d.astype(np.float32)


def instance_depth(vertices, faces, pose, K, h, w):
    """one instance alone, far = +inf -> (depth [h,w] float32 with 0 where nothing covers, status)"""
    depth = np.full((h, w), np.inf, np.float32)
    status = 0
    with np.errstate(all="ignore"):
        u, v, z = RS.project_points(vertices, pose, K)
        for face in np.asarray(faces, np.int64):
            t = np.stack([u[face], v[face]], -1).astype(np.float32)
            zt = z[face]
            skip = False
            if not np.isfinite(zt).all() or (zt.astype(np.float32) <= 0).any():
                status |= S_BEHIND
                skip = True
            if not np.isfinite(t).all():
                status |= S_NONFINITE
                skip = True
            if skip:
                continue
            box = triangle_box(t, h, w)
            if box is None:
                continue
            begx, endx, begy, endy = box
            ys, xs = np.mgrid[begy:endy + 1, begx:endx + 1]
            px, py = xs.astype(np.float32), ys.astype(np.float32)
            ok = triangle_coverage(t, px, py)
            d = np.where(ok, triangle_depth(t, zt, px, py), f32(np.inf))
            view = depth[begy:endy + 1, begx:endx + 1]
            np.minimum(view, d, out=view)
            # (a covered pixel whose depth is +inf -- camera z beyond float32 -- stays uncovered: it is below no `far`)
    return np.where(np.isinf(depth), f32(0), depth).astype(np.float32), status


def compose(depths, image_ids, labels, b, far=np.inf):
    """the composition: depths [q,h,w] float32 (0: not covered), per instance its image and label -> (depth [b,h,w] float32, labels
    [b,h,w] uint8, visible [q] int32).  A candidate is kept when 0 != depth < far; the smallest wins, the earlier instance at a tie."""
    q = len(depths)
    h, w = depths[0].shape if q else (0, 0)
    far = f32(far)
    assert far > 0
    best = np.full((b, h, w), np.inf, np.float32)
    owner = np.full((b, h, w), -1, np.int64)
    for i in range(q):
        d = depths[i]
        img = image_ids[i]
        take = (d != 0) & (d < far) & (d < best[img])   # strict: the earlier instance keeps a tie
        best[img][take] = d[take]
        owner[img][take] = i
    out_depth = np.where(owner >= 0, best, f32(0)).astype(np.float32)
    out_label = np.zeros((b, h, w), np.uint8)
    visible = np.zeros(q, np.int32)
    for i in range(q):
        won = owner[image_ids[i]] == i
        out_label[image_ids[i]][won] = labels[i]
        visible[i] = int(won.sum())
    return out_depth, out_label, visible


def render(meshes, instances, b, h, w, far=np.inf):
    """meshes: [(vertices, faces)]; instances: [(mesh_id, pose [3,4], K [3,3], image, label)] with non-decreasing image
    -> (depth [b,h,w] float32, labels [b,h,w] uint8, visible [q] int32, status [q] int32)"""
    depths, status = [], np.zeros(len(instances), np.int32)
    for i, (m, pose, K, _, _) in enumerate(instances):
        d, status[i] = instance_depth(meshes[m][0], meshes[m][1], pose, K, h, w)
        depths.append(d)
    if not instances:
        return np.zeros((b, h, w), np.float32), np.zeros((b, h, w), np.uint8), np.zeros(0, np.int32), status
    depth, label, visible = compose(depths, [ins[3] for ins in instances], [ins[4] for ins in instances], b, far)
    return depth, label, visible, status


def checksum(arrays):
    """sha256 over the bytes of the arrays (C order), for fixtures that regenerate an input instead of storing it"""
    import hashlib
    hsh = hashlib.sha256()
    for a in arrays:
        hsh.update(np.ascontiguousarray(a).tobytes())
    return hsh.hexdigest()
