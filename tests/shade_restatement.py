"""numpy restatement of include/pvnet_shade.h: the colour of a covered pixel exactly as THE DEFINITION there states it, float64 with one
rounding per operation (numpy's elementwise operations; ``sqrt`` and ``/`` are correctly rounded), no ``matmul`` anywhere.  Coverage and
the depth under one triangle are tests/depth_restatement.py's functions, the composition's depth, labels and visible counts its
``compose``; what this file adds to them is which FACE wins a pixel (the lower face index at equal depth) and its colour."""
import numpy as np

from tests import depth_restatement as DR
from tests import raster_restatement as RS

S_NONFINITE, S_BEHIND, S_BADFACE = DR.S_NONFINITE, DR.S_BEHIND, DR.S_BADFACE
NONE, FLAT, PHONG = 0, 1, 2
SHADING = {"none": NONE, "flat": FLAT, "phong": PHONG}
f32 = np.float32


def instance_layers(vertices, faces, pose, K, h, w):
    """one instance alone, far = +inf -> (depth [h,w] float32 with 0 where nothing covers, face [h,w] int64 with -1 there, status):
    tests/depth_restatement.py's instance_depth, which also remembers the face -- the lower index at equal depth"""
    depth = np.full((h, w), np.inf, np.float32)
    owner = np.full((h, w), -1, np.int64)
    status = 0
    with np.errstate(all="ignore"):
        u, v, z = RS.project_points(vertices, pose, K)
        for fi, face in enumerate(np.asarray(faces, np.int64)):
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
            box = DR.triangle_box(t, h, w)
            if box is None:
                continue
            begx, endx, begy, endy = box
            ys, xs = np.mgrid[begy:endy + 1, begx:endx + 1]
            px, py = xs.astype(np.float32), ys.astype(np.float32)
            ok = DR.triangle_coverage(t, px, py)
            d = np.where(ok, DR.triangle_depth(t, zt, px, py), f32(np.inf))
            view, who = depth[begy:endy + 1, begx:endx + 1], owner[begy:endy + 1, begx:endx + 1]
            take = d < view   # strict: the lower face index keeps a tie; +inf is below no `far` and stays uncovered
            view[take] = d[take]
            who[take] = fi
    return np.where(np.isinf(depth), f32(0), depth).astype(np.float32), owner, status


def _clamp01(l):
    l = np.where(l >= 0, l, 0.0)   # !(l >= 0): NaN too
    return np.where(l > 1, 1.0, l)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def shade_pixels(vertices, faces, colors, normals, pose, K, face, px, py, shading, ambient):
    """the colour of the pixels (px, py) (integer arrays [N]) under the faces ``face`` [N] of one posed mesh -> uint8 [N,3]; every line
    one float64 operation per element, in the header's order"""
    X = np.asarray(vertices, np.float64)
    R = np.asarray(pose, np.float64)
    faces = np.asarray(faces, np.int64)
    one, half = np.float64(1.0), np.float64(0.5)
    with np.errstate(all="ignore"):
        u, v, _ = RS.project_points(X, R, K)
        cam = [((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + R[r, 3] for r in range(3)]   # stage P's c_0, c_1, c_2
        idx = [faces[face, k] for k in range(3)]
        C = [[cam[r][idx[k]] for r in range(3)] for k in range(3)]                     # C[k][r]
        x0, x1, x2 = (u[idx[k]].astype(np.float64) for k in range(3))
        y0, y1, y2 = (v[idx[k]].astype(np.float64) for k in range(3))
        px, py = np.asarray(px).astype(np.float64), np.asarray(py).astype(np.float64)
        dx1, dy1, dx2, dy2, ex, ey = x1 - x0, y1 - y0, x2 - x0, y2 - y0, px - x0, py - y0
        area = dx1 * dy2 - dx2 * dy1
        l1 = (ex * dy2 - dx2 * ey) / area
        l2 = (dx1 * ey - ex * dy1) / area
        l0 = (one - l1) - l2
        l0, l1, l2 = _clamp01(l0), _clamp01(l1), _clamp01(l2)
        w0, w1, w2 = l0 / C[0][2], l1 / C[1][2], l2 / C[2][2]
        s = (w0 + w1) + w2
        degenerate = (area == 0) | ~(s > 0)

        def attribute(a0, a1, a2):
            return np.where(degenerate, a0, ((w0 * a0 + w1 * a1) + w2 * a2) / s)

        e = [attribute(C[0][r], C[1][r], C[2][r]) for r in range(3)]
        col8 = np.asarray(colors, np.uint8)
        col = [attribute(*(col8[idx[k], ch].astype(np.float64) for k in range(3))) for ch in range(3)]
        if shading == NONE:
            light = np.ones_like(s)
        else:
            le = np.sqrt(_dot(e, e))
            if shading == FLAT:
                a = [C[1][r] - C[0][r] for r in range(3)]
                b = [C[2][r] - C[0][r] for r in range(3)]
                g = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
                lg = np.sqrt(_dot(g, g))
                diffuse = np.abs(_dot(e, g)) / (le * lg)
                diffuse = np.where((le == 0) | (lg == 0), 0.0, diffuse)
            else:
                N = np.asarray(normals, np.float64)
                m = [[(R[r, 0] * N[idx[k], 0] + R[r, 1] * N[idx[k], 1]) + R[r, 2] * N[idx[k], 2] for r in range(3)] for k in range(3)]
                n = [attribute(m[0][r], m[1][r], m[2][r]) for r in range(3)]
                ln = np.sqrt(_dot(n, n))
                diffuse = (-_dot(e, n)) / (le * ln)
                diffuse = np.where(diffuse > 0, diffuse, 0.0)
                diffuse = np.where((le == 0) | (ln == 0), 0.0, diffuse)
            light = np.float64(f32(ambient)) + diffuse
            light = np.where(light < 1, light, 1.0)
        out = np.zeros((len(px), 3), np.uint8)
        for ch in range(3):
            val = np.floor(light * col[ch] + half)
            val = np.where(val >= 0, val, 0.0)
            val = np.where(val > 255, 255.0, val)
            out[:, ch] = val.astype(np.uint8)
    return out


def render(meshes, instances, b, h, w, far=np.inf, shading="flat", ambient=0.5, background=(0, 0, 0), layers=None):
    """meshes: [(vertices, faces, colors, normals or None)]; instances: [(mesh_id, pose [3,4], K [3,3], image, label)] with
    non-decreasing image; background: a colour triple or uint8 [b,h,w,3]; layers: None or a dict the caller keeps between calls, in
    which the instances' depth and face images are remembered (they do not depend on far, shading, ambient or background)
    -> (rgb [b,h,w,3] uint8, depth [b,h,w] float32, labels [b,h,w] uint8, visible [q] int32, status [q] int32)"""
    shading = SHADING[shading] if isinstance(shading, str) else int(shading)
    bg = np.asarray(background, np.uint8)
    rgb = np.ascontiguousarray(np.broadcast_to(bg, (b, h, w, 3))).copy()
    q = len(instances)
    status = np.zeros(q, np.int32)
    if not q:
        return rgb, np.zeros((b, h, w), np.float32), np.zeros((b, h, w), np.uint8), np.zeros(0, np.int32), status
    depths, owners = [], []
    for i, (m, pose, K, _, _) in enumerate(instances):
        key = (m, np.asarray(pose, np.float64).tobytes(), np.asarray(K, np.float64).tobytes(), h, w)
        if layers is None or key not in layers:
            got = instance_layers(meshes[m][0], meshes[m][1], pose, K, h, w)
            if layers is not None:
                layers[key] = got
        d, who, status[i] = got if layers is None else layers[key]
        depths.append(d)
        owners.append(who)
    images, labels = [ins[3] for ins in instances], [ins[4] for ins in instances]
    depth, label, visible = DR.compose(depths, images, labels, b, far)
    # which instance wins a pixel: compose's own rule (kept when 0 != depth < far, the smallest, the earlier instance at a tie)
    best = np.full((b, h, w), np.inf, np.float32)
    winner = np.full((b, h, w), -1, np.int64)
    for i in range(q):
        d = depths[i]
        take = (d != 0) & (d < f32(far)) & (d < best[images[i]])
        best[images[i]][take] = d[take]
        winner[images[i]][take] = i
    for i, (m, pose, K, img, _) in enumerate(instances):
        ys, xs = np.nonzero(winner[img] == i)
        assert len(ys) == visible[i]
        if len(ys):
            v, f, colors = meshes[m][:3]
            normals = meshes[m][3] if len(meshes[m]) > 3 else None
            assert shading != PHONG or normals is not None, "Phong shading needs the vertex normals"
            rgb[img, ys, xs] = shade_pixels(v, f, colors, normals, pose, K, owners[i][ys, xs], xs, ys, shading, ambient)
    return rgb, depth, label, visible, status
