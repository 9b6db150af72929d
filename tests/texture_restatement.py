"""numpy restatement of include/pvnet_texture.h: the colour of a covered pixel of a textured mesh exactly as THE DEFINITION there states
it, float64 with one rounding per operation, no ``matmul`` anywhere.  Which face wins a pixel, the clamps and the dot product are
tests/shade_restatement.py's; an untextured mesh is shaded by that file's ``shade_pixels`` itself.  What this file adds is the texel:
(u, v) by the attribute interpolation, the clamp to the edge, the nearest or bilinear fetch with the row flip folded in.

``affine=True`` interpolates (u, v) with the screen barycentrics l_k instead of l_k / z_k.  It is NOT the definition: it exists so that
a test can show its fixture tells the two apart."""
import numpy as np

from tests import depth_restatement as DR
from tests import raster_restatement as RS
from tests import shade_restatement as SR

NONE, FLAT, PHONG = SR.NONE, SR.FLAT, SR.PHONG
SHADING = SR.SHADING
NEAREST, BILINEAR = 0, 1
FILTER = {"nearest": NEAREST, "bilinear": BILINEAR}
f32 = np.float32


def sample(texture, u, v, filter):   # noqa: A002
    """c[ch] of the header for interpolated (u, v) (float64 [N]) -> [3] arrays of float64 [N]; ``texture`` uint8 [th,tw,>=3] as
    loaded, the top row first"""
    tex = np.asarray(texture)
    assert tex.dtype == np.uint8 and tex.ndim == 3 and tex.shape[2] >= 3
    th, tw = tex.shape[:2]
    t = tex[..., :3].astype(np.float64)
    one, half = np.float64(1.0), np.float64(0.5)
    with np.errstate(all="ignore"):
        u, v = SR._clamp01(u), SR._clamp01(v)
        if filter == NEAREST:
            i = np.minimum(np.floor(u * np.float64(tw)).astype(np.int64), tw - 1)
            j = np.minimum(np.floor(v * np.float64(th)).astype(np.int64), th - 1)
            row = th - 1 - j
            return [t[row, i, ch] for ch in range(3)]
        x = u * np.float64(tw) - half
        i0 = np.floor(x)
        fx = x - i0
        ia, ib = np.maximum(i0.astype(np.int64), 0), np.minimum(i0.astype(np.int64) + 1, tw - 1)
        y = v * np.float64(th) - half
        j0 = np.floor(y)
        fy = y - j0
        ja, jb = np.maximum(j0.astype(np.int64), 0), np.minimum(j0.astype(np.int64) + 1, th - 1)
        ra, rb = th - 1 - ja, th - 1 - jb
        out = []
        for ch in range(3):
            lo = (one - fx) * t[ra, ia, ch] + fx * t[ra, ib, ch]
            hi = (one - fx) * t[rb, ia, ch] + fx * t[rb, ib, ch]
            out.append((one - fy) * lo + fy * hi)
        return out


def shade_pixels(vertices, faces, colors, normals, uv, texture, pose, K, face, px, py, shading, ambient, filter=NEAREST,  # noqa: A002
                 affine=False, rounded=True):
    """the colour of the pixels (px, py) (integer arrays [N]) under the faces ``face`` [N] of one posed mesh -> uint8 [N,3] (float64,
    before ``floor(. + 0.5)`` and the clamp, with ``rounded=False``); every line one float64 operation per element, in the header's order.
    ``texture`` None: tests/shade_restatement.py's function."""
    if texture is None:
        assert rounded and not affine
        return SR.shade_pixels(vertices, faces, colors, normals, pose, K, face, px, py, shading, ambient)
    X = np.asarray(vertices, np.float64)
    R = np.asarray(pose, np.float64)
    faces = np.asarray(faces, np.int64)
    one, half = np.float64(1.0), np.float64(0.5)
    with np.errstate(all="ignore"):
        su, sv, _ = RS.project_points(X, R, K)
        cam = [((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + R[r, 3] for r in range(3)]
        idx = [faces[face, k] for k in range(3)]
        C = [[cam[r][idx[k]] for r in range(3)] for k in range(3)]
        x0, x1, x2 = (su[idx[k]].astype(np.float64) for k in range(3))
        y0, y1, y2 = (sv[idx[k]].astype(np.float64) for k in range(3))
        px, py = np.asarray(px).astype(np.float64), np.asarray(py).astype(np.float64)
        dx1, dy1, dx2, dy2, ex, ey = x1 - x0, y1 - y0, x2 - x0, y2 - y0, px - x0, py - y0
        area = dx1 * dy2 - dx2 * dy1
        l1 = (ex * dy2 - dx2 * ey) / area
        l2 = (dx1 * ey - ex * dy1) / area
        l0 = (one - l1) - l2
        l0, l1, l2 = SR._clamp01(l0), SR._clamp01(l1), SR._clamp01(l2)
        w0, w1, w2 = l0 / C[0][2], l1 / C[1][2], l2 / C[2][2]
        s = (w0 + w1) + w2
        degenerate = (area == 0) | ~(s > 0)

        def attribute(a0, a1, a2):
            return np.where(degenerate, a0, ((w0 * a0 + w1 * a1) + w2 * a2) / s)

        e = [attribute(C[0][r], C[1][r], C[2][r]) for r in range(3)]
        uv64 = np.asarray(uv).astype(np.float32).astype(np.float64)   # the library reads float32
        if affine:   # NOT the definition: the screen barycentrics as weights
            ls = (l0 + l1) + l2
            u, v = (((l0 * uv64[idx[0], c] + l1 * uv64[idx[1], c]) + l2 * uv64[idx[2], c]) / ls for c in range(2))
        else:
            u, v = (attribute(uv64[idx[0], c], uv64[idx[1], c], uv64[idx[2], c]) for c in range(2))
        col = sample(texture, u, v, filter)
        if shading == NONE:
            light = np.ones_like(s)
        else:
            le = np.sqrt(SR._dot(e, e))
            if shading == FLAT:
                a = [C[1][r] - C[0][r] for r in range(3)]
                b = [C[2][r] - C[0][r] for r in range(3)]
                g = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
                lg = np.sqrt(SR._dot(g, g))
                diffuse = np.abs(SR._dot(e, g)) / (le * lg)
                diffuse = np.where((le == 0) | (lg == 0), 0.0, diffuse)
            else:
                N = np.asarray(normals, np.float64)
                m = [[(R[r, 0] * N[idx[k], 0] + R[r, 1] * N[idx[k], 1]) + R[r, 2] * N[idx[k], 2] for r in range(3)] for k in range(3)]
                n = [attribute(m[0][r], m[1][r], m[2][r]) for r in range(3)]
                ln = np.sqrt(SR._dot(n, n))
                diffuse = (-SR._dot(e, n)) / (le * ln)
                diffuse = np.where(diffuse > 0, diffuse, 0.0)
                diffuse = np.where((le == 0) | (ln == 0), 0.0, diffuse)
            light = np.float64(f32(ambient)) + diffuse
            light = np.where(light < 1, light, 1.0)
        if not rounded:
            return np.stack([light * col[ch] for ch in range(3)], 1), np.stack([u, v], 1)
        out = np.zeros((len(px), 3), np.uint8)
        for ch in range(3):
            val = np.floor(light * col[ch] + half)
            val = np.where(val >= 0, val, 0.0)
            val = np.where(val > 255, 255.0, val)
            out[:, ch] = val.astype(np.uint8)
    return out


def render(meshes, instances, b, h, w, far=np.inf, shading="flat", ambient=0.5, background=(0, 0, 0), filter="nearest",  # noqa: A002
           layers=None, affine=False):
    """meshes: [(vertices, faces, colors, normals or None, uv or None, texture or None)]; everything else as
    tests/shade_restatement.py's ``render`` -> (rgb [b,h,w,3] uint8, depth [b,h,w] float32, labels [b,h,w] uint8, visible [q] int32,
    status [q] int32)"""
    shading = SHADING[shading] if isinstance(shading, str) else int(shading)
    filter = FILTER[filter] if isinstance(filter, str) else int(filter)   # noqa: A001
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
            got = SR.instance_layers(meshes[m][0], meshes[m][1], pose, K, h, w)
            if layers is not None:
                layers[key] = got
        d, who, status[i] = got if layers is None else layers[key]
        depths.append(d)
        owners.append(who)
    images, labels = [ins[3] for ins in instances], [ins[4] for ins in instances]
    depth, label, visible = DR.compose(depths, images, labels, b, far)
    best = np.full((b, h, w), np.inf, np.float32)
    winner = np.full((b, h, w), -1, np.int64)
    for i in range(q):   # compose's own rule: kept when 0 != depth < far, the smallest, the earlier instance at a tie
        d = depths[i]
        take = (d != 0) & (d < f32(far)) & (d < best[images[i]])
        best[images[i]][take] = d[take]
        winner[images[i]][take] = i
    for i, (m, pose, K, img, _) in enumerate(instances):
        ys, xs = np.nonzero(winner[img] == i)
        assert len(ys) == visible[i]
        if len(ys):
            v, f, colors, normals, uv, texture = meshes[m]
            assert shading != PHONG or normals is not None, "Phong shading needs the vertex normals"
            tex_kw = dict(filter=filter, affine=affine) if texture is not None else {}
            rgb[img, ys, xs] = shade_pixels(v, f, colors, normals, uv, texture, pose, K, owners[i][ys, xs], xs, ys, shading, ambient,
                                            **tex_kw)
    return rgb, depth, label, visible, status
