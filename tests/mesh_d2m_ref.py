"""The mesh data-to-model distance (include/spherehand_hip.h, the section of shr_mesh_d2m_fwd) restated in numpy (test
helper; not a conftest), operation by operation:

    points32     the data points of an observation and their pixels
    tri_dist2_32 the contract's fp32 sequence for every (point, face): numpy's float32 operators round once each
    forward32    dist and face by the serial rule -- NO cull: every face is measured for every point
    closest64    the seven regions in fp64 -> (v, w); taps64: the backward's terms per contributing pixel; grad64 their sums
    brute64      the distance by a constrained minimisation written without the regions (the plane's foot when it lies
                 inside, else the nearest of the three clamped segment feet)
    toy(), fit() the toy mesh and the translation fit of the tests
"""
import numpy as np

F32 = np.float32
REF_FG_MAX = float(np.nextafter(F32(99.0), F32(np.inf)))


def points32(observed, p2m, fg_max):
    """-> (b, i, j of every data point in pixel order, p [N,3] fp32)"""
    observed = np.asarray(observed, F32)
    ax, bx, ay, by = (F32(t) for t in p2m)
    with np.errstate(invalid="ignore"):
        b, i, j = np.nonzero(observed < F32(fg_max))
    p = np.stack([ax * j.astype(F32) + bx, ay * i.astype(F32) + by, observed[b, i, j]], -1).astype(F32)
    return b, i, j, p


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _regions(ab, ac, ap, one, zero):
    """the shared statement of the seven regions, in the dtype of its arguments -> (nv, dv, nw, dw, bc)"""
    bp, cp = ap - ab, ap - ac
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    den = (va + vb) + vc
    shape = den.shape
    full = lambda x: np.broadcast_to(x, shape)   # noqa: E731
    table = [(full(vb), den, full(vc), den, None),
             (zero, one, e43, e43 + e56, (va <= 0) & (e43 >= 0) & (e56 >= 0)),        # BC
             (zero, one, d2, d2 - d6, (vb <= 0) & (d2 >= 0) & (d6 <= 0)),              # AC
             (zero, one, one, one, (d6 >= 0) & (d5 <= d6)),                            # C
             (d1, d1 - d3, zero, one, (vc <= 0) & (d1 >= 0) & (d3 <= 0)),              # AB
             (one, one, zero, one, (d3 >= 0) & (d4 <= d3)),                            # B
             (zero, one, zero, one, (d1 <= 0) & (d2 <= 0))]                            # A: the first wins, applied last
    nv, dv, nw, dw = table[0][:4]
    bc = np.zeros(shape, bool)
    for k, (a, b, c, d, m) in enumerate(table[1:]):
        nv, dv, nw, dw = np.where(m, a, nv), np.where(m, b, dv), np.where(m, c, nw), np.where(m, d, dw)
        bc = m.copy() if k == 0 else bc & ~m
    return nv, dv, nw, dw, bc


def tri_dist2_32(ap, ab, ac):
    """ap, ab, ac [...,3] fp32 (broadcast against each other) -> d2 [...] fp32, the contract's sequence"""
    ap, ab, ac = np.broadcast_arrays(np.asarray(ap, F32), np.asarray(ab, F32), np.asarray(ac, F32))
    with np.errstate(all="ignore"):
        nv, dv, nw, dw, bc = _regions(ab, ac, ap, F32(1), F32(0))
        v, w = (nv / dv).astype(F32), (nw / dw).astype(F32)
        v = np.where(bc, F32(1) - w, v)
        v = np.where(v > 1, F32(1), v); v = np.where(v < 0, F32(0), v)
        w = np.where(w > 1, F32(1), w); w = np.where(w < 0, F32(0), w)
        e = ap - (v[..., None] * ab + w[..., None] * ac)
        d2 = _dot(e, e)
    assert d2.dtype == F32
    return d2


def valid_faces(faces, NV):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < NV)).all(1)


def forward32(observed, vertices, faces, p2m=(1, 0, 1, 0), fg_max=1000.0, max_dist=np.inf, with_d2=False):
    """-> (dist [B,H,W] fp32, face [B,H,W] int32) by the serial rule: faces ascending, taken iff valid and d2 < best"""
    observed = np.asarray(observed, F32)
    vertices = np.asarray(vertices, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    B, NV = vertices.shape[:2]
    dist = np.zeros(observed.shape, F32)
    face = np.full(observed.shape, -1, np.int32)
    best2 = np.full(observed.shape, np.inf, F32)
    b, i, j, p = points32(observed, p2m, fg_max)
    ok = valid_faces(faces, NV)
    safe = np.where(ok[:, None], faces, 0)
    for k in range(B):
        sel = b == k
        if not sel.any() or not len(faces):
            continue
        a = vertices[k, safe[:, 0], :3]
        ab, ac = vertices[k, safe[:, 1], :3] - a, vertices[k, safe[:, 2], :3] - a
        best = np.full(sel.sum(), np.inf, F32)
        arg = np.full(sel.sum(), -1, np.int64)
        for f0 in range(0, len(faces), 512):                      # (memory only: the rule is the serial one)
            s = slice(f0, f0 + 512)
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = tri_dist2_32(p[sel][:, None, :] - a[None, s], ab[None, s], ac[None, s])
            d2 = np.where(ok[None, s] & (d2 == d2), d2, F32(np.inf))
            m = d2.argmin(1)                                      # the first of equal minima: the smallest f
            v = d2[np.arange(len(m)), m]
            take = v < best                                       # strict: an earlier chunk keeps a tie
            best, arg = np.where(take, v, best), np.where(take, m + f0, arg)
        got = arg >= 0
        dist[k, i[sel][got], j[sel][got]] = np.minimum(np.sqrt(best[got]), F32(max_dist))
        face[k, i[sel], j[sel]] = arg
        best2[k, i[sel], j[sel]] = best
    return (dist, face, best2) if with_d2 else (dist, face)


def closest64(ab, ac, ap):
    """the seven regions in fp64, no clamp -> (v, w)"""
    ab, ac, ap = np.broadcast_arrays(np.asarray(ab, np.float64), np.asarray(ac, np.float64), np.asarray(ap, np.float64))
    with np.errstate(all="ignore"):
        nv, dv, nw, dw, bc = _regions(ab, ac, ap, 1.0, 0.0)
        v, w = nv / dv, nw / dw
        v = np.where(bc, 1.0 - w, v)
    return v, w


def taps64(observed, vertices, faces, dist, face, grad_dist, p2m=(1, 0, 1, 0), fg_max=1000.0, max_dist=np.inf):
    """The backward's terms: (g [N,3,3] fp64, crop [N], ids [N,3]) of the contributing pixels (fixed_point_ref.Terms.from_taps
    takes them as they are)."""
    vertices = np.asarray(vertices, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    B, NV = vertices.shape[:2]
    b, i, j, p = points32(observed, p2m, fg_max)
    d, f, gd = np.asarray(dist, F32)[b, i, j], np.asarray(face, np.int64)[b, i, j], np.asarray(grad_dist, F32)[b, i, j]
    with np.errstate(invalid="ignore"):
        keep = (f >= 0) & (f < len(faces)) & (gd != 0) & (d > 0) & (d < F32(max_dist))
    if len(faces):
        keep &= valid_faces(faces, NV)[np.clip(f, 0, len(faces) - 1)]
    b, p, f, gd = b[keep], p[keep], f[keep], gd[keep].astype(np.float64)
    if not len(b):
        return np.zeros((0, 3, 3)), np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    ids = faces[f]
    c = vertices[b[:, None], ids, :3].astype(np.float64)          # [N,3 corners,3]
    ab, ac, ap = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], p.astype(np.float64) - c[:, 0]
    v, w = closest64(ab, ac, ap)
    e = ap - (v[:, None] * ab + w[:, None] * ac)
    n = np.sqrt(_dot(e, e))
    with np.errstate(all="ignore"):
        live = (n > 0) & np.isfinite(n)
        wk = np.stack([(1.0 - v) - w, v, w], -1)
        g = -gd[:, None, None] * wk[:, :, None] * (e / n[:, None])[:, None, :]
    return g[live], b[live], ids[live]


def grad64(observed, vertices, faces, dist, face, grad_dist, p2m=(1, 0, 1, 0), fg_max=1000.0, max_dist=np.inf):
    """-> grad_vertices [B,NV,3] fp64"""
    B, NV = np.asarray(vertices).shape[:2]
    g, b, ids = taps64(observed, vertices, faces, dist, face, grad_dist, p2m, fg_max, max_dist)
    out = np.zeros((B, NV, 3))
    np.add.at(out, (b[:, None], ids), g)
    return out


def _segment(p, a, b):
    d = b - a
    with np.errstate(all="ignore"):
        t = np.clip(np.nan_to_num(_dot(p - a, d) / _dot(d, d)), 0.0, 1.0)
    q = a + t[..., None] * d
    return np.sqrt(_dot(p - q, p - q))


def brute64(p, tri):
    """p [N,3], tri [F,3,3] -> the fp64 distances [N,F]: the foot on the plane when its barycentric coordinates (from the
    2 x 2 normal equations) are all >= 0, else the nearest of the three segments, each by its clamped parameter."""
    p = np.asarray(p, np.float64)[:, None, :]
    a, b, c = (np.asarray(tri, np.float64)[None, :, k] for k in range(3))
    u, v, q = b - a, c - a, p - a
    uu, uv, vv, qu, qv = _dot(u, u), _dot(u, v), _dot(v, v), _dot(q, u), _dot(q, v)
    det = uu * vv - uv * uv
    with np.errstate(all="ignore"):
        s, t = (qu * vv - qv * uv) / det, (qv * uu - qu * uv) / det
        foot = a + s[..., None] * u + t[..., None] * v
        plane = np.sqrt(_dot(p - foot, p - foot))
        inside = (det > 0) & (s >= 0) & (t >= 0) & (s + t <= 1)
    edges = np.minimum(np.minimum(_segment(p, a, b), _segment(p, b, c)), _segment(p, c, a))
    return np.where(inside, plane, edges)


# ---- the toy mesh and the translation fit -------------------------------------------------------------------------------------
TOY_SIZE = 32
FIT_SHIFT = (2.5, -1.5, 4.0)
FIT_LR, FIT_STEPS = 0.5, 24


def _grid(xs, ys, z, base):
    """vertices over xs x ys at depth z(x, y), two faces per cell wound as sil_cover_ref._grid winds them"""
    gy, gx = np.meshgrid(ys, xs, indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), z(gx, gy).ravel(), np.ones(gx.size)], -1)
    nx, faces = len(xs), []
    for r in range(len(ys) - 1):
        for c in range(nx - 1):
            k, l, m, n = r * nx + c, r * nx + c + 1, (r + 1) * nx + c, (r + 1) * nx + c + 1
            faces += [[k, l, m], [l, n, m]]
    return v, np.array(faces) + base


def toy():
    """A tilted quad (3 x 3 vertices, 8 faces) over [6, 26] x [7, 25] of a 32 x 32 crop, z = 50 + 0.15 (x - 16) + 0.1 (y - 16),
    and a fin (3 x 2 vertices, 4 faces) over [8, 24] x [9, 19] that rises from it towards the camera between y = 19 and
    y = 9, by 14 in its middle column and by 2 at its ends: its two halves and the quad have three independent normals, so
    the distances see a translation in every direction.  15 vertices, 12 faces -> (vertices [1,15,4] fp32, faces [12,3]
    int32)"""
    plane = lambda x, y: 50.0 + 0.15 * (x - 16.0) + 0.1 * (y - 16.0)   # noqa: E731
    quad, fq = _grid(np.linspace(6.0, 26.0, 3), np.linspace(7.0, 25.0, 3), plane, 0)
    rise = lambda x: np.where(x == 16.0, 14.0, 2.0)   # noqa: E731
    fin, ff = _grid(np.array([8.0, 16.0, 24.0]), np.array([9.0, 19.0]), lambda x, y: plane(x, y) - rise(x) * (19.0 - y) / 10.0, 9)
    return np.concatenate([quad, fin])[None].astype(F32), np.concatenate([fq, ff]).astype(np.int32)


def moved(rest, t):
    v = np.asarray(rest, F32).copy()
    v[..., :3] = v[..., :3] + np.asarray(t, F32)
    return v


def loss_and_grad(observed, v, faces, p2m=(1, 0, 1, 0), fg_max=REF_FG_MAX, max_dist=50.0):
    """MeshDataToModelLoss restated: (the mean of dist over all pixels, accumulated in fp64; its gradient [B,NV,3] fp64)"""
    dist, face = forward32(observed, v, faces, p2m, fg_max, max_dist)
    gd = np.full(dist.shape, F32(1.0 / dist.size), F32)
    return float(dist.astype(np.float64).mean()), grad64(observed, v, faces, dist, face, gd, p2m, fg_max, max_dist)


def fit(rest, faces, observed, shift=FIT_SHIFT, lr=FIT_LR, steps=FIT_STEPS):
    """Plain gradient descent on the translation t of moved(rest, t), fp32 parameters -> (t [3], losses)"""
    t = np.asarray(shift, F32)
    losses = []
    for _ in range(steps):
        loss, g = loss_and_grad(observed, moved(rest, t), faces)
        losses.append(loss)
        t = (t - F32(lr) * g.sum((0, 1)).astype(F32)).astype(F32)
    return t, losses
