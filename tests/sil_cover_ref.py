"""Restatements of the nearest-site transform and of the silhouette coverage term (include/spherehand_hip.h,
shr_dt_nearest_fwd and shr_sil_cover_fwd / _bwd) on the CPU in numpy and torch, with no use of the library:

    nearest_brute            the definition: per pixel the nearest site, the smallest index among equally near ones
    nearest_separable        the two-pass rule the kernels follow, in integers: per column the vertically nearest site (an
                             up / down tie: the smaller row), per row the lexicographic minimum of (total, index)
    cover32                  the forward in fp32: the kernel's bits
    cover_grad64             the gradient in fp64: the map G summed per nearest pixel, handed to tri_interp_ref.grads as the
                             gradient of the attribute (x, y)
    frozen                   the frozen function of the central differences: the weights and the nearest pixel held
    mitten, model, fit       the toy mesh and the scale-and-shift fit of the tests
    patterns, SHAPES         tests/test_dist_transform_gpu.py's images
"""
import numpy as np
import torch

import dt_ref
import tri_interp_ref

F32 = np.float32
INDEX_BITS = 22                                            # H W <= 2^22


# ---- the transform --------------------------------------------------------------------------------------------------------
def nearest_brute(site):
    """site [H,W] bool -> (d2, nearest) int32 [H,W]: the minimum over the sites of (i - i')^2 + (j - j')^2 and i' W + j' of
    the site that attains it with the smallest index; (H H + W W, -1) without a site"""
    site = np.asarray(site, bool)
    H, W = site.shape
    si, sj = np.nonzero(site)                              # row-major: ascending index
    if len(si) == 0:
        return np.full((H, W), dt_ref.empty_value(H, W), np.int32), np.full((H, W), -1, np.int32)
    d2, near = np.empty((H, W), np.int64), np.empty((H, W), np.int64)
    j = np.arange(W)
    for i in range(H):
        d = ((i - si) ** 2)[None, :] + (j[:, None] - sj[None, :]) ** 2
        k = d.argmin(1)                                    # the first minimum: the smallest index
        d2[i], near[i] = d[j, k], si[k] * W + sj[k]
    return d2.astype(np.int32), near.astype(np.int32)


def column_nearest(site):
    """(g [H,W] int64 the vertical distance to the column's nearest site, row [H,W] its row, has [H,W] whether the column
    has a site): two sweeps; a site above and one below at the same distance: the one above (the smaller row)"""
    site = np.asarray(site, bool)
    H, W = site.shape
    none = H + W
    above, below = np.full((H, W), none, np.int64), np.full((H, W), none, np.int64)
    run = np.full(W, none, np.int64)
    for i in range(H):
        run = np.where(site[i], 0, np.minimum(run + 1, none))
        above[i] = run
    run = np.full(W, none, np.int64)
    for i in range(H - 1, -1, -1):
        run = np.where(site[i], 0, np.minimum(run + 1, none))
        below[i] = run
    i = np.arange(H)[:, None]
    up = above <= below
    g = np.where(up, above, below)
    return g, np.where(up, i - above, i + below), g < none


def nearest_separable(site):
    """site [H,W] bool -> (d2, nearest) int32 [H,W] by the two passes: the row pass minimises the single integer
    (total << 22) | index, which orders the pairs (total, index) lexicographically"""
    g, row, has = column_nearest(site)
    H, W = g.shape
    none2 = dt_ref.empty_value(H, W)
    j = np.arange(W)
    key = np.where(has, ((g * g) << INDEX_BITS) | (row * W + j[None, :]), np.int64(none2) << INDEX_BITS)
    dx2 = ((j[:, None] - j[None, :]) ** 2) << INDEX_BITS   # [x, x']
    best = np.empty((H, W), np.int64)
    rows = max(1, (1 << 22) // (W * W))
    for a in range(0, H, rows):
        best[a:a + rows] = (dx2[None] + key[a:a + rows, None, :]).min(2)
    d2 = best >> INDEX_BITS
    near = np.where(d2 >= none2, -1, best & ((1 << INDEX_BITS) - 1))
    return d2.astype(np.int32), near.astype(np.int32)


def transform(depth, fg_max):
    """depth [B,H,W] -> (d2, nearest) int32 [B,H,W] by nearest_separable"""
    out = [nearest_separable(dt_ref.sites(d, fg_max)) for d in np.asarray(depth)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- the coverage term ----------------------------------------------------------------------------------------------------
def cover32(observed, obs_fg_max, d2, max_dist=np.inf):
    """dist [B,H,W] fp32: min(sqrt((float)d2), max_dist) where observed < obs_fg_max (a NaN is not observed), 0 elsewhere"""
    t = np.minimum(np.sqrt(np.asarray(d2).astype(np.float32)), F32(max_dist)).astype(np.float32)
    return np.where(dt_ref.sites(observed, obs_fg_max), t, F32(0)).astype(np.float32)


def contributing(observed, obs_fg_max, d2, nearest, grad_dist, max_dist=np.inf):
    """(b, y, x, q) of the pixels that pass the backward's tests up to `nearest` (the owner, the face and the liveness of
    q are tri_interp_ref's)"""
    d2, nearest = np.asarray(d2), np.asarray(nearest)
    B, H, W = d2.shape
    ok = dt_ref.sites(observed, obs_fg_max) & (d2 > 0) & (np.sqrt(d2.astype(np.float32)) <= F32(max_dist))
    ok &= (np.asarray(grad_dist, np.float32) != 0) & (nearest >= 0) & (nearest < H * W)
    b, y, x = np.nonzero(ok)
    return b, y, x, nearest[b, y, x].astype(np.int64)


def pull_map(observed, obs_fg_max, d2, nearest, grad_dist, max_dist=np.inf):
    """G [B,2,H,W] fp64: G[b,:,q] = sum over the contributing pixels p with nearest(p) = q of -grad_dist(p) (p - q) / d,
    d = sqrt(d2) in fp64; and the pixels (b, y, x, q)"""
    d2 = np.asarray(d2)
    B, H, W = d2.shape
    b, y, x, q = contributing(observed, obs_fg_max, d2, nearest, grad_dist, max_dist)
    yq, xq = q // W, q % W
    d = np.sqrt(d2[b, y, x].astype(np.float64))
    gd = np.asarray(grad_dist, np.float32)[b, y, x].astype(np.float64)
    G = np.zeros((B, 2, H, W))
    np.add.at(G, (b, 0, yq, xq), -gd * (x - xq) / d)
    np.add.at(G, (b, 1, yq, xq), -gd * (y - yq) / d)
    return G, (b, y, x, q)


def cover_grad64(observed, obs_fg_max, d2, nearest, owner, vertices, faces, grad_dist, max_dist=np.inf, with_max=False):
    """grad_vertices[..., :2] [B,NV,2] fp64: the attribute gradient of the interpolation for the attribute (x, y) under the
    map G (tri_interp_ref.grads, unchanged: the fp32 clamp decisions, owner / face / vertex ids out of range skipped, the
    liveness rule).  with_max: also m [B], each crop's largest |term| -grad_dist(p) wh_a(q) u(p)."""
    v = np.asarray(vertices, np.float32)
    G, (b, y, x, q) = pull_map(observed, obs_fg_max, d2, nearest, grad_dist, max_dist)
    xy = np.ascontiguousarray(v[..., :2])
    grad = tri_interp_ref.grads(xy, owner, v, faces, G)[0]
    if not with_max:
        return grad
    B, H, W = np.asarray(d2).shape
    _, info = tri_interp_ref.interp32(xy, owner, v, faces, with_info=True)
    whmax = np.zeros((B, H, W))
    live = info["live"]
    whmax[info["b"][live], info["y"][live], info["x"][live]] = info["wh"][live].max(1)
    d = np.sqrt(np.asarray(d2)[b, y, x].astype(np.float64))
    u = np.maximum(np.abs(x - q % W), np.abs(y - q // W)) / d
    term = np.abs(np.asarray(grad_dist, np.float32)[b, y, x].astype(np.float64)) * whmax[b, q // W, q % W] * u
    m = np.zeros(B)
    np.maximum.at(m, b, term)
    return grad, m


def weight_maps(owner, vertices, faces):
    """M [B,NV,H,W] fp64: the normalised weight of every vertex at every pixel (the interpolation of the one-hot
    attributes; small meshes only)"""
    v = torch.as_tensor(np.asarray(vertices, np.float32))
    NV = v.shape[1]
    return tri_interp_ref.interp64(torch.eye(NV, dtype=torch.float64), owner, v, faces).numpy()


def frozen(delta, M, pixels, d2, grad_dist, W):
    """The frozen function at the vertices moved by delta [B,NV,2] fp64: sum over the contributing pixels p of
    grad_dist(p) |p - (q + sum_v M[v,q] delta_v)| -- q a material point of its owner face, the weights M and the choice of
    q held.  (Where no weight of q is clamped, q = sum_v M[v,q] V_v, and the term is |p - sum_a wh_a V_a|.)"""
    b, y, x, q = pixels
    yq, xq = q // W, q % W
    Mq = M[b, :, yq, xq]                                    # [P,NV]
    move = np.einsum("pv,pvc->pc", Mq, delta[b])
    r = np.stack([x - xq, y - yq], -1) - move
    gd = np.asarray(grad_dist, np.float32)[b, y, x].astype(np.float64)
    return float((gd * np.sqrt((r * r).sum(-1))).sum())


# ---- the toy mesh and the fit ---------------------------------------------------------------------------------------------
MITTEN_SIZE, MITTEN_MARGIN = 64, 12
# The mitten's box.  The outline lies a tenth of a pixel outside the outermost covered pixel centres on every side: a
# vertex on it samples a distance of 0.1 .. 0.2 px, so the two halves balance a fraction of a pixel inside s = 1 (an
# outline half a pixel off the centres would balance at s = 0.97)
X0, X1, Y0, Y1 = 13.9, 50.1, 12.9, 51.1
MITTEN_HALF_EXTENT = (Y1 - Y0) / 2                         # R: half the larger side of the box, 19.1 px
FIT_S0, FIT_T0 = 0.6, (6.0, -4.0)
# step 4 on the shift, 0.004 on the scale, 40 steps: the restated fit ends at s = 0.993, t = (0.04, -0.08) px (with step
# 8 on the shift the last steps hop about the minimum by a pixel of shift)
FIT_STEPS, FIT_LR_T, FIT_LR_S = 40, 4.0, 0.004
FIT_FG_MAX = 900.0


def _grid(x0, x1, nx, y0, y1, ny, z, base):
    """nx x ny vertices over [x0, x1] x [y0, y1] at depth z, faces as tri_normals_ref.tilt_grid winds them (every one
    drawn by the raster's cull), vertex ids from `base`"""
    gy, gx = np.meshgrid(np.linspace(y0, y1, ny), np.linspace(x0, x1, nx), indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), np.full(nx * ny, z), np.ones(nx * ny)], -1)
    faces = []
    for i in range(ny - 1):
        for j in range(nx - 1):
            p, q, r, s = i * nx + j, i * nx + j + 1, (i + 1) * nx + j, (i + 1) * nx + j + 1
            faces += [[p, q, r], [q, s, r]]
    return v, np.array(faces) + base


def mitten():
    """A palm (a 5 x 5 vertex grid) and three finger bars (2 x 5 grids) side by side above it, the middle one the longest:
    55 vertices, 56 faces, inside [13.9, 50.1] x [12.9, 51.1] of a 64 x 64 crop (a margin of 12 px and more).  The bars
    touch, so the outline is a mitten's and the shape is star-shaped about its vertex centroid: scaled down about it, every
    vertex lies inside the original.  -> (vertices [1,55,4] fp32, faces [56,3] int32 to be rastered with right_hand=False)"""
    parts = [(X0, X1, 5, 34.1, Y1, 5, 50.0)]
    w = (X1 - X0) / 3
    for k, (top, z) in enumerate(((18.9, 48.0), (Y0, 47.0), (16.9, 49.0))):
        parts.append((X0 + k * w, X0 + (k + 1) * w, 2, top, 34.1, 5, z))
    vs, fs, base = [], [], 0
    for p in parts:
        v, f = _grid(*p, base)
        vs.append(v)
        fs.append(f)
        base += len(v)
    return np.concatenate(vs)[None].astype(np.float32), np.concatenate(fs).astype(np.int32)


def model(rest, s, t):
    """rest [1,NV,4] fp32 scaled by s about its vertex centroid and moved by t, x and y only, in fp32 in this order:
    c + s (rest - c) + t"""
    rest = np.asarray(rest, np.float32)
    c = rest[0, :, :2].mean(0, dtype=np.float32)
    v = rest.copy()
    v[0, :, :2] = ((c + (F32(s) * (rest[0, :, :2] - c)).astype(np.float32)).astype(np.float32)
                   + np.asarray(t, np.float32)).astype(np.float32)
    return v


def render(v, faces, W, H):
    """(depth [1,H,W] of the reference raster on the CPU, owner [1,H,W]) of vertices [1,NV,4]"""
    from oracle import oracle
    depth = oracle.tri_raster_fwd(np.ascontiguousarray(v[:, faces.astype(np.int64), :3]), W, H)
    return depth, tri_interp_ref.cpu_owners(depth, v, faces)


def fit(rest, faces, observed, steps=FIT_STEPS, lr_t=FIT_LR_T, lr_s=FIT_LR_S, s0=FIT_S0, t0=FIT_T0, fg_max=FIT_FG_MAX,
        cover=True):
    """Plain gradient descent on (s, t) of model(rest, s, t) under loss = the mean sampled distance of the vertices to the
    observed silhouette (dt_ref.sample32: SilhouetteDistance) + with `cover` the mean distance of the observed pixels to
    the rendered silhouette (cover32 / cover_grad64: SilhouetteCoverage).  -> (s, t [2], losses)"""
    observed = np.asarray(observed, np.float32)
    _, H, W = observed.shape
    rest = np.asarray(rest, np.float32)
    c = rest[0, :, :2].mean(0, dtype=np.float32)
    NV = rest.shape[1]
    d2_obs = dt_ref.transform(observed, fg_max)
    count = max(1, int(dt_ref.sites(observed, fg_max).sum()))
    s, t = F32(s0), np.asarray(t0, np.float32)
    losses = []
    for _ in range(steps):
        v = model(rest, s, t)
        value, gxy = dt_ref.sample32(d2_obs, v)
        loss = float(value.astype(np.float64).mean())
        g = gxy[0].astype(np.float64) / NV
        if cover:
            depth, owner = render(v, faces, W, H)
            d2, near = transform(depth, 1000.0)
            loss += float(cover32(observed, fg_max, d2).astype(np.float64).sum() / count)
            gd = np.full((1, H, W), F32(1) / F32(count), np.float32)
            g = g + cover_grad64(observed, fg_max, d2, near, owner, v, faces, gd)[0]
        losses.append(loss)
        gs = float((g * (rest[0, :, :2] - c).astype(np.float64)).sum())
        gt = g.sum(0)
        s = F32(s - F32(lr_s) * F32(gs))
        t = (t - F32(lr_t) * gt.astype(np.float32)).astype(np.float32)
    return float(s), t, losses


# ---- tests/test_dist_transform_gpu.py's images ----------------------------------------------------------------------------
FG_MAX = 500.0
SHAPES = [(1, 1), (1, 7), (5, 1), (3, 130), (67, 65), (128, 128), (130, 257), (64, 640)]


def patterns(H, W, seed=0):
    """depth [13,H,W] fp32, sites where depth < FG_MAX: 0 empty, 1 full, 2..5 one site in a corner, 6 a column and the far
    corner, 7 checkerboard, 8 and 9 random, 10 NaN and FG_MAX itself among the non-sites, 11 all FG_MAX, 12 infinite"""
    rs = np.random.RandomState(seed + 1000 * H + W)
    bg, fg = np.float32(1000.0), np.float32(60.0)
    out = [np.full((H, W), bg), np.full((H, W), fg)]
    for i, j in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        d = np.full((H, W), bg)
        d[i, j] = fg
        out.append(d)
    d = np.full((H, W), bg)
    d[:, 0] = fg
    d[H - 1, W - 1] = fg
    out.append(d)
    i, j = np.mgrid[0:H, 0:W]
    out.append(np.where((i + j) % 2 == 0, fg, bg))
    out.append(np.where(rs.rand(H, W) < 0.001, fg, bg))
    out.append(np.where(rs.rand(H, W) < 0.3, fg, bg))
    d = np.where(rs.rand(H, W) < 0.02, fg, bg).astype(np.float32)
    d[rs.rand(H, W) < 0.3] = np.nan
    d[rs.rand(H, W) < 0.3] = FG_MAX
    out.append(d)
    out.append(np.full((H, W), np.float32(FG_MAX)))
    out.append(np.where(rs.rand(H, W) < 0.01, np.float32(-np.inf), np.float32(np.inf)))
    return np.stack(out).astype(np.float32)
