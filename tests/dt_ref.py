"""Restatements of the silhouette distance transform and its sampler (include/spherehand_hip.h, shr_dt_fwd and
shr_dt_sample_fwd / _bwd) on the CPU in numpy, with no use of the library:

    sites                    the foreground test: depth < fg_max, a NaN is not a site
    dt_brute                 the definition: the minimum over all sites, per pixel
    dt_separable             the column pass (vertical distance to the column's nearest site) followed by the row
                             minimum: what the kernels compute, in integers
    sample32 / sample_bwd32  the sampler in fp32 in the stated operation order: what the kernels must reproduce bit for bit
    sample64                 the same taps, cell and interpolation in fp64 (takes fp64 points: central differences)
    toy_silhouette, fit      the translation fit of the tests
"""
import numpy as np

F = np.float32


def sites(depth, fg_max):
    with np.errstate(invalid="ignore"):
        return np.asarray(depth, np.float32) < np.float32(fg_max)


def empty_value(H, W):
    return H * H + W * W


def dt_brute(site):
    """site [H,W] bool -> int32 [H,W]: min over the sites (i', j') of (i - i')^2 + (j - j')^2; H H + W W without a site"""
    site = np.asarray(site, bool)
    H, W = site.shape
    si, sj = np.nonzero(site)
    if len(si) == 0:
        return np.full((H, W), empty_value(H, W), np.int32)
    out = np.empty((H, W), np.int64)
    j = np.arange(W)
    for i in range(H):
        out[i] = (((i - si) ** 2)[None, :] + (j[:, None] - sj[None, :]) ** 2).min(1)
    return out.astype(np.int32)


def column_distance2(site):
    """g^2 [H,W] int64: the squared vertical distance to the nearest site of the pixel's column; H H + W W in a column
    without one (two sweeps, as the kernel makes them)"""
    site = np.asarray(site, bool)
    H, W = site.shape
    none = H + W                                           # larger than any real distance
    g = np.full((H, W), none, np.int64)
    run = np.full(W, none, np.int64)
    for i in range(H):                                     # nearest site at or above
        run = np.where(site[i], 0, np.minimum(run + 1, none))
        g[i] = run
    run = np.full(W, none, np.int64)
    for i in range(H - 1, -1, -1):                         # ... or below
        run = np.where(site[i], 0, np.minimum(run + 1, none))
        g[i] = np.minimum(g[i], run)
    return np.where(g >= none, empty_value(H, W), g * g)


def dt_separable(site):
    """site [H,W] bool -> int32 [H,W]: d2[i,x] = min over x' of (x - x')^2 + g^2[i,x']"""
    g2 = column_distance2(site)
    H, W = g2.shape
    j = np.arange(W)
    dx2 = (j[:, None] - j[None, :]) ** 2                   # [x, x']
    out = np.empty((H, W), np.int64)
    rows = max(1, (1 << 22) // (W * W))
    for a in range(0, H, rows):
        out[a:a + rows] = (dx2[None] + g2[a:a + rows, None, :]).min(2)
    return out.astype(np.int32)


def transform(depth, fg_max):
    """depth [B,H,W] -> int32 [B,H,W] by dt_separable"""
    return np.stack([dt_separable(sites(d, fg_max)) for d in np.asarray(depth)])


# ---- the sampler ----------------------------------------------------------------------------------------------------------
def _cell(x, n, R):
    """(i0 int64, f, clamped) of coordinates x (finite) on an axis of n samples, in the real type R"""
    xc = np.minimum(np.maximum(x, R(0)), R(n - 1))
    x0 = np.minimum(np.floor(xc), R(n - 2))
    return x0.astype(np.int64), (xc - x0).astype(R), xc != x


def _taps(d2, b, y0, x0, max_dist):
    """the four fp32 taps min(sqrt((float)d2), max_dist) of every point"""
    with np.errstate(invalid="ignore"):
        t = np.minimum(np.sqrt(np.asarray(d2).astype(np.float32)), F(max_dist)).astype(np.float32)
    return t[b, y0, x0], t[b, y0, x0 + 1], t[b, y0 + 1, x0], t[b, y0 + 1, x0 + 1]


def _sample(d2, points, max_dist, R):
    d2 = np.asarray(d2)
    B, H, W = d2.shape
    P = np.asarray(points, R)
    x, y = P[..., 0], P[..., 1]
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = np.where(ok, x, R(0)), np.where(ok, y, R(0))
    x0, fx, cx = _cell(x, W, R)
    y0, fy, cy = _cell(y, H, R)
    b = np.broadcast_to(np.arange(B)[:, None], x.shape)
    t00, t01, t10, t11 = (t.astype(R) for t in _taps(d2, b, y0, x0, max_dist))
    ux, uy = (R(1) - fx).astype(R), (R(1) - fy).astype(R)
    with np.errstate(invalid="ignore"):                    # (inf taps: max_dist = inf over a garbage transform)
        top = ((t00 * ux).astype(R) + (t01 * fx).astype(R)).astype(R)
        bot = ((t10 * ux).astype(R) + (t11 * fx).astype(R)).astype(R)
        value = ((top * uy).astype(R) + (bot * fy).astype(R)).astype(R)
        gx = (((t01 - t00).astype(R) * uy).astype(R) + ((t11 - t10).astype(R) * fy).astype(R)).astype(R)
        gy = (bot - top).astype(R)
    gx, gy = np.where(cx, R(0), gx), np.where(cy, R(0), gy)
    value = np.where(ok, value, R(0)).astype(R)
    grad = np.stack([np.where(ok, gx, R(0)), np.where(ok, gy, R(0))], -1).astype(R)
    return value, grad, np.maximum(np.maximum(t00, t01), np.maximum(t10, t11))


def sample32(d2, points, max_dist=np.inf):
    """d2 [B,H,W] int32, points [B,N,C] fp32 -> (value [B,N], grad_xy [B,N,2]) fp32, one rounding per written operation"""
    v, g, _ = _sample(d2, np.asarray(points, np.float32), max_dist, np.float32)
    return v, g


def sample64(d2, points, max_dist=np.inf):
    """the fp64 twin on the same fp32 taps: (value, grad_xy, the largest of each point's four taps)"""
    return _sample(d2, np.asarray(points, np.float64), max_dist, np.float64)


def sample_bwd32(grad_xy, grad_value, C):
    """grad_points [B,N,C] fp32: grad_value * grad_xy in components 0 and 1, 0 elsewhere"""
    gxy, gv = np.asarray(grad_xy, np.float32), np.asarray(grad_value, np.float32)
    out = np.zeros(gv.shape + (C,), np.float32)
    with np.errstate(invalid="ignore"):
        out[..., :2] = gv[..., None] * gxy
    return out


# ---- the fit --------------------------------------------------------------------------------------------------------------
def toy_silhouette(S=128):
    """a palm (an ellipse) with three fingers (bars) in the lower left of an S x S image, far enough from the borders
    that the silhouette shifted by (25, 18) stays inside: site [S,S] bool"""
    i, j = np.mgrid[0:S, 0:S]
    palm = ((j - 50) / 22.0) ** 2 + ((i - 70) / 18.0) ** 2 <= 1
    fingers = np.zeros((S, S), bool)
    for c in (38, 50, 62):
        fingers |= (np.abs(j - c) <= 3) & (i >= 22) & (i <= 60)
    return palm | fingers


def points_inside(site, n, seed=0):
    """n points [1,n,2] fp32 (x, y) on site pixels, jittered inside the pixel's cell"""
    rs = np.random.RandomState(seed)
    si, sj = np.nonzero(site)
    k = rs.randint(0, len(si), n)
    p = np.stack([sj[k] + rs.uniform(-0.4, 0.4, n), si[k] + rs.uniform(-0.4, 0.4, n)], -1)
    return p[None].astype(np.float32)


def fit(d2, points, steps, lr, max_dist=np.inf):
    """Plain gradient descent on a translation t (fp32, from 0) of points [1,N,C] fp32 under loss = mean of sample32 at
    points - t; the model's arithmetic in fp32 as the GPU fit does it (the mean's sum in fp64).  -> (t [2], losses)"""
    P = np.asarray(points, np.float32)
    N, C = P.shape[1], P.shape[2]
    t = np.zeros(2, np.float32)
    gv = np.full((1, N), F(1) / F(N), np.float32)
    losses = []
    for _ in range(steps):
        shift = np.zeros(C, np.float32)
        shift[:2] = t
        value, gxy = sample32(d2, (P - shift).astype(np.float32), max_dist)
        losses.append(float(value.astype(np.float64).mean()))
        gp = sample_bwd32(gxy, gv, C)
        gt = (-gp[0, :, :2].astype(np.float64).sum(0)).astype(np.float32)      # d loss / d t
        t = (t - F(lr) * gt).astype(np.float32)
    return t, losses
