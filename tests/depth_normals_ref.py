"""Restatements of the depth-image normals (include/spherehand_hip.h, shr_depth_normals_fwd / _bwd) on the CPU, with no use
of the library:

    forward32        (a) fp32 numpy in the stated operation order, `where` chains: what the forward kernel must reproduce bit
                     for bit, and the decisions (site, usable neighbours, zero rule) it made
    normals64        (b) fp64 torch with (a)'s decisions passed in: its autograd is the gradient reference
    loss64           render.NormalConsistencyLoss in fp64
    the input builders and the plane fit of the tests
"""
import numpy as np
import torch

import tri_normals_ref as tn

U = tn.U
F32 = np.float32
FG_MAX, MAX_STEP = 99.0, 2.0


def _shift(a, di, dj, fill=0):
    """(a[..., i + di, j + dj], inside) with `fill` outside the image"""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    inside = np.zeros(a.shape, bool)
    i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
    if i0 < i1 and j0 < j1:
        out[..., i0:i1, j0:j1] = a[..., i0 + di:i1 + di, j0 + dj:j1 + dj]
        inside[..., i0:i1, j0:j1] = True
    return out, inside


def forward32(depth, fg_max, scale=(1.0, 1.0), max_step=np.inf):
    """depth [B,H,W] -> dict: normals [B,3,H,W] fp32 and the decisions: site, ul, ur, uu, ud (usable left, right, upper,
    lower neighbour), has (site with a difference along both axes), live (has and unit3's zero rule passed); dx, dy, wx,
    wy as the contract names them (meaningless where has is False)."""
    c = np.asarray(depth, F32)
    fg, ms, sx, sy = F32(fg_max), F32(max_step), F32(scale[0]), F32(scale[1])
    with np.errstate(all="ignore"):
        site = c < fg
        (l, il), (r, ir), (u, iu), (d, id_) = _shift(c, 0, -1), _shift(c, 0, 1), _shift(c, -1, 0), _shift(c, 1, 0)
        usable = lambda n, inside: inside & (n < fg) & (np.abs((n - c).astype(F32)) <= ms)   # noqa: E731
        ul, ur, uu, ud = usable(l, il), usable(r, ir), usable(u, iu), usable(d, id_)
        dx = np.where(ul & ur, r - l, np.where(ur, r - c, c - l)).astype(F32)
        dy = np.where(uu & ud, d - u, np.where(ud, d - c, c - u)).astype(F32)
        wx = (np.where(ul & ur, F32(2), F32(1)) * sx).astype(F32)
        wy = (np.where(uu & ud, F32(2), F32(1)) * sy).astype(F32)
        N = np.stack([(dx * wy).astype(F32), (dy * wx).astype(F32), (-((wx * wy).astype(F32))).astype(F32)], -1)
        has = site & (ul | ur) & (uu | ud)
        n, live = tn.unit3_32(N)
    live = live & has
    n = np.where(live[..., None], n, F32(0)).astype(F32)
    return dict(normals=np.ascontiguousarray(np.moveaxis(n, -1, 1)), site=site, ul=ul, ur=ur, uu=uu, ud=ud, has=has, live=live,
                dx=dx, dy=dy, wx=wx, wy=wy)


DECISIONS = ("site", "ul", "ur", "uu", "ud", "live")


def _shift64(z, di, dj):
    H, W = z.shape[-2:]
    p = torch.nn.functional.pad(z, (1, 1, 1, 1))
    return p[..., 1 + di:1 + di + H, 1 + dj:1 + dj + W]


def normals64(depth, dec, scale=(1.0, 1.0)):
    """[B,3,H,W] fp64 tensor, differentiable in depth ([B,H,W] tensor), every decision taken from `dec` (forward32's).
    Depths that no difference may use (pixels that are no site, non-finite values) are replaced by 0 first: a NaN would
    otherwise reach the gradient through 0 x NaN."""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(dec[k]))   # noqa: E731
    z = depth.double()
    clean = t("site") & torch.isfinite(z.detach())
    c = torch.where(clean, z, torch.zeros_like(z))
    l, r, u, d = _shift64(c, 0, -1), _shift64(c, 0, 1), _shift64(c, -1, 0), _shift64(c, 1, 0)
    ul, ur, uu, ud = t("ul"), t("ur"), t("uu"), t("ud")
    zero = torch.zeros_like(c)
    dx = torch.where(ul & ur, r - l, torch.where(ur, r - c, torch.where(ul, c - l, zero)))
    dy = torch.where(uu & ud, d - u, torch.where(ud, d - c, torch.where(uu, c - u, zero)))
    wx = torch.where(ul & ur, 2.0, 1.0).double() * float(F32(scale[0]))
    wy = torch.where(uu & ud, 2.0, 1.0).double() * float(F32(scale[1]))
    N = torch.stack([dx * wy, dy * wx, -(wx * wy)], -1)
    return tn.unit3_64(N, dec["live"]).permute(0, 3, 1, 2)


def grad64(depth, grad_normals, fg_max, scale=(1.0, 1.0), max_step=np.inf):
    """d <grad_normals, normals64> / d depth: [B,H,W] fp64 numpy (the reference of shr_depth_normals_bwd)"""
    dec = forward32(depth, fg_max, scale, max_step)
    z = torch.from_numpy(np.asarray(depth, F32)).double().requires_grad_(True)
    (normals64(z, dec, scale) * torch.from_numpy(np.asarray(grad_normals, np.float64))).sum().backward()
    return z.grad.numpy()


def structural_zero(dec):
    """pixels whose gradient is zero by construction: the pixel has no normal and neither has a neighbour that reads it"""
    live = dec["live"]
    reads = live.copy()
    reads |= _shift(live & dec["ur"], 0, -1, False)[0]      # the left neighbour uses this pixel as its r
    reads |= _shift(live & dec["ul"], 0, 1, False)[0]
    reads |= _shift(live & dec["ud"], -1, 0, False)[0]
    reads |= _shift(live & dec["uu"], 1, 0, False)[0]
    return ~reads


def loss64(model_map, observed_map):
    """render.NormalConsistencyLoss.forward in the dtype given: [B]"""
    o = observed_map.detach()
    both = ((model_map.detach() != 0).any(1) & (o != 0).any(1)).to(model_map.dtype)
    return ((1.0 - (model_map * o).sum(1)) * both).sum((1, 2)) / both.sum((1, 2)).clamp(min=1.0)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def random_depth(B, H, W, seed, fg_max=FG_MAX, max_step=MAX_STEP):
    """Random heights with background holes, NaN and +-inf pixels, a value equal to fg_max, blocks raised by steps on both
    sides of max_step, and neighbour pairs whose difference is exactly max_step and one ulp above it."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 50 + 0.3 * xx - 0.2 * yy + 3 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + rs.uniform(-0.4, 0.4, (B, H, W))
    for b in range(B):
        for k in range(6):
            i0, j0 = rs.randint(0, H), rs.randint(0, W)
            d[b, i0:i0 + rs.randint(1, 9), j0:j0 + rs.randint(1, 9)] += (0.6, 3.0, -0.6, -3.0, 0.9, 2.5)[k] * max_step
    d = d.astype(F32)
    kind = rs.rand(B, H, W)
    d[kind < 0.10] = 100.0
    d[(kind >= 0.10) & (kind < 0.12)] = np.nan
    d[(kind >= 0.12) & (kind < 0.13)] = np.inf
    d[(kind >= 0.13) & (kind < 0.14)] = -np.inf
    d[(kind >= 0.14) & (kind < 0.15)] = fg_max
    above = np.nextafter(F32(40 + max_step), F32(np.inf))
    for b in range(B):
        for k in range(4):
            i, j = rs.randint(0, H), rs.randint(0, W)
            if j + 1 < W:
                d[b, i, j], d[b, i, j + 1] = 40.0, (40.0 + max_step if k % 2 == 0 else above)
            i, j = rs.randint(0, H), rs.randint(0, W)
            if i + 1 < H:
                d[b, i + 1, j], d[b, i, j] = 40.0, (40.0 + max_step if k % 2 == 0 else above)
    return np.ascontiguousarray(d)


def smooth_field(H, W, seed, hole_fraction=0.08):
    """[1,H,W] fp32: a smooth random height field on a 2^-10 grid of values (so that +-h, h >= 2^-10, is exact) with
    background holes"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 50 + sum(a * np.sin(xx * fx + p) * np.cos(yy * fy + q)
                 for a, fx, fy, p, q in zip(rs.uniform(1, 3, 4), rs.uniform(0.1, 0.5, 4), rs.uniform(0.1, 0.5, 4),
                                            rs.uniform(0, 6, 4), rs.uniform(0, 6, 4)))
    d = np.round(d * 1024) / 1024
    d[rs.rand(H, W) < hole_fraction] = 100.0
    return np.ascontiguousarray(d[None].astype(F32))


def plane_depth(a, b, size=48):
    """[1,size,size] fp64 tensor: z = a x + b y + 50 at the pixel centres (tri_normals_ref.tilt_grid's plane, exact)"""
    xs = torch.arange(size, dtype=torch.float64)
    gy, gx = torch.meshgrid(xs, xs, indexing="ij")
    return (a * gx + b * gy + 50.0)[None]


def plane_fit(model_map, device="cpu"):
    """Plain gradient descent on (a, b) from (0, 0), FIT_STEPS steps of FIT_LR, under the normal-consistency loss against
    the map observed at FIT_TARGET.  model_map(a, b) -> [1,3,48,48].  Returns the end point and the losses.  (Not
    tilt_fit's Adam: momentum overshoots the target by construction, so its loss rises on the way back and "the loss
    never rises" cannot be asked of it.  The loss of two planes is 1 - cos of the angle between their normals; its
    gradient's Lipschitz constant is below 1 for slopes up to FIT_TARGET's, so a fixed step of FIT_LR = 0.05 < 2 / L is a
    descent step every time, and the error contracts by about 1 - 0.05 x 0.8 per step: 0.3 x 0.96^100 = 0.005.)"""
    with torch.no_grad():
        target = model_map(*(torch.tensor(t, dtype=torch.float64) for t in tn.FIT_TARGET))
    t = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    losses = []
    for _ in range(tn.FIT_STEPS):
        loss = loss64(model_map(t[0], t[1]), target).mean()
        g, = torch.autograd.grad(loss, t)
        with torch.no_grad():
            t -= tn.FIT_LR * g
        losses.append(loss.item())
    return t.detach().numpy(), losses


def restated_plane_map(a, b):
    """the restated depth normals (fp64, decisions of the fp32 restatement) of the plane's exact depth"""
    z = plane_depth(a, b)
    return normals64(z, forward32(z.detach().numpy(), FG_MAX))
