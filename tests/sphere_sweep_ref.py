"""The sweep of the sphere fit's scan entries over sphere counts and tile edges (test helper, not a
conftest), on top of sphere_icp_ref, sphere_radii_ref and sphere_render_icp_ref, none of which it changes:

    table, sweep_case   a random table of J spheres and a case at W x H under V views whose observation holds data whatever
                        the geometry: the table's render at p*, every second background pixel at a random depth, a few NaN
                        pixels and a few exactly at fg_max
    icp_rows, render_rows   GIVEN the entry's own fp32 view-frame centres: the fp32 owner / render rule (the existing numpy
                        rules, bit for bit) and from those fp32 values the fp64 per-pixel terms as the header words them
    dense               the moments, A, g (and C, R, gs) summed densely in fp64, beside every sum the sum of the absolute
                        values of its terms, from which the bar of that sum follows
    partitioned         the same sums the way the kernels partition them: tiles of 1024, rounds of 256, a chain per entry,
                        the records added tiles ascending, views ascending; `wrong` names a deliberately wrong variant
    ratios              error / bar per quantity: the comparator of the CPU and the GPU tests

The bars are derived, not measured.  A sum of n fp64 terms formed in any order is within (n - 1) 2^-53 sum |terms| of the
exact sum; the kernel's chain and the dense sum it is compared with each are, so they differ by less than n 2^-52 sum |terms|.
The terms themselves are the same bits on both sides (fp64 operations on the same fp32 values, nothing contracted); 16 more
units cover the multiply-adds inside a term of A, g and C, where a term is a product of a moment and two Jacobian entries."""
import math

import numpy as np
import torch

import pose_icp_ref as ref
import pose_icp_views_ref as vref
import pose_ik_ref
import sphere_icp_ref as sref
import sphere_radii_ref as gref
import sphere_render_icp_ref as rref

TILE, ROUND = gref.TILE, 256
EPS, SLACK = 2.0 ** -52, 16
FG_MAX, MAX_DIST, BACKGROUND = sref.FG_MAX, sref.MAX_DIST, sref.BACKGROUND
MAX_RESID = rref.DEFAULT_MAX_RESID
KINDS = ("identity", "general", "y", "x", "general")
SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])

# (J, W, H, V, starred: also through the radii and the render entries, seed).  The seeds are chosen on the restatement
# alone so that tests/test_sphere_sweep_cpu.py's conditions hold.
CASES = (
    (1, 1, 1, 1, True, 21),         # one pixel, one sphere
    (1, 300, 1, 1, False, 3),       # H = 1, a partial tile, lanes past npix in wave 4
    (2, 1, 300, 2, True, 23),       # W = 1
    (7, 7, 5, 1, False, 4),         # 35 pixels: less than a wave
    (16, 16, 16, 1, True, 5),       # exactly one round; 16 x 16 entries = one chain
    (17, 17, 15, 3, True, 6),       # 255 pixels; first entry of the second chain at kMom = 16
    (21, 33, 31, 1, False, 7),      # 1023 pixels; 252 entries
    (22, 41, 25, 1, True, 8),       # 1025 pixels (a second tile of one pixel); 264 entries
    (32, 32, 33, 2, True, 9),       # 512 entries at kMom = 16 exactly
    (33, 48, 40, 1, True, 10),      # 528 entries
    (42, 61, 59, 1, False, 11),     # 3599 pixels, 4 tiles; 504 entries
    (43, 61, 59, 2, True, 12),      # 8 records; 516 entries: the third chain begins
    (63, 50, 41, 5, False, 13),     # 3 tiles x 5 views = 15 records
    (64, 33, 31, 1, True, 14),      # the full record, one partial tile
    (64, 128, 72, 1, True, 15),     # 9 full tiles: 9 records
    (64, 61, 59, 3, True, 16),      # 12 records; every chain slot of every thread in use
)


def case_id(spec):
    J, W, H, V = spec[:4]
    return "J%d_%dx%d_V%d" % (J, W, H, V)


def table(J, seed):
    """(bone [J] int32, wv [J,4] fp32, radii [J] fp32): bones drawn from 0..16 with bone 5 named at least twice when J >= 2,
    offsets in +-40 mm, radii in 4..14 mm."""
    rng = np.random.default_rng(seed)
    bone = rng.integers(0, 17, J).astype(np.int32)
    if J >= 2:
        bone[rng.choice(J, 2, replace=False)] = 5
    wv = np.concatenate([rng.uniform(-40.0, 40.0, (J, 3)), np.ones((J, 1))], axis=1).astype(np.float32)
    return bone, wv, rng.uniform(4.0, 14.0, J).astype(np.float32)


def grid(W, H):
    """pixel_to_model of the sweep: the reference's 300 mm window sampled at the pixels' CENTRES, so that a 1 x 1 image looks
    at the window's middle and W = 1 or H = 1 at its middle column or row."""
    return (300.0 / W, -150.0 + 150.0 / W, 300.0 / H, -150.0 + 150.0 / H)


def special_spheres(J):
    """For J >= 22: sphere 0, sphere J - 1 and the spheres that hold moment entries 256 and 512 of the [J x 12] and the
    [J x 16] record, where they exist -- the first entries of a thread's second and third chain."""
    if J < 22:
        return ()
    out = {0, J - 1}
    for kmom in (12, 16):
        out |= {e // kmom for e in (256, 512) if e < kmom * J}
    return tuple(sorted(out))


def _place(mesh, tab, p, k, target):
    """The table with sphere k's offset replaced so that at pose p [26] its centre is `target` (the frame ops.PoseSpheres
    outputs, right hand): what synthetic_case does with a view, done in the table, since the views are the cases' own."""
    bone, wv, radii = tab
    chain = pose_ik_ref.Chain(mesh, bone, wv, True, torch.float64)
    T = chain.fk.forward_torch(p[None].double())[0, int(np.clip(bone[k], 0, 16))].numpy()
    wv = wv.copy()
    wv[k] = np.linalg.solve(T, np.array([-target[0], target[1], target[2], 1.0])).astype(np.float32)
    wv[k, 3] = 1.0
    return bone, wv, radii


def sweep_case(mesh, J, W, H, V, B=2, seed=0):
    """The case of one row of CASES.  Poses: pose_icp_ref.poses(B, seed), evaluated at the starts; views: identity, then the
    general rotation, then y, x.  Sphere min(1, J - 1) is placed (in the table) 1 mm beside the image's last grid point of
    sample 0, view 0, 50 mm deep, and that pixel looks at it from 2 mm in front of its surface.  Observation: the table's
    render at p*; every second background pixel, by a seeded draw, at a depth uniform in 20..80 mm; in sample 0 the first and
    the last pixel of every tile made data points where they are not; for every sphere of special_spheres(J) the pixel
    nearest to its centre in sample 0, view 0 set 1 mm in front of its surface; then, where the image has more than one
    pixel, up to three pixels NaN and up to three exactly fg_max, none of them one of the pixels above."""
    rng = np.random.default_rng(1000 + seed)
    p, p0 = ref.poses(B, seed)
    p0 = p0.float().double()
    view = vref.views(B, KINDS[:V])
    p2m = grid(W, H)
    gx, gy = sref.grid32(p2m, W, H)
    tab = table(J, seed)
    pinned = min(1, J - 1)
    tab = _place(mesh, tab, p0[0], pinned, (float(gx[-1]) - 1.0, float(gy[-1]) - 1.0, 50.0))
    model = sref.Spheres(mesh, tab, True)
    obs = sref.render(model, view, p, W, H, p2m)
    draw = rng.random(obs.shape) < 0.5
    depth = rng.uniform(20.0, 80.0, obs.shape).astype(np.float32)
    obs = np.where((obs >= np.float32(BACKGROUND)) & draw, depth, obs).astype(np.float32)
    npix = H * W
    flat = obs.reshape(B, V, npix)
    held = set()
    tiles = (npix + TILE - 1) // TILE
    if tiles > 1:
        for t in range(tiles):
            for i in (t * TILE, min(npix, (t + 1) * TILE) - 1):
                for v in range(V):
                    if not flat[0, v, i] < np.float32(FG_MAX):
                        flat[0, v, i] = depth.reshape(B, V, npix)[0, v, i]
                    held.add((0, v, i))
    c32 = model.to(torch.float32).centres32(p0, view)
    for s in special_spheres(J):
        if s == pinned:
            continue
        col, row = int(np.abs(gx - c32[0, 0, s, 0]).argmin()), int(np.abs(gy - c32[0, 0, s, 1]).argmin())
        if (0, 0, row * W + col) not in held:
            flat[0, 0, row * W + col] = c32[0, 0, s, 2] - tab[2][s] - np.float32(1.0)
            held.add((0, 0, row * W + col))
    flat[0, 0, npix - 1] = np.float32(50.0) - tab[2][pinned] - np.float32(2.0)
    held.add((0, 0, npix - 1))
    nan_px, fg_px = [], []
    if npix > 1:
        free = [(b, v, i) for b in range(B) for v in range(V) for i in range(npix) if (b, v, i) not in held]
        pick = rng.permutation(len(free))[:min(6, 2 * (len(free) // 2))]
        for n, q in enumerate(pick):
            b, v, i = free[q]
            flat[b, v, i] = np.float32(np.nan) if n % 2 == 0 else np.float32(FG_MAX)
            (nan_px if n % 2 == 0 else fg_px).append((b, v, i))
    return dict(name="J%d_%dx%d_V%d" % (J, W, H, V), model=model, J=J, W=W, H=H, V=V, B=B, p2m=p2m, p_star=p, params0=p0,
                view=view, observed=obs, stiffness=torch.ones(26, dtype=torch.float64), pinned=pinned, nan_px=nan_px,
                fg_px=fg_px)


_CACHE = {}


def cached_case(mesh, spec):
    """sweep_case of a row of CASES, once per process; nothing modifies it."""
    if spec not in _CACHE:
        J, W, H, V, _, seed = spec
        _CACHE[spec] = sweep_case(mesh, J, W, H, V, seed=seed)
    return _CACHE[spec]


def cpu_inputs(case):
    """(c32 [B,V,J,3], jac32 [B,3J,26], view32 [B,V,4,4]) numpy fp32 of the fp32 CPU chain at the case's params0: what the
    entries are handed on the device up to the chain's own rounding."""
    m32 = case["model"].to(torch.float32)
    p0 = case["params0"]
    return (m32.centres32(p0, case["view"]), m32.chain.jacobian(p0.float())[1].numpy(),
            case["view"].numpy().astype(np.float32))


def second_radii(radii, B):
    """[B,J] fp32: one table per frame (G = B groups of N = 1), frame q's radii scaled by 1 - q / 10."""
    r = np.asarray(radii, np.float32)
    return np.stack([(r * np.float32(1.0 - 0.1 * q)).astype(np.float32) for q in range(B)])


# ---- the per-pixel terms ------------------------------------------------------------------------------------------------
def _moment_terms(u, d, kmom):
    cols = [u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2], d * u[0], d * u[1], d * u[2], d * d,
            np.ones_like(d), np.zeros_like(d)]
    if kmom > 12:
        cols += [u[0], u[1], u[2], d]
    return np.stack(cols, -1) if len(d) else np.zeros((0, kmom))


def icp_rows(observed, c32, radii, N, view32, p2m, kmom=12, fg_max=FG_MAX, max_dist=MAX_DIST):
    """shr_sphere_icp_normal's (kmom 12) or shr_sphere_icp_radii_normal's (16) rows GIVEN the entry's inputs.  radii [J], or
    [G,J] with N frames per group.  dist and owner by sphere_icp_ref.owner_dist32 (fp32, the header's rule); for a pixel
    with a row, from the fp32 p, c, r: e = p - c, n = sqrt((ex ex + ey ey) + ez ez), d = n - r, u_v = e / n,
    u_k = (R_0k u_v0 + R_1k u_v1) + R_2k u_v2, all fp64.  -> dict: b, v, pix (row-major, ascending inside a view), o, T
    [rows,kmom], c2 [B,V,H W] = (double)dist^2, dist, owner."""
    obs = np.asarray(observed, np.float32)
    c32 = np.asarray(c32, np.float32)[..., :3]
    radii = np.atleast_2d(np.asarray(radii, np.float32))
    B, V, H, W = obs.shape
    dist, owner = gref.group_maps(obs, c32, radii, N, p2m, fg_max, max_dist)
    px, py = sref.grid32(p2m, W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = (obs < np.float32(fg_max)) & (owner >= 0) & (dist < np.float32(max_dist))
        b, v, i, j = np.nonzero(keep)
        o = owner[b, v, i, j].astype(np.int64)
        c, r = c32[b, v, o].astype(np.float64), radii[b // N, o].astype(np.float64)
        ex, ey = px[j].astype(np.float64) - c[:, 0], py[i].astype(np.float64) - c[:, 1]
        ez = obs[b, v, i, j].astype(np.float64) - c[:, 2]
        n = np.sqrt((ex * ex + ey * ey) + ez * ez)
        live = (n > 0) & (n <= np.finfo(np.float64).max)
    b, v, i, j, o, ex, ey, ez, n, r = (t[live] for t in (b, v, i, j, o, ex, ey, ez, n, r))
    d = n - r
    uv = (ex / n, ey / n, ez / n)
    R = np.asarray(view32, np.float32)[b, v].astype(np.float64)
    u = [(R[:, 0, k] * uv[0] + R[:, 1, k] * uv[1]) + R[:, 2, k] * uv[2] for k in range(3)]
    c2 = dist.astype(np.float64) * dist.astype(np.float64)
    return dict(b=b, v=v, pix=i * W + j, o=o, T=_moment_terms(u, d, kmom), c2=c2.reshape(B, V, H * W), dist=dist, owner=owner,
                shape=(B, V, H, W), kmom=kmom)


def render_rows(observed, c32, radii, view32, p2m, fg_max=FG_MAX, background=BACKGROUND, max_resid=MAX_RESID):
    """shr_sphere_render_normal's rows GIVEN the entry's inputs.  depth and owner by sphere_render_icp_ref.render32 (fp32, the
    header's rule); e = (double)D - (double)O', the cost term min(|e|, max_resid)^2; for a pixel with a row, from the fp32
    values: dx = xg - x, dy = yg - y, s = sqrt((r r - dx dx) - dy dy), grad = (-dx / s, -dy / s, 1),
    u_k = -((R_0k grad_0 + R_1k grad_1) + R_2k), all fp64.  -> icp_rows' dict with depth in place of dist."""
    obs = np.asarray(observed, np.float32)
    c32 = np.asarray(c32, np.float32)[..., :3]
    radii = np.asarray(radii, np.float32)
    B, V, H, W = obs.shape
    depth, owner = rref.render32(c32, radii, p2m, W, H, background)
    target, valid = rref.target32(obs, fg_max, background)
    px, py = sref.grid32(p2m, W, H)
    cap = np.float64(np.float32(max_resid))
    with np.errstate(invalid="ignore", over="ignore"):
        e = depth.astype(np.float64) - target.astype(np.float64)
        ae = np.abs(e)
        cl = np.where(ae < cap, ae, cap)
        c2 = np.where(valid, cl * cl, 0.0)
        keep = valid & (owner >= 0) & (ae < cap)
        b, v, i, j = np.nonzero(keep)
        o = owner[b, v, i, j].astype(np.int64)
        c, rr = c32[b, v, o].astype(np.float64), radii[o].astype(np.float64)
        dx, dy = px[j].astype(np.float64) - c[:, 0], py[i].astype(np.float64) - c[:, 1]
        s = np.sqrt((rr * rr - dx * dx) - dy * dy)
        live = (s > 0) & (s <= np.finfo(np.float64).max)
    b, v, i, j, o, dx, dy, s = (t[live] for t in (b, v, i, j, o, dx, dy, s))
    er = e[b, v, i, j]
    g0, g1 = -dx / s, -dy / s
    R = np.asarray(view32, np.float32)[b, v].astype(np.float64)
    u = [-((R[:, 0, k] * g0 + R[:, 1, k] * g1) + R[:, 2, k]) for k in range(3)]
    return dict(b=b, v=v, pix=i * W + j, o=o, T=_moment_terms(u, er, 12), c2=c2.reshape(B, V, H * W), depth=depth, owner=owner,
                shape=(B, V, H, W), kmom=12)


# ---- the dense sums and their bars --------------------------------------------------------------------------------------
def dense(rows, jac32, J, N=1):
    """name -> (value, bar) of every output of the entry, summed densely in fp64 from `rows`; bar None: exact.
    moments [B,J,kmom]: bar (n + 16) 2^-52 sum |terms|, n the sphere's rows.  A [B,26,26] = sum_j Jc_j^T S_j Jc_j: a term is
    Jc[k,a] u_k u_l Jc[l,c] of one row, n = 9 rows of the sample; g = -sum_j Jc_j^T h_j: n = 3 rows; C [B,26,J]: n = 3 rows of
    the sphere; gs [G,J] = -sum d: n = the sphere's rows in the group.  rows [B,J], count [B] and R [G,J,J]: exact.  cost [B]:
    within 1e-15 of the exactly rounded sum (math.fsum) of the pixels' cost terms."""
    B, kmom = rows["shape"][0], rows["kmom"]
    idx = rows["b"] * J + rows["o"]
    T = rows["T"]
    mom = np.stack([np.bincount(idx, T[:, m], B * J) for m in range(kmom)], -1).reshape(B, J, kmom)
    amom = np.stack([np.bincount(idx, np.abs(T[:, m]), B * J) for m in range(kmom)], -1).reshape(B, J, kmom)
    nrow = mom[..., 10]
    count = nrow.sum(1)
    Jc = np.asarray(jac32, np.float32).astype(np.float64).reshape(B, J, 3, 26)
    aJ = np.abs(Jc)
    out = dict(moments=(mom, (nrow[..., None] + SLACK) * EPS * amom), rows=(nrow, None), count=(count, None))
    A = np.einsum("bjka,bjkl,bjlc->bac", Jc, mom[..., SYM], Jc)
    aA = np.einsum("bjka,bjkl,bjlc->bac", aJ, amom[..., SYM], aJ)
    out["A"] = (A, (9 * count[:, None, None] + SLACK) * EPS * aA)
    g = -np.einsum("bjka,bjk->ba", Jc, mom[..., 6:9])
    out["g"] = (g, (3 * count[:, None] + SLACK) * EPS * np.einsum("bjka,bjk->ba", aJ, amom[..., 6:9]))
    cost = np.array([math.fsum(rows["c2"][b].ravel().tolist()) for b in range(B)])
    out["cost"] = (cost, 1e-15 * np.abs(cost))
    if kmom > 12:
        G = B // N
        C = np.einsum("bjka,bjk->baj", Jc, mom[..., 12:15])
        out["C"] = (C, (3 * nrow[:, None, :] + SLACK) * EPS * np.einsum("bjka,bjk->baj", aJ, amom[..., 12:15]))
        grows = nrow.reshape(G, N, J).sum(1)
        Rm = np.zeros((G, J, J))
        Rm[:, np.arange(J), np.arange(J)] = grows
        out["R"] = (Rm, None)
        out["gs"] = (-mom[..., 15].reshape(G, N, J).sum(1), (grows + SLACK) * EPS * amom[..., 15].reshape(G, N, J).sum(1))
    return out


def ratios(got, want):
    """name -> the largest error / bar of `got` (name -> array) against dense()'s dict; an exact quantity gives 0 or inf."""
    out = {}
    for name, (val, bar) in want.items():
        x = np.asarray(got[name], np.float64)
        assert x.shape == val.shape, (name, x.shape, val.shape)
        if bar is None:
            out[name] = 0.0 if np.array_equal(x, val) else np.inf
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(x - val)
            r = np.where(err == 0, 0.0, err / bar)
        out[name] = float(np.where(np.isnan(r), np.inf, r).max()) if r.size else 0.0
    return out


def flagged(r):
    return sorted(name for name, x in r.items() if not x <= 1.0)


# ---- the sums the way the kernels partition them ------------------------------------------------------------------------
WRONG = ("last_pixel", "tile2_first_pixel", "entry_256", "last_sphere", "last_record", "record_stride", "cost_low",
         "stale_lane")


def _two_sum(hi, lo, x):
    t = hi + x
    bb = t - hi
    return t, lo + ((hi - (t - bb)) + (x - bb))


def partitioned(rows, jac32, J, N=1, wrong=None):
    """name -> array: sphere_icp_scan.h's sums on `rows`.  Scan: per (sample, view, tile of 1024) four rounds of 256 pixels;
    the pixels with a row or a cost term are walked in ascending order; entry idx = t + 256 e of the [J x kmom] record is a
    chain of its own from 0; the cost a compensated chain (hi, lo).  Assembly: the V x tiles records of a sample added from 0,
    tiles ascending in a view, views ascending; the records' hi two-summed, lo collecting; A's lower triangle and g from the
    moments, spheres ascending, a sphere without a row skipped; C, R and gs as shr_sphere_icp_radii_normal words them.
    wrong, one of WRONG, a deliberately wrong variant the comparator has to flag:
      last_pixel         the scan stops one pixel short of the image
      tile2_first_pixel  the first pixel of every view's second tile is not read
      entry_256          the chain of moment entry 256 takes nothing
      last_sphere        the assembly of A, g (and C) stops at sphere J - 2
      last_record        the assembly adds one record too few
      record_stride      the last record is read at the stride of J - 1 spheres
      cost_low           cost = hi, without the compensation
      stale_lane         in the image's last, partial round a lane past the image's end adds the record it left in the
                         round before"""
    assert wrong is None or wrong in WRONG
    B, V, H, W = rows["shape"]
    kmom, T = rows["kmom"], rows["T"]
    npix, nmom, stride = H * W, kmom * J, kmom * J + 4
    tiles = (npix + TILE - 1) // TILE
    row_of = np.full((B, V, npix), -1, np.int64)
    row_of[rows["b"], rows["v"], rows["pix"]] = np.arange(len(rows["b"]))
    part = np.zeros((B, V * tiles, stride))
    end = npix - 1 if wrong == "last_pixel" else npix
    for b in range(B):
        for v in range(V):
            ro, c2 = row_of[b, v], rows["c2"][b, v]
            for t in range(tiles):
                acc, hi, lo = np.zeros(nmom), 0.0, 0.0
                for r in range(TILE // ROUND):
                    i0 = t * TILE + r * ROUND
                    lanes = np.arange(i0, min(i0 + ROUND, end))
                    if wrong == "tile2_first_pixel" and t == 1:
                        lanes = lanes[lanes != TILE]
                    if wrong == "stale_lane" and r > 0 and i0 < npix < i0 + ROUND:
                        lanes = np.concatenate([lanes, np.arange(max(i0, npix), i0 + ROUND) - ROUND])
                    for i in lanes[(ro[lanes] >= 0) | (c2[lanes] != 0)]:
                        hi, lo = _two_sum(hi, lo, c2[i])
                        if ro[i] >= 0:
                            at = rows["o"][ro[i]] * kmom
                            acc[at:at + kmom] = acc[at:at + kmom] + T[ro[i]]
                            if wrong == "entry_256" and at <= 256 < at + kmom:
                                acc[256] = 0.0
                part[b, v * tiles + t, :nmom] = acc
                part[b, v * tiles + t, nmom], part[b, v * tiles + t, nmom + 1] = hi, lo
    records = V * tiles
    mom, cost = np.zeros((B, nmom)), np.zeros(B)
    for b in range(B):
        flat = part[b].ravel()
        hi, lo = 0.0, 0.0
        for t in range(records - 1 if wrong == "last_record" else records):
            at = t * (kmom * (J - 1) + 4 if wrong == "record_stride" and t == records - 1 else stride)
            mom[b] = mom[b] + flat[at:at + nmom]
            if wrong == "record_stride" and t == records - 1:
                at = t * stride
            hi, low = _two_sum(hi, 0.0, flat[at + nmom])
            lo = lo + (low + flat[at + nmom + 1])
        cost[b] = hi if wrong == "cost_low" else hi + lo
    mom = mom.reshape(B, J, kmom)
    Jc = np.asarray(jac32, np.float32).astype(np.float64).reshape(B, J, 3, 26)
    A, g, C = np.zeros((B, 26, 26)), np.zeros((B, 26)), np.zeros((B, 26, J))
    low = np.tril(np.ones((26, 26), bool))
    for b in range(B):
        acc, accg = np.zeros((26, 26)), np.zeros(26)
        for j in range(J - 1 if wrong == "last_sphere" else J):
            m, q = mom[b, j], Jc[b, j]
            if m[10] == 0.0:
                continue
            t = [(m[SYM[k, 0]] * q[0] + m[SYM[k, 1]] * q[1]) + m[SYM[k, 2]] * q[2] for k in range(3)]      # [26] over c
            acc = acc + ((q[0][:, None] * t[0][None] + q[1][:, None] * t[1][None]) + q[2][:, None] * t[2][None])
            accg = accg + ((q[0] * m[6] + q[1] * m[7]) + q[2] * m[8])
            if kmom > 12:
                C[b, :, j] = (q[0] * m[12] + q[1] * m[13]) + q[2] * m[14]
        A[b] = np.where(low, acc, acc.T)
        g[b] = -accg
    out = dict(moments=mom, rows=mom[..., 10], count=mom[..., 10].sum(1), A=A, g=g, cost=cost)
    if kmom > 12:
        G = B // N
        grows, sd = np.zeros((G, J)), np.zeros((G, J))
        for b in range(B):
            grows[b // N], sd[b // N] = grows[b // N] + mom[b, :, 10], sd[b // N] + mom[b, :, 15]
        R = np.zeros((G, J, J))
        R[:, np.arange(J), np.arange(J)] = grows
        out.update(C=C, R=R, gs=0.0 - sd)
    return out


def constant_cost_rows(W=128, H=72, value=0.1):
    """(rows, jac32) of one sample, one view, one sphere without a row, every pixel at the distance fp32(value): nine full
    tiles of one and the same cost term, whose plain chain drifts the same way at every step."""
    c2 = float(np.float32(value)) ** 2
    rows = dict(b=np.zeros(0, np.int64), v=np.zeros(0, np.int64), pix=np.zeros(0, np.int64), o=np.zeros(0, np.int64),
                T=np.zeros((0, 12)), c2=np.full((1, 1, H * W), c2), shape=(1, 1, H, W), kmom=12)
    return rows, np.zeros((1, 3, 26), np.float32)


# ---- the per-frame terms and the Jacobian at the ends of J --------------------------------------------------------------
FRAME_J = (1, 22, 64)


def frame_case(mesh, J, B=4):
    """A random table of J spheres (seed 500 + J) and B poses: the start of pose_icp_ref.poses(1, 500 + J) with N(0, 0.03)
    on every parameter per frame, so that consecutive frames lie millimetres apart -- the frames of one sequence."""
    tab = table(J, 500 + J)
    model = sref.Spheres(mesh, tab, True)
    _, p0 = ref.poses(1, 500 + J)
    gen = torch.Generator().manual_seed(500 + J)
    p = (p0 + 0.03 * torch.randn(B, 26, generator=gen, dtype=torch.float64)).float().double()
    return dict(name="frames_J%d" % J, model=model, J=J, params0=p, view=sref.identity_views(B, 1),
                observed=np.full((B, 1, 1, 1), BACKGROUND, np.float32), stiffness=torch.ones(26, dtype=torch.float64))


def jacobian_deviation(case):
    """The largest |fp32 CPU chain's Jacobian - the fp64 chain's| at the case's poses (mm / rad | mm / mm), and the largest
    entry."""
    m = case["model"]
    j64 = m.chain.jacobian(case["params0"])[1]
    j32 = m.to(torch.float32).chain.jacobian(case["params0"].float())[1]
    return (j32.double() - j64).abs().max().item(), j64.abs().max().item()


def all_pairs(radii):
    """(a, b, m) of every pair a < b of the table, m = fp32(3 (r_a + r_b)): J (J - 1) / 2 pairs, about a quarter of them active
    on frame_case's poses."""
    J = len(radii)
    a, b = np.triu_indices(J, 1)
    r = np.asarray(radii, np.float64)
    return a.astype(np.int32), b.astype(np.int32), (3.0 * (r[a] + r[b])).astype(np.float32)
