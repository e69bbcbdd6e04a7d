"""A restatement of the model-to-data term of the sphere fit (spherehand_amd/csrc/sphere_render_icp.hip;
include/spherehand_hip.h, the section of shr_sphere_render_normal), on top of tests/sphere_icp_ref.py's sphere model,
tests/pose_ik_ref.py's chain and tests/pose_icp_ref.py's LM, none of which it changes (test helper; not a conftest):

    render32       the render and its owner in numpy fp32, word for word (the rasterizer's operation sequence and owner rule)
    pixels         the pixels that give a row, and every pixel's cost term, under the header's rules
    residuals      e = c.z - sqrt(r^2 - rho^2) - O' of the held pixels at pose p, the OWNER HELD, differentiable in p
    rows           its derivative by forward-mode autograd through pose_ik_ref.Chain and the view transform: nothing about
                   R^T is stated
    directions     u = -d e / d c_j in the MODEL frame, by autograd through the view transform
    normal         A, g, cost, count and the per-sphere moments of the term alone, unweighted
    solve          the loop of ops.sphere_icp_render with pose_icp_ref.LM: sphere_icp_ref.normal + weight x normal
    render64       the observation the sphere model itself explains under the RASTERIZER's hit rule, fp64 inside
    cases          the inputs of the GPU tests: sphere_icp_ref's, and one odd shape
    study          d2m alone against d2m + render on DESIGN.md 4.4p's 20 poses and on the family the d2m term is blind to

dtype is the chain's, as in sphere_icp_ref: fp32 rounds the transforms, the centres, the view transform and the Jacobian as
the kernels do; e is the contract's either way (the fp32 render against the fp32 observation, subtracted in fp64), and every
sum is fp64."""
import numpy as np
import torch

import pose_icp_ref as ref
import pose_icp_views_ref as vref
import pose_ik_ref  # noqa: F401  (the chain under sphere_icp_ref.Spheres)
import sphere_icp_ref as sref

FG_MAX, BACKGROUND = sref.FG_MAX, sref.BACKGROUND
HIT_MIN = np.float32(0.01)
MOMENTS = sref.MOMENTS
DEFAULT_WEIGHT, DEFAULT_MAX_RESID = 1.0, 10.0      # render.SphereRenderPoseFitter's: the best row of study()


def render32(centres, radii, p2m, W, H, background=BACKGROUND):
    """(depth [B,V,H,W] fp32, owner [B,V,H,W] int32): the header's rule in numpy fp32.  D = background, owner = -1,
    behind = True; for k ascending: dx = xg - x, dy = yg - y, q = (r r - dx dx) - dy dy, a hit iff q > 0.01f, then
    d = z - sqrt(q); taken iff d < D, or d == D with no owner yet and every lower sphere a hit strictly behind the
    background."""
    c, r = np.asarray(centres, np.float32), np.asarray(radii, np.float32)
    B, V = c.shape[:2]
    px, py = sref.grid32(p2m, W, H)
    px, py = px[None, None, None, :], py[None, None, :, None]
    bg = np.float32(background)
    depth = np.full((B, V, H, W), bg, np.float32)
    owner = np.full((B, V, H, W), -1, np.int32)
    behind = np.ones((B, V, H, W), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(c.shape[2]):
            dx, dy = px - c[:, :, k, 0, None, None], py - c[:, :, k, 1, None, None]
            q = (r[k] * r[k] - dx * dx) - dy * dy
            hit = q > HIT_MIN
            d = c[:, :, k, 2, None, None] - np.sqrt(np.where(hit, q, np.float32(1)))
            take = hit & ((d < depth) | ((owner < 0) & behind & (d == depth)))
            depth, owner = np.where(take, d, depth).astype(np.float32), np.where(take, np.int32(k), owner)
            behind = behind & hit & (d > bg)
    return depth, owner


def target32(observed, fg_max=FG_MAX, background=BACKGROUND):
    """(O' fp32, valid): the observation with its background set to `background`; a NaN pixel is not valid."""
    obs = np.asarray(observed, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(obs < np.float32(fg_max), obs, np.float32(background)).astype(np.float32), ~np.isnan(obs)


def residual_map(observed, depth, fg_max=FG_MAX, background=BACKGROUND):
    """e [B,V,H,W] fp64 = (double)D - (double)O', NaN where the observation is a NaN."""
    target, valid = target32(observed, fg_max, background)
    return np.where(valid, np.asarray(depth, np.float32).astype(np.float64) - target.astype(np.float64), np.nan)


def cost_terms(observed, depth, fg_max=FG_MAX, background=BACKGROUND, max_resid=np.inf):
    """[B,V,H,W] fp64: min(|e|, (double)(float)max_resid)^2, 0 where the observation is a NaN."""
    e = residual_map(observed, depth, fg_max, background)
    cl = np.minimum(np.abs(np.nan_to_num(e, nan=0.0)), np.float64(np.float32(max_resid)))
    return cl * cl


def pixels(observed, centres32, radii, depth, owner, p2m, fg_max=FG_MAX, background=BACKGROUND, max_resid=np.inf):
    """The rows' pixels: (sample b [N], view v [N], grid point xy [N,2] fp64, owner [N], e [N] fp64, target O' [N] fp64).
    A pixel with an owner and |e| < max_resid whose s = sqrt((r r - dx dx) - dy dy), recomputed in fp64 from the fp32
    values, is finite and > 0."""
    c, r = np.asarray(centres32, np.float32), np.asarray(radii, np.float32)
    B, V, H, W = np.asarray(depth).shape
    px, py = sref.grid32(p2m, W, H)
    own = np.asarray(owner, np.int64)
    e = residual_map(observed, depth, fg_max, background)
    target, _ = target32(observed, fg_max, background)
    with np.errstate(invalid="ignore"):
        keep = (own >= 0) & (own < c.shape[2]) & (np.abs(e) < np.float64(np.float32(max_resid)))
    b, v, i, j = np.nonzero(keep)
    o = own[b, v, i, j]
    xy = np.stack([px[j], py[i]], -1).astype(np.float64)
    cc, rr = c[b, v, o].astype(np.float64), r[o].astype(np.float64)
    dx, dy = xy[:, 0] - cc[:, 0], xy[:, 1] - cc[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sqrt((rr * rr - dx * dx) - dy * dy)
        live = np.isfinite(s) & (s > 0)
    return b[live], v[live], xy[live], o[live], e[b, v, i, j][live], target[b, v, i, j][live].astype(np.float64)


def residuals(model, view, p, pts):
    """e [N] fp64 of the held pixels at pose p (differentiable in p), the owner held: c.z - sqrt(r^2 - rho^2) - O' with
    c = R c_owner(p) + t, the chain in model.dtype."""
    b, v, xy, o, _, target = pts
    c = model.view_centres(p, view)[torch.as_tensor(b), torch.as_tensor(v), torch.as_tensor(o)].double()
    r = torch.as_tensor(model.radii.astype(np.float64))[torch.as_tensor(o)]
    xy = torch.as_tensor(xy)
    rho2 = (xy[:, 0] - c[:, 0]) ** 2 + (xy[:, 1] - c[:, 1]) ** 2
    return c[:, 2] - torch.sqrt(r * r - rho2) - torch.as_tensor(target)


def rows(model, view, p, pts):
    """(e [N] of the chain, J [N,26]) fp64: row i = d e_i / d params of its sample, by forward-mode autograd."""
    p = p.detach().to(model.dtype)
    basis = torch.eye(26, dtype=model.dtype)

    def column(t):
        return torch.func.jvp(lambda q: residuals(model, view, q, pts), (p,), (t.expand_as(p),))

    e, J = torch.func.vmap(column, out_dims=(None, 1))(basis)
    return e.detach(), J.detach()


def directions(model, view, p, pts):
    """u [N,3] fp64 in the MODEL frame: minus the derivative of e with respect to the owner's model-frame centre."""
    b, v, xy, o, _, _ = pts
    if len(b) == 0:
        return torch.zeros(0, 3, dtype=torch.float64)
    k = model.centres(p.to(model.dtype)).detach().double()[torch.as_tensor(b), torch.as_tensor(o)].clone().requires_grad_(True)
    M = torch.as_tensor(view).double()[torch.as_tensor(b), torch.as_tensor(v)]
    cv = torch.matmul(M[:, :3, :3], k.unsqueeze(-1)).squeeze(-1) + M[:, :3, 3]
    r = torch.as_tensor(model.radii.astype(np.float64))[torch.as_tensor(o)]
    xy = torch.as_tensor(xy)
    D = cv[:, 2] - torch.sqrt(r * r - ((xy[:, 0] - cv[:, 0]) ** 2 + (xy[:, 1] - cv[:, 1]) ** 2))
    return -torch.autograd.grad(D.sum(), k)[0]


def normal(model, view, observed, p, p2m, owner=None, depth=None, centres32=None, fg_max=FG_MAX, background=BACKGROUND,
           max_resid=np.inf, chain_residual=False):
    """dict of A [B,26,26], g [B,26], cost [B], count [B], moments [B,J,12] (fp64; count int64), depth, owner, pixels of the
    term alone, unweighted, at pose p.  owner, depth: the kernel's own maps, or None: the numpy rule on the model's
    centres32 (or on `centres32`, the kernel's).  e is the contract's, the fp32 render against the fp32 observation;
    chain_residual: the chain's own value of the residual function instead, whose gradient g then is."""
    B, J = p.shape[0], model.J
    view = torch.as_tensor(view)
    c32 = model.centres32(p, view) if centres32 is None else np.asarray(centres32, np.float32)[..., :3]
    H, W = np.asarray(observed).shape[2:]
    if owner is None:
        depth, owner = render32(c32, model.radii, p2m, W, H, background)
    pts = pixels(observed, c32, model.radii, depth, owner, p2m, fg_max, background, max_resid)
    A, g = torch.zeros(B, 26, 26, dtype=torch.float64), torch.zeros(B, 26, dtype=torch.float64)
    count = torch.zeros(B, dtype=torch.int64)
    moments = torch.zeros(B * J, MOMENTS, dtype=torch.float64)
    if len(pts[0]):
        e_chain, Jr = rows(model, view, p, pts)
        e = e_chain.double() if chain_residual else torch.as_tensor(pts[4])
        b, o = torch.as_tensor(pts[0]), torch.as_tensor(pts[3])
        A.index_add_(0, b, Jr[:, :, None] * Jr[:, None, :])
        g.index_add_(0, b, e[:, None] * Jr)
        count.index_add_(0, b, torch.ones_like(b))
        u = directions(model, view, p, pts)
        terms = torch.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2],
                             u[:, 2] * u[:, 2], e * u[:, 0], e * u[:, 1], e * u[:, 2], e * e, torch.ones_like(e),
                             torch.zeros_like(e)], -1)
        moments.index_add_(0, b * J + o, terms)
    cost = torch.as_tensor(cost_terms(observed, depth, fg_max, background, max_resid)).sum((1, 2, 3))
    return dict(A=A, g=g, cost=cost, count=count, moments=moments.view(B, J, MOMENTS), depth=depth, owner=owner, pixels=pts)


def combined(model, view, observed, p, p2m, weight, max_resid=np.inf, background=BACKGROUND, fg_max=FG_MAX,
             max_dist=sref.MAX_DIST):
    """(A, g, cost) of sum dist^2 + weight x the render term at pose p: sphere_icp_ref.normal + weight x normal, in the
    entry's arithmetic (one product and one sum per entry)."""
    d = sref.normal(model, view, observed, p, p2m, fg_max=fg_max, max_dist=max_dist)
    if not weight > 0:
        return d["A"], d["g"], d["cost"]
    w = float(np.float32(weight))
    r = normal(model, view, observed, p, p2m, fg_max=fg_max, background=background, max_resid=max_resid)
    return d["A"] + w * r["A"], d["g"] + w * r["g"], d["cost"] + w * r["cost"]


def solve(model, view, observed, params0, p2m, weight, max_resid=np.inf, iters=10, lambda0=1e-3, stiffness=None, prior=None,
          background=BACKGROUND, fg_max=FG_MAX, max_dist=sref.MAX_DIST):
    """The loop of ops.sphere_icp_render in model.dtype -> (params, cost0, cost, lm): iters + 1 evaluations, the last
    without a solve."""
    start = params0.float().double() if model.dtype == torch.float32 else params0.double()
    lm = ref.LM(start, lambda0, model.dtype)
    trial = lm.trial
    for it in range(iters + 1):
        A, g, cost = combined(model, view, observed, trial, p2m, weight, max_resid, background, fg_max, max_dist)
        out = lm.step(A, g, cost, trial, prior, stiffness, solve=it < iters)
        trial = out if out is not None else trial
    return lm.p, lm.cost0, lm.cost, lm


def render64(model, view, p, W, H, p2m=None, background=BACKGROUND):
    """[B,V,H,W] fp32: the sphere model's front surface at pose p under the RASTERIZER's hit rule (q > 0.01), fp64 inside,
    rounded once: what the fp32 render of the same pose gives up to its own rounding."""
    p2m = ref.grid(W, H) if p2m is None else p2m
    c = model.to(torch.float64).centres32(p.double(), view).astype(np.float64)
    px, py = sref.grid32(p2m, W, H)
    x, y = px.astype(np.float64)[None, None, None, :], py.astype(np.float64)[None, None, :, None]
    out = np.full(c.shape[:2] + (H, W), float(background), np.float64)
    for k in range(model.J):
        r = float(model.radii[k])
        q = (r * r - (x - c[:, :, k, 0, None, None]) ** 2) - (y - c[:, :, k, 1, None, None]) ** 2
        z = c[:, :, k, 2, None, None] - np.sqrt(np.maximum(q, 0.0))
        out = np.where(q > 0.01, np.minimum(out, z), out)
    return out.astype(np.float32)


def undecided_hits(model, view, p, W, H, p2m, tol=1e-3):
    """[B,V,H,W] bool: the pixels at which some sphere's q, in fp64 on the fp32 centres, lies within `tol` of the hit
    threshold 0.01 -- the fp32 q (three roundings at r^2 <= 600: 1e-4) may decide the hit the other way there."""
    c = model.to(torch.float64).centres32(p.double(), view).astype(np.float64)
    px, py = sref.grid32(p2m, W, H)
    x, y = px.astype(np.float64)[None, None, None, :], py.astype(np.float64)[None, None, :, None]
    out = np.zeros(c.shape[:2] + (H, W), bool)
    for k in range(model.J):
        r = float(model.radii[k])
        q = (r * r - (x - c[:, :, k, 0, None, None]) ** 2) - (y - c[:, :, k, 1, None, None]) ** 2
        out |= np.abs(q - 0.01) < tol
    return out


def over_background(model, view, observed, p, p2m, fg_max=FG_MAX, background=BACKGROUND):
    """[B] int64: the model pixels of pose p that lie over observed background, all views."""
    H, W = np.asarray(observed).shape[2:]
    _, owner = render32(model.centres32(p, torch.as_tensor(view)), model.radii, p2m, W, H, background)
    with np.errstate(invalid="ignore"):
        return torch.as_tensor(((owner >= 0) & ~(np.asarray(observed, np.float32) < np.float32(fg_max))).sum((1, 2, 3)))


# ---- the GPU tests' inputs ----------------------------------------------------------------------------------------------
ODD_W, ODD_H = 33, 17


def odd_case(mesh):
    """The right hand at 33 x 17 (one partial tile, rows that are no multiple of anything), seed 24, B = 3, two views
    (identity, 90 degrees about x), sphere-rendered."""
    model = sref.Spheres(mesh, None, True)
    p, p0 = ref.poses(3, 24)
    view = vref.views(3, ("identity", "x"))
    return dict(name="odd", model=model, W=ODD_W, H=ODD_H, p2m=ref.grid(ODD_W, ODD_H), p_star=p, params0=p0, view=view,
                kinds=("identity", "x"), observed=sref.render(model, view, p, ODD_W, ODD_H),
                stiffness=torch.as_tensor(ref.STIFFNESS), iters=4)


_CACHE = {}


def cached_cases(mesh):
    """sphere_icp_ref.cases (right 32 x 32, left 48 x 40, end_to_end 48 x 40) and the odd shape, once per process."""
    if "cases" not in _CACHE:
        _CACHE["cases"] = list(sref.cached_cases(mesh)) + [odd_case(mesh)]
    return _CACHE["cases"]


def case(mesh, name):
    return [c for c in cached_cases(mesh) if c["name"] == name][0]


BLIND = 6          # sphere_icp_ref.synthetic_table's sphere on bone 12 (r = 7): the only one on its finger


def blind_case(mesh, centres32=None, B=3, W=32, H=32):
    """The case the data-to-model term is blind to, on sphere_icp_ref.synthetic_table in one identity view: the observation
    is the table's render at the pose WITHOUT sphere BLIND, and every observed point BLIND would still own under the
    data-to-model rule (where it cuts another sphere's surface) is set to background.  So no observed point is BLIND's,
    while BLIND's own pixels lie over observed background or in front of the observed surface.  centres32 [B,1,7,>=3]: the
    view-frame centres the observation is built on -- the kernel's own (the GPU test) or, by default, the fp32 chain's.
    `private`: the parameters that move BLIND and no other sphere (the columns of the chain's Jacobian that are zero on
    every other sphere)."""
    model = sref.Spheres(mesh, sref.synthetic_table(), True)
    p, _ = ref.poses(B, 23)
    p = p.float().double()
    view = sref.identity_views(B, 1)
    p2m = ref.grid(W, H)
    c32 = model.to(torch.float32).centres32(p, view) if centres32 is None else np.asarray(centres32, np.float32)[..., :3]
    without = model.radii.copy()
    without[BLIND] = 0.0                                       # q <= 0: never a hit
    observed, _ = render32(c32, without, p2m, W, H)
    _, own = sref.owner_dist32(observed, c32, model.radii, p2m)
    observed = np.where(own == BLIND, np.float32(BACKGROUND), observed).astype(np.float32)
    _, jac = model.chain.jacobian(p)
    Jc = jac.double().view(B, model.J, 3, 26)
    others = [j for j in range(model.J) if j != BLIND]
    private = ((Jc[:, others] == 0).all(0).all(0).all(0) & (Jc[:, BLIND] != 0).any(0).any(0)).nonzero().flatten()
    return dict(name="blind", model=model, W=W, H=H, p2m=p2m, params0=p, view=view, observed=observed, centres32=c32,
                private=private)


# ---- the study ----------------------------------------------------------------------------------------------------------
CURLED = (1.35, 1.45, 1.25)          # the flexes of the finger curled at p*: joint_angle's closed range
EXTENDED = (-0.1, -0.2, -0.17)       # and extended at the start: joint_angle's straight range
FINGER = 6                           # the index finger's parameters 6 .. 9 (abduction, three flexes)


def study_poses(family):
    """(p*, p0) [20,26]: DESIGN.md 4.4p's 20 poses (pose_icp_ref.poses(5, seed), seeds 21 .. 24) with its starts (`noise`), or
    the blind family (`blind`): p* with the index finger curled, the start p* with that finger extended and nothing else
    moved."""
    ps, p0s = zip(*(ref.poses(5, seed) for seed in (21, 22, 23, 24)))
    p, p0 = torch.cat(ps), torch.cat(p0s)
    if family == "blind":
        p = p.clone()
        p[:, FINGER + 1:FINGER + 4] = torch.tensor(CURLED, dtype=torch.float64)
        p0 = p.clone()
        p0[:, FINGER + 1:FINGER + 4] = torch.tensor(EXTENDED, dtype=torch.float64)
    return p, p0


def study(mesh, W=48, H=40, iters=10, weights=(0.0, 0.01, 0.1, 1.0, 3.0, 10.0), max_resids=(5.0, 10.0, 20.0, 50.0, np.inf),
          families=("noise", "blind"), view_sets=(("identity",), ("identity", "y", "x")), out=print):
    """The table of DESIGN.md 4.4q: per family, view set, render_weight and max_resid the mean (median) keypoint error, the
    median and worst cost0 / cost of the fit's own energy, and the model pixels over observed background before and
    after, over the 20 poses.  Observations: render64 of p*, the rasterizer's hit rule."""
    model = sref.Spheres(mesh, None, True)
    p2m = ref.grid(W, H)
    mu = torch.as_tensor(ref.STIFFNESS)
    rows_out = []
    for family in families:
        p, p0 = study_poses(family)
        for kinds in view_sets:
            view = vref.views(p.shape[0], kinds)
            obs = render64(model, view, p, W, H, p2m)
            start = sref.keypoint_error(model, p0, p)
            before = over_background(model, view, obs, p0.float().double(), p2m)
            out("%s, %d view(s): start keypoint error %.2f (median %.2f) mm, %.1f model pixels over background"
                % (family, len(kinds), start.mean(), start.median(), before.double().mean()))
            for w in weights:
                for mr in (max_resids if w > 0 else (np.inf,)):
                    q, c0, c, _ = solve(model, view, obs, p0, p2m, w, mr, iters, 1e-3, mu)
                    err = sref.keypoint_error(model, q, p)
                    after = over_background(model, view, obs, q, p2m)
                    ratio = c0 / c.clamp(min=1e-300)
                    row = dict(family=family, views=len(kinds), weight=w, max_resid=mr, mean=err.mean().item(),
                               median=err.median().item(), ratio_median=ratio.median().item(), ratio_worst=ratio.min().item(),
                               above7=int((err > 7).sum()), before=before.double().mean().item(),
                               after=after.double().mean().item())
                    rows_out.append(row)
                    out("  w %-5g max_resid %-4g: error %.2f (%.2f) mm, cost0/cost %.3g (worst %.3g), above 7 mm %d, "
                        "over background %.1f -> %.1f" % (w, mr, row["mean"], row["median"], row["ratio_median"],
                                                          row["ratio_worst"], row["above7"], row["before"], row["after"]))
    return rows_out


if __name__ == "__main__":
    from spherehand_amd import hand_model
    study(hand_model.load_mesh())
