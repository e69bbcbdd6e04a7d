#!/usr/bin/env python3
"""Edge-case golden vectors for the sphere path, by RUNNING the imported reference (PyTorch, CPU).

    python tests/golden/make_goldens_edges.py [--out DIR]

  tests/golden/g_edges_sphere.npz   BallRender + torch.min on scenes built to sit ON the rules: exact ties, a hit at
                                    exactly 100.0, the 0.01 clamp, radii <= 0, non-finite records, huge records;
                                    12 x 20, 10 x 14 and (a subset) 32 x 32 pixels
  tests/golden/g_edges_d2m.npz      DataToModelLoss on points at a centre / on a surface / on the clamp at 50 / at the
                                    99 threshold, non-finite pixels and centres; CollisionLoss on its hinge's kink

Reference entry points (file:line in /root/reference):
  mesh/render.py:10-53     BallRender
  mesh/render.py:89        torch.min over the part maps (HandBallPrimitiveRender.forward)
  mesh/render.py:93-142    DataToModelLoss
  mesh/render.py:145-176   CollisionLoss
torch.sqrt runs as the IEEE square root (make_goldens_sphere.ieee_sqrt).  The fixtures hold arrays and names only.

Pixel coordinates are formed as the reference forms them in fp32, ((u - W/2) * 300) / W, so a sphere or a point put
at px(u, W) sits on that pixel's centre exactly (dx == 0).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refimport import import_reference  # noqa: E402
from make_goldens_sphere import ieee_sqrt  # noqa: E402

F = np.float32
NAN, INF = float("nan"), float("inf")
SPHERE_SIZES = {"a": (12, 20), "b": (10, 14)}        # H, W; the second width is no multiple of four
# ... and a power-of-two image with rows of 32 pixels, the least the fused kernel's box variant takes: the scenes that
# reach its own tie / owner / general-path code
BOX_SIZE = (32, 32)
BOX_SCENES = ("dup_front", "dup_front_late", "mirror_tie", "mirror_tie_swapped", "hit100_lower_misses", "hit100_lower_deeper",
              "hit100_first", "hit100_twice", "centre_behind_background", "all_off_screen", "all_behind_covering",
              "all_behind_partial", "overhang_all_edges", "nan_x", "nan_z", "nan_r", "nan_z_twice", "inf_r", "minus_inf_z",
              "huge_x_r", "r_below_1e6")
D2M_SIZES = {"a": (8, 12), "b": (9, 14)}


def px(u, n):
    """Pixel-centre coordinate, the reference's three fp32 operations (mesh/render.py:31)."""
    return (F(u) - F(n / 2)) * F(300.0) / F(n)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def clamp_boundary_radii():
    """Radii r (dx = dy = 0, so q = fl(r*r)) with q exactly 0.01f, its upper and its lower fp32 neighbour, searched
    over the floats round 0.1.  None where no float squares to the value."""
    t = F(0.01)
    want = {"at": t, "above": up(t), "below": down(t)}
    out = dict.fromkeys(want)
    r = F(0.1)
    for _ in range(4000):
        r = down(r)
    for _ in range(8000):
        q = F(r * r)
        for k, v in want.items():
            if out[k] is None and q == v:
                out[k] = float(r)
        r = up(r)
    return out


def sphere_scenes(H, W):
    """[(name, [J,4] (x, y, z, r))] for one image size."""
    X = lambda u: float(px(u, W))
    Y = lambda v: float(px(v, H))
    uc, vc = W // 2, H // 2                       # X(uc) == Y(vc) == 0 exactly (both sizes are even)
    off = [1e4, 1e4, 0.0, 5.0]                    # off screen
    front = [X(2), Y(2), 20.0, 40.0]              # an ordinary sphere; misses pixel (W - 3, H - 3)
    tu, tv = W - 3, H - 3
    tie = [X(tu), Y(tv), 102.0, 2.0]              # covers one pixel, at 102 - sqrt(4) = exactly 100.0
    s = []
    s.append(("dup_front", [[X(uc), Y(vc), 10.0, 40.0], [X(uc), Y(vc), 10.0, 40.0], [X(uc - 1), Y(vc), 80.0, 60.0]]))
    s.append(("dup_front_late", [[X(uc - 1), Y(vc), 80.0, 60.0], [X(uc), Y(vc), 10.0, 40.0], [X(uc), Y(vc), 10.0, 40.0]]))
    s.append(("mirror_tie", [[-7.0, Y(vc), 20.0, 45.0], [7.0, Y(vc), 20.0, 45.0], [X(uc), Y(vc + 1), 70.0, 80.0]]))
    s.append(("mirror_tie_swapped", [[7.0, Y(vc), 20.0, 45.0], [X(uc), Y(vc + 1), 70.0, 80.0], [-7.0, Y(vc), 20.0, 45.0]]))
    s.append(("hit100_lower_misses", [front, tie, off]))
    s.append(("hit100_lower_deeper", [[X(tu), Y(tv), 105.0, 3.0], tie, front]))
    s.append(("hit100_first", [tie, front, off]))
    s.append(("hit100_twice", [[X(tu), Y(tv), 105.0, 3.0], tie, tie]))
    s.append(("centre_behind_background", [[X(uc), Y(vc), 120.0, 45.0], [X(2), Y(2), 130.0, 40.0], off]))
    cb = clamp_boundary_radii()
    for k in ("at", "above", "below"):
        if cb[k] is not None:
            s.append(("clamp_q_%s" % k, [[X(tu), Y(tv), 50.0, cb[k]], front, off]))
    s.append(("negative_radius", [[X(uc), Y(vc), 30.0, -40.0], [X(2), Y(2), 20.0, 40.0], [X(uc + 2), Y(vc), 25.0, -35.0]]))
    s.append(("zero_radius", [[X(uc), Y(vc), 30.0, 0.0], [X(2), Y(2), 20.0, 40.0], [X(uc + 2), Y(vc), 25.0, -0.0]]))
    s.append(("all_off_screen", [off, [-1e4, 300.0, 10.0, 30.0], [0.0, 5e3, -20.0, 100.0]]))
    s.append(("all_behind_covering", [[0.0, 0.0, 450.0, 300.0], [10.0, -5.0, 500.0, 350.0], [-20.0, 8.0, 480.0, 330.0]]))
    s.append(("all_behind_partial", [[X(uc), Y(vc), 150.0, 40.0], [X(2), Y(2), 200.0, 40.0], [X(uc + 1), Y(vc), 160.0, 45.0]]))
    s.append(("overhang_all_edges", [[0.0, 0.0, 50.0, 400.0], [10.0, -5.0, 80.0, 420.0], [X(uc), Y(vc), -380.0, 20.0]]))
    base = [[X(uc), Y(vc), 10.0, 40.0], [X(uc + 2), Y(vc - 1), 5.0, 35.0], [X(2), Y(2), 20.0, 40.0]]
    for name, col, val in (("nan_x", 0, NAN), ("nan_z", 2, NAN), ("nan_r", 3, NAN), ("inf_r", 3, INF),
                           ("inf_z", 2, INF), ("minus_inf_z", 2, -INF)):
        sc = [list(b) for b in base]
        sc[1][col] = val
        s.append((name, sc))
    # two NaN depths at one pixel: torch.min keeps the FIRST NaN's index, and sends it the gradient
    s.append(("nan_z_twice", [base[0][:2] + [NAN, 40.0], base[1][:2] + [NAN, 35.0], base[2]]))
    s.append(("nan_r_twice", [base[2], base[0][:3] + [NAN], base[1][:3] + [NAN]]))
    s.append(("huge_x_r", [[-2e6, 0.0, 2e6, 2e6 + 64.0], [X(uc), Y(vc), 10.0, 40.0], [2e6, 0.0, 2e6 - 30.0, -2e6 - 32.0]]))
    r_lim = float(down(1e6))
    s.append(("r_below_1e6", [[0.0, 0.0, r_lim + 20.0, r_lim], [X(uc), Y(vc), 30.0, 40.0], [X(2), Y(2), 1e6, -r_lim]]))
    return s


def sphere_scenes_j64(H, W):
    """dup_front with J = 64: the pair at indices 5 and 40, in front of 62 seeded spheres."""
    rs = np.random.RandomState(64)
    sp = np.concatenate([rs.uniform(-140, 140, (64, 2)), rs.uniform(40, 90, (64, 1)), rs.uniform(5, 40, (64, 1))], 1)
    sp = sp.astype(F)
    sp[5] = sp[40] = (px(W // 2, W), px(H // 2, H), 0.0, 45.0)
    return [("dup_front_j64", sp.tolist())]


# tests/test_oracle_sphere.py::test_nan_and_inf_semantics' three crops (16 x 16, J = 2)
RESTATED_CROPS = [("restated_nan_x", [[0, 0, 10, 20], [NAN, 0, 0, 5]]),
                  ("restated_nan_z", [[0, 0, NAN, 20], [50, 50, 0, 5]]),
                  ("restated_inf_x", [[INF, 0, 0, 20], [0, 0, 5, 30]])]


def run_sphere_group(torch, BallRender, scenes, H, W, seed):
    names = [n for n, _ in scenes]
    sp = np.asarray([a for _, a in scenes], F)                  # [N,J,4]
    N, J, _ = sp.shape
    rs = np.random.RandomState(seed)
    upstream = rs.standard_normal((N, H, W)).astype(F)
    target = np.where(rs.uniform(size=(N, H, W)) < 0.5, 100.0, rs.uniform(-60, 99, (N, H, W))).astype(F)
    br = BallRender(W, H)

    def render(c, r):
        part = br(c.view(-1, 3), r.view(-1)).view(N, J, H, W)
        return torch.min(part, dim=1)

    out = {"names": np.asarray(names), "hw": np.asarray([H, W]), "spheres": sp, "upstream": upstream, "target": target}
    with ieee_sqrt():
        c = torch.from_numpy(sp[..., :3].copy()).requires_grad_(True)
        r = torch.from_numpy(sp[..., 3].copy()).requires_grad_(True)
        depth, arg = render(c, r)
        (depth * torch.from_numpy(upstream)).sum().backward()
        out["depth"] = depth.detach().numpy()
        out["argmin"] = arg.numpy().astype(np.uint8)
        out["grad"] = np.concatenate([c.grad.numpy(), r.grad.numpy()[..., None]], -1)
        c = torch.from_numpy(sp[..., :3].copy()).requires_grad_(True)
        r = torch.from_numpy(sp[..., 3].copy()).requires_grad_(True)
        depth, _ = render(c, r)
        sse = ((depth - torch.from_numpy(target)) ** 2).sum(dim=(1, 2))
        sse.sum().backward()
        out["sse"] = sse.detach().numpy()
        out["sse_grad"] = np.concatenate([c.grad.numpy(), r.grad.numpy()[..., None]], -1)
    return out


def d2m_scenes(H, W):
    """[(name, depth [H,W], centres [3,3], radii [3])] for one image size: background 100 but for the named points."""
    X = lambda u: float(px(u, W))
    Y = lambda v: float(px(v, H))
    R = [10.0, 14.0, 8.0]
    u0, v0, z0 = 3, 2, 20.0
    c = [[X(u0), Y(v0), z0], [X(W - 3), Y(H - 3), -15.0], [X(1), Y(H - 2), 35.0]]      # sphere 0 on pixel (u0, v0)
    bg = lambda: np.full((H, W), 100.0, F)

    def one(z, u=u0, v=v0):
        d = bg()
        d[v, u] = z
        return d

    s = []
    s.append(("point_at_centre", one(z0), c, R))
    s.append(("point_on_surface", one(z0 - R[0]), c, R))
    on50 = F(z0 - R[0] - 50.0)
    s.append(("term_exactly_50", one(on50), c, R))
    s.append(("term_50_nearer", one(up(on50)), c, R))
    s.append(("term_50_farther", one(down(on50)), c, R))
    s.append(("depth_99", one(99.0), c, R))
    s.append(("depth_99_above", one(up(99.0)), c, R))
    s.append(("depth_99_below", one(down(99.0)), c, R))
    d = one(100.0)
    d[v0 + 1, u0 + 1] = up(100.0)
    s.append(("depth_100", d, c, R))
    s.append(("all_background", bg(), c, R))
    rs = np.random.RandomState(H * 100 + W)
    s.append(("all_foreground", rs.uniform(-60, 99, (H, W)).astype(F), c, R))
    d = one(z0 + 30.0)
    d[v0, u0 + 1] = z0 - 4.0
    s.append(("identical_spheres", d, [c[0], c[0], c[2]], [R[0], R[0], R[2]]))
    s.append(("identical_spheres_late", d, [c[2], c[0], c[0]], [R[2], R[0], R[0]]))
    d = one(z0 + 3.0)
    d[v0 + 1, u0] = z0 - 25.0
    s.append(("negative_radius", d, c, [-10.0, 14.0, -8.0]))
    gen = rs.uniform(-30, 60, (H, W)).astype(F)
    some = np.where(rs.uniform(size=(H, W)) < 0.4, gen, F(100.0)).astype(F)     # an ordinary crop round the bad record
    d = some.copy()
    d[v0, u0] = NAN
    s.append(("nan_depth_pixel", d, c, R))
    d = some.copy()
    d[v0, u0] = -INF
    s.append(("minus_inf_depth_pixel", d, c, R))
    for name, val in (("nan_centre", NAN), ("inf_centre", INF), ("minus_inf_centre", -INF)):
        cc = [list(a) for a in c]
        cc[1][1] = val
        s.append((name, some.copy(), cc, R))
    s.append(("farther_than_1km", one(-2000.0), c, R))
    s.append(("near_centre_above", one(F(z0) + F(6e-5)), c, R))
    s.append(("near_centre_below", one(F(z0) - F(6e-5)), c, R))
    return s


def run_d2m(torch, DataToModelLoss, scenes, H, W):
    out = {"names": np.asarray([n for n, *_ in scenes]), "hw": np.asarray([H, W]),
           "depth": np.asarray([d for _, d, _, _ in scenes], F), "centres": np.asarray([c for _, _, c, _ in scenes], F),
           "radii": np.asarray([r for _, _, _, r in scenes], F)}
    loss, grad = [], []
    for _, d, c, r in scenes:
        crit = DataToModelLoss(W, H, [float(x) for x in r])
        j = torch.from_numpy(np.asarray(c, F)[None]).requires_grad_(True)
        l = crit(torch.from_numpy(np.asarray(d, F)[None]), j)
        l.backward()
        loss.append(l.item())
        grad.append(j.grad.numpy()[0])
    out["loss"] = np.asarray(loss, np.float64)             # mean over the crop's H*W pixels
    out["grad"] = np.asarray(grad, F)                      # d loss / d joints
    return out


def run_collision(torch, CollisionLoss):
    """41 joints 100 mm apart, but joint 0 (palm) and joint 11 (a finger's first) exactly 6.0 apart along x -- the
    hinge argument min_dist^2 - |d|^2 is exactly 0 -- and one ulp nearer / farther."""
    base = np.zeros((41, 3), F)
    base[:, 1] = 100.0 * np.arange(41)
    base[0] = (0.0, -50.0, 7.0)
    names, joints = [], []
    for name, dxv in (("collision_at_6", F(6.0)), ("collision_nearer", down(6.0)), ("collision_farther", up(6.0))):
        j = base.copy()
        j[11] = (dxv, -50.0, 7.0)
        assert F(j[11, 0] - j[0, 0]) == dxv
        names.append(name)
        joints.append(j)
    joints = np.asarray(joints, F)
    crit = CollisionLoss()
    loss, grad = [], []
    for j in joints:
        t = torch.from_numpy(j[None].copy()).requires_grad_(True)
        l = crit(t)
        l.backward()
        loss.append(l.item())
        grad.append(t.grad.numpy()[0])
    return {"collision_names": np.asarray(names), "collision_joints": joints, "collision_loss": np.asarray(loss, np.float64),
            "collision_grad": np.asarray(grad, F), "collision_min_sq_dist": np.asarray(crit.min_sq_dist, np.float64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    out_dir = os.path.abspath(ap.parse_args().out)
    import_reference()
    import torch
    from mesh.render import BallRender, CollisionLoss, DataToModelLoss

    torch.set_num_threads(1)
    cb = clamp_boundary_radii()
    out = {"torch_version": np.asarray(torch.__version__),
           "clamp_q_found": np.asarray([cb[k] is not None for k in ("at", "above", "below")]),
           "clamp_q_radii": np.asarray([cb[k] if cb[k] is not None else NAN for k in ("at", "above", "below")], F)}
    groups = []
    for tag, (H, W) in SPHERE_SIZES.items():
        groups.append((tag + "3", sphere_scenes(H, W), H, W))
    H, W = SPHERE_SIZES["a"]
    groups.append(("a64", sphere_scenes_j64(H, W), H, W))
    groups.append(("r2", RESTATED_CROPS, 16, 16))
    H, W = BOX_SIZE
    groups.append(("c3", [sc for sc in sphere_scenes(H, W) if sc[0] in BOX_SCENES], H, W))
    for k, (tag, scenes, H, W) in enumerate(groups):
        for key, v in run_sphere_group(torch, BallRender, scenes, H, W, seed=100 + k).items():
            out["%s_%s" % (tag, key)] = v
    out["groups"] = np.asarray([g[0] for g in groups])
    out["scene_names"] = np.asarray(["%s/%s" % (g[0], n) for g in groups for n, _ in g[1]])
    np.savez_compressed(os.path.join(out_dir, "g_edges_sphere.npz"), **out)
    print("sphere scenes:", len(out["scene_names"]), "clamp boundary radii", cb)

    out = {"torch_version": np.asarray(torch.__version__), "groups": np.asarray(list(D2M_SIZES))}
    names = []
    with ieee_sqrt():
        for tag, (H, W) in D2M_SIZES.items():
            scenes = d2m_scenes(H, W)
            names += ["%s/%s" % (tag, n) for n, *_ in scenes]
            for key, v in run_d2m(torch, DataToModelLoss, scenes, H, W).items():
                out["%s_%s" % (tag, key)] = v
        out.update(run_collision(torch, CollisionLoss))
    out["scene_names"] = np.asarray(names + list(out["collision_names"]))
    np.savez_compressed(os.path.join(out_dir, "g_edges_d2m.npz"), **out)
    print("d2m scenes:", len(names), "done")


if __name__ == "__main__":
    main()
