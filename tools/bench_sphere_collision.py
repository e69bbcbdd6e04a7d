"""The collision term of the sphere fit (shr_sphere_collision_normal, sphere_collision.hip), HIP events on the launching
stream, through the C ABI (no Python op in the loop).  One iteration of the fit at the start poses, its seven launches timed
one by one:
  jacobian   shr_pose_keypoints_jacobian of the trial poses: the 41 centres and their 123 x 26 Jacobian
  views      shr_view_vertices_fwd with NV := 41: the centres in the view's frame
  normal     shr_sphere_icp_normal: the data-to-model term
  render     shr_sphere_render_normal with accumulate = 1 on top of it, the module's defaults
  prior      shr_sphere_prior_normal with accumulate = 1 on top of both, the module's defaults
  collision  shr_sphere_collision_normal with accumulate = 1 on top of the three (the NEW entry), the module's table: the
             reference's 690 pairs at 6 mm
  step       shr_pose_lm_step with the solve: the new entry and the prior entry have its launch shape (one workgroup per
             sample), so the three are reported side by side
and the new entry under two other tables: `radius` (m = min(r_a + r_b, rest distance): tens of active pairs per sample) and
`all` (m = 1000 mm: every one of the 690 pairs active, the collapsed hand's worst case).  One iteration with the term is the
sum of the seven; with it off the loop issues no launch of the entry and is the sum of the other six.
For 256 samples at 128 x 128 with one view (the term reads the model frame: it does not see the views), the hand's 41
spheres, observations rendered from the SPHERE model by the sphere rasterizer at sampled poses, keypoints the true centres
+ N(0, 2 mm), starts p* + N(0, 0.1) rad / N(0, 2 mm); in the same process, alternated, three rounds (every round is printed;
the summary is the median).  First measurements: no target is set.  Before anything is timed the whole loop runs once with
the term and without, and their keypoint errors and 6 mm penetrations are printed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import SphereCollisionPoseFitter  # noqa: E402
from tools.bench_sphere_icp import VIEWS  # noqa: E402

ROUNDS = 3
ITERS = 10
SIGMA_K = 2.0


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = torch.cuda.Stream()
    B, S, V = 256, 128, 1
    with torch.cuda.stream(stream):
        stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
        fit = SphereCollisionPoseFitter(mesh, S, S, iters=ITERS, stiffness=stiffness).cuda()
        off, inv, bone, wv, radii = fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv, fit.radii
        J = fit.num_spheres
        gen = torch.Generator().manual_seed(B)
        truth = sample_poses_batched(B, generator=gen)
        truth[:, 3:5] = 5.0 * torch.randn(B, 2, generator=gen)
        truth[:, 5] = 50.0
        start = truth + 0.1 * torch.randn(B, 26, generator=gen)
        start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
        noise = SIGMA_K * torch.randn(B, V, J, 3, generator=gen)
        truth, start = truth.float().cuda(), start.float().cuda()
        view = torch.stack(VIEWS[:V]).cuda().expand(B, V, 4, 4).contiguous()
        kp, _ = ops.pose_keypoints_jacobian(truth, off, inv, bone, wv, True)
        spheres = ops.view_vertices(kp, view).clone()
        targets = (spheres[..., :3] + noise.cuda()).contiguous()
        spheres[..., 3] = radii
        observed = torch.clamp(ops.sphere_raster_fwd(spheres.view(B * V, J, 4).contiguous(), S, S), max=100.0).view(B, V, S, S).contiguous()
        tabs = {"collision": (fit.pair_a, fit.pair_b, fit.pair_min)}
        for name, kw in (("radius", dict(radius_scale=1.0)), ("all", dict(min_dist=1000.0))):
            tabs[name] = tuple(torch.from_numpy(t).cuda() for t in hand_model.collision_table(mesh, **kw))
        q, c0, c = fit.solve(observed, start, view, keypoints=targets)
        off_fit = SphereCollisionPoseFitter(mesh, S, S, iters=ITERS, stiffness=stiffness, collision_weight=0.0).cuda()
        qo, _, _ = off_fit.solve(observed, start, view, keypoints=targets)
        err, pen = [], []
        for t in (start, qo, q, truth):
            err.append((ops.pose_keypoints_jacobian(t, off, inv, bone, wv, True)[0][..., :3] - kp[..., :3]).norm(dim=-1).mean(1))
            pen.append(ops.sphere_collision_normal(t, off, inv, bone, wv, True, tabs["collision"], 1.0)[3:])
        stream.synchronize()
        print("B=%d V=%d %dx%d, collision_weight %g at %g mm, sigma_k %g mm; %d iterations: cost <= cost0 on %d of %d; mean keypoint "
              "error %.2f mm at the start, %.2f with the term off, %.2f with it; 6 mm penetration per sample %.3f mm at the start, "
              "%.3f off, %.3f with it, %.3f at p*; samples with an active pair %d, %d, %d, %d"
              % (B, V, S, S, fit.collision_weight, fit.min_dist, SIGMA_K, ITERS, int((c <= c0).sum()), B, err[0].mean().item(),
                 err[1].mean().item(), err[2].mean().item(), *[x[1].sum(1).mean().item() for x in pen],
                 *[int((x[0] > 0).sum()) for x in pen]), flush=True)
        ax, bx, ay, by = fit.pixel_to_model
        fg, md, mr, bg, w = fit.fg_max, fit.max_dist, fit.max_resid, fit.background, fit.render_weight
        kw, km, lw, cw = fit.kp_weight, fit.kp_max, fit.limit_weight, fit.collision_weight
        lo, hi = fit.lower, fit.upper
        keypoints, jac = torch.empty(B, J, 4, device="cuda"), torch.empty(B, 3 * J, 26, device="cuda")
        centres = torch.empty(B, V, J, 4, device="cuda")
        A = torch.empty(B, 26, 26, dtype=torch.float64, device="cuda")
        g, cost = torch.empty(B, 26, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
        count, rows = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        prior_rows = torch.empty(B, 2, dtype=torch.int32, device="cuda")
        pair_rows = {k: torch.empty(B, dtype=torch.int32, device="cuda") for k in tabs}
        ws = torch.empty(max(16, lib.shr_sphere_render_normal_workspace_bytes(B, V, J, S, S)), dtype=torch.uint8, device="cuda")
        state, trial = ops.pose_lm_begin(start, 1e-3)
        nxt, par, cst, cst0 = (torch.empty(B, 26, device="cuda"), torch.empty(B, 26, device="cuda"), torch.empty(B, device="cuda"),
                               torch.empty(B, device="cuda"))
        mu = fit.stiffness

        def jacobian(s):
            return lib.shr_pose_keypoints_jacobian(p(trial), B, p(off), p(inv), J, p(bone), p(wv), 1, p(keypoints), p(jac), s)

        def views(s):
            return lib.shr_view_vertices_fwd(p(keypoints), p(view), B, V, J, p(centres), s)

        def normal(s):
            return lib.shr_sphere_icp_normal(p(observed), p(centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by, fg, md,
                                             p(A), p(g), p(cost), p(count), None, None, None, p(ws), s)

        def render(s):
            return lib.shr_sphere_render_normal(p(observed), p(centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by,
                                                fg, bg, mr, w, 1, p(A), p(g), p(cost), p(rows), None, None, None, p(ws), s)

        def prior(s):
            return lib.shr_sphere_prior_normal(p(centres), p(view), p(jac), p(trial), p(targets), None, kw, km, p(lo), p(hi), lw, B, V,
                                               J, 1, p(A), p(g), p(cost), p(prior_rows), None, None, s)

        def collision_of(name):
            a, b, m = tabs[name]
            return lambda s: lib.shr_sphere_collision_normal(p(keypoints), p(jac), p(a), p(b), p(m), cw, B, J, a.shape[0], 1, p(A),
                                                             p(g), p(cost), p(pair_rows[name]), None, None, s)

        def step(s):
            return lib.shr_pose_lm_step(p(state), p(A), p(g), p(cost), p(trial), None, p(mu), 1, B, p(nxt), p(par), p(cst), p(cst0), s)

        # (the accumulating entries add to A, g and cost on every call: the timed repetitions let them grow, which costs the same)
        runs = {"jacobian": jacobian, "views": views, "normal": normal, "render": render, "prior": prior,
                "collision": collision_of("collision"), "radius": collision_of("radius"), "all": collision_of("all"), "step": step}
        for label, fn in runs.items():
            assert fn(stream.cuda_stream) == 0, label
        stream.synchronize()
        print("  pairs with rows per sample at the start: %.2f at 6 mm, %.1f under `radius`, %.0f under `all`"
              % tuple(pair_rows[k].float().mean().item() for k in ("collision", "radius", "all")), flush=True)
        us = {k: [] for k in runs}
        for rnd in range(ROUNDS):
            for label, fn in runs.items():
                if label == "all" and rnd > 0:
                    continue                                     # the worst case is timed once
                if label == "step":
                    assert normal(stream.cuda_stream) == 0       # (a finite A, g and cost for the solve)
                us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
            print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
        us = {k: float(np.median(v)) for k, v in us.items()}
        total = sum(us[k] for k in ("jacobian", "views", "normal", "render", "prior", "collision", "step"))
        print("sphere collision B=%d V=%d %dx%d: jacobian %.2f us, views %.2f us, normal %.2f us, render %.2f us, prior %.2f us, "
              "collision %.2f us (`radius` %.2f us; `all`, once, %.2f us) beside step %.2f us; one iteration %.2f us (%.2f us with "
              "the term off)" % (B, V, S, S, us["jacobian"], us["views"], us["normal"], us["render"], us["prior"], us["collision"],
                                 us["radius"], us["all"], us["step"], total, total - us["collision"]), flush=True)
    return dict(us, total=total)


if __name__ == "__main__":
    main()
