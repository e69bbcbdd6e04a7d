"""Pose from observed depth points through the sphere model (shr_sphere_icp_normal, sphere_icp.hip), HIP events on the
launching stream, through the C ABI (no Python op in the loop).  One iteration of the fit at the start poses, its four launches
timed one by one:
  jacobian   shr_pose_keypoints_jacobian of the trial poses: the 41 centres and their 123 x 26 Jacobian
  views      shr_view_vertices_fwd with NV := 41: the centres in every view's frame
  normal     shr_sphere_icp_normal: owner search, residuals, per-sphere moments, A and g (the NEW entry)
  step       shr_pose_lm_step with the solve
and, to see where the new entry's time goes, the same entry on an all-background observation of the same shape (`empty`:
its launches, its reads of the depth and the assembly -- no data point, so no search and no sums) and on the real observation
with max_dist = 0 (`search`: every data point meets every sphere, but none gives a row and every distance is 0 -- no fp64
recomputation and no sums).
For 256 samples at 128 x 128 with one view and with three (identity, 90 degrees about y and about x through the palm), the
hand's 41 spheres, observations rendered from the SPHERE model by the sphere rasterizer at sampled poses, starts p* + N(0, 0.1)
rad / N(0, 2 mm); in the same process, alternated, three rounds (every round is printed; the summary is the median).  Then, for
scale, tools/bench_pose_icp.py's mesh iteration on its own inputs in the same run.  First measurements: no target is set.
The hand-derived floor of the new entry is its reads, B V H W 4 bytes of observed depth, at the HBM peak.  Before anything is
timed the whole loop (ops.sphere_icp, 10 iterations) runs once and its costs are printed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import SpherePoseFitter  # noqa: E402
from tools import bench_pose_icp  # noqa: E402

ROUNDS = 3
ITERS = 10
HBM_PEAK = 8.0e12      # bytes / s, MI355X


def about(R, depth=50.0):
    M = torch.eye(4)
    M[:3, :3] = torch.tensor(R)
    c = torch.tensor([0.0, 0.0, depth])
    M[:3, 3] = c - M[:3, :3] @ c
    return M


VIEWS = (torch.eye(4), about([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), about([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]))


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = torch.cuda.Stream()
    B, S = 256, 128
    sphere = {}
    with torch.cuda.stream(stream):
        for V in (1, 3):
            stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
            fit = SpherePoseFitter(mesh, S, S, iters=ITERS, stiffness=stiffness).cuda()
            off, inv, bone, wv, radii = fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv, fit.radii
            J = fit.num_spheres
            gen = torch.Generator().manual_seed(B)
            truth = sample_poses_batched(B, generator=gen)
            truth[:, 3:5] = 5.0 * torch.randn(B, 2, generator=gen)
            truth[:, 5] = 50.0
            start = truth + 0.1 * torch.randn(B, 26, generator=gen)
            start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
            truth, start = truth.float().cuda(), start.float().cuda()
            view = torch.stack(VIEWS[:V]).cuda().expand(B, V, 4, 4).contiguous()
            kp, _ = ops.pose_keypoints_jacobian(truth, off, inv, bone, wv, True)
            spheres = ops.view_vertices(kp, view).clone()
            spheres[..., 3] = radii
            observed = torch.clamp(ops.sphere_raster_fwd(spheres.view(B * V, J, 4).contiguous(), S, S), max=100.0).view(B, V, S, S).contiguous()
            q, c0, c = fit.solve(observed, start, view)
            stream.synchronize()
            points = (observed < fit.fg_max).sum((2, 3)).float().mean().item()
            print("B=%d V=%d %dx%d: %.0f data points per view; %d iterations: median cost %.4g from %.4g, cost <= cost0 on %d of %d"
                  % (B, V, S, S, points, ITERS, c.median().item(), c0.median().item(), int((c <= c0).sum()), B), flush=True)
            ax, bx, ay, by = fit.pixel_to_model
            fg, md = fit.fg_max, fit.max_dist
            keypoints, jac = torch.empty(B, J, 4, device="cuda"), torch.empty(B, 3 * J, 26, device="cuda")
            centres = torch.empty(B, V, J, 4, device="cuda")
            A = torch.empty(B, 26, 26, dtype=torch.float64, device="cuda")
            g, cost = torch.empty(B, 26, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
            count = torch.empty(B, dtype=torch.int32, device="cuda")
            ws = torch.empty(max(16, lib.shr_sphere_icp_normal_workspace_bytes(B, V, J, S, S)), dtype=torch.uint8, device="cuda")
            background = torch.full_like(observed, 100.0)
            state, trial = ops.pose_lm_begin(start, 1e-3)
            nxt, par, cst, cst0 = (torch.empty(B, 26, device="cuda"), torch.empty(B, 26, device="cuda"), torch.empty(B, device="cuda"),
                                   torch.empty(B, device="cuda"))
            mu = fit.stiffness

            def jacobian(s):
                return lib.shr_pose_keypoints_jacobian(p(trial), B, p(off), p(inv), J, p(bone), p(wv), 1, p(keypoints), p(jac), s)

            def views(s):
                return lib.shr_view_vertices_fwd(p(keypoints), p(view), B, V, J, p(centres), s)

            def normal_of(obs, max_dist=md):
                return lambda s: lib.shr_sphere_icp_normal(p(obs), p(centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by,
                                                           fg, max_dist, p(A), p(g), p(cost), p(count), None, None, None, p(ws), s)

            def step(s):
                return lib.shr_pose_lm_step(p(state), p(A), p(g), p(cost), p(trial), None, p(mu), 1, B, p(nxt), p(par), p(cst), p(cst0), s)

            runs = {"jacobian": jacobian, "views": views, "empty": normal_of(background), "search": normal_of(observed, 0.0),
                    "normal": normal_of(observed), "step": step}
            for label, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, label
            stream.synchronize()
            print("  rows per sample at the start: %.0f" % count.float().mean().item(), flush=True)
            us = {k: [] for k in runs}
            for rnd in range(ROUNDS):
                for label, fn in runs.items():
                    us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
                print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
            us = {k: float(np.median(v)) for k, v in us.items()}
            total = us["jacobian"] + us["views"] + us["normal"] + us["step"]
            floor = B * V * S * S * 4 / HBM_PEAK * 1e6
            print("sphere icp B=%d V=%d %dx%d: jacobian %.2f us, views %.2f us, normal %.2f us (on an empty observation %.2f us, with the "
                  "search alone %.2f us), step %.2f us; one iteration %.2f us; the entry's reads %.1f MB = %.2f us at the HBM peak: %.1f x that floor"
                  % (B, V, S, S, us["jacobian"], us["views"], us["normal"], us["empty"], us["search"], us["step"], total,
                     B * V * S * S * 4 / 1e6, floor, us["normal"] / floor), flush=True)
            sphere[V] = dict(us, total=total)
    mesh_us = bench_pose_icp.main()[(B, S)]
    mesh_total = sum(mesh_us.values())
    for V, us in sphere.items():
        print("sphere iteration V=%d %.2f us against the mesh iteration (one view) %.2f us: %.1f x shorter; the new entry %.2f us "
              "against search + normal of the mesh %.2f us" % (V, us["total"], mesh_total, mesh_total / us["total"], us["normal"],
                                                               mesh_us["search"] + mesh_us["normal"]), flush=True)


if __name__ == "__main__":
    main()
