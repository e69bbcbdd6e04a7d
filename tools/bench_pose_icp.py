"""Pose from observed depth points (shr_pose_icp_normal, shr_pose_lm_step, pose_icp.hip), HIP events on the launching
stream, through the C ABI (no Python op in the loop).  One iteration of the fit at the start poses, its four launches timed
one by one:
  vertices   shr_pose_vertices_fwd (project = 0) of the trial poses
  search     shr_mesh_d2m_fwd: the closest-point search, the EXISTING kernel
  normal     shr_pose_icp_normal: the normal equations of the pose
  step       shr_pose_lm_step with the solve
for 256 crops at 128 x 128 (and, with --large, 1152 at 256 x 256) of the hand's distinct mesh (1 721 vertices, 3 382 faces),
observations self-rendered by the triangle raster at sampled poses, starts p* + N(0, 0.1) rad / N(0, 2 mm); in the same
process, alternated, three rounds (every round is printed; the summary is the median).  First measurements: no target is
set.  Before anything is timed the whole loop (ops.pose_icp, 10 iterations) runs once and its costs are printed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import MeshDataToModelLoss, MeshPoseFitter, MeshVertices, TriangleDepthRaster  # noqa: E402

ROUNDS = 3
ITERS = 10


def main():
    configs = [(256, 128)] + ([(1152, 256)] if "--large" in sys.argv else [])
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = torch.cuda.Stream()
    summary = {}                                                    # (B, S) -> the launches' medians, us
    with torch.cuda.stream(stream):
        for B, S in configs:
            stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
            fit = MeshPoseFitter(mesh, S, S, iters=ITERS, stiffness=stiffness).cuda()
            lbs = fit.vertices.lbs
            off, inv, start_, bone, wv, faces = fit.fk.offset, fit.fk.offset_inv, lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv, fit.faces_i32
            NV, F = fit.vertices.num_vertices, faces.shape[0]
            gen = torch.Generator().manual_seed(B)
            truth = sample_poses_batched(B, generator=gen)
            truth[:, 3:5] = 5.0 * torch.randn(B, 2, generator=gen)
            truth[:, 5] = 50.0
            start = truth + 0.1 * torch.randn(B, 26, generator=gen)
            start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
            truth, start = truth.float().cuda(), start.float().cuda()
            pix = MeshVertices(mesh, camera=MeshVertices.pixel_camera(S, S)).cuda()
            with torch.no_grad():
                observed = torch.clamp(TriangleDepthRaster(S, S, pix.faces).cuda()(pix.pose_vertices(fit.fk, truth)), max=100.0).contiguous()
            q, c0, c = fit.solve(observed, start)
            stream.synchronize()
            points = (observed < MeshDataToModelLoss.REFERENCE_FG_MAX).sum((1, 2)).float().mean().item()
            print("B=%d %dx%d: %.0f data points per crop; %d iterations: median cost %.4g from %.4g, cost <= cost0 on %d of %d"
                  % (B, S, S, points, ITERS, c.median().item(), c0.median().item(), int((c <= c0).sum()), B), flush=True)
            ax, bx, ay, by = fit.pixel_to_model
            fg, md = fit.fg_max, fit.max_dist
            verts = torch.empty(B, NV, 4, device="cuda")
            dist, face = torch.empty(B, S, S, device="cuda"), torch.empty(B, S, S, dtype=torch.int32, device="cuda")
            A = torch.empty(B, 26, 26, dtype=torch.float64, device="cuda")
            g, cost = torch.empty(B, 26, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
            count = torch.empty(B, dtype=torch.int32, device="cuda")
            ws_d = torch.empty(max(16, lib.shr_mesh_d2m_workspace_bytes(B, F)), dtype=torch.uint8, device="cuda")
            ws_n = torch.empty(max(16, lib.shr_pose_icp_normal_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")
            state, trial = ops.pose_lm_begin(start, 1e-3)
            nxt, par, cst, cst0 = (torch.empty(B, 26, device="cuda"), torch.empty(B, 26, device="cuda"), torch.empty(B, device="cuda"),
                                   torch.empty(B, device="cuda"))
            mu = fit.stiffness

            def vertices(s):
                return lib.shr_pose_vertices_fwd(p(trial), B, p(off), p(inv), NV, p(start_), p(bone), p(wv), 1, 0, 0.0, 0.0, 1.0, 1.0,
                                                 None, p(verts), None, s)

            def search(s):
                return lib.shr_mesh_d2m_fwd(p(observed), p(verts), p(faces), B, NV, F, S, S, ax, bx, ay, by, fg, md, p(dist), p(face),
                                            p(ws_d), s)

            def normal(s):
                return lib.shr_pose_icp_normal(p(observed), p(verts), p(faces), p(dist), p(face), p(trial), p(off), p(inv), p(start_),
                                               p(bone), p(wv), 1, B, NV, F, S, S, ax, bx, ay, by, fg, md, p(A), p(g), p(cost), p(count),
                                               p(ws_n), s)

            def step(s):
                return lib.shr_pose_lm_step(p(state), p(A), p(g), p(cost), p(trial), None, p(mu), 1, B, p(nxt), p(par), p(cst), p(cst0), s)

            runs = {"vertices": vertices, "search": search, "normal": normal, "step": step}
            for label, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, label
            stream.synchronize()
            print("  rows per crop at the start: %.0f" % count.float().mean().item(), flush=True)
            us = {k: [] for k in runs}
            for rnd in range(ROUNDS):
                for label, fn in runs.items():
                    us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
                print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
            us = {k: float(np.median(v)) for k, v in us.items()}
            total = sum(us.values())
            print("pose icp B=%d %dx%d: vertices %.2f us, search %.2f us, normal %.2f us, step %.2f us; one iteration %.2f us, "
                  "the search %.1f %% of it" % (B, S, S, us["vertices"], us["search"], us["normal"], us["step"], total,
                                                 100.0 * us["search"] / total), flush=True)
            summary[(B, S)] = us
    return summary


if __name__ == "__main__":
    main()
