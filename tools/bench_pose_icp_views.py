"""One pose fitted to several depth views (shr_view_vertices_fwd, shr_pose_icp_normal_views, pose_icp_views.hip), HIP
events on the launching stream, through the C ABI (no Python op in the loop).  One iteration of the fit at the start poses,
its five launches timed one by one:
  vertices   shr_pose_vertices_fwd (project = 0) of the trial poses
  view       shr_view_vertices_fwd: the vertices in every view's frame
  search     shr_mesh_d2m_fwd over the B V crops: the closest-point search, the EXISTING kernel
  normal     shr_pose_icp_normal_views: the normal equations of the pose, summed over the views
  step       shr_pose_lm_step with the solve
for 256 samples x 3 views at 128 x 128 of the hand's distinct mesh (1 721 vertices, 3 382 faces): the model frame and the
views 90 degrees about y and about x through the palm, observations self-rendered by the triangle raster at sampled poses,
starts p* + N(0, 0.1) rad / N(0, 2 mm).  In the same process and the same rounds, for comparison, the single-view loop of
tools/bench_pose_icp.py on the same 768 crops taken as 768 samples (search1, normal1, step1, vertices1: each crop then has
a pose of its own; the maps, and so the rows of the normal equations, are the same).  Alternated, three rounds (every round
is printed; the summary is the median).  First measurements: no target is set.  Before anything is timed the whole loop
(ops.pose_icp_views, 10 iterations) runs once and its costs are printed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import MeshDataToModelLoss, MultiViewMeshPoseFitter, TriangleDepthRaster  # noqa: E402

ROUNDS = 3
ITERS = 10
RY90 = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]
RX90 = [[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]


def about(R, centre):
    R, c = np.asarray(R, np.float64), np.asarray(centre, np.float64)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, c - R @ c
    return M.astype(np.float32)


def main():
    B, V, S = 256, 3, 128
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
        fit = MultiViewMeshPoseFitter(mesh, S, S, iters=ITERS, stiffness=stiffness).cuda()
        lbs = fit.vertices.lbs
        off, inv, faces = fit.fk.offset, fit.fk.offset_inv, fit.faces_i32
        start_, bone, wv = lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv
        NV, F = fit.vertices.num_vertices, faces.shape[0]
        gen = torch.Generator().manual_seed(B)
        truth = sample_poses_batched(B, generator=gen)
        truth[:, 3:5] = 5.0 * torch.randn(B, 2, generator=gen)
        truth[:, 5] = 50.0
        start = truth + 0.1 * torch.randn(B, 26, generator=gen)
        start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
        truth, start = truth.float().cuda(), start.float().cuda()
        centre = (0.0, 0.0, 50.0)
        view = torch.from_numpy(np.stack([np.eye(4, dtype=np.float32), about(RY90, centre), about(RX90, centre)])).cuda()
        view = view.unsqueeze(0).expand(B, V, 4, 4).contiguous()
        with torch.no_grad():
            vv = ops.view_vertices(fit.vertices.pose_vertices(fit.fk, truth), view).view(B * V, NV, 4)
            pixel = torch.stack([vv[..., 0] * (S / 300.0) + S / 2.0, vv[..., 1] * (S / 300.0) + S / 2.0, vv[..., 2], vv[..., 3]], -1)
            raster = TriangleDepthRaster(S, S, fit.vertices.faces).cuda()
            observed = torch.clamp(raster(pixel.contiguous()), max=100.0).view(B, V, S, S).contiguous()
        q, c0, c = fit.solve(observed, view, start)
        stream.synchronize()
        points = (observed < MeshDataToModelLoss.REFERENCE_FG_MAX).sum((2, 3)).float().mean(0).tolist()
        print("B=%d V=%d %dx%d: %s data points per view; %d iterations: median cost %.4g from %.4g, cost <= cost0 on %d of %d"
              % (B, V, S, S, ["%.0f" % t for t in points], ITERS, c.median().item(), c0.median().item(), int((c <= c0).sum()), B),
              flush=True)
        ax, bx, ay, by = fit.pixel_to_model
        fg, md = fit.fg_max, fit.max_dist
        N = B * V
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")   # noqa: E731
        verts, vverts, verts1 = new(B, NV, 4), new(B, V, NV, 4), new(N, NV, 4)
        dist, face = new(B, V, S, S), new(B, V, S, S, dtype=torch.int32)
        A, g, cost, count = new(B, 26, 26, dtype=torch.float64), new(B, 26, dtype=torch.float64), new(B, dtype=torch.float64), \
            new(B, dtype=torch.int32)
        A1, g1, cost1, count1 = new(N, 26, 26, dtype=torch.float64), new(N, 26, dtype=torch.float64), new(N, dtype=torch.float64), \
            new(N, dtype=torch.int32)
        ws_d = new(max(16, lib.shr_mesh_d2m_workspace_bytes(N, F)), dtype=torch.uint8)
        ws_n = new(max(16, lib.shr_pose_icp_normal_views_workspace_bytes(B, V, S, S)), dtype=torch.uint8)
        ws_1 = new(max(16, lib.shr_pose_icp_normal_workspace_bytes(N, S, S)), dtype=torch.uint8)
        state, trial = ops.pose_lm_begin(start, 1e-3)
        trial1 = start.repeat_interleave(V, 0).contiguous()       # crop b V + v: sample b's start pose
        state1, trial1 = ops.pose_lm_begin(trial1, 1e-3)
        nxt, par, cst, cst0 = new(B, 26), new(B, 26), new(B), new(B)
        nxt1, par1, cst1, cst01 = new(N, 26), new(N, 26), new(N), new(N)
        mu = fit.stiffness

        def vertices(s):
            return lib.shr_pose_vertices_fwd(p(trial), B, p(off), p(inv), NV, p(start_), p(bone), p(wv), 1, 0, 0.0, 0.0, 1.0, 1.0,
                                             None, p(verts), None, s)

        def views(s):
            return lib.shr_view_vertices_fwd(p(verts), p(view), B, V, NV, p(vverts), s)

        def search(s):
            return lib.shr_mesh_d2m_fwd(p(observed), p(vverts), p(faces), N, NV, F, S, S, ax, bx, ay, by, fg, md, p(dist), p(face),
                                        p(ws_d), s)

        def normal(s):
            return lib.shr_pose_icp_normal_views(p(observed), p(vverts), p(faces), p(dist), p(face), p(view), p(trial), p(off),
                                                 p(inv), p(start_), p(bone), p(wv), 1, B, V, NV, F, S, S, ax, bx, ay, by, fg, md,
                                                 p(A), p(g), p(cost), p(count), p(ws_n), s)

        def step(s):
            return lib.shr_pose_lm_step(p(state), p(A), p(g), p(cost), p(trial), None, p(mu), 1, B, p(nxt), p(par), p(cst), p(cst0), s)

        # the single-view loop on the same 768 crops: the view-frame vertices stand in for shr_pose_vertices_fwd's (the
        # search and the rows' closest points are then the views'; the rows' derivatives are those of 768 poses)
        def vertices1(s):
            return lib.shr_pose_vertices_fwd(p(trial1), N, p(off), p(inv), NV, p(start_), p(bone), p(wv), 1, 0, 0.0, 0.0, 1.0, 1.0,
                                             None, p(verts1), None, s)

        def search1(s):
            return lib.shr_mesh_d2m_fwd(p(observed), p(vverts), p(faces), N, NV, F, S, S, ax, bx, ay, by, fg, md, p(dist), p(face),
                                        p(ws_d), s)

        def normal1(s):
            return lib.shr_pose_icp_normal(p(observed), p(vverts), p(faces), p(dist), p(face), p(trial1), p(off), p(inv), p(start_),
                                           p(bone), p(wv), 1, N, NV, F, S, S, ax, bx, ay, by, fg, md, p(A1), p(g1), p(cost1),
                                           p(count1), p(ws_1), s)

        def step1(s):
            return lib.shr_pose_lm_step(p(state1), p(A1), p(g1), p(cost1), p(trial1), None, p(mu), 1, N, p(nxt1), p(par1), p(cst1),
                                        p(cst01), s)

        runs = {"vertices": vertices, "view": views, "search": search, "normal": normal, "step": step,
                "vertices1": vertices1, "search1": search1, "normal1": normal1, "step1": step1}
        for label, fn in runs.items():
            assert fn(stream.cuda_stream) == 0, label
        stream.synchronize()
        print("  rows per sample at the start: %.0f over %d views; the single-view entry on the same %d crops: %.0f per crop"
              % (count.float().mean().item(), V, N, count1.float().mean().item()), flush=True)
        assert int(count.sum()) == int(count1.sum())
        us = {k: [] for k in runs}
        for rnd in range(ROUNDS):
            for label, fn in runs.items():
                us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
            print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
        us = {k: float(np.median(v)) for k, v in us.items()}
        total = us["vertices"] + us["view"] + us["search"] + us["normal"] + us["step"]
        total1 = us["vertices1"] + us["search1"] + us["normal1"] + us["step1"]
        print("pose icp views B=%d V=%d %dx%d: vertices %.2f us, view %.2f us, search %.2f us, normal %.2f us, step %.2f us; one "
              "iteration %.2f us, the search %.1f %% of it" % (B, V, S, S, us["vertices"], us["view"], us["search"], us["normal"],
                                                             us["step"], total, 100.0 * us["search"] / total), flush=True)
        print("pose icp single view B=%d %dx%d: vertices %.2f us, search %.2f us, normal %.2f us, step %.2f us; one iteration "
              "%.2f us; normal views / normal single %.3f" % (N, S, S, us["vertices1"], us["search1"], us["normal1"], us["step1"],
                                                              total1, us["normal"] / us["normal1"]), flush=True)


if __name__ == "__main__":
    main()
