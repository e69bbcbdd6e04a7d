"""The sequence fit of the sphere model (shr_sphere_temporal_normal, sphere_temporal.hip; shr_pose_lm_seq_step, lm_seq.hip),
HIP events on the launching stream, through the C ABI (no Python op in the loop).  At the start poses, on top of the
per-frame terms' A, g and cost (the image terms, the priors, the collision term, each run once before anything is timed):
  temporal   shr_sphere_temporal_normal with accumulate = 1 (a NEW entry): one workgroup per frame
  seq_step   shr_pose_lm_seq_step with the solve (a NEW entry): one workgroup of one wave PER SEQUENCE, the frames of a
             sequence one after the other -- with S workgroups it is a LATENCY CHAIN of T frames, reported as such
             (us per frame of the chain beside the total)
  step       shr_pose_lm_step with the solve, the per-frame step it replaces: one wave per frame, all frames side by side
for 256 frames at 128 x 128 with one view as 32 sequences of 8 frames and as 8 sequences of 32, the hand's 41 spheres;
sequences interpolated between two sampled poses, observations rendered from the SPHERE model by the sphere rasterizer,
keypoints the true centres + N(0, 2 mm) per frame, starts p* + N(0, 0.1) rad / N(0, 2 mm) per frame; in the same process,
alternated, three rounds (every round is printed; the summary is the median).  First measurements: no target is set.  Before
anything is timed the whole loop runs once as sequences and frame by frame, and their keypoint errors and jitters are
printed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import SphereCollisionPoseFitter, SphereSequencePoseFitter  # noqa: E402
from tools.bench_sphere_icp import VIEWS  # noqa: E402

ROUNDS = 3
ITERS = 10
SIGMA_K = 2.0


def one_shape(mesh, lib, stream, B, T, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    V, Q = 1, B // T
    stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
    fit = SphereSequencePoseFitter(mesh, S, S, T, iters=ITERS, stiffness=stiffness).cuda()
    frames = SphereCollisionPoseFitter(mesh, S, S, iters=ITERS, stiffness=stiffness).cuda()
    off, inv, bone, wv, radii = fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv, fit.radii
    J = fit.num_spheres
    gen = torch.Generator().manual_seed(B + T)
    ends = sample_poses_batched(2 * Q, generator=gen)
    ends[:, 3:5] = 5.0 * torch.randn(2 * Q, 2, generator=gen)
    ends[:, 5] = 50.0
    lam = torch.linspace(0, 1, T)
    truth = (ends[0::2, None] * (1 - lam)[None, :, None] + ends[1::2, None] * lam[None, :, None]).reshape(B, 26)
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
    q, c0, c = fit.solve(observed, start, view, keypoints=targets)
    qf, _, _ = frames.solve(observed, start, view, keypoints=targets)

    def centres(t):
        return ops.pose_keypoints_jacobian(t, off, inv, bone, wv, True)[0][..., :3].view(Q, T, J, 3)

    ct = centres(truth)
    err = [(centres(t) - ct).norm(dim=-1).mean().item() for t in (start, qf, q)]
    jit = [((centres(t)[:, 1:] - centres(t)[:, :-1]) - (ct[:, 1:] - ct[:, :-1])).norm(dim=-1).mean().item() for t in (start, qf, q)]
    stream.synchronize()
    print("B=%d as %d x %d, %dx%d, temporal_weight %g, ts_max %g, sigma_k %g mm; %d iterations: cost <= cost0 on %d of %d sequences; "
          "mean keypoint error %.2f mm at the start, %.2f frame by frame, %.2f as sequences; jitter %.2f, %.2f, %.2f mm"
          % (B, Q, T, S, S, fit.temporal_weight, fit.ts_max, SIGMA_K, ITERS, int((c <= c0).sum()), Q, err[0], err[1], err[2],
             jit[0], jit[1], jit[2]), flush=True)
    ax, bx, ay, by = fit.pixel_to_model
    fg, md, mr, bg, w = fit.fg_max, fit.max_dist, fit.max_resid, fit.background, fit.render_weight
    kw, km, lw, cw = fit.kp_weight, fit.kp_max, fit.limit_weight, fit.collision_weight
    tw, cap = fit.temporal_weight, fit.ts_max
    lo, hi = fit.lower, fit.upper
    pa, pb, pm = fit.pair_a, fit.pair_b, fit.pair_min
    f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    keypoints, jac, view_centres = f32(B, J, 4), f32(B, 3 * J, 26), f32(B, V, J, 4)
    A, g, E, cost = f64(B, 26, 26), f64(B, 26), f64(B, 26, 26), f64(B)
    count, rows, prior_rows, pair_rows, temporal_rows = i32(B), i32(B), i32(B, 2), i32(B), i32(B)
    ws = torch.empty(max(16, lib.shr_sphere_render_normal_workspace_bytes(B, V, J, S, S)), dtype=torch.uint8, device="cuda")
    seq_ws = f64(lib.shr_pose_lm_seq_workspace_bytes(B) // 8)
    state, trial = ops.pose_lm_begin(start, 1e-3)
    seq_state, seq_trial = ops.pose_lm_seq_begin(start, T, 1e-3)
    nxt, par, cst, cst0 = f32(B, 26), f32(B, 26), f32(B), f32(B)
    mu = fit.stiffness
    s0 = stream.cuda_stream
    for rc in (lib.shr_pose_keypoints_jacobian(p(trial), B, p(off), p(inv), J, p(bone), p(wv), 1, p(keypoints), p(jac), s0),
               lib.shr_view_vertices_fwd(p(keypoints), p(view), B, V, J, p(view_centres), s0),
               lib.shr_sphere_icp_normal(p(observed), p(view_centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by, fg,
                                         md, p(A), p(g), p(cost), p(count), None, None, None, p(ws), s0),
               lib.shr_sphere_render_normal(p(observed), p(view_centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by,
                                            fg, bg, mr, w, 1, p(A), p(g), p(cost), p(rows), None, None, None, p(ws), s0),
               lib.shr_sphere_prior_normal(p(view_centres), p(view), p(jac), p(trial), p(targets), None, kw, km, p(lo), p(hi), lw,
                                           B, V, J, 1, p(A), p(g), p(cost), p(prior_rows), None, None, s0),
               lib.shr_sphere_collision_normal(p(keypoints), p(jac), p(pa), p(pb), p(pm), cw, B, J, pa.shape[0], 1, p(A), p(g),
                                               p(cost), p(pair_rows), None, None, s0)):
        assert rc == 0
    stream.synchronize()
    A0, g0, cost0 = A.clone(), g.clone(), cost.clone()       # the per-frame terms' sums: what the new entry adds to

    def reset():
        A.copy_(A0), g.copy_(g0), cost.copy_(cost0)

    def temporal(s):
        return lib.shr_sphere_temporal_normal(p(keypoints), p(jac), None, tw, cap, B, T, J, 1, p(A), p(g), p(E), p(cost),
                                              p(temporal_rows), None, s)

    def seq_step(s):
        return lib.shr_pose_lm_seq_step(p(seq_state), p(A), p(g), p(E), p(cost), p(seq_trial), None, p(mu), 1, B, T, p(nxt), p(par),
                                        p(cst), p(cst0), p(seq_ws), s)

    def step(s):
        return lib.shr_pose_lm_step(p(state), p(A), p(g), p(cost), p(trial), None, p(mu), 1, B, p(nxt), p(par), p(cst), p(cst0), s)

    runs = {"temporal": temporal, "seq_step": seq_step, "step": step}
    for label, fn in runs.items():
        assert fn(s0) == 0, label
    stream.synchronize()
    print("  spheres with temporal rows per pair at the start: %.1f of %d" % (temporal_rows.float().sum().item() / (B - Q), J), flush=True)
    us = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for label, fn in runs.items():
            reset()                                              # (the accumulating entry lets A grow over the timed repetitions,
            assert temporal(s0) == 0                             #  which costs the same; the steps start from one sum of it)
            us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
    us = {k: float(np.median(v)) for k, v in us.items()}
    print("sphere sequence B=%d as %d sequences x %d frames, %dx%d: temporal %.2f us, seq_step %.2f us (%d workgroups, a latency "
          "chain of %d frames: %.2f us per frame of the chain) beside step %.2f us (%d workgroups)"
          % (B, Q, T, S, S, us["temporal"], us["seq_step"], Q, T, us["seq_step"] / T, us["step"], B), flush=True)
    return us


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    stream = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(stream):
        for T in (8, 32):
            out[T] = one_shape(mesh, lib, stream, 256, T, 128)
    return out


if __name__ == "__main__":
    main()
