"""The constant-velocity term and the block-pentadiagonal step of the sphere model's sequence fit (shr_sphere_accel_normal,
sphere_accel.hip; shr_pose_lm_seq2_step, lm_seq2.hip), HIP events on the launching stream, through the C ABI (no Python op
in the loop).  At the start poses, on top of the per-frame terms' and the first-difference term's A, g, E and cost (each
run once before anything is timed):
  accel        shr_sphere_accel_normal with accumulate = 1 and accumulate_E = 1 (a NEW entry): one workgroup per frame
  seq2_step    shr_pose_lm_seq2_step with F and the solve (a NEW entry): one workgroup of one wave PER SEQUENCE, a latency
               chain of T frames, reported per frame of the chain too
  seq2_no_F    the same entry with F = NULL, which hands the call to shr_pose_lm_seq_step
  seq_step     shr_pose_lm_seq_step, the step it extends, from THIS build's library -- a substitution for the build of the
               commit before this unit, which a single process cannot load beside this one: lm_seq.hip is byte for byte
               what it was and is compiled with the same flags, so the kernel is the same
for 256 frames at 128 x 128 with one view as 32 sequences of 8 frames and as 8 sequences of 32, the hand's 41 spheres;
tools/bench_sphere_sequence.py's sequences, observations, keypoints and starts; in the same process, alternated, three
rounds, the odd ones in reverse order (every round is printed; the summary is the median, the spread is max - min over the rounds).  No target is set for
the new work.  The one condition: without F the step's median is not above shr_pose_lm_seq_step's by more than the
run-to-run spread (the larger of the two entries'); both are printed with the spread, and the tool exits with status 1
where the condition is missed.  Before anything is timed the whole loop runs once as trajectories, as sequences and
frame by frame, and their keypoint errors and jitters are printed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import (SphereCollisionPoseFitter, SphereSequencePoseFitter,  # noqa: E402
                                   SphereTrajectoryPoseFitter)
from tools.bench_sphere_icp import VIEWS  # noqa: E402

ROUNDS = 3
ITERS = 10
SIGMA_K = 2.0


def one_shape(mesh, lib, stream, B, T, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    V, Q = 1, B // T
    stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
    fit = SphereTrajectoryPoseFitter(mesh, S, S, T, iters=ITERS, stiffness=stiffness).cuda()
    seq = SphereSequencePoseFitter(mesh, S, S, T, iters=ITERS, stiffness=stiffness).cuda()
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
    qs, _, _ = seq.solve(observed, start, view, keypoints=targets)
    qf, _, _ = frames.solve(observed, start, view, keypoints=targets)

    def centres(t):
        return ops.pose_keypoints_jacobian(t, off, inv, bone, wv, True)[0][..., :3].view(Q, T, J, 3)

    ct = centres(truth)
    err = [(centres(t) - ct).norm(dim=-1).mean().item() for t in (start, qf, qs, q)]
    jit = [((centres(t)[:, 1:] - centres(t)[:, :-1]) - (ct[:, 1:] - ct[:, :-1])).norm(dim=-1).mean().item() for t in (start, qf, qs, q)]
    stream.synchronize()
    print("B=%d as %d x %d, %dx%d, accel_weight %g, acc_max %g, temporal_weight %g, sigma_k %g mm; %d iterations: cost <= cost0 on "
          "%d of %d sequences; mean keypoint error %.2f mm at the start, %.2f frame by frame, %.2f as sequences, %.2f as "
          "trajectories; jitter %.2f, %.2f, %.2f, %.2f mm"
          % (B, Q, T, S, S, fit.accel_weight, fit.acc_max, fit.temporal_weight, SIGMA_K, ITERS, int((c <= c0).sum()), Q, *err, *jit),
          flush=True)
    ax, bx, ay, by = fit.pixel_to_model
    fg, md, mr, bg, w = fit.fg_max, fit.max_dist, fit.max_resid, fit.background, fit.render_weight
    kw, km, lw, cw = fit.kp_weight, fit.kp_max, fit.limit_weight, fit.collision_weight
    tw, cap = seq.temporal_weight, seq.ts_max                     # (the first-difference term at ITS default, so that E is shared)
    aw, amax = fit.accel_weight, fit.acc_max
    lo, hi = fit.lower, fit.upper
    pa, pb, pm = fit.pair_a, fit.pair_b, fit.pair_min
    f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    keypoints, jac, view_centres = f32(B, J, 4), f32(B, 3 * J, 26), f32(B, V, J, 4)
    A, g, E, F, cost = f64(B, 26, 26), f64(B, 26), f64(B, 26, 26), f64(B, 26, 26), f64(B)
    count, rows, prior_rows, pair_rows, temporal_rows, accel_rows = i32(B), i32(B), i32(B, 2), i32(B), i32(B), i32(B)
    ws = torch.empty(max(16, lib.shr_sphere_render_normal_workspace_bytes(B, V, J, S, S)), dtype=torch.uint8, device="cuda")
    seq_ws = f64(lib.shr_pose_lm_seq_workspace_bytes(B) // 8)
    seq2_ws = f64(lib.shr_pose_lm_seq2_workspace_bytes(B) // 8)
    seq_state, seq_trial = ops.pose_lm_seq_begin(start, T, 1e-3)
    seq2_state, seq2_trial = ops.pose_lm_seq2_begin(start, T, 1e-3)
    bare_state, bare_trial = ops.pose_lm_seq2_begin(start, T, 1e-3)
    nxt, par, cst, cst0 = f32(B, 26), f32(B, 26), f32(Q), f32(Q)
    mu = fit.stiffness
    s0 = stream.cuda_stream
    for rc in (lib.shr_pose_keypoints_jacobian(p(seq_trial), B, p(off), p(inv), J, p(bone), p(wv), 1, p(keypoints), p(jac), s0),
               lib.shr_view_vertices_fwd(p(keypoints), p(view), B, V, J, p(view_centres), s0),
               lib.shr_sphere_icp_normal(p(observed), p(view_centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by, fg,
                                         md, p(A), p(g), p(cost), p(count), None, None, None, p(ws), s0),
               lib.shr_sphere_render_normal(p(observed), p(view_centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay, by,
                                            fg, bg, mr, w, 1, p(A), p(g), p(cost), p(rows), None, None, None, p(ws), s0),
               lib.shr_sphere_prior_normal(p(view_centres), p(view), p(jac), p(seq_trial), p(targets), None, kw, km, p(lo), p(hi),
                                           lw, B, V, J, 1, p(A), p(g), p(cost), p(prior_rows), None, None, s0),
               lib.shr_sphere_collision_normal(p(keypoints), p(jac), p(pa), p(pb), p(pm), cw, B, J, pa.shape[0], 1, p(A), p(g),
                                               p(cost), p(pair_rows), None, None, s0),
               lib.shr_sphere_temporal_normal(p(keypoints), p(jac), None, tw, cap, B, T, J, 1, p(A), p(g), p(E), p(cost),
                                              p(temporal_rows), None, s0)):
        assert rc == 0
    stream.synchronize()
    A0, g0, E0, cost0 = A.clone(), g.clone(), E.clone(), cost.clone()         # what the new entry adds to

    def reset():
        A.copy_(A0), g.copy_(g0), E.copy_(E0), cost.copy_(cost0)

    def accel(s):
        return lib.shr_sphere_accel_normal(p(keypoints), p(jac), None, aw, amax, B, T, J, 1, 1, p(A), p(g), p(E), p(F), p(cost),
                                           p(accel_rows), None, s)

    def seq2_step(s):
        return lib.shr_pose_lm_seq2_step(p(seq2_state), p(A), p(g), p(E), p(F), p(cost), p(seq2_trial), None, p(mu), 1, B, T,
                                         p(nxt), p(par), p(cst), p(cst0), p(seq2_ws), s)

    def seq2_no_F(s):
        return lib.shr_pose_lm_seq2_step(p(bare_state), p(A), p(g), p(E), None, p(cost), p(bare_trial), None, p(mu), 1, B, T,
                                         p(nxt), p(par), p(cst), p(cst0), p(seq2_ws), s)

    def seq_step(s):
        return lib.shr_pose_lm_seq_step(p(seq_state), p(A), p(g), p(E), p(cost), p(seq_trial), None, p(mu), 1, B, T, p(nxt), p(par),
                                        p(cst), p(cst0), p(seq_ws), s)

    runs = {"accel": accel, "seq2_step": seq2_step, "seq2_no_F": seq2_no_F, "seq_step": seq_step}
    for label, fn in runs.items():
        assert fn(s0) == 0, label
    stream.synchronize()
    print("  spheres with acceleration rows per triple at the start: %.1f of %d"
          % (accel_rows.float().sum().item() / max(1, B - 2 * Q), J), flush=True)
    us = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for label, fn in (list(runs.items()) if rnd % 2 == 0 else list(runs.items())[::-1]):      # (odd rounds in reverse order)
            reset()                                              # (the accumulating entry lets A grow over the timed repetitions,
            assert accel(s0) == 0                                #  which costs the same; the steps start from one sum of it)
            us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
    spread = {k: float(max(v) - min(v)) for k, v in us.items()}
    us = {k: float(np.median(v)) for k, v in us.items()}
    within = us["seq2_no_F"] - us["seq_step"] <= max(spread["seq2_no_F"], spread["seq_step"])     # (slower by no more)
    print("sphere trajectory B=%d as %d sequences x %d frames, %dx%d: accel %.2f us; seq2_step %.2f us (%d workgroups, a latency "
          "chain of %d frames: %.2f us per frame of the chain), %.2f x seq_step; without F %.2f us (spread %.2f) beside seq_step "
          "%.2f us (spread %.2f): the difference %.2f us is %s the spread"
          % (B, Q, T, S, S, us["accel"], us["seq2_step"], Q, T, us["seq2_step"] / T, us["seq2_step"] / us["seq_step"],
             us["seq2_no_F"], spread["seq2_no_F"], us["seq_step"], spread["seq_step"], us["seq2_no_F"] - us["seq_step"],
             "within" if within else "SLOWER than"), flush=True)
    us["within"] = within
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
    sys.exit(0 if all(r["within"] for r in main().values()) else 1)
