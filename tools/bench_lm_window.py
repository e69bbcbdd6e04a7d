"""The sliding-window tracker's two entries (shr_pose_window_marginalize and shr_pose_window_prior_normal, lm_window.hip), HIP
events on the launching stream, through the C ABI (no Python op in the loop).  On the normal equations of
SphereTrajectoryPoseFitter at the start poses (formed once before anything is timed), for S in {32, 256} sequences:
  marginalize  the entry on S x 3 frames with E and F, a prior pose and a stiffness: one workgroup of 256 threads per sequence
  prior        the carried prior's term (accumulate = 1, accumulate_E = 1) on S x 3 and on S x 8 frames: one workgroup per frame,
               all but the first two of a sequence returning at once
  seq2_step    shr_pose_lm_seq2_step with F and the solve on the SAME S at T = 3 and T = 8.  lm_seq2.hip is byte for byte what it
               was, so this is the parent's number
in the same process, alternated, three rounds, the odd ones in reverse order (every round is printed; the summary is the
median, the spread max - min over the rounds).  First measurements: no target is set, the ratios are reported.
Then the tracker itself, wall time between HIP events around the Python calls (launch overhead included), S = 8 streams at
128 x 128, W = 8, iters = 10: one advance (departing system, marginalisation, shift, fit with the prior) against one fit of the
same window without a prior, and against SphereTrajectoryPoseFitter.solve over all N = 32 frames."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import SphereTrajectoryPoseFitter, SphereWindowTracker  # noqa: E402

ROUNDS = 3
SIGMA_K = 2.0
STIFFNESS = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)


def scene(fit, Q, T, S, seed):
    """(observed [B,S,S], keypoint targets [B,J,3], start [B,26]) of Q sequences of T frames: tools/bench_lm_covariance.py's"""
    B, J = Q * T, fit.num_spheres
    gen = torch.Generator().manual_seed(seed)
    ends = sample_poses_batched(2 * Q, generator=gen)
    ends[:, 3:5] = 5.0 * torch.randn(2 * Q, 2, generator=gen)
    ends[:, 5] = 50.0
    lam = torch.linspace(0, 1, T)
    truth = (ends[0::2, None] * (1 - lam)[None, :, None] + ends[1::2, None] * lam[None, :, None]).reshape(B, 26)
    start = truth + 0.1 * torch.randn(B, 26, generator=gen)
    start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
    noise = SIGMA_K * torch.randn(B, J, 3, generator=gen)
    truth, start = truth.float().cuda(), start.float().cuda()
    kp, _ = ops.pose_keypoints_jacobian(truth, fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv, True)
    spheres = kp.clone()
    targets = (spheres[..., :3] + noise.cuda()).contiguous()
    spheres[..., 3] = fit.radii
    observed = torch.clamp(ops.sphere_raster_fwd(spheres.contiguous(), S, S), max=100.0).contiguous()
    return observed, targets, start


def entries(mesh, lib, stream, Q, S=64):
    p = lambda t: t.data_ptr()  # noqa: E731
    f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    runs, keep = {}, []
    for T in (3, 8):
        B = Q * T
        fit = SphereTrajectoryPoseFitter(mesh, S, S, T, stiffness=STIFFNESS).cuda()
        observed, targets, start = scene(fit, Q, T, S, Q + T)
        A, g, E, F, cost, _ = fit.normal_equations(observed, start, keypoints=targets)
        mu = fit.stiffness
        if T == 3:
            prior = (start + 0.01).contiguous()
            Lam, eta, off, point, status = f64(Q, 52, 52), f64(Q, 52), f64(Q), f32(Q, 52), torch.empty(Q, dtype=torch.int32, device="cuda")

            def marginalize(s, A=A, g=g, E=E, F=F, cost=cost, start=start, prior=prior, B=B):
                return lib.shr_pose_window_marginalize(p(A), p(g), p(E), p(F), p(cost), p(start), p(prior), p(mu), B, 3, p(Lam),
                                                       p(eta), p(off), p(point), p(status), None, s)
            assert marginalize(stream.cuda_stream) == 0
            stream.synchronize()
            print("S=%d: %d of %d leaving frames factorise" % (Q, int((status == 0).sum()), Q), flush=True)
            runs["marginalize"] = marginalize
        A2, g2, E2, c2 = A.clone(), g.clone(), E.clone(), cost.clone()

        def prior_term(s, T=T, B=B, start=start, A2=A2, g2=g2, E2=E2, c2=c2):
            return lib.shr_pose_window_prior_normal(p(start), p(Lam), p(eta), p(off), p(point), None, B, T, 1, 1, p(A2), p(g2), p(E2),
                                                    p(c2), None, s)
        ws = f64(lib.shr_pose_lm_seq2_workspace_bytes(B) // 8)
        state, trial = ops.pose_lm_seq2_begin(start, T, 1e-3)
        nxt, par, cst, cst0 = f32(B, 26), f32(B, 26), f32(Q), f32(Q)

        def seq2_step(s, T=T, B=B, A=A, g=g, E=E, F=F, cost=cost, state=state, trial=trial, ws=ws, out=(nxt, par, cst, cst0)):
            return lib.shr_pose_lm_seq2_step(p(state), p(A), p(g), p(E), p(F), p(cost), p(trial), None, p(mu), 1, B, T, p(out[0]),
                                             p(out[1]), p(out[2]), p(out[3]), p(ws), s)
        runs["prior_T%d" % T], runs["seq2_step_T%d" % T] = prior_term, seq2_step
        keep.append((A, g, E, F, cost, start))
    for label, fn in runs.items():
        assert fn(stream.cuda_stream) == 0, label
    stream.synchronize()
    us = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for label, fn in (list(runs.items()) if rnd % 2 == 0 else list(runs.items())[::-1]):      # (odd rounds in reverse order)
            us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
    spread = {k: float(max(v) - min(v)) for k, v in us.items()}
    us = {k: float(np.median(v)) for k, v in us.items()}
    print("lm window S=%d: marginalize %.2f us (spread %.2f; %d workgroups); prior term %.2f us at T=3, %.2f us at T=8 (spreads %.2f, "
          "%.2f); seq2_step %.2f us at T=3, %.2f us at T=8 (spreads %.2f, %.2f): a marginalisation is %.2f x one T=3 step, "
          "%.2f x one T=8 step" % (Q, us["marginalize"], spread["marginalize"], Q, us["prior_T3"], us["prior_T8"], spread["prior_T3"],
                                   spread["prior_T8"], us["seq2_step_T3"], us["seq2_step_T8"], spread["seq2_step_T3"],
                                   spread["seq2_step_T8"], us["marginalize"] / us["seq2_step_T3"],
                                   us["marginalize"] / us["seq2_step_T8"]), flush=True)
    return us


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def tracker(mesh, stream, Q=8, W=8, N=32, S=128):
    track = SphereWindowTracker(mesh, S, S, W, stiffness=STIFFNESS).cuda()
    whole = SphereTrajectoryPoseFitter(mesh, S, S, N, stiffness=STIFFNESS).cuda()
    observed, targets, start = scene(track, Q, N, S, 77)
    per = lambda t: t.view((Q, N) + tuple(t.shape[1:]))  # noqa: E731
    head = lambda t, a: per(t)[:, a:a + W].reshape((Q * W,) + tuple(t.shape[1:])).contiguous()  # noqa: E731
    window = track.begin(head(observed, 0), head(start, 0), keypoints=head(targets, 0))[0]
    window = track.advance(window, per(observed)[:, W], keypoints_new=per(targets)[:, W])[0]       # (a window that carries a prior)
    runs = {"advance": lambda: track.advance(window, per(observed)[:, W + 1], keypoints_new=per(targets)[:, W + 1]),
            "window_fit": lambda: track.begin(head(observed, 2), window["start"], keypoints=head(targets, 2)),
            "whole_fit": lambda: whole.solve(observed, start, keypoints=targets)}
    for fn in runs.values():
        fn()
    stream.synchronize()
    ms = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for label, fn in (list(runs.items()) if rnd % 2 == 0 else list(runs.items())[::-1]):
            ms[label].append(timed(fn, stream))
        print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in ms.items())), flush=True)
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
    ms = {k: float(np.median(v)) for k, v in ms.items()}
    print("tracker %d streams, W=%d, %dx%d, iters=%d: one advance %.2f ms (spread %.2f), one fit of the same window %.2f ms (spread "
          "%.2f): %.2f x; SphereTrajectoryPoseFitter.solve over all %d frames %.2f ms (spread %.2f): %.2f advances"
          % (Q, W, S, S, track.iters, ms["advance"], spread["advance"], ms["window_fit"], spread["window_fit"],
             ms["advance"] / ms["window_fit"], N, ms["whole_fit"], spread["whole_fit"], ms["whole_fit"] / ms["advance"]), flush=True)
    return ms


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    stream = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(stream):
        for Q in (32, 256):
            out[Q] = entries(mesh, lib, stream, Q)
        out["tracker"] = tracker(mesh, stream)
    return out


if __name__ == "__main__":
    main()
