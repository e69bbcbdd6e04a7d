"""The pose-VAE prior's entry (shr_pose_vae_normal, pose_vae.hip), HIP events on the launching stream, through the C ABI (no
Python op in the loop), tools/bench_lm_window.py's method.  On the frames of SphereCollisionPoseFitter at sampled start
poses, for B in {32, 256}:
  pose_vae   the entry with accumulate = 1 on top of the other terms' equations: one workgroup of four waves per frame
  collision  shr_sphere_collision_normal with accumulate = 1 on the SAME frames, the module's table
  lm_step    shr_pose_lm_step with the solve on the SAME frames
  torch_jvp  the baseline: the torch composition on the GPU, PoseVae in fp32 with torch.func.jvp over the 26 tangents
             (vmap), r and J_r only -- no normal equations; wall time between HIP events, launch overhead included
in the same process, alternated, three rounds, the odd ones in reverse order (every round is printed; the summary is the
median, the spread max - min over the rounds).  First measurements: no target is set.  The only prior figure is arithmetic,
3 312 MFMAs per frame at 64 cycles per SIMD each over four SIMDs: about 22 us for one frame per CU at 2.4 GHz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops, pose_vae  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import PoseVaePrior, SphereCollisionPoseFitter  # noqa: E402

ROUNDS = 3


def timed(fn, stream, reps=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def entries(mesh, lib, stream, B):
    p = lambda t: t.data_ptr()  # noqa: E731
    fit = SphereCollisionPoseFitter(mesh, 64, 64).cuda()
    prior = PoseVaePrior(weight=0.1, latent_weight=1.0).cuda()
    gen = torch.Generator().manual_seed(B)
    start = sample_poses_batched(B, generator=gen).float().cuda()
    tabs = fit._tables()[:4]
    kp, jac = ops.pose_keypoints_jacobian(start, *tabs, True)
    J = kp.shape[1]
    A, g, cost = ops.sphere_collision_normal(start, *tabs, True, fit._pairs(), 1.0)[:3]
    A = A + torch.eye(26, dtype=torch.float64, device="cuda") * 1e3        # (a system the step can factorise)
    pa, pb, pm = fit._pairs()
    rows = torch.empty(B, dtype=torch.int32, device="cuda")
    state, trial = ops.pose_lm_begin(start, 1e-3)
    nxt, par, cst, cst0 = (torch.empty(s, device="cuda") for s in ((B, 26), (B, 26), (B,), (B,)))
    A2, g2, c2 = A.clone(), g.clone(), cost.clone()
    blob = prior.blob
    module = pose_vae.default_pose_vae().cuda()
    x = (kp[..., :3] / 100).reshape(B, 123).contiguous()
    tangents = (jac / 100).permute(2, 0, 1).contiguous()                    # [26,B,123]

    def recon(v):
        return module.decoder(module.mu(module.base(v)))

    def torch_jvp():
        value, d = torch.func.vmap(lambda t: torch.func.jvp(recon, (x,), (t,)), out_dims=(None, 0))(tangents)
        return 100 * (x - value), jac - 100 * d.permute(1, 2, 0)

    runs = {
        "pose_vae": lambda s: lib.shr_pose_vae_normal(p(kp), p(jac), p(blob), blob.shape[0], 0.1, 1.0, B, J, 1, p(A2), p(g2), p(c2),
                                                      None, None, None, None, s),
        "collision": lambda s: lib.shr_sphere_collision_normal(p(kp), p(jac), p(pa), p(pb), p(pm), 1.0, B, J, pa.shape[0], 1, p(A2),
                                                               p(g2), p(c2), p(rows), None, None, s),
        "lm_step": lambda s: lib.shr_pose_lm_step(p(state), p(A), p(g), p(cost), p(trial), None, None, 1, B, p(nxt), p(par), p(cst),
                                                  p(cst0), s),
    }
    for label, fn in runs.items():
        assert fn(stream.cuda_stream) == 0, label
    with torch.no_grad():
        r, Jr = torch_jvp()
    stream.synchronize()
    res = ops.pose_vae_normal(start, *tabs, True, blob, 1.0)[3]
    print("B=%d: torch's r against the entry's: %.3g mm at most" % (B, float((r.double() - res).abs().max())), flush=True)
    us = {k: [] for k in list(runs) + ["torch_jvp"]}
    for rnd in range(ROUNDS):
        order = list(us) if rnd % 2 == 0 else list(us)[::-1]                 # (odd rounds in reverse order)
        for label in order:
            if label == "torch_jvp":
                with torch.no_grad():
                    us[label].append(timed(torch_jvp, stream))
            else:
                us[label].append(bench.mean_launch_us(runs[label], stream, 20, 3, 5, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
    spread = {k: float(max(v) - min(v)) for k, v in us.items()}
    us = {k: float(np.median(v)) for k, v in us.items()}
    print("pose vae B=%d: entry %.2f us (spread %.2f; %d workgroups); collision %.2f us (spread %.2f); lm_step %.2f us (spread %.2f); "
          "torch jvp %.2f us (spread %.2f): the entry is %.2f x the collision entry, %.2f x one step, 1 / %.1f of the torch composition"
          % (B, us["pose_vae"], spread["pose_vae"], B, us["collision"], spread["collision"], us["lm_step"], spread["lm_step"],
             us["torch_jvp"], spread["torch_jvp"], us["pose_vae"] / us["collision"], us["pose_vae"] / us["lm_step"],
             us["torch_jvp"] / us["pose_vae"]), flush=True)
    return us


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    stream = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(stream):
        for B in (32, 256):
            out[B] = entries(mesh, lib, stream, B)
    return out


if __name__ == "__main__":
    main()
