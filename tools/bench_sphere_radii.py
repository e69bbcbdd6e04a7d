"""The radius term and the arrowhead step of the sphere model's calibration (shr_sphere_icp_radii_normal, sphere_icp_radii.hip;
shr_pose_lm_shared_step, lm_shared.hip), HIP events on the launching stream, through the C ABI (no Python op in the loop).  At
the start poses and the shipped radii:
  radii_normal   shr_sphere_icp_radii_normal (a NEW entry): sphere_icp_scan.h's scan with sixteen moments, the assembly with
                 C, and the group pass
  icp_normal     shr_sphere_icp_normal of THIS build on the same inputs: the same scan with twelve moments
  parent_normal  shr_sphere_icp_normal of the PARENT commit's library (--parent-lib), loaded beside this one
  shared_step    shr_pose_lm_shared_step with K = 41 and the solve (a NEW entry): four launches, parallel over the frames
  lm_step        shr_pose_lm_step on the same A, g: one wave per frame, no shared block
  seq_step       shr_pose_lm_seq_step with E = 0 on the same A, g: one wave per group, a latency chain of its frames
for 256 frames at 128 x 128 with one view as 32 groups of 8 frames and as 8 groups of 32, the hand's 41 spheres, sphere-rendered
observations, starts 0.1 rad / 2 mm off; in the same process, alternated, three rounds, the odd ones in reverse order (every
round is printed; the summary is the median, the spread is max - min over the rounds).  These are first measurements: no target
is set for the new entries.  The one condition, because shr_sphere_icp_normal's scan now lives in a header both units include:
its median in this build is not above the parent library's by more than the run-to-run spread (the larger of the two);
the tool exits with status 1 where it is missed, and says so where no parent library was given (status 0: nothing to hold)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import SphereRadiiCalibrator  # noqa: E402
from tools.bench_sphere_icp import VIEWS  # noqa: E402

ROUNDS = 3
ITERS = 10
SIGMA_K = 5.0


def load_parent(path):
    """The parent commit's library beside this build's: its own handle, the one entry's signature set from this loader's."""
    h = ctypes.CDLL(os.path.abspath(path))
    args, res = _lib.SIGNATURES["shr_sphere_icp_normal"]
    h.shr_sphere_icp_normal.argtypes, h.shr_sphere_icp_normal.restype = args, res
    return h


def one_shape(mesh, lib, parent, stream, B, N, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    V, G = 1, B // N
    stiffness = np.array([1.0] * 3 + [0.0] * 3 + [1.0] * 20, np.float32)
    fit = SphereRadiiCalibrator(mesh, S, S, N, iters=ITERS, stiffness=stiffness).cuda()
    off, inv, bone, wv, radii = fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv, fit.radii
    J = fit.num_spheres
    gen = torch.Generator().manual_seed(B + N)
    truth = sample_poses_batched(B, generator=gen)
    truth[:, 3:5] = 5.0 * torch.randn(B, 2, generator=gen)
    truth[:, 5] = 50.0
    start = truth + 0.1 * torch.randn(B, 26, generator=gen)
    start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
    factors = 0.7 + 0.4 * torch.rand(G, J, generator=gen)
    noise = SIGMA_K * torch.randn(B, V, J, 3, generator=gen)
    truth, start = truth.float().cuda(), start.float().cuda()
    true = (radii[None] * factors.cuda()).contiguous()
    view = torch.stack(VIEWS[:V]).cuda().expand(B, V, 4, 4).contiguous()
    kp, _ = ops.pose_keypoints_jacobian(truth, off, inv, bone, wv, True)
    spheres = ops.view_vertices(kp, view).clone()
    targets = (spheres[..., :3] + noise.cuda()).contiguous()
    spheres[..., 3] = true.repeat_interleave(N, 0)[:, None]
    observed = torch.clamp(ops.sphere_raster_fwd(spheres.view(B * V, J, 4).contiguous(), S, S), max=100.0).view(B, V, S, S).contiguous()
    q, fitted, c0, c = fit.solve(observed, start, view, keypoints=targets)
    stream.synchronize()
    print("B=%d as %d groups x %d frames, %dx%d, shape_stiffness %g, sigma_k %g mm; %d iterations: cost < cost0 on %d of %d "
          "groups; mean |radius - true| %.2f mm at the start, %.2f calibrated"
          % (B, G, N, S, S, fit.shape_stiffness[0].item(), SIGMA_K, ITERS, int((c < c0).sum()), G,
             (radii[None] - true).abs().mean().item(), (fitted - true).abs().mean().item()), flush=True)
    ax, bx, ay, by = fit.pixel_to_model
    fg, md = fit.fg_max, fit.max_dist
    f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    keypoints, jac, view_centres = f32(B, J, 4), f32(B, 3 * J, 26), f32(B, V, J, 4)
    A, g, cost, C, R, gs, E = f64(B, 26, 26), f64(B, 26), f64(B), f64(B, 26, J), f64(G, J, J), f64(G, J), torch.zeros(
        B, 26, 26, dtype=torch.float64, device="cuda")
    A1, g1, cost1, count = f64(B, 26, 26), f64(B, 26), f64(B), i32(B)
    group_radii = radii[None].expand(G, J).contiguous()
    ws = torch.empty(max(16, lib.shr_sphere_icp_radii_normal_workspace_bytes(B, V, J, S, S)), dtype=torch.uint8, device="cuda")
    lm_ws = f64(lib.shr_pose_lm_shared_workspace_bytes(B, G, J) // 8)
    seq_ws = f64(lib.shr_pose_lm_seq_workspace_bytes(B) // 8)
    sh_state, sh_trial, sh_shape = ops.pose_lm_shared_begin(start, group_radii, N, 1e-3)
    lm_state, lm_trial = ops.pose_lm_begin(start, 1e-3)
    seq_state, seq_trial = ops.pose_lm_seq_begin(start, N, 1e-3)
    nxt, nxt_shape, par, shape = f32(B, 26), f32(G, J), f32(B, 26), f32(G, J)
    cst, cst0, cstB, cstB0 = f32(G), f32(G), f32(B), f32(B)
    mu, nu = fit.stiffness, fit.shape_stiffness
    s0 = stream.cuda_stream
    for rc in (lib.shr_pose_keypoints_jacobian(p(sh_trial), B, p(off), p(inv), J, p(bone), p(wv), 1, p(keypoints), p(jac), s0),
               lib.shr_view_vertices_fwd(p(keypoints), p(view), B, V, J, p(view_centres), s0)):
        assert rc == 0

    def radii_normal(s):
        return lib.shr_sphere_icp_radii_normal(p(observed), p(view_centres), p(group_radii), p(view), p(jac), B, V, J, S, S, N, ax,
                                               bx, ay, by, fg, md, p(A), p(g), p(cost), p(count), p(C), p(R), p(gs), None, None,
                                               None, p(ws), s)

    def normal_of(h):
        return lambda s: h.shr_sphere_icp_normal(p(observed), p(view_centres), p(radii), p(view), p(jac), B, V, J, S, S, ax, bx, ay,
                                                 by, fg, md, p(A1), p(g1), p(cost1), p(count), None, None, None, p(ws), s)

    def shared_step(s):
        return lib.shr_pose_lm_shared_step(p(sh_state), p(A), p(g), p(C), p(R), p(gs), p(cost), p(sh_trial), p(sh_shape), None,
                                           p(mu), None, p(nu), 1, B, N, J, p(nxt), p(nxt_shape), p(par), p(shape), p(cst), p(cst0),
                                           p(lm_ws), s)

    def lm_step(s):
        return lib.shr_pose_lm_step(p(lm_state), p(A), p(g), p(cost), p(lm_trial), None, p(mu), 1, B, p(nxt), p(par), p(cstB),
                                    p(cstB0), s)

    def seq_step(s):
        return lib.shr_pose_lm_seq_step(p(seq_state), p(A), p(g), p(E), p(cost), p(seq_trial), None, p(mu), 1, B, N, p(nxt), p(par),
                                        p(cst), p(cst0), p(seq_ws), s)

    runs = {"radii_normal": radii_normal, "icp_normal": normal_of(lib)}
    if parent is not None:
        runs["parent_normal"] = normal_of(parent)
    runs.update(shared_step=shared_step, lm_step=lm_step, seq_step=seq_step)
    for label, fn in runs.items():
        assert fn(s0) == 0, label
    stream.synchronize()
    assert torch.equal(A.view(torch.int64), A1.view(torch.int64)) and torch.equal(g.view(torch.int64), g1.view(torch.int64))
    us = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for label, fn in (list(runs.items()) if rnd % 2 == 0 else list(runs.items())[::-1]):      # (odd rounds in reverse order)
            us[label].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
    spread = {k: float(max(v) - min(v)) for k, v in us.items()}
    us = {k: float(np.median(v)) for k, v in us.items()}
    print("sphere radii B=%d as %d groups x %d frames, %dx%d: radii_normal %.2f us (spread %.2f), %.2f x icp_normal %.2f us "
          "(spread %.2f); shared_step %.2f us (spread %.2f) beside lm_step %.2f us and seq_step %.2f us (a chain of %d frames)"
          % (B, G, N, S, S, us["radii_normal"], spread["radii_normal"], us["radii_normal"] / us["icp_normal"], us["icp_normal"],
             spread["icp_normal"], us["shared_step"], spread["shared_step"], us["lm_step"], us["seq_step"], N), flush=True)
    within = True
    if parent is not None:
        within = us["icp_normal"] - us["parent_normal"] <= max(spread["icp_normal"], spread["parent_normal"])
        print("  shr_sphere_icp_normal: this build %.2f us (spread %.2f) beside the parent's %.2f us (spread %.2f): the difference "
              "%.2f us is %s the spread" % (us["icp_normal"], spread["icp_normal"], us["parent_normal"], spread["parent_normal"],
                                            us["icp_normal"] - us["parent_normal"], "within" if within else "SLOWER than"), flush=True)
    us["within"] = within
    return us


def main(parent_lib=None):
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    parent = load_parent(parent_lib) if parent_lib else None
    if parent is None:
        print("no --parent-lib: shr_sphere_icp_normal is not held against the parent commit's library", flush=True)
    stream = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(stream):
        for N in (8, 32):
            out[N] = one_shape(mesh, lib, parent, stream, 256, N, 128)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None, help="libspherehand_hip.so built from the parent commit")
    sys.exit(0 if all(r["within"] for r in main(ap.parse_args().parent_lib).values()) else 1)
