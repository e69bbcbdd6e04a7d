"""Keypoints -> pose (shr_pose_ik_fwd / _bwd, shr_pose_keypoints_jacobian, pose_ik.hip), HIP events on the launching
stream, through the C ABI (no Python op in the loop):
  solver     12 Levenberg-Marquardt iterations from starts p* + N(0, 0.1) rad / N(0, 2 mm) on exact keypoints
  jacobian   the keypoints and their Jacobian
  backward   the implicit-function gradient at the solved pose
  spheres    for scale: 12 x (shr_pose_spheres_fwd + shr_pose_spheres_bwd), the launches 12 steps of a first-order fit of
             the same keypoints would make (the optimiser's own work not counted)
for 256 and 1152 sampled poses on the hand's 41 keypoints, in the same process, alternated, three rounds (every round
is printed; the summary is the median).  First measurements: no target is set.  The solved poses are compared with p*
before anything is timed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.kinematicsTransformation import HandTransformationMat, keypoint_skinning  # noqa: E402

ROUNDS = 3
BATCHES = (256, 1152)
ITERS = 12


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
    off, inv = fk.offset, fk.offset_inv
    lbs = keypoint_skinning(mesh).cuda()
    bone, wv, bstart, bpoints = lbs.kp_bone, lbs.skin_wv, lbs.kp_bone_start, lbs.kp_bone_points
    J = bone.numel()
    radii = torch.ones(J, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for B in BATCHES:
            gen = torch.Generator().manual_seed(B)
            truth = sample_poses_batched(B, generator=gen)
            start = truth + 0.1 * torch.randn(B, 26, generator=gen)
            start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
            truth, start = truth.float().cuda(), start.float().cuda()
            sph = torch.empty(B, J, 4, device="cuda")
            assert lib.shr_pose_spheres_fwd(p(truth), B, p(off), p(inv), J, p(bone), p(wv), p(radii), 1, p(sph), None,
                                            stream.cuda_stream) == 0
            target = sph[..., :3].contiguous()
            out, c0, c = torch.empty(B, 26, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
            kp, jac = torch.empty(B, J, 4, device="cuda"), torch.empty(B, 3 * J, 26, device="cuda")
            gp, gt = torch.randn(B, 26, device="cuda"), torch.empty(B, J, 3, device="cuda")
            gs, gq = torch.randn(B, J, 4, device="cuda"), torch.empty(B, 26, device="cuda")

            def solver(s):
                return lib.shr_pose_ik_fwd(p(target), p(start), B, p(off), p(inv), J, p(bone), p(wv), 1, None, 0, None, ITERS,
                                           1e-3, p(out), p(c0), p(c), s)

            def jacobian(s):
                return lib.shr_pose_keypoints_jacobian(p(truth), B, p(off), p(inv), J, p(bone), p(wv), 1, p(kp), p(jac), s)

            def backward(s):
                return lib.shr_pose_ik_bwd(p(out), p(gp), B, p(off), p(inv), J, p(bone), p(wv), 1, None, 0, None, p(gt), s)

            def spheres(s):
                rc = 0
                for _ in range(ITERS):
                    rc = rc or lib.shr_pose_spheres_fwd(p(start), B, p(off), p(inv), J, p(bone), p(wv), p(radii), 1, p(sph), None, s)
                    rc = rc or lib.shr_pose_spheres_bwd(p(start), B, p(off), p(inv), J, p(bstart), p(bpoints), p(wv), 1, p(gs),
                                                        p(gq), s)
                return rc

            runs = {"solver": solver, "jacobian": jacobian, "backward": backward, "spheres": spheres}
            for label, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, label
            stream.synchronize()
            err = (out - truth).abs().max().item()
            print("B=%d: max |p - p*| %.3g after %d iterations, cost %.3g from %.3g" % (B, err, ITERS, c.max().item(), c0.max().item()),
                  flush=True)
            assert err < 1e-3, err
            us = {k: [] for k in runs}
            for rnd in range(ROUNDS):
                for label, fn in runs.items():
                    us[label].append(bench.mean_launch_us(fn, stream, 50, 3, 5, warm_ms=20.0))
                print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
            us = {k: float(np.median(v)) for k, v in us.items()}
            print("pose ik B=%d J=%d: solver (%d iterations) %.2f us, jacobian %.2f us, backward %.2f us; for scale %d x "
                  "(pose_spheres fwd + bwd) %.2f us" % (B, J, ITERS, us["solver"], us["jacobian"], us["backward"], ITERS,
                                                          us["spheres"]), flush=True)


if __name__ == "__main__":
    main()
