"""Pose -> mesh vertices and back (shr_pose_vertices_fwd / _bwd, pose_vertices.hip), HIP events on the launching stream,
through the C ABI (no Python op in the loop):
  fused     the one-launch forward and the one-launch backward
  composed  shr_fk_fwd + shr_lbs_project, and shr_lbs_vertices_bwd + shr_fk_bwd: the two launches each replaces, with
            T and grad_T in HBM between them
for 256 and 1152 sampled poses on the hand's distinct skin table (NV = 1 721) and its full table (10 144), pixel space
(project = 1, no rand_f), in the same process, alternated, three rounds (every round is printed; the summary is the
median).  The comparison is between the columns of one run, never against an earlier figure.  The outputs of the two
paths are compared bit for bit before anything is timed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model  # noqa: E402
from spherehand_amd.joint_angle import sample_poses  # noqa: E402
from spherehand_amd.kinematicsTransformation import HandTransformationMat  # noqa: E402

ROUNDS = 3
CAMERA = (320.0, 320.0, 640 / 300, 640 / 300)
BATCHES = (256, 1152)


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
    off, inv = fk.offset, fk.offset_inv
    tables = {"distinct": hand_model.unique_skin(mesh)[:3], "full": hand_model.sparse_skin(mesh)}
    cx, cy, fx, fy = CAMERA
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for B in BATCHES:
            params = torch.cat([sample_poses(min(128, B - lo), seed=1 + lo) for lo in range(0, B, 128)]).float().cuda()
            for name, tab in tables.items():
                start, bone, wv = (torch.from_numpy(a).cuda() for a in tab)
                NV = start.numel() - 1
                T = torch.empty(B, 17, 4, 4, device="cuda")
                gT = torch.empty(B, 17, 4, 4, device="cuda")
                v1, v2 = torch.empty(B, NV, 4, device="cuda"), torch.empty(B, NV, 4, device="cuda")
                g1, g2 = torch.empty(B, 26, device="cuda"), torch.empty(B, 26, device="cuda")
                gv = torch.randn(B, NV, 4, device="cuda")

                def fwd_fused(s):
                    return lib.shr_pose_vertices_fwd(p(params), B, p(off), p(inv), NV, p(start), p(bone), p(wv), 1, 1, cx, cy,
                                                     fx, fy, None, p(v1), None, s)

                def fwd_composed(s):
                    return lib.shr_fk_fwd(p(params), B, p(off), p(inv), p(T), s) or \
                        lib.shr_lbs_project(p(T), B, 17, NV, p(start), p(bone), p(wv), 1, 1, cx, cy, fx, fy, None, p(v2), s)

                def bwd_fused(s):
                    return lib.shr_pose_vertices_bwd(p(params), B, p(off), p(inv), NV, p(start), p(bone), p(wv), 1, 1, cx, cy,
                                                     fx, fy, None, p(gv), p(g1), s)

                def bwd_composed(s):
                    return lib.shr_lbs_vertices_bwd(p(gv), B, 17, NV, p(start), p(bone), p(wv), 1, 1, cx, cy, fx, fy, None,
                                                    p(gT), s) or \
                        lib.shr_fk_bwd(p(params), B, p(off), p(inv), p(gT), p(g2), s)

                runs = {"forward fused": fwd_fused, "forward composed": fwd_composed, "backward fused": bwd_fused,
                        "backward composed": bwd_composed}
                for label, fn in runs.items():
                    assert fn(stream.cuda_stream) == 0, label
                stream.synchronize()
                assert torch.equal(v1, v2) and torch.equal(g1, g2), (B, name)
                us = {k: [] for k in runs}
                for rnd in range(ROUNDS):
                    for label, fn in runs.items():
                        us[label].append(bench.mean_launch_us(fn, stream, 100, 3, 10, warm_ms=20.0))
                    print("  round %d: %s" % (rnd, " | ".join("%s %.2f" % (k, v[-1]) for k, v in us.items())), flush=True)
                us = {k: float(np.median(v)) for k, v in us.items()}
                print("pose vertices B=%d NV=%d (%s): forward fused %.2f us, composed %.2f us (x%.2f); backward fused %.2f us, "
                      "composed %.2f us (x%.2f); same bits"
                      % (B, NV, name, us["forward fused"], us["forward composed"], us["forward composed"] / us["forward fused"],
                         us["backward fused"], us["backward composed"], us["backward composed"] / us["backward fused"]),
                      flush=True)


if __name__ == "__main__":
    main()
