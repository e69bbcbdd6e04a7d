"""The antialias pass of the triangle raster through the C ABI (no Python op in the loop), HIP events on the launching
stream, hand crops from sampled poses (the 1721 distinct vertices, so the faces' ids are already welded):
  forward          shr_tri_antialias_fwd on clamp(raw, max=100) (values, owners and depths of the owner forward)
  backward         shr_tri_antialias_bwd -> grad_values [B,H,W] and grad_vertices [B,NV,4]
at 256 crops @640x640 and 64 crops @640x480, against a device copy of the values (the copy rate): the forward's floor is
a read of owner and values and a write of the output, 12 bytes per pixel."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses  # noqa: E402
from spherehand_amd.kinematicsTransformation import HandTransformationMat  # noqa: E402
from spherehand_amd.render import DepthRender  # noqa: E402

mesh = hand_model.load_mesh()
lib = _lib.lib()
fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
stream = torch.cuda.Stream()
p = lambda t: t.data_ptr()  # noqa: E731
with torch.cuda.stream(stream):
    for B, W, H in ((256, 640, 640), (64, 640, 480)):
        dr = DepthRender(mesh, 128).cuda()
        with torch.no_grad():
            verts = dr.lbs(fk(sample_poses(B, seed=1).cuda()).contiguous(), dr.camera, None).contiguous()
        faces = dr.rasterizer.faces_i32
        edges = torch.from_numpy(ops.tri_edge_table(faces.cpu())).cuda()
        NV, F = verts.shape[1], faces.shape[0]
        depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, verts, faces)
        values = torch.clamp(depth, max=100.0).contiguous()
        out, copy = torch.empty_like(values), torch.empty_like(values)
        g = torch.randn(B, H, W, device="cuda")
        g_c, g_v = torch.empty_like(values), torch.empty(B, NV, 4, device="cuda")
        ws = torch.empty(lib.shr_tri_antialias_bwd_workspace_bytes(B, NV), dtype=torch.uint8, device="cuda")
        args = lambda: (p(values), p(depth), p(owner), p(verts), p(faces), p(edges), B, NV, F, W, H)  # noqa: E731

        def copy_values(s):   # (on the current stream: the timed one)
            copy.copy_(values)
            return 0

        runs = {
            "copy": copy_values,
            "forward": lambda s: lib.shr_tri_antialias_fwd(*args(), p(out), s),
            "backward": lambda s: lib.shr_tri_antialias_bwd(*args(), p(g), p(g_c), p(g_v), p(ws), s),
            "backward values": lambda s: lib.shr_tri_antialias_bwd(*args(), p(g), p(g_c), None, None, s),
        }
        for name, fn in runs.items():
            assert fn(stream.cuda_stream) == 0, name
        stream.synchronize()
        changed = (out != values).sum().item() / B
        times = {name: bench.mean_launch_us(fn, stream, 20, 3, 3, warm_ms=20.0) for name, fn in runs.items()}
        npix = B * W * H
        copy_rate = 8 * npix / (times["copy"] * 1e-6) / 1e12
        floor_us = 12 * npix / (copy_rate * 1e12) * 1e6
        print("B=%d %dx%d (%.0f owned, %.0f blended pixels per crop; %d unshared edge slots): " %
              (B, W, H, (owner >= 0).sum().item() / B, changed, int((edges < 0).sum()))
              + " | ".join("%s %.1f us" % kv for kv in times.items())
              + " | copy %.2f TB/s, forward %.2f B/px at %.2f TB/s effective, floor %.1f us (x%.2f)"
              % (copy_rate, 12.0, 12 * npix / (times["forward"] * 1e-6) / 1e12, floor_us, times["forward"] / floor_us),
              flush=True)
