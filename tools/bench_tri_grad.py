"""The triangle raster at its own resolution and its backward, through the C ABI (no Python op in the loop), HIP events on
the launching stream, hand crops from sampled poses:
  forward          depth_rasterization.forward (shr_tri_raster_fwd, face soups [B,3382,3,3])
  owner forward    shr_tri_raster_owner_fwd (soups) and shr_tri_raster_indexed_owner_fwd (the 1721 distinct vertices)
  backward         shr_tri_raster_bwd (soups -> [B,F,3,3]) and shr_tri_raster_indexed_bwd (-> [B,NV,4])
at 256 crops @640x640 and 64 crops @640x480 (rows 0 .. 479 of the 640 x 640 camera)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model  # noqa: E402
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
        NV, F = verts.shape[1], faces.shape[0]
        fv = verts[:, faces.long(), 0:3].contiguous()
        depth = torch.empty(B, H, W, device="cuda")
        d_own = torch.empty_like(depth)
        owner = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
        owner_i = torch.empty_like(owner)
        g = torch.randn(B, H, W, device="cuda")
        g_fv = torch.empty(B, F, 3, 3, device="cuda")
        g_v = torch.empty(B, NV, 4, device="cuda")
        ws = torch.empty(lib.shr_tri_raster_bwd_workspace_bytes(B, F), dtype=torch.uint8, device="cuda")
        ws_i = torch.empty(lib.shr_tri_raster_indexed_bwd_workspace_bytes(B, NV), dtype=torch.uint8, device="cuda")
        runs = {
            "forward": lambda s: lib.shr_tri_raster_fwd(p(fv), B, F, W, H, p(depth), s),
            "owner forward": lambda s: lib.shr_tri_raster_owner_fwd(p(fv), B, F, W, H, p(d_own), p(owner), s),
            "owner forward indexed": lambda s: lib.shr_tri_raster_indexed_owner_fwd(p(verts), p(faces), B, NV, F, W, H,
                                                                                    p(d_own), p(owner_i), s),
            "backward": lambda s: lib.shr_tri_raster_bwd(p(fv), p(owner), p(g), B, F, W, H, p(g_fv), p(ws), s),
            "backward indexed": lambda s: lib.shr_tri_raster_indexed_bwd(p(verts), p(faces), p(owner_i), p(g), B, NV, F, W, H,
                                                                         p(g_v), p(ws_i), s),
        }
        for name, fn in runs.items():
            assert fn(stream.cuda_stream) == 0, name
        stream.synchronize()
        same = torch.equal(depth, d_own)
        owned = (owner >= 0).sum().item() / B
        times = {name: bench.mean_launch_us(fn, stream, 20, 3, 3, warm_ms=20.0) for name, fn in runs.items()}
        print("B=%d %dx%d (%.0f owned pixels per crop, owner depth bits equal: %s): " % (B, W, H, owned, same)
              + " | ".join("%s %.1f us" % kv for kv in times.items()), flush=True)
