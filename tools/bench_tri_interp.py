"""Vertex-attribute interpolation through the C ABI (no Python op in the loop), HIP events on the launching stream, hand
crops from sampled poses (the 1721 distinct vertices), C = 3 and C = 17 per-crop attributes:
  forward             shr_tri_interp_fwd on the owners of the owner forward
  backward            shr_tri_interp_bwd -> grad_attr [B,NV,C] and grad_vertices [B,NV,4]; each part alone
at 256 crops @640x640 and 64 crops @640x480, against
  copy                a device copy of the output's bytes (the copy rate): the forward's floor is a read of the owner and
                      a write of C planes, 4 + 4 C bytes per pixel
  torch               the composition a user writes without the kernel (gather of faces[owner] and of the corners,
                      barycentric set-up, clamp, normalise, weighted sum) and its autograd backward, on the same inputs."""
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


def torch_interp(attr, owner, verts, faces):
    B, H, W = owner.shape
    ids = faces.long()[owner.clamp(min=0).long()]                                   # [B,H,W,3]
    bi = torch.arange(B, device=owner.device)[:, None, None, None]
    P = verts[bi, ids]                                                              # [B,H,W,3,4]
    x, y = P[..., 0], P[..., 1]
    py, px = torch.meshgrid(torch.arange(H, device=owner.device, dtype=torch.float32),
                            torch.arange(W, device=owner.device, dtype=torch.float32), indexing="ij")
    px, py = px[None, :, :, None], py[None, :, :, None]
    den = (x[..., 1] - x[..., 0]) * (y[..., 2] - y[..., 0]) - (x[..., 2] - x[..., 0]) * (y[..., 1] - y[..., 0])
    xb, yb, xe, ye = x[..., [1, 2, 0]], y[..., [1, 2, 0]], x[..., [2, 0, 1]], y[..., [2, 0, 1]]
    c = (((xb - px) * (ye - py) - (xe - px) * (yb - py)) / den[..., None]).clamp(0, 1)
    wh = c / c.sum(-1, keepdim=True)
    out = (wh[..., None] * attr[bi, ids]).sum(3)                                    # [B,H,W,C]
    return torch.where((owner >= 0)[..., None], out, torch.zeros((), device=out.device)).permute(0, 3, 1, 2)


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
        depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, verts, faces)
        npix = B * W * H
        for C in (3, 17):
            attr = torch.randn(B, NV, C, device="cuda")
            out = torch.empty(B, C, H, W, device="cuda")
            copy = torch.empty_like(out)
            g = torch.randn(B, C, H, W, device="cuda")
            g_a, g_v = torch.empty(B, NV, C, device="cuda"), torch.empty(B, NV, 4, device="cuda")
            ws = torch.empty(lib.shr_tri_interp_bwd_workspace_bytes(B, NV, C, 1, 1), dtype=torch.uint8, device="cuda")
            args = lambda: (p(owner), p(verts), p(faces), p(attr), NV * C, B, NV, F, W, H, C)  # noqa: E731

            def copy_out(s):   # (on the current stream: the timed one)
                copy.copy_(out)
                return 0

            runs = {
                "copy": copy_out,
                "forward": lambda s: lib.shr_tri_interp_fwd(*args(), p(out), s),
                "backward": lambda s: lib.shr_tri_interp_bwd(*args(), p(g), p(g_a), p(g_v), p(ws), s),
                "backward attr": lambda s: lib.shr_tri_interp_bwd(*args(), p(g), p(g_a), None, p(ws), s),
                "backward vertices": lambda s: lib.shr_tri_interp_bwd(*args(), p(g), None, p(g_v), p(ws), s),
            }
            for name, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, name
            stream.synchronize()
            times = {name: bench.mean_launch_us(fn, stream, 10, 3, 3, warm_ms=20.0) for name, fn in runs.items()}
            del copy
            # the torch composition, a few crops at a time where the [B,H,W,3,C] intermediates would not fit
            chunk = 32
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            tf = tb = 0.0
            for rep in range(2):                                    # (the first repetition warms up)
                tf = tb = 0.0
                for i in range(0, B, chunk):
                    sl = slice(i, i + chunk)
                    a_, v_ = attr[sl].clone().requires_grad_(True), verts[sl].clone().requires_grad_(True)
                    ev[0].record()
                    o = torch_interp(a_, owner[sl], v_, faces)
                    ev[1].record()
                    torch.autograd.grad(o, (a_, v_), g[sl])
                    ev[2].record()
                    ev[2].synchronize()
                    tf += ev[0].elapsed_time(ev[1]) * 1e3
                    tb += ev[1].elapsed_time(ev[2]) * 1e3
                    del o, a_, v_
            copy_rate = 8 * C * npix / (times["copy"] * 1e-6) / 1e12
            floor_us = (4 + 4 * C) * npix / (copy_rate * 1e12) * 1e6
            print("B=%d %dx%d C=%d (%.0f owned pixels per crop, NV %d): " % (B, W, H, C, (owner >= 0).sum().item() / B, NV)
                  + " | ".join("%s %.1f us" % kv for kv in times.items())
                  + " | torch forward %.0f us, backward %.0f us" % (tf, tb)
                  + " | copy %.2f TB/s, forward floor %.1f us (x%.2f)" % (copy_rate, floor_us, times["forward"] / floor_us),
                  flush=True)
            del out, g, attr
