"""The mesh data-to-model distance (shr_mesh_d2m_fwd / _bwd, mesh_d2m.hip), HIP events on the launching stream:
  ours    forward (records + search) and backward through the C ABI (no Python op in the loop) on sampled hand poses at
          256 crops @128x128 and 1152 @256x256: the observation is each pose's own depth at that size, the model the same
          pose's 640 x 640 vertices moved by (12, 8, 3), pixel_to_model = (640 / S, 0, 640 / S, 0)
  torch   for context, the same definition as a torch composition a user writes without the kernels: per crop the data
          points are gathered, the seven regions evaluated for every (point, face) with torch.where in chunks of faces,
          the minimum taken with its argument; forward only, on TORCH_CROPS crops, reported per crop and scaled to the batch
in the same process, alternated, three rounds (every round is printed; the summary is the median)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses  # noqa: E402
from spherehand_amd.kinematicsTransformation import HandTransformationMat  # noqa: E402
from spherehand_amd.render import DepthRender  # noqa: E402

ROUNDS = 3
FG_MAX = 900.0
MOVE = (12.0, 8.0, 3.0, 0.0)
TORCH_CROPS = 4
TORCH_FACE_CHUNK = 512


def hand_case(mesh, fk, B, S):
    """(observed [B,S,S], the model's vertices [B,NV,4] in the 640 x 640 pixel space, the faces) of B sampled poses"""
    dr = DepthRender(mesh, 128).cuda()
    depth, verts = [], []
    with torch.no_grad():
        for lo in range(0, B, 256):
            n = min(256, B - lo)
            v = dr.lbs(fk(sample_poses(n, seed=1 + lo).cuda()).contiguous(), dr.camera, None).contiguous()
            small = v.clone()
            small[..., :2] *= S / 640.0
            depth.append(ops.tri_raster_indexed_fwd(S, S, small, dr.rasterizer.faces_i32))
            verts.append((v + torch.tensor(MOVE, device="cuda")).contiguous())
    return torch.cat(depth), torch.cat(verts), dr.rasterizer.faces_i32


def torch_dist2(ap, ab, ac):
    """the contract's sequence for ap [N,1,3] against ab, ac [1,F,3] -> d2 [N,F]"""
    dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]   # noqa: E731
    bp, cp = ap - ab, ap - ac
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    den = (va + vb) + vc
    one, zero = torch.ones_like(den), torch.zeros_like(den)
    nv, dv, nw, dw = vb, den, vc, den
    bc = (va <= 0) & (e43 >= 0) & (e56 >= 0)
    for m, a, b, c, d in ((bc, zero, one, e43, e43 + e56), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, one, d2, d2 - d6),
                          ((d6 >= 0) & (d5 <= d6), zero, one, one, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, d1 - d3, zero, one),
                          ((d3 >= 0) & (d4 <= d3), one, one, zero, one), ((d1 <= 0) & (d2 <= 0), zero, one, zero, one)):
        nv, dv, nw, dw = torch.where(m, a, nv), torch.where(m, b, dv), torch.where(m, c, nw), torch.where(m, d, dw)
        if m is not bc:
            bc = bc & ~m
    v, w = nv / dv, nw / dw
    v = torch.where(bc, 1 - w, v).clamp(0, 1)
    w = w.clamp(0, 1)
    e = ap - (v[..., None] * ab + w[..., None] * ac)
    return dot(e, e)


def torch_forward(observed, verts, faces, scale):
    """dist [TORCH_CROPS,S,S] of the first crops"""
    S = observed.shape[1]
    out = torch.zeros_like(observed[:TORCH_CROPS])
    idx = faces.long()
    for b in range(TORCH_CROPS):
        i, j = torch.nonzero(observed[b] < FG_MAX, as_tuple=True)
        p = torch.stack([scale * j.float(), scale * i.float(), observed[b, i, j]], -1)
        a = verts[b, idx[:, 0], :3]
        ab, ac = verts[b, idx[:, 1], :3] - a, verts[b, idx[:, 2], :3] - a
        best = torch.full((len(p),), float("inf"), device="cuda")
        for f0 in range(0, len(idx), TORCH_FACE_CHUNK):
            s = slice(f0, f0 + TORCH_FACE_CHUNK)
            d2 = torch_dist2(p[:, None, :] - a[None, s], ab[None, s], ac[None, s])
            best = torch.minimum(best, torch.nan_to_num(d2, nan=float("inf")).min(1).values)
        out[b, i, j] = best.sqrt()
    return out.view(TORCH_CROPS, S, S)


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
    stream = torch.cuda.Stream()
    inf = float("inf")
    with torch.cuda.stream(stream):
        for B, S in ((256, 128), (1152, 256)):
            observed, verts, faces = hand_case(mesh, fk, B, S)
            NV, F, scale = verts.shape[1], faces.shape[0], 640.0 / S
            dist = torch.empty((B, S, S), dtype=torch.float32, device="cuda")
            face = torch.empty((B, S, S), dtype=torch.int32, device="cuda")
            gd = torch.randn(B, S, S, device="cuda")
            out = torch.empty((B, NV, 4), dtype=torch.float32, device="cuda")
            ws = torch.empty(max(16, lib.shr_mesh_d2m_workspace_bytes(B, F)), dtype=torch.uint8, device="cuda")
            wsb = torch.empty(max(16, lib.shr_mesh_d2m_bwd_workspace_bytes(B, NV)), dtype=torch.uint8, device="cuda")

            def composed(s):   # (on the current stream: the timed one)
                composed.out = torch_forward(observed, verts, faces, scale)
                return 0

            runs = {"forward": lambda s: lib.shr_mesh_d2m_fwd(p(observed), p(verts), p(faces), B, NV, F, S, S, scale, 0.0, scale,
                                                              0.0, FG_MAX, inf, p(dist), p(face), p(ws), s),
                    "backward": lambda s: lib.shr_mesh_d2m_bwd(p(observed), p(verts), p(faces), p(dist), p(face), p(gd), B, NV, F,
                                                               S, S, scale, 0.0, scale, 0.0, FG_MAX, inf, p(out), p(wsb), s),
                    "torch": composed}
            for name, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, name
            stream.synchronize()
            us = {k: [] for k in runs}
            for rnd in range(ROUNDS):
                for name, fn in runs.items():
                    us[name].append(bench.mean_launch_us(fn, stream, 3, 3, 2, warm_ms=20.0))
                print("  round %d: %s" % (rnd, " | ".join("%s %.1f" % (k, v[-1]) for k, v in us.items())), flush=True)
            us = {k: float(np.median(v)) for k, v in us.items()}
            points = (observed < FG_MAX).sum().item()
            err = (composed.out - dist[:TORCH_CROPS]).abs().max().item()
            print("mesh d2m B=%d %dx%d NV=%d F=%d: %.1f %% data points (%.0f per crop), %.3g point-face pairs; mean distance "
                  "%.2f; forward %.1f us (%.1f ps per pair), backward %.1f us; torch composition %.1f us per crop = %.0f us "
                  "scaled to the batch (x%.0f); max |dist - torch| %.3g"
                  % (B, S, S, NV, F, 100.0 * points / observed.numel(), points / B, float(points) * F,
                     dist.sum().item() / max(1, points), us["forward"], us["forward"] * 1e6 / (float(points) * F), us["backward"],
                     us["torch"] / TORCH_CROPS, us["torch"] / TORCH_CROPS * B, us["torch"] / TORCH_CROPS * B / us["forward"], err),
                  flush=True)


if __name__ == "__main__":
    main()
