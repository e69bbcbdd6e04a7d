"""Torch restatement of the owner raster's gradient at its own resolution (test helper; not a conftest).

tests/mesh_grad_ref.py's construction with ONE tap of weight 1 per pixel: `pixel_depth` is, at every pixel that has an
owner, the raw depth zp recomputed from that owner face exactly as the rasterizer defines it
(depth_rasterization_cuda_kernel.cu:57-110) at the integer pixel, in fp64 through autograd, with the fp32 clamp
decisions of the kernel.  Its gradient is the contract of ops.TriRaster / ops.TriRasterIndexed: the gradient routes to
the owner and holds coverage fixed."""
import numpy as np
import torch

import mesh_grad_ref as ref


def soup_as_indexed(face_vertices):
    """face_vertices [B,F,3,3] -> (vertices [B,3F,3], faces [F,3] int64): corner k of face f is vertex 3 f + k."""
    B, F = face_vertices.shape[:2]
    return face_vertices.reshape(B, 3 * F, 3), np.arange(3 * F, dtype=np.int64).reshape(F, 3)


def random_soup(B, F, W, H, seed):
    """[B,F,3,3] fp32: free triangles of three sizes centred up to 20 px off a W x H image, depths of both signs."""
    rs = np.random.RandomState(seed)
    c = rs.uniform(-20, [W + 20, H + 20], (B, F, 1, 2))
    spread = rs.choice([3.0, 12.0, 40.0], (B, F, 1, 1))
    return np.concatenate([c + rs.normal(0, 1, (B, F, 3, 2)) * spread, rs.uniform(-50, 50, (B, F, 3, 1))], -1).astype(np.float32)


def _owned(owner):
    own = owner.cpu().numpy() if isinstance(owner, torch.Tensor) else np.asarray(owner)
    b, y, x = np.nonzero(own >= 0)
    return own, b, y, x


def pixel_depth(vertices, faces, owner, keep=None):
    """[B,H,W] fp64 tensor: zp of the owner face at every owned pixel, 0 elsewhere; differentiable in `vertices`
    ([B,NV,>=3] tensor, pixel space).  faces [F,3] vertex ids (original corner order).  keep: mesh_grad_ref.face_zp's,
    one row per owned pixel."""
    faces = faces.cpu().numpy().astype(np.int64) if isinstance(faces, torch.Tensor) else np.asarray(faces, np.int64)
    own, b, y, x = _owned(owner)
    B, H, W = own.shape
    out = torch.zeros(B * H * W, dtype=torch.float64, device=vertices.device)
    if len(b) == 0:
        return out.view(B, H, W) + 0.0 * vertices.double().sum()
    zp = ref.face_zp(vertices, faces, (b, own[b, y, x]), x, y, keep)
    out = out.index_add(0, torch.from_numpy((b * H + y) * W + x).to(zp.device), zp)
    return out.view(B, H, W)


def pixel_zp32(vertices, faces, owner):
    """fp32 recomputation of every owned pixel's raw depth with the kernel's operation order (.cu:97-110):
    ((b, y, x) of the owned pixels, zp [N] fp32)."""
    faces = np.asarray(faces, np.int64)
    v32 = vertices.cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices, np.float32)
    own, b, y, x = _owned(owner)
    corners = faces[own[b, y, x]]
    order = ref.sort_order(v32[b[:, None], corners][..., :3])
    p = v32[b[:, None], np.take_along_axis(corners, order, 1)][..., :3].astype(np.float32)
    _, c = ref.clamp_decisions(p, x, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (c[:, 0] + c[:, 1]) + c[:, 2]
        w = [(c[:, k] / s).astype(np.float32) for k in range(3)]
        q = ((w[0] / p[:, 0, 2] + w[1] / p[:, 1, 2]).astype(np.float32) + w[2] / p[:, 2, 2]).astype(np.float32)
        zp = (np.float32(1) / q).astype(np.float32)
    return (b, y, x), zp


def vertex_grad(vertices, faces, owner, grad_depth):
    """d <grad_depth, pixel_depth> / d vertices, fp64 numpy [B,NV,C]."""
    v = vertices.detach().cpu().double().requires_grad_(True)
    d = pixel_depth(v, faces, owner.cpu())
    (d * grad_depth.detach().cpu().double()).sum().backward()
    return v.grad.numpy()
