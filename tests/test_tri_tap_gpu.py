"""What csrc/tri_tap.h's callers share, on the GPU, at a small shape: every backward of the triangle family gives the same
bytes whether fixed_point.h keeps its accumulators in LDS (NV <= 2048) or in global memory (NV = 2049: for the raster's
and the interpolation's walkers also the RUNS instantiation)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, W, H, NX, NY = 2, 97, 61, 6, 5   # 5 917 pixels: two workgroups of either PixelWalk, a width no multiple of 4 or 64
NV = NX * NY
NV_PAD = 2049                       # one more than fixed_point.h's kBwdLdsVerts
SEED = 6                            # (on the CPU, tri_interp_ref.cpu_owners: about 3 600 owned pixels per crop)


def grid_mesh(seed, z_values=None):
    """A jittered NX x NY grid of vertices reaching 8 px off the W x H image, two faces per cell, each of either winding
    (about half are drawn); z uniform in 20 .. 180, or drawn from z_values.  (vertices [B,NV,4] fp32, faces [F,3] int32)"""
    rng = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:NY, 0:NX].astype(np.float64)
    v = np.zeros((B, NV, 4), np.float32)
    v[..., 0] = (gx.ravel() * (W + 16) / (NX - 1) - 8)[None] + rng.uniform(-3, 3, (B, NV))
    v[..., 1] = (gy.ravel() * (H + 16) / (NY - 1) - 8)[None] + rng.uniform(-3, 3, (B, NV))
    v[..., 2] = rng.uniform(20, 180, (B, NV)) if z_values is None else rng.choice(z_values, (B, NV))
    v[..., 3] = 1
    i = (np.arange(NY - 1)[:, None] * NX + np.arange(NX - 1)[None]).ravel()
    a, b, c, d = i, i + 1, i + NX, i + NX + 1
    flip = rng.integers(0, 2, 2 * len(i)).astype(bool)
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([b, c, d], 1)])
    f[flip] = f[flip][:, [1, 0, 2]]
    return v, np.ascontiguousarray(f, np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pad_rows(t, n):
    out = torch.zeros((t.shape[0], n) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def test_lds_and_global_accumulators_give_the_same_bytes():
    from spherehand_amd import ops
    v, f = grid_mesh(SEED)
    verts, faces = dev(v), dev(f)
    gen = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=gen).cuda()  # noqa: E731
    depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, verts, faces)
    owned = (owner >= 0).sum((1, 2)).cpu().numpy()
    assert owned.min() >= 200, owned
    edges = dev(ops.tri_edge_table(f))
    values = torch.clamp(depth, max=100.0).contiguous()
    g, g4, attr = rand(B, H, W), rand(B, 4, H, W), rand(B, NV, 4)
    src, S = 64, 16
    _, mesh_owner = ops.mesh_depth_owner_fwd(verts, faces, S, src, 100.0)
    assert (mesh_owner >= 0).any()
    gm = rand(B, S, S)

    def grads(x, a):
        out = {"raster": ops.tri_raster_indexed_bwd(x, faces, owner, g),
               "antialias": ops.tri_antialias_bwd(values, depth, owner, x, faces, edges, g, False, True)[1],
               "mesh": ops.mesh_depth_bwd(x, faces, mesh_owner, gm, src)}
        out["interp attr"], out["interp vertices"] = ops.tri_interpolate_bwd(a, owner, x, faces, g4)
        return {k: t.cpu().numpy() for k, t in out.items()}

    small, large = grads(verts, attr), grads(pad_rows(verts, NV_PAD), pad_rows(attr, NV_PAD))
    for name in small:
        s, l = small[name], large[name]
        assert s.shape[1] == NV and l.shape[1] == NV_PAD, name
        assert np.isfinite(s).all() and np.abs(s).max(-1).max() > 0, name                 # some row is not zero
        assert s.tobytes() == np.ascontiguousarray(l[:, :NV]).tobytes(), name
        assert not l[:, NV:].view(np.uint32).any(), name                                  # the padded rows: +0 bits
