"""Torch restatement of the differentiable mesh depth's gradient (test helper; not a conftest).

Given the vertices [B,NV,>=3] (pixel space), the faces [F,3] and the forward's owners [B,S,S,4], `owner_depth` is
sum over every output pixel's owner taps of (bilinear weight) x zp, where zp is the tap's raw depth recomputed from its
owner face exactly as the rasterizer defines it (depth_rasterization_cuda_kernel.cu:57-110): corners sorted by x, the
barycentric weights clamped to [0, 1] and normalised, zp = 1 / sum_k w_k / z_k.  Its autograd gradient is the kernel's
contract: the gradient routes to the owner and holds coverage fixed.

The clamp decisions (which weights are strictly outside [0, 1]) are taken in fp32 with the kernel's arithmetic; the
derivatives are evaluated in fp64 through autograd.  The bilinear taps follow ATen (align_corners=False)."""
import numpy as np
import torch


def axis_taps(S, src=640):
    """ATen's bilinear source indices and weights of one axis: (i0, i1, l0, l1) as [S] int64 / fp32 arrays."""
    scale = np.float32(src) / np.float32(S)
    d = np.arange(S)
    # scale * (d + 0.5) - 0.5 with one rounding (the kernel's fma): exact in fp64, then rounded once
    s = (np.float64(scale) * (d + 0.5) - 0.5).astype(np.float32)
    s = np.maximum(s, np.float32(0))
    i0 = np.minimum(s.astype(np.int64), src - 1)
    i1 = i0 + (i0 < src - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def tap_grid(S, src=640):
    """[S,S,4] source (x, y) and weight of every output pixel's four taps, ATen order y0x0, y0x1, y1x0, y1x1."""
    xi0, xi1, xl0, xl1 = axis_taps(S, src)
    yi0, yi1, yl0, yl1 = axis_taps(S, src)
    xs = np.stack([xi0, xi1, xi0, xi1], -1)[None, :, :].repeat(S, 0)
    ys = np.stack([yi0, yi0, yi1, yi1], -1)[:, None, :].repeat(S, 1)
    wx = np.stack([xl0, xl1, xl0, xl1], -1).astype(np.float64)
    wy = np.stack([yl0, yl0, yl1, yl1], -1).astype(np.float64)
    w = wy[:, None, :] * wx[None, :, :]
    return xs, ys, w


def sort_order(fv32):
    """The rasterizer's sort of a face's corners by x: [..., 3] original corner index of sorted corners 0, 1, 2."""
    x0, x1, x2 = fv32[..., 0, 0], fv32[..., 1, 0], fv32[..., 2, 0]
    c = x0 < x1
    p0 = np.where(c, np.where(x2 < x0, 2, 0), np.where(x2 < x1, 2, 1))
    p2 = np.where(c, np.where(x1 < x2, 2, 1), np.where(x0 < x2, 2, 0))
    return np.stack([p0, 3 - p0 - p2, p2], -1)


def clamp_decisions(p32, xf, yf):
    """fp32 weights of the sorted corners p32 [...,3,3] at pixel (xf, yf), with the kernel's operation order:
    (pass [...,3]: weight inside [0, 1], clamped weight [...,3])."""
    f = np.float32
    p = p32.astype(np.float32)
    P = lambda a, d: p[..., a, d]
    fi = [P(1, 1) - P(2, 1), P(2, 0) - P(1, 0), P(1, 0) * P(2, 1) - P(2, 0) * P(1, 1),
          P(2, 1) - P(0, 1), P(0, 0) - P(2, 0), P(2, 0) * P(0, 1) - P(0, 0) * P(2, 1),
          P(0, 1) - P(1, 1), P(1, 0) - P(0, 0), P(0, 0) * P(1, 1) - P(1, 0) * P(0, 1)]
    den = (P(2, 0) * (P(0, 1) - P(1, 1)) + P(0, 0) * (P(1, 1) - P(2, 1))) + P(1, 0) * (P(2, 1) - P(0, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        fi = [(a / den).astype(np.float32) for a in fi]
        xf, yf = f(xf) if np.isscalar(xf) else xf.astype(np.float32), f(yf) if np.isscalar(yf) else yf.astype(np.float32)
        w = np.stack([(fi[3 * k] * xf + fi[3 * k + 1] * yf) + fi[3 * k + 2] for k in range(3)], -1).astype(np.float32)
    return (w >= 0) & (w <= 1), np.clip(w, 0, 1).astype(np.float32)


def face_zp(vertices, faces, face, xi, yi, keep=None):
    """zp of face[i] at source pixel (xi[i], yi[i]) for the flat lists face / xi / yi (crop index bi in vertices'
    first axis given as a pair (bi, face)): differentiable (fp64) in `vertices`.  vertices: [B,NV,>=3] tensor.
    keep: a dict that receives the gathered sorted corners `p` [N,3,3] (its gradient retained: after a backward, p.grad
    holds every tap's nine terms), their crop `bi` [N] and their vertex ids `sorted_ids` [N,3]
    (tests/fixed_point_ref.py)."""
    bi, f = face
    f = np.asarray(f, np.int64)
    bi = np.asarray(bi, np.int64)
    corners = faces[f]                                                  # [N,3] vertex ids (original corner order)
    v32 = vertices.detach().cpu().float().numpy()
    fv32 = v32[bi[:, None], corners][..., :3]                           # [N,3,3]
    order = sort_order(fv32)                                            # [N,3]
    sorted_ids = np.take_along_axis(corners, order, 1)
    p32 = v32[bi[:, None], sorted_ids][..., :3]
    ok, c32 = clamp_decisions(p32, np.asarray(xi), np.asarray(yi))
    V = vertices.double()
    p = V[torch.from_numpy(bi)[:, None], torch.from_numpy(sorted_ids)][..., :3]   # [N,3,3] fp64, differentiable
    if keep is not None:
        if p.requires_grad:
            p.retain_grad()
        keep.update(p=p, bi=bi, sorted_ids=sorted_ids)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    px = torch.from_numpy(np.asarray(xi, np.float64))[:, None].to(V.device)
    py = torch.from_numpy(np.asarray(yi, np.float64))[:, None].to(V.device)
    den = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    b_, e_ = [1, 2, 0], [2, 0, 1]
    n = (x[:, b_] - px) * (y[:, e_] - py) - (x[:, e_] - px) * (y[:, b_] - py)
    w = n / den[:, None]
    c = torch.where(torch.from_numpy(ok).to(V.device), w, torch.from_numpy(c32).double().to(V.device))
    s = c.sum(1, keepdim=True)
    q = (c / s / z).sum(1)
    return 1.0 / q


def owner_depth(vertices, faces, owner, src=640, keep=None):
    """sum over all crops, pixels and owner taps of (bilinear weight) x zp(owner face at the tap), as a [B,S,S] fp64
    tensor of per-pixel sums (taps without an owner contribute nothing).  Its gradient w.r.t. vertices is the
    differentiable mesh depth's.  keep: face_zp's, one row per owner tap."""
    own = owner.cpu().numpy() if isinstance(owner, torch.Tensor) else np.asarray(owner)
    faces = faces.cpu().numpy().astype(np.int64) if isinstance(faces, torch.Tensor) else np.asarray(faces, np.int64)
    B, S = own.shape[0], own.shape[1]
    xs, ys, wt = tap_grid(S, src)
    b, yy, xx, t = np.nonzero(own >= 0)
    out = torch.zeros(B * S * S, dtype=torch.float64, device=vertices.device)
    if len(b) == 0:
        return out.view(B, S, S) + 0.0 * vertices.double().sum()
    zp = face_zp(vertices, faces, (b, own[b, yy, xx, t]), xs[yy, xx, t], ys[yy, xx, t], keep)
    contrib = zp * torch.from_numpy(wt[yy, xx, t]).to(zp.device)
    out = out.index_add(0, torch.from_numpy((b * S + yy) * S + xx).to(zp.device), contrib)
    return out.view(B, S, S)


def owner_zp32(vertices, faces, owner, src=640):
    """fp32 recomputation of every owner tap's raw depth with the kernel's operation order (.cu:97-110): (indices
    (b, y, x, t) of the owner taps, zp [N] fp32)."""
    own = owner.cpu().numpy() if isinstance(owner, torch.Tensor) else np.asarray(owner)
    faces = np.asarray(faces, np.int64)
    v32 = vertices.cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices, np.float32)
    S = own.shape[1]
    xs, ys, _ = tap_grid(S, src)
    b, yy, xx, t = np.nonzero(own >= 0)
    f = own[b, yy, xx, t].astype(np.int64)
    corners = faces[f]
    order = sort_order(v32[b[:, None], corners][..., :3])
    p = v32[b[:, None], np.take_along_axis(corners, order, 1)][..., :3].astype(np.float32)
    _, c = clamp_decisions(p, xs[yy, xx, t], ys[yy, xx, t])
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (c[:, 0] + c[:, 1]) + c[:, 2]
        w = [(c[:, k] / s).astype(np.float32) for k in range(3)]
        q = ((w[0] / p[:, 0, 2] + w[1] / p[:, 1, 2]).astype(np.float32) + w[2] / p[:, 2, 2]).astype(np.float32)
        zp = (np.float32(1) / q).astype(np.float32)
    return (b, yy, xx, t), zp
