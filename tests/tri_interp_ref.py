"""Restatements of the vertex-attribute interpolation (include/spherehand_hip.h, shr_tri_interp_fwd / _bwd; test helper,
not a conftest).

(a) `interp32`: steps 1-3 of the contract in numpy fp32, one rounding per written operator -- the kernel's bits.
(b) `interp64`: the same value in fp64 torch, differentiable in `attr` and `vertices`, with the fp32 clamp decisions
    fixed: tests/mesh_grad_ref.py's `face_zp` construction with sum_k wh_k a_k in place of the depth.  Its autograd
    gradient is the contract of shr_tri_interp_bwd (coverage and owner held fixed).
`cpu_owners` restates the second pass of the global-atomic owner kernel (the smallest face whose recomputed fp32 depth
has the raster's bits at the pixel) for tests that have no GPU."""
import os

import numpy as np
import torch

from mesh_grad_ref import clamp_decisions, sort_order


def _np(a, dtype=None):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def taps(owner, vertices, faces):
    """The owned pixels whose face and vertex ids are in range: (b, y, x, sorted vertex ids [N,3], sorted corners p
    [N,3,3] fp32, order [N,3])."""
    own, v32, faces = _np(owner), _np(vertices, np.float32), _np(faces, np.int64)
    F, NV = len(faces), v32.shape[1]
    b, y, x = np.nonzero((own >= 0) & (own < F))
    corners = faces[own[b, y, x]].reshape(-1, 3)
    ok = ((corners >= 0) & (corners < NV)).all(1)
    b, y, x, corners = b[ok], y[ok], x[ok], corners[ok]
    order = sort_order(v32[b[:, None], corners][..., :3]) if len(b) else np.zeros((0, 3), np.int64)
    sid = np.take_along_axis(corners, order, 1)
    p = v32[b[:, None], sid][..., :3].astype(np.float32)
    return b, y, x, sid, p, order


def face_matrix32(p):
    """tri_face.h face_matrix in fp32: (fi: nine [N] arrays already divided by den, den [N], the nine numerators)."""
    P = lambda a, d: p[..., a, d]   # noqa: E731
    num = [P(1, 1) - P(2, 1), P(2, 0) - P(1, 0), P(1, 0) * P(2, 1) - P(2, 0) * P(1, 1),
           P(2, 1) - P(0, 1), P(0, 0) - P(2, 0), P(2, 0) * P(0, 1) - P(0, 0) * P(2, 1),
           P(0, 1) - P(1, 1), P(1, 0) - P(0, 0), P(0, 0) * P(1, 1) - P(1, 0) * P(0, 1)]
    den = (P(2, 0) * (P(0, 1) - P(1, 1)) + P(0, 0) * (P(1, 1) - P(2, 1))) + P(1, 0) * (P(2, 1) - P(0, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        fi = [(a / den).astype(np.float32) for a in num]
    return fi, den, num


def weights32(p, x, y):
    """Steps 1 and 2 at pixels (x, y) of the sorted corners p [N,3,3]: (w [N,3] unclamped, c [N,3] clamped -- a NaN
    clamps to 0, fminf(fmaxf(w, 0), 1) --, s [N], wh [N,3] = c / s), all fp32."""
    p = p.astype(np.float32)
    fi, _, _ = face_matrix32(p)
    xf, yf = np.asarray(x).astype(np.float32), np.asarray(y).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.stack([(fi[3 * k] * xf + fi[3 * k + 1] * yf) + fi[3 * k + 2] for k in range(3)], -1).astype(np.float32)
        c = np.fmin(np.fmax(w, np.float32(0)), np.float32(1)).astype(np.float32)
        s = ((c[:, 0] + c[:, 1]) + c[:, 2]).astype(np.float32)
        wh = (c / s[:, None]).astype(np.float32)
    return w, c, s, wh


def _rows(attr, b, sid):
    """attribute rows [N,3,C] of the sorted corners; attr [B,NV,C] or [NV,C]"""
    return attr[b[:, None], sid] if attr.ndim == 3 else attr[sid]


def interp32(attr, owner, vertices, faces, with_info=False):
    """Restatement (a): out [B,C,H,W] fp32.  with_info: also a dict of the owned pixels' (b, y, x), unclamped weights w,
    clamped sum s, `live` (s > 0 and finite: the pixels that are not written 0) and the sorted ids and corners."""
    a32 = _np(attr, np.float32)
    own = _np(owner)
    B, H, W = own.shape
    C = a32.shape[-1]
    out = np.zeros((B, C, H, W), np.float32)
    b, y, x, sid, p, order = taps(owner, vertices, faces)
    w, c, s, wh = weights32(p, x, y)
    live = (s > 0) & np.isfinite(s)
    rows = _rows(a32, b, sid)
    with np.errstate(invalid="ignore", over="ignore"):
        val = ((wh[:, 0, None] * rows[:, 0] + wh[:, 1, None] * rows[:, 1]).astype(np.float32)
               + wh[:, 2, None] * rows[:, 2]).astype(np.float32)
    out[b[live], :, y[live], x[live]] = val[live]
    if with_info:
        return out, dict(b=b, y=y, x=x, w=w, c=c, s=s, wh=wh, live=live, sid=sid, p=p, order=order)
    return out


def interp64(attr, owner, vertices, faces, keep=None):
    """Restatement (b): [B,C,H,W] fp64 tensor, differentiable in attr ([B,NV,C] or [NV,C] tensor) and vertices
    ([B,NV,>=3] tensor); the clamp decisions and the zeroed pixels are restatement (a)'s.  keep: a dict that receives the
    live pixels' gathered sorted corners `P` [N,3,2] and attribute rows `rows` [N,3,C] (their gradients retained: after
    a backward they hold every pixel's vertex and attribute terms), their crop `b` [N] and vertex ids `sid` [N,3]
    (tests/fixed_point_ref.py)."""
    own = _np(owner)
    B, H, W = own.shape
    A, V = attr.double(), vertices.double()
    C = A.shape[-1]
    b, y, x, sid, p32, _ = taps(owner, vertices, faces)
    _, _, s32, _ = weights32(p32, x, y)
    live = (s32 > 0) & np.isfinite(s32)
    b, y, x, sid, p32 = b[live], y[live], x[live], sid[live], p32[live]
    out = torch.zeros(B * H * W, C, dtype=torch.float64)
    if len(b) == 0:
        return out.view(B, H, W, C).permute(0, 3, 1, 2) + 0.0 * (A.sum() + V.sum())
    ok, c32 = clamp_decisions(p32, x, y)
    c32 = np.nan_to_num(c32, nan=0.0)                       # (fminf(fmaxf(NaN, 0), 1) = 0; such a weight does not pass)
    tb, tsid = torch.from_numpy(b)[:, None], torch.from_numpy(sid)
    P = V[tb, tsid][..., :2]
    px, py = P[..., 0], P[..., 1]
    qx, qy = torch.from_numpy(x.astype(np.float64))[:, None], torch.from_numpy(y.astype(np.float64))[:, None]
    den = (px[:, 1] - px[:, 0]) * (py[:, 2] - py[:, 0]) - (px[:, 2] - px[:, 0]) * (py[:, 1] - py[:, 0])
    b_, e_ = [1, 2, 0], [2, 0, 1]
    n = (px[:, b_] - qx) * (py[:, e_] - qy) - (px[:, e_] - qx) * (py[:, b_] - qy)
    w = n / den[:, None]
    c = torch.where(torch.from_numpy(ok), w, torch.from_numpy(c32).double())
    wh = c / c.sum(1, keepdim=True)
    rows = A[tb, tsid] if A.dim() == 3 else A[tsid]         # [N,3,C]
    if keep is not None:
        for t in (P, rows):
            if t.requires_grad:
                t.retain_grad()
        keep.update(P=P, rows=rows, b=b, sid=sid)
    val = (wh[:, :, None] * rows).sum(1)
    out = out.index_add(0, torch.from_numpy((b * H + y) * W + x), val)
    return out.view(B, H, W, C).permute(0, 3, 1, 2)


def grads(attr, owner, vertices, faces, grad_out):
    """d <grad_out, interp64> / d (attr, vertices): fp64 numpy arrays of the inputs' shapes."""
    a = torch.as_tensor(_np(attr)).double().requires_grad_(True)
    v = torch.as_tensor(_np(vertices)).double().requires_grad_(True)
    out = interp64(a, owner, v, faces)
    (out * torch.as_tensor(_np(grad_out)).double()).sum().backward()
    return a.grad.numpy(), v.grad.numpy()


def depth32(p, x, y):
    """The raster's fp32 depth (.cu:97-110) of the sorted corners p [N,3,3] at pixels (x, y)."""
    _, c, s, wh = weights32(p, x, y)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = ((wh[:, 0] / p[:, 0, 2] + wh[:, 1] / p[:, 1, 2]).astype(np.float32) + wh[:, 2] / p[:, 2, 2]).astype(np.float32)
        return (np.float32(1) / q).astype(np.float32)


def cpu_owners(depth, vertices, faces):
    """owner [B,H,W] int32 for a raster's depth [B,H,W] (background 1000): the smallest face whose recomputed fp32 depth
    has the raster's bits at the pixel, looked for in the face's bounding box."""
    d, v32, faces = _np(depth, np.float32), _np(vertices, np.float32), _np(faces, np.int64)
    B, H, W = d.shape
    owner = np.full((B, H, W), -1, np.int32)
    dbits = d.view(np.uint32)
    for bi in range(B):
        fv = v32[bi][faces][..., :3]                                      # [F,3,3]
        order = sort_order(fv)
        p = np.take_along_axis(fv, order[:, :, None], 1)
        x0 = np.clip(np.ceil(fv[..., 0].min(1)), 0, W - 1).astype(int)
        x1 = np.clip(np.floor(fv[..., 0].max(1)), -1, W - 1).astype(int)
        y0 = np.clip(np.ceil(fv[..., 1].min(1) - 1), 0, H - 1).astype(int)
        y1 = np.clip(np.floor(fv[..., 1].max(1) + 1), -1, H - 1).astype(int)
        # .cu:33, :54: back faces and faces with x0 == x2 offer no depth
        drawn = ~((fv[:, 2, 1] - fv[:, 0, 1]) * (fv[:, 1, 0] - fv[:, 0, 0]) <
                  (fv[:, 1, 1] - fv[:, 0, 1]) * (fv[:, 2, 0] - fv[:, 0, 0])) & (p[:, 0, 0] != p[:, 2, 0])
        for f in range(len(faces) - 1, -1, -1):                           # descending: the smaller index wins
            if not drawn[f] or x1[f] < x0[f] or y1[f] < y0[f]:
                continue
            gy, gx = np.mgrid[y0[f]:y1[f] + 1, x0[f]:x1[f] + 1]
            gy, gx = gy.ravel(), gx.ravel()
            zp = depth32(np.broadcast_to(p[f], (len(gx), 3, 3)), gx, gy)
            hit = (zp.view(np.uint32) == dbits[bi, gy, gx]) & (d[bi, gy, gx] != np.float32(1000.0))
            owner[bi, gy[hit], gx[hit]] = f
    return owner


def hand_verts(B=4, W=640, H=640):
    """g2_mesh.npz's four sampled hand poses [B,10144,4] at z = 212 .. 475, x, y mapped onto W x H; crops 4 .. repeat
    crop 0 mirrored in x (a left hand for the cull); the faces with the right hand's winding."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2_mesh.npz"))
    v = g["verts"].copy()
    v = np.concatenate([v, v[:1], v[:1], v[:1]])[:B]
    v[4:, :, 0] = 420.0 - v[4:, :, 0]
    v[..., 0] = (v[..., 0] + 110.0) * (W / 640.0)
    v[..., 1] = (v[..., 1] - 165.0) * (H / 490.0)
    v[..., 2] += 300.0
    return np.ascontiguousarray(v, np.float32), g["faces_swapped"].astype(np.int32)
