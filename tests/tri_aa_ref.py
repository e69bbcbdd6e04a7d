"""fp64 restatement of the antialias pass (include/spherehand_hip.h, shr_tri_antialias_fwd / _bwd; test helper, not a
conftest).

The pairs, front pixels, drawn faces and silhouette edges are taken as the contract states them -- the drawn test is the
reference's fp32 cull, restated bit for bit in numpy float32 -- and the crossing s and the gains in fp64 through torch,
so that autograd gives the contract's gradient to the values and to the vertices' x, y.  `antialias` also reports the
pixels whose fp64 decision lies within `eps` of a threshold (s near 0 or 1, a crossing row at an edge's endpoint,
|dx| - |dy| near 0, and s near 1/2, where the gaining pixel -- whose upstream gradient the vertex terms take -- changes
sides): an fp32 kernel may decide those either way."""
import numpy as np
import torch


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def drawn(vertices, faces):
    """[B,F] bool: face_sort accepts the face (front-facing by .cu:33 in fp32, x0 != x2) and its ids are in range."""
    v = _np(vertices).astype(np.float32)
    f = _np(faces).astype(np.int64)
    NV = v.shape[1]
    ok = ((f >= 0) & (f < NV)).all(1)
    p = v[:, np.clip(f, 0, NV - 1), :3]                                        # [B,F,3,3]
    x0, y0, x1, y1, x2, y2 = p[..., 0, 0], p[..., 0, 1], p[..., 1, 0], p[..., 1, 1], p[..., 2, 0], p[..., 2, 1]
    back = (y2 - y0) * (x1 - x0) < (y1 - y0) * (x2 - x0)
    flat = p[..., 0].min(-1) == p[..., 0].max(-1)
    return ok[None] & ~back & ~flat


def _pairs(owner, depth):
    """Every 4-neighbour pair with different owners: (b, first pixel (y, x), second pixel, vertical, front_is_first)."""
    B, H, W = owner.shape
    out = []
    for vert in (False, True):
        a = owner[:, :-1, :] if vert else owner[:, :, :-1]
        c = owner[:, 1:, :] if vert else owner[:, :, 1:]
        b, y, x = np.nonzero(a != c)
        y2, x2 = (y + 1, x) if vert else (y, x + 1)
        op, oq = owner[b, y, x], owner[b, y2, x2]
        fp = (op >= 0) & ((oq < 0) | ~(depth[b, y2, x2] < depth[b, y, x]))
        out.append((b, y, x, y2, x2, np.full(len(b), vert), fp))
    return [np.concatenate(z) for z in zip(*out)]


def antialias(values, depth, owner, vertices, faces, edges, eps=1e-4):
    """(out [B,H,W] fp64 tensor, differentiable in `values` and `vertices` (tensors), info).  info: 'gain' [B,H,W] bool
    (pixels that gained), 'touched' (pixels of a qualifying pair), 'ambiguous' (pixels of a pair with a decision within
    eps of a threshold), 'pairs' (the number of qualifying pairs)."""
    own, dep = _np(owner).astype(np.int64), _np(depth).astype(np.float32)
    f = _np(faces).astype(np.int64)
    e = _np(edges).astype(np.int64)
    v64 = _np(vertices).astype(np.float64)
    B, H, W = own.shape
    F, NV = len(f), v64.shape[1]
    dr = drawn(vertices, f) if F else np.zeros((B, 0), bool)
    allp = _pairs(own, dep)
    b, y, x, y2, x2, vert, fp = allp
    t = np.where(fp, own[b, y, x], own[b, y2, x2])
    valid = (t >= 0) & (t < F)
    tt = np.where(valid, t, 0)
    sigma = np.where(fp, 1.0, -1.0)
    uf = np.where(vert, np.where(fp, y, y2), np.where(fp, x, x2)).astype(np.float64)
    row = np.where(vert, x, y).astype(np.float64)
    chosen = np.full(len(b), -1)
    s_chosen = np.zeros(len(b))
    amb = np.zeros(len(b), bool)
    for k in range(3):
        va, vb = f[tt, k] if F else tt, f[tt, (k + 1) % 3] if F else tt
        ids = (va >= 0) & (va < NV) & (vb >= 0) & (vb < NV)
        va, vb = np.clip(va, 0, NV - 1), np.clip(vb, 0, NV - 1)
        pa, pb = v64[b, va], v64[b, vb]
        ua, wa = np.where(vert, pa[:, 1], pa[:, 0]), np.where(vert, pa[:, 0], pa[:, 1])
        ub, wb = np.where(vert, pb[:, 1], pb[:, 0]), np.where(vert, pb[:, 0], pb[:, 1])
        du, dw = ub - ua, wb - wa
        across = e[tt, k] if F else tt
        shared = (across >= 0) & (across < F)
        sil = ~(shared & dr[b, np.where(shared, across, 0)]) if F else np.zeros(len(b), bool)
        base = valid & ids & dr[b, tt] & sil if F else np.zeros(len(b), bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = sigma * (ua + (row - wa) * du / dw - uf)
        lo, hi = np.minimum(wa, wb), np.maximum(wa, wb)
        steep = np.abs(dw) - np.abs(du)

        def conds(d):   # the geometric conditions, widened (d > 0) or narrowed (d < 0) by |d|
            st = np.where(vert, steep > -d, steep >= -d)
            return st & (np.abs(dw) > 0) & (lo - d <= row) & (row <= hi + d) & (s >= -d) & (s <= 1 + d)

        exact, loose, tight = conds(0.0), conds(eps), conds(-eps)
        amb |= base & loose & ~tight & (chosen < 0)
        take = base & exact & (chosen < 0)
        chosen[take] = k
        s_chosen[take] = s[take]
    q = chosen >= 0
    amb |= q & (np.abs(s_chosen - 0.5) < eps)
    b, y, x, y2, x2, vert, fp, t, sigma, uf, row, k = (a[q] for a in (b, y, x, y2, x2, vert, fp, t, sigma, uf, row, chosen))
    # fp64 autograd: s from the vertices, gains from the values
    vt = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(v64)
    vt = vt.double()
    ct = values if isinstance(values, torch.Tensor) else torch.from_numpy(_np(values))
    ct = ct.double()
    dev = ct.device
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    va, vb = T(f[t, k]), T(f[t, (k + 1) % 3])
    bt = T(b)
    pa, pb = vt[bt, va], vt[bt, vb]
    vm = T(vert)
    ua, wa = torch.where(vm, pa[:, 1], pa[:, 0]), torch.where(vm, pa[:, 0], pa[:, 1])
    ub, wb = torch.where(vm, pb[:, 1], pb[:, 0]), torch.where(vm, pb[:, 0], pb[:, 1])
    s = T(sigma) * (ua + (T(row) - wa) * (ub - ua) / (wb - wa) - T(uf))
    i1, i2 = T((b * H + y) * W + x), T((b * H + y2) * W + x2)
    fpt = T(fp)
    i_f, i_o = torch.where(fpt, i1, i2), torch.where(fpt, i2, i1)
    flat = ct.reshape(-1)
    cf, co = flat[i_f], flat[i_o]
    o_gains = s.detach() >= 0.5
    gain = torch.where(o_gains, (s - 0.5) * (cf - co), (0.5 - s) * (co - cf))
    out = flat.index_add(0, torch.where(o_gains, i_o, i_f), gain).view(B, H, W)
    info = {"gain": np.zeros((B, H, W), bool), "touched": np.zeros((B, H, W), bool),
            "ambiguous": np.zeros((B, H, W), bool), "pairs": int(q.sum())}
    g = _np(torch.where(o_gains, i_o, i_f))
    info["gain"].reshape(-1)[g] = True
    info["touched"].reshape(-1)[_np(i1)] = True
    info["touched"].reshape(-1)[_np(i2)] = True
    ba, ya, xa, ya2, xa2 = (a[amb] for a in allp[:5])
    info["ambiguous"][ba, ya, xa] = True
    info["ambiguous"][ba, ya2, xa2] = True
    return out, info


def grads(values, depth, owner, vertices, faces, edges, grad_out):
    """(d<grad_out, out>/d values [B,H,W], d/d vertices [B,NV,C]) in fp64 numpy."""
    c = torch.as_tensor(_np(values)).double().requires_grad_(True)
    v = torch.as_tensor(_np(vertices)).double().requires_grad_(True)
    out, _ = antialias(c, depth, owner, v, faces, edges)
    (out * torch.as_tensor(_np(grad_out)).double()).sum().backward()
    return c.grad.numpy(), v.grad.numpy()
