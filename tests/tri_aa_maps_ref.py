"""fp64 restatement of the antialias pass over multi-channel maps (include/spherehand_hip.h,
shr_tri_antialias_maps_fwd / _bwd; test helper, not a conftest): by contract the pass is the single-plane pass on every
channel plane, so this calls tests/tri_aa_ref.py per channel and sums."""
import numpy as np
import torch

import tri_aa_ref as ref


def antialias(values, depth, owner, vertices, faces, edges, eps=1e-4):
    """(out [B,C,H,W] fp64 tensor, info): tri_aa_ref.antialias on every plane.  info does not depend on the values (the
    decisions take none): it is channel 0's."""
    outs, info = [], None
    for ch in range(values.shape[1]):
        o, i = ref.antialias(values[:, ch], depth, owner, vertices, faces, edges, eps)
        outs.append(o)
        info = info or i
    return torch.stack(outs, 1), info


def grads(values, depth, owner, vertices, faces, edges, grad_out):
    """(d<grad_out, out>/d values [B,C,H,W], d/d vertices [B,NV,C']) in fp64 numpy: the sum over the channels of
    tri_aa_ref.grads' vertex gradients, one autograd pass."""
    c = torch.as_tensor(ref._np(values)).double().requires_grad_(True)
    v = torch.as_tensor(ref._np(vertices)).double().requires_grad_(True)
    g = torch.as_tensor(ref._np(grad_out)).double()
    loss = 0.0
    for ch in range(c.shape[1]):
        out, _ = ref.antialias(c[:, ch], depth, owner, v, faces, edges)
        loss = loss + (out * g[:, ch]).sum()
    loss.backward()
    return c.grad.numpy(), (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape)))
