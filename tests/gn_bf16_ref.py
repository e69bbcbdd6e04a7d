"""numpy restatement of the bf16 GroupNorm+ReLU kernel pair (spherehand_amd/csrc/group_norm_relu_bf16.hip): the
fp32 <-> bf16 conversions on bit patterns, and forward and backward in fp64 on given bf16 inputs."""
import numpy as np


def bf16_round(a):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even: the kernels' gn_bf16_rne.  An infinity stays one,
    a finite value beyond the largest bf16 rounds to infinity, a NaN stays a NaN (quiet bit set, sign and upper payload
    kept)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    rounded = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rounded).astype(np.uint16)


def bf16_widen(bits):
    """bf16 bit patterns (uint16) -> fp32, exactly: the 16 bits are the upper half of the fp32 pattern."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_truncate(a):
    """What a kernel that drops the lower half instead of rounding would store (the tests show their bound refuses it)."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def reference(x_bits, gamma, beta, G, eps, pre_bias=None, dy_bits=None):
    """relu(GroupNorm(x + pre_bias)) in fp64.  x_bits, dy_bits: bf16 patterns [N, C, H, W]; gamma, beta, pre_bias [C].
    Returns a dict: 'pre' (the fp64 pre-activation that decides the ReLU mask), 'y', 'mean', 'rstd' [N, G] and, with
    dy_bits, 'dx', 'dgamma', 'dbeta', 'dpre' (the producing convolution's bias gradient = sum of dx per channel)."""
    x = bf16_widen(x_bits).astype(np.float64)
    N, C, H, W = x.shape
    g64, b64 = np.asarray(gamma, np.float64).reshape(1, C, 1, 1), np.asarray(beta, np.float64).reshape(1, C, 1, 1)
    if pre_bias is not None:
        x = x + np.asarray(pre_bias, np.float64).reshape(1, C, 1, 1)
    xg = x.reshape(N, G, -1)
    M = xg.shape[2]
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = ((xg - mean[..., None]) * rstd[..., None]).reshape(N, C, H, W)
    pre = xhat * g64 + b64
    out = {"pre": pre, "y": np.maximum(pre, 0.0), "mean": mean, "rstd": rstd}
    if dy_bits is None:
        return out
    d = bf16_widen(dy_bits).astype(np.float64) * (pre > 0)
    out["dgamma"] = (d * xhat).sum((0, 2, 3))
    out["dbeta"] = d.sum((0, 2, 3))
    dg = d * g64
    s1 = dg.reshape(N, G, -1).sum(-1)[..., None]
    s2 = (dg * xhat).reshape(N, G, -1).sum(-1)[..., None]
    dx = rstd[..., None] * (dg.reshape(N, G, -1) - (s1 + xhat.reshape(N, G, -1) * s2) / M)
    out["dx"] = dx.reshape(N, C, H, W)
    out["dpre"] = out["dx"].sum((0, 2, 3))
    return out


# ---- the cases of the tests (torch is needed from here on) ----------------------------------------------------------
# (N, C, H, W, G): C/G = 16; C/G = 4, a lane's two halves in two groups; C/G = 8; C/G = 32; 35 pixels, one short round
# of the 32-pixel stride; many rounds
SHAPES = [(3, 64, 8, 8, 4), (3, 64, 8, 8, 16), (2, 128, 4, 4, 16), (2, 256, 4, 4, 8), (3, 32, 5, 7, 8), (2, 64, 32, 32, 16)]


def case(N, C, H, W, G, seed, with_pre=True):
    """x, dy (bf16) and gamma, beta, pre_bias (fp32) of a case, as torch CPU tensors."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, H, W, generator=g) * 3 + 1).bfloat16()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    pre = torch.randn(C, generator=g) * 2
    dy = torch.randn(N, C, H, W, generator=g).bfloat16()
    return x, gamma, beta, (pre if with_pre else None), dy


def bits(t):
    """A torch bf16 tensor's bit patterns as a numpy uint16 array."""
    import torch
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def clear_seed(N, C, H, W, G, with_pre, margin=1e-5, tries=8):
    """The first seed whose fp64 pre-activation has no element within `margin` of zero (a ReLU decision that differs
    between fp32 and fp64 is no arithmetic error, but moves a group sum by O(1/M))."""
    for seed in range(tries):
        x, gamma, beta, pre, dy = case(N, C, H, W, G, seed, with_pre)
        r = reference(bits(x), gamma.numpy(), beta.numpy(), G, 1e-5, None if pre is None else pre.numpy())
        if np.abs(r["pre"]).min() > margin:
            return seed
    return None
