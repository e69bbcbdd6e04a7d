"""The depth-image normals (shr_depth_normals_fwd / _bwd, depth_normals.hip), HIP events on the launching stream:
  ours    forward and backward through the C ABI (no Python op in the loop) on rendered depth of sampled hand poses at
          256 crops @128x128, 1152 @256x256 and 256 @640x640, background 1000, fg_max 900, max_step 8, scale 640 / S
  loss    render.NormalConsistencyLoss (a torch composition) on the kernel's map against the map of the batch rolled by
          one crop: its forward, and its forward with the backward to the model map
  torch   for the ratio, the same forward as a torch composition a user writes without the kernel (pad, where chains)
in the same process, alternated, three rounds (every round is printed; the summary is the median).  Each kernel time is
reported against its byte floor -- forward 4 B read + 12 B written per pixel, backward 4 + 12 B read + 4 B written -- at
bench.HBM_PEAK_GBS (MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec; 6.29 TB/s is what a float4 copy measures there)."""
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
from spherehand_amd.render import DepthRender, NormalConsistencyLoss  # noqa: E402

ROUNDS = 3
FG_MAX = 900.0
MAX_STEP = 8.0
COPY_GBS = 6290.0
CASES = ((256, 128), (1152, 256), (256, 640))


def hand_depth(mesh, fk, B, S):
    """[B,S,S]: the triangle raster's depth of B sampled poses at S x S"""
    dr = DepthRender(mesh, 128).cuda()
    depth = []
    with torch.no_grad():
        for lo in range(0, B, 128):
            n = min(128, B - lo)
            v = dr.lbs(fk(sample_poses(n, seed=1 + lo).cuda()).contiguous(), dr.camera, None).contiguous()
            v[..., :2] *= S / 640.0
            depth.append(ops.tri_raster_indexed_fwd(S, S, v, dr.rasterizer.faces_i32))
    return torch.cat(depth)


def torch_forward(d, fg_max, sx, sy, max_step):
    """the contract's sequence as a torch composition: [B,3,H,W]"""
    p = torch.nn.functional.pad(d, (1, 1, 1, 1), value=float("inf"))      # outside the image: never usable
    c, l, r, u, dn = d, p[:, 1:-1, :-2], p[:, 1:-1, 2:], p[:, :-2, 1:-1], p[:, 2:, 1:-1]
    use = lambda n: (n < fg_max) & ((n - c).abs() <= max_step)   # noqa: E731
    ul, ur, uu, ud = use(l), use(r), use(u), use(dn)
    dx = torch.where(ul & ur, r - l, torch.where(ur, r - c, c - l))
    dy = torch.where(uu & ud, dn - u, torch.where(ud, dn - c, c - u))
    wx = torch.where(ul & ur, 2.0, 1.0) * sx
    wy = torch.where(uu & ud, 2.0, 1.0) * sy
    N = torch.stack([dx * wy, dy * wx, -(wx * wy)], 1)
    s = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
    live = (c < fg_max) & (ul | ur) & (uu | ud) & (s > 0) & torch.isfinite(s)
    root = torch.where(live, s, torch.ones_like(s)).sqrt()
    return torch.where(live[:, None], N / root[:, None], torch.zeros_like(N))


def main():
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
    term = NormalConsistencyLoss()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for B, S in CASES:
            depth = hand_depth(mesh, fk, B, S)
            scale = 640.0 / S
            normals = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
            gn = torch.randn(B, 3, S, S, device="cuda")
            gd = torch.empty_like(depth)
            assert lib.shr_depth_normals_fwd(p(depth), B, S, S, FG_MAX, scale, scale, MAX_STEP, p(normals), stream.cuda_stream) == 0
            model = normals.clone().requires_grad_(True)
            observed = normals.roll(1, 0)

            def composed(s):   # (on the current stream: the timed one)
                composed.out = torch_forward(depth, FG_MAX, scale, scale, MAX_STEP)
                return 0

            def loss_fwd(s):
                with torch.no_grad():
                    loss_fwd.out = term.loss(model, observed)
                return 0

            def loss_both(s):
                loss_both.out, = torch.autograd.grad(term.loss(model, observed), model)
                return 0

            runs = {"forward": lambda s: lib.shr_depth_normals_fwd(p(depth), B, S, S, FG_MAX, scale, scale, MAX_STEP,
                                                                   p(normals), s),
                    "backward": lambda s: lib.shr_depth_normals_bwd(p(depth), p(gn), B, S, S, FG_MAX, scale, scale, MAX_STEP,
                                                                    p(gd), s),
                    "loss": loss_fwd, "loss+grad": loss_both, "torch": composed}
            for name, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, name
            stream.synchronize()
            us = {k: [] for k in runs}
            for rnd in range(ROUNDS):
                for name, fn in runs.items():
                    us[name].append(bench.mean_launch_us(fn, stream, 5, 3, 2, warm_ms=20.0))
                print("  round %d: %s" % (rnd, " | ".join("%s %.1f" % (k, v[-1]) for k, v in us.items())), flush=True)
            us = {k: float(np.median(v)) for k, v in us.items()}
            pixels = float(depth.numel())
            fwd, bwd = bench.roof(16 * pixels, us["forward"]), bench.roof(20 * pixels, us["backward"])
            err = (composed.out - normals).abs().max().item()
            print("depth normals B=%d %dx%d: %.1f %% foreground, %.1f %% with a normal; forward %.1f us = %.0f GB/s of its "
                  "16 B per pixel (%.2f of %.0f, %.2f of the %.0f a copy reaches), backward %.1f us = %.0f GB/s of its 20 B "
                  "per pixel (%.2f, %.2f); loss %.1f us, loss with its backward %.1f us (x%.1f the two kernels); torch "
                  "composition of the forward %.1f us (x%.1f); max |normals - torch| %.3g, loss %.4f"
                  % (B, S, S, 100.0 * (depth < FG_MAX).float().mean().item(), 100.0 * (normals != 0).any(1).float().mean().item(),
                     us["forward"], fwd["achieved"], fwd["frac"], bench.HBM_PEAK_GBS, fwd["achieved"] / COPY_GBS, COPY_GBS,
                     us["backward"], bwd["achieved"], bwd["frac"], bwd["achieved"] / COPY_GBS, us["loss"], us["loss+grad"],
                     us["loss+grad"] / (us["forward"] + us["backward"]), us["torch"], us["torch"] / us["forward"], err,
                     loss_fwd.out.item()), flush=True)
            del depth, normals, gn, gd, model, observed
            composed.out = loss_both.out = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
