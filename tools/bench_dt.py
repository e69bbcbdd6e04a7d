"""The silhouette distance transform and its sampler, HIP events on the launching stream:
  transform   shr_dt_fwd through the C ABI (no Python op in the loop) at 256 images @128x128, 1152 @256x256 and
              256 @640x640, on three kinds of input -- hand silhouettes rendered from sampled poses, an almost-empty image
              (one site in a corner: the row pass's worst case) and a full image -- against the byte floor at the tool's own
              copy rate: 4 B read + 4 B written per pixel plus the workspace's 2 B written and 2 B read, 12 B/px (the
              kernels move 16: the column pass writes and reads the workspace once more)
  sampler     ops.DistanceSample forward + backward at N = 10 144 points per image against the torch composition a user
              writes without the kernels -- F.grid_sample (bilinear, border padding, align_corners) on the fp32 distance
              map, which is prepared outside the timed region, with torch's autograd
  nearest     shr_dt_nearest_fwd (the transform with its argument, sil_cover.hip) against shr_dt_fwd on the same images, at
              the same three sizes and three kinds of input
  cover       shr_sil_cover_fwd and shr_sil_cover_bwd through the C ABI for the hand at 256 @128x128 and 1152 @256x256: the
              observation is the batch's hand images, the model each image's hand scaled by 0.8 about the image centre and
              moved by a tenth of the image (rendered by the owner raster and transformed outside the timed region)
in the same process, alternated, three rounds (every round is printed; the summary is the median).  `--parts` picks which
of the four run (default: all)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses  # noqa: E402
from spherehand_amd.kinematicsTransformation import HandTransformationMat  # noqa: E402
from spherehand_amd.render import DepthRender  # noqa: E402

ROUNDS = 3
FG_MAX = 900.0
N_POINTS = 10144
FLOOR_BYTES = 12


def fwd_bwd(make, leaf, g):
    """(forward us, backward us) of out = make() and autograd.grad(out, leaf, g), timed apart; mean of 5 after a warm-up"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for rep in range(6):
        ev[0].record()
        out = make()
        ev[1].record()
        torch.autograd.grad(out, leaf, g)
        ev[2].record()
        ev[2].synchronize()
        if rep:
            tf += ev[0].elapsed_time(ev[1]) * 1e3 / 5
            tb += ev[1].elapsed_time(ev[2]) * 1e3 / 5
    return tf, tb


def hand_images(mesh, fk, B, S):
    """(depth [B,S,S], the projected vertices [B,NV,4] in its pixel space, the raster's faces) of B sampled poses,
    background 1000"""
    dr = DepthRender(mesh, 128).cuda()
    depth, verts = [], []
    with torch.no_grad():
        for lo in range(0, B, 256):
            n = min(256, B - lo)
            v = dr.lbs(fk(sample_poses(n, seed=1 + lo).cuda()).contiguous(), dr.camera, None).contiguous()
            v[..., :2] *= S / 640.0
            depth.append(ops.tri_raster_indexed_fwd(S, S, v, dr.rasterizer.faces_i32))
            verts.append(v)
    return torch.cat(depth), torch.cat(verts), dr.rasterizer.faces_i32


def rounds(runs, stream, slow=()):
    """{name: median us over ROUNDS alternated rounds} of the launches in `runs` (name -> fn(stream handle))"""
    for name, fn in runs.items():
        assert fn(stream.cuda_stream) == 0, name
    stream.synchronize()
    us = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for name, fn in runs.items():
            us[name].append(bench.mean_launch_us(fn, stream, 3 if name in slow else 10, 3, 2, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.1f" % (k, v[-1]) for k, v in us.items())), flush=True)
    return {k: float(np.median(v)) for k, v in us.items()}


def nearest_part(lib, stream, kinds, B, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    d2 = torch.empty((B, S, S), dtype=torch.int32, device="cuda")
    d2n, near = torch.empty_like(d2), torch.empty_like(d2)
    ws = torch.empty(max(16, lib.shr_dt_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")
    wsn = torch.empty(max(16, lib.shr_dt_nearest_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")
    runs = {}
    for kind, img in kinds.items():
        runs[kind + " dt"] = (lambda s, img=img: lib.shr_dt_fwd(p(img), B, S, S, FG_MAX, p(d2), p(ws), s))
        runs[kind + " nearest"] = (lambda s, img=img: lib.shr_dt_nearest_fwd(p(img), B, S, S, FG_MAX, p(d2n), p(near), p(wsn), s))
    us = rounds(runs, stream, slow=("almost empty dt", "almost empty nearest"))
    assert torch.equal(d2, d2n)                            # (the last kind's: the same bits)
    print("nearest B=%d %dx%d: %s" % (B, S, S, "; ".join(
        "%s: dt %.1f us, nearest %.1f us (x%.2f)" % (k, us[k + " dt"], us[k + " nearest"], us[k + " nearest"] / us[k + " dt"])
        for k in kinds)), flush=True)


def cover_part(lib, stream, hand, verts, faces, B, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    NV, F = verts.shape[1], faces.shape[0]
    model = verts.clone()
    model[..., :2] = (verts[..., :2] - S / 2) * 0.8 + S / 2 + torch.tensor([0.1 * S, 0.07 * S], device="cuda")
    model = model.contiguous()
    depth, owner = ops.tri_raster_indexed_owner_fwd(S, S, model, faces)
    d2, near = ops.nearest_site_transform(depth, 1000.0)
    dist = torch.empty((B, S, S), dtype=torch.float32, device="cuda")
    gd = torch.randn(B, S, S, device="cuda")
    out = torch.empty((B, NV, 4), dtype=torch.float32, device="cuda")
    ws = torch.empty(max(16, lib.shr_sil_cover_bwd_workspace_bytes(B, NV)), dtype=torch.uint8, device="cuda")
    ws_n = torch.empty(max(16, lib.shr_dt_nearest_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")
    inf = float("inf")
    runs = {"cover forward": lambda s: lib.shr_sil_cover_fwd(p(hand), FG_MAX, p(d2), B, S, S, inf, p(dist), s),
            "cover backward": lambda s: lib.shr_sil_cover_bwd(p(hand), FG_MAX, p(d2), p(near), p(owner), p(model), p(faces),
                                                              p(gd), B, NV, F, S, S, inf, p(out), p(ws), s),
            "nearest": lambda s: lib.shr_dt_nearest_fwd(p(depth), B, S, S, 1000.0, p(d2), p(near), p(ws_n), s)}
    us = rounds(runs, stream)
    pulled = ((hand < FG_MAX) & (d2 > 0)).float().mean().item()
    print("cover B=%d %dx%d NV=%d (%.1f %% of the pixels observed and uncovered, mean distance %.2f px): %s"
          % (B, S, S, NV, 100 * pulled, dist.sum().item() / max(1.0, (hand < FG_MAX).sum().item()),
             "; ".join("%s %.1f us" % kv for kv in us.items())), flush=True)


def transform_part(lib, stream, kinds, hand, B, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    npix = B * S * S
    d2 = torch.empty((B, S, S), dtype=torch.int32, device="cuda")
    ws = torch.empty(max(16, lib.shr_dt_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")
    copy = torch.empty_like(hand)

    def copy_image(s):   # (on the current stream: the timed one)
        copy.copy_(hand)
        return 0

    runs = {"copy": copy_image}
    for kind, img in kinds.items():
        runs[kind] = (lambda s, img=img: lib.shr_dt_fwd(p(img), B, S, S, FG_MAX, p(d2), p(ws), s))
    ours = rounds(runs, stream, slow=("almost empty",))
    copy_us = ours["copy"]
    rate = 8 * npix / (copy_us * 1e-6) / 1e12
    floor = FLOOR_BYTES * npix / (rate * 1e12) * 1e6
    fg = (hand < FG_MAX).float().mean().item()
    print("transform B=%d %dx%d (hand: %.1f %% foreground): copy %.1f us = %.2f TB/s, floor %.1f us at %d B/px; %s"
          % (B, S, S, 100 * fg, copy_us, rate, floor, FLOOR_BYTES,
             "; ".join("%s %.1f us (x%.2f)" % (k, v, v / floor) for k, v in ours.items() if k != "copy")), flush=True)


def sampler_part(lib, stream, hand, verts, B, S):
    p = lambda t: t.data_ptr()  # noqa: E731
    d2 = torch.empty((B, S, S), dtype=torch.int32, device="cuda")
    ws = torch.empty(max(16, lib.shr_dt_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")
    # the sampler on the hand's transform, at 10 144 points per image: the hand's own vertices (the 1 721 distinct
    # ones, repeated) moved off the silhouette by a tenth of the image
    assert lib.shr_dt_fwd(p(hand), B, S, S, FG_MAX, p(d2), p(ws), stream.cuda_stream) == 0
    idx = torch.arange(N_POINTS, device="cuda") % verts.shape[1]
    pts = (verts[:, idx] + torch.tensor([0.1 * S, 0.07 * S, 0, 0], device="cuda")).contiguous()
    dist = d2.float().sqrt().unsqueeze(1)
    scale = torch.tensor([2.0 / (S - 1), 2.0 / (S - 1)], device="cuda")
    g = torch.randn(B, N_POINTS, device="cuda")
    res = {"ours forward": [], "ours backward": [], "grid_sample forward": [], "grid_sample backward": []}
    for rnd in range(ROUNDS):
        x = pts.clone().requires_grad_(True)
        a, b = fwd_bwd(lambda: ops.DistanceSample.apply(x, d2, float("inf")), x, g)
        res["ours forward"].append(a)
        res["ours backward"].append(b)
        a, b = fwd_bwd(lambda: Fn.grid_sample(dist, (x[..., :2] * scale - 1.0).unsqueeze(2), mode="bilinear",
                                              padding_mode="border", align_corners=True)[:, 0, :, 0], x, g)
        res["grid_sample forward"].append(a)
        res["grid_sample backward"].append(b)
        print("  round %d: %s" % (rnd, " | ".join("%s %.1f" % (k, v[-1]) for k, v in res.items())), flush=True)
    with torch.no_grad():
        ref = Fn.grid_sample(dist, (pts[..., :2] * scale - 1.0).unsqueeze(2), mode="bilinear", padding_mode="border",
                             align_corners=True)[:, 0, :, 0]
        err = (ops.dt_sample(d2, pts)[0] - ref).abs().max().item()
    print("sampler B=%d %dx%d N=%d: %s; max |value - grid_sample| %.3g px"
          % (B, S, S, N_POINTS, " | ".join("%s %.1f us" % (k, float(np.median(v))) for k, v in res.items()), err),
          flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="transform,sampler,nearest,cover")
    parts = set(ap.parse_args().parts.split(","))
    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for B, S in ((256, 128), (1152, 256), (256, 640)):
            hand, verts, faces = hand_images(mesh, fk, B, S)
            corner = torch.full_like(hand, 1000.0)
            corner[:, S - 1, S - 1] = 1.0
            kinds = {"hand": hand, "almost empty": corner, "full": torch.ones_like(hand)}
            if "transform" in parts:
                transform_part(lib, stream, kinds, hand, B, S)
            if "sampler" in parts:
                sampler_part(lib, stream, hand, verts, B, S)
            if "nearest" in parts:
                nearest_part(lib, stream, kinds, B, S)
            if "cover" in parts and S <= 256:
                cover_part(lib, stream, hand, verts, faces, B, S)


if __name__ == "__main__":
    main()
