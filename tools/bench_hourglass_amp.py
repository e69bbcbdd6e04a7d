"""The bf16 GroupNorm+ReLU kernels and the hourglass under bf16 autocast, HIP events on the launching stream:
  kernels     shr_group_norm_relu_bf16_fwd / _bwd through the C ABI (no Python op in the loop) at the hourglass's own
              activation shapes for the reference-sized step's 123 crops, against the fp32 kernels on the same values and
              against a copy of the same bytes at the tool's own copy rate -- the byte floor: 4 B per element forward
              (2 read, 2 written), 6 B backward (x and dy read, dx written); the re-reads of a slab are expected to hit
              the L2
  network     the hourglass forward + backward (loss = out.square().mean()) at 123 crops @ 64 x 64, three ways: fp32
              with the fused kernels (the baseline), bf16 autocast with FUSED_GROUP_NORM_RELU = False (torch's group_norm
              in fp32 between bf16 convolutions), bf16 autocast with the bf16 kernels
in the same process, alternated, three rounds (every round is printed; the summary is the median).  `--miopen_find` lets
MIOpen time every convolution shape first (Engine's opts.miopen_find); `--parts` picks which of the two run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, ops  # noqa: E402
from spherehand_amd.hourglass import create_hourglass_network  # noqa: E402

ROUNDS = 3
CROPS = 123                 # 48 synthetic + 25 x 3 real views: the reference-sized step
# (C, G, HW, pairs per forward pass) of the 35 GroupNorm+ReLU pairs of create_hourglass_network(82, 1) at 64 x 64 crops
SHAPES = [(64, 4, 1024, 1), (64, 16, 1024, 3), (128, 16, 256, 9), (256, 16, 256, 4), (128, 16, 64, 6), (256, 16, 64, 3),
          (128, 16, 16, 6), (256, 16, 16, 3)]
assert sum(s[3] for s in SHAPES) == 35


def rounds(runs, stream):
    """{name: median us over ROUNDS alternated rounds} of the launches in `runs` (name -> fn(stream handle))"""
    for name, fn in runs.items():
        assert fn(stream.cuda_stream) == 0, name
    stream.synchronize()
    us = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for name, fn in runs.items():
            us[name].append(bench.mean_launch_us(fn, stream, 20, 3, 3, warm_ms=20.0))
        print("  round %d: %s" % (rnd, " | ".join("%s %.1f" % (k, v[-1]) for k, v in us.items())), flush=True)
    return {k: float(np.median(v)) for k, v in us.items()}


def kernels_part(lib, stream):
    p = lambda t: t.data_ptr()  # noqa: E731
    total = {k: 0.0 for k in ("bf16 fwd", "fp32 fwd", "floor fwd", "bf16 bwd", "fp32 bwd", "floor bwd")}
    for C, G, HW, count in SHAPES:
        N = CROPS
        g = torch.Generator(device="cuda").manual_seed(C + HW)
        xb = (torch.randn(N, HW, C, device="cuda", generator=g) * 3 + 1).bfloat16()
        db = torch.randn(N, HW, C, device="cuda", generator=g).bfloat16()
        xf, df = xb.float(), db.float()
        yb, ob, yf, of = torch.empty_like(xb), torch.empty_like(xb), torch.empty_like(xf), torch.empty_like(xf)
        gamma, beta = torch.randn(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g) * 0.5
        pre = torch.randn(C, device="cuda", generator=g) * 2
        mean, rstd = torch.empty(N, G, device="cuda"), torch.empty(N, G, device="cuda")
        part, dgb = torch.empty(3, N, C, device="cuda"), torch.empty(3, C, device="cuda")
        copy = torch.empty_like(xb)

        def copy_bytes(s):   # (on the current stream: the timed one) 2 B read + 2 B written per element
            copy.copy_(xb)
            return 0

        def fwd(fn, x, y):
            return lambda s: fn(p(x), p(pre), p(gamma), p(beta), N, C, HW, G, 1e-5, p(y), p(mean), p(rstd), s)

        def bwd(fn, x, d, o):
            return lambda s: fn(p(x), p(pre), p(d), p(gamma), p(beta), p(mean), p(rstd), N, C, HW, G, p(o), p(part[0]),
                                p(part[1]), p(part[2]), p(dgb[0]), p(dgb[1]), p(dgb[2]), s)

        us = rounds({"copy": copy_bytes,
                     "bf16 fwd": fwd(lib.shr_group_norm_relu_bf16_fwd, xb, yb), "fp32 fwd": fwd(lib.shr_group_norm_relu_fwd, xf, yf),
                     "bf16 bwd": bwd(lib.shr_group_norm_relu_bf16_bwd, xb, db, ob), "fp32 bwd": bwd(lib.shr_group_norm_relu_bwd, xf, df, of)},
                    stream)
        assert torch.equal(yb, yf.bfloat16()) and torch.equal(ob, of.bfloat16())        # the same values, rounded once
        us["floor fwd"], us["floor bwd"] = us["copy"], us["copy"] * 1.5
        rate = 4 * xb.numel() / (us["copy"] * 1e-6) / 1e12
        print("N=%d C=%d G=%d HW=%d (x%d per pass): copy %.1f us = %.2f TB/s | forward: bf16 %.1f us (x%.2f of its floor, "
              "x%.2f of fp32 %.1f us) | backward with the parameter sums: bf16 %.1f us (x%.2f of its floor, x%.2f of fp32 %.1f us)"
              % (N, C, G, HW, count, us["copy"], rate, us["bf16 fwd"], us["bf16 fwd"] / us["floor fwd"],
                 us["bf16 fwd"] / us["fp32 fwd"], us["fp32 fwd"], us["bf16 bwd"], us["bf16 bwd"] / us["floor bwd"],
                 us["bf16 bwd"] / us["fp32 bwd"], us["fp32 bwd"]), flush=True)
        for k in total:
            total[k] += count * us[k]
    print("kernels, all 35 pairs of a pass at %d crops: forward bf16 %.0f us, fp32 %.0f us, floor %.0f us; backward bf16 %.0f us, "
          "fp32 %.0f us, floor %.0f us" % (CROPS, total["bf16 fwd"], total["fp32 fwd"], total["floor fwd"], total["bf16 bwd"],
                                           total["fp32 bwd"], total["floor bwd"]), flush=True)


def network_part(stream, find):
    torch.manual_seed(0)
    net = create_hourglass_network(82, 1).cuda().to(memory_format=torch.channels_last)
    x = torch.randn(CROPS, 1, 64, 64, device="cuda").to(memory_format=torch.channels_last)
    ways = {"fp32 fused": (False, True), "bf16 autocast, torch group_norm": (True, False), "bf16 autocast, bf16 kernels": (True, True)}

    def step(amp, fused):
        ops.FUSED_GROUP_NORM_RELU = fused
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out, _ = net(x)
        out[0].float().square().mean().backward()

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in ways}
    try:
        for name, (amp, fused) in ways.items():       # every shape's solver chosen, code objects loaded
            for _ in range(3):
                step(amp, fused)
        stream.synchronize()
        for rnd in range(ROUNDS):
            for name, (amp, fused) in ways.items():
                for _ in range(3):
                    step(amp, fused)
                e0.record(stream)
                for _ in range(20):
                    step(amp, fused)
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / 20)
            print("  round %d: %s" % (rnd, " | ".join("%s %.3f" % (k, v[-1]) for k, v in ms.items())), flush=True)
    finally:
        ops.FUSED_GROUP_NORM_RELU = True
    med = {k: float(np.median(v)) for k, v in ms.items()}
    base = med["fp32 fused"]
    print("hourglass forward + backward, %d crops @ 64x64, miopen_find %s: %s"
          % (CROPS, "on" if find else "off", "; ".join("%s %.3f ms (x%.2f)" % (k, v, v / base) for k, v in med.items())),
          flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernels,network")
    ap.add_argument("--miopen_find", action="store_true")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    if args.miopen_find:
        torch.backends.cudnn.benchmark = True
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        if "kernels" in parts:
            kernels_part(_lib.lib(), stream)
        if "network" in parts:
            network_part(stream, args.miopen_find)


if __name__ == "__main__":
    main()
