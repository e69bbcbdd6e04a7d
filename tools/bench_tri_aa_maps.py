"""The antialias pass over multi-channel maps through the C ABI (no Python op in the loop), HIP events on the launching
stream, hand crops from sampled poses (the 1721 distinct vertices, so the faces' ids are already welded), the values
shr_tri_interp_fwd's maps of C = 3 and C = 17 per-crop attributes:
  forward          shr_tri_antialias_maps_fwd
  backward         shr_tri_antialias_maps_bwd -> grad_values [B,C,H,W] and grad_vertices [B,NV,4]; each part alone
at 256 crops @640x640 and 64 crops @640x480, against
  copy             a device copy of the maps (the copy rate): the forward's floor is a read of owner and depth and a read
                   and a write of C planes, 8 + 8 C bytes per pixel
  planes           the composition the single-plane entries allow: C calls of shr_tri_antialias_fwd / _bwd on the same
                   planes (laid out [C,B,H,W] beforehand, outside the timing), the C vertex gradients summed.
The entries under comparison are timed in alternation, `--rounds` times; a line reports the mean and the spread (min ..
max) of the rounds.  Every case runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/bench_tri_aa_maps.py [--rounds 3] [--timeout 240]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(256, 640, 640, 3), (256, 640, 640, 17), (64, 640, 480, 3), (64, 640, 480, 17)]


def case(B, W, H, C, rounds):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from spherehand_amd import _lib, hand_model, ops
    from spherehand_amd.joint_angle import sample_poses
    from spherehand_amd.kinematicsTransformation import HandTransformationMat
    from spherehand_amd.render import DepthRender

    mesh = hand_model.load_mesh()
    lib = _lib.lib()
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
    stream = torch.cuda.Stream()
    p = lambda t: t.data_ptr()  # noqa: E731
    with torch.cuda.stream(stream):
        dr = DepthRender(mesh, 128).cuda()
        with torch.no_grad():
            verts = dr.lbs(fk(sample_poses(B, seed=1).cuda()).contiguous(), dr.camera, None).contiguous()
        faces = dr.rasterizer.faces_i32
        edges = torch.from_numpy(ops.tri_edge_table(faces.cpu())).cuda()
        NV, F = verts.shape[1], faces.shape[0]
        depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, verts, faces)
        values = ops.tri_interpolate(torch.randn(B, NV, C, device="cuda"), owner, verts, faces)
        out, copy = torch.empty_like(values), torch.empty_like(values)
        g = torch.randn(B, C, H, W, device="cuda")
        g_c, g_v = torch.empty_like(values), torch.empty(B, NV, 4, device="cuda")
        ws = torch.empty(lib.shr_tri_antialias_maps_bwd_workspace_bytes(B, NV), dtype=torch.uint8, device="cuda")
        # the composition's planes: [C,B,H,W], every plane a contiguous [B,H,W] the single-plane entries take
        v_pl, g_pl = values.transpose(0, 1).contiguous(), g.transpose(0, 1).contiguous()
        o_pl, gc_pl = torch.empty_like(v_pl), torch.empty_like(v_pl)
        gv_pl, gv_sum = torch.empty(C, B, NV, 4, device="cuda"), torch.empty(B, NV, 4, device="cuda")
        geo = (p(depth), p(owner), p(verts), p(faces), p(edges), B, NV, F, W, H)

        def copy_values(s):   # (on the current stream: the timed one)
            copy.copy_(values)
            return 0

        def planes_fwd(s):
            rc = 0
            for ch in range(C):
                rc |= lib.shr_tri_antialias_fwd(p(v_pl[ch]), *geo, p(o_pl[ch]), s)
            return rc

        def planes_bwd(s):
            rc = 0
            for ch in range(C):
                rc |= lib.shr_tri_antialias_bwd(p(v_pl[ch]), *geo, p(g_pl[ch]), p(gc_pl[ch]), p(gv_pl[ch]), p(ws), s)
            torch.sum(gv_pl, 0, out=gv_sum)
            return rc

        runs = {
            "copy": copy_values,
            "forward": lambda s: lib.shr_tri_antialias_maps_fwd(p(values), *geo, C, p(out), s),
            "planes forward": planes_fwd,
            "backward": lambda s: lib.shr_tri_antialias_maps_bwd(p(values), *geo, C, p(g), p(g_c), p(g_v), p(ws), s),
            "planes backward": planes_bwd,
            "backward values": lambda s: lib.shr_tri_antialias_maps_bwd(p(values), *geo, C, p(g), p(g_c), None, None, s),
            "backward vertices": lambda s: lib.shr_tri_antialias_maps_bwd(p(values), *geo, C, p(g), None, p(g_v), p(ws), s),
        }
        for name, fn in runs.items():
            assert fn(stream.cuda_stream) == 0, name
        stream.synchronize()
        # the two routes give the same maps (bit for bit) and the same vertex gradient up to the fixed-point unit
        assert torch.equal(out, o_pl.transpose(0, 1)) and torch.equal(g_c, gc_pl.transpose(0, 1))
        dev_v = (g_v - gv_sum).abs().max().item() / max(gv_sum.abs().max().item(), 1e-30)
        changed = (out != values).any(1).sum().item() / B
        rows = {name: [] for name in runs}
        for _ in range(rounds):                      # alternating: every entry once per round
            for name, fn in runs.items():
                rows[name].append(bench.mean_launch_us(fn, stream, 5, 2, 1, warm_ms=20.0))
        mean = {k: sum(v) / len(v) for k, v in rows.items()}
        npix = B * W * H
        copy_rate = 8 * C * npix / (mean["copy"] * 1e-6) / 1e12
        floor_us = (8 + 8 * C) * npix / (copy_rate * 1e12) * 1e6
        print("B=%d %dx%d C=%d (%.0f owned, %.0f blended pixels per crop, NV %d): " %
              (B, W, H, C, (owner >= 0).sum().item() / B, changed, NV)
              + " | ".join("%s %.1f us (%.1f .. %.1f)" % (k, mean[k], min(v), max(v)) for k, v in rows.items())
              + " | copy %.2f TB/s, forward floor %.1f us (x%.2f)" % (copy_rate, floor_us, mean["forward"] / floor_us)
              + " | planes / maps: forward x%.2f, backward x%.2f" % (mean["planes forward"] / mean["forward"],
                                                                    mean["planes backward"] / mean["backward"])
              + " | vertex gradient against the summed planes: %.2e of its maximum" % dev_v, flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", help="B,W,H,C: run this one case in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    a = ap.parse_args()
    if a.case:
        case(*[int(t) for t in a.case.split(",")], a.rounds)
        sys.exit(0)
    for c in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", ",".join(map(str, c)),
                            "--rounds", str(a.rounds)], timeout=a.timeout)
        if r.returncode != 0:     # nothing more is started on a device that has just failed a case
            sys.exit("case %s ended with status %d" % (c, r.returncode))
