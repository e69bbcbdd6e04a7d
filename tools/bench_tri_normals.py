"""Vertex normals, unit3 and the normal-map module, HIP events on the launching stream, hand crops from sampled poses at
both weldings (10 144 vertices welded into 1 721 points; the 1 721 distinct vertices), 256 crops @640x640 and 64 crops
@640x480:
  normals forward / backward   shr_tri_vertex_normals_fwd / _bwd through the C ABI (no Python op in the loop)
  unit3 forward / backward     shr_unit3_maps_fwd / _bwd on the interpolated normal maps, and their byte floors at the
                               tool's own copy rate: 24 B/px forward (read 3 planes, write 3), 36 B/px backward
  module forward / backward    render.MeshNormalRaster (owner forward, normals, interpolation, unit3) and its autograd
each against the torch composition a user writes without the kernels -- index_add_ of the face cross products and
F.normalize, with torch's autograd; for the module the same pipeline with those two stages in torch -- in the same
process, alternated, three rounds (every round is printed; the summary is the median)."""
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
from spherehand_amd.render import DepthRender, MeshNormalRaster  # noqa: E402

ROUNDS = 3


def torch_normals(points, faces, point, NP):
    P, f = points[..., :3], faces.long()
    p0 = P[:, f[:, 0]]
    nf = torch.cross(P[:, f[:, 1]] - p0, P[:, f[:, 2]] - p0, dim=-1)
    N = torch.zeros(P.shape[0], NP, 3, device=P.device)
    for k in range(3):
        N.index_add_(1, point[f[:, k]], nf)
    return Fn.normalize(N[:, point], dim=-1)


def timed(fn, reps=3):
    """mean us of fn() over `reps` calls on the current stream, after one warm-up call"""
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def fwd_bwd(make, leaves, g):
    """(forward us, backward us) of out = make() and autograd.grad(out, leaves, g), timed apart"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for rep in range(3):                                        # (the first repetition warms up)
        ev[0].record()
        out = make()
        ev[1].record()
        torch.autograd.grad(out, leaves, g)
        ev[2].record()
        ev[2].synchronize()
        if rep:
            tf += ev[0].elapsed_time(ev[1]) * 1e3 / 2
            tb += ev[1].elapsed_time(ev[2]) * 1e3 / 2
        del out
    return tf, tb


def med(rows):
    return " | ".join("%s %.1f us" % (k, float(np.median(v))) for k, v in rows.items())


mesh = hand_model.load_mesh()
lib = _lib.lib()
fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
stream = torch.cuda.Stream()
p = lambda t: t.data_ptr()  # noqa: E731
with torch.cuda.stream(stream):
    for B, W, H in ((256, 640, 640), (64, 640, 480)):
        dr = DepthRender(mesh, 128).cuda()
        with torch.no_grad():
            distinct = dr.lbs(fk(sample_poses(B, seed=1).cuda()).contiguous(), dr.camera, None).contiguous()
        index = np.asarray(dr.lbs.vertex_index, np.int64)
        faces_d = dr.rasterizer.faces_i32.cpu().numpy()
        faces_all = np.array(mesh["faces"], np.int64)
        faces_all[:, [0, 1]] = faces_all[:, [1, 0]]
        npix = B * W * H
        for label, verts, faces_np, weld in (
                ("10144 welded", distinct[:, torch.from_numpy(index).cuda()].contiguous(), faces_all, index),
                ("1721 distinct", distinct, faces_d, None)):
            NV = verts.shape[1]
            faces = torch.from_numpy(np.ascontiguousarray(faces_np, np.int32)).cuda()
            F = faces.shape[0]
            T = ops.tri_vertex_tables(faces_np, NV, weld).to("cuda")
            NP, NI, NO = T.NP, T.inc.numel(), T.own.numel()
            point = T.point.long()
            normals, g_n, g_p = (torch.empty(B, NV, 4, device="cuda") for _ in range(3))
            g_n.normal_()
            ws = torch.empty(max(16, lib.shr_tri_vertex_normals_bwd_workspace_bytes(B, NP)), dtype=torch.uint8, device="cuda")
            tabs = (p(verts), p(faces), p(T.point), p(T.inc_start), p(T.inc), p(T.copy_start), p(T.copy))
            _, owner = ops.tri_raster_indexed_owner_fwd(W, H, verts, faces)
            maps = ops.tri_interpolate(ops.tri_vertex_normals(verts, faces, T)[..., :3].contiguous(), owner, verts, faces)
            out, g_m, g_o = torch.empty_like(maps), torch.empty_like(maps), torch.randn_like(maps)
            copy = torch.empty_like(maps)

            def copy_maps(s):   # (on the current stream: the timed one)
                copy.copy_(maps)
                return 0

            runs = {
                "copy": copy_maps,
                "normals forward": lambda s: lib.shr_tri_vertex_normals_fwd(*tabs, B, NV, F, NP, NI, p(normals), None, s),
                "normals backward": lambda s: lib.shr_tri_vertex_normals_bwd(*tabs, p(T.own_start), p(T.own), B, NV, F, NP, NI,
                                                                             NO, p(g_n), p(g_p), p(ws), s),
                "unit3 forward": lambda s: lib.shr_unit3_maps_fwd(p(maps), B, W, H, p(out), s),
                "unit3 backward": lambda s: lib.shr_unit3_maps_bwd(p(maps), p(g_o), B, W, H, p(g_m), s),
            }
            for name, fn in runs.items():
                assert fn(stream.cuda_stream) == 0, name
            stream.synchronize()
            module = MeshNormalRaster(W, H, faces_np, right_hand=False, np_vertices=weld).cuda()
            turned = module.normal_faces_i32

            def torch_module(v):
                _, own = ops.TriRasterIndexedOwner.apply(v, faces, W, H)
                n = torch_normals(v, turned, point, NP)
                return Fn.normalize(ops.TriInterpolate.apply(n, own, v, faces), dim=1)

            ours, theirs = {k: [] for k in runs}, {}
            for k in ("module forward", "module backward"):
                ours[k] = []
            for k in ("normals forward", "normals backward", "unit3 forward", "unit3 backward", "module forward", "module backward"):
                theirs[k] = []
            for rnd in range(ROUNDS):
                for name, fn in runs.items():
                    ours[name].append(bench.mean_launch_us(fn, stream, 10, 3, 3, warm_ms=20.0))
                vs = verts.clone().requires_grad_(True)
                a, b = fwd_bwd(lambda: torch_normals(vs, faces, point, NP), (vs,), g_n[..., :3])
                theirs["normals forward"].append(a)
                theirs["normals backward"].append(b)
                ms = maps.clone().requires_grad_(True)
                a, b = fwd_bwd(lambda: Fn.normalize(ms, dim=1), (ms,), g_o)
                theirs["unit3 forward"].append(a)
                theirs["unit3 backward"].append(b)
                del ms
                a, b = fwd_bwd(lambda: module(vs)[0], (vs,), g_o)
                ours["module forward"].append(a)
                ours["module backward"].append(b)
                a, b = fwd_bwd(lambda: torch_module(vs), (vs,), g_o)
                theirs["module forward"].append(a)
                theirs["module backward"].append(b)
                print("  round %d: ours %s || torch %s" % (rnd, " | ".join("%s %.1f" % (k, v[-1]) for k, v in ours.items()),
                                                         " | ".join("%s %.1f" % (k, v[-1]) for k, v in theirs.items())), flush=True)
            copy_us = float(np.median(ours["copy"]))
            rate = 24 * npix / (copy_us * 1e-6) / 1e12            # the copy reads and writes three planes: 24 B/px
            ff, fb = 24 * npix / (rate * 1e12) * 1e6, 36 * npix / (rate * 1e12) * 1e6
            uf, ub = float(np.median(ours["unit3 forward"])), float(np.median(ours["unit3 backward"]))
            print("B=%d %dx%d %s (%.0f owned pixels per crop, NV %d, NP %d, F %d): ours: %s || torch: %s || copy %.2f TB/s; "
                  "unit3 floors: forward %.1f us (x%.2f), backward %.1f us (x%.2f)"
                  % (B, W, H, label, (owner >= 0).sum().item() / B, NV, NP, F, med(ours), med(theirs), rate, ff, uf / ff,
                     fb, ub / fb), flush=True)
            del maps, out, g_m, g_o, copy, module
