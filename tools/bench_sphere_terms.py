"""The sphere fit's `*_normal` entries of THIS build beside the PARENT commit's library (--parent-lib), loaded in one process:
what a change that restates their shared text (normal_eq.h, sphere_icp_scan.h) must neither change by a bit nor slow down.
HIP events on the launching stream, through the C ABI (no Python op in the loop):
  icp          shr_sphere_icp_normal, 256 samples at 128 x 128, one view and three views
  radii        shr_sphere_icp_radii_normal, the same crops in groups of 8 frames
  render       shr_sphere_render_normal, written and with accumulate = 1, one view and three views
  prior        shr_sphere_prior_normal, keypoints and limits, written and with accumulate = 1, one view and three views
  collision    shr_sphere_collision_normal with the hand's table (the reference's pairs at 6 mm), written and accumulate = 1
  pose_vae     shr_pose_vae_normal with the latent rows, written and accumulate = 1
  temporal     shr_sphere_temporal_normal, the 256 frames as 32 x 8 and as 8 x 32, written and accumulate = 1
  accel        shr_sphere_accel_normal, the same, written and with accumulate = 1 and accumulate_E = 1
  mesh_icp     shr_pose_icp_normal of the mesh fit (icp_tile.h takes the entry map), 256 crops at 128 x 128
the hand's 41 spheres; poses, observations, keypoints and starts as tools/bench_sphere_collision.py makes them (the sequence
entries see the same 256 frames under both groupings).  Both libraries read the SAME input buffers and write their OWN
output buffers; an accumulating form starts from the same seeded A, g, cost (and E).  Every row is run from both libraries
before anything is timed, and every output buffer of the two is compared bit for bit; then alternated, three rounds, the odd
ones in reverse order (every round is printed; the summary is the median, the spread is max - min over the rounds).  The
condition, per row: this build's median is not above the parent library's by more than the run-to-run spread (the larger of
the two); the tool exits with status 1 where it is missed, and says so where no parent library was given (status 0: nothing
to hold)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib, hand_model, ops  # noqa: E402
from spherehand_amd.joint_angle import sample_poses_batched  # noqa: E402
from spherehand_amd.render import (MeshPoseFitter, MeshVertices, PoseVaePrior, SphereCollisionPoseFitter,  # noqa: E402
                                   TriangleDepthRaster)
from tools.bench_sphere_icp import VIEWS  # noqa: E402

ROUNDS = 3
B, S, N = 256, 128, 8
SIGMA_K = 2.0
ENTRIES = ("shr_sphere_icp_normal", "shr_sphere_icp_radii_normal", "shr_sphere_render_normal", "shr_sphere_prior_normal",
           "shr_sphere_collision_normal", "shr_pose_vae_normal", "shr_sphere_temporal_normal", "shr_sphere_accel_normal",
           "shr_pose_icp_normal")


def load_parent(path):
    """The parent commit's library beside this build's: its own handle, the entries' signatures set from this loader's (the
    ABI is the same)."""
    h = ctypes.CDLL(os.path.abspath(path))
    for name in ENTRIES:
        getattr(h, name).argtypes, getattr(h, name).restype = _lib.SIGNATURES[name]
    return h


def inputs(mesh):
    """What both libraries read: made once, by this build's ops (none of it is an output of an entry under test)."""
    fit = SphereCollisionPoseFitter(mesh, S, S).cuda()
    tabs = (fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv)
    J = fit.num_spheres
    gen = torch.Generator().manual_seed(B)
    truth = sample_poses_batched(B, generator=gen)
    truth[:, 3:5] = 5.0 * torch.randn(B, 2, generator=gen)
    truth[:, 5] = 50.0
    start = truth + 0.1 * torch.randn(B, 26, generator=gen)
    start[:, 3:6] = truth[:, 3:6] + 2.0 * torch.randn(B, 3, generator=gen)
    noise = SIGMA_K * torch.randn(B, 3, J, 3, generator=gen)
    rnd64 = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    base = dict(A=rnd64(B, 26, 26), g=rnd64(B, 26), cost=rnd64(B).abs(), E=rnd64(B, 26, 26))
    base["A"] = base["A"] + base["A"].transpose(1, 2)
    truth, start = truth.float().cuda(), start.float().cuda()
    kp_true, _ = ops.pose_keypoints_jacobian(truth, *tabs, True)
    kp, jac = ops.pose_keypoints_jacobian(start, *tabs, True)
    d = dict(J=J, tabs=tabs, start=start, kp=kp, jac=jac, radii=fit.radii, lower=fit.lower, upper=fit.upper,
             pairs=(fit.pair_a, fit.pair_b, fit.pair_min), p2m=tuple(fit.pixel_to_model), fg=fit.fg_max, bg=fit.background,
             base={k: v.contiguous().cuda() for k, v in base.items()}, blob=PoseVaePrior(weight=0.1, latent_weight=1.0).cuda().blob,
             group_radii=fit.radii[None].expand(B // N, J).contiguous())
    for V in (1, 3):
        view = torch.stack(VIEWS[:V]).cuda().expand(B, V, 4, 4).contiguous()
        spheres = ops.view_vertices(kp_true, view).clone()
        targets = (spheres[..., :3] + noise[:, :V].cuda()).contiguous()
        spheres[..., 3] = fit.radii
        observed = torch.clamp(ops.sphere_raster_fwd(spheres.view(B * V, J, 4).contiguous(), S, S), max=100.0)
        d[V] = dict(view=view, targets=targets, observed=observed.view(B, V, S, S).contiguous(),
                    centres=ops.view_vertices(kp, view).contiguous())
    # the mesh fit's crops
    mfit = MeshPoseFitter(mesh, S, S).cuda()
    lbs = mfit.vertices.lbs
    pix = MeshVertices(mesh, camera=MeshVertices.pixel_camera(S, S)).cuda()
    with torch.no_grad():
        mobs = torch.clamp(TriangleDepthRaster(S, S, pix.faces).cuda()(pix.pose_vertices(mfit.fk, truth)), max=100.0).contiguous()
        verts = torch.empty(B, mfit.vertices.num_vertices, 4, device="cuda")
        assert _lib.lib().shr_pose_vertices_fwd(start.data_ptr(), B, mfit.fk.offset.data_ptr(), mfit.fk.offset_inv.data_ptr(),
                                                verts.shape[1], lbs.skin_vertex_start.data_ptr(), lbs.skin_bone.data_ptr(),
                                                lbs.skin_wv.data_ptr(), 1, 0, 0.0, 0.0, 1.0, 1.0, None, verts.data_ptr(), None,
                                                torch.cuda.current_stream().cuda_stream) == 0
        dist, face = ops.mesh_data_to_model(mobs, verts, mfit.faces_i32, mfit.pixel_to_model, mfit.fg_max, mfit.max_dist)
    d["mesh"] = dict(observed=mobs, verts=verts, faces=mfit.faces_i32, dist=dist.contiguous(), face=face.contiguous(),
                     tabs=(mfit.fk.offset, mfit.fk.offset_inv, lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv),
                     p2m=tuple(mfit.pixel_to_model), fg=mfit.fg_max, md=mfit.max_dist)
    return d


def runs_of(h, d):
    """{label: (fn(stream), outputs, reset)} of one library: `outputs` are the buffers the call writes, `reset` puts the seeded
    base into the ones an accumulating form adds to."""
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    f32 = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    J, kp, jac, radii, start, base = d["J"], d["kp"], d["jac"], d["radii"], d["start"], d["base"]
    runs = {}

    def add(label, make, extra, acc, with_E=False):
        """make(A, g, cost, E, *extra) -> fn(stream); the row's own A, g, cost (and E)."""
        A, g, cost, E = f64(B, 26, 26), f64(B, 26), f64(B), f64(B, 26, 26) if with_E else None
        held = [A, g, cost] + ([E] if with_E else [])

        def reset():
            for t, k in zip(held, ("A", "g", "cost", "E")):
                t.copy_(base[k]) if acc else t.zero_()
        runs[label] = (make(A, g, cost, E, *extra), held + list(extra), reset)

    for V in (1, 3):
        v = d[V]
        obs, view, centres, targets = v["observed"], v["view"], v["centres"], v["targets"]
        ws_bytes = max(16, h.shr_sphere_icp_radii_normal_workspace_bytes(B, V, J, S, S))
        ws = lambda: torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")  # noqa: E731   (its padding is compared too)
        add("icp V=%d" % V, lambda A, g, c, E, n, m, dist, own, w, obs=obs, view=view, centres=centres, V=V: lambda s: h.shr_sphere_icp_normal(
            p(obs), p(centres), p(radii), p(view), p(jac), B, V, J, S, S, *d["p2m"], d["fg"], float("inf"), p(A), p(g), p(c), p(n), p(m),
            p(dist), p(own), p(w), s), (i32(B), f64(B, J, 12), f32(B, V, S, S), i32(B, V, S, S), ws()), False)
        add("radii V=%d" % V, lambda A, g, c, E, n, C, R, gs, m, w, obs=obs, view=view, centres=centres, V=V: lambda s:
            h.shr_sphere_icp_radii_normal(p(obs), p(centres), p(d["group_radii"]), p(view), p(jac), B, V, J, S, S, N, *d["p2m"], d["fg"],
                                          float("inf"), p(A), p(g), p(c), p(n), p(C), p(R), p(gs), p(m), None, None, p(w), s),
            (i32(B), f64(B, 26, J), f64(B // N, J, J), f64(B // N, J), f64(B, J, 16), ws()), False)
        for acc in (0, 1):
            add("render V=%d acc=%d" % (V, acc), lambda A, g, c, E, n, m, depth, own, w, obs=obs, view=view, centres=centres, V=V,
                acc=acc: lambda s: h.shr_sphere_render_normal(
                    p(obs), p(centres), p(radii), p(view), p(jac), B, V, J, S, S, *d["p2m"], d["fg"], d["bg"], float("inf"), 0.5, acc,
                    p(A), p(g), p(c), p(n), p(m), p(depth), p(own), p(w), s),
                (i32(B), f64(B, J, 12), f32(B, V, S, S), i32(B, V, S, S), ws()), acc)
            add("prior V=%d acc=%d" % (V, acc), lambda A, g, c, E, n, m, view=view, centres=centres, targets=targets, V=V, acc=acc:
                lambda s: h.shr_sphere_prior_normal(p(centres), p(view), p(jac), p(start), p(targets), None, 0.25, 30.0, p(d["lower"]),
                                                    p(d["upper"]), 10.0, B, V, J, acc, p(A), p(g), p(c), p(n), p(m), None, s),
                (i32(B, 2), f64(B, J, 12)), acc)
    pa, pb, pm = d["pairs"]
    K, blob = pa.shape[0], d["blob"]
    for acc in (0, 1):
        add("collision acc=%d" % acc, lambda A, g, c, E, n, pen, acc=acc: lambda s: h.shr_sphere_collision_normal(
            p(kp), p(jac), p(pa), p(pb), p(pm), 2.0, B, J, K, acc, p(A), p(g), p(c), p(n), p(pen), None, s), (i32(B), f64(B, K)), acc)
        add("pose_vae acc=%d" % acc, lambda A, g, c, E, res, lat, mask, acc=acc: lambda s: h.shr_pose_vae_normal(
            p(kp), p(jac), p(blob), blob.shape[0], 0.1, 1.0, B, J, acc, p(A), p(g), p(c), p(res), p(lat), p(mask), None, s),
            (f64(B, 123), f64(B, 32), i32(B, 32)), acc)
        for T in (8, 32):
            shape = "%dx%d" % (B // T, T)
            add("temporal %s acc=%d" % (shape, acc), lambda A, g, c, E, n, T=T, acc=acc: lambda s: h.shr_sphere_temporal_normal(
                p(kp), p(jac), None, 1.5, 40.0, B, T, J, acc, p(A), p(g), p(E), p(c), p(n), None, s), (i32(B),), acc, True)
            add("accel %s acc=%d" % (shape, acc), lambda A, g, c, E, F, n, T=T, acc=acc: lambda s: h.shr_sphere_accel_normal(
                p(kp), p(jac), None, 0.75, 40.0, B, T, J, acc, acc, p(A), p(g), p(E), p(F), p(c), p(n), None, s),
                (f64(B, 26, 26), i32(B)), acc, True)
    m = d["mesh"]
    NV, F = m["verts"].shape[1], m["faces"].shape[0]
    add("mesh_icp", lambda A, g, c, E, n, w: lambda s: h.shr_pose_icp_normal(
        p(m["observed"]), p(m["verts"]), p(m["faces"]), p(m["dist"]), p(m["face"]), p(start), *(p(t) for t in m["tabs"]), 1, B, NV, F,
        S, S, *m["p2m"], m["fg"], m["md"], p(A), p(g), p(c), p(n), p(w), s),
        (i32(B), torch.zeros(max(16, h.shr_pose_icp_normal_workspace_bytes(B, S, S)), dtype=torch.uint8, device="cuda")), False)
    return runs


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def main(parent_lib=None):
    lib = _lib.lib()
    parent = load_parent(parent_lib) if parent_lib else None
    if parent is None:
        print("no --parent-lib: the entries are not held against the parent commit's library", flush=True)
    stream = torch.cuda.Stream()
    within = True
    with torch.cuda.stream(stream):
        d = inputs(hand_model.load_mesh())
        s0 = stream.cuda_stream
        this = runs_of(lib, d)
        theirs = runs_of(parent, d) if parent is not None else {}
        runs = {(k, who): r[k][0] for k in this for who, r in (("this", this), ("parent", theirs)) if k in r}
        for k in this:                                             # every row from both libraries before anything is timed,
            for r in (this, theirs):                               # and every output buffer of the two compared bit for bit
                if k in r:
                    r[k][2]()
                    assert r[k][0](s0) == 0, k
            stream.synchronize()
            if parent is not None:
                for i, (a, b) in enumerate(zip(this[k][1], theirs[k][1])):
                    assert same_bits(a, b), "%s: output buffer %d differs from the parent library's" % (k, i)
        if parent is not None:
            print("every output buffer of the %d rows: the parent library's bits" % len(this), flush=True)
        for key, fn in runs.items():
            for _ in range(3):
                assert fn(s0) == 0, key
        stream.synchronize()
        # (the accumulating entries add to A, g and cost on every call: the timed repetitions let them grow, which costs the same)
        us = {k: [] for k in runs}
        for rnd in range(ROUNDS):
            for key, fn in (list(runs.items()) if rnd % 2 == 0 else list(runs.items())[::-1]):      # (odd rounds in reverse order)
                us[key].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
            print("  round %d: %s" % (rnd, " | ".join("%s/%s %.2f" % (k[0], k[1], v[-1]) for k, v in us.items())), flush=True)
        spread = {k: float(max(v) - min(v)) for k, v in us.items()}
        us = {k: float(np.median(v)) for k, v in us.items()}
        print("| entry and shape | this build, us | spread | parent, us | spread | difference | |\n|---|---|---|---|---|---|---|")
        for k in this:
            if parent is None:
                print("| %s | %.2f | %.2f | | | | |" % (k, us[k, "this"], spread[k, "this"]), flush=True)
                continue
            diff, bar = us[k, "this"] - us[k, "parent"], max(spread[k, "this"], spread[k, "parent"])
            within = within and diff <= bar
            print("| %s | %.2f | %.2f | %.2f | %.2f | %+.2f | %s the spread |"
                  % (k, us[k, "this"], spread[k, "this"], us[k, "parent"], spread[k, "parent"], diff,
                     "within" if diff <= bar else "SLOWER than"), flush=True)
    return within


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None, help="libspherehand_hip.so built from the parent commit")
    sys.exit(0 if main(ap.parse_args().parent_lib) else 1)
