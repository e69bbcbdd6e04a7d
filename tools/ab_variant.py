"""A/B of the sphere rasterizer forward / backward between the product library and a variant built with extra -D flags:
    python tools/ab_variant.py build -DSHR_ROW_PAD=4 ...     (anywhere: tools/libspherehand_exp.so; any right-result tunable)
    python tools/ab_variant.py build:NAME -DSHR_... ...    (several variants side by side: tools/libspherehand_exp_NAME.so)
(another commit's library copied to tools/libspherehand_exp_NAME.so is a variant like any other)
    python tools/ab_variant.py                          (GPU box: alternating timings at 256 / 1152 / 9216 crops, same-bits check,
                                                         the product library against every variant library found)
Environment: S (image size), NS (crop counts), MSE=1 (the fused render-and-compare kernel as well: its SSE partials, gradient
partials and depth output are compared with the product's, byte for byte), C5=1 (config 5's wide boxes), NODEPTH=1, REPS_X (a
factor on the launches per timing).  Every round prints a line per library; the medians of the three rounds and their ratio
to the PRODUCT's follow at the end (a variant's percentage is variant / product - 1: with the parent's library as the
variant, a positive figure means the tree is FASTER than the parent -- the opposite sign of tables that compare against the parent).  The exit status is 1 if any line said `same bits: False`."""
import ctypes, glob, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXP = os.path.join(ROOT, "tools", "libspherehand_exp.so")


def build(flags, name=""):
    """(SRC=data_to_model in the environment: the variant flags go to that translation unit instead of sphere_raster)"""
    global EXP
    if name:
        EXP = os.path.join(ROOT, "tools", "libspherehand_exp_%s.so" % name)
    from spherehand_amd import build as b
    b.build()
    unit = os.environ.get("SRC", "sphere_raster")
    obj = "/tmp/%s_exp%s.o" % (unit, name)
    subprocess.check_call([b.HIPCC] + [f for f in b.FLAGS if f != "-shared"] + flags +
                          ["-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(b.PKG, "csrc"), "-o", obj,
                           os.path.join(b.PKG, "csrc", unit + ".hip")])
    objs = [o for o in glob.glob(os.path.join(b.OBJ_DIR, "*.o")) if not o.endswith(unit + ".o")]
    subprocess.check_call([b.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", EXP, obj] + objs)
    print(EXP, flags)


def main():
    import torch
    import bench
    from spherehand_amd import _lib, hand_model
    from spherehand_amd.joint_angle import sample_poses
    from spherehand_amd.kinematicsTransformation import HandTransformationMat
    from spherehand_amd.render import HandBallPrimitiveRender
    vp, i = ctypes.c_void_p, ctypes.c_int
    libs = {"product": _lib.lib()}
    for f in sorted(glob.glob(os.path.join(ROOT, "tools", "libspherehand_exp*.so"))):
        libs[os.path.basename(f)[len("libspherehand_exp"):-3].lstrip("_") or "variant"] = ctypes.CDLL(f)
    for l in libs.values():
        l.shr_sphere_raster_fwd_ex.argtypes = [vp, i, i, i, i, vp, vp, i, vp]
        l.shr_sphere_raster_bwd.argtypes = [vp, vp, vp, i, i, i, i, vp, vp]
        l.shr_sphere_raster_mse.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, vp, vp]
        l.shr_sphere_raster_mse_regions.argtypes = [i, i]
    dev = torch.device("cuda", 0)
    S, J = int(os.environ.get("S", 128)), 41
    mesh = hand_model.load_mesh()
    fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).to(dev)
    hbr = HandBallPrimitiveRender(mesh["bones"], S, S).to(dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        times, all_same = {}, True
        for n in [int(v) for v in os.environ.get("NS", "256,1152,9216").split(",")]:
            with torch.no_grad():
                sph = hbr.spheres(fk(sample_poses(n, seed=7).to(dev))).contiguous()
            obs = index = None
            if os.environ.get("C5"):    # config 5's own projections (WIDE boxes) and observed images (three crops share one): n = 9 B
                from spherehand_amd.datasets import SyntheticMultiviewDataset
                from spherehand_amd.multiview_utility import MutualProjectionLoss
                ds = SyntheticMultiviewDataset(mesh, n // 9, S, seed=0, device=dev)
                crit = MutualProjectionLoss(S, mesh).to(dev)
                with torch.no_grad():
                    _, pts = crit.mutual_projection(ds.cam.to(dev), ds.inv_cam.to(dev), ds.joints.to(dev) + torch.randn(ds.joints.shape, device=dev))
                rad = crit.data_to_model_criterion.radiuses.view(-1)
                sph = torch.cat([pts.squeeze(-1).reshape(n, J, 3), rad.view(1, J, 1).expand(n, J, 1)], -1).contiguous()
                obs = ds.dms.to(dev).view(n // 3, S, S).contiguous()
                index = crit._indices(n // 9, 3, dev)[0]
            depth = torch.empty(n, S, S, device=dev); owner = torch.empty(n, S, S, device=dev, dtype=torch.uint8)
            grad = torch.randn(n, S, S, device=dev); gs = torch.empty(n, J, 4, device=dev)
            p = [t.data_ptr() for t in (sph, depth, owner, grad, gs)]
            reps = (200 if n == 256 else (40 if n == 1152 else 8)) * int(os.environ.get("REPS_X", 1))
            ref, tgt = {}, obs
            for rnd in range(3):
                for name, l in libs.items():
                    f = lambda s: l.shr_sphere_raster_fwd_ex(p[0], n, J, S, S, p[1], p[2], 1, s)
                    f0 = lambda s: l.shr_sphere_raster_fwd_ex(p[0], n, J, S, S, p[1], None, 0, s)
                    b = lambda s: l.shr_sphere_raster_bwd(p[0], p[3], p[2], n, J, S, S, p[4], s)
                    assert f(stream.cuda_stream) == 0
                    tf = bench.mean_launch_us(f, stream, reps, 3, 3, warm_ms=30.0)
                    tb = bench.mean_launch_us(b, stream, reps, 3, 3, warm_ms=30.0)
                    t0 = bench.mean_launch_us(f0, stream, reps, 3, 3, warm_ms=30.0)
                    f(stream.cuda_stream); b(stream.cuda_stream); stream.synchronize()
                    key = (depth.clone(), gs.clone())
                    ok = name == "product" or (torch.equal(key[0], ref["d"]) and torch.equal(key[1], ref["g"]))
                    same = "" if name == "product" else "  same bits: %s" % ok
                    if name == "product": ref.update(d=key[0], g=key[1])
                    rows = [("fwd+owner", tf), ("bwd", tb), ("fwd depth-only", t0)]
                    if os.environ.get("MSE"):   # the fused render-and-compare kernel on the same crops (target: the depth map + noise)
                        R = l.shr_sphere_raster_mse_regions(S, S)
                        if tgt is None:         # (one target for every library and round: the product's first depth map + noise)
                            tgt = (ref["d"] + 3.0 * torch.randn_like(depth)).contiguous()
                        sse = torch.zeros(n * R, device=dev); gsp = torch.zeros(n * R * J * 4, device=dev)
                        m = lambda s: l.shr_sphere_raster_mse(p[0], n, J, S, S, tgt.data_ptr(), None if index is None else index.data_ptr(),
                                                              None if os.environ.get("NODEPTH") else p[1], sse.data_ptr(), gsp.data_ptr(), s)
                        depth.zero_()
                        assert m(stream.cuda_stream) == 0
                        stream.synchronize()
                        mkey = (sse.clone(), gsp.clone(), depth.clone())   # raw tensors: SSE partials, gradient partials, depth output
                        mok = name == "product" or all(torch.equal(a, b) for a, b in zip(mkey, ref["m"]))
                        if name == "product" and "m" not in ref: ref["m"] = mkey
                        tm = bench.mean_launch_us(m, stream, reps, 3, 3, warm_ms=30.0)
                        rows.append(("render-and-compare", tm))
                        print("n %5d %-10s render-and-compare %7.2f us%s" % (n, name, tm, "" if name == "product" else "  same bits: %s" % mok), flush=True)
                        ok = ok and mok
                    all_same = all_same and ok
                    for row, t in rows: times.setdefault((n, row), {}).setdefault(name, []).append(t)
                    print("n %5d %-10s fwd+owner %7.2f  bwd %7.2f  fwd depth-only %7.2f us%s" % (n, name, tf, tb, t0, same), flush=True)
        for (n, row), by in times.items():   # medians of the rounds, and each library's against the product's
            med = {name: statistics.median(v) for name, v in by.items()}
            print("median n %5d %-18s " % (n, row) + "  ".join("%s %.2f (%+.2f %%)" % (k, v, 100.0 * (v / med["product"] - 1.0)) for k, v in med.items()), flush=True)
    if not all_same:
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1].startswith("build"):
        build(sys.argv[2:], sys.argv[1][6:])
    else:
        main()
