"""Randomised differential testing of the HIP kernels against the CPU oracle (run on the GPU box; the permanent
tests in tests/ are fixed seeds, this explores).

    python tools/fuzz.py [seconds per family] [seed] [families]      # the long run (profiles/rNN_fuzz_summary.txt)
    fuzz.run(families, cases, seconds, seed)                          # tests/test_fuzz_gpu.py: a bounded, seeded slice
"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_rasterization
from oracle import oracle
from spherehand_amd import ops
oracle.build()
rs = np.random.RandomState(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
fails = 0
skips = 0        # cases a family could not judge (trigrad, interp: a reference term that is not finite); run() counts them

def sphere_case():
    global fails
    H = int(rs.choice([8, 16, 33, 64, 96, 128, 130, 200, 256, 512, 1000])); W = int(rs.choice([8, 16, 36, 64, 100, 128, 132, 256, 258, 512, 1024]))
    N = int(rs.randint(1, 5)); J = int(rs.choice([1, 2, 7, 41, 64]))
    scale = rs.choice([20.0, 80.0, 160.0, 400.0])
    sp = np.concatenate([rs.uniform(-scale, scale, (N, J, 2)), rs.uniform(-120, 130, (N, J, 1)),
                         rs.uniform(0.02, 1.0, (N, J, 1)) * rs.choice([2.0, 12.0, 45.0, 300.0])], -1).astype(np.float32)
    if rs.rand() < 0.3: sp[:, :, 3] *= rs.choice([-1.0, 1.0], (N, J))          # negative radii (|r| matters)
    if rs.rand() < 0.2: sp[:, :, 2] = np.abs(sp[:, :, 2]) + 101                  # everything behind the background
    if rs.rand() < 0.1: sp[rs.randint(N), rs.randint(J), rs.randint(4)] = rs.choice([np.nan, np.inf, -np.inf, 1e30])   # the general path
    mode = rs.randint(0, 4)
    ops.set_tuning(ops.TUNE_FORCE_GENERAL, 1 if mode == 1 else 0)
    ops.set_tuning(ops.TUNE_FWD_LDS_BYTES, 16 * 1024 if mode == 2 else 0)
    ops.set_tuning(ops.TUNE_FWD_OWNER_LDS_BYTES, 24 * 1024 if mode == 2 else 0)
    ops.set_tuning(ops.TUNE_BWD_LDS_BYTES, 16 * 1024 if mode == 2 else 128 * 1024)
    ops.set_tuning(ops.TUNE_FWD_WAVES, 4 if mode == 3 else 16)
    zb = int(rs.choice([0, 0, 6, 20, 48, 80])) * 1024                           # forward z-buffer: several row bands per box
    ops.set_tuning(ops.TUNE_FWD_ZBUF_BYTES, zb)
    ops.set_tuning(ops.TUNE_BWD_WAVES, int(rs.choice([0, 8, 16])))
    ops.set_tuning(ops.TUNE_MSE_BOX, int(rs.choice([-1, 0, 1, 20 * 1024, 60 * 1024])))
    d, a = ops.sphere_raster_fwd(dev(sp), H, W, want_argmin=True)
    od, oa = oracle.sphere_raster_fwd(sp, H, W)
    if not np.isfinite(sp).all() or np.abs(sp).max() > 1e20:
        # non-finite records: depth only (NaN where the oracle has NaN, bit-exact elsewhere), as tests/test_nan_inf
        dn = d.cpu().numpy()
        ok = np.array_equal(np.isnan(dn), np.isnan(od)) and np.array_equal(bits(dn)[~np.isnan(od)], bits(od)[~np.isnan(od)])
        if not ok:
            fails += 1
            print("SPHERE (non-finite) MISMATCH", dict(N=N, J=J, H=H, W=W, mode=mode, zb=zb))
        return   # (gradients of non-finite records: tests/golden/g_edges_sphere.npz, tests/test_edges_gpu.py)
    ok = np.array_equal(bits(d.cpu().numpy()), bits(od)) and np.array_equal(a.cpu().numpy(), oa)
    why = [] if ok else ['fwd depth %d px, owner %d px' % (int((bits(d.cpu().numpy()) != bits(od)).sum()), int((a.cpu().numpy() != oa).sum()))]
    gd = rs.standard_normal((N, H, W)).astype(np.float32)
    og = oracle.sphere_raster_bwd(sp, gd)
    # the autograd pair's owner map: written on the touched rows only, over whatever the buffer held
    d2, a2 = ops.sphere_raster_fwd(dev(sp), H, W, want_argmin=True, flags=ops.RASTER_OWNER_TOUCHED_ROWS)
    fg_rows = (od < 100).any(2)
    if not (torch.equal(d2, d) and np.array_equal(a2.cpu().numpy()[fg_rows], oa[fg_rows])):
        ok = False
        why.append('touched-rows forward')
    for owner, label in ((a, 'owner map'), (a2, 'touched-rows owner map'), (None, 'recomputed')):
        gs = ops.sphere_raster_bwd(dev(sp), dev(gd), owner).cpu().numpy()
        okb = bool(np.abs(gs - og).max() <= 1e-5 * np.abs(og).max() + 2e-4)
        if not okb: why.append('bwd(%s) err %.3g of %.3g' % (label, np.abs(gs - og).max(), np.abs(og).max()))
        ok = ok and okb
    tgt = rs.uniform(-50, 100, (N, H, W)).astype(np.float32)
    if ops.sphere_raster_mse_supported(dev(sp), dev(tgt), H, W):
        dep, sse, gsp = ops.sphere_raster_mse(dev(sp), dev(tgt))
        e = (od.astype(np.float64) - tgt)
        ref_sse = (e * e).reshape(N, -1).sum(1)
        og2 = oracle.sphere_raster_bwd(sp, (2 * (od - tgt)).astype(np.float32))
        checks = {'fused depth': np.array_equal(bits(dep.cpu().numpy()), bits(od)),
                  'fused sse err %.3g of %.3g' % (np.abs(sse.double().cpu().numpy() - ref_sse).max(), ref_sse.max()):
                      bool(np.abs(sse.double().cpu().numpy() - ref_sse).max() <= 1e-5 * ref_sse.max() + 1e-3),
                  'fused grad err %.3g of %.3g' % (np.abs(gsp.cpu().numpy() - og2).max(), np.abs(og2).max()):
                      bool(np.abs(gsp.cpu().numpy() - og2).max() <= 2e-5 * np.abs(og2).max() + 1e-3)}
        why += [k for k, v in checks.items() if not v]
        ok = ok and all(checks.values())
    if not ok:
        fails += 1
        print("SPHERE MISMATCH", dict(N=N, J=J, H=H, W=W, scale=scale, mode=mode, zb=zb), why)
        if os.environ.get("FUZZ_DUMP"):
            np.savez(os.environ["FUZZ_DUMP"], sp=sp, gd=gd, tgt=tgt, H=H, W=W, mode=mode, zb=zb)

def tri_case():
    global fails
    W = int(rs.choice([5, 16, 33, 96, 200, 320])); H = int(rs.choice([7, 16, 40, 72, 160, 256]))
    B = int(rs.randint(1, 4)); F = int(rs.choice([1, 31, 33, 64, 200, 500]))
    c = rs.uniform(-0.2 * W, 1.2 * W, (B, F, 1, 1)) * np.array([1.0, H / W])
    spread = rs.choice([0.7, 3.0, 12.0, 60.0], (B, F, 1, 1))
    fv = np.concatenate([c + rs.normal(0, 1, (B, F, 3, 2)) * spread, rs.uniform(-50, 50, (B, F, 3, 1))], -1).astype(np.float32)
    if rs.rand() < 0.3: fv[:, :, :, 0] = np.round(fv[:, :, :, 0])               # vertices on pixel columns, equal x
    if rs.rand() < 0.2: fv[:, ::7, 1] = fv[:, ::7, 0]                            # degenerate faces
    d = depth_rasterization.forward(W, H, dev(fv)).cpu().numpy()
    if not np.array_equal(bits(d), bits(oracle.tri_raster_fwd(fv, W, H))):
        fails += 1
        print("TRI MISMATCH", dict(B=B, F=F, W=W, H=H), int((bits(d) != bits(oracle.tri_raster_fwd(fv, W, H))).sum()))

def d2m_case():
    global fails
    H = int(rs.choice([8, 16, 37, 64, 100, 128, 130, 256])); W = int(rs.choice([H, H, 53, 70, 128]))
    N = int(rs.randint(1, 4)); J = int(rs.choice([1, 5, 41, 64]))
    depth = np.where(rs.rand(N, H, W) < rs.uniform(0.02, 0.6), rs.uniform(-60, 60, (N, H, W)), 100.0).astype(np.float32)
    cen = rs.uniform(-120, 120, (N, J, 3)).astype(np.float32); rad = rs.uniform(1, 30, (J,)).astype(np.float32)
    if J >= 5 and rs.rand() < 0.3:      # duplicated spheres: exact ties, the first index must own the pixel
        cen[:, J - 1] = cen[:, 1]; rad[J - 1] = rad[1]
    # a point whose distance sits on the clamp at 50 (torch.clamp's kink): fp32 rounding decides whether it has a
    # gradient, in the reference as here -- not a comparable case
    xs = (np.arange(W) - W / 2) * 300.0 / W; ys = (np.arange(H) - H / 2) * 300.0 / H
    X, Y = np.meshgrid(xs, ys)
    for n in range(N):
        fg = depth[n] <= 99
        P = np.stack([X[fg], Y[fg], depth[n][fg]], -1).astype(np.float64)
        if len(P):
            D = np.abs(np.linalg.norm(P[:, None, :] - cen[n][None].astype(np.float64), axis=-1) - rad[None].astype(np.float64))
            m = D.min(1)
            if (np.abs(m - 50.0) < 2e-4).any() or (m < 2e-4).any():
                return   # (on the clamp, on a surface: pinned by tests/golden/g_edges_d2m.npz, term_exactly_50 / point_on_surface)
            # a point equidistant from two DIFFERENT spheres to within a few fp32 ulps: which of them owns it (and gets
            # its unit vector) is decided by the last bit of the root -- v_sqrt_f32 here, sqrtf in the oracle, whatever
            # the reference's platform computes -- while the loss is the same: not a comparable case either (the long
            # run of round 3 met one in 3590: gap 7e-6 on 45.7, two gradient rows off by one unit vector)
            if J > 1:
                part = np.partition(D, 1, axis=1)
                close = (part[:, 1] - part[:, 0]) < 6e-7 * np.maximum(part[:, 1], 1.0)
                if close.any():
                    order = np.argsort(D[close], axis=1)[:, :2]
                    same_record = np.all(cen[n][order[:, 0]] == cen[n][order[:, 1]], axis=1) & (rad[order[:, 0]] == rad[order[:, 1]])
                    if (~same_record).any():     # (duplicated spheres tie EXACTLY: the first index must win, that is checked)
                        return   # (exact ties are pinned by tests/golden/g_edges_d2m.npz, identical_spheres)
    loss, grad = ops.data_to_model(dev(depth), dev(cen), dev(rad), want_grad=True)
    # any launch shape gives the same bits (the sums are integers)
    ops.set_tuning(ops.TUNE_D2M_WAVES, int(rs.choice([4, 8, 16]))); ops.set_tuning(ops.TUNE_D2M_BAND_UNITS, int(rs.choice([1, 2, 3, 8])))
    loss2, grad2 = ops.data_to_model(dev(depth), dev(cen), dev(rad), want_grad=True)
    loss3 = ops.data_to_model(dev(depth), dev(cen), dev(rad))
    ops.set_tuning(ops.TUNE_D2M_WAVES, 0); ops.set_tuning(ops.TUNE_D2M_BAND_UNITS, 0)
    if H * W < 192 * 192:    # one workgroup per crop: integer sums, identical bits whatever the launch shape
        same = bool(torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(loss, loss3))
    else:                    # two partial results per crop, added in fp32: the split moves with the launch shape
        same = bool(torch.equal(loss2, loss3) and (loss - loss2).abs().max() <= 1e-6 * loss.abs().max()
                    and (grad - grad2).abs().max() <= 1e-6 * grad.abs().max() + 1e-6)
    ol = oracle.data_to_model_fwd(depth, cen, rad); og = oracle.data_to_model_bwd(depth, cen, rad) * depth.size   # oracle: gradient of the mean
    ok = same and bool(np.abs(loss.cpu().numpy() - ol).max() <= 1e-5 * np.abs(ol).max() + 1e-4)
    ok = ok and bool(np.abs(grad.cpu().numpy() - og).max() <= 1e-5 * np.abs(og).max() + 1e-4)
    if not ok:
        fails += 1
        print("D2M MISMATCH", dict(N=N, J=J, H=H, W=W, same_bits_across_launch_shapes=same), "loss diff", np.abs(loss.cpu().numpy() - ol).max(), "of", np.abs(ol).max(),
              "grad diff", np.abs(grad.cpu().numpy() - og).max(), "of", np.abs(og).max())
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        np.savez(os.path.join(ROOT, "gpurun_out", "fuzz_d2m_fail.npz"), depth=depth, cen=cen, rad=rad, loss=loss.cpu().numpy(), grad=grad.cpu().numpy(), ol=ol, og=og)

def mesh_case():
    """fused raster + clamp + bilinear resize against the explicit chain (which is checked against the oracle above)"""
    global fails
    src = int(rs.choice([640, 320, 257, 96])); S = int(rs.choice([s_ for s_ in (16, 32, 64, 96, 128, 200, 256, 400) if s_ <= src]))
    B = int(rs.randint(1, 3)); NV = int(rs.choice([12, 200, 1500])); F = int(rs.choice([1, 100, 700, 3382]))
    xy = rs.uniform(-0.15 * src, 1.15 * src, (B, NV, 2)); z = rs.uniform(-80, 140, (B, NV, 1))
    verts = np.concatenate([xy, z, np.ones((B, NV, 1))], -1).astype(np.float32)
    base = rs.randint(0, NV, (F, 1)); faces = ((base + rs.randint(0, max(2, NV // rs.choice([4, 40, 400])), (F, 3))) % NV).astype(np.int32)
    if rs.rand() < 0.5:   # spatially coherent small faces: vertices sorted along x so that neighbouring indices are neighbours
        verts = np.take_along_axis(verts, np.argsort(verts[:, :, 0] + verts[:, :, 1] * 0.01, 1)[:, :, None], 1)
    tile = ops.mesh_depth_fwd(dev(verts), dev(faces), S, src, 100.0)
    raw = ops.tri_raster_indexed_fwd(src, src, dev(verts), dev(faces))
    chain = torch.nn.functional.interpolate(torch.clamp(raw, max=100.0).unsqueeze(1), size=(S, S), mode="bilinear",
                                            align_corners=False).squeeze(1)
    fv = verts[:, faces.reshape(-1), :3].reshape(B, F, 3, 3)
    ok = np.array_equal(bits(raw.cpu().numpy()), bits(oracle.tri_raster_fwd(fv, src, src)))
    ok = ok and bool((tile - chain).abs().max().item() <= 1e-5 * max(1.0, chain.abs().max().item()))
    if not ok:
        fails += 1
        print("MESH MISMATCH", dict(B=B, NV=NV, F=F, src=src, S=S), (tile - chain).abs().max().item())
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        np.savez(os.path.join(ROOT, "gpurun_out", "fuzz_mesh_fail.npz"), verts=verts, faces=faces, S=S, src=src,
                 tile=tile.cpu().numpy(), chain=chain.cpu().numpy(), raw=raw.cpu().numpy())

def band_case():
    """sizes whose resize samples at least half of the source pixels: the triangle band kernel with clamp + resize as its
    stream-out (tri_raster.hip RESIZE) against the tile kernel -- same rasterized values, same bilinear formula: bit for bit;
    both against the explicit chain on the raw raster (1e-5)"""
    global fails
    src = int(rs.choice([640, 320, 200, 96])); S = int(rs.choice([s_ for s_ in (64, 80, 96, 128, 160, 200, 256, 300, 320, 400, 512, 639) if s_ < src and 8 * s_ * s_ >= src * src]))
    B = int(rs.choice([1, 2, 5, 70, 300])) if src <= 200 else int(rs.choice([1, 2, 5]))
    NV = int(rs.choice([12, 200, 1500])); F = int(rs.choice([1, 100, 700, 3382]))
    xy = rs.uniform(-0.15 * src, 1.15 * src, (B, NV, 2)); z = rs.uniform(-80, 140, (B, NV, 1))
    verts = np.concatenate([xy, z, np.ones((B, NV, 1))], -1).astype(np.float32)
    base = rs.randint(0, NV, (F, 1)); faces = ((base + rs.randint(0, max(2, NV // rs.choice([4, 40, 400])), (F, 3))) % NV).astype(np.int32)
    if rs.rand() < 0.5:
        verts = np.take_along_axis(verts, np.argsort(verts[:, :, 0] + verts[:, :, 1] * 0.01, 1)[:, :, None], 1)
    band_rows = int(rs.choice([-1, -1, 8, 20]))
    try:
        ops.set_tuning(ops.TUNE_TRI_BAND, band_rows)      # (band heights: several launch plans of the same problem)
        band = ops.mesh_depth_fwd(dev(verts), dev(faces), S, src, 100.0)
        ops.set_tuning(ops.TUNE_MESH_BAND, 0)
        tile = ops.mesh_depth_fwd(dev(verts), dev(faces), S, src, 100.0)
    finally:
        ops.set_tuning(ops.TUNE_MESH_BAND, 1); ops.set_tuning(ops.TUNE_TRI_BAND, -1)
    raw = ops.tri_raster_indexed_fwd(src, src, dev(verts), dev(faces))
    chain = torch.nn.functional.interpolate(torch.clamp(raw, max=100.0).unsqueeze(1), size=(S, S), mode="bilinear",
                                            align_corners=False).squeeze(1)
    ok = torch.equal(band, tile) and bool((band - chain).abs().max().item() <= 1e-5 * max(1.0, chain.abs().max().item()))
    if not ok:
        fails += 1
        print("BAND-RESIZE MISMATCH", dict(B=B, NV=NV, F=F, src=src, S=S, band_rows=band_rows), int((band != tile).sum()),
              (band - chain).abs().max().item())

_syn = {}
def synth_case():
    """HandSynthesizer: ONE launch == three launches bit for bit (draws included); noise off == the module chain on the same
    draws; noise on == DepthNoise on the numpy restatement of the kernels' generator (2e-5)"""
    global fails
    from spherehand_amd import hand_model, synth_rng
    from spherehand_amd.util_modules import HandSynthesizer
    S, hm = [(32, 8), (64, 16), (128, 32), (128, 16), (64, 4)][rs.randint(5)]
    noise, heat = bool(rs.randint(2)), bool(rs.randint(2))
    key = (S, hm)
    if key not in _syn:
        mesh = hand_model.load_mesh()
        _syn[key] = [HandSynthesizer(mesh, S, hm, 1.0, 0.01).cuda() for _ in range(2)]
    a, b = _syn[key]
    B = int(rs.choice([1, 2, 7, 40, 300]))
    p = (rs.uniform(-1, 1, (B, 26)) * rs.choice([0.3, 1.5, 3.2])).astype(np.float32)
    p[:, 3:6] = rs.uniform(-40, 40, (B, 3))
    pose = dev(p)
    seed, ctr = int(rs.randint(1, 2 ** 31)), int(rs.randint(0, 1000))
    for m, one in ((a, True), (b, False)):
        m.add_noise, m.out_heatmap, m.one_launch = noise, heat, one
        m.reseed(seed, device=pose.device, counter=ctr)
    oa, ob = a(pose), b(pose)
    oa, ob = (oa, ob) if heat else ((oa,), (ob,))
    why = []
    if not (torch.equal(a.last_draws.view(torch.int32), b.last_draws.view(torch.int32)) and all(torch.equal(x, y) for x, y in zip(oa, ob))):
        why.append("one launch != three launches: draws %s, outputs %s" % (torch.equal(a.last_draws.view(torch.int32), b.last_draws.view(torch.int32)),
                                                                          [int((x != y).sum()) for x, y in zip(oa, ob)]))
    f, keys = synth_rng.sample_draws(seed, ctr, B, 0.1)
    d = a.last_draws.cpu().numpy()
    if not (np.array_equal(bits(d[0:4]), bits(f)) and np.array_equal(d[4:6].view(np.uint32), keys)):
        why.append("draws != numpy restatement")
    dr = a.last_draws
    T = a.hand_skeleton_transform(pose) * torch.cat([dr[0:3].t(), torch.ones(B, 1, device="cuda")], 1).view(B, 1, 4, 1)
    with torch.no_grad():
        clean = a.dm_render(T, dr[3].clone()) * a.depth_scale
    if noise:
        expect = synth_rng.depth_noise(clean.cpu().numpy(), keys, 0.5, 0.05)
        err = np.abs(oa[0].cpu().numpy() - expect)
        if not err.max() <= 2e-5:      # (v_log_f32 near 1: see tests/test_synth_gpu.py)
            why.append("noise: max err %.3g at %s (%d px above 2e-5)" % (err.max(), np.unravel_index(err.argmax(), err.shape), int((err > 2e-5).sum())))
    elif not torch.equal(oa[0], clean):
        why.append("clean depth != module chain")
    if heat:
        with torch.no_grad():
            hm_ref = a.hm_render(T, dr[3].clone(), a.uv_hm_scale, a.depth_scale)
        if not all(torch.equal(x, y) for x, y in zip(oa[1:], hm_ref)):
            why.append("heat-maps != module")
    if why:
        fails += 1
        print("SYNTH MISMATCH", dict(S=S, hm=hm, B=B, noise=noise, heat=heat, seed=seed, ctr=ctr), why)

_fk = None
def fk_case():
    """forward kinematics forward / backward against the torch-op evaluation of the same chain"""
    global fails, _fk
    if _fk is None:
        from spherehand_amd import hand_model
        from spherehand_amd.kinematicsTransformation import HandTransformationMat
        _fk = HandTransformationMat([b["offset_matrix"].astype(np.float32) for b in hand_model.load_mesh()["bones"]]).cuda()
    B = int(rs.choice([1, 3, 64, 300]))
    p = (rs.uniform(-1, 1, (B, 26)) * rs.choice([0.1, 1.5, 3.2, 10.0])).astype(np.float32)
    p[:, 3:6] = rs.uniform(-60, 60, (B, 3))
    p1 = dev(p).requires_grad_(True); p2 = dev(p).requires_grad_(True)
    G = dev(rs.standard_normal((B, 17, 4, 4)).astype(np.float32))
    T1 = _fk(p1); T2 = _fk.forward_torch(p2)
    (T1 * G).sum().backward(); (T2 * G).sum().backward()
    ok = bool((T1 - T2).abs().max().item() <= 3e-4) and bool((p1.grad - p2.grad).abs().max().item() <= 2e-4 * max(1.0, p2.grad.abs().max().item()))
    if not ok:
        fails += 1
        print("FK MISMATCH", B, (T1 - T2).abs().max().item(), (p1.grad - p2.grad).abs().max().item(), p2.grad.abs().max().item())

def gn_case():
    """NHWC GroupNorm + ReLU forward / backward against torch in fp64"""
    global fails
    C = int(rs.choice([32, 64, 128, 256])); G = int(rs.choice([g for g in (4, 8, 16) if C % g == 0 and (C // g) % 4 == 0]))
    N = int(rs.randint(1, 9)); H = int(rs.choice([1, 3, 4, 8, 16, 33])); W = int(rs.choice([1, 4, 7, 16, 32]))
    # (offset in units of the spread: fp32 cannot resolve x - mean below ulp(mean) whatever the algorithm)
    x = (torch.from_numpy(rs.standard_normal((N, C, H, W)).astype(np.float32)) + float(rs.uniform(-3, 3))) * float(rs.choice([0.01, 1.0, 30.0]))
    x = x.cuda().to(memory_format=torch.channels_last).requires_grad_(True)
    gn = torch.nn.GroupNorm(G, C).cuda()
    with torch.no_grad():
        gn.weight.copy_(dev(rs.standard_normal(C).astype(np.float32))); gn.bias.copy_(dev(rs.standard_normal(C).astype(np.float32) * 0.5))
    if not ops.group_norm_relu_supported(x, G):
        return
    up = dev(rs.standard_normal((N, C, H, W)).astype(np.float32)).to(memory_format=torch.channels_last)
    y = ops.group_norm_relu(x, gn); (y * up).sum().backward()
    got = (y.detach(), x.grad.clone(), gn.weight.grad.clone(), gn.bias.grad.clone())
    xd = x.detach().double().requires_grad_(True)
    gd = torch.nn.GroupNorm(G, C).cuda().double(); gd.load_state_dict({k: v.double() for k, v in gn.state_dict().items()})
    z = gd(xd)
    if (z.abs().min() < 1e-5 * z.abs().max()).item():
        return   # an activation on the ReLU kink: fp32 and fp64 may disagree on its sign, the gradients then differ by a whole term
    yr = torch.relu(z); (yr * up.double()).sum().backward()
    ref = (yr.detach(), xd.grad, gd.weight.grad, gd.bias.grad)
    for a, b, tol in zip(got, ref, (4e-6, 4e-5, 4e-5, 4e-5)):
        if (a.double() - b).abs().max().item() > tol * max(1.0, b.abs().max().item()):
            fails += 1
            print("GN MISMATCH", dict(N=N, C=C, H=H, W=W, G=G), (a.double() - b).abs().max().item(), b.abs().max().item())
            break

_mv = {}
def mv_case():
    """MutualProjectionLoss: the fused path (render-and-compare kernel, indexed data-to-model) against the
    reference wiring on the separate kernels -- loss, projections, gradient w.r.t. the joints"""
    global fails
    from spherehand_amd.multiview_utility import MutualProjectionLoss
    from spherehand_amd.datasets import random_rotations
    S = int(rs.choice([32, 64, 128, 256])); J = 41
    if S not in _mv:
        from spherehand_amd import hand_model
        _mv[S] = MutualProjectionLoss(S, hand_model.load_mesh()).cuda()
    crit = _mv[S]
    B = int(rs.randint(1, 5)); V = 3
    gen = torch.Generator().manual_seed(int(rs.randint(1 << 30)))
    R = random_rotations(B * V, float(rs.choice([5.0, 30.0, 90.0])), generator=gen).reshape(B, V, 3, 3)
    cam = torch.eye(4).repeat(B, V, 1, 1); cam[:, :, :3, :3] = R; cam[:, :, :3, 3] = torch.from_numpy(rs.uniform(-10, 10, (B, V, 3)).astype(np.float32))
    inv = torch.linalg.inv(cam)
    joints = torch.from_numpy((rs.uniform(-70, 70, (B, V, J, 3)) * np.array([1, 1, 0.5])).astype(np.float32))
    dms = torch.from_numpy(np.where(rs.rand(B, V, S, S) < 0.2, rs.uniform(-60, 60, (B, V, S, S)), 100.0).astype(np.float32))
    is_mv = bool(rs.rand() < 0.5)
    out = {}
    for fused in (True, False):
        crit.fused = fused
        j = joints.cuda().requires_grad_(True)
        loss, proj = crit(cam.cuda(), inv.cuda(), j, dms.cuda(), is_mv)
        loss.backward()
        out[fused] = (loss.item(), proj.detach().cpu().numpy(), j.grad.cpu().numpy())
    ok = abs(out[True][0] - out[False][0]) <= 5e-6 * abs(out[False][0]) + 1e-6
    ok = ok and np.array_equal(bits(out[True][1]), bits(out[False][1]))
    ok = ok and bool(np.abs(out[True][2] - out[False][2]).max() <= 5e-5 * np.abs(out[False][2]).max() + 1e-7)
    if not ok:
        fails += 1
        print("MV MISMATCH", dict(B=B, S=S, is_mv=is_mv), out[True][0], out[False][0], np.abs(out[True][2] - out[False][2]).max(), np.abs(out[False][2]).max())

def sa_case():
    """soft-argmax (RecoverXYZCoordinateFromHeatmap) forward / backward against the torch ops in fp64"""
    global fails
    from spherehand_amd.util_modules import RecoverXYZCoordinateFromHeatmap
    S = int(rs.choice([8, 16, 32])); J = int(rs.choice([1, 2, 14, 41])); N = int(rs.randint(1, 12))
    hm = torch.from_numpy((rs.standard_normal((N, 2 * J, S, S)) * rs.choice([0.1, 0.6, 3.0])).astype(np.float32)).cuda()
    if rs.rand() < 0.5: hm = hm.to(memory_format=torch.channels_last)
    hm = hm.requires_grad_(True)
    if not ops.soft_argmax_supported(hm, J):
        return
    rec = RecoverXYZCoordinateFromHeatmap(S, S, 0.01).cuda()
    up = dev(rs.standard_normal((N, J, 3)).astype(np.float32))
    xyz = rec.from_output(hm); (xyz * up).sum().backward()
    hd = hm.detach().double().requires_grad_(True)
    ref = RecoverXYZCoordinateFromHeatmap(S, S, 0.01).cuda().double().forward(hd[:, :J], hd[:, J:])
    (ref * up.double()).sum().backward()
    # yardstick: the same torch formulation in fp32 (its own distance from fp64 on these inputs)
    h32 = hm.detach().clone().requires_grad_(True)
    t32 = rec.forward(h32[:, :J], h32[:, J:]); (t32 * up).sum().backward()
    ex_t = (t32.detach().double() - ref.detach()).abs().max().item(); eg_t = (h32.grad.double() - hd.grad).abs().max().item()
    ok = bool((xyz.detach().double() - ref.detach()).abs().max().item() <= 4e-5 * max(1.0, ref.abs().max().item()) + 4 * ex_t)
    ok = ok and bool((hm.grad.double() - hd.grad).abs().max().item() <= 4e-5 * max(1.0, hd.grad.abs().max().item()) + 4 * eg_t)
    if not ok:
        fails += 1
        print("SOFT-ARGMAX MISMATCH", dict(N=N, J=J, S=S), (xyz.detach().double() - ref.detach()).abs().max().item(),
              (hm.grad.double() - hd.grad).abs().max().item(), hd.grad.abs().max().item(), "torch fp32:", ex_t, eg_t)

_skin = None
_uskin = None
def lbs_case():
    """skinning + camera against the oracle, bit for bit (random bone matrices, with / without camera and rand_f)"""
    global fails, _skin
    if _skin is None:
        from spherehand_amd import hand_model
        _skin = hand_model.sparse_skin(hand_model.load_mesh())
    start, bone, wv = _skin
    B = int(rs.randint(1, 6))
    T = (rs.standard_normal((B, 17, 4, 4)) * rs.choice([0.5, 1.0, 30.0])).astype(np.float32)
    mode = int(rs.randint(0, 3))
    cam = None if mode == 0 else (float(rs.uniform(0, 640)), float(rs.uniform(0, 640)), float(rs.uniform(0.5, 4)), float(rs.uniform(0.5, 4)))
    rf = rs.uniform(0.8, 1.2, (B,)).astype(np.float32) if mode == 2 else None
    rh = bool(rs.rand() < 0.5)
    out = ops.lbs_project(dev(T), dev(start), dev(bone), dev(wv), rh, cam, None if rf is None else dev(rf)).cpu().numpy()
    o = oracle.lbs_project(T, start, bone, wv, rh, cam, rf)
    if not np.array_equal(bits(out), bits(o)):
        fails += 1
        print("LBS MISMATCH", dict(B=B, mode=mode, right_hand=rh), np.abs(out - o).max())
    if cam is not None and rs.rand() < 0.5:
        # DepthRender.forward as one launch (the lattice kernel skins its crop's vertices into LDS) against skinning followed
        # by the raster: the mesh's distinct vertices (1 721: they fit next to the lattice), random faces over them
        global _uskin
        if _uskin is None:
            from spherehand_amd import hand_model
            from spherehand_amd.render import unique_skin
            _uskin = unique_skin(hand_model.load_mesh())[:3]
        us, ub, uw = _uskin
        NV = len(us) - 1
        F = int(rs.choice([1, 50, 900, 3382]))
        base = rs.randint(0, NV, (F, 1))
        faces = ((base + rs.randint(0, max(2, NV // rs.choice([4, 40, 400])), (F, 3))) % NV).astype(np.int32)
        S = int(rs.choice([128, 64, 32, 80]))
        T2 = T.copy()
        T2[:, :, :3, 3] = rs.uniform(-60, 60, (B, 17, 3))          # (keep a part of the mesh on the screen)
        T2[:, :, :3, :3] = (rs.standard_normal((B, 17, 3, 3)) * 0.6).astype(np.float32)
        cam2 = (320.0 + float(rs.uniform(-40, 40)), 320.0 + float(rs.uniform(-40, 40)), float(rs.uniform(1.0, 3.0)), float(rs.uniform(1.0, 3.0)))
        rfd = None if rf is None else dev(rf)
        verts = ops.lbs_project(dev(T2), dev(us), dev(ub), dev(uw), rh, cam2, rfd)
        want = ops.mesh_depth_fwd(verts, dev(faces), S, 640, 100.0)
        got = ops.mesh_render_fwd(dev(T2), dev(us), dev(ub), dev(uw), rh, cam2, rfd, dev(faces), S, 640, 100.0)
        if not torch.equal(got, want):
            fails += 1
            print("MESH RENDER MISMATCH", dict(B=B, F=F, S=S, right_hand=rh), (got - want).abs().max().item())

_hm = {}
def hm_case():
    """heat-map painting + back-projection (no-grad kernels) against the torch ops of the same module"""
    global fails, _fk
    from spherehand_amd import hand_model
    from spherehand_amd.render import Hand3DHeatmapRender
    if _fk is None:
        fk_case()
    S = int(rs.choice([8, 16, 32]))
    if S not in _hm:
        _hm[S] = Hand3DHeatmapRender(hand_model.load_mesh()["bones"], S).cuda()
    B = int(rs.randint(1, 20))
    p = (rs.uniform(-1, 1, (B, 26)) * rs.choice([0.3, 1.5, 3.0])).astype(np.float32); p[:, 3:6] = rs.uniform(-40, 40, (B, 3))
    T = _fk(dev(p)).detach()
    rf = dev(rs.uniform(0.85, 1.15, (B,)).astype(np.float32)) if rs.rand() < 0.5 else None
    uv, ds = float(rs.choice([1.0, 0.5])), float(rs.choice([0.01, 1.0]))
    with torch.no_grad():
        a = _hm[S](T, rf, uv, ds)
    with torch.enable_grad():
        b = _hm[S](T, rf, uv, ds)
    # (the depth map is gated by uv_hm > 0.05: pixels whose Gaussian sits on the threshold may go either way)
    off_gate = (b[0] / uv - 0.05).abs() > 1e-5
    for k, (x, y, tol) in enumerate(zip(a, b, (6e-6, 1e-6, 4e-4))):   # (1 case in 38 k reached 4.4e-6 on the Gaussians: the exponent's rounding)
        if k == 1:
            x, y = x * off_gate, y * off_gate
        if x.shape != y.shape or (x - y).abs().max().item() > tol * max(1.0, y.abs().max().item()):
            fails += 1
            print("HEATMAP MISMATCH", dict(B=B, S=S, uv=uv, ds=ds, rand_f=rf is not None), (x - y).abs().max().item(), y.abs().max().item())
            break

_pl = None
def pl_case():
    """CollisionLoss + BoneLengthLoss in one launch against the torch modules (values and gradients)"""
    global fails, _pl
    from spherehand_amd.render import BoneLengthLoss, CollisionLoss
    if _pl is None:
        _pl = (CollisionLoss().cuda(), BoneLengthLoss().cuda())
    cc, bc = _pl
    B = int(rs.randint(1, 9)); V = int(rs.choice([1, 3]))
    xyz = (rs.standard_normal((B, V, 41, 3)) * rs.choice([2.0, 15.0, 60.0])).astype(np.float32)
    wa, wb = float(rs.uniform(0.1, 2)), float(rs.uniform(0.1, 2))
    a = dev(xyz).requires_grad_(True)
    ca, ba = cc(a), bc(a); (ca * wa + ba * wb).backward()
    b = dev(xyz).requires_grad_(True)
    col, bone = ops.PairLosses.apply(b.reshape(B, -1, 3), 41, 11, 6, float(cc.min_sq_dist), bc.joint_1.to(torch.int32),
                                     bc.joint_2.to(torch.int32), bc.min_length.reshape(-1).clone(), bc.max_length.reshape(-1).clone())
    (col * wa + bone * wb).backward()
    ok = abs(col.item() - ca.item()) <= 2e-5 * max(1.0, abs(ca.item())) and abs(bone.item() - ba.item()) <= 2e-5 * max(1.0, abs(ba.item()))
    gd = (b.grad - a.grad).abs().reshape(-1, 3).max(1).values
    tolg = 2e-5 * max(1.0, a.grad.abs().max().item())
    # one pair sitting on its hinge's kink (distance == threshold up to rounding) switches its two points' terms
    # on or off with no change of the loss: not a comparable case
    on_kink = int((gd > tolg).sum().item()) <= 2
    ok = ok and (bool(gd.max().item() <= tolg) or on_kink)
    if not ok:
        fails += 1
        print("PAIR-LOSS MISMATCH", dict(B=B, V=V), col.item(), ca.item(), bone.item(), ba.item(), (b.grad - a.grad).abs().max().item(), a.grad.abs().max().item())

def ks_case():
    """key-point skinning -> sphere records (keypoint_skin.hip) against the torch ops of the same module, both directions"""
    global fails, _fk
    from spherehand_amd import hand_model
    from spherehand_amd.render import HandBallPrimitiveRender
    if _fk is None:
        fk_case()
    if "hbr" not in _hm:
        _hm["hbr"] = HandBallPrimitiveRender(hand_model.load_mesh()["bones"], 64, 64).cuda()
    hbr = _hm["hbr"]
    B = int(rs.randint(1, 70))
    p = (rs.uniform(-1, 1, (B, 26)) * rs.choice([0.3, 1.5, 3.0])).astype(np.float32); p[:, 3:6] = rs.uniform(-60, 60, (B, 3))
    T1 = _fk(dev(p)).detach().requires_grad_(True)
    T2 = T1.detach().clone().requires_grad_(True)
    sph = hbr.spheres(T1)
    pts = hbr.lbs(T2)
    ref = torch.cat([pts[:, :, 0:3], hbr.radiuses.expand(B, -1).unsqueeze(-1)], dim=2)
    G = dev(rs.standard_normal((B, 41, 4)).astype(np.float32))
    (sph * G).sum().backward(); (ref * G).sum().backward()
    ok = (sph - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item()) + 2e-5 and \
        (T1.grad - T2.grad).abs().max().item() <= 2e-6 * max(1.0, T2.grad.abs().max().item())
    # the one-launch chain pose -> records (fk.hip, shr_pose_spheres_*) = the two modules chained, bit for bit
    q1 = dev(p).requires_grad_(True); q2 = dev(p).requires_grad_(True)
    one = hbr.pose_spheres(_fk, q1); two = hbr.spheres(_fk(q2))
    (one * G).sum().backward(); (two * G).sum().backward()
    ok = ok and torch.equal(one, two) and torch.equal(q1.grad, q2.grad)
    if not ok:
        fails += 1
        print("KEYPOINT-SPHERES MISMATCH", dict(B=B), (sph - ref).abs().max().item(), (T1.grad - T2.grad).abs().max().item(),
              torch.equal(one, two), torch.equal(q1.grad, q2.grad))

def _grad_helpers():
    """tests/fixed_point_ref.py (the per-tap terms of the fp64 restatements and the error bound fixed_point.h's design
    allows on every accumulator) and tests/tri_interp_ref.py"""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import fixed_point_ref, tri_interp_ref
    return fixed_point_ref, tri_interp_ref

def grad_case_draw(interp):
    """One case of the trigrad / interp families, numpy only (tests/test_fixed_point_cpu.py draws it without a GPU): an
    indexed mesh whose faces are tri_case's -- vertices on integer columns, degenerate faces, both windings -- at depths
    20 .. 60, some faces welded to their predecessor's last corner, padded with unreferenced vertices to an NV on either
    side of fixed_point.h's 2048 points; an upstream gradient +- 2^U(-20, 20) times one 2^k per crop."""
    W = int(rs.choice([1, 5, 33, 64, 97])); H = int(rs.choice([1, 7, 40, 61]))
    B = int(rs.randint(1, 4)); F = int(rs.choice([1, 31, 200, 683]))
    c = rs.uniform(-0.2 * W, 1.2 * W, (B, F, 1, 1)) * np.array([1.0, H / W])
    spread = rs.choice([0.7, 3.0, 12.0, 60.0], (B, F, 1, 1))
    fv = np.concatenate([c + rs.normal(0, 1, (B, F, 3, 2)) * spread, rs.uniform(20, 60, (B, F, 3, 1))], -1).astype(np.float32)
    if rs.rand() < 0.3: fv[:, :, :, 0] = np.round(fv[:, :, :, 0])
    if rs.rand() < 0.2: fv[:, ::7, 1] = fv[:, ::7, 0]
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    weld = np.nonzero(rs.rand(F) < 0.3)[0]
    weld = weld[weld > 0]
    faces[weld, 0] = faces[weld - 1, 2]
    NV = int(rs.choice([n for n in (2040, 2047, 2048, 2049, 2300) if n >= 3 * F]))
    pad = np.concatenate([rs.uniform(0, 60, (B, NV - 3 * F, 3)), np.ones((B, NV - 3 * F, 1))], -1)
    verts = np.concatenate([np.concatenate([fv.reshape(B, 3 * F, 3), np.ones((B, 3 * F, 1))], -1), pad], 1).astype(np.float32)
    case = dict(W=W, H=H, B=B, F=F, NV=NV, verts=np.ascontiguousarray(verts), faces=faces, band=int(rs.choice([-1, 0, 8])))
    crop_scale = np.exp2(rs.randint(-30, 31, (B, 1, 1, 1)).astype(np.float64))
    C = int(rs.choice([1, 3, 4, 17, 64])) if interp else 1
    g = rs.choice([-1.0, 1.0], (B, C, H, W)) * np.exp2(rs.uniform(-20, 20, (B, C, H, W))) * crop_scale
    case["grad"] = np.ascontiguousarray(g if interp else g[:, 0], np.float32)
    if interp:
        case["shared"] = bool(rs.rand() < 0.5)
        case["attr"] = rs.standard_normal((NV, C) if case["shared"] else (B, NV, C)).astype(np.float32)
    return case

def grad_case_terms(case, owner):
    """{entry: fixed_point_ref.Terms} of a drawn case for the owner map [B,H,W] of its indexed mesh"""
    fx, _ = _grad_helpers()
    if "attr" in case:
        tv, ta, _ = fx.interp_terms(case["attr"], owner, case["verts"], case["faces"], case["grad"])
        return {"vertices": tv, "attributes": ta}
    B, F = case["B"], case["F"]
    soup = case["verts"][:, case["faces"].astype(np.int64), :3].reshape(B, 3 * F, 3)
    return {"indexed": fx.raster_terms(case["verts"], case["faces"], owner, case["grad"])[0],
            "soup": fx.raster_terms(soup, np.arange(3 * F).reshape(F, 3), owner, case["grad"])[0]}

def _grad_case(interp):
    global fails, skips
    fx, iref = _grad_helpers()
    case = grad_case_draw(interp)
    W, H, B, F, NV = (case[k] for k in ("W", "H", "B", "F", "NV"))
    x, fc, g = dev(case["verts"]), dev(case["faces"]), dev(case["grad"])
    fv = np.ascontiguousarray(case["verts"][:, case["faces"].astype(np.int64), :3])
    try:
        ops.set_tuning(ops.TUNE_TRI_BAND, case["band"])
        want = depth_rasterization.forward(W, H, dev(fv))
        ds, os_ = ops.tri_raster_owner_fwd(W, H, dev(fv))
        di, oi = ops.tri_raster_indexed_owner_fwd(W, H, x, fc)
    finally:
        ops.set_tuning(ops.TUNE_TRI_BAND, -1)
    why = []
    if not (np.array_equal(bits(ds.cpu().numpy()), bits(want.cpu().numpy())) and torch.equal(di, ds) and torch.equal(oi, os_)):
        why.append("owner forward: depth or owners differ from depth_rasterization.forward / between soup and indexed")
    owner = oi.cpu().numpy()
    terms = grad_case_terms(case, owner)
    if not all(t.all_finite() for t in terms.values()):
        skips += 1
        return
    nbits = fx.term_bits(3, W, H)
    if interp:
        a = dev(case["attr"])
        if not np.array_equal(bits(ops.tri_interpolate(a, oi, x, fc).cpu().numpy()), bits(iref.interp32(case["attr"], owner, case["verts"], case["faces"]))):
            why.append("interpolation forward bits")
        ga, gv = ops.tri_interpolate_bwd(a, oi, x, fc, g)
        got = {"vertices": gv.cpu().numpy()[..., :2], "attributes": ga.cpu().numpy()}
    else:
        got = {"indexed": ops.tri_raster_indexed_bwd(x, fc, oi, g).cpu().numpy()[..., :3], "soup": ops.tri_raster_bwd(dev(fv), os_, g).cpu().numpy()}
    for name, t in terms.items():
        worst, at = fx.worst_ratio(got[name], t, nbits)
        if not worst <= 1.0:
            why.append("%s: err / bound %.3g at %s" % (name, worst, at))
    if why:
        fails += 1
        print("INTERP MISMATCH" if interp else "TRIGRAD MISMATCH", {k: v for k, v in case.items() if np.isscalar(v) or isinstance(v, bool)}, why)
        if os.environ.get("FUZZ_DUMP"):      # (as the sphere family: the failing case, where the caller asks for it)
            np.savez(os.environ["FUZZ_DUMP"], **case)

def trigrad_case():
    """the owner raster forward (soup and indexed, any band plan) against depth_rasterization.forward bit for bit; both
    backwards against the per-accumulator bound of tests/fixed_point_ref.py"""
    _grad_case(False)

def interp_case():
    """the attribute interpolation: forward bits against tri_interp_ref.interp32, both gradients against the bound"""
    _grad_case(True)


FAMILIES = (("sphere", sphere_case), ("tri", tri_case), ("d2m", d2m_case), ("mesh", mesh_case), ("fk", fk_case), ("gn", gn_case),
            ("mv", mv_case), ("sa", sa_case), ("pl", pl_case), ("lbs", lbs_case), ("hm", hm_case), ("ks", ks_case),
            ("band", band_case), ("synth", synth_case), ("trigrad", trigrad_case), ("interp", interp_case))


def reset_tuning():
    """the sphere and triangle families vary the launch shapes through shr_set_tuning: back to the launcher's choices"""
    for key, val in ((ops.TUNE_FORCE_GENERAL, 0), (ops.TUNE_FWD_LDS_BYTES, 0), (ops.TUNE_FWD_OWNER_LDS_BYTES, 0),
                     (ops.TUNE_BWD_LDS_BYTES, 128 * 1024), (ops.TUNE_FWD_WAVES, 16), (ops.TUNE_FWD_ZBUF_BYTES, 0),
                     (ops.TUNE_BWD_WAVES, 0), (ops.TUNE_MSE_BOX, -1), (ops.TUNE_TRI_BAND, -1)):
        ops.set_tuning(key, val)


skipped = {}

def run(families=None, cases=None, seconds=None, seed=0, log=print):
    """Each family until `cases` cases (an int, or {family: int, "*": default}) or `seconds` seconds (whichever comes
    first; None = unbounded by that measure).
    Returns {family: (cases run, mismatches)}; `skipped` (module level) then holds {family: cases the family could not
    judge} for the same run, and every log line names the count."""
    global rs, fails, skips
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)      # (the module paths under test draw from torch's generators: same draws per seed)
    out = {}
    skipped.clear()
    try:
        for name, fn in FAMILIES:
            if families and name not in families:
                continue
            before, skips0, t0, n = fails, skips, time.time(), 0
            ncase = cases.get(name, cases.get("*")) if isinstance(cases, dict) else cases
            while (ncase is None or n < ncase) and (seconds is None or time.time() - t0 < seconds):
                fn(); n += 1
            out[name] = (n, fails - before)
            skipped[name] = skips - skips0
            log("%s: %d cases in %.1f s, %d mismatches, %d skipped" % (name, n, time.time() - t0, fails - before, skips - skips0))
    finally:
        reset_tuning()
    return out


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 20.0
    res = run(sys.argv[3].split(",") if len(sys.argv) > 3 else None, None, budget, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    print("TOTAL: %d cases over %d families, %d mismatches (seed %s, %.0f s per family)"
          % (sum(n for n, _ in res.values()), len(res), sum(m for _, m in res.values()), sys.argv[2] if len(sys.argv) > 2 else "0", budget))
    sys.exit(1 if fails else 0)
