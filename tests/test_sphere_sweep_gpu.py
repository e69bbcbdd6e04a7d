"""The sphere fit's terms swept over sphere counts and tile edges on the GPU.  The three scan entries
(ops.sphere_icp_normal, sphere_icp_radii_normal, sphere_render_normal) at J in {1, 2, 7, 16, 17, 21, 22, 32, 33, 42, 43, 63, 64}
on images from 1 x 1 to 128 x 72 (one pixel, W = 1, H = 1, less than a wave, exactly one round, 255 / 1023 / 1025 pixels, up to
nine tiles and fifteen records), GIVEN their own fp32 centres and Jacobian: the maps bit for bit against the numpy rules, the
counts exactly, and every moment and every entry of A, g, C and gs within (n + 16) 2^-52 sum |terms| of the dense fp64 sum
(tests/sphere_sweep_ref.py; tests/test_sphere_sweep_cpu.py shows that the comparator can fail).  The Jacobian entry and the
per-frame terms (prior, collision, temporal, acceleration) at J in {1, 22, 64} against the existing numpy chains at those
units' own equalities; every entry's refusal of J = 0 and J = 65."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_prior_ref as pref
import sphere_render_icp_ref as rref
import sphere_sequence_ref as qref
import sphere_sweep_ref as sw
import sphere_trajectory_ref as tref
import test_sphere_collision_gpu as cgpu
import test_sphere_prior_cpu as pcpu
import test_sphere_sequence_gpu as qgpu
import test_sphere_sweep_cpu as cpu
import test_sphere_trajectory_gpu as tgpu
from test_sphere_icp_gpu import on_device, tables, within
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu
SHR_EINVAL, SHR_ETOOLARGE = -1, -2
_DEV = {}


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def device_case(mesh, spec):
    """A row of sphere_sweep_ref.CASES with its tables on the device, and the entries' own inputs: c32 [B,V,J,3], jac32
    [B,3J,26], view32 [B,V,4,4] numpy fp32 of ops.pose_keypoints_jacobian and ops.view_vertices.  Once per process."""
    from spherehand_amd import ops
    if spec not in _DEV:
        case = on_device(sw.cached_case(mesh, spec))
        d = case["dev"]
        kp, jac = ops.pose_keypoints_jacobian(d["params0"], *tables(case)[:4], True)
        case["own"] = (ops.view_vertices(kp, d["view"]).cpu().numpy()[..., :3], jac.cpu().numpy(), d["view"].cpu().numpy())
        _DEV[spec] = case
    return _DEV[spec]


def npy(t):
    return t.cpu().numpy()


def held_to_the_bars(case, what, got, rows, J, N=1):
    """The entry's outputs against the dense fp64 sums on `rows`, printed per quantity and asserted; then, printed only,
    whether they are the bits of the sums partitioned the way the kernels partition them."""
    jac32 = case["own"][1][:rows["shape"][0]]
    r = sw.ratios(got, sw.dense(rows, jac32, J, N))
    part = sw.partitioned(rows, jac32, J, N)
    same = {k: bool(np.array_equal(np.asarray(got[k], np.float64).view(np.int64), np.ascontiguousarray(v).view(np.int64)))
            for k, v in part.items()}
    print("%s %s: error / bar %s; bit-equal to the partitioned restatement: %s"
          % (case["name"], what, {k: "%.3g" % x for k, x in r.items()}, same))
    assert sw.flagged(r) == [], (case["name"], what, r)
    assert int(min(got["count"])) >= 1
    return r


@pytest.mark.parametrize("spec", sw.CASES, ids=sw.case_id)
def test_data_term(mesh, spec):
    """shr_sphere_icp_normal on every case of the sweep: dist and owner bit-equal to the numpy rule on the entry's own
    centres, the counts exact, A bit-symmetric, the spare moment 0, every moment and every entry of A and g within its
    derived bar of the dense fp64 sum, the cost within 1e-15 of the exactly rounded sum; two runs give the same bits."""
    from spherehand_amd import ops
    case = device_case(mesh, spec)
    d, m = case["dev"], case["model"]
    c32, jac32, view32 = case["own"]
    run = lambda: ops.sphere_icp_normal(d["observed"], d["view"], d["params0"], *tables(case), True, case["p2m"], ref.FG_MAX,   # noqa: E731
                                        ref.MAX_DIST, want_maps=True)
    A, g, cost, count, moments, dist, owner = out = run()
    rows = sw.icp_rows(case["observed"], c32, m.radii, case["B"], view32, case["p2m"], 12)
    assert np.array_equal(npy(owner), rows["owner"])
    assert np.array_equal(npy(dist).view(np.uint32), rows["dist"].view(np.uint32))
    assert torch.equal(A, A.transpose(1, 2)) and not bool(moments[..., 11].any())
    mom = npy(moments)
    held_to_the_bars(case, "data term", dict(moments=mom, rows=mom[..., 10], count=npy(count), A=npy(A), g=npy(g), cost=npy(cost)),
                     rows, m.J)
    assert npy(owner)[0, 0, -1, -1] >= 0 and all(mom[:, s, 10].sum() > 0 for s in sw.special_spheres(m.J))
    for a, b in zip(out, run()):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("spec", [s for s in sw.CASES if s[4]], ids=sw.case_id)
def test_radius_term(mesh, spec):
    """shr_sphere_icp_radii_normal on the starred cases.  G = 1, N = 1 (the first frame): A, g, cost, count, dist, owner and
    moments[..., :12] are shr_sphere_icp_normal's bits.  G = 2, N = 1 (one table per frame, the second's radii x 0.9): the maps
    bit for bit, the counts and R exact, the sixteen moments, A, g, C and gs within their derived bars."""
    from spherehand_amd import ops
    case = device_case(mesh, spec)
    d, m = case["dev"], case["model"]
    c32, jac32, view32 = case["own"]
    J = m.J
    run = lambda rows_, radii: ops.sphere_icp_radii_normal(d["observed"][rows_].contiguous(), d["view"][rows_].contiguous(),    # noqa: E731
                                                           d["params0"][rows_].contiguous(), *tables(case)[:4], radii, 1, True,
                                                           case["p2m"], ref.FG_MAX, ref.MAX_DIST, want_maps=True)
    one = run(slice(0, 1), d["radii"][None].contiguous())
    plain = ops.sphere_icp_normal(d["observed"][:1].contiguous(), d["view"][:1].contiguous(), d["params0"][:1].contiguous(),
                                  *tables(case), True, case["p2m"], ref.FG_MAX, ref.MAX_DIST, want_maps=True)
    for i, j in ((0, 0), (1, 1), (2, 2), (3, 3), (8, 5), (9, 6)):
        assert torch.equal(bits(one[i]), bits(plain[j])), (i, j)
    assert torch.equal(bits(one[7][..., :12]), bits(plain[4])) and one[7].shape == (1, J, 16) and one[5].shape == (1, J, J)
    radii = sw.second_radii(m.radii, case["B"])
    for what, rows_, rad in (("radius term, G = 1", slice(0, 1), radii[:1]), ("radius term, G = 2", slice(None), radii)):
        A, g, cost, count, C, R, gs, moments, dist, owner = run(rows_, torch.from_numpy(rad).cuda())
        rows = sw.icp_rows(case["observed"][rows_], c32[rows_], rad, 1, view32[rows_], case["p2m"], 16)
        assert np.array_equal(npy(owner), rows["owner"])
        assert np.array_equal(npy(dist).view(np.uint32), rows["dist"].view(np.uint32))
        assert torch.equal(A, A.transpose(1, 2)) and not bool(moments[..., 11].any())
        mom = npy(moments)
        held_to_the_bars(case, what, dict(moments=mom, rows=mom[..., 10], count=npy(count), A=npy(A), g=npy(g), cost=npy(cost),
                                          C=npy(C), R=npy(R), gs=npy(gs)), rows, J)


@pytest.mark.parametrize("spec", [s for s in sw.CASES if s[4]], ids=sw.case_id)
def test_render_term(mesh, spec):
    """shr_sphere_render_normal (weight 1, max_resid 10 mm) on the starred cases: depth and owner bit-equal to the numpy
    render rule on the entry's own centres, the counts exact, A bit-symmetric, every moment and every entry of A and g
    within its derived bar, the cost within 1e-15 of the exactly rounded sum of the clipped squares."""
    from spherehand_amd import ops
    case = device_case(mesh, spec)
    d, m = case["dev"], case["model"]
    c32, jac32, view32 = case["own"]
    A, g, cost, count, moments, depth, owner = ops.sphere_render_normal(d["observed"], d["view"], d["params0"], *tables(case), True,
                                                                        case["p2m"], ref.FG_MAX, sw.MAX_RESID, rref.BACKGROUND, 1.0,
                                                                        None, want_maps=True)
    rows = sw.render_rows(case["observed"], c32, m.radii, view32, case["p2m"])
    assert np.array_equal(npy(owner), rows["owner"])
    assert np.array_equal(npy(depth).view(np.uint32), rows["depth"].view(np.uint32))
    assert torch.equal(A, A.transpose(1, 2)) and not bool(moments[..., 11].any())
    mom = npy(moments)
    held_to_the_bars(case, "render term", dict(moments=mom, rows=mom[..., 10], count=npy(count), A=npy(A), g=npy(g), cost=npy(cost)),
                     rows, m.J)


# ---- the Jacobian and the per-frame terms at the ends of J --------------------------------------------------------------
def frame_case(mesh, J):
    """sphere_sweep_ref.frame_case on the device with the entry's own keypoints [B,J,4] and Jacobian [B,3J,26] (numpy fp32)."""
    from spherehand_amd import ops
    key = ("frames", J)
    if key not in _DEV:
        case = on_device(sw.frame_case(mesh, J))
        kp, jac = ops.pose_keypoints_jacobian(case["dev"]["params0"], *tables(case)[:4], True)
        case["kp"], case["jac"] = kp.cpu().numpy(), jac.cpu().numpy()
        _DEV[key] = case
    return _DEV[key]


@pytest.mark.parametrize("J", sw.FRAME_J)
def test_jacobian(mesh, J):
    """shr_pose_keypoints_jacobian on a random table of J spheres against pose_ik_ref.Chain.jacobian in fp64, within 4 x the
    deviation of the fp32 CPU chain on the same table (tests/test_sphere_sweep_cpu.py); the keypoints' 4th float is 1; at
    J = 64 point 63's rows and column 25 are not zero."""
    case = frame_case(mesh, J)
    kp64, want = case["model"].chain.jacobian(case["params0"])
    jac, kp = torch.from_numpy(case["jac"]).double(), torch.from_numpy(case["kp"])
    err = (jac - want).abs().max().item()
    print("J = %d: |jac - fp64 autograd| %.3g (bar %.3g, entries up to %.4g)" % (J, err, cpu.JACOBIAN_BAR[J], want.abs().max().item()))
    assert jac.shape == (4, 3 * J, 26) and err <= cpu.JACOBIAN_BAR[J]
    assert bool((kp[..., 3] == 1).all()) and (kp[..., :3].double() - kp64).abs().max().item() < 1e-3
    if J == 64:
        assert bool((jac[:, 3 * 63:].abs().amax(2) > 0).all()) and bool((jac[:, :, 25].abs().amax(1) > 0).all())


def with_a_far_sphere(case, frame=2):
    """The entry's own keypoints with sphere J - 1 of one frame moved by 100 mm: over any cap of a few centimetres."""
    c = case["kp"].copy()
    c[frame, -1, 0] += np.float32(100.0)
    return c


@pytest.mark.parametrize("J", sw.FRAME_J)
def test_temporal_and_acceleration_terms(mesh, J):
    """shr_sphere_temporal_normal and shr_sphere_accel_normal through the C ABI at T = 4 (previous, middle and next triples all
    exist) on the entry's own keypoints and Jacobian, one sphere forced over ts_max / acc_max: the first against the numpy
    chain at its unit's equality (count exact, cost bit for bit, A, g, E to 1e-13), the second bit for bit."""
    case = frame_case(mesh, J)
    c, jac = with_a_far_sphere(case), case["jac"]
    T, w, cap = 4, 0.5, 30.0
    d = qref.decide(c, T, cap)
    assert int((d["valid"] & ~d["act"]).sum()) >= 1 and (J == 1 or int(d["act"].sum()) >= 1)
    count = qgpu.against_chain(qgpu.raw(c, jac, T, w, cap), c, jac, T, w, cap, None)
    print("J = %d: temporal rows %s" % (J, count.tolist()))
    d = tref.decide(c, T, cap)
    assert int((d["valid"] & ~d["act"]).sum()) >= 1 and (J == 1 or int(d["act"].sum()) >= 1)
    out = tgpu.raw(c, jac, T, w, cap)
    tgpu.equals_chain(out, tref.chain(c, jac, T, w, cap))
    assert torch.equal(out[0], out[0].transpose(1, 2))
    plain = tgpu.raw(case["kp"], jac, T, w, float("inf"))           # without the far sphere and without a cap: all rows
    tgpu.equals_chain(plain, tref.chain(case["kp"], jac, T, w, float("inf")))
    assert plain[5].tolist() == [0, 0, J, J]


def raw_prior(centres, view, jac, params, k, conf, kw, km, lower, upper, lw):
    """The C entry on view-frame centres [B,V,J,4], view [B,V,4,4], jac [B,3J,26], params [B,26], keypoints [B,V,J,3] and
    confidence [B,V,J] (numpy fp32): (A, g, cost, count [B,2], moments [B,J,12]) on the device."""
    from spherehand_amd import _lib
    dev = [torch.from_numpy(np.ascontiguousarray(t, np.float32)).cuda() for t in (centres, view, jac, params, k, conf, lower, upper)]
    B, V, J = dev[0].shape[:3]
    A, g, cost, moments = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
                           for s in ((B, 26, 26), (B, 26), (B,), (B, J, 12)))
    count = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().shr_sphere_prior_normal(*(t.data_ptr() for t in dev[:6]), float(kw), float(km), dev[6].data_ptr(), dev[7].data_ptr(),
                                            float(lw), B, V, J, 0, A.data_ptr(), g.data_ptr(), cost.data_ptr(), count.data_ptr(),
                                            moments.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return A, g, cost, count, moments


@pytest.mark.parametrize("J", sw.FRAME_J)
def test_prior_term(mesh, J):
    """shr_sphere_prior_normal through the C ABI on the entry's own centres and Jacobian, keypoints 3 mm off the centres with
    one pair forced over kp_max: the counts exact, the cost bit-equal to the fp64 chain in the header's order, A
    bit-symmetric, A and g within that unit's bars of the row-wise fp64 sums on the same Jacobian."""
    case = frame_case(mesh, J)
    rng = np.random.default_rng(J)
    c = case["kp"][:, None].copy()                                  # the identity view: the view-frame centres are the keypoints
    view = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1, 1))
    k = (c[..., :3] + rng.normal(0.0, 3.0, c[..., :3].shape)).astype(np.float32)
    k[1, 0, J - 1, 0] += np.float32(60.0)
    conf = rng.uniform(0.5, 1.0, k.shape[:3]).astype(np.float32)
    lo, hi = pref.limits()
    p = case["params0"].float().numpy()
    kw, km, lw = 0.5, 20.0, 100.0
    A, g, cost, count, moments = raw_prior(c, view, case["jac"], p, k, conf, kw, km, lo, hi, lw)
    b, v, j, e, w, rowed, _ = pref.pairs(c[..., :3], k, conf, km)
    want_rows = np.zeros((4, J))
    np.add.at(want_rows, (b[rowed], j[rowed]), 1.0)
    h = pref.hinge(p, lo, hi)
    print("J = %d: pairs with rows %s, limit rows %s" % (J, want_rows.sum(1).tolist(), (h != 0).sum(1).tolist()))
    assert not bool(rowed.all()) and (J == 1 or want_rows.sum(1).min() >= 1)
    assert np.array_equal(npy(count), np.stack([want_rows.sum(1), (h != 0).sum(1)], 1).astype(np.int32))
    assert np.array_equal(npy(moments)[..., 10], want_rows) and not bool(moments[..., 11].any())
    assert torch.equal(A, A.transpose(1, 2))
    chain = pref.cost_chain(c[..., :3], k, conf, kw, km, p, lo, hi, lw)
    assert np.array_equal(npy(cost).view(np.int64), chain.view(np.int64)), (cost.tolist(), chain.tolist())
    A_rows, g_rows = pref.given(case["jac"], view, c[..., :3], p, k, conf, kw, km, lo, hi, lw)
    within(A, A_rows, pcpu.A_BAR, "A")
    within(g, g_rows, pcpu.G_BAR, "g")


def test_collision_term_with_every_pair(mesh):
    """shr_sphere_collision_normal through the C ABI with the all-pairs table: 2016 pairs at J = 64 (kScnMaxK is 4096) and 231
    at J = 22, against the numpy chain at that unit's equality (count exact, penetration and cost bit for bit, A and g to
    1e-13); K = 0 at J = 1: exact zeros."""
    for J in (64, 22):
        case = frame_case(mesh, J)
        tab = sw.all_pairs(case["model"].radii)
        assert len(tab[0]) == J * (J - 1) // 2
        count = cgpu.against_chain(cgpu.raw(case["kp"], case["jac"], tab, 0.5), case["kp"], case["jac"], tab, 0.5)
        print("J = %d: %d pairs, with rows %s" % (J, len(tab[0]), count.tolist()))
        assert int(count.min()) >= 3 * J and int(count.max()) < len(tab[0])      # several groups of 64 rows, and pairs without
    case = frame_case(mesh, 1)
    A, g, cost, count, pen = cgpu.raw(case["kp"], case["jac"], None, 0.5)
    assert not any(bool(bits(t).any()) for t in (A, g, cost)) and not bool(count.any())


# ---- rejections ---------------------------------------------------------------------------------------------------------
def test_every_entry_refuses_J_0_and_J_65():
    """J = 0 is SHR_EINVAL and J = 65 SHR_ETOOLARGE for every entry of the sweep, before any launch: the output buffers,
    filled with a sentinel, are untouched."""
    from spherehand_amd import _lib
    lib = _lib.lib()
    B, V, W, H, J = 2, 1, 4, 4, 65
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")                  # noqa: E731
    outs = []

    def out(shape, dtype=torch.float64):
        t = torch.full(shape, -12345, dtype=dtype, device="cuda")
        outs.append(t)
        return t.data_ptr()

    obs, centres, radii, view, jac, params = f32(B, V, H, W), f32(B, V, J, 4), f32(B, J), f32(B, V, 4, 4), f32(B, 3 * J, 26), f32(B, 26)
    kp, offset, wv, conf, bound = f32(B, J, 4), f32(17, 4, 4), f32(J, 4), f32(B, V, J), f32(26)
    bone = torch.zeros(J, dtype=torch.int32, device="cuda")
    pair_a = torch.zeros(4, dtype=torch.int32, device="cuda")
    pair_m = f32(4)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr()                                                        # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    Ag = lambda: (out((B, 26, 26)), out((B, 26)))                                        # noqa: E731
    i32 = torch.int32
    for bad, code in ((0, SHR_EINVAL), (65, SHR_ETOOLARGE)):
        del outs[:]
        calls = {
            "shr_pose_keypoints_jacobian": lambda: lib.shr_pose_keypoints_jacobian(
                ptr(params), B, ptr(offset), ptr(offset), bad, ptr(bone), ptr(wv), 1, out((B, J, 4), torch.float32),
                out((B, 3 * J, 26), torch.float32), stream),
            "shr_sphere_icp_normal": lambda: lib.shr_sphere_icp_normal(
                ptr(obs), ptr(centres), ptr(radii), ptr(view), ptr(jac), B, V, bad, W, H, 1.0, 0.0, 1.0, 0.0, 99.0, 50.0, *Ag(),
                out((B,)), out((B,), i32), out((B, J, 12)), out((B, V, H, W), torch.float32), out((B, V, H, W), i32), ptr(ws), stream),
            "shr_sphere_icp_radii_normal": lambda: lib.shr_sphere_icp_radii_normal(
                ptr(obs), ptr(centres), ptr(radii), ptr(view), ptr(jac), B, V, bad, W, H, 1, 1.0, 0.0, 1.0, 0.0, 99.0, 50.0, *Ag(),
                out((B,)), out((B,), i32), out((B, 26, J)), out((B, J, J)), out((B, J)), out((B, J, 16)),
                out((B, V, H, W), torch.float32), out((B, V, H, W), i32), ptr(ws), stream),
            "shr_sphere_render_normal": lambda: lib.shr_sphere_render_normal(
                ptr(obs), ptr(centres), ptr(radii), ptr(view), ptr(jac), B, V, bad, W, H, 1.0, 0.0, 1.0, 0.0, 99.0, 100.0, 10.0, 1.0, 0,
                *Ag(), out((B,)), out((B,), i32), out((B, J, 12)), out((B, V, H, W), torch.float32), out((B, V, H, W), i32), ptr(ws),
                stream),
            "shr_sphere_prior_normal": lambda: lib.shr_sphere_prior_normal(
                ptr(centres), ptr(view), ptr(jac), ptr(params), ptr(centres), ptr(conf), 1.0, 10.0, ptr(bound), ptr(bound), 1.0, B, V,
                bad, 0, *Ag(), out((B,)), out((B, 2), i32), out((B, J, 12)), None, stream),
            "shr_sphere_collision_normal": lambda: lib.shr_sphere_collision_normal(
                ptr(kp), ptr(jac), ptr(pair_a), ptr(pair_a), ptr(pair_m), 1.0, B, bad, 4, 0, *Ag(), out((B,)), out((B,), i32),
                out((B, 4)), None, stream),
            "shr_sphere_temporal_normal": lambda: lib.shr_sphere_temporal_normal(
                ptr(kp), ptr(jac), None, 1.0, 10.0, B, 2, bad, 0, *Ag(), out((B, 26, 26)), out((B,)), out((B,), i32), None, stream),
            "shr_sphere_accel_normal": lambda: lib.shr_sphere_accel_normal(
                ptr(kp), ptr(jac), None, 1.0, 10.0, B, 2, bad, 0, 0, *Ag(), out((B, 26, 26)), out((B, 26, 26)), out((B,)),
                out((B,), i32), None, stream),
        }
        for name, call in calls.items():
            assert call() == code, (name, bad)
        torch.cuda.synchronize()
        assert len(outs) > 40 and all(bool((t == -12345).all()) for t in outs)
