"""The marginal covariances of the sequence fit on the GPU (shr_pose_lm_seq2_covariance through ops.pose_lm_covariance and the
fitters' uncertainty()), held to tests/lm_covariance_ref.py by that file's ONE comparator: every sequence of every case within
MARGIN x the restatement's own distance to numpy.linalg.inv of the dense matrix, which is the project's bar (DESIGN.md 4.4w,
4.4y); both sides are fp64 in one stated order, so bits are expected, and the number of sequences that match bit for bit is
printed.  The inputs are lm_covariance_ref's, stated and checked on the CPU (tests/test_lm_covariance_cpu.py)."""
import numpy as np
import pytest
import torch

import lm_covariance_ref as cref
import pose_icp_ref as ref
import sphere_sequence_ref as qref

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.cuda().contiguous()


def run(eqs, T, mu=None, jac=None, workspace=None):
    from spherehand_amd import ops
    A, E, F = eqs
    cov, sph, status = ops.pose_lm_covariance(dev(A), dev(E), dev(F), T, dev(mu), dev(jac), workspace)
    return cov.cpu(), None if sph is None else sph.cpu(), status.cpu()


def held(name, eqs, T, mu, jac, got=None):
    """the run against the reference; returns (got, want, the comparator's counts)"""
    got = run(eqs, T, mu, jac) if got is None else got
    want = cref.reference(*eqs, T, mu, jac)
    out = {}
    bad = cref.compare(got, want, out)
    print("%-36s %d of %d sequences bit for bit; largest error / bar %.3g; largest |restatement - dense| %.3g"
          % (name, out["exact"], out["live"], out["ratio"], want["gap"].max()))
    assert not bad, (name, bad)
    return got, want, out


def test_shapes_kinds_and_sphere_counts():
    """S = 3 at T in {1, 2, 3, 4, 6}, seq (F None) and seq2, J in {1, 41, 64}, without a stiffness and with one up to 0.5,
    E None at T = 3 (with and without an F, which is then not read): every sequence factorises and is held to the bar; the
    3 x 3 blocks are symmetric expansions; the same call twice gives the same bits."""
    for name, kind, T, eqs, mu, J in cref.shape_cases():
        jac = cref.jacobian(eqs[0].shape[0], J)
        got, want, _ = held(name, eqs, T, mu, jac)
        assert not want["status"].any() and got[1].shape == (eqs[0].shape[0], J, 3, 3)
        assert torch.equal(got[1], got[1].transpose(2, 3))
        again = run(eqs, T, mu, jac)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), name
        alone = run(eqs, T, mu, None)
        assert alone[1] is None and torch.equal(alone[0], got[0]) and torch.equal(alone[2], got[2]), name
    A, E, F = cref.shape_cases()[-1][3]
    with_f, without = run((A, None, F), 3), run((A, None, None), 3)
    assert torch.equal(with_f[0], without[0])
    frames = run((A, None, None), 1)                           # E None: every frame is its own system
    assert torch.equal(frames[0], without[0])


def test_long_chains_and_many_sequences():
    """One chain of T = 64 at S = 2 and S = 65 at T = 2: the last sequence has the first one's inputs and its bits."""
    for name, kind, T, eqs, mu, J in cref.long_cases():
        jac = cref.jacobian(eqs[0].shape[0], J)
        jac[-T:] = jac[:T]
        got, want, _ = held(name, eqs, T, mu, jac)
        assert not want["status"].any()
        assert torch.equal(got[0][-T:], got[0][:T]) and torch.equal(got[1][-T:], got[1][:T]), name


def test_conditioning():
    """The conditioning sweep at T = 5 (own rows 40, 6, 0; stiffness 0, 1e-3, 0.5; coupling weight 1, 1e4), the cases that
    factorise at lambda = 0: the bar grows with the condition number because the restatement's own distance to the dense
    inverse does, and nothing else is allowed."""
    cases = cref.conditioning_cases()
    assert len(cases) >= 24
    exact = live = 0
    for name, kind, T, eqs, mu, J in cases:
        _, want, out = held(name, eqs, T, mu, cref.jacobian(eqs[0].shape[0], J))
        assert not want["status"].any()
        exact, live = exact + out["exact"], live + out["live"]
    print("conditioning: %d of %d sequences bit for bit" % (exact, live))


def test_a_failing_sequence_between_two_good_ones():
    """The middle sequence's pivot fails at frame t (through E at every t >= 1, through F at every t >= 2): status 1 + t,
    every cov and sphere_cov entry of its frames a NaN, and its neighbours' bits are those of the batch without the failure.
    A second call on the SAME workspace after the failed one gives the clean result."""
    from spherehand_amd import _lib
    T = cref.PIVOT_T
    mu = cref.random_stiffness(5)
    jac = cref.jacobian(3 * T, 41)
    ws = torch.empty(_lib.lib().shr_pose_lm_seq2_covariance_workspace_bytes(3 * T) // 8, dtype=torch.float64, device="cuda")
    for name, kind, bad_eqs, good_eqs, t in cref.pivot_cases():
        clean = run(good_eqs, T, mu, jac)
        got = run(bad_eqs, T, mu, jac, ws)
        after = run(good_eqs, T, mu, jac, ws)
        held(name, bad_eqs, T, mu, jac, got)
        assert got[2].tolist() == [0, 1 + t, 0], (name, got[2])
        assert bool(torch.isnan(got[0][T:2 * T]).all()) and bool(torch.isnan(got[1][T:2 * T]).all()), name
        for s in (0, 2):
            sl = slice(s * T, s * T + T)
            assert torch.equal(got[0][sl], clean[0][sl]) and torch.equal(got[1][sl], clean[1][sl]), (name, s)
        assert all(torch.equal(a, b) for a, b in zip(after, clean)), name
        assert not clean[2].any()


def test_in_a_graph():
    """No host synchronisation: both launches captured into a graph and replayed on other equations give the eager bits."""
    from spherehand_amd import ops
    T = 3
    A, E, F = (dev(t) for t in cref.equations("seq2", 2, T, seed=900))
    A2, E2, F2 = (dev(t) for t in cref.equations("seq2", 2, T, seed=901))
    jac, mu = dev(cref.jacobian(2 * T, 41)), dev(cref.random_stiffness(9))
    sA, sE, sF = A.clone(), E.clone(), F.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.pose_lm_covariance(sA, sE, sF, T, mu, jac)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.pose_lm_covariance(sA, sE, sF, T, mu, jac)
    sA.copy_(A2), sE.copy_(E2), sF.copy_(F2)
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.pose_lm_covariance(A2, E2, F2, T, mu, jac)
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert not torch.equal(eager[0], ops.pose_lm_covariance(A, E, F, T, mu, jac)[0])


def test_fitters_end_to_end():
    """SphereTrajectoryPoseFitter.uncertainty and SpherePoseFitter.uncertainty at 48 x 40 on six frames (two sequences of
    three): held to the restatement fed with the fitter's OWN normal_equations and the entry's own Jacobian; sigma is
    sqrt(trace); residual_var scales the covariances; SphereRadiiCalibrator.uncertainty raises."""
    from spherehand_amd import hand_model, ops
    from spherehand_amd.render import SpherePoseFitter, SphereRadiiCalibrator, SphereTrajectoryPoseFitter
    mesh = hand_model.load_mesh()
    W, H, S, T = 48, 40, 2, 3
    B = S * T
    stiffness = np.maximum(ref.STIFFNESS, 0.01).astype(np.float32)       # every direction held: the matrix is definite
    p_star, p0 = (t.float().cuda() for t in qref.sequence_poses(S, T, 31))
    traj = SphereTrajectoryPoseFitter(mesh, W, H, T, stiffness=stiffness).cuda()
    frames = SpherePoseFitter(mesh, W, H, stiffness=stiffness).cuda()
    J = traj.num_spheres
    tabs = (traj.fk.offset, traj.fk.offset_inv, traj.kp_bone, traj.kp_wv)
    kp, _ = ops.pose_keypoints_jacobian(p_star, *tabs, True)
    spheres = kp.clone()
    spheres[..., 3] = traj.radii
    observed = torch.clamp(ops.sphere_raster_fwd(spheres.contiguous(), H, W), max=100.0).contiguous()
    gen = torch.Generator().manual_seed(5)
    keypoints = (kp[..., :3] + 2.0 * torch.randn(B, J, 3, generator=gen).cuda()).contiguous()
    jac = ops.pose_keypoints_jacobian(p0, *tabs, True)[1].cpu()
    mu = torch.from_numpy(stiffness)
    for name, fit, TT, kw in (("trajectory", traj, T, dict(keypoints=keypoints)), ("frames", frames, 1, {})):
        eqs = fit.normal_equations(observed, p0, **kw)
        E, F = fit._bands(eqs)
        cov, sph, sigma, ok = fit.uncertainty(observed, p0, **kw)
        assert (E is None) == (TT == 1) and bool(ok.all()) and ok.shape == (B // TT,)
        assert cov.shape == (B, 26, 26) and sph.shape == (B, J, 3, 3) and sigma.shape == (B, J)
        host = tuple(None if t is None else t.cpu() for t in (eqs[0], E, F))
        held(name, host, TT, mu, jac, (cov.cpu(), sph.cpu(), (~ok).int().cpu()))
        assert torch.equal(sigma, (sph[..., 0, 0] + sph[..., 1, 1] + sph[..., 2, 2]).sqrt())
        assert bool((sigma > 0).all()) and bool(torch.isfinite(sigma).all())
        cov4, sph4, sigma4, _ = fit.uncertainty(observed, p0, residual_var=4.0, **kw)
        assert torch.equal(cov4, cov * 4.0) and torch.equal(sph4, sph * 4.0)
        assert torch.allclose(sigma4, 2.0 * sigma, rtol=1e-15)
        print("%s: sigma %.3g ... %.3g mm" % (name, sigma.min(), sigma.max()))
    with pytest.raises(NotImplementedError):
        SphereRadiiCalibrator(mesh, W, H, T, stiffness=stiffness).cuda().uncertainty(observed, p0)
