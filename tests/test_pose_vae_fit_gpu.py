"""The pose-VAE prior of the sphere fit on the GPU (ops.pose_vae_normal / sphere_icp_priors with `pose_prior`,
render.PoseVaePrior): GIVEN the entry's own fp32 keypoints and Jacobian and its own ReLU decisions, A, g, cost, residual and
latent against the fp64 restatement (tests/pose_vae_fit_ref.py) at the fp32 bars tests/test_pose_vae_fit_cpu.py measures on
the same cases; the decisions themselves against the fp64 restatement's under a condition on the ReLU input; the bitwise
properties; the argument rules through the C ABI; the loop, eager and in a graph; and the sequence classes.

Shapes: the hand's 41 spheres, both hands, B in {0, 1, 3, 5}; the rest pose, poses of sample_poses and one at
pose_limits(); the loops at 32 x 32."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import pose_vae_fit_ref as vr
import sphere_collision_ref as cref
import sphere_prior_ref as pref
import sphere_render_icp_ref as rref
import test_pose_vae_fit_cpu as cpu
from test_sphere_icp_gpu import tables
from test_sphere_prior_gpu import on_device
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu

# a decision of the entry may differ from the fp64 restatement's only where the fp64 ReLU input is smaller than this
MASK_MARGIN = 1e-5


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


@pytest.fixture(scope="module")
def fitters(mesh):
    """right hand? -> a fitter on the device, for its key-point tables."""
    from spherehand_amd.render import SphereCollisionPoseFitter
    return {right: SphereCollisionPoseFitter(mesh, 32, 32, right_hand=right).cuda() for right in (True, False)}


@pytest.fixture(scope="module")
def blob():
    from spherehand_amd import pose_vae
    return pose_vae.pack_fit_weights(pose_vae.default_pose_vae()).cuda()


@pytest.fixture(scope="module")
def vae_cases(mesh):
    return {c["name"]: c for c in vr.cached_cases(mesh)}


@pytest.fixture(scope="module")
def loop_case(mesh):
    return on_device(pref.case(mesh, "right"))


def entry(fitters, case, blob, w=1.0, lw=0.0, into=None, rows=slice(None)):
    """(A, g, cost, residual, latent, relu_mask) of the entry on the case's poses."""
    from spherehand_amd import ops
    fit = fitters[case["right_hand"]]
    p = torch.from_numpy(np.ascontiguousarray(case["params"][rows])).cuda()
    return ops.pose_vae_normal(p, *fit._tables()[:4], fit.right_hand, blob, w, lw, into)


def own_inputs(fitters, case, rows=slice(None)):
    """(kp [B,41,4], jac [B,123,26]) numpy fp32: what the entry is handed."""
    from spherehand_amd import ops
    fit = fitters[case["right_hand"]]
    p = torch.from_numpy(np.ascontiguousarray(case["params"][rows])).cuda()
    kp, jac = ops.pose_keypoints_jacobian(p, *fit._tables()[:4], fit.right_hand)
    return kp.cpu().numpy(), jac.cpu().numpy()


def raw(kp, jac, blob, w=1.0, lw=0.0, accumulate=0, J=41, floats=None, outputs=None):
    """The C entry on keypoints and a Jacobian of the test's own making -> (rc, A, g, cost); NaN-filled buffers unless given."""
    from spherehand_amd import _lib
    B = kp.shape[0]
    if outputs is None:
        outputs = tuple(torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, 26, 26), (B, 26), (B,)))
    A, g, cost = outputs
    rc = _lib.lib().shr_pose_vae_normal(kp.data_ptr(), jac.data_ptr(), blob.data_ptr(), blob.shape[0] if floats is None else floats,
                                        w, lw, B, J, accumulate, A.data_ptr(), g.data_ptr(), cost.data_ptr(), None, None, None,
                                        None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, A, g, cost


@pytest.mark.parametrize("name", ["right1", "right3", "right5", "left3", "left5"])
def test_normal_equations(fitters, vae_cases, blob, name):
    """GIVEN the entry's own fp32 keypoints, Jacobian and ReLU decisions: residual, latent, and at each of the CPU file's
    WEIGHTS A, g and cost within the fp32 bars of the fp64 restatement; A bit-symmetric.  The decisions differ from the fp64
    restatement's own only at units whose fp64 ReLU input is below MASK_MARGIN in magnitude."""
    case = vae_cases[name]
    kp, jac = own_inputs(fitters, case)
    x = cpu.contract_x(kp)
    own = vr.forward(kp, jac, np.float64, x=x)
    rel = lambda a, b: (np.abs(a - b).reshape(len(a), -1).max(1) / np.abs(b).reshape(len(b), -1).max(1)).max()   # noqa: E731
    for w, lw in cpu.WEIGHTS:
        A, g, cost, residual, latent, words = entry(fitters, case, blob, w, lw)
        mask = vr.unpack_mask(words.cpu().numpy())
        differ = mask != own["mask"]
        print("%s w %g lw %g: %d of %d decisions differ from the fp64 restatement's; their |ReLU input| %s"
              % (name, w, lw, int(differ.sum()), differ.size, np.abs(own["relu_in"][differ]).tolist()))
        assert bool((np.abs(own["relu_in"][differ]) < MASK_MARGIN).all())
        f = vr.forward(kp, jac, np.float64, mask=mask, x=x)
        A64, g64, c64 = vr.normal(f, w, lw)
        figures = dict(A=rel(A.cpu().numpy(), A64), g=rel(g.cpu().numpy(), g64), cost=rel(cost.cpu().numpy(), c64),
                       residual=rel(residual.cpu().numpy(), f["r"]), latent=rel(latent.cpu().numpy(), f["mu"]))
        print("  against the fp64 restatement: %s (bars A %.3g, g %.3g, cost %.3g, residual %.3g, latent %.3g)"
              % (figures, cpu.A_BAR, cpu.G_BAR, cpu.COST_BAR, cpu.RESIDUAL_BAR, cpu.LATENT_BAR))
        assert torch.equal(bits(A), bits(A.transpose(1, 2).contiguous()))
        assert figures["residual"] <= cpu.RESIDUAL_BAR and figures["latent"] <= cpu.LATENT_BAR
        assert figures["A"] <= cpu.A_BAR and figures["g"] <= cpu.G_BAR and figures["cost"] <= cpu.COST_BAR
        # the fp64 sums GIVEN the entry's own rows are the entry's to the order of 155 terms: the cost from its residual and latent
        c_own = float(np.float32(w)) * ((residual.cpu().numpy() ** 2).sum(1)
                                        + float(np.float32(lw)) * (latent.cpu().numpy() ** 2).sum(1) * (lw > 0))
        assert rel(cost.cpu().numpy(), c_own) <= cpu.ORDER_BAR
    assert float(np.abs(own["r"]).max()) > 1.0                  # (not an empty term)


def test_bitwise(fitters, vae_cases, blob):
    """Two runs give the same bits; frame 3 of B = 5 equals the same frame at B = 1; accumulate = 1 onto random buffers is
    into + w x the accumulate = 0, weight = 1 result with one product and one sum per entry, computed in numpy fp64;
    weight = 0 leaves NaN-filled buffers NaN and still writes the term's own outputs."""
    case = vae_cases["right5"]
    one, two = (entry(fitters, case, blob, 0.75, 3.0) for _ in range(2))
    for a, b in zip(one, two):
        assert torch.equal(bits(a) if a.dtype != torch.int32 else a, bits(b) if b.dtype != torch.int32 else b)
    alone = entry(fitters, case, blob, 0.75, 3.0, rows=slice(3, 4))
    for a, b in zip(one, alone):
        assert torch.equal(a[3:4], b)
    unit = entry(fitters, case, blob, 1.0, 3.0)
    gen = torch.Generator().manual_seed(5)
    L = torch.randn(5, 26, 26, generator=gen, dtype=torch.float64)
    M = L @ L.transpose(1, 2)
    into = ((M.tril() + M.tril(-1).transpose(1, 2)).cuda(), torch.randn(5, 26, generator=gen, dtype=torch.float64).cuda(),
            torch.rand(5, generator=gen, dtype=torch.float64).cuda())
    assert torch.equal(into[0], into[0].transpose(1, 2))
    want = [t.cpu().numpy() + np.float64(np.float32(0.3)) * u.cpu().numpy() for t, u in zip(into, unit[:3])]
    got = entry(fitters, case, blob, 0.3, 3.0, into=tuple(t.clone() for t in into))
    for a, b in zip(got[:3], want):
        assert np.array_equal(a.cpu().numpy().view(np.int64), b.view(np.int64))
    assert torch.equal(got[0], got[0].transpose(1, 2))
    kp, jac = (torch.from_numpy(t).cuda() for t in own_inputs(fitters, case))
    for accumulate in (0, 1):
        rc, A, g, cost = raw(kp, jac, blob, 0.0, 1.0, accumulate)
        assert rc == 0 and bool(torch.isnan(A).all()) and bool(torch.isnan(g).all()) and bool(torch.isnan(cost).all())
    zero = entry(fitters, case, blob, 0.0, 0.0)
    for a, b in zip(zero[3:], unit[3:]):
        assert torch.equal(a, b)


def test_empty_batch(fitters, vae_cases, blob):
    out = entry(fitters, vae_cases["empty"], blob)
    assert out[0].shape == (0, 26, 26) and out[3].shape == (0, 123) and out[5].shape == (0, 32)


def test_bad_arguments(fitters, vae_cases, blob):
    """J = 40, a short blob and a negative weight each return SHR_EINVAL through the C ABI and write nothing."""
    kp, jac = (torch.from_numpy(t).cuda() for t in own_inputs(fitters, vae_cases["right3"]))
    for kwargs in (dict(J=40), dict(floats=blob.shape[0] - 1), dict(w=-1.0), dict(lw=-0.5), dict(accumulate=2)):
        rc, A, g, cost = raw(kp, jac, blob, **kwargs)
        assert rc == -1, kwargs
        assert bool(torch.isnan(A).all()) and bool(torch.isnan(cost).all())
    assert raw(kp, jac, blob)[0] == 0


def solve(case, pose_prior, iters=cpu.LOOP_ITERS, observed=None, rows=slice(0, cpu.LOOP_ROWS), **extra):
    from spherehand_amd import ops
    d = case["dev"]
    if "pairs" not in d:                                       # (once: no copy inside a graph capture)
        d["pairs"] = tuple(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in cref.table(case["model"].mesh))
    pairs = d["pairs"]
    obs = d["observed"][rows].contiguous() if observed is None else observed
    return ops.sphere_icp_priors(obs, d["view"][rows].contiguous(), d["params0"][rows].contiguous(), *tables(case),
                                 case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST, iters, 1e-3, d["stiffness"], None,
                                 rref.DEFAULT_WEIGHT, rref.DEFAULT_MAX_RESID, rref.BACKGROUND, d["keypoints"][rows].contiguous(),
                                 d["confidence"][rows].contiguous(), cpu.KP_WEIGHT, cpu.KP_MAX, (d["lower"], d["upper"]),
                                 cpu.LIMIT_WEIGHT, collision=pairs, collision_weight=cpu.COLLISION_WEIGHT,
                                 **(dict(pose_prior=pose_prior) if pose_prior != "absent" else {}), **extra)


def test_no_prior_is_the_parent_loop(mesh, loop_case, blob):
    """ops.sphere_icp_priors with pose_prior = None or weight 0, and a fitter built with pose_prior = None, equal the same
    without the argument, bit for bit; with a weighted prior the pose differs."""
    from spherehand_amd.render import PoseVaePrior, SphereCollisionPoseFitter
    want = solve(loop_case, "absent")
    for out in (solve(loop_case, None), solve(loop_case, (blob, 0.0, 1.0))):
        for a, b in zip(out, want):
            assert torch.equal(bits(a), bits(b))
    assert not torch.equal(solve(loop_case, (blob, cpu.LOOP_WEIGHT, cpu.LOOP_LATENT_WEIGHT))[0], want[0])
    d = loop_case["dev"]
    rows = slice(0, cpu.LOOP_ROWS)
    args = (d["observed"][rows].contiguous(), d["params0"][rows].contiguous(), d["view"][rows].contiguous())
    kw = dict(right_hand=loop_case["model"].right_hand, iters=2)
    plain = SphereCollisionPoseFitter(mesh, 32, 32, **kw).cuda()
    none = SphereCollisionPoseFitter(mesh, 32, 32, pose_prior=None, **kw).cuda()
    zero = SphereCollisionPoseFitter(mesh, 32, 32, pose_prior=PoseVaePrior(weight=0.0), **kw).cuda()
    with_prior = SphereCollisionPoseFitter(mesh, 32, 32, pose_prior=PoseVaePrior(weight=cpu.LOOP_WEIGHT), **kw).cuda()
    base = plain.solve(*args)
    for fit in (none, zero):
        for a, b in zip(fit.solve(*args), base):
            assert torch.equal(bits(a), bits(b))
        for a, b in zip(fit.normal_equations(args[0], args[1], args[2]), plain.normal_equations(args[0], args[1], args[2])):
            assert torch.equal(a, b)
    assert not torch.equal(with_prior.solve(*args)[0], base[0])
    # the module's equations are the parent's plus the entry's, one sum per entry
    A0, g0, c0 = plain.normal_equations(args[0], args[1], args[2])[:3]
    A1, g1, c1 = with_prior.normal_equations(args[0], args[1], args[2])[:3]
    from spherehand_amd import ops
    Ar, gr, cr = ops.pose_vae_normal(args[1], *plain._tables()[:4], plain.right_hand, blob, cpu.LOOP_WEIGHT)[:3]
    assert torch.equal(bits(A1), bits(A0 + Ar)) and torch.equal(bits(g1), bits(g0 + gr)) and torch.equal(bits(c1), bits(c0 + cr))


def test_loop_against_the_restatement(mesh, loop_case, blob):
    """solve at 32 x 32, B = 3, three iterations with the prior: cost <= cost0 on every sample, and the pose within POSE_BAR
    of the fp64 restatement's loop on the samples where the CPU fp32 and fp64 restatements keep the same accept sequence."""
    q, cost0, cost = solve(loop_case, (blob, cpu.LOOP_WEIGHT, cpu.LOOP_LATENT_WEIGHT))
    assert bool((cost <= cost0).all())
    run = cpu.loop_runs(mesh)
    q64, c064, c64, lm64 = run[torch.float64]
    same = cpu.kept(lm64, run[torch.float32][3])
    err = (q.double().cpu() - q64).abs().amax(1)
    print("|pose - pose64| %s (bar %.3g); kept %s; cost0 %s -> %s (restatement %s -> %s)"
          % (err.tolist(), cpu.POSE_BAR, same.tolist(), cost0.tolist(), cost.tolist(), c064.tolist(), c64.tolist()))
    assert int(same.sum()) >= 2 and bool((err[same] <= cpu.POSE_BAR).all())


def test_solve_in_a_graph(loop_case, blob):
    """The loop with the term captured in a torch.cuda.graph and replayed on other observations gives the eager bits."""
    d = loop_case["dev"]
    rows = slice(0, cpu.LOOP_ROWS)
    prior = (blob, cpu.LOOP_WEIGHT, cpu.LOOP_LATENT_WEIGHT)
    static_obs = d["observed"][rows].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        solve(loop_case, prior, observed=static_obs)            # warm-up: the library, the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = solve(loop_case, prior, observed=static_obs)
    other = torch.roll(d["observed"][rows], 1, 0).contiguous()
    static_obs.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = solve(loop_case, prior, observed=other)
    for a, b in zip(out, eager):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(eager[0], solve(loop_case, prior)[0])


def test_sequence_classes_carry_the_term(mesh, loop_case, blob):
    """SphereTrajectoryPoseFitter.normal_equations and SphereWindowTracker.advance with a prior, T = 3 at 32 x 32: A, g and
    the cost of frame 0 minus the same without the prior equal w x the entry's alone, to the order bar (the difference of
    two sums that share every other term); the tracker's departing system carries it too, and its fit moves."""
    from spherehand_amd import ops
    from spherehand_amd.render import PoseVaePrior, SphereTrajectoryPoseFitter, SphereWindowTracker
    d = loop_case["dev"]
    rows = slice(0, 3)
    obs, p, view = d["observed"][rows].contiguous(), d["params0"][rows].contiguous(), d["view"][rows].contiguous()
    w = cpu.LOOP_WEIGHT
    kw = dict(right_hand=loop_case["model"].right_hand, iters=2)
    for cls in (SphereTrajectoryPoseFitter, SphereWindowTracker):
        plain = cls(mesh, 32, 32, 3, **kw).cuda()
        fit = cls(mesh, 32, 32, 3, pose_prior=PoseVaePrior(weight=w), **kw).cuda()
        Ar, gr, cr = ops.pose_vae_normal(p, *plain._tables()[:4], plain.right_hand, blob, w)[:3]
        e0, e1 = plain.normal_equations(obs, p, view), fit.normal_equations(obs, p, view)
        for i, term in ((0, Ar), (1, gr), (4, cr)):
            diff, scale = (e1[i] - e0[i])[0], e1[i][0].abs().max()
            assert bool(((diff - term[0]).abs() <= cpu.ORDER_BAR * scale * 8).all()), (cls.__name__, i)
            assert float(term[0].abs().max()) > 1e-6 * float(scale)
        for i in (2, 3):                                       # E and F: the term is per frame
            assert torch.equal(e1[i], e0[i])
        assert not torch.equal(fit.solve(obs, p, view)[0], plain.solve(obs, p, view)[0])
    tracker, bare = fit, plain
    new_obs = d["observed"][3:4].contiguous()
    new_view = d["view"][3:4].contiguous()
    out = {}
    for name, t in (("with", tracker), ("without", bare)):
        window = t.begin(obs, p, view)[0]
        window["params"] = p.clone()                           # the same poses leave both windows
        out[name] = t.advance(window, new_obs, view_new=new_view)[0]
    A1, A0 = out["with"]["departing"][0], out["without"]["departing"][0]
    diff, scale = (A1 - A0)[0], A1[0].abs().max()
    assert bool(((diff - Ar[0]).abs() <= cpu.ORDER_BAR * scale * 8).all())
    assert torch.equal(A1[1:], A0[1:])
    assert not torch.equal(out["with"]["params"], out["without"]["params"])
