"""The keypoint and joint-limit terms of the sphere fit on the GPU (ops.sphere_prior_normal / sphere_icp_priors,
render.SpherePriorPoseFitter): the counts exactly, the cost bit for bit against the fp64 chain in the header's order, A, g
and the moments against the fp64 restatement (tests/sphere_prior_ref.py) at the fp32 bars tests/test_sphere_prior_cpu.py
measures on the same inputs, the edge rules, and the loop.

Shapes: B in {0, 1, 3, 5}, V in {1, 2, 3}; the hand's 41 spheres, both hands; sphere_icp_ref.synthetic_table's 7 spheres;
the loops at 32 x 32 and 48 x 40."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_icp_ref as sref
import sphere_prior_ref as pref
import sphere_render_icp_ref as rref
import test_sphere_prior_cpu as cpu
from test_sphere_icp_gpu import identity, kernel_centres, tables, within
from test_sphere_icp_gpu import on_device as base_on_device
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu
INF = float("inf")

# g against autograd through the fp32 first-order path (ops.PoseSpheres -> the view transform in torch): that path's
# backward sums up to 3 x 41 x V terms per parameter in fp32, each within 2^-24 of its magnitude, against a g whose
# largest entry those terms partly cancel in: 1e-4 of the largest entry, the bar of the render term's autograd test.
AUTOGRAD_BAR = 1e-4


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def on_device(case):
    c = base_on_device(case)
    c["dev"].update(keypoints=torch.from_numpy(case["keypoints"]).cuda(), confidence=torch.from_numpy(case["confidence"]).cuda(),
                    lower=torch.from_numpy(case["lower"]).cuda(), upper=torch.from_numpy(case["upper"]).cuda())
    return c


@pytest.fixture(scope="module")
def cases(mesh):
    """name -> the case of sphere_prior_ref.cached_cases with its tables on the device (`dev`)."""
    return {case["name"]: on_device(case) for case in pref.cached_cases(mesh)}


def inputs(case, rows=slice(None), views=slice(None)):
    d = case["dev"]
    return (d["params0"][rows].contiguous(), d["view"][rows, views].contiguous(), d["keypoints"][rows, views].contiguous(),
            d["confidence"][rows, views].contiguous())


def prior(case, p, view, k, conf, kw=1.0, km=INF, lw=0.0, into=None, limits=True):
    """(A, g, cost, count, moments) of the entry at pose p [B,26] under view [B,V,4,4]."""
    from spherehand_amd import ops
    d = case["dev"]
    if limits is True:
        limits = (d["lower"], d["upper"])
    return ops.sphere_prior_normal(view, p, *tables(case)[:4], case["model"].right_hand, k, conf, kw, km, limits or None, lw, into)


def image_terms(case, p, obs, view):
    """(A, g, cost) of the two image terms at the module's defaults: what the entry accumulates on."""
    from spherehand_amd import ops
    A, g, cost = ops.sphere_icp_normal(obs, view, p, *tables(case), case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST)[:3]
    return ops.sphere_render_normal(obs, view, p, *tables(case), case["model"].right_hand, case["p2m"], ref.FG_MAX,
                                    rref.DEFAULT_MAX_RESID, rref.BACKGROUND, rref.DEFAULT_WEIGHT, (A, g, cost))[:3]


def npy(t):
    return None if t is None else t.cpu().numpy()


@pytest.mark.parametrize("name,rows,views,kw,km,lw", cpu.EVALUATIONS)
def test_normal_equations(cases, name, rows, views, kw, km, lw):
    """Given the entry's own fp32 centres and Jacobian: count and the per-sphere counts exact; A bit-symmetric; the cost
    bit-equal to the fp64 chain in the header's order; A and g within 4 x the fp32 bars of the row-wise fp64 sums formed
    on that Jacobian (sphere_prior_ref.given), the moments within theirs of the restatement's (directions by autograd)."""
    case = cases[name]
    p, view, k, conf = inputs(case, slice(0, rows), slice(*views))
    A, g, cost, count, moments = prior(case, p, view, k, conf, kw, km, lw)
    c32, _ = kernel_centres(case, p, view)
    lo, hi = case["lower"], case["upper"]
    want = pref.normal(case["model"], view.double().cpu(), p.double().cpu(), npy(k), npy(conf), kw, km, lo, hi, lw, centres32=c32)
    print("pairs with rows %s, limit rows %s" % (want["count"][:, 0].tolist(), want["count"][:, 1].tolist()))
    assert torch.equal(count.cpu().long(), want["count"]) and int(want["count"][:, 0].min()) > 3
    assert torch.equal(moments[..., 10].cpu(), want["moments"][..., 10]) and not bool(moments[..., 11].any())
    assert torch.equal(A, A.transpose(1, 2))
    chain = pref.cost_chain(c32, npy(k), npy(conf), kw, km, npy(p), lo, hi, lw)
    print("cost %s, the chain %s" % (cost.tolist(), chain.tolist()))
    assert np.array_equal(cost.cpu().numpy().view(np.int64), chain.view(np.int64))
    from spherehand_amd import ops
    d = case["dev"]
    _, jac = ops.pose_keypoints_jacobian(p, d["offset"], d["offset_inv"], d["bone"], d["wv"], case["model"].right_hand)
    A_rows, g_rows = pref.given(npy(jac), npy(view), c32, npy(p), npy(k), npy(conf), kw, km, lo, hi, lw)
    within(A, A_rows, cpu.A_BAR, "A")
    within(g, g_rows, cpu.G_BAR, "g")
    scale = want["A"].abs().flatten(1).amax(1)
    print("A against the fp64 CHAIN's (not given the Jacobian; printed only): %.3g of its largest entry"
          % ((A.cpu() - want["A"]).abs().flatten(1).amax(1) / scale).max().item())
    for grp, what in zip(cpu.MOMENT_GROUPS, ("sum w uu^T", "sum w e u")):
        within(moments[..., grp], want["moments"][..., grp], cpu.M_BAR, what)
    within(moments[..., 9:10], want["moments"][..., 9:10], 1e-13, "sum w e^2 over the rows")     # (the same terms: only the order)


@pytest.mark.parametrize("km", (INF, 12.0))
def test_g_is_the_autograd_gradient_of_the_first_order_path(cases, km):
    """g = the gradient of 1/2 cost by autograd through ops.PoseSpheres -> a torch matmul with `view` -> the torch
    expression of the cost (the truncated quadratic and the hinge), under three views, one a general rotation."""
    from spherehand_amd import ops
    case = cases["right"]
    d = case["dev"]
    p, view, k, conf = inputs(case)
    kw, lw = 0.5, 30.0
    A, g, cost, count, moments = prior(case, p, view, k, conf, kw, km, lw)
    q = p.clone().requires_grad_(True)
    sph = ops.PoseSpheres.apply(q, d["offset"], d["offset_inv"], d["bone"], d["wv"], d["radii"], d["bone_start"], d["bone_points"],
                                case["model"].right_hand)
    cv = torch.matmul(view[:, :, None, :3, :3], sph[:, None, :, :3, None]).squeeze(-1) + view[:, :, None, :3, 3]
    live = ~torch.isnan(k).any(-1) & (conf != 0)
    e = torch.where(live[..., None], k.double() - cv.double(), torch.zeros_like(cv, dtype=torch.float64))
    n2 = (e * e).sum(-1)
    term = torch.where(n2 < km * km, n2, torch.full_like(n2, min(km * km, 1e300)))
    qd = q.double()
    lo, hi = d["lower"].double(), d["upper"].double()
    h = torch.where(qd > hi, qd - hi, torch.where(qd < lo, qd - lo, torch.zeros_like(qd)))
    total = kw * (conf.double() * term * live).sum((1, 2)) + lw * (h * h).sum(1)
    (0.5 * total.sum()).backward()
    print("cost %s against torch's %s; limit rows %s" % (cost.tolist(), total.tolist(), count[:, 1].tolist()))
    assert torch.allclose(total.detach(), cost, rtol=1e-5) and int(count[:, 1].sum()) > 0
    if km < INF:
        assert 0 < int(count[:, 0].sum()) < int(live.sum())
    within(g, q.grad.double().cpu(), AUTOGRAD_BAR, "g against autograd through ops.PoseSpheres")


def test_dropped_pairs_and_absent_terms(cases):
    """A NaN keypoint component, a confidence of 0 and a confidence of NaN drop the pair in the same way, bit for bit: with one
    view the sphere has no moments and the count is one less.  keypoints = None equals the call whose pairs are all dropped;
    limits = None equals the call whose bounds are all infinite."""
    case = cases["left"]
    p, view, k, conf = inputs(case, slice(0, 3), slice(0, 1))
    full = prior(case, p, view, k, conf, 0.5, INF, 100.0)
    B, J = 3, 41
    b, j = 1, 17
    assert bool(torch.isfinite(k[b, 0, j]).all()) and float(conf[b, 0, j]) > 0
    variants = []
    for kind in ("nan_keypoint", "zero", "nan_confidence"):
        kk, cc = k.clone(), conf.clone()
        if kind == "nan_keypoint":
            kk[b, 0, j, 1] = float("nan")
        else:
            cc[b, 0, j] = 0.0 if kind == "zero" else float("nan")
        variants.append(prior(case, p, view, kk, cc, 0.5, INF, 100.0))
    for out in variants[1:]:
        for x, y in zip(variants[0], out):
            assert torch.equal(bits(x), bits(y))
    out = variants[0]
    assert int(out[3][b, 0]) == int(full[3][b, 0]) - 1 and not bool(out[4][b, j].any()) and bool(full[4][b, j, :6].any())
    assert not torch.equal(out[0][b], full[0][b]) and torch.equal(bits(out[0][0]), bits(full[0][0]))
    none = prior(case, p, view, None, None, 0.5, INF, 100.0)
    dropped = prior(case, p, view, torch.full_like(k, float("nan")), conf, 0.5, INF, 100.0)
    zeroed = prior(case, p, view, k, torch.zeros_like(conf), 0.5, INF, 100.0)
    for other in (dropped, zeroed):
        for x, y in zip(none, other):
            assert torch.equal(bits(x), bits(y))
    assert not bool(none[4].any()) and not bool(none[3][:, 0].any()) and int(none[3][:, 1].sum()) > 0 and bool(none[2].sum() > 0)
    d = case["dev"]
    free = (torch.full_like(d["lower"], -INF), torch.full_like(d["upper"], INF))
    for x, y in zip(prior(case, p, view, k, conf, 0.5, INF, 100.0, limits=free), prior(case, p, view, k, conf, 0.5, INF, 100.0, limits=False)):
        assert torch.equal(bits(x), bits(y))                       # infinite bounds never fire


def exact_offset(c):
    """(k, d): k fp32 [3] with (double)k - (double)c == d exactly, d a permutation / sign change of (3, 4, 0): |d| = 5."""
    for d in ((3, 4, 0), (-3, 4, 0), (3, -4, 0), (-3, -4, 0), (0, 3, 4), (0, -3, 4), (4, 0, 3), (-4, 0, -3), (0, 3, -4), (4, 3, 0)):
        k = (c + np.asarray(d, np.float32)).astype(np.float32)
        if np.array_equal(k.astype(np.float64) - c.astype(np.float64), np.asarray(d, np.float64)):
            return k, d
    raise AssertionError("no exact offset from %r" % (c,))


def test_saturation_edge_and_zero_residual(cases):
    """On the synthetic table under its translation views: a keypoint at a distance of exactly 5 from its centre (the fp32
    difference is exact) is SATURATED at kp_max = 5 -- no row, cost w 25 -- and gives rows at the next fp32 above 5.
    Keypoints equal to the entry's own centres: e = 0 gives all rows, cost 0 and g = 0."""
    case = cases["synthetic"]
    p, view, k, conf = inputs(case)
    B, V, J = k.shape[:3]
    c32, _ = kernel_centres(case, p, view)
    k_np = c32.copy()
    b, v, j = 1, 1, 5
    k_np[b, v, j], d = exact_offset(c32[b, v, j])
    kk = torch.from_numpy(k_np).cuda()
    ones = torch.ones_like(conf)
    w = 0.75
    ones[b, v, j] = w
    at = prior(case, p, view, kk, ones, 2.0, 5.0, 0.0)
    above = prior(case, p, view, kk, ones, 2.0, float(np.nextafter(np.float32(5.0), np.float32(6.0))), 0.0)
    print("offset %s: pairs with rows %s at kp_max = 5, %s just above; cost %s, %s" % (d, at[3][:, 0].tolist(), above[3][:, 0].tolist(),
                                                                                     at[2].tolist(), above[2].tolist()))
    assert at[3][:, 0].tolist() == [V * J, V * J - 1, V * J] and above[3][:, 0].tolist() == [V * J] * 3
    assert at[2].tolist() == [0.0, 2.0 * (w * 25.0), 0.0] and above[2].tolist() == at[2].tolist()
    assert not bool(at[1].any()) and bool(above[1][b].any()) and not bool(above[1][0].any())
    assert float(at[4][b, j, 10]) == 1.0 and float(above[4][b, j, 10]) == 2.0
    zero = prior(case, p, view, torch.from_numpy(c32.copy()).cuda(), conf, 2.0, 5.0, 0.0)
    assert zero[3][:, 0].tolist() == [int((conf[i] != 0).sum()) for i in range(B)] and not bool(zero[2].any()) and not bool(zero[1].any())
    assert bool((zero[0].abs().amax((1, 2)) > 0).all()) and not bool(zero[4][..., 6:10].any())


def test_hinge_at_the_bounds(cases):
    """A parameter exactly ON a bound gives no row; one fp32 beyond it gives one: limit_weight on A_ii, limit_weight h on g_i,
    limit_weight h^2 in the cost, bit for bit.  The palm's infinite bounds never fire."""
    case = cases["right"]
    d = case["dev"]
    lo, hi = case["lower"], case["upper"]
    p = torch.zeros(3, 26)
    p[:, :6] = torch.tensor([3.0, -3.0, 3.1, -1000.0, 1000.0, 50.0])
    p[0, 8], p[0, 22] = float(hi[8]), float(lo[22])
    p[1, 8], p[1, 22] = float(np.nextafter(hi[8], np.float32(INF))), float(np.nextafter(lo[22], np.float32(-INF)))
    p[2, 13] = float(hi[13]) + 0.5
    p = p.cuda()
    view = identity(3, 1)
    A, g, cost, count, moments = prior(case, p, view, None, None, 0.0, INF, 100.0)
    h = torch.as_tensor(pref.hinge(p.cpu().numpy(), lo, hi))
    print("limit rows %s, h %s" % (count[:, 1].tolist(), h[h != 0].tolist()))
    assert count.cpu().tolist() == [[0, 0], [0, 2], [0, 1]] and (h != 0).sum(1).tolist() == [0, 2, 1]
    assert torch.equal(bits(A.cpu()), bits(torch.diag_embed(100.0 * (h != 0).double())))
    assert torch.equal(bits(g.cpu()), bits(100.0 * h))
    assert np.array_equal(cost.cpu().numpy().view(np.int64), pref.cost_chain(np.zeros((3, 1, 41, 3), np.float32), None, None,
                                                                             0.0, INF, p.cpu().numpy(), lo, hi, 100.0).view(np.int64))
    assert not bool(moments.any())


def test_two_identical_views_double(cases):
    """V = 2 with two identical views, the general rotation: count, A, g, cost and the moments of the keypoint part are
    exactly 2 x the single view's."""
    case = cases["right"]
    p, view, k, conf = inputs(case, slice(0, 3), slice(2, 3))
    R = view[0, 0, :3, :3].cpu().numpy()
    assert np.abs(R - R.T).max() > 0.3
    twice = lambda t: t.expand(3, 2, *t.shape[2:]).contiguous()   # noqa: E731
    one = prior(case, p, view, k, conf, 0.5, 15.0, 0.0, limits=False)
    two = prior(case, p, twice(view), twice(k), twice(conf), 0.5, 15.0, 0.0, limits=False)
    assert bool((one[3][:, 0] > 10).all())
    for a, b in zip(one, two):
        assert torch.equal(2 * a, b)


def test_accumulate(cases):
    """accumulate = 1 on top of the two image terms: A, g and cost are their sum plus the accumulate = 0 result, one fp64
    rounding each (bit-equal to the sum formed in torch); A stays bit-symmetric; count and moments are the terms' own.  Both
    weights 0, or neither term, with accumulate = 1 leave the buffers bit-identical."""
    case = cases["left"]
    p, view, k, conf = inputs(case)
    obs = case["dev"]["observed"]
    base = image_terms(case, p, obs, view)
    alone = prior(case, p, view, k, conf, 0.25, 15.0, 1e4)
    into = tuple(t.clone() for t in base)
    both = prior(case, p, view, k, conf, 0.25, 15.0, 1e4, into)
    for i in range(3):
        assert both[i].data_ptr() == into[i].data_ptr()
        assert torch.equal(bits(both[i]), bits(base[i] + alone[i])), i
    assert torch.equal(both[0], both[0].transpose(1, 2))
    assert torch.equal(both[3], alone[3]) and torch.equal(bits(both[4]), bits(alone[4]))
    assert bool((alone[3][:, 0] > 30).all()) and int(alone[3][:, 1].sum()) > 0
    for kwargs in (dict(kw=0.0, lw=0.0), dict(k=None, conf=None, limits=False, kw=1.0, lw=1.0), dict(k=None, conf=None, kw=1.0, lw=0.0)):
        args = dict(k=k, conf=conf, kw=0.25, km=15.0, lw=1e4, limits=True)
        args.update(kwargs)
        into = tuple(t.clone() for t in base)
        none = prior(case, p, view, into=into, **args)
        for i in range(3):
            assert torch.equal(bits(none[i]), bits(base[i])), (kwargs, i)
    assert torch.equal(prior(case, p, view, k, conf, 0.0, 15.0, 0.0, tuple(t.clone() for t in base))[3], alone[3])
    zero = prior(case, p, view, k, conf, 0.0, 15.0, 0.0)
    assert not bool(zero[0].any()) and not bool(zero[1].any()) and not bool(zero[2].any()) and torch.equal(bits(zero[4]), bits(alone[4]))


def solve(case, rows=slice(None), views=slice(None), iters=None, observed=None, keypoints=None, kw=cpu.KP_WEIGHT, km=cpu.KP_MAX,
          lw=cpu.LIMIT_WEIGHT, terms=True):
    from spherehand_amd import ops
    d = case["dev"]
    obs = d["observed"][rows, views].contiguous() if observed is None else observed
    k = d["keypoints"][rows, views].contiguous() if keypoints is None else keypoints
    return ops.sphere_icp_priors(obs, d["view"][rows, views].contiguous(), d["params0"][rows].contiguous(), *tables(case),
                                 case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST,
                                 case["iters"] if iters is None else iters, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT,
                                 rref.DEFAULT_MAX_RESID, rref.BACKGROUND, k if terms else None,
                                 d["confidence"][rows, views].contiguous() if terms else None, kw, km,
                                 (d["lower"], d["upper"]) if terms else None, lw)


def render_solve(case, iters):
    from spherehand_amd import ops
    d = case["dev"]
    return ops.sphere_icp_render(d["observed"], d["view"], d["params0"], *tables(case), case["model"].right_hand, case["p2m"],
                                 ref.FG_MAX, ref.MAX_DIST, iters, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT,
                                 rref.DEFAULT_MAX_RESID, rref.BACKGROUND)


def test_no_prior_term_is_sphere_icp_render(cases):
    """Both weights 0, or neither keypoints nor limits: ops.sphere_icp_render bit for bit; with the terms the pose differs."""
    case = cases["left"]
    want = render_solve(case, 3)
    for out in (solve(case, iters=3, kw=0.0, lw=0.0), solve(case, iters=3, terms=False)):
        for a, b in zip(out, want):
            assert torch.equal(bits(a), bits(b))
    assert not torch.equal(solve(case, iters=3)[0], want[0])


def test_no_iterations_and_empty_batch(cases):
    case = cases["right"]
    d = case["dev"]
    q, c0, c = solve(case, iters=0)
    assert torch.equal(q, d["params0"]) and torch.equal(c, c0) and bool((c0 > 0).all())
    p, view, k, conf = inputs(case)
    into = image_terms(case, p, d["observed"], view)
    assert torch.equal(c0, prior(case, p, view, k, conf, cpu.KP_WEIGHT, cpu.KP_MAX, cpu.LIMIT_WEIGHT, into)[2].float())
    q, c0, c = solve(case, slice(0, 0))
    assert q.shape == (0, 26) and c0.shape == (0,) and c.shape == (0,)
    out = prior(case, *inputs(case, slice(0, 0)))
    assert out[0].shape == (0, 26, 26) and out[3].shape == (0, 2) and out[4].shape == (0, 41, 12)


def test_reproducible_and_independent_of_the_batch(cases):
    """Twice the same bits; sample i of a batch equals the batch of sample i alone, for the equations and for the whole
    solve (three views)."""
    case = cases["left"]
    one, two = (prior(case, *inputs(case), 0.25, 15.0, 1e4) for _ in range(2))
    for a, b in zip(one, two):
        assert torch.equal(bits(a), bits(b))
    s1, s2 = solve(case, iters=3), solve(case, iters=3)
    for a, b in zip(s1, s2):
        assert torch.equal(bits(a), bits(b))
    for i in (1, 4):
        rows = slice(i, i + 1)
        alone = prior(case, *inputs(case, rows), 0.25, 15.0, 1e4)
        for a, b in zip(one, alone):
            assert torch.equal(bits(a[rows]), bits(b)), i
        for a, b in zip(s1, solve(case, rows, iters=3)):
            assert torch.equal(bits(a[rows]), bits(b)), i


def test_solve_in_a_graph(cases):
    """The whole loop (V = 3) captured into one torch.cuda.graph on a single stream and replayed on other observations and
    keypoints equals the eager result bit for bit: nothing in the loop returns to the host."""
    case = cases["right"]
    d = case["dev"]
    static_obs, static_k = d["observed"].clone(), d["keypoints"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        solve(case, observed=static_obs, keypoints=static_k, iters=4)      # warm-up: the library and the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = solve(case, observed=static_obs, keypoints=static_k, iters=4)
    other_obs, other_k = torch.roll(d["observed"], 1, 0).contiguous(), torch.roll(d["keypoints"], 1, 0).contiguous()
    static_obs.copy_(other_obs)
    static_k.copy_(other_k)
    graph.replay()
    torch.cuda.synchronize()
    eager = solve(case, observed=other_obs, keypoints=other_k, iters=4)
    for a, b in zip(out, eager):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(eager[0], solve(case, iters=4)[0])


def test_module(mesh, cases):
    """render.SpherePriorPoseFitter is the ops with the hand's tables and pose_limits(): solve and normal_equations (the
    four terms' sum) bit for bit, with views and, for [B,H,W] and keypoints [B,41,3], with the identity view; without
    keypoints and with limit_weight = 0 it is SphereRenderPoseFitter."""
    from spherehand_amd.render import SpherePriorPoseFitter, SphereRenderPoseFitter
    case = cases["left"]
    d = case["dev"]
    kw = dict(right_hand=case["model"].right_hand, iters=2, stiffness=case["stiffness"].numpy())
    fit = SpherePriorPoseFitter(mesh, case["W"], case["H"], **kw).cuda()
    p, view, k, conf = inputs(case)
    obs = d["observed"]
    for a, b in zip(fit.solve(obs, p, view, keypoints=k, confidence=conf), solve(case, iters=2)):
        assert torch.equal(bits(a), bits(b))
    into = image_terms(case, p, obs, view)
    for a, b in zip(fit.normal_equations(obs, p, view, k, conf), prior(case, p, view, k, conf, cpu.KP_WEIGHT, cpu.KP_MAX,
                                                                        cpu.LIMIT_WEIGHT, into)):
        assert torch.equal(bits(a), bits(b))
    from spherehand_amd import ops
    single = ops.sphere_icp_priors(obs[:, :1].contiguous(), identity(5, 1), p, *tables(case), case["model"].right_hand, case["p2m"],
                                   ref.FG_MAX, ref.MAX_DIST, 2, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT,
                                   rref.DEFAULT_MAX_RESID, rref.BACKGROUND, k[:, :1].contiguous(), conf[:, :1].contiguous(),
                                   cpu.KP_WEIGHT, cpu.KP_MAX, (d["lower"], d["upper"]), cpu.LIMIT_WEIGHT)
    for a, b in zip(fit.solve(obs[:, 0].contiguous(), p, keypoints=k[:, 0].contiguous(), confidence=conf[:, 0].contiguous()), single):
        assert torch.equal(bits(a), bits(b))
    off = SpherePriorPoseFitter(mesh, case["W"], case["H"], limit_weight=0.0, **kw).cuda()
    for a, b in zip(off.solve(obs, p, view), SphereRenderPoseFitter(mesh, case["W"], case["H"], **kw).cuda().solve(obs, p, view)):
        assert torch.equal(bits(a), bits(b))


def test_end_to_end(cases):
    """The right hand at 48 x 40, seed sphere_prior_ref.END_TO_END_SEED, one view, the module's defaults, keypoints with
    sigma_k = 2 mm, 6 iterations, B = 5.  cost <= cost0 on every sample.  The pose is within 4 x the fp32 bar of the fp64
    restatement's on the samples where the CPU fp32 and fp64 restatements keep the same accept sequence and the same active
    hinge rows; at most one of five may be left out."""
    case = cases["end_to_end"]
    q, c0, c = solve(case, iters=pref.END_TO_END_ITERS)
    assert bool((c <= c0).all()) and bool(torch.isfinite(q).all())
    run = cpu.end_to_end_runs(case)
    q64, c064, c64, lm64 = run[torch.float64]
    same = cpu.kept(lm64, run[torch.float32][3])
    err = (q.cpu().double() - q64).abs().max(1).values
    print("last fp64 step %s, the fp32 restatement keeps %s; |pose - restatement| %s; cost %s against %s"
          % (lm64.last_step.tolist(), same.tolist(), err.tolist(), c.tolist(), c64.tolist()))
    assert torch.allclose(c0.cpu().double(), c064, rtol=cpu.COST_BAR + 2.0 ** -23)       # (cost0 leaves the loop as fp32)
    assert int(same.sum()) >= 4
    assert bool((err[same] <= cpu.POSE_BAR).all()), (err, cpu.POSE_BAR)
    e = sref.keypoint_error(case["model"], q.cpu(), case["p_star"]).mean().item()
    print("mean keypoint error %.4g mm (the restatement's %.4g)" % (e, sref.keypoint_error(case["model"], q64, case["p_star"]).mean().item()))
