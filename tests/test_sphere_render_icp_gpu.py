"""The model-to-data term of the sphere fit on the GPU (ops.sphere_render_normal / sphere_icp_render,
render.SphereRenderPoseFitter): the render and its owner map bit for bit against the numpy rule and against the sphere
rasterizer, the counts exactly, the cost bit for bit against the exactly rounded sum, and A, g, the moments and the solve
against the fp64 restatement (tests/sphere_render_icp_ref.py) at the fp32 bars tests/test_sphere_render_icp_cpu.py measures
on the same inputs.

Shapes: B in {0, 1, 3, 5}, V in {1, 2, 3}; the hand's 41 spheres, both hands, at 32 x 32 (one tile per view), 48 x 40 (two
tiles per view), 33 x 17 (one partial tile) and 64 x 64 (four tiles); sphere_icp_ref.synthetic_table's 7 spheres."""
import math

import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_icp_ref as sref
import sphere_render_icp_ref as rref
import test_sphere_render_icp_cpu as cpu
from test_sphere_icp_gpu import identity, kernel_centres, on_device, tables, within

pytestmark = pytest.mark.gpu

# g against autograd through the fp32 first-order path (ops.PoseSpheres -> the view transform -> ops.SphereDepthRaster): that
# path sums up to ~10^3 rows per sphere in fp32, each sum within 10^3 x 2^-24 = 6e-5 of its terms' magnitude; 1e-4 of the
# largest entry of g.
AUTOGRAD_BAR = 1e-4


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


@pytest.fixture(scope="module")
def cases(mesh):
    """name -> the case of sphere_render_icp_ref.cached_cases with its tables on the device (`dev`)."""
    return {case["name"]: on_device(case) for case in rref.cached_cases(mesh)}


def evaluate(case, p, observed, view, weight=1.0, max_resid=float("inf"), into=None, p2m=None):
    """(A, g, cost, count, moments, depth, owner) of the kernels at pose p [B,26] under view [B,V,4,4]."""
    from spherehand_amd import ops
    return ops.sphere_render_normal(observed, view, p, *tables(case), case["model"].right_hand, case["p2m"] if p2m is None else p2m,
                                    ref.FG_MAX, max_resid, rref.BACKGROUND, weight, into, want_maps=True)


def d2m(case, p, observed, view):
    from spherehand_amd import ops
    return ops.sphere_icp_normal(observed, view, p, *tables(case), case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST)


def inputs(case, rows=slice(None), views=slice(None)):
    d = case["dev"]
    return d["params0"][rows].contiguous(), d["observed"][rows, views].contiguous(), d["view"][rows, views].contiguous()


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def exact_cost(observed, depth, weight, max_resid=np.inf):
    terms = rref.cost_terms(observed, depth, max_resid=max_resid)
    return torch.tensor([math.fsum(terms[b].ravel().tolist()) * weight for b in range(terms.shape[0])], dtype=torch.float64)


def check_equations(case, p, obs, view, weight, max_resid, centres32=None):
    """Every check of one evaluation against the numpy rule and the fp64 restatement given the kernel's own owner map."""
    A, g, cost, count, moments, depth, owner = evaluate(case, p, obs, view, weight, max_resid)
    m = case["model"]
    c32, _ = kernel_centres(case, p, view)
    if centres32 is not None:
        assert np.array_equal(c32, centres32)
    H, W = obs.shape[2:]
    depth_np, owner_np = rref.render32(c32, m.radii, case["p2m"], W, H)
    assert np.array_equal(owner.cpu().numpy(), owner_np)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), depth_np.view(np.uint32))
    want = rref.normal(m, view.double().cpu(), obs.cpu().numpy(), p.double().cpu(), case["p2m"], owner=owner_np, depth=depth_np,
                       centres32=c32, max_resid=max_resid)
    assert torch.equal(count.cpu().long(), want["count"]) and int(want["count"].min()) > 10
    assert torch.equal(moments[..., 10].cpu(), want["moments"][..., 10]) and not bool(moments[..., 11].any())
    assert torch.equal(A, A.transpose(1, 2))
    within(A, weight * want["A"], cpu.A_BAR, "A")
    within(g, weight * want["g"], cpu.G_BAR, "g")
    for grp, what in zip(cpu.MOMENT_GROUPS, ("sum uu^T", "sum e u")):
        within(moments[..., grp], want["moments"][..., grp], cpu.M_BAR, what)
    within(moments[..., 9:10], want["moments"][..., 9:10], 1e-13, "sum e^2 over the rows")      # (the same terms: only the order)
    exact = exact_cost(obs.cpu().numpy(), depth_np, weight, max_resid)
    print("cost %s, exactly rounded %s" % (cost.tolist(), exact.tolist()))
    assert torch.equal(cost.cpu(), exact)
    return (A, g, cost, count, moments, depth, owner), want


@pytest.mark.parametrize("name,rows,views,weight,max_resid", cpu.EVALUATIONS)
def test_normal_equations(cases, name, rows, views, weight, max_resid):
    """depth and owner bit-equal to the numpy rule on the entry's own centres; count and the per-sphere counts exact; A
    bit-symmetric; A, g and the moments within 4 x the fp32 bars of weight x the fp64 restatement given the kernel's maps;
    cost bit-equal to weight x the exactly rounded sum (math.fsum) of the clipped squares."""
    case = cases[name]
    p, obs, view = inputs(case, slice(0, rows), slice(*views))
    check_equations(case, p, obs, view, weight, max_resid)


def test_synthetic_table(mesh):
    """The 7-sphere table (a bone named twice, two identical spheres, a radius of 0): the twin and the radius-0 sphere never
    own a pixel and have no moments; everything else as for the hand."""
    from spherehand_amd import ops
    probe = on_device(sref.synthetic_case(mesh))
    d = probe["dev"]
    kp, _ = ops.pose_keypoints_jacobian(d["params0"], d["offset"], d["offset_inv"], d["bone"], d["wv"], True)
    case = on_device(sref.synthetic_case(mesh, kp.cpu().numpy()))
    d = case["dev"]
    (A, g, cost, count, moments, depth, owner), _ = check_equations(case, d["params0"], d["observed"], d["view"], 1.0, float("inf"),
                                                                    case["centres32"])
    owner = owner.cpu().numpy()
    assert (owner == sref.SYN_TWIN_OF).any() and not (owner == sref.SYN_TWIN).any() and not (owner == sref.SYN_ZERO).any()
    assert not bool(moments[:, sref.SYN_TWIN].any()) and not bool(moments[:, sref.SYN_ZERO].any())


@pytest.mark.parametrize("S", (32, 64))
def test_render_is_the_rasterizer(cases, S):
    """On the rasterizer's grid (a power-of-two S, p2m = (300 / S, -150, 300 / S, -150), background 100) depth equals
    ops.sphere_raster_fwd's in every bit on the same records, and owner equals its argmin with 255 as -1."""
    from spherehand_amd import ops
    case = cases["right"]
    p, _, view = inputs(case)
    B, V = view.shape[:2]
    obs = torch.full((B, V, S, S), rref.BACKGROUND, device="cuda")
    out = evaluate(case, p, obs, view, p2m=ref.grid(S, S))
    c32, _ = kernel_centres(case, p, view)
    spheres = torch.from_numpy(np.concatenate([c32, np.broadcast_to(case["model"].radii[None, None, :, None], c32.shape[:3] + (1,))],
                                              -1).astype(np.float32)).cuda().view(B * V, -1, 4).contiguous()
    depth, argmin = ops.sphere_raster_fwd(spheres, S, S, want_argmin=True)
    assert torch.equal(bits(out[5].view(B * V, S, S)), bits(depth))
    want_owner = torch.where(argmin == 255, torch.full_like(argmin, 0, dtype=torch.int32) - 1, argmin.int())
    assert torch.equal(out[6].view(B * V, S, S), want_owner)
    assert int((want_owner >= 0).sum()) > 50 * B * V / (1 if S == 64 else 4)


def test_g_is_the_autograd_gradient_of_the_first_order_path(cases):
    """g = the gradient of 1/2 weight sum (D - O')^2 by autograd through ops.PoseSpheres -> the view transform (torch,
    shr_view_vertices_fwd's association) -> ops.SphereDepthRaster, with no saturated pixel (max_resid = inf): the two paths
    hold the same owner and the same silhouette fixed."""
    from spherehand_amd import ops
    case = cases["right"]
    d = case["dev"]
    p, obs, view = inputs(case)
    w = 0.25
    A, g, cost, count, moments, depth, owner = evaluate(case, p, obs, view, w)
    q = p.clone().requires_grad_(True)
    sph = ops.PoseSpheres.apply(q, d["offset"], d["offset_inv"], d["bone"], d["wv"], d["radii"], d["bone_start"], d["bone_points"],
                                case["model"].right_hand)
    x, y, z = (sph[:, None, :, k] for k in range(3))
    M = view[:, :, None]
    cv = [((M[..., r, 0] * x + M[..., r, 1] * y) + M[..., r, 2] * z) + M[..., r, 3] for r in range(3)]
    B, V, H, W = obs.shape
    spheres = torch.stack(cv + [sph[:, None, :, 3].expand(B, V, -1)], -1).reshape(B * V, -1, 4)
    D = ops.SphereDepthRaster.apply(spheres, H, W).view(B, V, H, W)
    target = torch.where(obs < ref.FG_MAX, obs, torch.full_like(obs, rref.BACKGROUND))
    assert torch.equal(bits(D.detach()), bits(depth))
    loss = 0.5 * w * ((D.double() - target.double()) ** 2).sum()
    loss.backward()
    assert torch.allclose(2 * loss.detach(), cost.sum(), rtol=1e-12)
    within(g, q.grad.double().cpu(), AUTOGRAD_BAR, "g against autograd through ops.SphereDepthRaster")


def test_accumulate(cases):
    """accumulate = 1 on top of shr_sphere_icp_normal's output: A, g and cost are that output plus the accumulate = 0 result,
    one fp64 rounding each (bit-equal to the sum formed in torch); A stays bit-symmetric; count and moments are the term's
    own.  weight = 0 with accumulate = 1 leaves A, g and cost bit-identical and still returns the term's count and moments."""
    case = cases["left"]
    p, obs, view = inputs(case)
    base = d2m(case, p, obs, view)
    alone = evaluate(case, p, obs, view, 0.25, 10.0)
    into = tuple(t.clone() for t in base[:3])
    both = evaluate(case, p, obs, view, 0.25, 10.0, into)
    for k in range(3):
        assert both[k].data_ptr() == into[k].data_ptr()
        assert torch.equal(bits(both[k]), bits(base[k] + alone[k])), k
    assert torch.equal(both[0], both[0].transpose(1, 2))
    for k in (3, 4, 5, 6):
        assert torch.equal(both[k], alone[k]), k
    assert bool((alone[3] > 100).all()) and bool((alone[1].abs().amax(1) > 0).all())
    into = tuple(t.clone() for t in base[:3])
    none = evaluate(case, p, obs, view, 0.0, 10.0, into)
    for k in range(3):
        assert torch.equal(bits(none[k]), bits(base[k])), k
    assert torch.equal(none[3], alone[3]) and torch.equal(none[4], alone[4])
    zero = evaluate(case, p, obs, view, 0.0, 10.0)
    assert not bool(zero[0].any()) and not bool(zero[1].any()) and not bool(zero[2].any()) and torch.equal(zero[3], alone[3])


def test_two_identical_views_double(cases):
    """V = 2 with identical identity views at 32 x 32: count, A, g, cost and the moments are exactly 2 x the single view's."""
    case = cases["right"]
    p, obs, _ = inputs(case, slice(0, 3), slice(0, 1))
    one = evaluate(case, p, obs, identity(3, 1), 0.5, 20.0)
    two = evaluate(case, p, obs.expand(3, 2, 32, 32).contiguous(), identity(3, 2), 0.5, 20.0)
    for a, b in zip(one[:5], two[:5]):
        assert torch.equal(2 * a, b)
    assert bool((one[3] > 30).all())


def test_views_without_an_observation(cases):
    """A view of NaNs adds nothing at all: A, g, cost, count and the moments of V = 3 are the bits of the two real views
    alone, and its depth and owner maps are still written.  An all-background view is NOT nothing for this term: where the
    model covers it, every pixel is a row with e = D - background; alone, its cost is the exactly rounded sum of
    (D - background)^2 over the covered pixels and its count their number, and in a set of views they add up."""
    case = cases["left"]
    p, obs, view = inputs(case, views=slice(1, 3))
    two = evaluate(case, p, obs, view)
    nan = torch.full_like(obs[:, :1], float("nan"))
    three = evaluate(case, p, torch.cat([obs[:, :1], nan, obs[:, 1:]], 1).contiguous(),
                     torch.cat([view[:, :1], view[:, :1], view[:, 1:]], 1).contiguous())
    for a, b in zip(two[:5], three[:5]):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(three[5][:, 1]), bits(three[5][:, 0])) and torch.equal(three[6][:, 1], three[6][:, 0])
    empty = torch.full_like(obs[:, :1], rref.BACKGROUND)
    alone = evaluate(case, p, empty, view[:, :1].contiguous())
    covered = alone[6] >= 0
    assert torch.equal(alone[3].long(), covered.sum((1, 2, 3))) and bool((alone[3] > 100).all())
    assert torch.equal(alone[2].cpu(), exact_cost(empty.cpu().numpy(), alone[5].cpu().numpy(), 1.0))
    assert bool((alone[5][~covered] == rref.BACKGROUND).all())
    with_empty = evaluate(case, p, torch.cat([obs, empty], 1).contiguous(), torch.cat([view, view[:, :1]], 1).contiguous())
    assert torch.equal(with_empty[3], two[3] + alone[3])
    assert torch.allclose(with_empty[2], two[2] + alone[2], rtol=1e-14) and torch.allclose(with_empty[0], two[0] + alone[0], rtol=1e-12)


def test_max_resid(cases):
    """max_resid = 3 mm: A, g, count and the moments are the bits of the call on an observation without the saturated
    pixels (NaN there: no term, no row), the cost max_resid^2 weight per saturated pixel more."""
    case = cases["left"]
    p, obs, view = inputs(case, views=slice(1, 3))
    w = 0.5
    full = evaluate(case, p, obs, view, w)
    near = evaluate(case, p, obs, view, w, 3.0)
    target = torch.where(obs < ref.FG_MAX, obs, torch.full_like(obs, rref.BACKGROUND))
    saturated = (near[5].double() - target.double()).abs() >= 3.0
    assert int(saturated.sum()) > 100 and bool((near[3] < full[3]).all()) and bool((near[3] > 30).all())
    pruned = evaluate(case, p, torch.where(saturated, torch.full_like(obs, float("nan")), obs), view, w, 3.0)
    for k in (0, 1, 3, 4):
        assert torch.equal(bits(near[k]), bits(pruned[k])), k
    assert torch.allclose(near[2] - pruned[2], 9.0 * w * saturated.sum((1, 2, 3)).double(), rtol=1e-12)


def test_blind_case(mesh):
    """sphere_render_icp_ref.blind_case on the kernel's own centres: no observed point is sphere BLIND's, so the
    data-to-model term gives the parameters that move BLIND alone a gradient of exactly 0 (and BLIND no moment); the render
    term gives BLIND rows and those parameters a gradient that is not 0."""
    probe = on_device(dict(rref.blind_case(mesh), stiffness=torch.ones(26, dtype=torch.float64)))
    c32, _ = kernel_centres(probe, probe["dev"]["params0"], probe["dev"]["view"])
    case = on_device(dict(rref.blind_case(mesh, c32), stiffness=torch.ones(26, dtype=torch.float64)))
    d = case["dev"]
    p, obs, view = d["params0"], d["observed"], d["view"]
    private = case["private"].cuda()
    base = d2m(case, p, obs, view)
    out = evaluate(case, p, obs, view)
    print("private parameters %s: d2m g %s, render g %s; BLIND's render rows %s"
          % (private.tolist(), base[1][:, private].tolist(), out[1][:, private].tolist(), out[4][:, rref.BLIND, 10].tolist()))
    assert len(private) >= 2 and bool((base[3] > 10).all())
    assert not bool(base[4][:, rref.BLIND].any()) and not bool(base[1][:, private].any())
    assert bool((out[4][:, rref.BLIND, 10] >= 1).all()) and bool((out[1][:, private].abs().amax(1) > 1.0).all())


def solve(case, rows=slice(None), views=slice(None), iters=None, observed=None, weight=cpu.WEIGHT, max_resid=cpu.MAX_RESID,
          view=None):
    from spherehand_amd import ops
    d = case["dev"]
    obs = d["observed"][rows, views].contiguous() if observed is None else observed
    view = d["view"][rows, views].contiguous() if view is None else view
    return ops.sphere_icp_render(obs, view, d["params0"][rows].contiguous(), *tables(case),
                                 case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST,
                                 case["iters"] if iters is None else iters, 1e-3, d["stiffness"], None, weight, max_resid,
                                 rref.BACKGROUND)


def test_render_weight_zero_is_sphere_icp(cases):
    from spherehand_amd import ops
    case = cases["left"]
    d = case["dev"]
    want = ops.sphere_icp(d["observed"], d["view"], d["params0"], *tables(case), case["model"].right_hand, case["p2m"], ref.FG_MAX,
                          ref.MAX_DIST, 3, 1e-3, d["stiffness"], None)
    for a, b in zip(solve(case, iters=3, weight=0.0), want):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(solve(case, iters=3)[0], want[0])


def test_no_iterations_and_empty_batch(cases):
    case = cases["right"]
    d = case["dev"]
    q, c0, c = solve(case, iters=0)
    assert torch.equal(q, d["params0"]) and torch.equal(c, c0) and bool((c0 > 0).all())
    p, obs, view = inputs(case)
    into = tuple(t.clone() for t in d2m(case, p, obs, view)[:3])
    assert torch.equal(c0, evaluate(case, p, obs, view, cpu.WEIGHT, cpu.MAX_RESID, into)[2].float())
    q, c0, c = solve(case, slice(0, 0))
    assert q.shape == (0, 26) and c0.shape == (0,) and c.shape == (0,)
    out = evaluate(case, *inputs(case, slice(0, 0)))
    assert out[0].shape == (0, 26, 26) and out[3].shape == (0,) and out[4].shape == (0, 41, 12) and out[6].shape == (0, 3, 32, 32)


def test_reproducible_and_independent_of_the_batch(cases):
    """Twice the same bits; sample i of a batch equals the batch of sample i alone, for the equations and for the whole
    solve (two tiles per view, three views)."""
    case = cases["left"]
    p, obs, view = inputs(case)
    one, two = (evaluate(case, p, obs, view, 0.25, 10.0) for _ in range(2))
    for a, b in zip(one, two):
        assert torch.equal(bits(a), bits(b))
    s1, s2 = solve(case, iters=3), solve(case, iters=3)
    for a, b in zip(s1, s2):
        assert torch.equal(bits(a), bits(b))
    for i in (1, 4):
        rows = slice(i, i + 1)
        alone = evaluate(case, *inputs(case, rows), 0.25, 10.0)
        for a, b in zip(one, alone):
            assert torch.equal(bits(a[rows]), bits(b)), i
        for a, b in zip(s1, solve(case, rows, iters=3)):
            assert torch.equal(bits(a[rows]), bits(b)), i


def test_solve_in_a_graph(cases):
    """The whole combined solve (V = 3) captured into one torch.cuda.graph on a single stream and replayed on other
    observations equals the eager result bit for bit: nothing in the loop returns to the host."""
    case = cases["right"]
    d = case["dev"]
    static_obs = d["observed"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        solve(case, observed=static_obs, iters=4)                  # warm-up: the library and the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = solve(case, observed=static_obs, iters=4)
    other = torch.roll(d["observed"], 1, 0).contiguous()           # every sample gets another sample's observations
    static_obs.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = solve(case, observed=other, iters=4)
    for a, b in zip(out, eager):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(eager[0], solve(case, iters=4)[0])


def test_module(mesh, cases):
    """render.SphereRenderPoseFitter is the ops with the hand's tables: solve and normal_equations (the two terms' sum)
    bit for bit, with views and, for [B,H,W], with the identity view; render_weight = 0 is
    SpherePoseFitter."""
    from spherehand_amd.render import SpherePoseFitter, SphereRenderPoseFitter
    case = cases["left"]
    d = case["dev"]
    kw = dict(right_hand=case["model"].right_hand, iters=2, stiffness=case["stiffness"].numpy())
    fit = SphereRenderPoseFitter(mesh, case["W"], case["H"], **kw).cuda()
    p, obs, view = inputs(case)
    for a, b in zip(fit.solve(obs, p, view), solve(case, iters=2)):
        assert torch.equal(bits(a), bits(b))
    into = tuple(t.clone() for t in d2m(case, p, obs, view)[:3])
    for a, b in zip(fit.normal_equations(obs, p, view), evaluate(case, p, obs, view, cpu.WEIGHT, cpu.MAX_RESID, into)[:5]):
        assert torch.equal(bits(a), bits(b))
    single = obs[:, 0].contiguous()
    for a, b in zip(fit.solve(single, p), solve(case, iters=2, observed=single[:, None].contiguous(), view=identity(5, 1))):
        assert torch.equal(bits(a), bits(b))
    off = SphereRenderPoseFitter(mesh, case["W"], case["H"], render_weight=0.0, **kw).cuda()
    for a, b in zip(off.solve(obs, p, view), SpherePoseFitter(mesh, case["W"], case["H"], **kw).cuda().solve(obs, p, view)):
        assert torch.equal(bits(a), bits(b))


def test_end_to_end(cases):
    """The right hand at 48 x 40, seed 21, sphere-rendered, starts p* + N(0, 0.1 rad / 2 mm), STIFFNESS, one view, the
    module's default render_weight and max_resid, END_TO_END_ITERS iterations.  cost <= cost0 on every sample, exact.  cost0
    within 4 x the fp32 bar of the fp64 restatement's.  The pose is within 4 x the fp32 bar of the fp64 restatement's on the
    samples whose accept sequence the fp32 CPU run reproduces; at most one of five may be left out."""
    case = cases["end_to_end"]
    q, c0, c = solve(case, iters=cpu.END_TO_END_ITERS)
    assert bool((c <= c0).all()) and bool(torch.isfinite(q).all())
    run = cpu.end_to_end_runs(case)
    q64, c064, c64, lm64 = run[torch.float64]
    lm32 = run[torch.float32][3]
    same = (torch.stack(lm64.history) == torch.stack(lm32.history)).all(0)
    err = (q.cpu().double() - q64).abs().max(1).values
    print("last fp64 step %s, fp32 reproduces the sequence %s; |pose - restatement| %s; cost %s against %s"
          % (lm64.last_step.tolist(), same.tolist(), err.tolist(), c.tolist(), c64.tolist()))
    assert torch.allclose(c0.cpu().double(), c064, rtol=cpu.COST_BAR + 2.0 ** -23)       # (cost0 leaves the loop as fp32)
    assert int(same.sum()) >= 4
    assert bool((err[same] <= cpu.POSE_BAR).all()), (err, cpu.POSE_BAR)
    e = sref.keypoint_error(case["model"], q.cpu(), case["p_star"]).mean().item()
    print("mean keypoint error %.4g mm (the restatement's %.4g)" % (e, sref.keypoint_error(case["model"], q64, case["p_star"]).mean().item()))
