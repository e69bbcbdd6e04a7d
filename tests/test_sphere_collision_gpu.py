"""The collision term of the sphere fit on the GPU (ops.sphere_collision_normal / sphere_icp_priors with `collision`,
render.SphereCollisionPoseFitter): against the numpy chain in the header's order GIVEN the entry's own fp32 centres and
Jacobian -- the count exactly, the penetration and the cost bit for bit, A and g to the order of 690 fp64 terms -- against
the fp64 restatement (tests/sphere_collision_ref.py) and autograd at the fp32 bars tests/test_sphere_collision_cpu.py
measures on the same inputs, the edge rules on a synthetic table handed to the C ABI directly, and the loop.

Shapes: the hand's 41 spheres and 690 pairs, both hands, B in {0, 1, 3, 4, 5}; a synthetic table of 6 spheres with
K in {0, 1, 255, 256, 257}; the loops at 32 x 32 and 48 x 40."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_collision_ref as cref
import sphere_icp_ref as sref
import sphere_render_icp_ref as rref
import test_sphere_collision_cpu as cpu
from test_sphere_icp_gpu import tables, within
from test_sphere_prior_gpu import image_terms, on_device, prior
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


@pytest.fixture(scope="module")
def cases(mesh):
    """name -> the case of sphere_collision_ref.cached_cases with its tables on the device (`dev`)."""
    return {case["name"]: on_device(case) for case in cref.cached_cases(mesh)}


@pytest.fixture(scope="module")
def pair_tables(mesh):
    """name -> (the numpy table, the same on the device)."""
    return {name: (tab, tuple(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in tab))
            for name, tab in cref.tables(mesh).items()}


def collision(case, p, pairs, w=1.0, into=None):
    """(A, g, cost, count, penetration) of the entry at pose p [B,26]."""
    from spherehand_amd import ops
    return ops.sphere_collision_normal(p, *tables(case)[:4], case["model"].right_hand, pairs, w, into)


def own_inputs(case, p):
    """(centres [B,J,4], jac [B,3J,26]) numpy fp32: what the entry is handed."""
    from spherehand_amd import ops
    kp, jac = ops.pose_keypoints_jacobian(p, *tables(case)[:4], case["model"].right_hand)
    return kp.cpu().numpy(), jac.cpu().numpy()


def raw(centres, jac, tab, w=1.0, into=None, want_penetration=True):
    """The C entry on centres [B,J,4] and jac [B,3J,26] (numpy fp32) of the test's own making: (A, g, cost, count,
    penetration) on the device.  tab = (a, b, m) numpy, or None."""
    from spherehand_amd import _lib
    c, j = torch.from_numpy(np.ascontiguousarray(centres, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(jac, np.float32)).cuda()
    B, J = c.shape[:2]
    assert tuple(c.shape) == (B, J, 4) and tuple(j.shape) == (B, 3 * J, 26)
    K = 0 if tab is None else len(tab[0])
    dev = [None] * 3 if tab is None else [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in tab]
    if tab is not None:
        assert dev[0].dtype == dev[1].dtype == torch.int32 and dev[2].dtype == torch.float32
    if into is None:
        A, g, cost = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, 26, 26), (B, 26), (B,)))
    else:
        A, g, cost = into
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    pen = torch.full((B, max(K, 1)), float("nan"), dtype=torch.float64, device="cuda") if want_penetration else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = _lib.lib().shr_sphere_collision_normal(ptr(c), ptr(j), ptr(dev[0]) if K else None, ptr(dev[1]) if K else None,
                                                ptr(dev[2]) if K else None, float(w), B, J, K, int(into is not None), ptr(A),
                                                ptr(g), ptr(cost), ptr(count), ptr(pen) if K else None, None,
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return A, g, cost, count, (pen[:, :K] if pen is not None else None)


def against_chain(out, centres, jac, tab, w):
    """The entry's outputs against the numpy chain given the same inputs: the issue's bars."""
    A, g, cost, count, pen = out
    cA, cg, ccost, ccount, cpen = cref.chain(centres, jac, tab, w)
    assert np.array_equal(count.cpu().numpy(), ccount), (count.tolist(), ccount.tolist())
    if pen is not None:
        assert np.array_equal(pen.cpu().numpy().view(np.int64), cpen.view(np.int64))
    print("cost %s, the chain %s" % (cost.tolist(), ccost.tolist()))
    assert np.array_equal(cost.cpu().numpy().view(np.int64), ccost.view(np.int64))
    assert torch.equal(A, A.transpose(1, 2))
    gA, gg = cref.given(centres, jac, tab, w)
    for got, want, what in ((A, gA, "A"), (g, gg, "g")):
        scale = want.abs().flatten(1).amax(1)
        err = (got.cpu() - want).abs().flatten(1).amax(1)
        print("%s against the fp64 row-wise sums: %.3g of the largest entry (bar %.3g)"
              % (what, (err / scale.clamp(min=1e-300)).max().item(), cpu.ORDER_BAR))
        assert bool((err <= cpu.ORDER_BAR * scale).all()), what
    return ccount


@pytest.mark.parametrize("name,rows,tab,w", cpu.EVALUATIONS)
def test_normal_equations(cases, pair_tables, name, rows, tab, w):
    """Given the entry's own fp32 centres and Jacobian: count exact; penetration and cost bit-equal to the numpy chain in
    the header's order; A bit-symmetric; A and g within 1e-13 of the largest entry of the fp64 row-wise sums (690 terms x
    2^-53).  Against the fp64 restatement given those centres (the rows formed on the fp64 chain's Jacobian): 4 x the fp32
    bars.  At 1.0 (r_a + r_b) every sample has more than 3 pairs with rows: an empty term cannot pass."""
    case = cases[name]
    p = case["dev"]["params0"][:rows].contiguous()
    table, pairs = pair_tables[tab]
    out = collision(case, p, pairs, w)
    centres, jac = own_inputs(case, p)
    count = against_chain(out, centres, jac, table, w)
    print("pairs with rows %s" % count.tolist())
    if tab in ("1.0", "all"):
        assert int(out[3].min()) > 3
    if tab == "all":
        assert out[3].tolist() == [690] * rows
    if name == "crossed":
        assert int(out[3].min()) >= 1
    rows_ = torch.as_tensor(count)
    wantA, wantg = cref.given(centres, case["model"].chain.jacobian(p.double().cpu())[1].numpy(), table, w)
    if int(rows_.max()) > 0:
        live = rows_ > 0
        within(out[0][live], wantA[live], cpu.A_BAR, "A against the restatement")
        within(out[1][live], wantg[live], cpu.G_BAR, "g against the restatement")
    assert not bool(out[0][rows_ == 0].any()) and not bool(out[1][rows_ == 0].any())


def test_g_is_the_autograd_gradient_of_the_first_order_path(cases, pair_tables):
    """g = the gradient of 1/2 cost by autograd through ops.PoseSpheres -> the torch expression of the hinge on the pair
    table, at 1.0 (r_a + r_b): tens of active pairs per sample."""
    from spherehand_amd import ops
    case = cases["right"]
    d = case["dev"]
    p = d["params0"]
    table, pairs = pair_tables["1.0"]
    w = 0.5
    A, g, cost, count, pen = collision(case, p, pairs, w)
    q = p.clone().requires_grad_(True)
    sph = ops.PoseSpheres.apply(q, d["offset"], d["offset_inv"], d["bone"], d["wv"], d["radii"], d["bone_start"], d["bone_points"],
                                case["model"].right_hand)
    c = sph[..., :3].double()
    a, b, m = (t.long() if t.dtype == torch.int32 else t.double() for t in pairs)
    n = (c[:, a] - c[:, b]).norm(dim=-1)
    h = torch.where(n < m, m - n, torch.zeros_like(n))
    total = w * (h * h).sum(1)
    (0.5 * total.sum()).backward()
    print("cost %s against torch's %s; pairs with rows %s" % (cost.tolist(), total.tolist(), count.tolist()))
    assert torch.allclose(total.detach(), cost, rtol=1e-12) and int(count.min()) > 3
    assert torch.equal((h > 0).sum(1).int(), count)
    within(g, q.grad.double().cpu(), cpu.AUTOGRAD_BAR, "g against autograd through ops.PoseSpheres")


def synthetic(B=3, J=6, seed=0):
    """(centres [B,J,4], jac [B,3J,26]) fp32 of the test's own making: sphere 1 is sphere 0 + (3, 4, 0) exactly (a distance
    of exactly 5), sphere 2 coincides with sphere 0, the others are scattered within a few mm; a random Jacobian."""
    rng = np.random.default_rng(seed)
    c = np.zeros((B, J, 4), np.float32)
    c[..., :3] = rng.uniform(-4.0, 4.0, (B, J, 3)).astype(np.float32)
    c[:, 0, :3] = np.float32([1.0, 2.0, 3.0]) + np.arange(B, dtype=np.float32)[:, None]
    c[:, 1, :3] = c[:, 0, :3] + np.float32([3.0, 4.0, 0.0])
    c[:, 2] = c[:, 0]
    c[..., 3] = 1.0
    assert np.array_equal(c[:, 1, :3].astype(np.float64) - c[:, 0, :3].astype(np.float64), np.tile([3.0, 4.0, 0.0], (B, 1)))
    return c, rng.standard_normal((B, 3 * J, 26)).astype(np.float32)


def table_of(*triples):
    a, b, m = zip(*triples)
    return np.asarray(a, np.int32), np.asarray(b, np.int32), np.asarray(m, np.float32)


def test_kink_coincident_and_nan():
    """A distance of exactly 5 (an fp32 offset (3, 4, 0)) is inactive at m = 5 and active at the next fp32 above, with
    h = m - 5 exactly.  Coincident centres pay m^2, give no row and leave g = 0.  A NaN centre gives no term."""
    c, jac = synthetic()
    up = float(np.nextafter(np.float32(5.0), np.float32(6.0)))
    at = raw(c, jac, table_of((0, 1, 5.0)), 2.0)
    assert at[3].tolist() == [0, 0, 0] and not bool(at[0].any()) and not bool(at[1].any()) and not bool(at[2].any()) \
        and not bool(at[4].any())
    above = raw(c, jac, table_of((0, 1, up)), 2.0)
    h = np.float64(np.float32(up)) - 5.0
    assert above[3].tolist() == [1, 1, 1] and above[4][:, 0].tolist() == [h] * 3 and above[2].tolist() == [2.0 * (h * h)] * 3
    assert bool(above[1].abs().amax(1).gt(0).all())
    against_chain(above, c, jac, table_of((0, 1, up)), 2.0)
    same = raw(c, jac, table_of((0, 2, 7.0)), 0.5)
    assert same[3].tolist() == [0, 0, 0] and same[2].tolist() == [0.5 * 49.0] * 3 and same[4][:, 0].tolist() == [7.0] * 3
    assert not bool(same[0].any()) and not bool(same[1].any())
    mixed = table_of((0, 2, 7.0), (3, 4, 100.0), (0, 1, up))
    against_chain(raw(c, jac, mixed, 1.5), c, jac, mixed, 1.5)
    bad = c.copy()
    bad[1, 3, 1] = np.nan
    tab = table_of((3, 4, 100.0), (4, 5, 100.0), (5, 3, 100.0))
    out = raw(bad, jac, tab, 1.0)
    assert out[3].tolist() == [3, 1, 3] and out[4][1].tolist()[0] == 0.0 and out[4][1].tolist()[2] == 0.0
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[2]).all())
    against_chain(out, bad, jac, tab, 1.0)


def test_skipped_pairs_and_swapped_pairs():
    """A pair with an index of -1, with index J, with a == b, or with m of 0, below 0 or NaN is skipped: the result is
    bit-identical to the table without it, its penetration is 0.  (a, b) swapped is bit-identical."""
    c, jac = synthetic()
    J = c.shape[1]
    good = [(3, 4, 100.0), (0, 1, 6.0), (5, 3, 50.0), (1, 4, 80.0)]
    want = raw(c, jac, table_of(*good), 1.25)
    assert want[3].tolist() == [4, 4, 4]
    for skipped in ((-1, 2, 100.0), (2, J, 100.0), (J, 2, 100.0), (3, 3, 100.0), (0, 1, 0.0), (0, 1, -6.0), (0, 1, float("nan")),
                    (1 << 30, 0, 100.0), (0, -(1 << 31), 100.0)):
        for at in (0, 2, 4):
            tab = table_of(*(good[:at] + [skipped] + good[at:]))
            out = raw(c, jac, tab, 1.25)
            for x, y in zip(out[:4], want[:4]):
                assert torch.equal(bits(x), bits(y)), (skipped, at)
            keep = [i for i in range(len(good) + 1) if i != at]
            assert not bool(out[4][:, at].any()) and torch.equal(bits(out[4][:, keep]), bits(want[4]))
    swapped = raw(c, jac, table_of(*[(b, a, m) for a, b, m in good]), 1.25)
    for x, y in zip(swapped, want):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("K", (0, 1, 255, 256, 257))
def test_chunk_edges(K):
    """K at the edges of the 256-pair chunks: random pairs of 6 spheres a few mm apart, a third of them active, some
    skipped; everything against the numpy chain.  K = 0 with accumulate = 0 writes exact zeros."""
    c, jac = synthetic(seed=K)
    rng = np.random.default_rng(100 + K)
    a, b = rng.integers(0, 6, K).astype(np.int32), rng.integers(0, 6, K).astype(np.int32)
    m = rng.uniform(1.0, 9.0, K).astype(np.float32)
    if K > 1:
        a[K // 2] = -1
    tab = (a, b, m) if K else None
    out = raw(c, jac, tab, 0.75)
    if K == 0:
        assert out[3].tolist() == [0, 0, 0]
        for t in out[:3]:
            assert not bool(t.any()) and not bool(torch.signbit(t).any())
        return
    count = against_chain(out, c, jac, tab, 0.75)
    if K >= 255:
        assert int(count.min()) > 30 and int((cref.decide(c, tab)["active"][:, 200:].sum(1)).min()) > 3
    none = raw(c, jac, tab, 0.75, want_penetration=False)
    for x, y in zip(none[:4], out[:4]):
        assert torch.equal(bits(x), bits(y))


def test_accumulate(cases, pair_tables):
    """accumulate = 1 on top of the four other terms: A, g and cost are their sum plus the accumulate = 0 result, one fp64
    rounding each (bit-equal to the sum formed in torch); A stays bit-symmetric; count and penetration are the term's own.
    weight 0, or no table, with accumulate = 1 leaves the buffers bit-identical; with accumulate = 0 they are exact zeros
    and count and penetration are what they are at any weight."""
    case = cases["left"]
    d = case["dev"]
    p, view = d["params0"], d["view"]
    base = prior(case, p, view, d["keypoints"], d["confidence"], 0.25, 15.0, 1e4, image_terms(case, p, d["observed"], view))[:3]
    table, pairs = pair_tables["1.0"]
    alone = collision(case, p, pairs, 0.5)
    into = tuple(t.clone() for t in base)
    both = collision(case, p, pairs, 0.5, into)
    for i in range(3):
        assert both[i].data_ptr() == into[i].data_ptr()
        assert torch.equal(bits(both[i]), bits(base[i] + alone[i])), i
        assert not torch.equal(both[i], base[i])
    assert torch.equal(both[0], both[0].transpose(1, 2))
    assert torch.equal(both[3], alone[3]) and torch.equal(bits(both[4]), bits(alone[4])) and int(alone[3].min()) > 3
    for kwargs in (dict(pairs=pairs, w=0.0), dict(pairs=None, w=1.0)):
        into = tuple(t.clone() for t in base)
        none = collision(case, p, into=into, **kwargs)
        for i in range(3):
            assert torch.equal(bits(none[i]), bits(base[i])), (kwargs, i)
    zero = collision(case, p, pairs, 0.0)
    assert not bool(zero[0].any()) and not bool(zero[1].any()) and not bool(zero[2].any())
    assert torch.equal(zero[3], alone[3]) and torch.equal(bits(zero[4]), bits(alone[4]))
    assert torch.equal(collision(case, p, pairs, 0.0, tuple(t.clone() for t in base))[3], alone[3])
    empty = collision(case, p, None, 1.0)
    assert not bool(empty[0].any()) and not bool(empty[3].any()) and empty[4].shape == (5, 0)


def solve(case, rows=slice(None), iters=None, observed=None, keypoints=None, pairs=None, w=cpu.WEIGHT, **extra):
    from spherehand_amd import ops
    d = case["dev"]
    obs = d["observed"][rows].contiguous() if observed is None else observed
    k = d["keypoints"][rows].contiguous() if keypoints is None else keypoints
    return ops.sphere_icp_priors(obs, d["view"][rows].contiguous(), d["params0"][rows].contiguous(), *tables(case),
                                 case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST,
                                 case["iters"] if iters is None else iters, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT,
                                 rref.DEFAULT_MAX_RESID, rref.BACKGROUND, k, d["confidence"][rows].contiguous(), cpu.KP_WEIGHT,
                                 cpu.KP_MAX, (d["lower"], d["upper"]), cpu.LIMIT_WEIGHT,
                                 **(dict(collision=pairs, collision_weight=w) if pairs is not None else {}), **extra)


def test_no_collision_term_is_the_parent_loop(cases, pair_tables):
    """Without a weighted collision term ops.sphere_icp_priors is what it is without the two arguments, bit for bit
    (weight 0 with a table; a weight without a table), and with no prior term at all it is ops.sphere_icp_render; with the
    term the pose differs."""
    from spherehand_amd import ops
    case = cases["crossed"]
    d = case["dev"]
    _, pairs = pair_tables["6mm"]
    want = solve(case, iters=3)
    for out in (solve(case, iters=3, pairs=pairs, w=0.0), solve(case, iters=3, collision=None, collision_weight=5.0)):
        for a, b in zip(out, want):
            assert torch.equal(bits(a), bits(b))
    assert not torch.equal(solve(case, iters=3, pairs=pairs)[0], want[0])
    args = (d["observed"], d["view"], d["params0"], *tables(case), case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST,
            3, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT, rref.DEFAULT_MAX_RESID, rref.BACKGROUND)
    for a, b in zip(ops.sphere_icp_priors(*args, collision=pairs, collision_weight=0.0), ops.sphere_icp_render(*args)):
        assert torch.equal(bits(a), bits(b))


def test_no_iterations_and_empty_batch(cases, pair_tables):
    case = cases["crossed"]
    d = case["dev"]
    _, pairs = pair_tables["6mm"]
    q, c0, c = solve(case, iters=0, pairs=pairs)
    assert torch.equal(q, d["params0"]) and torch.equal(c, c0) and bool((c0 > 0).all())
    p, view = d["params0"], d["view"]
    into = prior(case, p, view, d["keypoints"], d["confidence"], cpu.KP_WEIGHT, cpu.KP_MAX, cpu.LIMIT_WEIGHT,
                 image_terms(case, p, d["observed"], view))[:3]
    assert torch.equal(c0, collision(case, p, pairs, cpu.WEIGHT, into)[2].float())
    q, c0, c = solve(case, slice(0, 0), pairs=pairs)
    assert q.shape == (0, 26) and c0.shape == (0,) and c.shape == (0,)
    out = collision(case, p[:0].contiguous(), pairs)
    assert out[0].shape == (0, 26, 26) and out[3].shape == (0,) and out[4].shape == (0, 690)


def test_reproducible_and_independent_of_the_batch(cases, pair_tables):
    """Twice the same bits; sample i of a batch equals the batch of sample i alone, for the equations and the whole solve."""
    case = cases["crossed"]
    p = case["dev"]["params0"]
    _, wide = pair_tables["1.0"]
    _, pairs = pair_tables["6mm"]
    one, two = (collision(case, p, wide, 0.5) for _ in range(2))
    for a, b in zip(one, two):
        assert torch.equal(bits(a), bits(b))
    s1, s2 = solve(case, iters=3, pairs=pairs), solve(case, iters=3, pairs=pairs)
    for a, b in zip(s1, s2):
        assert torch.equal(bits(a), bits(b))
    for i in (0, 3):
        rows = slice(i, i + 1)
        for a, b in zip(one, collision(case, p[rows].contiguous(), wide, 0.5)):
            assert torch.equal(bits(a[rows]), bits(b)), i
        for a, b in zip(s1, solve(case, rows, iters=3, pairs=pairs)):
            assert torch.equal(bits(a[rows]), bits(b)), i


def test_solve_in_a_graph(cases, pair_tables):
    """The whole loop with the term captured into one torch.cuda.graph on a single stream and replayed on other observations
    and keypoints equals the eager result bit for bit: nothing in the loop returns to the host."""
    case = cases["crossed"]
    d = case["dev"]
    _, pairs = pair_tables["6mm"]
    static_obs, static_k = d["observed"].clone(), d["keypoints"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        solve(case, observed=static_obs, keypoints=static_k, iters=4, pairs=pairs)      # warm-up: the library, the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = solve(case, observed=static_obs, keypoints=static_k, iters=4, pairs=pairs)
    other_obs, other_k = torch.roll(d["observed"], 1, 0).contiguous(), torch.roll(d["keypoints"], 1, 0).contiguous()
    static_obs.copy_(other_obs)
    static_k.copy_(other_k)
    graph.replay()
    torch.cuda.synchronize()
    eager = solve(case, observed=other_obs, keypoints=other_k, iters=4, pairs=pairs)
    for a, b in zip(out, eager):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(eager[0], solve(case, iters=4, pairs=pairs)[0])


def test_module(mesh, cases, pair_tables):
    """render.SphereCollisionPoseFitter is the ops with the hand's tables, pose_limits() and collision_table(): solve and
    normal_equations (the five terms' sum) bit for bit; collision_weight = 0 is SpherePriorPoseFitter."""
    from spherehand_amd.render import SphereCollisionPoseFitter, SpherePriorPoseFitter
    case = cases["crossed"]
    d = case["dev"]
    kw = dict(right_hand=case["model"].right_hand, iters=2, stiffness=case["stiffness"].numpy())
    fit = SphereCollisionPoseFitter(mesh, case["W"], case["H"], **kw).cuda()
    _, pairs = pair_tables["6mm"]
    for a, b in zip((fit.pair_a, fit.pair_b, fit.pair_min), pairs):
        assert torch.equal(a, b)
    p, view, obs, k, conf = d["params0"], d["view"], d["observed"], d["keypoints"], d["confidence"]
    for a, b in zip(fit.solve(obs, p, view, keypoints=k, confidence=conf), solve(case, iters=2, pairs=pairs)):
        assert torch.equal(bits(a), bits(b))
    into = prior(case, p, view, k, conf, cpu.KP_WEIGHT, cpu.KP_MAX, cpu.LIMIT_WEIGHT, image_terms(case, p, obs, view))[:3]
    for a, b in zip(fit.normal_equations(obs, p, view, k, conf), collision(case, p, pairs, cpu.WEIGHT, into)):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(fit.solve(obs[:, 0].contiguous(), p, keypoints=k[:, 0].contiguous(), confidence=conf[:, 0].contiguous()),
                    solve(case, iters=2, pairs=pairs)):
        assert torch.equal(bits(a), bits(b))                        # (the case's one view is the identity)
    off = SphereCollisionPoseFitter(mesh, case["W"], case["H"], collision_weight=0.0, **kw).cuda()
    for a, b in zip(off.solve(obs, p, view, keypoints=k, confidence=conf),
                    SpherePriorPoseFitter(mesh, case["W"], case["H"], **kw).cuda().solve(obs, p, view, keypoints=k, confidence=conf)):
        assert torch.equal(bits(a), bits(b))
    scaled = SphereCollisionPoseFitter(mesh, case["W"], case["H"], radius_scale=1.0, **kw).cuda()
    rest = torch.zeros(2, 26, device="cuda")
    assert collision(case, rest, (scaled.pair_a, scaled.pair_b, scaled.pair_min))[3].tolist() == [0, 0]   # capped at rest
    assert int(collision(case, rest, pair_tables["1.0"][1])[3].min()) > 20                     # (26 on the CPU) without the cap


def test_end_to_end(cases, pair_tables):
    """The crossed family's poses of seed sphere_collision_ref.END_TO_END_SEED at 48 x 40, one view, the module's defaults,
    keypoints with sigma_k = 2 mm, 6 iterations, B = 5.  cost <= cost0 on every sample.  The pose is within 4 x the fp32 bar
    of the fp64 restatement's on the samples where the CPU fp32 and fp64 restatements keep the same accept sequence, the
    same active pairs and the same hinge rows; at most one of five may be left out."""
    case = cases["crossed"]
    _, pairs = pair_tables["6mm"]
    assert np.array_equal(case["table"][2], pair_tables["6mm"][0][2])
    q, c0, c = solve(case, iters=cref.END_TO_END_ITERS, pairs=pairs)
    assert bool((c <= c0).all()) and bool(torch.isfinite(q).all())
    run = cpu.end_to_end_runs(case)
    q64, c064, c64, lm64 = run[torch.float64]
    same = cpu.kept(lm64, run[torch.float32][3])
    err = (q.cpu().double() - q64).abs().max(1).values
    print("the fp32 restatement keeps %s; |pose - restatement| %s (bar %.3g); cost %s against %s; active pairs at the start %s"
          % (same.tolist(), err.tolist(), cpu.POSE_BAR, c.tolist(), c64.tolist(), lm64.actives[0].sum(1).tolist()))
    assert torch.allclose(c0.cpu().double(), c064, rtol=cpu.COST_BAR + 2.0 ** -23)       # (cost0 leaves the loop as fp32)
    assert int(same.sum()) >= 4
    assert bool((err[same] <= cpu.POSE_BAR).all()), (err, cpu.POSE_BAR)
    e = sref.keypoint_error(case["model"], q.cpu(), case["p_star"]).mean().item()
    print("mean keypoint error %.4g mm (the restatement's %.4g)" % (e, sref.keypoint_error(case["model"], q64, case["p_star"]).mean().item()))
