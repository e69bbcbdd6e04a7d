"""Parameters that the frames of a group share, on the GPU.  The arrowhead step (ops.pose_lm_shared_begin /
pose_lm_shared_step) against shr_pose_lm_step bit for bit without a shared block, and against the restated Schur solve
(tests/sphere_radii_ref.py, word for word) given the same fp64 equations; the group's decision through two steps; a bad
pivot or a NaN in one frame's coupling holds its whole group and no other; a group does not depend on its batch; two steps
captured in a graph.  The radius term (ops.sphere_icp_radii_normal) against shr_sphere_icp_normal bit for bit, against the
numpy chain in the header's order given its own fp32 centres and Jacobian bit for bit, and against the fp64 restatement at
the fp32 bars tests/test_sphere_radii_cpu.py measures; the radius guard; the loop (ops.sphere_icp_calibrate,
render.SphereRadiiCalibrator) eager, in a graph, and end to end.

Shapes: G in {1, 2} groups of N in {1, 3, 4, 8} frames (B <= 8), K in {0, 1, 7, 41, 64} shared parameters; images of 32 x 32
(one tile of the scan) and 40 x 32 (a partial second tile), V in {1, 2}, the hand's 41 spheres and the synthetic table's 7."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_collision_ref as cref
import sphere_prior_ref as pref
import sphere_radii_ref as sref
import test_sphere_icp_cpu as icpu
import test_sphere_radii_cpu as cpu
from test_sphere_icp_gpu import on_device as base_on_device, tables, within
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu
INF = float("inf")


def dev(x, dtype=None):
    return None if x is None else (x if dtype is None else x.to(dtype)).cuda()


def run_script(script, shared, N=1):
    """ref.lm_scripts' script through ops.pose_lm_step (shared False) or ops.pose_lm_shared_step with K = 0 and groups of N
    frames -> per step (trial_out, params, cost, cost0)."""
    from spherehand_amd import ops
    lam0, p0, prior, mu, steps = script
    p0, prior, mu = dev(p0, torch.float32), dev(prior, torch.float32), dev(mu, torch.float32)
    if shared:
        state, trial, none = ops.pose_lm_shared_begin(p0, None, N, lam0)
        assert none is None
    else:
        state, trial = ops.pose_lm_begin(p0, lam0)
    out = []
    for A, g, cost, solve in steps:
        A, g, cost = A.cuda(), g.cuda(), cost.cuda()
        if shared:
            r = ops.pose_lm_shared_step(state, A, g, None, None, None, cost, trial, None, N, prior, mu, solve=solve)
            assert r[1] is None and r[3] is None
            r = (r[0], r[2], r[4], r[5])
        else:
            r = ops.pose_lm_step(state, A, g, cost, trial, prior, mu, solve)
        out.append(r)
        trial = r[0] if solve else trial
    return out, state


def test_K0_N1_step_is_pose_lm_step():
    """Without a shared block and with groups of one frame every output of shr_pose_lm_shared_step and the state equal
    shr_pose_lm_step's bit for bit, on pose_icp_ref.lm_scripts: accepted and rejected steps, costs that are not finite, a pivot
    that is not positive, both clamps of lambda, a step without a solve."""
    for script in ref.lm_scripts():
        want, state_w = run_script(script, False)
        got, state_g = run_script(script, True)
        assert torch.equal(bits(state_w), bits(state_g))
        for k, (a, b) in enumerate(zip(got, want)):
            for i, (x, y) in enumerate(zip(a, b)):
                assert (x is None) == (y is None)
                if x is not None and (i < 3 or k == 0):                 # (cost0 is written by the first step only)
                    assert torch.equal(bits(x), bits(y)), (k, i)


def test_K0_groups_of_three():
    """K = 0, N = 3: the frames' steps are shr_pose_lm_step's bit for bit -- a pivot that is not positive stays with its frame --
    and the decision is the GROUP's: a group whose total falls is accepted with a frame whose own cost rose, a group whose
    total rises is rejected with frames whose own cost fell."""
    from spherehand_amd import ops
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    B, N = 6, 3
    Rm = rnd(2, B, 40, 26)
    A = Rm.transpose(2, 3) @ Rm
    A[0, 4] = -torch.eye(26, dtype=torch.float64)                  # step 1, frame 4: no step
    g = rnd(2, B, 26)
    p0 = (0.3 * rnd(B, 26)).float()
    mu = (torch.rand(26, generator=gen) * 1e-3).float()
    first = torch.tensor([10.0, 10.0, 10.0, 10.0, 10.0, 10.0], dtype=torch.float64)
    group = torch.tensor([8.0, 12.5, 9.0, 11.0, 9.0, 10.5], dtype=torch.float64)      # totals 29.5 < 30 and 30.5 > 30
    twin = torch.tensor([8.0, 9.0, 9.0, 11.0, 11.0, 10.5], dtype=torch.float64)       # the same decisions, frame by frame
    state, trial, _ = ops.pose_lm_shared_begin(p0.cuda(), None, N, 1e-3)
    state1, trial1 = ops.pose_lm_begin(p0.cuda(), 1e-3)
    assert torch.equal(bits(trial), bits(trial1))
    for k, (cs, ct) in enumerate(((first, first), (group, twin))):
        got = ops.pose_lm_shared_step(state, A[k].cuda(), g[k].cuda(), None, None, None, cs.cuda(), trial, None, N, None, mu.cuda())
        want = ops.pose_lm_step(state1, A[k].cuda(), g[k].cuda(), ct.cuda(), trial1, None, mu.cuda())
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[2]), bits(want[1])), k
        assert got[4].shape == (2,) and got[1] is None and got[3] is None
        if k == 0:
            assert torch.equal(got[0][4].cpu(), p0[4]) and not torch.equal(got[0][3].cpu(), p0[3])     # frame 4 alone stays
            assert got[4].tolist() == [30.0, 30.0] and got[5].tolist() == [30.0, 30.0]
            kept = got[0].clone()
        else:
            assert torch.equal(got[2][:3], kept[:3]) and torch.equal(got[2][3:].cpu(), p0[3:])     # accepted | rejected
            assert 29.5 <= got[4][0].item() < 29.51 and got[4][1].item() == 30.0     # (the stiffness term is small)
        trial, trial1 = got[0], want[0]


def upload(sys_):
    A, g, C, R, gs, cost, p0, s0, mu, nu = sys_
    return tuple(t.cuda() for t in (A, g, C, R, gs, cost)) + tuple(t.float().cuda() for t in (p0, s0, mu, nu))


def one_step(d, N, lam0=1e-3, C=None, rows=slice(None), groups=slice(None), shape_prior=None):
    """begin and the first step on the uploaded system `d` (its frames `rows`, their groups `groups`)."""
    from spherehand_amd import ops
    A, g, C0, R, gs, cost, p0, s0, mu, nu = d
    C = C0 if C is None else C
    state, trial, trial_shape = ops.pose_lm_shared_begin(p0[rows].contiguous(), s0[groups].contiguous(), N, lam0)
    assert torch.equal(trial, p0[rows]) and torch.equal(trial_shape, s0[groups])
    return ops.pose_lm_shared_step(state, A[rows].contiguous(), g[rows].contiguous(), C[rows].contiguous(), R[groups].contiguous(),
                                   gs[groups].contiguous(), cost[rows].contiguous(), trial, trial_shape, N, None, mu, shape_prior,
                                   nu)


@pytest.mark.parametrize("G,N,K", cpu.SOLVE_CASES)
def test_schur_step(G, N, K):
    """trial_out and trial_shape_out of the step against the restated Schur solve (sphere_radii_ref.schur_solve, word for word)
    given the same fp64 equations: the fp32 rounding of p + delta and sigma + d sigma or a neighbour (TRIAL_BAR), and far
    from the step that ignores C.  A NaN in one frame's C leaves its WHOLE group at (p, sigma) and the other group's bits
    alone; a group of the batch equals the batch of that group alone; two runs give the same bits."""
    sys_ = sref.random_system(G, N, K)
    A, g, C, R, gs, cost, p0, s0, mu, nu = sys_
    d = upload(sys_)
    out = one_step(d, N)
    trial_out, shape_out, params, shape, c, c0 = out
    assert torch.equal(params, d[6]) and torch.equal(shape, d[7]) and torch.equal(bits(c), bits(c0)) and c.shape == (G,)
    assert torch.allclose(c.cpu().double(), cost.view(G, N).sum(1), rtol=2.0 ** -23)       # (the priors are the starts: no term)
    without = one_step(d, N, C=torch.zeros_like(d[2]))
    for q in range(G):
        sl = slice(q * N, q * N + N)
        x, xs = sref.schur_solve(*cpu.group_args(sys_, q, N))
        for got, want, step, other in ((trial_out[sl], p0[sl] + torch.as_tensor(x), x, without[0][sl]),
                                       (shape_out[q], s0[q] + torch.as_tensor(xs), xs, without[1][q])):
            err = (got.cpu().double() - want).abs()
            print("G %d N %d K %d, group %d: |trial - restated| %.3g; the largest step %.3g; without C the trial is off by %.3g"
                  % (G, N, K, q, err.max().item(), np.abs(step).max(), (other.cpu().double() - want).abs().max().item()))
            assert bool((err <= cpu.TRIAL_BAR_REL * want.abs() + cpu.TRIAL_BAR_ABS).all())
            assert np.abs(step).max() > 1e-3
            assert (other.cpu().double() - want).abs().max().item() > 1e3 * 2.0 ** -23 * want.abs().max().item()
    again = one_step(d, N)
    for a, b in zip(out, again):
        assert torch.equal(bits(a), bits(b))
    for q in range(G):
        alone = one_step(d, N, rows=slice(q * N, q * N + N), groups=slice(q, q + 1))
        assert torch.equal(bits(alone[0]), bits(trial_out[q * N:q * N + N])) and torch.equal(bits(alone[1]), bits(shape_out[q:q + 1]))
        assert torch.equal(bits(alone[4]), bits(c[q:q + 1]))
    bad = d[2].clone()
    hit = G - 1
    bad[hit * N + N // 2, 3, K // 2] = float("nan")
    out_bad = one_step(d, N, C=bad)
    sl = slice(hit * N, hit * N + N)
    assert torch.equal(out_bad[0][sl], d[6][sl]) and torch.equal(out_bad[1][hit], d[7][hit])       # the whole group stays
    assert torch.equal(bits(out_bad[0][:hit * N]), bits(trial_out[:hit * N])) and torch.equal(bits(out_bad[1][:hit]), bits(shape_out[:hit]))
    for i in (2, 3, 4, 5):
        assert torch.equal(bits(out_bad[i]), bits(out[i]))
    bad_A = d[0].clone()
    bad_A[hit * N, 5, 5] = float("nan")                            # a pivot that is not finite in one frame's factor
    dd = (bad_A,) + d[1:]
    out_bad = one_step(dd, N)
    assert torch.equal(out_bad[0][sl], d[6][sl]) and torch.equal(out_bad[1][hit], d[7][hit])
    assert torch.equal(bits(out_bad[0][:hit * N]), bits(trial_out[:hit * N]))


def two_steps(d, N, sprior, second, trial_io=None):
    """begin and two steps on the uploaded system; the second step's equations are `second` = (A, g, C, R, gs, cost).  ->
    the second step's outputs and the state."""
    from spherehand_amd import ops
    A, g, C, R, gs, cost, p0, s0, mu, nu = d
    state, trial, trial_shape = ops.pose_lm_shared_begin(p0, s0, N, 1e-3)
    t1 = ops.pose_lm_shared_step(state, A, g, C, R, gs, cost, trial, trial_shape, N, None, mu, sprior, nu)
    t2 = ops.pose_lm_shared_step(state, *second, t1[0], t1[1], N, None, mu, sprior, nu)
    return t1, t2, state


def test_two_steps_follow_the_restated_decisions():
    """Two steps against sphere_radii_ref.SharedLM with a shape prior and both stiffnesses: group 0's second trial is accepted,
    group 1's rejected (one of its frames has a cost of +inf), so its step is formed again from the FIRST equations kept in
    the state with lambda x 10; params, shape, cost and the second trials follow the restatement."""
    G, N, K = 2, 3, 5
    sys_ = sref.random_system(G, N, K, seed=11)
    A, g, C, R, gs, cost, p0, s0, mu, nu = sys_
    sprior = (s0 + 0.5).float().double()
    cost2 = cost * 0.5
    cost2[4] = INF
    second = (2 * A, g, 0.5 * C, R, gs, cost2)
    lm = sref.SharedLM(p0, s0, N, 1e-3)
    w1 = lm.step(A, g, C, R, gs, cost, p0, s0, None, mu, sprior, nu)
    d = upload(sys_)
    t1, t2, state = two_steps(d, N, sprior.float().cuda(), tuple(t.cuda() for t in second))
    w2 = lm.step(*second, t1[0].cpu().double(), t1[1].cpu().double(), None, mu, sprior, nu)      # (from the entry's own trial)
    assert lm.history[-1].tolist() == [True, False]
    close = lambda got, want: bool(((got.cpu().double() - want).abs()                      # noqa: E731
                                    <= cpu.TRIAL_BAR_REL * want.abs() + cpu.TRIAL_BAR_ABS).all())
    assert close(t1[0], w1[0]) and close(t1[1], w1[1])
    assert close(t2[0], w2[0]) and close(t2[1], w2[1])
    assert torch.equal(t2[2][:N], t1[0][:N]) and torch.equal(t2[2][N:], d[6][N:])          # params: accepted | rejected
    assert torch.equal(t2[3][0], t1[1][0]) and torch.equal(t2[3][1], d[7][1])              # shape likewise
    assert torch.allclose(t2[4].cpu().double(), lm.cost, rtol=2.0 ** -23) and torch.allclose(t1[5].cpu().double(), lm.cost0, rtol=2.0 ** -23)
    st = state.cpu()
    lam = torch.stack([st[q * N * ref.LM_STATE + ref.LM_LAMBDA] for q in range(G)])
    assert torch.equal(lam, lm.lam) and st[ref.LM_ACCEPTS] == 2 and st[N * ref.LM_STATE + ref.LM_REJECTS] == 1
    # the rejected group's second trial is a SHORTER step from the same point
    assert (t2[0][N:] - d[6][N:]).norm() < (t1[0][N:] - d[6][N:]).norm()


def test_two_steps_in_a_graph():
    """begin and two steps captured into one torch.cuda.graph on a single stream and replayed on other equations equal the
    eager result bit for bit: nothing in the step returns to the host."""
    G, N, K = 2, 3, 41
    d = upload(sref.random_system(G, N, K))
    other = upload(sref.random_system(G, N, K, seed=8))
    static = tuple(t.clone() for t in d)
    second = lambda s: (s[0], s[1], s[2], s[3], s[4], 0.5 * s[5])          # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        static_second = second(static)
        two_steps(static, N, None, static_second)                  # warm-up: the library, the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        t1, t2, _ = two_steps(static, N, None, static_second)
    for s, o in zip(static, other):
        s.copy_(o)
    static_second[5].copy_(0.5 * other[5])
    graph.replay()
    torch.cuda.synchronize()
    e1, e2, _ = two_steps(other, N, None, second(other))
    for a, b in zip(t1 + t2, e1 + e2):
        assert torch.equal(bits(a), bits(b))
    f1, _, _ = two_steps(d, N, None, second(d))
    assert not torch.equal(e1[0], f1[0])


# ---- the radius term ----------------------------------------------------------------------------------------------------
_DEV = {}


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def device_case(mesh, G, N, table="hand", W=32, H=32, V=1, seed=31):
    """sphere_radii_ref.radii_case with its tables on the device (`dev`), once per process."""
    key = (G, N, table, W, H, V, seed)
    if key not in _DEV:
        case = base_on_device(sref.radii_case(mesh, G, N, table, W, H, V, seed))
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
        tab = case["table"]
        case["dev"].update(keypoints=up(case["keypoints"]), confidence=up(case["confidence"]), lower=up(case["lower"]),
                           upper=up(case["upper"]), radii0=up(case["radii0"]),
                           pairs=None if tab is None else tuple(up(t) for t in tab))
        _DEV[key] = case
    return _DEV[key]


def radii_eval(case, p, radii, N, rows=slice(None)):
    """(A, g, cost, count, C, R, gs, moments, dist, owner) of the entry at poses p with the groups' radii."""
    from spherehand_amd import ops
    d = case["dev"]
    return ops.sphere_icp_radii_normal(d["observed"][rows].contiguous(), d["view"][rows].contiguous(), p, *tables(case)[:4], radii, N,
                                       case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST, want_maps=True)


def two_tables(case):
    radii = case["radii0"].copy()
    radii[-1] = (radii[-1] * np.float32(0.9)).astype(np.float32)
    return radii


@pytest.mark.parametrize("G,N,table,W,H,V", cpu.EVALUATIONS)
def test_one_group_is_the_existing_entry(mesh, G, N, table, W, H, V):
    """With ONE group and the same radii A, g, cost, count, dist, owner and moments[..., :12] are shr_sphere_icp_normal's bits."""
    from spherehand_amd import ops
    case = device_case(mesh, G, N, table, W, H, V)
    d = case["dev"]
    B = G * N
    got = radii_eval(case, d["params0"], d["radii0"][:1].contiguous(), B)
    want = ops.sphere_icp_normal(d["observed"], d["view"], d["params0"], *tables(case)[:4], d["radii0"][0].contiguous(),
                                 case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST, want_maps=True)
    for i, j in ((0, 0), (1, 1), (2, 2), (3, 3), (8, 5), (9, 6)):
        assert torch.equal(bits(got[i]), bits(want[j])), (i, j)
    assert torch.equal(bits(got[7][..., :12]), bits(want[4])) and got[7].shape == (B, case["model"].J, 16)
    assert int(got[3].min()) > 10 and got[5].shape == (1, case["model"].J, case["model"].J)


@pytest.mark.parametrize("G,N,table,W,H,V", cpu.EVALUATIONS)
def test_chains(mesh, G, N, table, W, H, V):
    """Given the entry's own fp32 centres and Jacobian, C, R, gs and the four new moments are BIT-EQUAL to the numpy chain in
    the header's order (sphere_radii_ref.radii_chain); R is exactly diagonal with integer entries, the moments' row counts
    summed over the group; a sphere without rows has exact +0 columns; C is within 4 x its fp32 bar of the fp64 restatement
    (autograd) given the entry's own owner map, gs within its bar and R exactly; two runs give the same bits."""
    from spherehand_amd import ops
    case = device_case(mesh, G, N, table, W, H, V)
    d, m = case["dev"], case["model"]
    radii = two_tables(case)
    p = d["params0"]
    out = radii_eval(case, p, torch.from_numpy(radii).cuda(), N)
    A, g, cost, count, C, R, gs, moments, dist, owner = out
    kp, jac = ops.pose_keypoints_jacobian(p, *tables(case)[:4], m.right_hand)
    c32 = ops.view_vertices(kp, d["view"]).cpu().numpy()[..., :3]
    extra, rows, Cn, Rn, gsn = sref.radii_chain(case["observed"], c32, radii, d["view"].cpu().numpy(), jac.cpu().numpy(), N, case["p2m"])
    mom = moments.cpu().numpy()
    for name, x, y in (("sum u, sum d", mom[..., 12:], extra), ("rows", mom[..., 10], rows), ("C", C.cpu().numpy(), Cn),
                       ("R", R.cpu().numpy(), Rn), ("gs", gs.cpu().numpy(), gsn)):
        same = np.array_equal(x.view(np.int64), np.ascontiguousarray(y).view(np.int64))
        print("G %d N %d %s %dx%d V %d: %s bit-equal to the numpy chain: %s (largest difference %.3g of %.3g)"
              % (G, N, table, W, H, V, name, same, np.abs(x - y).max(), np.abs(y).max()))
        assert same, name
    Rc = R.cpu()
    diag = torch.diagonal(Rc, dim1=1, dim2=2)
    assert torch.equal(diag, moments[..., 10].cpu().view(G, N, m.J).sum(1)) and torch.equal(diag, diag.round())
    assert not bool(bits(Rc - torch.diag_embed(diag)).any())                           # every off-diagonal entry an exact +0
    empty = moments[..., 10] == 0
    assert bool(empty.any()) and not bool(bits(C.transpose(1, 2)[empty]).any()) and not bool(bits(moments[..., 12:][empty]).any())
    want = sref.radii_normal(m, d["view"].double().cpu(), case["observed"], p.double().cpu(), radii, N, case["p2m"],
                             owner=owner.cpu().numpy(), dist=dist.cpu().numpy(), centres32=c32)
    within(C.flatten(1)[:, None], want["C"].flatten(1)[:, None], cpu.C_BAR, "C")
    within(A, want["A"], icpu.A_BAR, "A")
    within(g, want["g"], icpu.G_BAR, "g")
    assert torch.equal(Rc, want["R"]) and torch.equal(count.cpu().long(), want["count"])
    within(gs[:, None], want["gs"][:, None], cpu.GS_BAR, "gs")                         # (the centres' fp32 rounding in sum d)
    for a, b in zip(out, radii_eval(case, p, torch.from_numpy(radii).cuda(), N)):
        assert torch.equal(bits(a), bits(b))


def test_groups_have_their_own_radii(mesh):
    """Two groups with different radii give each group's result alone, bit for bit; a radius that is 0, negative, NaN or +inf
    makes its own group +inf / 0 and leaves the other group's bits alone."""
    for table, W, H, V in (("hand", 40, 32, 2), ("synthetic", 32, 32, 1)):
        N = 3
        case = device_case(mesh, 2, N, table, W, H, V)
        d = case["dev"]
        radii = torch.from_numpy(two_tables(case)).cuda()
        both = radii_eval(case, d["params0"], radii, N)
        for q in range(2):
            sl = slice(q * N, q * N + N)
            alone = radii_eval(case, d["params0"][sl].contiguous(), radii[q:q + 1].contiguous(), N, sl)
            for i in (0, 1, 2, 3, 4, 7, 8, 9):
                assert torch.equal(bits(alone[i]), bits(both[i][sl])), (q, i)
            assert torch.equal(bits(alone[5]), bits(both[5][q:q + 1])) and torch.equal(bits(alone[6]), bits(both[6][q:q + 1]))
        assert not torch.equal(both[8][:N], radii_eval(case, d["params0"], radii.flip(0).contiguous(), N)[8][:N])
        for value in (0.0, -1.0, float("nan"), float("inf")):
            bad = radii.clone()
            bad[1, 2] = value
            out = radii_eval(case, d["params0"], bad, N)
            assert bool((out[2][N:] == float("inf")).all())
            assert not any(bool(bits(out[i][N:]).any()) for i in (0, 1, 4)) and not bool(bits(out[5][1]).any())
            assert not bool(bits(out[6][1]).any())
            for i in (0, 1, 2, 3, 4, 7, 8, 9):
                assert torch.equal(bits(out[i][:N]), bits(both[i][:N])), (value, i)
            assert torch.equal(bits(out[5][0]), bits(both[5][0])) and torch.equal(bits(out[6][0]), bits(both[6][0]))


def calibrate(case, N, rows=slice(None), groups=slice(None), iters=None, observed=None, keypoints=None, nu=cpu.SHAPE_STIFFNESS):
    from spherehand_amd import ops
    d = case["dev"]
    obs = d["observed"][rows].contiguous() if observed is None else observed
    k = d["keypoints"][rows].contiguous() if keypoints is None else keypoints
    limits = None if d["lower"] is None else (d["lower"], d["upper"])
    J = case["model"].J
    return ops.sphere_icp_calibrate(obs, d["view"][rows].contiguous(), d["params0"][rows].contiguous(), *tables(case)[:4],
                                    d["radii0"][groups].contiguous(), N, case["model"].right_hand, case["p2m"], ref.FG_MAX,
                                    ref.MAX_DIST, case["iters"] if iters is None else iters, 1e-3, d["stiffness"], None,
                                    torch.full((J,), nu, device="cuda"), None, k, d["confidence"][rows].contiguous(),
                                    pref.DEFAULT_KP_WEIGHT, pref.DEFAULT_KP_MAX, limits,
                                    pref.DEFAULT_LIMIT_WEIGHT if limits else 0.0, d["pairs"],
                                    cref.DEFAULT_COLLISION_WEIGHT if d["pairs"] else 0.0)


def test_module(mesh):
    """render.SphereRadiiCalibrator is ops.sphere_icp_calibrate; with the radii held by a stiffness of 1e12 the fitted radii
    stay within fp32 of radii0 and, with N = 1, the poses are within the end-to-end bar of SphereCollisionPoseFitter's
    (render_weight 0) on the same frames; a group of a batch is that group alone; iters = 0 returns the starts."""
    from spherehand_amd.render import SphereCollisionPoseFitter, SphereRadiiCalibrator
    case = device_case(mesh, 2, 3)
    d = case["dev"]
    kw = dict(right_hand=case["model"].right_hand, iters=3, stiffness=case["stiffness"].numpy())
    fit = SphereRadiiCalibrator(mesh, 32, 32, 3, **kw).cuda()
    p, view, obs, k, conf = d["params0"], d["view"], d["observed"], d["keypoints"], d["confidence"]
    got = fit.solve(obs, p, view, keypoints=k, confidence=conf)
    want = calibrate(case, 3, iters=3)
    for a, b in zip(got, want):
        assert torch.equal(bits(a), bits(b))
    assert got[0].shape == (6, 26) and got[1].shape == (2, 41) and got[2].shape == (2,) and bool((got[3] < got[2]).all())
    assert (got[1] - d["radii0"]).abs().max() > 0.1
    for q in range(2):
        sl = slice(3 * q, 3 * q + 3)
        alone = calibrate(case, 3, sl, slice(q, q + 1), iters=3)
        assert torch.equal(bits(alone[0]), bits(want[0][sl])) and torch.equal(bits(alone[1]), bits(want[1][q:q + 1]))
    eq = fit.normal_equations(obs, p, view, k, conf)
    assert eq[4].shape == (6, 26, 41) and eq[5].shape == (2, 41, 41) and eq[6].shape == (2, 41)
    parent = SphereCollisionPoseFitter(mesh, 32, 32, render_weight=0.0, **kw).cuda()
    for a, b in zip(eq[:3], parent.normal_equations(obs, p, view, k, conf)[:3]):
        assert torch.equal(bits(a), bits(b))                                           # (the shipped radii: the same terms)
    q0 = calibrate(case, 3, iters=0)
    assert torch.equal(q0[0], p) and torch.equal(q0[1], d["radii0"]) and torch.equal(bits(q0[2]), bits(q0[3]))
    held = SphereRadiiCalibrator(mesh, 32, 32, 1, shape_stiffness=1e12, **kw).cuda()
    q, radii, c0, c = held.solve(obs, p, view, keypoints=k, confidence=conf)
    assert radii.shape == (6, 41) and (radii - fit.radii).abs().max().item() <= 2.0 ** -23 * 24.0      # (radii up to 24 mm)
    qp = parent.solve(obs, p, view, keypoints=k, confidence=conf)[0]
    err = (q - qp).abs().max().item()
    print("radii held by 1e12: |radii - radii0| %.3g; |pose - SphereCollisionPoseFitter's| %.3g (bar %.3g)"
          % ((radii - fit.radii).abs().max().item(), err, cpu.POSE_BAR))
    assert err <= cpu.POSE_BAR and not torch.equal(q, p)


def test_calibrate_in_a_graph(mesh):
    """The whole loop captured into one torch.cuda.graph on a single stream and replayed on other observations and keypoints
    equals the eager result bit for bit: nothing in the loop returns to the host."""
    N = 3
    case = device_case(mesh, 2, N)
    d = case["dev"]
    static_obs, static_k = d["observed"].clone(), d["keypoints"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        calibrate(case, N, observed=static_obs, keypoints=static_k, iters=3)        # warm-up: the library, the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = calibrate(case, N, observed=static_obs, keypoints=static_k, iters=3)
    other_obs, other_k = torch.roll(d["observed"], 1, 0).contiguous(), torch.roll(d["keypoints"], 1, 0).contiguous()
    static_obs.copy_(other_obs)
    static_k.copy_(other_k)
    graph.replay()
    torch.cuda.synchronize()
    eager = calibrate(case, N, observed=other_obs, keypoints=other_k, iters=3)
    for a, b in zip(out, eager):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(eager[0], calibrate(case, N, iters=3)[0])


def test_end_to_end(mesh):
    """The stable case (two groups of three frames, 32 x 32, four iterations, the module's defaults): poses and radii within
    4 x the fp32 bars of the fp64 restatement's and cost0 within its bar.  The decisions are held through the final cost: a
    step accepted on one side and rejected on the other leaves costs that differ by percent (the restatement's costs fall
    by a factor of ten in four steps), the bar on it is 1e-3."""
    G, N, table, seed = cpu.END_TO_END
    case = device_case(mesh, G, N, table, seed=seed)
    q, radii, c0, c = calibrate(case, N)
    q64, r64, c064, c64, lm = cpu.end_to_end_run(mesh, torch.float64)
    err_p, err_r = (q.cpu().double() - q64).abs().max().item(), (radii.cpu().double() - r64).abs().max().item()
    print("end to end: |pose - fp64| %.3g (bar %.3g), |radii - fp64| %.3g (bar %.3g); cost0 %s, cost %s; decisions %s"
          % (err_p, cpu.POSE_BAR, err_r, cpu.RADII_BAR, c0.tolist(), c.tolist(), [h.tolist() for h in lm.history]))
    assert bool((c < c0).all()) and bool(torch.isfinite(q).all())
    assert torch.allclose(c0.cpu().double(), c064, rtol=cpu.COST_BAR + 2.0 ** -23)
    assert torch.allclose(c.cpu().double(), c64, rtol=1e-3)
    assert err_p <= cpu.POSE_BAR and err_r <= cpu.RADII_BAR
