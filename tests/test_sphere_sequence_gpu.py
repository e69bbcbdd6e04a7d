"""The sequence fit of the sphere model on the GPU (ops.sphere_temporal_normal / pose_lm_seq_step / sphere_icp_sequence,
render.SphereSequencePoseFitter): the temporal entry against the numpy chain in the header's order GIVEN its own fp32
centres and Jacobian and against the fp64 restatement (tests/sphere_sequence_ref.py) at the fp32 bars
tests/test_sphere_sequence_cpu.py measures on the same inputs; the edge rules on centres handed to the C ABI directly; the
sequence step against shr_pose_lm_step bit for bit at T = 1 and against the restated block solve; and the loop.

Shapes: S in {0, 1, 2, 3} sequences of T in {1, 2, 3, 8} frames (B <= 24) at 32 x 32, one view, the hand's 41 spheres and
pose_ik_ref.synthetic_table's 7 points."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_collision_ref as cref
import sphere_prior_ref as pref
import sphere_render_icp_ref as rref
import sphere_sequence_ref as qref
import test_sphere_sequence_cpu as cpu
from test_sphere_icp_gpu import tables, within
from test_sphere_prior_gpu import on_device
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu
INF = float("inf")
_DEV = {}


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def device_case(mesh, S, T, table="hand"):
    """sphere_sequence_ref.sequence_case with its tables on the device (`dev`), once per process."""
    key = (S, T, table)
    if key not in _DEV:
        case = on_device(qref.sequence_case(mesh, S, T, table))
        tab = case["table"]
        case["dev"]["pairs"] = None if tab is None else tuple(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in tab)
        _DEV[key] = case
    return _DEV[key]


def dev32(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def temporal(case, p, T, w=1.0, cap=INF, fw=None, into=None):
    """(A, g, E, cost, count) of the entry at poses p [B,26]."""
    from spherehand_amd import ops
    return ops.sphere_temporal_normal(p, *tables(case)[:4], T, case["model"].right_hand, w, cap, dev32(fw), into)


def own_inputs(case, p):
    """(centres [B,J,4], jac [B,3J,26]) numpy fp32: what the entry is handed."""
    from spherehand_amd import ops
    kp, jac = ops.pose_keypoints_jacobian(p, *tables(case)[:4], case["model"].right_hand)
    return kp.cpu().numpy(), jac.cpu().numpy()


def raw(centres, jac, T, w=1.0, cap=INF, fw=None, into=None):
    """The C entry on centres [B,J,4] and jac [B,3J,26] (numpy fp32) of the test's own making: (A, g, E, cost, count)."""
    from spherehand_amd import _lib
    c, j, f = dev32(centres), dev32(jac), dev32(fw)
    B, J = c.shape[:2]
    assert tuple(c.shape) == (B, J, 4) and tuple(j.shape) == (B, 3 * J, 26)
    if into is None:
        A, g, cost = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, 26, 26), (B, 26), (B,)))
    else:
        A, g, cost = into
    E = torch.full((B, 26, 26), float("nan"), dtype=torch.float64, device="cuda")
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = _lib.lib().shr_sphere_temporal_normal(ptr(c), ptr(j), ptr(f), float(w), float(cap), B, T, J, int(into is not None), ptr(A),
                                               ptr(g), ptr(E), ptr(cost), ptr(count), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return A, g, E, cost, count


def against_chain(out, centres, jac, T, w, cap, fw):
    """The entry's outputs against the numpy chain given the same inputs: count exact, the cost bit for bit, A bit-symmetric,
    E of a last frame exactly +0, A, g and E to the order bar."""
    A, g, E, cost, count = out
    cA, cg, cE, ccost, ccount = qref.chain(centres, jac, T, w, cap, fw)
    assert np.array_equal(count.cpu().numpy(), ccount), (count.tolist(), ccount.tolist())
    assert np.array_equal(cost.cpu().numpy().view(np.int64), ccost.view(np.int64)), (cost.tolist(), ccost.tolist())
    assert torch.equal(A, A.transpose(1, 2))
    last = torch.arange(A.shape[0]) % T == T - 1
    assert not bool(bits(E[last.cuda()]).any())                                  # exactly +0
    for got, want, what in ((A, cA, "A"), (g, cg, "g"), (E, cE, "E")):
        want = torch.as_tensor(want)
        scale = want.abs().flatten(1).amax(1)
        err = (got.cpu() - want).abs().flatten(1).amax(1)
        print("%s against the numpy chain: %.3g of the largest entry (bar %.3g); bit-equal: %s"
              % (what, (err / scale.clamp(min=1e-300)).max().item(), cpu.ORDER_BAR, torch.equal(bits(got.cpu()), bits(want))))
        assert bool((err <= cpu.ORDER_BAR * scale).all()), what
    return ccount


@pytest.mark.parametrize("S,T,table,w,cap,fw_on", cpu.EVALUATIONS)
def test_normal_equations(mesh, S, T, table, w, cap, fw_on):
    """Given the entry's own fp32 centres and Jacobian: count exact, cost bit-equal to the numpy chain in the header's order,
    A bit-symmetric, E of every last frame exactly +0, A, g and E within 1e-13 of the chain and so within 4 x the fp32 bars of
    the restatement given the entry's own Jacobian.  The same against the chain formed on the fp64 chain's Jacobian is
    printed, not asserted: that difference is the Jacobian's, shr_pose_keypoints_jacobian's own fp32 arithmetic, which
    tests/test_pose_ik_gpu.py holds to its own bar (first GPU run: A 1.06e-6, E 1.0e-6 of the largest entry at worst, 4.0 and
    5.1 x the CPU fp32 chain's deviation)."""
    case = device_case(mesh, S, T, table)
    p = case["dev"]["params0"]
    fw = cpu.frame_weights(S * T, T, fw_on)
    out = temporal(case, p, T, w, cap, fw)
    centres, jac = own_inputs(case, p)
    count = against_chain(out, centres, jac, T, w, cap, fw)
    print("spheres with rows %s" % count.tolist())
    if T == 1:
        assert not any(bool(t.any()) for t in out)
        return
    assert int(count.sum()) > 0
    own = [torch.as_tensor(t) for t in qref.chain(centres, jac, T, w, cap, fw)[:3]]
    other = [torch.as_tensor(t) for t in qref.chain(centres, case["model"].chain.jacobian(p.double().cpu())[1].numpy(), T, w, cap, fw)[:3]]
    for got, want, far, bar, what in zip(out[:3], own, other, (cpu.A_BAR, cpu.G_BAR, cpu.E_BAR), "AgE"):
        live = want.abs().flatten(1).amax(1) > 0
        within(got[live.cuda()], want[live], bar, what + " against the restatement given the entry's own Jacobian")
        assert not bool(got[(~live).cuda()].any())
        scale = far.abs().flatten(1).amax(1).clamp(min=1e-300)
        print("%s given the fp64 chain's Jacobian instead (pose_ik.hip's fp32 Jacobian against it; not asserted here): %.3g"
              % (what, ((got.cpu() - far).abs().flatten(1).amax(1) / scale).max().item()))


def test_accumulate_weight_zero_and_empty(mesh):
    """accumulate = 1 adds the term to what A, g and cost hold (A read in the lower triangle, written to both) and E is
    written, never accumulated; weight 0 with accumulate = 1 touches nothing, E is +0 and the counts stay; T = 1 touches
    nothing; an empty batch is a no-op."""
    case = device_case(mesh, 2, 3)
    p = case["dev"]["params0"]
    fw = cpu.frame_weights(6, 3, True)
    alone = temporal(case, p, 3, 0.5, 40.0, fw)
    gen = torch.Generator().manual_seed(2)
    R = torch.randn(6, 26, 26, generator=gen, dtype=torch.float64)
    base = ((R + R.transpose(1, 2)).cuda(), torch.randn(6, 26, generator=gen, dtype=torch.float64).cuda(),
            torch.rand(6, generator=gen, dtype=torch.float64).cuda())
    added = temporal(case, p, 3, 0.5, 40.0, fw, tuple(t.clone() for t in base))
    assert torch.equal(bits(added[0]), bits(base[0] + alone[0])) and torch.equal(bits(added[1]), bits(base[1] + alone[1]))
    assert torch.equal(bits(added[3]), bits(base[2] + alone[3])) and torch.equal(bits(added[2]), bits(alone[2]))
    assert torch.equal(added[4], alone[4]) and torch.equal(added[0], added[0].transpose(1, 2))
    upper = tuple(t.clone() for t in base)
    upper[0][:] = torch.tril(base[0]) + 7.0 * torch.triu(base[0], 1)          # only the LOWER triangle is read
    low = temporal(case, p, 3, 0.5, 40.0, fw, tuple(t.clone() for t in upper))[0]
    touched = torch.tensor([True, True, False, True, True, True]).cuda()       # (frame 2: the pair before it is cut, none after)
    assert torch.equal(bits(low[touched]), bits(added[0][touched])) and torch.equal(bits(low[~touched]), bits(upper[0][~touched]))
    for kwargs in (dict(T=3, w=0.0), dict(T=1, w=0.5)):
        into = tuple(t.clone() for t in base)
        none = temporal(case, p, kwargs["T"], kwargs["w"], 40.0, None, into)
        for i, j in ((0, 0), (1, 1), (3, 2)):
            assert torch.equal(bits(none[i]), bits(base[j])), (kwargs, i)
        assert not bool(bits(none[2]).any())
    zero = temporal(case, p, 3, 0.0, 40.0, fw)
    assert not any(bool(bits(zero[i]).any()) for i in range(4)) and torch.equal(zero[4], alone[4])
    empty = temporal(case, p[:0].contiguous(), 3)
    assert empty[0].shape == (0, 26, 26) and empty[2].shape == (0, 26, 26) and empty[4].shape == (0,)


def test_truncation_rule():
    """The kp_max rule on centres of the test's own making: a sphere moved by (3, 4, 0), exactly 5, is saturated at ts_max = 5
    and has rows at the next fp32 above; results with a saturated sphere are bit-equal to the call without it, plus its
    capped cost; a NaN centre adds nothing; +inf never saturates; e = 0 still gives rows."""
    c = np.zeros((2, 4, 4), np.float32)
    c[0, :, :3] = [(1.0, 2.0, 3.0), (0.5, 0.25, 0.0), (5.0, 5.0, 5.0), (7.0, 7.0, 7.0)]
    c[1, :, :3] = [(4.0, 6.0, 3.0), (0.5, 0.25, 0.0), (np.nan, 5.0, 5.0), (7.0, 7.5, 7.0)]
    c[..., 3] = 1.0
    up = np.nextafter(np.float32(5.0), np.float32(6.0))
    jac = np.random.default_rng(0).standard_normal((2, 12, 26)).astype(np.float32)
    rows_of = lambda idx: np.ascontiguousarray(jac.reshape(2, 4, 3, 26)[:, idx]).reshape(2, 3 * len(idx), 26)   # noqa: E731
    sat = raw(c, jac, 2, 2.0, 5.0)
    assert sat[4].tolist() == [0, 2]                                          # spheres 1 (e = 0) and 3; 0 saturated, 2 a NaN
    without = raw(np.ascontiguousarray(c[:, [1, 3]]), rows_of([1, 3]), 2, 2.0, 5.0)
    for i in (0, 1, 2):
        assert torch.equal(bits(sat[i]), bits(without[i])), i
    assert sat[3].tolist() == [0.0, without[3][1].item() + 2.0 * 25.0] and without[3][1].item() == 2.0 * 0.25
    for cap in (float(up), INF):
        rowed = raw(c, jac, 2, 2.0, cap)
        assert rowed[4].tolist() == [0, 3] and rowed[3].tolist() == [0.0, 2.0 * ((25.0 + 0.0) + 0.25)]
        no_nan = raw(np.ascontiguousarray(c[:, [0, 1, 3]]), rows_of([0, 1, 3]), 2, 2.0, cap)
        for i in range(4):
            assert torch.equal(bits(rowed[i]), bits(no_nan[i])), i
    for out in (sat, rowed):
        for got, want in zip(out, qref.chain(c, jac, 2, 2.0, 5.0 if out is sat else INF)):
            assert np.allclose(got.cpu().numpy(), want, rtol=1e-13, atol=0)
    still = raw(np.ascontiguousarray(c[:, [1]]), rows_of([1]), 2, 1.0, 5.0)      # e = 0 alone: rows, no gradient, no cost
    assert still[4].tolist() == [0, 1] and bool(still[0].any()) and bool(still[2][0].any())
    assert not bool(still[1].any()) and not bool(still[3].any())


def run_script(script, seq, with_E):
    """ref.lm_scripts' script through ops.pose_lm_step (seq False) or ops.pose_lm_seq_step with T = 1 -> per step the outputs."""
    from spherehand_amd import ops
    lam0, p0, prior, mu, steps = script
    p0 = p0.float().cuda()
    prior = None if prior is None else prior.float().cuda()
    mu = None if mu is None else mu.float().cuda()
    state, trial = ops.pose_lm_seq_begin(p0, 1, lam0) if seq else ops.pose_lm_begin(p0, lam0)
    out = []
    for A, g, cost, solve in steps:
        A, g, cost = A.cuda(), g.cuda(), cost.cuda()
        if seq:
            r = ops.pose_lm_seq_step(state, A, g, torch.zeros_like(A) if with_E else None, cost, trial, 1, prior, mu, solve)
        else:
            r = ops.pose_lm_step(state, A, g, cost, trial, prior, mu, solve)
        out.append(r)
        trial = r[0] if solve else trial
    return out


def test_T1_step_is_pose_lm_step():
    """With T = 1 (E zero, or not given) every output of shr_pose_lm_seq_step equals shr_pose_lm_step's bit for bit, on
    pose_icp_ref.lm_scripts: accepted and rejected steps, costs that are not finite, a pivot that is not positive, both
    clamps of lambda, a step without a solve."""
    for script in ref.lm_scripts():
        want = run_script(script, False, False)
        for with_E in (True, False):
            got = run_script(script, True, with_E)
            for k, (a, b) in enumerate(zip(got, want)):
                for i, (x, y) in enumerate(zip(a, b)):
                    assert (x is None) == (y is None)
                    if x is not None and (i < 3 or k == 0):             # (cost0 is written by the first step only)
                        assert torch.equal(bits(x), bits(y)), (k, i, with_E)


def seq_solve(case, T, rows=slice(None), iters=None, observed=None, keypoints=None, w=cpu.TEMPORAL_WEIGHT, cap=cpu.TS_MAX, fw=None):
    from spherehand_amd import ops
    d = case["dev"]
    obs = d["observed"][rows].contiguous() if observed is None else observed
    k = d["keypoints"][rows].contiguous() if keypoints is None else keypoints
    pairs = d["pairs"]
    return ops.sphere_icp_sequence(obs, d["view"][rows].contiguous(), d["params0"][rows].contiguous(), *tables(case), T,
                                   case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST,
                                   case["iters"] if iters is None else iters, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT,
                                   rref.DEFAULT_MAX_RESID, rref.BACKGROUND, k, d["confidence"][rows].contiguous(),
                                   pref.DEFAULT_KP_WEIGHT, pref.DEFAULT_KP_MAX, (d["lower"], d["upper"]),
                                   pref.DEFAULT_LIMIT_WEIGHT, pairs, cref.DEFAULT_COLLISION_WEIGHT if pairs else 0.0,
                                   w, cap, dev32(fw))


def test_T1_fitter_is_the_collision_fitter(mesh):
    """seq_len = 1: ops.sphere_icp_sequence is ops.sphere_icp_priors and render.SphereSequencePoseFitter is
    SphereCollisionPoseFitter, bit for bit, whatever the temporal weight; the module's solve and normal_equations are the
    ops'."""
    from spherehand_amd import ops
    from spherehand_amd.render import SphereCollisionPoseFitter, SphereSequencePoseFitter
    case = device_case(mesh, 3, 1)
    d = case["dev"]
    kw = dict(right_hand=case["model"].right_hand, iters=3, stiffness=case["stiffness"].numpy())
    parent = SphereCollisionPoseFitter(mesh, 32, 32, **kw).cuda()
    p, view, obs, k, conf = d["params0"], d["view"], d["observed"], d["keypoints"], d["confidence"]
    want = parent.solve(obs, p, view, keypoints=k, confidence=conf)
    for tw in (None, 0.0, 5.0):
        fit = SphereSequencePoseFitter(mesh, 32, 32, 1, temporal_weight=tw, **kw).cuda()
        for a, b in zip(fit.solve(obs, p, view, keypoints=k, confidence=conf), want):
            assert torch.equal(bits(a), bits(b)), tw
    for a, b in zip(seq_solve(case, 1, iters=3), want):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(want[0], p)
    case = device_case(mesh, 2, 3)
    d = case["dev"]
    p, view, obs, k, conf = d["params0"], d["view"], d["observed"], d["keypoints"], d["confidence"]
    fit = SphereSequencePoseFitter(mesh, 32, 32, 3, temporal_weight=0.5, ts_max=40.0, **kw).cuda()
    for a, b in zip(fit.solve(obs, p, view, keypoints=k, confidence=conf), seq_solve(case, 3, iters=3, w=0.5, cap=40.0)):
        assert torch.equal(bits(a), bits(b))
    into = SphereCollisionPoseFitter(mesh, 32, 32, **kw).cuda().normal_equations(obs, p, view, k, conf)[:3]
    for a, b in zip(fit.normal_equations(obs, p, view, k, conf), temporal(case, p, 3, 0.5, 40.0, None, into)):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(fit.solve(obs, p, view, keypoints=k, confidence=conf)[0],
                           SphereSequencePoseFitter(mesh, 32, 32, 3, temporal_weight=0.0, **kw).cuda().solve(
                               obs, p, view, keypoints=k, confidence=conf)[0])
    q, c0, c = seq_solve(case, 3, slice(0, 0))
    assert q.shape == (0, 26) and c0.shape == (0,) and c.shape == (0,)
    q, c0, c = seq_solve(case, 3, iters=0)
    assert torch.equal(q, p) and torch.equal(c, c0) and c0.shape == (2,) and bool((c0 > 0).all())


def test_reproducible_independent_and_identical_sequences(mesh):
    """Twice the same bits; sequence s of a batch equals the batch of sequence s alone, for the equations and the whole
    solve; two sequences of identical frames give identical results."""
    T = 3
    case = device_case(mesh, 3, T)
    p = case["dev"]["params0"]
    fw = cpu.frame_weights(9, T, True)
    one, two = (temporal(case, p, T, 0.5, 40.0, fw) for _ in range(2))
    for a, b in zip(one, two):
        assert torch.equal(bits(a), bits(b))
    s1, s2 = seq_solve(case, T, iters=3, w=0.5), seq_solve(case, T, iters=3, w=0.5)
    for a, b in zip(s1, s2):
        assert torch.equal(bits(a), bits(b))
    for s in (0, 2):
        rows = slice(s * T, s * T + T)
        for a, b in zip(one, temporal(case, p[rows].contiguous(), T, 0.5, 40.0, fw[rows])):
            assert torch.equal(bits(a[rows]), bits(b)), s
        alone = seq_solve(case, T, rows, iters=3, w=0.5)
        assert torch.equal(bits(s1[0][rows]), bits(alone[0])), s
        assert torch.equal(bits(s1[1][s:s + 1]), bits(alone[1])) and torch.equal(bits(s1[2][s:s + 1]), bits(alone[2])), s
    d = case["dev"]
    twice = torch.cat([torch.arange(T), torch.arange(T)]).cuda()
    obs, k = d["observed"][twice].contiguous(), d["keypoints"][twice].contiguous()
    from spherehand_amd import ops
    q, c0, c = ops.sphere_icp_sequence(obs, d["view"][twice].contiguous(), p[twice].contiguous(), *tables(case), T,
                                       case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST, 3, 1e-3, d["stiffness"],
                                       keypoints=k, confidence=d["confidence"][twice].contiguous(), kp_weight=0.1,
                                       temporal_weight=0.5)
    assert torch.equal(bits(q[:T]), bits(q[T:])) and c0[0] == c0[1] and c[0] == c[1] and not torch.equal(q[:T], p[:T])
    pair = temporal(case, p[twice].contiguous(), T, 0.5, 40.0)
    for t in pair:
        assert torch.equal(bits(t[:T]), bits(t[T:]))


def test_solve_in_a_graph(mesh):
    """The whole loop captured into one torch.cuda.graph on a single stream and replayed on other observations and keypoints
    equals the eager result bit for bit: nothing in the loop returns to the host."""
    T = 3
    case = device_case(mesh, 2, T)
    d = case["dev"]
    static_obs, static_k = d["observed"].clone(), d["keypoints"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        seq_solve(case, T, observed=static_obs, keypoints=static_k, iters=3, w=0.5)  # warm-up: the library, the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = seq_solve(case, T, observed=static_obs, keypoints=static_k, iters=3, w=0.5)
    other_obs, other_k = torch.roll(d["observed"], 1, 0).contiguous(), torch.roll(d["keypoints"], 1, 0).contiguous()
    static_obs.copy_(other_obs)
    static_k.copy_(other_k)
    graph.replay()
    torch.cuda.synchronize()
    eager = seq_solve(case, T, observed=other_obs, keypoints=other_k, iters=3, w=0.5)
    for a, b in zip(out, eager):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(eager[0], seq_solve(case, T, iters=3, w=0.5)[0])


def random_system(S, T, seed=7):
    """(A, g, E [B,26,26 | 26], cost [B], p0 [B,26], mu [26]) fp64 on the CPU: diagonal blocks R^T R of 60 rows (smallest eigenvalue about 7),
    off-diagonal blocks of norm about 0.5, so every sequence's system is positive definite."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    B = S * T
    R = rnd(B, 60, 26)
    A = R.transpose(1, 2) @ R
    E = 0.05 * rnd(B, 26, 26)
    E[torch.arange(B) % T == T - 1] = 0.0
    p0 = (0.3 * rnd(B, 26)).float().double()
    mu = (torch.rand(26, generator=gen, dtype=torch.float64) * 1e-3).float().double()
    return A, rnd(B, 26), E, 1.0 + torch.rand(B, generator=gen, dtype=torch.float64), p0, mu


@pytest.mark.parametrize("S,T", ((1, 2), (2, 3), (3, 8), (3, 1)))
def test_block_solve(S, T):
    """trial_out of the sequence step against the restated block solve (sphere_sequence_ref.block_solve, word for word) given
    the same fp64 equations: within the step bar of p + delta, and in fact its fp32 rounding or a neighbour.  A sequence
    with a NaN in one frame's A (a pivot that is not finite) keeps trial = p on ALL its frames and leaves the other
    sequences' bits alone; cost, cost0 and params are the sequences' own."""
    from spherehand_amd import ops
    A, g, E, cost, p0, mu = random_system(S, T)
    lam0 = 1e-3

    def step(A_):
        state, trial = ops.pose_lm_seq_begin(p0.float().cuda(), T, lam0)
        return ops.pose_lm_seq_step(state, A_.cuda(), g.cuda(), E.cuda(), cost.cuda(), trial, T, None, mu.float().cuda(), True)

    trial_out, params, c, c0 = step(A)
    assert torch.equal(params.cpu().double(), p0) and torch.equal(bits(c), bits(c0)) and c.shape == (S,)
    assert torch.allclose(c.cpu().double(), cost.view(S, T).sum(1), rtol=2.0 ** -23)        # (prior = params0: no stiffness term)
    for s in range(S):
        sl = slice(s * T, s * T + T)
        x = qref.block_solve(A[sl], g[sl], E[sl], float(np.float32(lam0)), mu, p0[sl], p0[sl], T)
        want = p0[sl] + torch.as_tensor(x)
        err = (trial_out[sl].cpu().double() - want).abs().max().item()
        y = qref.dense_solve(A[sl], g[sl], E[sl], float(np.float32(lam0)), mu, p0[sl], p0[sl], T)
        print("sequence %d: |trial_out - (p + delta)| %.3g (bar %.3g); the largest step %.3g; block against dense %.3g"
              % (s, err, cpu.STEP_BAR, np.abs(x).max(), np.abs(x - y).max()))
        assert err <= cpu.STEP_BAR
        assert bool(((trial_out[sl].cpu().double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-12).all())
        assert np.abs(x).max() > 1e-3
    bad = A.clone()
    bad[(S - 1) * T + T // 2, 5, 5] = float("nan")
    out_bad = step(bad)
    hit = slice((S - 1) * T, S * T)
    assert torch.equal(out_bad[0][hit].cpu().double(), p0[hit])                  # the whole sequence stays
    assert torch.equal(bits(out_bad[0][:(S - 1) * T]), bits(trial_out[:(S - 1) * T]))
    for i in (1, 2, 3):
        assert torch.equal(bits(out_bad[i]), bits((params, c, c0)[i - 1]))


def test_end_to_end(mesh):
    """Two sequences of eight frames at 32 x 32, one view, the module's defaults, keypoints with sigma_k = 2 mm drawn per frame:
    cost <= cost0 per sequence, and the poses within 4 x the fp32 bar of the fp64 restatement's (the CPU test holds that the
    fp32 restatement keeps both sequences' decisions)."""
    S, T, table = cpu.END_TO_END
    case = device_case(mesh, S, T, table)
    q, c0, c = seq_solve(case, T, iters=qref.END_TO_END_ITERS)
    assert c.shape == (S,) and bool((c <= c0).all()) and bool((c < c0).any()) and bool(torch.isfinite(q).all())
    q64, c064, c64, lm64 = cpu.end_to_end_run(mesh, torch.float64)
    err = (q.cpu().double() - q64).abs().view(S, -1).amax(1)
    print("|pose - restatement| %s (bar %.3g); cost0 %s against %s; cost %s against %s; decisions %s"
          % (err.tolist(), cpu.POSE_BAR, c0.tolist(), c064.tolist(), c.tolist(), c64.tolist(), [h.tolist() for h in lm64.history]))
    assert torch.allclose(c0.cpu().double(), c064, rtol=cpu.COST_BAR + 2.0 ** -23)       # (cost0 leaves the loop as fp32)
    assert bool((err <= cpu.POSE_BAR).all()), (err, cpu.POSE_BAR)
    print("mean keypoint error %.4g mm, jitter %.4g mm (the restatement's %.4g, %.4g)"
          % (qref.sref.keypoint_error(case["model"], q.cpu(), case["p_star"]).mean(), qref.jitter(case["model"], q.cpu(), case["p_star"], T).mean(),
             qref.sref.keypoint_error(case["model"], q64, case["p_star"]).mean(), qref.jitter(case["model"], q64, case["p_star"], T).mean()))
