"""The constant-velocity term and the block-pentadiagonal step on the GPU (ops.sphere_accel_normal / pose_lm_seq2_step /
sphere_icp_trajectory, render.SphereTrajectoryPoseFitter): the entry against the numpy chain in the header's order GIVEN its
own fp32 centres and Jacobian, bit for bit; the edge rules on centres handed to the C ABI directly; the step without F against
shr_pose_lm_seq_step bit for bit and with F against the restated block solve (tests/sphere_trajectory_ref.py); and the loop,
at the fp32 bars tests/test_sphere_trajectory_cpu.py measures on the same inputs.

Shapes: 2 sequences of T in {1, 2, 3, 4, 5, 8} frames (B <= 16) at 32 x 32, one view, the hand's 41 spheres and
pose_ik_ref.synthetic_table's 7 points."""
import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_collision_ref as cref
import sphere_prior_ref as pref
import sphere_render_icp_ref as rref
import sphere_sequence_ref as qref
import sphere_trajectory_ref as tref
import test_sphere_sequence_gpu as sgpu
import test_sphere_trajectory_cpu as cpu
from test_sphere_icp_gpu import tables
from test_sphere_prior_gpu import on_device
from test_sphere_render_icp_gpu import bits

pytestmark = pytest.mark.gpu
INF = float("inf")
device_case, dev32, own_inputs = sgpu.device_case, sgpu.dev32, sgpu.own_inputs


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def accel(case, p, T, w=1.0, cap=INF, fw=None, into=None, into_E=None):
    """(A, g, E, F, cost, count) of the entry at poses p [B,26]."""
    from spherehand_amd import ops
    return ops.sphere_accel_normal(p, *tables(case)[:4], T, case["model"].right_hand, w, cap, dev32(fw), into, into_E)


def raw(centres, jac, T, w=1.0, cap=INF, fw=None):
    """The C entry on centres [B,J,4] and jac [B,3J,26] (numpy fp32) of the test's own making: (A, g, E, F, cost, count)."""
    from spherehand_amd import _lib
    c, j, f = dev32(centres), dev32(jac), dev32(fw)
    B, J = c.shape[:2]
    assert tuple(c.shape) == (B, J, 4) and tuple(j.shape) == (B, 3 * J, 26) and B % T == 0
    A, g, E, F, cost = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
                        for s in ((B, 26, 26), (B, 26), (B, 26, 26), (B, 26, 26), (B,)))
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = _lib.lib().shr_sphere_accel_normal(ptr(c), ptr(j), ptr(f), float(w), float(cap), B, T, J, 0, 0, ptr(A), ptr(g), ptr(E),
                                            ptr(F), ptr(cost), ptr(count), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return A, g, E, F, cost, count


def equals_chain(out, want):
    """The entry's six outputs are the numpy chain's bit for bit (count: the same integers)."""
    for got, w, what in zip(out[:5], want[:5], ("A", "g", "E", "F", "cost")):
        w = torch.as_tensor(w)
        scale = w.abs().max().clamp(min=1e-300)
        print("%s against the numpy chain: %.3g of the largest entry; bit-equal: %s"
              % (what, ((got.cpu() - w).abs().max() / scale).item(), same_bits(got.cpu(), w)))
        assert same_bits(got.cpu(), w), what
    assert np.array_equal(out[5].cpu().numpy(), want[5]), (out[5].tolist(), want[5].tolist())


@pytest.mark.parametrize("S,T,table,w,cap,fw_on", cpu.EVALUATIONS)
def test_normal_equations(mesh, S, T, table, w, cap, fw_on):
    """Given the entry's own fp32 centres and Jacobian: count and cost exact, A, g, E and F bit-equal to the numpy chain in the
    header's order, A bit-symmetric, F of a sequence's last two frames and E of its last exactly +0; T <= 2 gives exact
    zeros.  Against the chain formed on the fp64 chain's Jacobian the deviation is printed, not asserted: that difference
    is shr_pose_keypoints_jacobian's own fp32 arithmetic, which tests/test_pose_ik_gpu.py holds to its own bar."""
    case = device_case(mesh, S, T, table)
    p = case["dev"]["params0"]
    fw = cpu.triple_weights(S * T, T, fw_on)
    out = accel(case, p, T, w, cap, fw)
    centres, jac = own_inputs(case, p)
    want = tref.chain(centres, jac, T, w, cap, fw)
    equals_chain(out, want)
    A, g, E, F, cost, count = out
    print("spheres with rows %s" % count.tolist())
    assert torch.equal(A, A.transpose(1, 2))
    t = (torch.arange(S * T) % T).cuda()
    assert not bool(bits(F[t >= T - 2]).any()) and not bool(bits(E[t == T - 1]).any())          # exactly +0
    assert not bool(count[t < 2].any()) and not bool(bits(cost[t < 2]).any())
    if T <= 2:
        assert not any(bool(bits(x).any()) for x in out[:5]) and not bool(count.any())
        return
    assert int(count.sum()) > 0 and bool(F.any()) and bool(E.any())
    if cap < INF:
        d = tref.decide(centres, T, cap, fw)
        assert int((d["valid"] & ~d["act"]).sum()) > 0 and int(d["act"].sum()) > 0
    far = tref.chain(centres, case["model"].chain.jacobian(p.double().cpu())[1].numpy(), T, w, cap, fw)
    for got, other, bar, what in zip(out[:4], far[:4], (cpu.A_BAR, cpu.G_BAR, cpu.E_BAR, cpu.F_BAR), "AgEF"):
        other = torch.as_tensor(other)
        scale = other.abs().flatten(1).amax(1).clamp(min=1e-300)
        print("%s given the fp64 chain's Jacobian instead (pose_ik.hip's fp32 Jacobian against it; not asserted here): %.3g "
              "(4 x the CPU fp32 chain's deviation: %.3g)" % (what, ((got.cpu() - other).abs().flatten(1).amax(1) / scale).max(), bar))


def test_accumulate_and_nothing_to_add(mesh):
    """accumulate = 1 equals base + the accumulate = 0 result bit for bit and reads only the LOWER triangle of A;
    accumulate_E = 1 after shr_sphere_temporal_normal equals that entry's E + this entry's bit for bit; F is written either
    way; at weight 0 or T <= 2 nothing is touched (and E with accumulate_E = 0 and F are +0); an empty batch is a no-op."""
    T = 4
    case = device_case(mesh, 2, T)
    p = case["dev"]["params0"]
    B = 2 * T
    fw = cpu.triple_weights(B, T, True)                            # the triple centred at frame 2 is cut
    alone = accel(case, p, T, 0.5, 30.0, fw)
    gen = torch.Generator().manual_seed(2)
    R = torch.randn(B, 26, 26, generator=gen, dtype=torch.float64)
    base = ((R + R.transpose(1, 2)).cuda(), torch.randn(B, 26, generator=gen, dtype=torch.float64).cuda(),
            torch.rand(B, generator=gen, dtype=torch.float64).cuda())
    clone = lambda ts: tuple(t.clone() for t in ts)                # noqa: E731
    added = accel(case, p, T, 0.5, 30.0, fw, clone(base))
    assert same_bits(added[0], base[0] + alone[0]) and same_bits(added[1], base[1] + alone[1])
    assert same_bits(added[4], base[2] + alone[4]) and same_bits(added[2], alone[2]) and same_bits(added[3], alone[3])
    assert torch.equal(added[5], alone[5]) and torch.equal(added[0], added[0].transpose(1, 2))
    upper = clone(base)
    upper[0][:] = torch.tril(base[0]) + 7.0 * torch.triu(base[0], 1)          # only the LOWER triangle is read
    low = accel(case, p, T, 0.5, 30.0, fw, clone(upper))[0]
    # sequence 0 has the triple centred at frame 1 alone (frames 0, 1, 2); its frame 3 and nothing else is without a triple
    touched = torch.tensor([True, True, True, False] + [True] * T).cuda()
    assert same_bits(low[touched], added[0][touched]) and same_bits(low[~touched], upper[0][~touched])
    # E on top of the first-difference entry's
    first = sgpu.temporal(case, p, T, 0.3, 40.0)
    both = accel(case, p, T, 0.5, 30.0, fw, (first[0].clone(), first[1].clone(), first[3].clone()), first[2].clone())
    assert same_bits(both[2], first[2] + alone[2]) and same_bits(both[0], first[0] + alone[0]) and same_bits(both[3], alone[3])
    assert bool(first[2].any()) and bool(alone[2].any())
    base_E = torch.randn(B, 26, 26, generator=gen, dtype=torch.float64).cuda()
    full = accel(case, p, T, 0.5, 30.0)[5]
    assert int(full[3]) > 0 and int(alone[5][3]) == 0              # the cut triple has no rows
    for kwargs in (dict(T=T, w=0.0), dict(T=2, w=0.5), dict(T=1, w=0.5)):
        none = accel(case, p, kwargs["T"], kwargs["w"], 30.0, None, clone(base), base_E.clone())
        for i, want in ((0, base[0]), (1, base[1]), (4, base[2]), (2, base_E)):
            assert same_bits(none[i], want), (kwargs, i)
        assert not bool(bits(none[3]).any())
        written = accel(case, p, kwargs["T"], kwargs["w"], 30.0)
        assert not any(bool(bits(written[i]).any()) for i in range(5))
        assert torch.equal(written[5], full if kwargs["T"] == T else torch.zeros_like(full))      # whatever the weight
    empty = accel(case, p[:0].contiguous(), 3)
    assert empty[0].shape == (0, 26, 26) and empty[3].shape == (0, 26, 26) and empty[5].shape == (0,)


def test_truncation_rule():
    """The cap rule on centres of the test's own making (test_sphere_trajectory_cpu.truncation_inputs): a second difference
    of (3, 4, 0), exactly 5, is saturated at acc_max = 5 and has rows at the next fp32 above; results with a saturated
    sphere are bit-equal to the call without it, plus its capped cost; a NaN centre adds nothing; +inf never saturates;
    a = 0 still gives rows."""
    c, jac = cpu.truncation_inputs()
    up = np.nextafter(np.float32(5.0), np.float32(6.0))
    pick = lambda idx: (np.ascontiguousarray(c[:, idx]),                                  # noqa: E731
                        np.ascontiguousarray(jac.reshape(3, 4, 3, 26)[:, idx]).reshape(3, 3 * len(idx), 26))
    sat = raw(c, jac, 3, 2.0, 5.0)
    assert sat[5].tolist() == [0, 0, 2]                                       # spheres 1 (a = 0) and 3; 0 saturated, 2 a NaN
    without = raw(*pick([1, 3]), 3, 2.0, 5.0)
    for i in range(4):
        assert same_bits(sat[i], without[i]), i
    assert sat[4].tolist() == [0.0, 0.0, without[4][2].item() + 2.0 * 25.0] and without[4][2].item() == 2.0 * 0.25
    equals_chain(sat, tref.chain(c, jac, 3, 2.0, 5.0))
    for cap in (float(up), INF):
        rowed = raw(c, jac, 3, 2.0, cap)
        assert rowed[5].tolist() == [0, 0, 3] and rowed[4].tolist() == [0.0, 0.0, 2.0 * ((25.0 + 0.0) + 0.25)]
        no_nan = raw(*pick([0, 1, 3]), 3, 2.0, cap)
        for i in range(5):
            assert same_bits(rowed[i], no_nan[i]), i
        equals_chain(rowed, tref.chain(c, jac, 3, 2.0, cap))
    still = raw(*pick([1]), 3, 1.0, 5.0)                                      # a = 0 alone: rows, no gradient, no cost
    assert still[5].tolist() == [0, 0, 1] and bool(still[0].any()) and bool(still[2][0].any()) and bool(still[3][0].any())
    assert not bool(still[1].any()) and not bool(still[4].any())


def sequence_script(script, T, seed=3):
    """pose_icp_ref.lm_scripts' script with every crop made a sequence of T frames: the crop's A, g, pose and prior in each of
    its frames, its cost in the first and 0 in the others (a cost that is not finite stays so, the gaps stay), and small
    off-diagonal blocks E, zero at a sequence's last frame."""
    lam0, p0, prior, mu, steps = script
    gen = torch.Generator().manual_seed(seed)
    rep = lambda x: None if x is None else x.repeat_interleave(T, 0).contiguous()   # noqa: E731
    B = p0.shape[0] * T
    head = (torch.arange(B) % T == 0).double()
    out = []
    for A, g, cost, solve in steps:
        E = 0.05 * torch.randn(B, 26, 26, generator=gen, dtype=torch.float64)
        E[torch.arange(B) % T == T - 1] = 0.0
        c = rep(cost)
        out.append((rep(A), rep(g), E, torch.where(head > 0, c, torch.zeros_like(c)), solve))
    return lam0, rep(p0), rep(prior), mu, out


def run_script(script, T, second):
    """A sequence_script through ops.pose_lm_seq2_step without F (`second`) or ops.pose_lm_seq_step -> per step the outputs."""
    from spherehand_amd import ops
    lam0, p0, prior, mu, steps = script
    p0 = p0.float().cuda()
    prior = None if prior is None else prior.float().cuda()
    mu = None if mu is None else mu.float().cuda()
    state, trial = ops.pose_lm_seq2_begin(p0, T, lam0) if second else ops.pose_lm_seq_begin(p0, T, lam0)
    out = []
    for A, g, E, cost, solve in steps:
        A, g, E, cost = A.cuda(), g.cuda(), E.cuda(), cost.cuda()
        if second:
            r = ops.pose_lm_seq2_step(state, A, g, E, None, cost, trial, T, prior, mu, solve)
        else:
            r = ops.pose_lm_seq_step(state, A, g, E, cost, trial, T, prior, mu, solve)
        out.append(r)
        trial = r[0] if solve else trial
    return out


@pytest.mark.parametrize("T", (1, 3))
def test_step_without_F_is_the_sequence_step(T):
    """With F NULL every output of shr_pose_lm_seq2_step equals shr_pose_lm_seq_step's bit for bit, on pose_icp_ref.lm_scripts
    with every crop a sequence of T frames: accepted and rejected steps, costs that are not finite, a pivot that is not
    positive, both clamps of lambda, a step without a solve."""
    moved = False
    for script in ref.lm_scripts():
        script = sequence_script(script, T)
        want, got = run_script(script, T, False), run_script(script, T, True)
        for k, (a, b) in enumerate(zip(got, want)):
            for i, (x, y) in enumerate(zip(a, b)):
                assert (x is None) == (y is None)
                if x is not None and (i < 3 or k == 0):             # (cost0 is written by the first step only)
                    assert same_bits(x, y), (k, i)
        moved = moved or not torch.equal(want[0][0], script[1].float().cuda())
    assert moved


def random_system(S, T, seed=7):
    """test_sphere_sequence_gpu.random_system with second off-diagonal blocks F of norm about 0.3, zero at a sequence's last
    two frames: (A, g, E, F, cost, p0, mu)."""
    A, g, E, cost, p0, mu = sgpu.random_system(S, T, seed)
    F = 0.03 * torch.randn(S * T, 26, 26, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    F[torch.arange(S * T) % T >= T - 2] = 0.0
    return A, g, E, F, cost, p0, mu


@pytest.mark.parametrize("T", (3, 4, 5))
def test_block_solve(T):
    """trial_out of the step with F against the restated block solve (sphere_trajectory_ref.block_solve, word for word) given
    the same fp64 equations: within 4 x the fp32 step bar of p + delta, and in fact its fp32 rounding.  F matters: the step
    without it differs.  A NaN in one frame's F keeps trial = p on ALL frames of its sequence and leaves the other
    sequence's bits alone; cost, cost0 and params are the sequences' own."""
    from spherehand_amd import ops
    S = 2
    A, g, E, F, cost, p0, mu = random_system(S, T)
    lam0 = 1e-3

    def step(F_):
        state, trial = ops.pose_lm_seq2_begin(p0.float().cuda(), T, lam0)
        return ops.pose_lm_seq2_step(state, A.cuda(), g.cuda(), E.cuda(), None if F_ is None else F_.cuda(), cost.cuda(), trial, T,
                                     None, mu.float().cuda(), True)

    trial_out, params, c, c0 = step(F)
    assert torch.equal(params.cpu().double(), p0) and same_bits(c, c0) and c.shape == (S,)
    assert torch.allclose(c.cpu().double(), cost.view(S, T).sum(1), rtol=2.0 ** -23)        # (prior = params0: no stiffness term)
    for s in range(S):
        sl = slice(s * T, s * T + T)
        args = (A[sl], g[sl], E[sl], F[sl], float(np.float32(lam0)), mu, p0[sl], p0[sl], T)
        x, y = tref.block_solve(*args), tref.dense_solve(*args)
        want = p0[sl] + torch.as_tensor(x)
        err = (trial_out[sl].cpu().double() - want).abs().max().item()
        print("sequence %d: |trial_out - (p + delta)| %.3g (bar %.3g); the largest step %.3g; block against dense %.3g"
              % (s, err, cpu.STEP_BAR, np.abs(x).max(), np.abs(x - y).max()))
        assert err <= cpu.STEP_BAR
        assert bool(((trial_out[sl].cpu().double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-12).all())
        assert np.abs(x).max() > 1e-3
    assert not torch.equal(step(None)[0], trial_out)
    bad = F.clone()
    bad[(S - 1) * T, 5, 7] = float("nan")
    out_bad = step(bad)
    hit = slice((S - 1) * T, S * T)
    assert torch.equal(out_bad[0][hit].cpu().double(), p0[hit])                  # the whole sequence stays
    assert same_bits(out_bad[0][:(S - 1) * T], trial_out[:(S - 1) * T])
    for i in (1, 2, 3):
        assert same_bits(out_bad[i], (params, c, c0)[i - 1])


def traj_solve(case, T, rows=slice(None), iters=None, observed=None, keypoints=None, tw=cpu.TEMPORAL_WEIGHT, aw=cpu.ACCEL_WEIGHT,
               cap=cpu.ACC_MAX, fw=None):
    from spherehand_amd import ops
    d = case["dev"]
    obs = d["observed"][rows].contiguous() if observed is None else observed
    k = d["keypoints"][rows].contiguous() if keypoints is None else keypoints
    pairs = d["pairs"]
    return ops.sphere_icp_trajectory(obs, d["view"][rows].contiguous(), d["params0"][rows].contiguous(), *tables(case), T,
                                     case["model"].right_hand, case["p2m"], ref.FG_MAX, ref.MAX_DIST,
                                     case["iters"] if iters is None else iters, 1e-3, d["stiffness"], None, rref.DEFAULT_WEIGHT,
                                     rref.DEFAULT_MAX_RESID, rref.BACKGROUND, k, d["confidence"][rows].contiguous(),
                                     pref.DEFAULT_KP_WEIGHT, pref.DEFAULT_KP_MAX, (d["lower"], d["upper"]),
                                     pref.DEFAULT_LIMIT_WEIGHT, pairs, cref.DEFAULT_COLLISION_WEIGHT if pairs else 0.0,
                                     tw, qref.DEFAULT_TS_MAX, None, aw, cap, dev32(fw))


def test_without_the_term_it_is_the_sequence_fitter(mesh):
    """accel_weight = 0 (or seq_len < 3): ops.sphere_icp_trajectory is ops.sphere_icp_sequence and
    render.SphereTrajectoryPoseFitter is SphereSequencePoseFitter, bit for bit; with the term the module's solve and
    normal_equations are the ops', and the result differs."""
    from spherehand_amd.render import SphereSequencePoseFitter, SphereTrajectoryPoseFitter
    for T in (3, 2):
        case = device_case(mesh, 6 // T, T)
        d = case["dev"]
        kw = dict(right_hand=case["model"].right_hand, iters=3, stiffness=case["stiffness"].numpy())
        p, view, obs, k, conf = d["params0"], d["view"], d["observed"], d["keypoints"], d["confidence"]
        want = SphereSequencePoseFitter(mesh, 32, 32, T, temporal_weight=0.5, ts_max=40.0, **kw).cuda().solve(
            obs, p, view, keypoints=k, confidence=conf)
        fit = SphereTrajectoryPoseFitter(mesh, 32, 32, T, temporal_weight=0.5, ts_max=40.0,
                                         accel_weight=0.0 if T == 3 else 1.0, **kw).cuda()
        for a, b in zip(fit.solve(obs, p, view, keypoints=k, confidence=conf), want):
            assert same_bits(a, b), T
        assert not torch.equal(want[0], p)
    case = device_case(mesh, 2, 3)
    for a, b in zip(traj_solve(case, 3, iters=3, tw=0.1, aw=0.0), sgpu.seq_solve(case, 3, iters=3, w=0.1)):
        assert same_bits(a, b)
    d = case["dev"]
    kw = dict(right_hand=case["model"].right_hand, iters=3, stiffness=case["stiffness"].numpy())
    p, view, obs, k, conf = d["params0"], d["view"], d["observed"], d["keypoints"], d["confidence"]
    fit = SphereTrajectoryPoseFitter(mesh, 32, 32, 3, temporal_weight=0.1, accel_weight=0.5, acc_max=30.0, **kw).cuda()
    got = fit.solve(obs, p, view, keypoints=k, confidence=conf)
    for a, b in zip(got, traj_solve(case, 3, iters=3, tw=0.1, aw=0.5, cap=30.0)):
        assert same_bits(a, b)
    assert not torch.equal(got[0], sgpu.seq_solve(case, 3, iters=3, w=0.1)[0])
    parent = SphereSequencePoseFitter(mesh, 32, 32, 3, temporal_weight=0.1, **kw).cuda().normal_equations(obs, p, view, k, conf)
    for a, b in zip(fit.normal_equations(obs, p, view, k, conf),
                    accel(case, p, 3, 0.5, 30.0, None, (parent[0], parent[1], parent[3]), parent[2])):
        assert same_bits(a, b)
    default = SphereTrajectoryPoseFitter(mesh, 32, 32, 3, **kw).cuda()           # the first-difference entry is not launched
    for a, b in zip(default.solve(obs, p, view, keypoints=k, confidence=conf), traj_solve(case, 3, iters=3)):
        assert same_bits(a, b)
    q, c0, c = traj_solve(case, 3, slice(0, 0))
    assert q.shape == (0, 26) and c0.shape == (0,) and c.shape == (0,)
    q, c0, c = traj_solve(case, 3, iters=0)
    assert torch.equal(q, p) and torch.equal(c, c0) and c0.shape == (2,) and bool((c0 > 0).all())


def test_reproducible_and_independent_sequences(mesh):
    """Twice the same bits; sequence s of a batch equals the batch of sequence s alone, for the equations and the whole
    solve."""
    T = 4
    case = device_case(mesh, 2, T)
    p = case["dev"]["params0"]
    fw = cpu.triple_weights(2 * T, T, True)
    one, two = (accel(case, p, T, 0.5, 30.0, fw) for _ in range(2))
    for a, b in zip(one, two):
        assert same_bits(a, b)
    s1, s2 = (traj_solve(case, T, iters=3, tw=0.1, aw=0.5, cap=30.0) for _ in range(2))
    for a, b in zip(s1, s2):
        assert same_bits(a, b)
    for s in (0, 1):
        rows = slice(s * T, s * T + T)
        for a, b in zip(one, accel(case, p[rows].contiguous(), T, 0.5, 30.0, fw[rows])):
            assert same_bits(a[rows], b), s
        alone = traj_solve(case, T, rows, iters=3, tw=0.1, aw=0.5, cap=30.0)
        assert same_bits(s1[0][rows], alone[0]), s
        assert same_bits(s1[1][s:s + 1], alone[1]) and same_bits(s1[2][s:s + 1], alone[2]), s
    assert not torch.equal(s1[0], p)


def test_solve_in_a_graph(mesh):
    """The whole loop captured into one torch.cuda.graph on a single stream and replayed on other observations and keypoints
    equals the eager result bit for bit: nothing in the loop returns to the host."""
    T = 4
    case = device_case(mesh, 2, T)
    d = case["dev"]
    kw = dict(iters=3, tw=0.1, aw=0.5, cap=30.0)
    static_obs, static_k = d["observed"].clone(), d["keypoints"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        traj_solve(case, T, observed=static_obs, keypoints=static_k, **kw)      # warm-up: the library, the allocator
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = traj_solve(case, T, observed=static_obs, keypoints=static_k, **kw)
    other_obs, other_k = torch.roll(d["observed"], 1, 0).contiguous(), torch.roll(d["keypoints"], 1, 0).contiguous()
    static_obs.copy_(other_obs)
    static_k.copy_(other_k)
    graph.replay()
    torch.cuda.synchronize()
    eager = traj_solve(case, T, observed=other_obs, keypoints=other_k, **kw)
    for a, b in zip(out, eager):
        assert same_bits(a, b)
    assert not torch.equal(eager[0], traj_solve(case, T, **kw)[0])


def test_end_to_end(mesh):
    """Two sequences of five frames at 32 x 32 (test_sphere_trajectory_cpu.END_TO_END: the draw that does not amplify
    rounding), one view, the module's defaults, four iterations: cost < cost0 per sequence,
    and the poses of BOTH sequences within 4 x the CPU-measured fp32 bar of the fp64 restatement's (the CPU test holds that
    the fp32 restatement keeps every decision and the same rows in both).

    4 x: the GPU's shr_pose_keypoints_jacobian rounds differently from the numpy fp32 chain the bar is measured with."""
    S, T = cpu.END_TO_END[:2]
    case = on_device(qref.sequence_case(mesh, *cpu.END_TO_END))
    case["dev"]["pairs"] = tuple(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in case["table"])
    q, c0, c = traj_solve(case, T, iters=qref.END_TO_END_ITERS)
    assert c.shape == (S,) and bool((c < c0).all()) and bool(torch.isfinite(q).all())
    q64, c064, c64, lm64 = cpu.end_to_end_run(mesh, torch.float64)
    err = (q.cpu().double() - q64).abs().view(S, -1).amax(1)
    print("|pose - restatement| %s (bar %.3g); cost0 %s against %s; cost %s against %s; decisions %s"
          % (err.tolist(), cpu.POSE_BAR, c0.tolist(), c064.tolist(), c.tolist(), c64.tolist(), [h.tolist() for h in lm64.history]))
    assert torch.allclose(c0.cpu().double(), c064, rtol=cpu.COST_BAR + 2.0 ** -23)       # (cost0 leaves the loop as fp32)
    assert bool((err <= cpu.POSE_BAR).all()), (err, cpu.POSE_BAR)
    print("mean keypoint error %.4g mm, jitter %.4g mm (the restatement's %.4g, %.4g)"
          % (qref.sref.keypoint_error(case["model"], q.cpu(), case["p_star"]).mean(), qref.jitter(case["model"], q.cpu(), case["p_star"], T).mean(),
             qref.sref.keypoint_error(case["model"], q64, case["p_star"]).mean(), qref.jitter(case["model"], q64, case["p_star"], T).mean()))
