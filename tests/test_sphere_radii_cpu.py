"""Parameters that the frames of a group share, without a device: the entries of the arrowhead step in the C ABI with their
argument rules, the unit's code-object metadata, and the restatement (tests/sphere_radii_ref.py) with what keeps it honest --
the Schur solve equals a dense solve of the (26 N + K) system on systems where the coupling matters, without a shared block
and with groups of one frame it is pose_icp_ref.LM exactly, the group's decision rules, and a bad pivot anywhere holds the
whole group.  The GPU tests (tests/test_sphere_radii_gpu.py) hold the kernels to the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_collision_ref as cref
import sphere_icp_ref as iref
import sphere_radii_ref as sref
from conftest import ROOT
from test_pose_ik_cpu import _metadata

ENTRIES = ("shr_sphere_icp_radii_normal_workspace_bytes", "shr_sphere_icp_radii_normal", "shr_pose_lm_shared_state_bytes", "shr_pose_lm_shared_workspace_bytes", "shr_pose_lm_shared_begin",
           "shr_pose_lm_shared_step")
INF = float("inf")
# The Schur solve against numpy.linalg.solve of the dense (26 N + K) system on SOLVE_CASES, max |x_schur - x_dense| /
# max |x_dense| per group over the poses' and the shared parameters' steps together, measured
# (test_schur_solve_equals_the_dense_solve prints it); asserted at 4 x, as DESIGN.md 4.4u does for its block solve.
SCHUR_DENSE_DEVIATION = 1.8e-13
# (G, N, K): K = 41 is the first user's (the hand's radii), K = 64 the largest, K = 1 a single scale; N = 1 a group of one
SOLVE_CASES = ((2, 3, 41), (2, 1, 64), (1, 4, 1), (2, 3, 7), (1, 8, 64))
# The GPU test's bar on a trial against the restated solve given the same fp64 equations: both run the same fp64 recurrences
# in the same order, so what is left is the rounding of p + delta to fp32 -- half a step of fp32 -- and a step of slack for
# a last-place difference of the fp64 sums beneath it (the sequence step's test holds its trial to the same).
TRIAL_BAR_REL, TRIAL_BAR_ABS = 2.0 ** -23, 1e-12


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    contract = text[text.index("Parameters that the frames of a group SHARE"):
                    text.index("long long shr_pose_lm_shared_state_bytes(")]
    for cite in ("mesh/render.py:93-142", "no counterpart of the shared solve", "ARROWHEAD", "0 <= K <= 64", "b / N",
                 "FIRST frame", "BEHIND", "k ascending", "frames ascending, m ascending", "LOWER triangle", "WHOLE group",
                 "ANY frame's factor or in S", "BIT FOR BIT", "no atomics", "capturable in a hipGraph", "2^24", "B % N == 0",
                 "EVERY step"):
        assert cite in contract, cite
    assert text.index("int shr_pose_lm_seq2_step(") < text.index("shr_pose_lm_shared_state_bytes(")     # at the end of the header
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23
    sb, wb = lib.shr_pose_lm_shared_state_bytes, lib.shr_pose_lm_shared_workspace_bytes
    for B, G, K in ((6, 2, 41), (6, 6, 64), (4, 1, 1), (6, 2, 0), (0, 0, 0)):
        assert sb(B, G, K) == 8 * (760 * B + G * K * (K + 3) + 26 * B * K), (B, G, K)
        assert wb(B, G, K) == 8 * (B * (704 + 26 * K) + G * (8 + K)), (B, G, K)
    for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert sb(*bad) == -1 and wb(*bad) == -1
    assert sb(5, 5, 0) == lib.shr_pose_lm_state_bytes(5)           # without a shared block the state is the crop step's
    # host-side argument rules (every call below returns before a launch)
    P = 1 << 20                                                    # an aligned stand-in for a device address
    nan = float("nan")
    #          0 params0 1 shape0 2 B 3 N 4 K 5 lambda0 6 state 7 trial 8 trial_shape 9 stream
    begin = [P, P, 6, 3, 41, 1e-3, P, P, P, None]
    bad = lambda i, val: lib.shr_pose_lm_shared_begin(*(begin[:i] + [val] + begin[i + 1:]))   # noqa: E731
    assert bad(2, 0) == 0
    for i in (0, 1, 6, 7, 8):
        assert bad(i, None) == -1 and bad(i, P + 2) == -1, i
    assert bad(6, P + 4) == -1                                     # the state: 8 bytes
    assert bad(2, -3) == -1 and bad(3, 0) == -1 and bad(3, 4) == -1 and bad(4, -1) == -1
    assert bad(5, 0.0) == -1 and bad(5, nan) == -1
    assert bad(2, (1 << 24) + 2) == -2 and bad(4, 65) == -2
    assert lib.shr_pose_lm_shared_begin(P, P, 0, 0, 41, 1e-3, P, P, P, None) == -1       # the rules come before the no-op
    assert lib.shr_pose_lm_shared_begin(P, None, 0, 3, 0, 1e-3, P, P, None, None) == 0   # K = 0: no shape arrays
    #          0 state 1 A 2 g 3 C 4 R 5 gs 6 cost_data 7 trial 8 trial_shape 9 prior 10 stiffness 11 shape_prior
    #          12 shape_stiffness | 13 solve 14 B 15 N 16 K | 17 trial_out 18 trial_shape_out 19 params 20 shape 21 cost
    #          22 cost0 23 workspace 24 stream
    step = [P] * 13 + [1, 6, 3, 41] + [P] * 7 + [None]
    bad = lambda i, val: lib.shr_pose_lm_shared_step(*(step[:i] + [val] + step[i + 1:]))   # noqa: E731
    assert bad(14, 0) == 0
    required, optional = [0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 18, 19, 20, 21, 22, 23], [9, 10, 11, 12]
    for i in required:
        assert bad(i, None) == -1, i
    for i in required + optional:
        assert bad(i, P + 2) == -1, i
    for i in (0, 1, 2, 3, 4, 5, 6, 23):                            # fp64 buffers: 8 bytes
        assert bad(i, P + 4) == -1, i
    assert bad(15, 4) == -1 and bad(15, 0) == -1 and bad(14, -3) == -1 and bad(16, -1) == -1
    assert bad(14, (1 << 24) + 2) == -2 and bad(16, 65) == -2
    none = list(step)
    none[14] = 0
    for i, val, rc in ((15, 0, -1), (16, 65, -2), (0, None, -1)):  # the rules come before the no-op
        assert lib.shr_pose_lm_shared_step(*(none[:i] + [val] + none[i + 1:])) == rc
    nosolve = list(step)
    nosolve[13], nosolve[17], nosolve[18], nosolve[14] = 0, None, None, 0      # without a solve: no trial outputs
    assert lib.shr_pose_lm_shared_step(*nosolve) == 0
    k0 = list(step)                                                # K = 0: no shared array is needed
    for i in (3, 4, 5, 8, 11, 12, 18, 20):
        k0[i] = None
    k0[16] = 0
    unlaunched = lambda args, i, val: lib.shr_pose_lm_shared_step(*(args[:i] + [val] + args[i + 1:]))   # noqa: E731
    assert unlaunched(k0, 14, 0) == 0
    for i in (1, 2, 6, 7, 17, 19, 21, 22, 23):
        assert unlaunched(k0, i, None) == -1, i
    k0[15], k0[14] = 1, 6                                          # K = 0, N = 1: the crop step's own rules (no workspace)
    for i in (1, 2, 6, 7, 17, 19, 21, 22):
        assert unlaunched(k0, i, None) == -1, i
    assert unlaunched(k0, 14, 0) == 0


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """lm_shared.hip: five kernels, no scratch, no spills, no atomics.  begin uses no LDS; decide 512 bytes (the cost terms);
    frame A, L [26 x 26], x [26], the pivot and Y [26 x 64] in fp64: 24 344 bytes; schur S [64 x 65] (factored in place),
    a frame's Y [26 x 64], z [26], x [64], the pivot and the verdict: 47 328 bytes, three groups per CU by LDS; back L, x
    and d sigma: 6 128 bytes.  DESIGN.md 4.4v tables the figures.  The unit includes lm_state.h alone (which includes
    lm_solve.h alone)."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4v"):design.index("### 4.5 ")]
    assert design.index("### 4.4u") < design.index("### 4.4v")
    sizes, kernels = _metadata("lm_shared", tmp_path)
    assert sizes == [0] * 5 and len(kernels) == 5
    # LDS exact; (VGPRs, SGPRs) as built, the ceilings a few above: they only catch a change of code that costs registers
    want = {"begin": (0, 14, 31), "decide": (64 * 8, 18, 67), "frame": ((2 * 676 + 26 + 1 + 26 * 64) * 8, 26, 55),
            "schur": ((64 * 65 + 26 * 64 + 26 + 64 + 1) * 8 + 8, 30, 56), "back": ((676 + 26 + 64) * 8, 22, 28)}
    seen = set()
    for name, k in kernels.items():
        print(name, k)
        which = re.search(r"pose_lm_shared_([a-z]+)_kernel", name).group(1)
        seen.add(which)
        lds, vgpr, sgpr = want[which]
        assert "pose_lm_shared_%s_kernel" % which in section
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        assert k["group_segment_fixed_size"] == lds, which
        assert k["vgpr_count"] <= vgpr + 6 and k["sgpr_count"] <= sgpr + 8, which
    assert seen == set(want)
    assert want["frame"][0] == 24344 and want["schur"][0] == 47328 and want["back"][0] == 6128
    assert "24 344" in section and "47 328" in section and "6 128" in section
    inc = lambda unit: re.findall(r'#include\s+[<"]([^>"]+)[>"]',                       # noqa: E731
                                  open(os.path.join(ROOT, "spherehand_amd", "csrc", unit)).read())
    assert inc("lm_shared.hip") == ["lm_state.h"] and inc("lm_state.h") == ["lm_solve.h"] and inc("lm_solve.h") == ["normal_eq.h"]
    assert inc("normal_eq.h") == ["common.h"]
    for unit in ("lm_shared.hip", "lm_state.h", "lm_solve.h", "normal_eq.h"):
        assert "atomic" not in open(os.path.join(ROOT, "spherehand_amd", "csrc", unit)).read().lower()


def group_args(sys_, q, N, lam=1e-3):
    A, g, C, R, gs, cost, p0, s0, mu, nu = sys_
    sl = slice(q * N, q * N + N)
    return (A[sl].numpy(), g[sl].numpy(), C[sl].numpy(), R[q].numpy(), gs[q].numpy(), float(np.float32(lam)), mu.numpy(),
            nu.numpy(), p0[sl].numpy(), p0[sl].numpy(), s0[q].numpy(), s0[q].numpy())


def test_schur_solve_equals_the_dense_solve():
    """shr_pose_lm_shared_step's solve (sphere_radii_ref.schur_solve, word for word) against numpy.linalg.solve of the dense
    (26 N + K) system on SOLVE_CASES with lambda = 1e-3 and both stiffnesses; SharedLM's step is that rounded to fp32.  On
    these systems the coupling moves the step by orders of magnitude more than the tolerance, so a step that ignores C
    fails; only the lower triangle of R is read; a bad pivot in one frame, in S, or a NaN in one frame's C fails the whole
    group."""
    worst = 0.0
    for G, N, K in SOLVE_CASES:
        sys_ = sref.random_system(G, N, K)
        A, g, C, R, gs, cost, p0, s0, mu, nu = sys_
        lm = sref.SharedLM(p0, s0, N, 1e-3)
        trial, trial_shape = lm.step(A, g, C, R, gs, cost, p0, s0, None, mu, None, nu)
        assert bool(lm.history[0].all()) and torch.equal(lm.cost, lm.cost0)
        for q in range(G):
            args = group_args(sys_, q, N)
            x, xs = sref.schur_solve(*args)
            y, ys = sref.dense_solve(*args)
            scale = max(np.abs(y).max(), np.abs(ys).max())
            dev = max(np.abs(x - y).max(), np.abs(xs - ys).max()) / scale
            worst = max(worst, dev)
            H, rhs = sref.dense_system(*args)
            w, ws = sref.schur_solve(*args, use_C=False)
            moved = max(np.abs(w - y).max(), np.abs(ws - ys).max()) / scale
            print("G %d N %d K %d, group %d: |schur - dense| %.3g of the largest step %.3g; condition %.3g; without C the step "
                  "is off by %.3g" % (G, N, K, q, dev, scale, np.linalg.cond(H), moved))
            assert dev <= 4 * SCHUR_DENSE_DEVIATION
            assert moved > 1e6 * 4 * SCHUR_DENSE_DEVIATION             # (C matters in these systems)
            sl = slice(q * N, q * N + N)
            assert torch.equal(trial[sl], (p0[sl] + torch.as_tensor(x)).float().double())
            assert torch.equal(trial_shape[q], (s0[q] + torch.as_tensor(xs)).float().double())
            upper = list(args)
            upper[3] = np.tril(args[3]) + 7.0 * np.triu(np.ones_like(args[3]), 1)          # the upper triangle is not read
            again = sref.schur_solve(*upper)
            assert np.array_equal(again[0], x) and np.array_equal(again[1], xs)
    print("schur against dense: worst %.3g" % worst)
    assert SCHUR_DENSE_DEVIATION / 4 <= worst <= 4 * SCHUR_DENSE_DEVIATION
    args = list(group_args(sref.random_system(2, 3, 7), 1, 3))
    for field, index, value in ((0, (1, 3, 3), np.nan), (0, (2,), -np.eye(26)), (2, (0, 4, 2), np.nan), (3, (5, 5), -1e9),
                                (4, (0,), np.nan)):
        broken = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
        broken[field][index] = value
        out = sref.schur_solve(*broken)
        if field == 4:                                             # (a NaN in gs is no bad pivot: it reaches every unknown)
            assert out is not None and np.isnan(out[0]).all() and np.isnan(out[1]).all()
        else:
            assert out is None, (field, index)


def test_without_a_shared_block_it_is_the_crop_step_exactly():
    """K = 0 and N = 1: the restated step gives pose_icp_ref.LM's trial, state and decisions exactly on pose_icp_ref.lm_scripts
    (rejected steps, costs that are not finite, a pivot that is not positive, both clamps of lambda, a step without a solve)."""
    for lam0, p0, prior, mu, steps in ref.lm_scripts():
        a, b = ref.LM(p0, lam0), sref.SharedLM(p0, None, 1, lam0)
        trial = a.trial
        for A, g, cost, solve in steps:
            x = a.step(A, g, cost, trial, prior, mu, solve)
            y, ys = b.step(A, g, None, None, None, cost, trial, None, prior, mu, None, None, solve)
            assert (x is None) == (y is None) and (ys is None) == (y is None)
            if x is not None:
                assert torch.equal(x, y)
                trial = x
            assert torch.equal(a.p, b.p) and torch.equal(a.lam, b.lam) and torch.equal(a.cost, b.cost)
            assert torch.equal(a.history[-1], b.history[-1])
        assert torch.equal(a.cost0.view(torch.int64), b.cost0.view(torch.int64)) and torch.equal(a.accepts, b.accepts) and torch.equal(a.rejects, b.rejects)


def test_the_decision_is_the_groups():
    """One lambda, one cost and one decision per group: the group's total is the chain over its frames, then the shape term;
    a trial is accepted or rejected for all its frames and its shared parameters together; a cost that is not finite in ONE
    frame rejects the group; the first accepted step leaves lambda, then x 0.3 / x 10."""
    G, N, K = 2, 3, 5
    A, g, C, R, gs, cost, p0, s0, mu, nu = sref.random_system(G, N, K, seed=11)
    lm = sref.SharedLM(p0, s0, N, 1e-3)
    sprior = (s0 + 0.5).float().double()
    t1, ts1 = lm.step(A, g, C, R, gs, cost, p0, s0, None, mu, sprior, nu)
    want = torch.stack([(cost[0] + cost[1]) + cost[2], (cost[3] + cost[4]) + cost[5]])
    for k in range(K):
        want = want + nu[k] * ((s0[:, k] - sprior[:, k]) * (s0[:, k] - sprior[:, k]))
    assert torch.equal(lm.cost, want) and torch.equal(lm.cost0, want) and lm.lam.tolist() == [float(np.float32(1e-3))] * 2
    assert not torch.equal(t1, p0) and not torch.equal(ts1, s0)
    worse = cost.clone()
    worse[4] = INF                                                 # group 1: one frame's cost is not finite
    better = cost * 0.5
    better[3:] = worse[3:]
    t2, ts2 = lm.step(2 * A, g, C, R, gs, better, t1, ts1, None, mu, sprior, nu)
    assert lm.history[-1].tolist() == [True, False]
    assert torch.equal(lm.p[:3], t1[:3]) and torch.equal(lm.p[3:], p0[3:])
    assert torch.equal(lm.s[0], ts1[0]) and torch.equal(lm.s[1], s0[1])
    assert torch.equal(lm.A[:3], 2 * A[:3]) and torch.equal(lm.A[3:], A[3:])
    lam0 = float(np.float32(1e-3))
    assert lm.lam.tolist() == [lam0 * 0.3, lam0 * 10.0]
    assert not torch.equal(t2[3:], t1[3:]) and (t2[3:] - p0[3:]).abs().max() < (t1[3:] - p0[3:]).abs().max()  # a shorter step


def test_ops_refuse_what_the_kernels_do_not_take():
    """No device here: the ops refuse CPU tensors, bad group sizes and shapes with a RuntimeError."""
    from spherehand_amd import ops
    p0, s0 = torch.zeros(6, 26), torch.ones(2, 41)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)           # noqa: E731
    for call in (lambda: ops.pose_lm_shared_begin(p0, s0, 3),
                 lambda: ops.pose_lm_shared_begin(p0, s0, 4),
                 lambda: ops.pose_lm_shared_begin(p0, torch.ones(2, 65), 3),
                 lambda: ops.pose_lm_shared_begin(p0, None, 0),
                 lambda: ops.pose_lm_shared_step(f64(6 * 760), f64(6, 26, 26), f64(6, 26), None, None, None, f64(6), p0, None, 3),
                 lambda: ops.pose_lm_shared_step(f64(6 * 3000), f64(6, 26, 26), f64(6, 26), f64(6, 26, 41), f64(2, 41, 41),
                                                 f64(2, 41), f64(6), p0, s0, 3)):
        with pytest.raises(RuntimeError):
            call()
    assert ops.PoseLmSharedMaxK == sref.MAX_K == 64
    for args in ((6, 4, 1), (6, 0, 1), (6, 3, 65), (6, 3, -1), (6, "x", 1)):
        with pytest.raises(RuntimeError):
            ops._pose_lm_shared_args(*args)
    assert ops._pose_lm_shared_args(6, 3, 41) == (3, 41, 2) and ops._pose_lm_shared_args(0, 3, 0) == (3, 0, 0)


# ---- the radius term ----------------------------------------------------------------------------------------------------
# The evaluations the GPU tests run and the bars are measured on: (G, N, table, W, H, V).  32 x 32 is exactly one tile of the
# scan, 40 x 32 has a partial second one; N = 1 is a group of one frame.
EVALUATIONS = ((2, 3, "hand", 32, 32, 1), (2, 1, "hand", 40, 32, 2), (2, 3, "synthetic", 40, 32, 1), (2, 1, "synthetic", 32, 32, 2))
# The chains (sphere_radii_ref.radii_chain, the header's order) against autograd's blocks given the fp64 chain's Jacobian and
# the same held centres, of the largest entry, measured (test_chains_give_the_autograd_blocks prints them); asserted at 4 x.
CHAIN_C_DEVIATION = 3.8e-16
CHAIN_GS_DEVIATION = 1.9e-16
# The fp32 bars, by DESIGN.md 4.4p's method: the restatement with an fp32 chain against the fp64 one, the largest deviation
# per quantity; the GPU tolerance is 4 x that.  A and g are shr_sphere_icp_normal's bits, so its bars hold them
# (tests/test_sphere_icp_cpu.py); R is exact and gs, GIVEN the same centres, is the same chain in both, so the GPU tests hold
# them to the numpy chain bit for bit.  Against the fp64 restatement on its own fp64 centres -- the GPU test's other
# comparison, which shr_sphere_icp_normal's bars are measured for too -- C and gs differ by the fp32 chain's centres (sum u and
# sum d are formed on them) and, C, by its Jacobian: both are measured on the fp32 chain's OWN centres and maps.  Given the
# same centres C differs by the Jacobian alone, FP32_C_HELD_DEVIATION, a tenth of that: recorded, not a bar.
# test_fp32_bars measures them again and holds the constants to within [1/2, 2].
FP32_C_DEVIATION = 2.5e-6         # max |C32 - C64| / max |C64| per frame with rows, the fp32 chain's own centres and maps
FP32_C_HELD_DEVIATION = 2.5e-7    # the same given the fp64 run's centres, rounded once
FP32_GS_DEVIATION = 1.3e-6        # max |gs32 - gs64| / max |gs64| per group: d on the fp32 chain's centres and maps against the fp64 chain's
FP32_COST_DEVIATION = 5.8e-7      # |cost32 - cost64| / cost64 per group of the two runs' own maps, the combined cost
FP32_STEP_DEVIATION = 1.1e-5      # rad | mm: the first step of the calibration at the start, poses and radii
FP32_POSE_DEVIATION = 3.8e-6      # rad | mm: the final poses of the end-to-end case
FP32_RADII_DEVIATION = 3.8e-6     # mm: its final radii
C_BAR, GS_BAR, COST_BAR, STEP_BAR, POSE_BAR, RADII_BAR = (4 * d for d in (
    FP32_C_DEVIATION, FP32_GS_DEVIATION, FP32_COST_DEVIATION, FP32_STEP_DEVIATION, FP32_POSE_DEVIATION, FP32_RADII_DEVIATION))
SHAPE_STIFFNESS = 1.0             # the module's default
# The end-to-end case: two groups of three frames at 32 x 32, four iterations, (G, N, table, seed).  Four iterations do not
# converge; the case is a draw on which a perturbation of the start by 1e-9, with either sign, moves no pose parameter and no
# radius of the fp64 restatement by more than END_TO_END_STABLE (four fp32 steps of a value up to 64) and keeps every accept
# decision: test_end_to_end_case_is_stable holds that.
END_TO_END = (2, 3, "hand", 31)
END_TO_END_STABLE = 4 * 2.0 ** -18


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def test_radii_entry_argument_rules():
    from spherehand_amd import _lib
    lib = _lib.lib()
    ws = lib.shr_sphere_icp_radii_normal_workspace_bytes
    assert ws(6, 2, 41, 40, 32) == 8 * (6 * 2 * 2 * (16 * 41 + 4) + 6 * 41 * 2) and ws(0, 0, 0, 0, 0) == 0
    for i in range(5):
        assert ws(*[-1 if k == i else 1 for k in range(5)]) == -1
    P = 1 << 20
    #          0 observed 1 view_centres 2 radii 3 view 4 jac | 5 B 6 V 7 J 8 W 9 H 10 N | 11 ax 12 bx 13 ay 14 by 15 fg_max
    #          16 max_dist | 17 A 18 g 19 cost 20 count 21 C 22 R 23 gs 24 moments 25 dist 26 owner 27 workspace 28 stream
    args = [P] * 5 + [6, 2, 41, 32, 32, 3] + [1.0, 0.0, 1.0, 0.0, 1000.0, 50.0] + [P] * 11 + [None]
    bad = lambda i, val: lib.shr_sphere_icp_radii_normal(*(args[:i] + [val] + args[i + 1:]))   # noqa: E731
    assert bad(5, 0) == 0
    required, optional = [0, 1, 2, 3, 4, 17, 18, 19, 20, 21, 22, 23, 27], [24, 25, 26]
    for i in required:
        assert bad(i, None) == -1, i
    for i in required + optional:
        assert bad(i, P + 2) == -1, i
    for i in (17, 18, 19, 21, 22, 23, 24, 1, 27):                  # fp64 buffers 8 bytes; view_centres and workspace 16
        assert bad(i, P + 4) == -1, i
    for i in (1, 27):
        assert bad(i, P + 8) == -1, i
    assert bad(10, 0) == -1 and bad(10, -1) == -1 and bad(10, 4) == -1 and bad(5, 7) == -1         # 1 <= N, B % N == 0
    assert bad(5, -3) == -1 and bad(6, 0) == -1 and bad(7, 0) == -1 and bad(16, -1.0) == -1 and bad(16, float("nan")) == -1
    assert bad(7, 65) == -2 and bad(8, 2049) == -2 and bad(5, 65538) == -2
    none = list(args)
    none[5], none[10] = 0, 0
    assert lib.shr_sphere_icp_radii_normal(*none) == -1            # the rules come before the no-op
    none[10], none[16] = 5, INF
    assert lib.shr_sphere_icp_radii_normal(*([None] * 5 + none[5:17] + [None] * 12)) == 0


def test_radii_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """sphere_icp_radii.hip: three kernels, no scratch, no spills, no atomics.  The scan is sphere_icp_scan.h's with sixteen
    moments: 64 (centre, radius) records, 256 pixel records of 17 doubles, 256 owners and four ballots in LDS, 36 896
    bytes (four workgroups per CU by LDS and by its launch bounds); the assembly 64 x 16 moments and the 192 x 26 fp32
    Jacobian, 28 160 bytes; the group pass none.  sphere_icp.hip, over the same header, keeps its own figures
    (tests/test_sphere_icp_cpu.py).  DESIGN.md 4.4v tables them."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4v"):design.index("### 4.5 ")]
    sizes, kernels = _metadata("sphere_icp_radii", tmp_path)
    assert sizes == [0, 0, 0] and len(kernels) == 3
    want = {"scan": (64 * 16 + 256 * 17 * 8 + 256 * 4 + 4 * 8, 96, 96), "assemble": (64 * 16 * 8 + 192 * 26 * 4, 48, 80),
            "group": (0, 16, 32)}
    for name, k in kernels.items():
        print(name, k)
        which = re.search(r"sphere_icp_radii_([a-z]+)_kernel", name).group(1)
        lds, vgpr, sgpr = want[which]
        assert "sphere_icp_radii_%s_kernel" % which in section
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        assert k["group_segment_fixed_size"] == lds, which
        assert k["vgpr_count"] <= vgpr and k["sgpr_count"] <= sgpr, which
    assert want["scan"][0] == 36896 and want["assemble"][0] == 28160 and "36 896" in section and "28 160" in section
    inc = lambda unit: re.findall(r'#include\s+[<"]([^>"]+)[>"]',                       # noqa: E731
                                  open(os.path.join(ROOT, "spherehand_amd", "csrc", unit)).read())
    assert inc("sphere_icp_radii.hip") == ["sphere_icp_scan.h"] == inc("sphere_icp.hip")
    assert inc("sphere_icp_scan.h") == ["normal_eq.h"] and inc("normal_eq.h") == ["common.h"]
    for unit in ("sphere_icp_radii.hip", "sphere_icp_scan.h", "normal_eq.h"):
        assert "atomic" not in open(os.path.join(ROOT, "spherehand_amd", "csrc", unit)).read().lower().replace("no atomics", "")


def evaluation(mesh, G, N, table, W, H, V):
    case = sref.radii_case(mesh, G, N, table, W, H, V)
    radii = case["radii0"].copy()
    radii[-1] = (radii[-1] * np.float32(0.9)).astype(np.float32)   # the groups' tables differ
    return case, case["params0"].float().double(), radii


def test_g_is_the_autograd_gradient(mesh):
    """(g, gs) of the restatement (the Jacobian of a group's stacked residuals) = the reverse-mode gradient of
    1/2 sum min(d, max_dist)^2 with respect to (the poses, the group's radii), to 1e-12 of its largest entry; with one table
    for all frames A, g and the cost are sphere_icp_ref.normal's; R is diagonal with the spheres' row counts; the (26 N + J)
    matrix of a group is symmetric positive semi-definite."""
    for G, N, table, W, H, V in EVALUATIONS:
        case, p, radii = evaluation(mesh, G, N, table, W, H, V)
        m, view = case["model"], torch.as_tensor(case["view"])
        n = sref.radii_normal(m, view, case["observed"], p, radii, N, case["p2m"])
        b, v, y, o = (torch.as_tensor(t) for t in n["points"])
        q = p.clone().requires_grad_(True)
        r = torch.as_tensor(radii.astype(np.float64)).requires_grad_(True)
        d = (y - m.view_centres(q, view)[b, v, o]).norm(dim=-1) - r[b // N, o]
        saturated = torch.as_tensor(n["dist"].astype(np.float64) ** 2).sum() - (d.detach() ** 2).sum()     # (constant in p and r)
        (0.5 * ((d * d).sum() + saturated)).backward()
        for name, got, want in (("g", n["g"], q.grad), ("gs", n["gs"], r.grad)):
            err, scale = (got - want).abs().max().item(), want.abs().max().item()
            print("G %d N %d %s %dx%d V %d: |%s - autograd| %.3g of %.3g" % (G, N, table, W, H, V, name, err, scale))
            assert err <= 1e-12 * scale and scale > 0
        assert int(n["count"].min()) > 10 and saturated.item() >= -1e-6 * float(n["cost"].sum())
        same = sref.radii_normal(m, view, case["observed"], p, case["radii0"], N, case["p2m"])
        old = iref.normal(m, view, case["observed"], p, case["p2m"])
        assert torch.equal(same["cost"], old["cost"]) and torch.equal(same["count"], old["count"])
        assert (same["A"] - old["A"]).abs().max() <= 1e-12 * old["A"].abs().max()
        assert (same["g"] - old["g"]).abs().max() <= 1e-12 * old["g"].abs().max()
        for g_ in range(G):
            R = n["R"][g_]
            rows = torch.bincount(o[(b // N) == g_], minlength=m.J).double()
            assert torch.equal(torch.diagonal(R), rows) and not bool((R - torch.diag(rows)).any())
            sl = slice(g_ * N, g_ * N + N)
            Hd, _ = sref.dense_system(n["A"][sl], n["g"][sl], n["C"][sl], R, n["gs"][g_], 0.0, np.zeros(26), np.zeros(m.J), p[sl],
                                      p[sl], radii[g_], radii[g_])
            assert np.linalg.eigvalsh(Hd)[0] >= -1e-9 * np.abs(Hd).max()


def test_chains_give_the_autograd_blocks(mesh):
    """C, R and gs of the header's chains (sphere_radii_ref.radii_chain: tiles of 1024 pixels, pixels ascending) equal the
    blocks of autograd's J^T J and J^T d given the fp64 chain's Jacobian and centres (the fp32 centres deciding the rows): R exactly, C and gs
    to 4 x the measured deviation of the largest entry; a sphere without a row has exact +0 columns; the four new moments
    are sum u and sum d of the rows."""
    worst = dict(C=0.0, gs=0.0)
    for G, N, table, W, H, V in EVALUATIONS:
        case, p, radii = evaluation(mesh, G, N, table, W, H, V)
        m, view = case["model"], torch.as_tensor(case["view"])
        c32 = m.centres32(p, view)
        _, jac = m.chain.jacobian(p)
        n = sref.radii_normal(m, view, case["observed"], p, radii, N, case["p2m"], centres32=c32)
        extra, rows, C, R, gs = sref.radii_chain(case["observed"], c32, radii, view.float().numpy(), jac.numpy(), N, case["p2m"],
                                                 centres=m.view_centres(p, view).numpy())
        assert np.array_equal(R, n["R"].numpy()) and np.array_equal(rows.sum(1), n["count"].numpy())
        for name, x, y in (("C", C, n["C"].numpy()), ("gs", gs, n["gs"].numpy())):
            dev = np.abs(x - y).max() / np.abs(y).max()
            worst[name] = max(worst[name], dev)
            print("G %d N %d %s %dx%d V %d: %s chains against autograd %.3g" % (G, N, table, W, H, V, name, dev))
        empty = rows == 0
        assert empty.any() and not C.transpose(0, 2, 1)[empty].any() and not np.signbit(C.transpose(0, 2, 1)[empty]).any()
        assert not extra[empty].any()
        u = iref.directions(m, view, p, n["points"]).numpy()
        b, o = n["points"][0], n["points"][3]
        su = np.zeros((G * N, m.J, 3))
        np.add.at(su, (b, o), u)
        assert np.abs(su - extra[..., :3]).max() <= 1e-12 * np.abs(su).max()
    print("chains against autograd: C %.3g, gs %.3g" % (worst["C"], worst["gs"]))
    assert worst["C"] <= 4 * CHAIN_C_DEVIATION and worst["gs"] <= 4 * CHAIN_GS_DEVIATION
    assert worst["C"] >= CHAIN_C_DEVIATION / 4 and worst["gs"] >= CHAIN_GS_DEVIATION / 4


def test_radius_guard(mesh):
    """A group with a radius that is not finite or not > 0 -- sphere_icp_ref.synthetic_table's own radius of 0, a NaN, +inf, a
    negative one -- is void: cost = +inf and A = g = C = 0 for every frame of it, R = gs = 0; the other group is what it is
    alone; the step rejects the void group and keeps its start."""
    case, p, radii = evaluation(mesh, 2, 3, "synthetic", 40, 32, 1)
    m, view = case["model"], torch.as_tensor(case["view"])
    good = sref.radii_normal(m, view, case["observed"], p, radii, 3, case["p2m"])
    _, jac = m.chain.jacobian(p)
    c32 = m.centres32(p, view)
    for value in (0.0, float("nan"), INF, -3.0):
        bad = radii.copy()
        bad[1, sref.sref.SYN_ZERO] = value
        assert sref.void_groups(bad).tolist() == [False, True]
        n = sref.radii_normal(m, view, case["observed"], p, bad, 3, case["p2m"])
        assert bool((n["cost"][3:] == INF).all()) and not any(bool(n[k][3:].any()) for k in ("A", "g", "C"))
        assert not bool(n["R"][1].any()) and not bool(n["gs"][1].any())
        for k in ("A", "g", "C", "cost"):
            assert torch.equal(n[k][:3], good[k][:3]), k
        assert torch.equal(n["R"][0], good["R"][0]) and torch.equal(n["gs"][0], good["gs"][0])
        _, _, C, R, gs = sref.radii_chain(case["observed"], c32, bad, view.float().numpy(), jac.numpy(), 3, case["p2m"])
        assert not C[3:].any() and not R[1].any() and not gs[1].any() and C[:3].any() and R[0].any()
    lm = sref.SharedLM(p, torch.as_tensor(bad), 3, 1e-3)
    lm.step(n["A"], n["g"], n["C"], n["R"], n["gs"], n["cost"], p, torch.as_tensor(bad).double(), None, None, None, torch.ones(7))
    assert lm.history[0].tolist() == [True, False] and lm.cost[1] == INF
    assert sref.synthetic_table(zero=True)[2][sref.sref.SYN_ZERO] == 0 and sref.void_groups(sref.synthetic_table(zero=True)[2][None])[0]


def test_module_refuses_what_it_does_not_take(mesh):
    """The module's defaults and refusals; without a device the ops refuse CPU tensors."""
    from spherehand_amd import ops
    from spherehand_amd.render import SphereCollisionPoseFitter, SphereRadiiCalibrator
    fit = SphereRadiiCalibrator(mesh, 32, 32, 3, stiffness=ref.STIFFNESS)
    assert isinstance(fit, SphereCollisionPoseFitter) and fit.group_size == 3 and fit.render_weight == 0.0
    assert fit.shape_stiffness.tolist() == [SphereRadiiCalibrator.DEFAULT_SHAPE_STIFFNESS] * 41 == [SHAPE_STIFFNESS] * 41
    assert SphereRadiiCalibrator(mesh, 32, 32, 3, shape_stiffness=0.0).shape_stiffness.tolist() == [0.0] * 41
    for word in ("SphereCollisionPoseFitter", "NO autograd", "NOT checked", "4.4v", "fitter.radii.copy_(radii[g])", "out of scope",
                 "render_weight", "arrowhead", "collision table"):
        assert word in SphereRadiiCalibrator.__doc__, word
    for bad in (dict(render_weight=1.0), dict(render_weight=None), dict(shape_stiffness=-1.0), dict(group_size=0)):
        kw = dict(group_size=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            SphereRadiiCalibrator(mesh, 32, 32, kw.pop("group_size"), **kw)
    obs, view, p0 = torch.full((6, 1, 32, 32), 100.0), torch.eye(4).expand(6, 1, 4, 4).contiguous(), torch.zeros(6, 26)
    tables = (fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv)
    radii = fit.radii.expand(2, 41).contiguous()
    for call in (lambda: fit.solve(obs, p0, view), lambda: fit.normal_equations(obs, p0, view),
                 lambda: fit.solve(obs[:5], p0[:5], view[:5]),
                 lambda: ops.sphere_icp_radii_normal(obs, view, p0, *tables, radii, 3),
                 lambda: ops.sphere_icp_radii_normal(obs, view, p0, *tables, radii, 4),
                 lambda: ops.sphere_icp_radii_normal(obs, view, p0, *tables, fit.radii, 3),
                 lambda: ops.sphere_icp_calibrate(obs, view, p0, *tables, radii[:1], 3)):
        with pytest.raises(RuntimeError):
            call()


_RUNS = {}


def end_to_end_run(mesh, dtype=torch.float64, eps=0.0, seed=None):
    """sphere_radii_ref.calibrate of the end-to-end case with the module's defaults in `dtype`, once per process."""
    G, N, table, seed0 = END_TO_END
    seed = seed0 if seed is None else seed
    key = (dtype, eps, seed)
    if key not in _RUNS:
        case = sref.radii_case(mesh, G, N, table, seed=seed)
        start = case["params0"].float().double()
        noise = torch.randn(G * N, 26, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
        _RUNS[key] = sref.calibrate(case["model"].to(dtype), case["view"], case["observed"], start + eps * noise, case["radii0"],
                                    N, case["p2m"], case["table"], cref.DEFAULT_COLLISION_WEIGHT, sref.END_TO_END_ITERS, 1e-3,
                                    case["stiffness"], start, np.full(case["model"].J, SHAPE_STIFFNESS), None,
                                    **sref.terms_of(case))
    return _RUNS[key]


def test_end_to_end_case_is_stable(mesh):
    """The end-to-end case does not amplify rounding: the fp64 restatement's final poses and radii move by at most
    END_TO_END_STABLE under a perturbation of the start by +-1e-9 (the prior held), and every accept decision stays."""
    base = end_to_end_run(mesh)
    moved = 0.0
    for eps in (1e-9, -1e-9):
        other = end_to_end_run(mesh, eps=eps)
        moved = max(moved, (other[0] - base[0]).abs().max().item(), (other[1] - base[1]).abs().max().item())
        assert all(torch.equal(x, y) for x, y in zip(base[4].history, other[4].history))
    print("a 1e-9 perturbation of the start moves the result by %.3g; bar %.3g; decisions %s"
          % (moved, END_TO_END_STABLE, [h.tolist() for h in base[4].history]))
    assert moved <= END_TO_END_STABLE


def fp32_deviations(mesh):
    dev = dict(C=0.0, C_own=0.0, gs=0.0, cost=0.0, step=0.0, pose=0.0, radii=0.0)
    for G, N, table, W, H, V in EVALUATIONS:
        case, p, radii = evaluation(mesh, G, N, table, W, H, V)
        m64, m32 = case["model"], case["model"].to(torch.float32)
        view = torch.as_tensor(case["view"])
        held = m64.centres32(p, view)
        C64, C32 = (sref.radii_chain(case["observed"], held, radii, view.float().numpy(), m.chain.jacobian(p.to(m.dtype))[1].numpy(),
                                     N, case["p2m"])[2] for m in (m64, m32))
        own32 = sref.radii_chain(case["observed"], m32.centres32(p.float(), view), radii, view.float().numpy(),
                                 m32.chain.jacobian(p.float())[1].numpy(), N, case["p2m"])        # (the fp32 chain's own centres and maps)
        gs32 = own32[4]
        own64 = sref.radii_chain(case["observed"], held, radii, view.float().numpy(), m64.chain.jacobian(p)[1].numpy(), N, case["p2m"],
                                 centres=m64.view_centres(p, view).numpy())
        gs64 = own64[4]
        dev["C_own"] = max(dev["C_own"], (np.abs(own32[2] - own64[2]).reshape(G * N, -1).max(1)
                                          / np.abs(own64[2]).reshape(G * N, -1).max(1)).max())
        dev["gs"] = max(dev["gs"], (np.abs(gs32 - gs64).max(1) / np.abs(gs64).max(1)).max())
        big = np.abs(C64).reshape(G * N, -1).max(1)
        dev["C"] = max(dev["C"], (np.abs(C64 - C32).reshape(G * N, -1).max(1) / big).max())
        steps, costs = [], []
        tab = case["table"]
        for m in (m64, m32):                                                     # the first step, the runs' own maps
            A, g, C, R, gs, cost, _ = sref.combined(m, view, case["observed"], p, radii, N, case["p2m"], tab,
                                                    cref.DEFAULT_COLLISION_WEIGHT, **sref.terms_of(case))
            lm = sref.SharedLM(p, torch.as_tensor(radii), N, 1e-3)
            tp, ts = lm.step(A, g, C, R, gs, cost, p, torch.as_tensor(radii).double(), None, case["stiffness"], None,
                             np.full(m.J, SHAPE_STIFFNESS))
            steps.append(torch.cat([(tp - p).flatten(), (ts - torch.as_tensor(radii).double()).flatten()]))
            costs.append(cost.view(G, N).sum(1))
        dev["cost"] = max(dev["cost"], ((costs[0] - costs[1]).abs() / costs[0]).max().item())
        dev["step"] = max(dev["step"], (steps[0] - steps[1]).abs().max().item())
        print("G %d N %d %s %dx%d V %d: C %.3g, cost %.3g, step %.3g so far" % (G, N, table, W, H, V, dev["C"], dev["cost"], dev["step"]))
    r64, r32 = end_to_end_run(mesh, torch.float64), end_to_end_run(mesh, torch.float32)
    same = all(torch.equal(x, y) for x, y in zip(r64[4].history, r32[4].history)) and \
        all(torch.equal(x, y) for x, y in zip(r64[4].rows, r32[4].rows))
    dev["pose"], dev["radii"] = (r64[0] - r32[0]).abs().max().item(), (r64[1] - r32[1]).abs().max().item()
    return dev, same


def test_fp32_bars(mesh):
    """The constants above, measured again.  The fp32 / fp64 CPU pair keeps EVERY accept decision and the same rows in the
    end-to-end case; the calibration's cost falls on both groups and its radii move."""
    dev, same = fp32_deviations(mesh)
    print("fp32 against fp64: C own centres %.3g" % dev["C_own"])
    print("fp32 against fp64: C %.3g, gs %.3g, cost %.3g, step %.3g, pose %.3g, radii %.3g; same %s"
          % (dev["C"], dev["gs"], dev["cost"], dev["step"], dev["pose"], dev["radii"], same))
    assert same
    q, radii, cost0, cost, lm = end_to_end_run(mesh, torch.float64)
    case = sref.radii_case(mesh, *END_TO_END[:3], seed=END_TO_END[3])
    print("end_to_end: cost0 %s, cost %s, decisions %s" % (cost0.tolist(), cost.tolist(), [h.tolist() for h in lm.history]))
    assert bool((cost < cost0).all()) and bool(torch.stack(lm.history).any())
    assert (radii - torch.as_tensor(case["radii0"]).double()).abs().max() > 0.1
    for name, const in (("C_own", FP32_C_DEVIATION), ("C", FP32_C_HELD_DEVIATION), ("gs", FP32_GS_DEVIATION), ("cost", FP32_COST_DEVIATION),
                        ("step", FP32_STEP_DEVIATION), ("pose", FP32_POSE_DEVIATION), ("radii", FP32_RADII_DEVIATION)):
        assert const / 2 <= dev[name] <= 2 * const, (name, dev[name], const)
