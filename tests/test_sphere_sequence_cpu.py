"""The sequence fit of the sphere model without a device: the entries of the C ABI with their argument rules, the new units'
code-object metadata, the restatement (tests/sphere_sequence_ref.py) and what keeps it honest -- its g is the reverse-mode
gradient of 1/2 cost, the header's chains equal the blocks autograd gives, the block solve equals a dense solve, with
T = 1 it is sphere_collision_ref's loop exactly -- and the fp32 bars the GPU tests (tests/test_sphere_sequence_gpu.py) hold
the kernels to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_icp_ref as ref
import sphere_collision_ref as cref
import sphere_sequence_ref as qref
from conftest import ROOT
from test_pose_ik_cpu import _metadata

ENTRIES = ("shr_sphere_temporal_normal_workspace_bytes", "shr_sphere_temporal_normal", "shr_pose_lm_seq_state_bytes",
           "shr_pose_lm_seq_workspace_bytes", "shr_pose_lm_seq_begin", "shr_pose_lm_seq_step")
INF = float("inf")

# The fp32 bars, by DESIGN.md 4.4p's method: the restatement run with an fp32 chain against the fp64 one on the GPU tests'
# inputs (EVALUATIONS below), the largest deviation per quantity; the GPU tolerance is 4 x that.  A, g and E are compared GIVEN
# THE SAME model-frame centres (the fp64 run's, rounded once), so that both runs hold the same spheres with rows and the
# same e, as the kernel and the restatement do: what differs is the Jacobian (sphere_sequence_ref.chain on each).
# test_fp32_bars measures them again and holds the constants to within [1/2, 2].
FP32_A_DEVIATION = 2.64e-7        # max |A32 - A64| / max |A64| per frame with rows
FP32_G_DEVIATION = 3.31e-7        # max |g32 - g64| / max |g64| per frame with rows
FP32_E_DEVIATION = 1.95e-7        # max |E32 - E64| / max |E64| per frame with a weighted next pair
FP32_COST_DEVIATION = 1.38e-7     # |cost32 - cost64| / cost64 per sequence of the two runs' own centres, the combined cost
FP32_STEP_DEVIATION = 5.72e-5     # rad | mm: the first step of the combined sequence fit at params0
FP32_POSE_DEVIATION = 1.28e-4     # rad | mm: the final pose of the end-to-end case, the sequences that keep the decisions
# Between the kernel and the numpy chain GIVEN the entry's own centres and Jacobian nothing is left but the rounding of at
# most 2 x 41 x 3 fp64 terms per entry, both computed in the same order: 1e-13 of the largest entry is generous.
ORDER_BAR = 1e-13
# The block solve against numpy.linalg.solve of the dense 26 T x 26 T system on SOLVE_CASES, max |x_block - x_dense| /
# max |x_dense| per sequence, measured (test_block_solve_equals_the_dense_solve prints it); asserted at 4 x.
BLOCK_DENSE_DEVIATION = 2.0e-13
A_BAR, G_BAR, E_BAR, COST_BAR, STEP_BAR, POSE_BAR = (4 * FP32_A_DEVIATION, 4 * FP32_G_DEVIATION, 4 * FP32_E_DEVIATION,
                                                     4 * FP32_COST_DEVIATION, 4 * FP32_STEP_DEVIATION, 4 * FP32_POSE_DEVIATION)
TEMPORAL_WEIGHT, TS_MAX = qref.DEFAULT_TEMPORAL_WEIGHT, qref.DEFAULT_TS_MAX
# The evaluations the GPU test of the equations runs and the bars are measured on: (S, T, table, temporal_weight, ts_max,
# frame weights or None).  The finite ts_max saturate some spheres of the interpolated sequences and keep others.
EVALUATIONS = ((1, 2, "hand", 1.0, INF, False), (2, 3, "hand", 0.5, 40.0, True), (3, 2, "synthetic", 2.0, INF, False),
               (1, 8, "hand", 0.1, 12.0, False), (3, 8, "synthetic", 1.0, 6.0, True), (3, 1, "hand", 1.0, INF, False))
SOLVE_CASES = ((2, 3, "hand"), (1, 8, "hand"), (3, 2, "synthetic"))
END_TO_END = (2, 8, "hand")


def frame_weights(B, T, on):
    """[B] fp32 in [0.5, 1.5) with one pair per batch at 0 (a cut) where B allows, or None."""
    if not on:
        return None
    fw = (0.5 + torch.rand(B, generator=torch.Generator().manual_seed(5))).numpy().astype(np.float32)
    if T > 2:
        fw[1] = 0.0
    return fw


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    contract = text[text.index("A sequence of frames fitted jointly"):
                    text.index("long long shr_sphere_temporal_normal_workspace_bytes(")]
    for cite in ("network/util_modules.py:360-381", "network/util_modules.py:349-358", "create_network_and_criterion.py:242-245",
                 "no counterpart", "DETACHES", "SYMMETRIC", "block-TRIDIAGONAL", "MODEL frame", "exactly ts_max is saturated",
                 "+inf never saturates", "e = 0 still gives rows", "NO term", "ALWAYS WRITTEN, NEVER accumulated", "exact +0",
                 "LOWER triangle", "bit-symmetric", "not touched", "no atomics", "nothing contracted", "65535", "B % T == 0",
                 "LATER frame", "one workgroup per frame", "One workgroup per sequence", "BIT FOR BIT", "11 520", "11 072",
                 "ANYWHERE in the sequence"):
        assert cite in contract, cite
    assert text.index("shr_sphere_collision_normal(") < text.index("shr_sphere_temporal_normal(")  # after the collision section
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23
    ws = lib.shr_sphere_temporal_normal_workspace_bytes
    assert ws(24, 8, 41) == 0 and ws(0, 0, 0) == 0 and ws(-1, 1, 1) == -1 and ws(1, -1, 1) == -1 and ws(1, 1, -1) == -1
    assert lib.shr_pose_lm_seq_state_bytes(3) == 3 * 1440 * 8 and lib.shr_pose_lm_seq_state_bytes(-1) == -1
    assert lib.shr_pose_lm_seq_workspace_bytes(3) == 3 * 1384 * 8 and lib.shr_pose_lm_seq_workspace_bytes(-1) == -1
    assert lib.shr_pose_lm_seq_state_bytes(0) == 0 and 1440 >= 2 * 676 + 3 * 26 + 6 and 1384 >= 2 * 676 + 26
    # host-side argument rules (every call below returns before a launch)
    P = 1 << 20                                                    # a 16-byte aligned stand-in for a device address
    #          0 keypoints 1 jac 2 frame_weight | 3 temporal_weight 4 ts_max | 5 B 6 T 7 J 8 accumulate |
    #          9 A 10 g 11 E 12 cost 13 count 14 workspace 15 stream
    normal = [P] * 3 + [1.0, 20.0, 6, 3, 41, 1] + [P] * 6 + [None]
    bad = lambda i, val: lib.shr_sphere_temporal_normal(*(normal[:i] + [val] + normal[i + 1:]))   # noqa: E731
    assert bad(5, 0) == 0                                          # B == 0: nothing to do
    required, optional = [0, 1, 9, 10, 11, 12, 13], [2, 14]
    for i in required:
        assert bad(i, None) == -1, i
    for i in required + optional:
        assert bad(i, P + 2) == -1, i
    for i in (0, 14, 9, 10, 11, 12):                               # keypoints, workspace: 16 bytes; A, g, E, cost: 8
        assert bad(i, P + 4) == -1, i
    for i in (0, 14):
        assert bad(i, P + 8) == -1, i
    for i in (5, 6, 7):
        assert bad(i, -1) == -1, i
    assert bad(7, 0) == -1 and bad(6, 0) == -1                     # 1 <= J, 1 <= T
    assert bad(6, 4) == -1 and bad(5, 7) == -1                     # B % T == 0
    nan = float("nan")
    assert bad(3, -0.5) == -1 and bad(3, INF) == -1 and bad(3, nan) == -1      # the weight: finite and >= 0
    assert bad(4, -1.0) == -1 and bad(4, nan) == -1                # ts_max >= 0 ...
    none = list(normal)
    none[5], none[4] = 0, INF                                      # ... or +inf; the rules come before the no-op
    assert lib.shr_sphere_temporal_normal(*none) == 0
    assert bad(8, 2) == -1 and bad(8, -1) == -1                    # accumulate 0 or 1
    assert bad(5, 65536 - 65536 % 3 + 3) == -2 and bad(7, 65) == -2
    none[7] = 65
    assert lib.shr_sphere_temporal_normal(*none) == -2
    none[7], none[3] = 41, -1.0
    assert lib.shr_sphere_temporal_normal(*none) == -1
    none[3], none[6] = 0.0, 0
    assert lib.shr_sphere_temporal_normal(*none) == -1
    assert lib.shr_sphere_temporal_normal(*([None] * 3 + [0.0, 0.0, 0, 1, 1, 0] + [None] * 7)) == 0
    #          0 params0 1 B 2 T 3 lambda0 4 state 5 trial 6 stream
    begin = [P, 6, 3, 1e-3, P, P, None]
    bad = lambda i, val: lib.shr_pose_lm_seq_begin(*(begin[:i] + [val] + begin[i + 1:]))   # noqa: E731
    assert bad(1, 0) == 0
    for i in (0, 4, 5):
        assert bad(i, None) == -1 and bad(i, P + 2) == -1, i
    assert bad(4, P + 4) == -1                                     # the state: 8 bytes
    assert bad(1, -3) == -1 and bad(2, 0) == -1 and bad(2, 4) == -1 and bad(3, 0.0) == -1 and bad(3, nan) == -1
    assert bad(1, (1 << 24) + 2) == -2
    assert lib.shr_pose_lm_seq_begin(P, 0, 0, 1e-3, P, P, None) == -1         # the rules come before the no-op
    #          0 state 1 A 2 g 3 E 4 cost_data 5 trial 6 prior 7 stiffness | 8 solve 9 B 10 T |
    #          11 trial_out 12 params 13 cost 14 cost0 15 workspace 16 stream
    step = [P] * 8 + [1, 6, 3] + [P] * 5 + [None]
    bad = lambda i, val: lib.shr_pose_lm_seq_step(*(step[:i] + [val] + step[i + 1:]))   # noqa: E731
    assert bad(9, 0) == 0
    for i in (0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 15):
        assert bad(i, None) == -1, i
    for i in list(range(8)) + [11, 12, 13, 14, 15]:
        assert bad(i, P + 2) == -1, i
    for i in (0, 1, 2, 3, 4, 15):                                  # fp64 buffers: 8 bytes
        assert bad(i, P + 4) == -1, i
    assert bad(10, 4) == -1 and bad(10, 0) == -1 and bad(9, -3) == -1 and bad(9, (1 << 24) + 2) == -2
    one = list(step)
    one[3], one[9], one[10] = None, 0, 1                           # E may be NULL with T == 1 (B = 0: no launch here)
    assert lib.shr_pose_lm_seq_step(*one) == 0
    nosolve = list(step)
    nosolve[8], nosolve[11], nosolve[15], nosolve[9] = 0, None, None, 0       # without a solve: no trial_out, no workspace
    assert lib.shr_pose_lm_seq_step(*nosolve) == 0


def test_units_compile_for_gfx950_without_scratch(tmp_path):
    """sphere_temporal.hip: one kernel, one workgroup of 256 threads per FRAME, no scratch, no spills, no atomics; two 192 x 26
    fp32 Jacobians (2 x 19 968 bytes), both pairs' e [64 x 3] fp64, cost terms and flags in LDS: 44 544 bytes.  lm_seq.hip: the
    step is one wave per SEQUENCE with A, L, W [26 x 26] fp64, x, y and the pivot in LDS: 16 648 bytes; begin uses none.
    DESIGN.md 4.4t tables the figures.  sphere_temporal.hip includes common.h alone, lm_seq.hip lm_band.h alone (which
    includes lm_state.h alone, which includes lm_solve.h alone)."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4t"):design.index("### 4.5 ")]
    assert design.index("### 4.4s") < design.index("### 4.4t")
    sizes, kernels = _metadata("sphere_temporal", tmp_path)
    assert sizes == [0] and len(kernels) == 1
    for name, k in kernels.items():
        print(name, k)
        assert "sphere_temporal_kernel" in name and "sphere_temporal_kernel" in section
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        assert k["group_segment_fixed_size"] == 2 * 192 * 26 * 4 + 2 * 64 * 3 * 8 + 2 * 64 * 8 + 2 * 64 * 4 == 44544
        assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 106
    sizes, kernels = _metadata("lm_seq", tmp_path)
    assert sizes == [0, 0] and len(kernels) == 2
    for name, k in kernels.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        if "step" in name:
            assert "pose_lm_seq_step_kernel" in name and "pose_lm_seq_step_kernel" in section
            assert k["group_segment_fixed_size"] == (3 * 26 * 26 + 2 * 26 + 1) * 8 == 16648
            assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 106
        else:
            assert "pose_lm_seq_begin_kernel" in name and k["group_segment_fixed_size"] == 0 and k["vgpr_count"] <= 16
    assert "44 544" in section and "16 648" in section
    inc = lambda unit: re.findall(r'#include\s+[<"]([^>"]+)[>"]',                       # noqa: E731
                                  open(os.path.join(ROOT, "spherehand_amd", "csrc", unit)).read())
    assert inc("sphere_temporal.hip") == ["normal_eq.h"] and inc("lm_seq.hip") == ["lm_band.h"]
    assert inc("lm_band.h") == ["lm_state.h"] and inc("lm_state.h") == ["lm_solve.h"] and inc("lm_solve.h") == ["normal_eq.h"]
    assert inc("normal_eq.h") == ["common.h"]
    for unit in ("sphere_temporal.hip", "lm_seq.hip", "lm_band.h", "lm_state.h", "lm_solve.h", "normal_eq.h"):
        assert "atomic" not in open(os.path.join(ROOT, "spherehand_amd", "csrc", unit)).read().lower()


def evaluation_inputs(mesh, S, T, table, weights_on):
    case = qref.sequence_case(mesh, S, T, table)
    return case, case["params0"].float().double(), frame_weights(S * T, T, weights_on)


def test_g_is_the_autograd_gradient(mesh):
    """g of the restatement (the Jacobian of the stacked residuals) = the reverse-mode gradient of 1/2 w sum min(n2, cap) through
    pose_ik_ref.Chain, to 1e-12 of its largest entry; the sequence's 26 T x 26 T matrix is symmetric positive
    semi-definite; cost and count are the pairs' own, stored with the LATER frame."""
    for S, T, table, w, cap, fw_on in EVALUATIONS:
        case, p, fw = evaluation_inputs(mesh, S, T, table, fw_on)
        m = case["model"]
        n = qref.normal(m, p, T, w, cap, fw, chain_residual=True)
        q = p.clone().requires_grad_(True)
        cost = qref.energy(m, q, T, w, cap, fw, held=n["decided"])
        (0.5 * cost.sum()).backward()
        err, scale = (q.grad - n["g"]).abs().max().item(), n["g"].abs().max().item()
        d = n["decided"]
        print("S %d T %d %s ts_max %g: spheres with rows %s, saturated %d; |g - autograd| %.3g of %.3g"
              % (S, T, table, cap, n["count"].tolist(), int((d["valid"] & ~d["act"]).sum()), err, scale))
        assert err <= 1e-12 * max(scale, 1e-300)
        assert torch.allclose(cost.detach(), n["cost"], rtol=1e-5, atol=0)     # (the contract's e is on the fp32 centres:
        # a centre 100 mm out is rounded by 4e-6 mm, a difference of a few mm by 1e-6 of itself)
        first = torch.arange(S * T) % T == 0
        assert not n["cost"][first].any() and not n["count"][first].any()
        assert not n["E"][torch.arange(S * T) % T == T - 1].any()
        if T == 1:
            assert not n["A"].any() and not n["g"].any() and not n["E"].any()
            continue
        assert scale > 0 and int(n["count"].sum()) > 0
        if cap < INF:
            assert int((d["valid"] & ~d["act"]).sum()) > 0 and int(d["act"].sum()) > 0     # both sides of the cap are met
        for s in range(S):
            sl = slice(s * T, s * T + T)
            H, _ = qref.dense_system(n["A"][sl], n["g"][sl], n["E"][sl], 0.0, np.zeros(26), p[sl], p[sl], T)
            assert np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max())
            assert np.linalg.eigvalsh(0.5 * (H + H.T))[0] >= -1e-9 * np.abs(H).max()


def test_chains_give_the_autograd_blocks(mesh):
    """A, g, E, cost and count of the header's chains (sphere_sequence_ref.chain: +Jc in frame t + 1's columns, -Jc in frame
    t's, spheres ascending) equal the blocks of autograd's J^T W J given the fp64 chain's Jacobian, to 1e-13 of the largest
    entry.  A is bit-symmetric, E of a last frame and of a cut pair is exactly 0; accumulate = 1 adds to what is there
    and leaves a frame without a weighted pair alone; weight 0 touches nothing."""
    for S, T, table, w, cap, fw_on in EVALUATIONS:
        case, p, fw = evaluation_inputs(mesh, S, T, table, fw_on)
        m = case["model"]
        _, jac = m.chain.jacobian(p)
        c32 = m.centres(p).float().numpy()
        A, g, E, cost, count = qref.chain(c32, jac.numpy(), T, w, cap, fw)
        n = qref.normal(m, p, T, w, cap, fw, centres32=c32)
        assert np.array_equal(A, A.transpose(0, 2, 1)) and np.array_equal(count, n["count"].numpy())
        for name, x, y in (("A", A, n["A"]), ("g", g, n["g"]), ("E", E, n["E"]), ("cost", cost, n["cost"])):
            scale = max(np.abs(x).max(), 1e-300)
            dev = np.abs(x - y.numpy()).max() / scale
            print("S %d T %d %s: %s chains against autograd %.3g" % (S, T, table, name, dev))
            assert dev <= ORDER_BAR
        last = np.arange(S * T) % T == T - 1
        assert not E[last].any() and not np.signbit(E[last]).any()
        if fw is not None and T > 2:
            assert not E[1].any() and count[2] == 0 and cost[2] == 0
        rng = np.random.default_rng(3)
        base = (rng.standard_normal((S * T, 26, 26)), rng.standard_normal((S * T, 26)), rng.standard_normal(S * T))
        A2, g2, E2, cost2, _ = qref.chain(c32, jac.numpy(), T, w, cap, fw, into=base)
        assert np.array_equal(E2, E)
        assert np.array_equal(A2, base[0] + A) and np.array_equal(g2, base[1] + g) and np.array_equal(cost2, base[2] + cost)
        A0, g0, E0, cost0, count0 = qref.chain(c32, jac.numpy(), T, 0.0, cap, fw, into=base)
        assert np.array_equal(A0, base[0]) and np.array_equal(g0, base[1]) and np.array_equal(cost0, base[2])
        assert not E0.any() and np.array_equal(count0, count)


def test_truncation_rule():
    """The kp_max rule of 4.4r on a pair of frames: a sphere moved by (3, 4, 0), exactly 5 in fp32 and fp64, is saturated at
    ts_max = 5 and at the fp32 below and has rows at the next fp32 above; a saturated sphere pays cap2 and the result is
    the call without it plus that; a NaN centre gives no term; +inf never saturates; e = 0 still gives rows (of zero
    residual: A and E without g)."""
    c = np.zeros((2, 4, 4), np.float32)
    c[0, :, :3] = [(1.0, 2.0, 3.0), (0.0, 0.0, 0.0), (5.0, 5.0, 5.0), (7.0, 7.0, 7.0)]
    c[1, :, :3] = [(4.0, 6.0, 3.0), (0.0, 0.0, 0.0), (np.nan, 5.0, 5.0), (7.0, 7.5, 7.0)]
    up, down = np.nextafter(np.float32(5.0), np.float32(6.0)), np.nextafter(np.float32(5.0), np.float32(4.0))
    jac = np.random.default_rng(0).standard_normal((2, 12, 26)).astype(np.float32)
    for cap, rows, term0 in ((5.0, [False, True, False, True], 25.0), (down, [False, True, False, True], float(down) ** 2),
                             (up, [True, True, False, True], 25.0), (INF, [True, True, False, True], 25.0)):
        d = qref.decide(c, 2, cap)
        assert d["act"][0].tolist() == rows and not d["act"][1].any()
        assert d["valid"][0].tolist() == [True, True, False, True] and d["n2"][0, 0] == 25.0
        assert d["term"][0, 0] == term0 and d["term"][0, 1] == 0.0 and d["term"][0, 2] == 0.0 and d["term"][0, 3] == 0.25
    A, g, E, cost, count = qref.chain(c, jac, 2, 2.0, 5.0)
    assert count.tolist() == [0, 2] and cost[0] == 0.0 and cost[1] == 2.0 * ((25.0 + 0.0) + 0.25)
    without = qref.chain(np.ascontiguousarray(c[:, [1, 3]]), np.ascontiguousarray(jac.reshape(2, 4, 3, 26)[:, [1, 3]]).reshape(2, 6, 26),
                         2, 2.0, 5.0)
    assert np.array_equal(A, without[0]) and np.array_equal(g, without[1]) and np.array_equal(E, without[2])
    assert cost[1] == without[3][1] + 2.0 * 25.0
    still = qref.chain(c[:, [1]], jac[:, 3:6], 2, 1.0, 5.0)                   # e = 0 alone: rows, no gradient
    assert still[4].tolist() == [0, 1] and still[0].any() and still[2][0].any() and not still[1].any() and not still[3].any()


def test_block_solve_equals_the_dense_solve(mesh):
    """shr_pose_lm_seq_step's block Cholesky with forward and back substitution (sphere_sequence_ref.block_solve, word for
    word) against numpy.linalg.solve of the dense 26 T x 26 T system, on the combined equations of SOLVE_CASES at params0
    with lambda = 1e-3 and STIFFNESS; the restatement's LAPACK-based step (SeqLM) against both; a bad pivot in one frame
    fails the whole sequence."""
    worst = 0.0
    mu = ref.STIFFNESS
    for S, T, table in SOLVE_CASES:
        case = qref.sequence_case(mesh, S, T, table)
        p = case["params0"].float().double()
        A, g, E, cost, _ = qref.combined(case["model"], case["view"], case["observed"], p, case["p2m"], T, case["table"],
                                         cref.DEFAULT_COLLISION_WEIGHT if case["table"] is not None else 0.0, 1.0, INF, None,
                                         **qref.terms_of(case))
        lm = qref.SeqLM(p, T, 1e-3)
        trial = lm.step(A, g, E, cost, p, None, torch.as_tensor(mu))
        for s in range(S):
            sl = slice(s * T, s * T + T)
            args = (A[sl].numpy(), g[sl].numpy(), E[sl].numpy(), float(np.float32(1e-3)), mu, p[sl].numpy(), p[sl].numpy(), T)
            x, y = qref.block_solve(*args), qref.dense_solve(*args)
            dev = np.abs(x - y).max() / np.abs(y).max()
            worst = max(worst, dev)
            H, rhs = qref.dense_system(*args)
            print("S %d T %d %s, sequence %d: |block - dense| %.3g of the largest step %.3g; condition %.3g; residual %.3g"
                  % (S, T, table, s, dev, np.abs(y).max(), np.linalg.cond(H), np.abs(H @ x.reshape(-1) - rhs).max() / np.abs(rhs).max()))
            assert dev <= 4 * BLOCK_DENSE_DEVIATION
            want = p[sl] + torch.as_tensor(x)                          # (the trial is that rounded to fp32: half an ulp, or one)
            assert bool(((trial[sl] - want).abs() <= 2.0 ** -23 * want.abs() + 1e-12).all())
    print("block against dense: worst %.3g" % worst)
    assert worst <= 4 * BLOCK_DENSE_DEVIATION
    bad = A[:T].numpy().copy()
    bad[T - 1] = -np.eye(26)
    assert qref.block_solve(bad, g[:T].numpy(), E[:T].numpy(), 1e-3, mu, p[:T].numpy(), p[:T].numpy(), T) is None
    nan = A[:T].numpy().copy()
    nan[1, 3, 3] = np.nan
    assert qref.block_solve(nan, g[:T].numpy(), E[:T].numpy(), 1e-3, mu, p[:T].numpy(), p[:T].numpy(), T) is None


def test_T1_is_the_collision_loop_exactly(mesh):
    """With T = 1 the restatement's loop gives sphere_collision_ref.solve's poses, costs and decisions exactly, whatever the
    temporal weight."""
    case = qref.sequence_case(mesh, 3, 1)
    terms = qref.terms_of(case)
    args = (case["model"], case["view"], case["observed"], case["params0"], case["p2m"])
    a = cref.solve(*args, case["table"], 1.0, 4, 1e-3, case["stiffness"], **terms)
    b = qref.solve(*args, 1, case["table"], 1.0, 0.5, 20.0, None, 4, 1e-3, case["stiffness"], **terms)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3].history, b[3].history)) and torch.equal(a[3].lam, b[3].lam)


def test_ops_refuse_what_the_kernels_do_not_take(mesh):
    """No device here: the ops refuse CPU tensors and bad scalars with a RuntimeError; the module's defaults."""
    from spherehand_amd import ops
    from spherehand_amd.render import SphereCollisionPoseFitter, SphereSequencePoseFitter
    fit = SphereSequencePoseFitter(mesh, 32, 32, 3, stiffness=ref.STIFFNESS)
    assert isinstance(fit, SphereCollisionPoseFitter) and fit.seq_len == 3
    assert fit.temporal_weight == SphereSequencePoseFitter.DEFAULT_TEMPORAL_WEIGHT == TEMPORAL_WEIGHT
    assert fit.ts_max == SphereSequencePoseFitter.DEFAULT_TS_MAX == TS_MAX
    for word in ("SphereCollisionPoseFitter", "NO autograd", "NOT checked", "4.4t", "network/util_modules.py:360-381",
                 "bit for bit", "block-tridiagonal", "detaches"):
        assert word in SphereSequencePoseFitter.__doc__, word
    for bad in (dict(temporal_weight=-1.0), dict(temporal_weight=INF), dict(temporal_weight=float("nan")), dict(ts_max=-1.0),
                dict(ts_max=float("nan"))):
        with pytest.raises(ValueError):
            SphereSequencePoseFitter(mesh, 32, 32, 3, **bad)
    with pytest.raises(ValueError):
        SphereSequencePoseFitter(mesh, 32, 32, 0)
    obs, view, p0 = torch.full((6, 1, 32, 32), 100.0), torch.eye(4).expand(6, 1, 4, 4).contiguous(), torch.zeros(6, 26)
    tables = (fit.fk.offset, fit.fk.offset_inv, fit.kp_bone, fit.kp_wv, fit.radii)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)           # noqa: E731
    for call in (lambda: fit.solve(obs, p0, view), lambda: fit.normal_equations(obs, p0, view),
                 lambda: ops.sphere_temporal_normal(p0, *tables[:4], 3),
                 lambda: ops.sphere_temporal_normal(p0, *tables[:4], 4),
                 lambda: ops.sphere_temporal_normal(p0, *tables[:4], 3, temporal_weight=-1.0),
                 lambda: ops.sphere_icp_sequence(obs, view, p0, *tables, 4),
                 lambda: ops.sphere_icp_sequence(obs, view, p0, *tables, 3, temporal_weight=INF),
                 lambda: ops.sphere_icp_sequence(obs, view, p0, *tables, 3, ts_max=float("nan")),
                 lambda: ops.pose_lm_seq_begin(p0, 3),
                 lambda: ops.pose_lm_seq_step(f64(6 * 1440), f64(6, 26, 26), f64(6, 26), None, f64(6), p0, 3)):
        with pytest.raises(RuntimeError):
            call()


_RUNS = {}


def end_to_end_run(mesh, dtype=torch.float64):
    """sphere_sequence_ref.solve of the end-to-end case (END_TO_END: two sequences of eight frames) with the module's
    defaults in `dtype`, once per process (the GPU tests run the same)."""
    if dtype not in _RUNS:
        S, T, table = END_TO_END
        case = qref.sequence_case(mesh, S, T, table)
        p0 = case["params0"].float().double()
        _RUNS[dtype] = qref.solve(case["model"].to(dtype), case["view"], case["observed"], p0, case["p2m"], T, case["table"],
                                  cref.DEFAULT_COLLISION_WEIGHT, TEMPORAL_WEIGHT, TS_MAX, None, qref.END_TO_END_ITERS, 1e-3,
                                  case["stiffness"], **qref.terms_of(case))
    return _RUNS[dtype]


def end_to_end_runs(mesh):
    return {dt: end_to_end_run(mesh, dt) for dt in (torch.float64, torch.float32)}


def kept(lm64, lm32):
    """[S] bool: the sequences on which the two runs keep the same accept sequence and the same spheres with rows."""
    same = (torch.stack(lm64.history) == torch.stack(lm32.history)).all(0)
    for a, b in zip(lm64.rowed, lm32.rowed):
        if a is not None:
            same &= (a == b).view(lm64.S, -1).all(1)
    return same


def fp32_deviations(mesh):
    dev = dict(A=0.0, g=0.0, E=0.0, cost=0.0, step=0.0, pose=0.0)
    for S, T, table, w, cap, fw_on in EVALUATIONS:
        if T == 1:
            continue
        case, p, fw = evaluation_inputs(mesh, S, T, table, fw_on)
        m64, m32 = case["model"], case["model"].to(torch.float32)
        held = m64.centres(p).float().numpy()
        (A64, g64, E64, _, cnt), (A32, g32, E32, _, _) = (qref.chain(held, m.chain.jacobian(p)[1].numpy(), T, w, cap, fw)
                                                          for m in (m64, m32))
        for name, x, y in (("A", A64, A32), ("g", g64, g32), ("E", E64, E32)):
            big = np.abs(x).reshape(S * T, -1).max(1)
            live = big > 0
            dev[name] = max(dev[name], (np.abs(x - y).reshape(S * T, -1).max(1)[live] / big[live]).max())
        print("S %d T %d %s: A %.3g, g %.3g, E %.3g so far" % (S, T, table, dev["A"], dev["g"], dev["E"]))
    for S, T, table in SOLVE_CASES:                                              # the combined fit's first step, own centres
        case = qref.sequence_case(mesh, S, T, table)
        p, mu = case["params0"].float().double(), case["stiffness"]
        steps, costs = [], []
        for m in (case["model"], case["model"].to(torch.float32)):
            A, g, E, cost, _ = qref.combined(m, case["view"], case["observed"], p, case["p2m"], T, case["table"],
                                             cref.DEFAULT_COLLISION_WEIGHT if case["table"] is not None else 0.0, TEMPORAL_WEIGHT,
                                             TS_MAX, None, **qref.terms_of(case))
            lm = qref.SeqLM(p, T, 1e-3, m.dtype)
            steps.append(lm.step(A, g, E, cost, p, None, mu, True) - p)
            costs.append(cost.view(S, T).sum(1))
        dev["cost"] = max(dev["cost"], ((costs[0] - costs[1]).abs() / costs[0]).max().item())
        dev["step"] = max(dev["step"], (steps[0] - steps[1]).abs().max().item())
        print("S %d T %d %s: cost %.3g, step %.3g so far" % (S, T, table, dev["cost"], dev["step"]))
    run = end_to_end_runs(mesh)
    (q64, _, _, lm64), (q32, _, _, lm32) = run[torch.float64], run[torch.float32]
    same = kept(lm64, lm32)
    T = END_TO_END[1]
    diff = (q64 - q32).abs().view(-1, T * 26).amax(1)
    print("end_to_end: the fp32 run keeps the decisions and the rows: %s; |pose32 - pose64| %s; decisions %s"
          % (same.tolist(), diff.tolist(), [h.tolist() for h in lm64.history]))
    dev["pose"] = diff[same].max().item() if bool(same.any()) else float("nan")
    return dev, same


def test_fp32_bars(mesh):
    """The constants above, measured again.  The fp32 / fp64 CPU pair keeps both sequences of the end-to-end case; the
    fit's cost falls on every sequence (cost <= cost0 per sequence) and the temporal term has rows inside the loop."""
    dev, same = fp32_deviations(mesh)
    print("fp32 against fp64: A %.3g, g %.3g, E %.3g, cost %.3g, step %.3g, pose %.3g; same %s"
          % (dev["A"], dev["g"], dev["E"], dev["cost"], dev["step"], dev["pose"], same.tolist()))
    assert bool(same.all())
    _, cost0, cost, lm = end_to_end_runs(mesh)[torch.float64]
    print("end_to_end: cost0 %s, cost %s" % (cost0.tolist(), cost.tolist()))
    assert bool((cost <= cost0).all()) and bool((cost < cost0).any()) and int(lm.rowed[0].sum()) > 0
    for name, const in (("A", FP32_A_DEVIATION), ("g", FP32_G_DEVIATION), ("E", FP32_E_DEVIATION), ("cost", FP32_COST_DEVIATION),
                        ("step", FP32_STEP_DEVIATION), ("pose", FP32_POSE_DEVIATION)):
        assert const / 2 <= dev[name] <= 2 * const, (name, dev[name], const)
