"""The keypoint pose solver without a device: the torch restatement (tests/pose_ik_ref.py) and the property that keeps it
honest, its backward formula against central differences of its own converged solution, KeypointPoseSolver.initial_pose,
the three entries of the C ABI with their argument rules, the new unit's code-object metadata, and the fp32 bar the GPU
tests (tests/test_pose_ik_gpu.py) hold the kernels to."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pose_ik_ref as ref
from conftest import ROOT

ENTRIES = ("shr_pose_keypoints_jacobian", "shr_pose_ik_fwd", "shr_pose_ik_bwd")

# The fp32 bar.  The restatement run in fp32 on the CPU (torch's own association of the sums) on the GPU tests' inputs
# (pose_ik_ref.solver_cases), its worst deviation from the fp64 run: what fp32 arithmetic of this chain costs.  The GPU
# tolerance is 4 x that, so that another, equally valid, order of the sums does not cost a pass.  test_fp32_bar measures
# both again and holds the constants to within [1/2, 2] of the measurement (another torch build rounds its sums
# differently, not by a factor).
FP32_POSE_DEVIATION = 1.8e-4        # rad | mm, the worst of the cases: noisy 1.79e-4 (3 mm residuals times the Jacobian's
                                    # rounding move the minimiser), synthetic 3.4e-5, exact 2.9e-6 / 3.8e-6
FP32_EXACT_POSE_DEVIATION = 3.8e-6  # ... of the two exact cases alone (one unit in the last place of a translation of 32 .. 64 mm)
FP32_JACOBIAN_DEVIATION = 2.8e-5    # mm/rad | mm/mm at the cases' p*, entries up to 114
FP32_BACKWARD_DEVIATION = 1.3e-5    # rad/mm (synthetic; exact 2.7e-7 / 3.5e-7): the backward formula at the cases' p*, upstream pose_ik_ref.upstream(5, 23)
POSE_BAR = 4 * FP32_POSE_DEVIATION
EXACT_POSE_BAR = 4 * FP32_EXACT_POSE_DEVIATION   # exact data: the tighter bar, from the same measurement
BACKWARD_BAR = 4 * FP32_BACKWARD_DEVIATION
JACOBIAN_BAR = 4 * FP32_JACOBIAN_DEVIATION


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def test_restatement_recovers_the_seeded_poses(mesh):
    """256 poses of sample_poses_batched (generator seed 0), starts p* + N(0, 0.2) rad with the translation at
    p* + N(0, 2 mm): 12 iterations of the loop as the header states it recover every pose to < 1e-8 (observed 1.3e-14),
    the cost never rises, and iters = 0 returns the start."""
    chain = ref.Chain(mesh)
    p, p0 = ref.start_poses(256, 0.2)
    K = chain.keypoints(p)
    q, c0, c, _ = ref.solve(chain, K, p0, iters=12)
    err = (q - p).abs().max().item()
    print("256 poses, 12 iterations: max |p - p*| %.3g, max cost %.3g (start %.3g)" % (err, c.max().item(), c0.max().item()))
    assert err < 1e-8 and bool((c <= c0).all())
    q, c0, c, _ = ref.solve(chain, K[:3], p0[:3], iters=0)
    assert torch.equal(q, p0[:3]) and torch.equal(c, c0)


def test_backward_formula_against_central_differences(mesh):
    """At zero residual the Gauss-Newton implicit-function gradient is exact: <G, p(K)> differentiated by central
    differences of the restatement's converged solution (20 iterations from p*) along random target directions, at
    h = 2^-4 and h / 2 mm.  The discrepancy is the differences' own second-order term: it falls by 4."""
    chain = ref.Chain(mesh)
    B = 2
    p, _ = ref.start_poses(B, 0.1, seed=3)
    K = chain.keypoints(p)
    gen = torch.Generator().manual_seed(4)
    G = torch.randn(B, 26, generator=gen, dtype=torch.float64)
    gt = ref.backward(chain, p, G)
    directions = [torch.randn(B, chain.J, 3, generator=gen, dtype=torch.float64) for _ in range(4)]
    err = []
    for h in (2.0 ** -4, 2.0 ** -5):
        worst = 0.0
        for D in directions:
            up = ref.solve(chain, K + h * D, p, iters=20)[0]
            dn = ref.solve(chain, K - h * D, p, iters=20)[0]
            fd = ((up - dn) * G).sum(-1) / (2 * h)
            worst = max(worst, ((gt * D).sum((1, 2)) - fd).abs().max().item())
        err.append(worst)
    scale = gt.abs().max().item()
    print("|fd - formula| %.3g at h = 2^-4, %.3g at h / 2: ratio %.2f; largest |gradient| %.3g" % (err[0], err[1], err[0] / err[1], scale))
    assert 3.5 < err[0] / err[1] < 4.5 and err[1] < 1e-3 * scale


@pytest.mark.parametrize("right_hand", (True, False))
def test_initial_pose_aligns_the_palm(mesh, right_hand):
    """On exact data the palm keypoints of kp(initial_pose(K)) are K's to 1e-9 in fp64 (keypoints, not angles: the Euler
    triple is not unique), the fingers are at 0, also at cos(y) = 0."""
    from spherehand_amd.render import KeypointPoseSolver
    solver = KeypointPoseSolver(mesh, right_hand=right_hand)
    chain = ref.Chain(mesh, right_hand=right_hand)
    p, _ = ref.start_poses(64, 0.1, seed=2)
    p[0, 1], p[1, 1] = -np.pi / 2, np.pi / 2
    K = chain.keypoints(p)
    p_init = solver.initial_pose(K)
    assert p_init.dtype == torch.float64 and p_init.shape == (64, 26) and bool((p_init[:, 6:] == 0).all())
    palm = chain.bone < 2
    err = (chain.keypoints(p_init)[:, palm] - K[:, palm]).abs().max().item()
    print("right_hand %s: palm keypoints after initial_pose: max error %.3g" % (right_hand, err))
    assert int(palm.sum()) == 11 and err < 1e-9
    assert solver.initial_pose(torch.cat([K, torch.ones(64, 41, 1, dtype=K.dtype)], -1).float()).dtype == torch.float32
    assert "74 %" in KeypointPoseSolver.initial_pose.__doc__


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    contract = text[text.index("Pose from keypoints"):text.index("int shr_pose_keypoints_jacobian(")]
    for cite in ("mesh/kinematicsTransformation.py:157-177", "mesh/render.py:65-88", "fp64", "[1e-9, 1e6]", "gets zeros"):
        assert cite in contract, cite
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23
    # host-side argument rules (every call below returns before a launch)
    A = 1 << 20                                                    # a 16-byte aligned stand-in for a device address
    jac = [A, 2, A, A, 41, A, A, 1, A, A, None]
    fwd = [A, A, 2, A, A, 41, A, A, 1, None, 0, None, 12, 1e-3, A, A, A, None]
    bwd = [A, A, 2, A, A, 41, A, A, 1, None, 0, None, A, None]
    for entry, args, nB, nJ, pointers, aligned16 in ((lib.shr_pose_keypoints_jacobian, jac, 1, 4, (0, 2, 3, 5, 6, 8, 9), (2, 3, 6, 8)),
                                                     (lib.shr_pose_ik_fwd, fwd, 2, 5, (0, 1, 3, 4, 6, 7, 14, 15, 16), (3, 4, 7)),
                                                     (lib.shr_pose_ik_bwd, bwd, 2, 5, (0, 1, 3, 4, 6, 7, 12), (3, 4, 7))):
        bad = lambda i, val: entry(*(args[:i] + [val] + args[i + 1:]))   # noqa: E731
        assert bad(nB, 0) == 0                                     # B == 0: nothing to do
        for i in pointers:
            assert bad(i, None) == -1, (entry, i)
            assert bad(i, A + 2) == -1, (entry, i)
        for i in aligned16:
            assert bad(i, A + 4) == -1, (entry, i)
        assert bad(nB, -1) == -1 and bad(nJ, 0) == -1 and bad(nJ, -1) == -1
        assert bad(nB, (1 << 24) + 1) == -2 and bad(nJ, 65) == -2
    bad = lambda i, val: lib.shr_pose_ik_fwd(*(fwd[:i] + [val] + fwd[i + 1:]))   # noqa: E731
    assert bad(12, -1) == -1 and bad(13, 0.0) == -1 and bad(13, -1.0) == -1 and bad(13, float("nan")) == -1
    for entry, args in ((lib.shr_pose_ik_fwd, fwd), (lib.shr_pose_ik_bwd, bwd)):
        with_w = args[:9] + [A, 7] + args[11:]
        assert entry(*with_w) == -1                                # a weight stride that is neither 0 nor J
        assert entry(*(args[:9] + [A + 2, 0] + args[11:])) == -1 and entry(*(args[:11] + [A + 2] + args[12:])) == -1


def _metadata(unit, tmp_path):
    from spherehand_amd import build
    out = str(tmp_path / (unit + ".s"))
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", unit + ".hip")],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(s) for s in re.findall(r"; ScratchSize: (\d+)", text)]
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
                                                          r"group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", block)}
    return sizes, kernels


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_pose_vertices_cpu.py's reading of the code-object metadata.  pose_ik.hip: three kernels, no scratch, no
    spills, one 64-lane workgroup each with the crop's whole state in LDS -- the sincos table and the 17 transforms, the
    45 x 3 finger tangent rows, the 192 x 26 fp32 Jacobian, A and its factor in fp64, and the vectors: 36 704 bytes, four
    crops per CU by LDS; at most 256 VGPRs (one wave per crop: the solver's 186 leave two waves per SIMD).  The units the
    new code shares a header with keep their kernels.  DESIGN.md 4.4m has the figures."""
    sizes, kernels = _metadata("pose_ik", tmp_path)
    assert len(sizes) == 3 and max(sizes) == 0, sizes
    assert len(kernels) == 3
    lds = 23 * 12 + 12 + 68 * 16 + 135 * 16 + 192 * 26 * 4 + 2 * 26 * 26 * 8 + (26 + 26 + 64 + 1) * 8 + (192 + 64) * 4 + 4 * 26 * 4 + 8
    for name, k in kernels.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["vgpr_count"] <= 256, name
        assert k["group_segment_fixed_size"] == lds == 36704, name
    assert {n for n in kernels if "pose_keypoints_jacobian_kernel" in n} and {n for n in kernels if "pose_ik_fwd_kernel" in n} \
        and {n for n in kernels if "pose_ik_bwd_kernel" in n}
    for unit, count in (("pose_vertices", 2), ("fk", 6)):
        sizes, others = _metadata(unit, tmp_path)
        assert len(others) == count and max(sizes) == 0, (unit, sorted(others))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4m"):design.index("### 4.5 ")]
    for word in ("pose_keypoints_jacobian_kernel", "pose_ik_fwd_kernel", "pose_ik_bwd_kernel", "36 704"):
        assert word in section, word


def test_ops_refuse_what_the_kernels_do_not_take(mesh):
    """No device here: the ops refuse CPU tensors with a RuntimeError; the module's tables."""
    from spherehand_amd import hand_model, ops
    from spherehand_amd.render import KeypointPoseSolver
    solver = KeypointPoseSolver(mesh, stiffness=np.full(26, 0.5))
    wv, _, bone = hand_model.sphere_model(mesh)
    assert solver.num_keypoints == 41 and solver.iters == 12 and solver.lambda0 == 1e-3 and solver.right_hand
    assert np.array_equal(solver.kp_bone.numpy(), bone) and solver.kp_bone.dtype == torch.int32
    assert np.array_equal(solver.kp_wv.numpy(), wv) and tuple(solver.stiffness.shape) == (26,)
    assert KeypointPoseSolver(mesh).stiffness is None
    K, p0 = torch.zeros(2, 41, 3), torch.zeros(2, 26)
    with pytest.raises(RuntimeError):
        solver(K, p0)
    with pytest.raises(RuntimeError):
        solver.solve(K, p0)
    with pytest.raises(RuntimeError):
        solver.jacobian(p0)
    with pytest.raises(RuntimeError):
        ops.pose_ik_bwd(p0, p0, solver.fk.offset, solver.fk.offset_inv, solver.kp_bone, solver.kp_wv)


def test_fp32_bar(mesh):
    """The two constants above, measured again: the restatement in fp32 against fp64 on the GPU tests' inputs.  The fp64
    run itself is at its minimiser in every case (last step < 1e-9 on at least 4 of the 5 noisy crops, on all others)."""
    pose_dev, jac_dev, jac_max, bwd_dev, exact_dev = 0.0, 0.0, 0.0, 0.0, 0.0
    G = ref.upstream(5, 23)
    for case in ref.solver_cases(mesh):
        q64, _, _, last = ref.solve_case(mesh, case)
        q32 = ref.solve_case(mesh, case, torch.float32)[0]
        good = last < 1e-9
        assert int(good.sum()) >= (4 if case["name"] == "noisy" else 5), (case["name"], last)
        dev = (q32.double() - q64)[good].abs().max().item()
        if case["name"].startswith("exact"):
            assert (q64 - case["p_star"]).abs().max().item() < 1e-8
            exact_dev = max(exact_dev, dev)
        c64, c32 = ref.case_chain(mesh, case), ref.case_chain(mesh, case, torch.float32)
        j64, j32 = c64.jacobian(case["p_star"])[1], c32.jacobian(case["p_star"].float())[1]
        jdev = (j32.double() - j64).abs().max().item()
        print("%s: fp32 restatement against fp64: pose %.3g, Jacobian %.3g (entries up to %.4g)" % (case["name"], dev, jdev, j64.abs().max().item()))
        pose_dev, jac_dev, jac_max = max(pose_dev, dev), max(jac_dev, jdev), max(jac_max, j64.abs().max().item())
        if case["name"] != "noisy":                            # (the GPU tests take the backward at these three)
            p = case["p_star"].float()
            b64 = ref.backward(c64, p.double(), G, case["weights"], case["stiffness"])
            b32 = ref.backward(c32, p, G.float(), case["weights"], case["stiffness"])
            bdev = (b32.double() - b64).abs().max().item()
            print("    backward %.3g (entries up to %.3g)" % (bdev, b64.abs().max().item()))
            bwd_dev = max(bwd_dev, bdev)
    print("worst: pose %.3g, Jacobian %.3g (entries up to %.4g), backward %.3g" % (pose_dev, jac_dev, jac_max, bwd_dev))
    assert FP32_POSE_DEVIATION / 2 <= pose_dev <= 2 * FP32_POSE_DEVIATION
    assert FP32_EXACT_POSE_DEVIATION / 2 <= exact_dev <= 2 * FP32_EXACT_POSE_DEVIATION
    assert FP32_JACOBIAN_DEVIATION / 2 <= jac_dev <= 2 * FP32_JACOBIAN_DEVIATION
    assert FP32_BACKWARD_DEVIATION / 2 <= bwd_dev <= 2 * FP32_BACKWARD_DEVIATION
