"""The mesh pose fit without a device: the entries of the C ABI with their argument rules, the new unit's code-object
metadata, the torch restatement (tests/pose_icp_ref.py) and the properties that keep it honest -- its g is the autograd
gradient of 1/2 sum dist^2, its rows agree with central differences of the distance, its state machine does what the header
says -- and the fp32 bars the GPU tests (tests/test_pose_icp_gpu.py) hold the kernels to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_d2m_ref
import pose_icp_ref as ref
from conftest import ROOT
from test_pose_ik_cpu import _metadata

ENTRIES = ("shr_pose_icp_normal_workspace_bytes", "shr_pose_icp_normal", "shr_pose_lm_state_bytes", "shr_pose_lm_begin",
           "shr_pose_lm_step")

# The fp32 bars.  The restatement run with an fp32 chain (transforms, vertices, the rows' tangents, the trial pose) against
# the fp64 one on the GPU tests' own inputs (pose_icp_ref.cases), the largest deviation per quantity; the GPU tolerance is
# 4 x that, the project's margin for another, equally valid, order of the sums.  test_fp32_bars measures them again and
# holds the constants to within [1/2, 2] of the measurement.
FP32_A_DEVIATION = 6.8e-7       # max |A32 - A64| / max |A64| per crop, at the cases' params0, given the same maps
FP32_G_DEVIATION = 4.3e-6       # max |g32 - g64| / max |g64| per crop
FP32_COST_DEVIATION = 5.8e-7    # |cost32 - cost64| / cost64 of the two searches' maps
FP32_STEP_DEVIATION = 1.7e-5    # rad | mm: the first step, (M + lambda diag M)^-1 rhs, at params0
FP32_POSE_DEVIATION = 7.6e-5    # rad | mm: the final pose of the end-to-end case, on the crops both runs treat alike
FP32_CONVERGED_POSE_DEVIATION = 6.0e-8   # rad | mm: the final pose of pose_icp_ref.converged_case, all 5 crops (one ulp of an angle)
A_BAR, G_BAR, COST_BAR, STEP_BAR, POSE_BAR = (4 * FP32_A_DEVIATION, 4 * FP32_G_DEVIATION, 4 * FP32_COST_DEVIATION,
                                              4 * FP32_STEP_DEVIATION, 4 * FP32_POSE_DEVIATION)
CONVERGED_POSE_BAR = 4 * FP32_CONVERGED_POSE_DEVIATION
CONVERGED = 1e-6                # the end-to-end comparison takes the crops whose last restatement step is below this


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
    contract = text[text.index("Pose from observed depth points"):text.index("long long shr_pose_icp_normal_workspace_bytes(")]
    for cite in ("mesh/kinematicsTransformation.py:157-177", "mesh/pointTransformation.py:39-46", "mesh/render.py:93-142",
                 "NOT checked", "tiles of 1024", "[1e-9, 1e6]", "envelope", "760 doubles"):
        assert cite in contract, cite
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23
    assert lib.shr_pose_icp_normal_workspace_bytes(3, 48, 40) == 3 * 2 * 3072 and lib.shr_pose_icp_normal_workspace_bytes(2, 32, 32) == 2 * 3072
    assert lib.shr_pose_icp_normal_workspace_bytes(-1, 8, 8) == -1 and lib.shr_pose_icp_normal_workspace_bytes(0, 8, 8) == 0
    assert lib.shr_pose_lm_state_bytes(5) == 5 * 760 * 8 and lib.shr_pose_lm_state_bytes(-1) == -1
    # host-side argument rules (every call below returns before a launch)
    P = 1 << 20                                                    # a 16-byte aligned stand-in for a device address
    normal = [P] * 11 + [1, 2, 70, 24, 32, 32, 1.0, 0.0, 1.0, 0.0, 99.0, 50.0] + [P] * 5 + [None]
    bad = lambda i, val: lib.shr_pose_icp_normal(*(normal[:i] + [val] + normal[i + 1:]))   # noqa: E731
    assert bad(12, 0) == 0                                         # B == 0: nothing to do
    for i in list(range(11)) + [23, 24, 25, 26, 27]:
        assert bad(i, None) == -1, i
        assert bad(i, P + 2) == -1, i
    for i in (1, 6, 7, 10, 27):                                    # vertices, offset, offset_inv, skin_wv, workspace: 16 bytes
        assert bad(i, P + 4) == -1, i
    for i in (23, 24, 25):                                         # A, g, cost: 8 bytes
        assert bad(i, P + 4) == -1, i
    assert bad(12, -1) == -1 and bad(13, 0) == -1 and bad(14, -1) == -1 and bad(15, 0) == -1 and bad(16, 0) == -1
    assert bad(22, -1.0) == -1 and bad(22, float("nan")) == -1
    assert bad(12, 65536) == -2 and bad(15, 2049) == -2 and bad(16, 2049) == -2 and bad(13, (1 << 31) // 3 + 1) == -2
    big = list(normal)
    big[12], big[13] = 65535, 1 << 15                              # B NV above 2^30
    assert lib.shr_pose_icp_normal(*big) == -2
    faces0 = list(normal)
    faces0[2], faces0[14], faces0[12] = None, 0, 0                 # faces may be NULL when F == 0 (B == 0: no launch)
    assert lib.shr_pose_icp_normal(*faces0) == 0
    begin = [P, 2, 1e-3, P, P, None]
    bad = lambda i, val: lib.shr_pose_lm_begin(*(begin[:i] + [val] + begin[i + 1:]))   # noqa: E731
    assert bad(1, 0) == 0 and bad(1, -1) == -1 and bad(1, (1 << 24) + 1) == -2
    for i in (0, 3, 4):
        assert bad(i, None) == -1 and bad(i, P + 2) == -1, i
    assert bad(3, P + 4) == -1                                     # state: 8 bytes
    assert bad(2, 0.0) == -1 and bad(2, -1.0) == -1 and bad(2, float("nan")) == -1
    step = [P, P, P, P, P, None, None, 1, 2, P, P, P, P, None]
    bad = lambda i, val: lib.shr_pose_lm_step(*(step[:i] + [val] + step[i + 1:]))   # noqa: E731
    assert bad(8, 0) == 0 and bad(8, -1) == -1 and bad(8, (1 << 24) + 1) == -2
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12):
        assert bad(i, None) == -1 and bad(i, P + 2) == -1, i
    for i in (0, 1, 2, 3):
        assert bad(i, P + 4) == -1, i
    assert bad(5, P + 2) == -1 and bad(6, P + 2) == -1             # prior, stiffness: optional, 4 bytes when given
    no_solve = list(step)
    no_solve[7], no_solve[9], no_solve[8] = 0, None, 0             # solve == 0: trial_out may be NULL
    assert lib.shr_pose_lm_step(*no_solve) == 0
    no_solve[8], no_solve[0] = 2, None
    assert lib.shr_pose_lm_step(*no_solve) == -1


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_pose_ik_cpu.py's reading of the code-object metadata.  pose_icp.hip: four kernels, no scratch, no spills.
    The tiles kernel holds the crop's transforms and tangents, 256 rows of 27 floats and two vectors of 256 doubles in LDS:
    35 536 bytes (35 280 of the kernel's struct; 256 more appear with __syncthreads_or), four workgroups per CU by LDS; the step kernel A and its factor in fp64: 11 032 bytes.  pose_ik.hip and
    mesh_d2m.hip, which now share lm_solve.h and d2m_tap.h with it, keep their kernels (tests/test_pose_ik_cpu.py and
    tests/test_mesh_d2m_cpu.py assert their figures).  DESIGN.md 4.4n has the table."""
    sizes, kernels = _metadata("pose_icp", tmp_path)
    assert len(sizes) == 4 and max(sizes) == 0, sizes
    assert len(kernels) == 4
    lds = {"pose_icp_tiles_kernel": 23 * 12 + 12 + 68 * 16 + 135 * 16 + 256 * 27 * 4 + 2 * 256 * 8 + 256,   # (+ 256: __syncthreads_or's)
           "pose_icp_reduce_kernel": 0, "pose_lm_begin_kernel": 0, "pose_lm_step_kernel": (2 * 676 + 26 + 1) * 8}
    assert lds["pose_icp_tiles_kernel"] == 35536 and lds["pose_lm_step_kernel"] == 11032
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4n"):design.index("### 4.5 ")]
    for name, k in kernels.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        short = [n for n in lds if n in name]
        assert len(short) == 1, name
        assert k["group_segment_fixed_size"] == lds[short[0]], name
        assert k["vgpr_count"] <= 128, name
        assert short[0] in section, short[0]
    assert "35 536" in section and "11 032" in section


def test_g_is_the_autograd_gradient(mesh):
    """The identity the feature rests on: g = sum d_i J_i is the gradient of 1/2 sum dist^2 over the contributing points,
    through the restated distance and skinning, by reverse-mode autograd (the rows come from forward mode)."""
    for case in ref.cached_cases(mesh):
        m, obs, p = case["model"], case["observed"], case["params0"]
        v = m.vertices(p).detach()
        dist, face = ref.search(m, obs, v, case["p2m"])
        A, g, cost, count = ref.normal(m, obs, p, dist, face, case["p2m"])
        q = p.clone().requires_grad_(True)
        pts = ref.points(m, obs, v.numpy(), dist, face, case["p2m"])
        d = ref.distances(m, q, pts)
        (0.5 * (d * d).sum()).backward()
        err, scale = (q.grad - g).abs().max().item(), g.abs().max().item()
        print("%s: %s rows; |g - autograd| %.3g of %.3g" % (case["name"], count.tolist(), err, scale))
        assert int(count.min()) >= 40 and err < 1e-12 * scale
        assert torch.equal(A, A.transpose(1, 2)) and bool((torch.linalg.eigvalsh(A)[:, 0] > -1e-9 * scale).all())
        assert torch.allclose(cost, torch.as_tensor(dist.astype(np.float64) ** 2).sum((1, 2)))


def test_rows_against_central_differences(mesh):
    """d(p + h t) - d(p - h t) over 2 h against J t for random directions t, d the TRUE distance (the closest point
    recomputed on the perturbed mesh), on the points whose closest face and region are the same at p, p + h t and
    p - h t (synthetic table: every face for every point is cheap): the discrepancy is the differences' own second-order
    term, it falls by 4 from h = 2^-14 to h / 2 (points at least 1 mm from the mesh: the term grows as |J|^3 / d^2)."""
    case = [c for c in ref.cached_cases(mesh) if c["name"] == "synthetic"][0]
    m, obs, p, p2m = case["model"], case["observed"], case["params0"], case["p2m"]
    gen = torch.Generator().manual_seed(5)

    def closest(q):
        v = m.vertices(q).detach().numpy()[..., :3]
        b, i, j, y = mesh_d2m_ref.points32(obs, p2m, ref.FG_MAX)
        tri = v[b[:, None, None], m.faces.astype(np.int64)[None]]               # [N,F,3,3]
        ab, ac, ap = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], y.astype(np.float64)[:, None] - tri[:, :, 0]
        vv, ww = mesh_d2m_ref.closest64(ab, ac, ap)
        e = ap - (vv[..., None] * ab + ww[..., None] * ac)
        d = np.sqrt((e * e).sum(-1))
        f = d.argmin(1)
        n = np.arange(len(f))
        return d[n, f], f, ref.region(vv[n, f], ww[n, f]), (b, y, vv[n, f], ww[n, f])

    d0, f0, r0, (b, y, vv, ww) = closest(p)
    keep0 = (d0 > 1.0) & (d0 < ref.MAX_DIST)
    ids = m.faces.astype(np.int64)[f0]
    pts = (b[keep0], y[keep0].astype(np.float64), ids[keep0], np.stack([(1 - vv) - ww, vv, ww], -1)[keep0])
    _, J = ref.rows(m, p, pts)
    errs = []
    directions = [torch.randn(p.shape, generator=gen, dtype=torch.float64) for _ in range(3)]
    for h in (2.0 ** -14, 2.0 ** -15):
        worst, used = 0.0, 0
        for t in directions:
            t = t / t.norm(dim=1, keepdim=True)
            up, fu, ru, _ = closest(p + 2.0 ** -14 * t)
            dn, fd, rd, _ = closest(p - 2.0 ** -14 * t)
            same = ((fu == f0) & (fd == f0) & (ru == r0) & (rd == r0))[keep0]
            if h != 2.0 ** -14:
                up, dn = closest(p + h * t)[0], closest(p - h * t)[0]
            fd_ = torch.as_tensor((up - dn)[keep0] / (2 * h))
            jt = (J * t[torch.as_tensor(pts[0])]).sum(-1)
            worst = max(worst, (fd_ - jt)[torch.as_tensor(same)].abs().max().item())
            used += int(same.sum())
        errs.append(worst)
    print("|fd - J t| %.3g at h = 2^-14, %.3g at h / 2: ratio %.2f over %d point-directions; largest |J| %.3g"
          % (errs[0], errs[1], errs[0] / errs[1], used, J.abs().max().item()))
    assert used > 300 and 3.5 < errs[0] / errs[1] < 4.5 and errs[1] < 1e-3 * J.abs().max().item()


def test_lm_state_machine():
    """The restatement's begin / step on pose_icp_ref.lm_scripts: the decisions and lambda as the header states them."""
    (s0, lm0), (s1, lm1), (s2, lm2) = (ref.run_script(s) for s in ref.lm_scripts())
    accept = torch.stack([s[2] for s in s0]).t().tolist()
    assert accept == [[True, True, True, True], [True, False, False, True], [False, True, False, True],
                      [True, True, True, True]]
    lam = torch.stack([s[1] for s in s0]).t()
    expect = torch.tensor([[1e-3, 3e-4, 9e-5, 2.7e-5], [1e-3, 1e-2, 1e-1, 3e-2], [1e-2, 1e-2, 1e-1, 3e-2],
                           [1e-3, 3e-4, 9e-5, 2.7e-5]], dtype=torch.float64)
    assert torch.allclose(lam, expect, rtol=1e-7, atol=0)             # (lambda0 is an fp32 argument: 1e-3 to 5e-8)
    lm_p0 = ref.lm_scripts()[0][1]
    # crop 3: A = -I is not positive definite -> every trial is the accepted pose; crop 2's first cost is a NaN
    for k in range(3):
        assert torch.equal(s0[k][0][3], s0[k][3][3])
        assert not torch.equal(s0[k][0][0], s0[k][3][0])
    assert torch.equal(s0[0][3][2], lm_p0[2]) and s0[0][4][2].item() == float("inf") and bool(torch.isnan(lm0.cost0[2]))
    assert s0[3][0] is None                                        # solve = 0
    assert lm0.accepts.tolist() == [4, 2, 2, 4] and lm0.rejects.tolist() == [0, 2, 2, 0]
    assert torch.allclose(torch.stack([s[1] for s in s1]).flatten(), torch.tensor([2e-9, 1e-9, 1e-9], dtype=torch.float64), rtol=1e-7)
    assert torch.allclose(torch.stack([s[1] for s in s2]).flatten(), torch.tensor([5e5, 1e6, 1e6], dtype=torch.float64), rtol=1e-7)
    # the total: cost_data + the stiffness term in index order; a step: (M + lambda diag M) delta = -(g + mu (p - prior))
    lam0, p0, prior, mu, steps = ref.lm_scripts()[0]
    A, g, cost, _ = steps[0]
    M = A[0] + torch.diag(mu)
    delta = torch.linalg.solve(M + float(np.float32(1e-3)) * torch.diag(torch.diagonal(M)), -(g[0] + mu * (p0[0] - prior[0])))
    assert torch.allclose(s0[0][0][0], (p0[0] + delta).float().double(), rtol=0, atol=1e-7)
    assert abs(s0[0][4][0].item() - (10.0 + (mu * (p0[0] - prior[0]) ** 2).sum().item())) < 1e-12


def test_ops_refuse_what_the_kernels_do_not_take(mesh):
    """No device here: the ops refuse CPU tensors with a RuntimeError; the module's tables."""
    from spherehand_amd import ops
    from spherehand_amd.render import MeshDataToModelLoss, MeshPoseFitter
    fit = MeshPoseFitter(mesh, 48, 40, stiffness=ref.STIFFNESS)
    assert fit.iters == 10 and fit.lambda0 == 1e-3 and fit.right_hand and fit.max_dist == 50.0
    assert fit.pixel_to_model == MeshDataToModelLoss.reference_grid(48, 40) == ref.grid(48, 40)
    assert fit.fg_max == MeshDataToModelLoss.REFERENCE_FG_MAX == ref.FG_MAX
    assert fit.vertices.num_vertices == 1721 and tuple(fit.faces_i32.shape) == (3382, 3) and fit.faces_i32.dtype == torch.int32
    assert tuple(fit.stiffness.shape) == (26,) and MeshPoseFitter(mesh, 8, 8).stiffness is None
    model = ref.hand_model(mesh)
    assert np.array_equal(fit.faces_i32.numpy(), model.faces)
    assert np.array_equal(fit.vertices.lbs.skin_bone.numpy(), model.table[1])
    for word in ("KeypointPoseSolver", "previous frame", "NO autograd"):
        assert word in MeshPoseFitter.__doc__, word
    obs, p0 = torch.full((2, 40, 48), 100.0), torch.zeros(2, 26)
    with pytest.raises(RuntimeError):
        fit.solve(obs, p0)
    with pytest.raises(RuntimeError):
        fit.normal_equations(obs, p0)
    with pytest.raises(RuntimeError):
        fit.solve(obs[:, :8], p0)
    with pytest.raises(RuntimeError):
        ops.pose_lm_begin(p0)
    with pytest.raises(RuntimeError):
        ops.pose_lm_step(torch.zeros(2 * 760, dtype=torch.float64), torch.zeros(2, 26, 26, dtype=torch.float64),
                         torch.zeros(2, 26, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), p0)


def converged_runs(case):
    """dtype -> pose_icp_ref.solve of the converged case (the GPU test runs the same)."""
    p0 = case["params0"].float().double()
    return {dt: ref.solve(case["model"].to(dt), case["observed"], p0, case["p2m"], case["iters"], stiffness=case["stiffness"],
                          prior=case["prior"]) for dt in (torch.float64, torch.float32)}


def fp32_deviations(mesh):
    """The figures, measured: (A, g, cost, step, pose, converged), and `kept`: the crops of pose_icp_ref.converged_case
    whose last fp64 step is below CONVERGED and whose accept sequence the fp32 run reproduces; `converged` is the pose
    figure over them.  `pose` is that of the END_TO_END case (the documented stiffness, 10 iterations, where no step gets
    below CONVERGED), over the crops whose accept sequence the fp32 run reproduces: two runs that decide alike stay within it."""
    dev = dict(A=0.0, g=0.0, cost=0.0, step=0.0, pose=0.0, converged=0.0)
    runs = [(case, ref.MAX_DIST) for case in ref.cached_cases(mesh)]
    runs.append(([c for c in ref.cached_cases(mesh) if c["name"] == SATURATED[0]][0], SATURATED[1]))
    for case, max_dist in runs:
        m64, m32 = case["model"], case["model"].to(torch.float32)
        obs, p, p2m, mu = case["observed"], case["params0"].float().double(), case["p2m"], case["stiffness"]
        out = {}
        for m in (m64, m32):
            v = m.vertices(p).detach()
            dist, face = ref.search(m, obs, v, p2m, max_dist=max_dist)
            if m is m32:                                           # the same maps for A and g: the fp64 search's
                A, g, _, _ = ref.normal(m, obs, p, out[m64][4], out[m64][5], p2m, max_dist=max_dist)
                cost = ref.normal(m, obs, p, dist, face, p2m, max_dist=max_dist)[2]
            else:
                A, g, cost, _ = ref.normal(m, obs, p, dist, face, p2m, max_dist=max_dist)
            lm = ref.LM(p, 1e-3, m.dtype)
            trial = lm.step(A, g, cost, p, None, mu, True)
            out[m] = (A, g, cost, trial - p, dist, face)
        a, b = out[m64], out[m32]
        dev["A"] = max(dev["A"], ((a[0] - b[0]).abs().amax((1, 2)) / a[0].abs().amax((1, 2))).max().item())
        dev["g"] = max(dev["g"], ((a[1] - b[1]).abs().amax(1) / a[1].abs().amax(1)).max().item())
        dev["cost"] = max(dev["cost"], ((a[2] - b[2]).abs() / a[2]).max().item())
        dev["step"] = max(dev["step"], (a[3] - b[3]).abs().max().item())
        print("%s, max_dist %g: A %.3g, g %.3g, cost %.3g, step %.3g so far" % (case["name"], max_dist, dev["A"], dev["g"], dev["cost"], dev["step"]))
        if max_dist != ref.MAX_DIST:
            continue
        if case["name"] == END_TO_END:
            q64, _, _, lm64 = ref.solve(m64, obs, p, p2m, case["iters"], stiffness=mu)
            q32, _, _, lm32 = ref.solve(m32, obs, p, p2m, case["iters"], stiffness=mu)
            same = (torch.stack(lm64.history) == torch.stack(lm32.history)).all(0)
            print("%s: last fp64 step %s; the fp32 run reproduces the accept sequence: %s" % (case["name"], lm64.last_step.tolist(), same.tolist()))
            dev["pose"] = (q64 - q32)[same].abs().max().item() if bool(same.any()) else float("nan")
    case = ref.cached_converged(mesh)
    run = converged_runs(case)
    (q64, _, _, lm64), (q32, _, _, lm32) = run[torch.float64], run[torch.float32]
    same = (torch.stack(lm64.history) == torch.stack(lm32.history)).all(0)
    kept = same & (lm64.last_step < CONVERGED)
    print("%s: last fp64 step %s; the fp32 run reproduces the accept sequence: %s" % (case["name"], lm64.last_step.tolist(), same.tolist()))
    dev["converged"] = (q64 - q32)[kept].abs().max().item() if bool(kept.any()) else float("nan")
    return dev, kept


END_TO_END = "hand_left"
SATURATED = ("hand_left", 3.0)       # the case and max_dist of the GPU test of saturated points: measured with the others


def test_fp32_bars(mesh):
    """The constants above, measured again.  The converged case keeps all 5 crops in this CPU run alone: the condition its
    set-up was chosen under (tests/test_pose_icp_gpu.py::test_end_to_end may lose one)."""
    dev, kept = fp32_deviations(mesh)
    print("fp32 against fp64: A %.3g, g %.3g, cost %.3g, step %.3g, pose %.3g, converged pose %.3g; kept %s"
          % (dev["A"], dev["g"], dev["cost"], dev["step"], dev["pose"], dev["converged"], kept.tolist()))
    assert bool(kept.all())
    for name, const in (("A", FP32_A_DEVIATION), ("g", FP32_G_DEVIATION), ("cost", FP32_COST_DEVIATION),
                        ("step", FP32_STEP_DEVIATION), ("pose", FP32_POSE_DEVIATION),
                        ("converged", FP32_CONVERGED_POSE_DEVIATION)):
        assert const / 2 <= dev[name] <= 2 * const, (name, dev[name], const)
