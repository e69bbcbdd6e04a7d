"""The differentiable skinning without a device: the dense torch restatement (tests/skin_ref.py) against the reference's
own vertices, its fp64 autograd chained after the torch forward kinematics against central differences over the 26 pose
parameters, the three entries of the C ABI with their argument rules, and the new kernels' code-object metadata."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import skin_ref
from conftest import ROOT, golden

ENTRIES = ("shr_lbs_vertices_bwd", "shr_pose_vertices_fwd", "shr_pose_vertices_bwd")
CAMERA = (320.0, 320.0, 640 / 300, 640 / 300)


@pytest.fixture(scope="module")
def mesh():
    from spherehand_amd import hand_model
    return hand_model.load_mesh()


def test_restatement_against_the_reference(mesh):
    """g2_mesh.npz holds the reference's skinned points, projected vertices and rand_f vertices of four poses (all 10 144
    records, right hand), fp32 results of its dense sum.  tests/test_mesh_gpu.py's tolerance for lbs_project_kernel,
    1e-4, is asserted for the fp64 restatement: what remains is the reference's own fp32 rounding (measured 2.9e-5 /
    8.5e-5 / 7.8e-5 in the three modes, coordinates up to 640: 1.4 units in the last place).  The fp32 restatement rounds
    as well, in another association; it is held to the fp64 one by the fp32 format's own bound for coordinates up to 640:
    the sum's last two roundings amplified by rand_f * fx <= 2.35, then the roundings of * rand_f, * fx and + cx, together
    8 half-units in the last place of 640, 8 * 2^-24 * 640 = 3.05e-4 (measured 1.13e-4 at worst; its distance from the
    reference's fp32 values, printed: 3.1e-5 / 9.2e-5 / 1.22e-4)."""
    from spherehand_amd import hand_model
    g = golden("g2_mesh.npz")
    start, bone, wv = hand_model.sparse_skin(mesh)
    exact = {}
    for dtype in (torch.float64, torch.float32):
        dense = skin_ref.dense_table(start, bone, wv, 17, dtype)
        T = torch.from_numpy(g["T"]).to(dtype)
        rf = torch.from_numpy(g["rand_f"]).to(dtype)
        for mode, (camera, rand_f, want) in enumerate(((None, None, g["skinned"]), (CAMERA, None, g["verts"]),
                                                       (CAMERA, rf, g["verts_rand_f"]))):
            out = skin_ref.skin(T, dense, True, camera, rand_f)
            assert out.dtype == dtype
            err = np.abs(out.numpy().astype(np.float64) - want).max()
            print("%s camera %s rand_f %s: max |restated - reference| %.3g" % (dtype, camera is not None, rand_f is not None, err))
            if dtype == torch.float64:
                exact[mode] = out.numpy()
                assert err <= 1e-4
            else:
                own = np.abs(out.numpy().astype(np.float64) - exact[mode]).max()
                print("    max |fp32 restated - fp64 restated| %.3g" % own)
                assert own <= 8 * 2.0 ** -24 * 640
    # the left hand keeps the sign of x, [B,NB,1,4,4] is the same input, the distinct table gives the same points
    left = skin_ref.skin(T, dense, False)
    right = skin_ref.skin(T, dense, True)
    assert torch.equal(left[..., 0], -right[..., 0]) and torch.equal(left[..., 1:], right[..., 1:])
    assert torch.equal(skin_ref.skin(T.unsqueeze(2), dense, True, CAMERA), skin_ref.skin(T, dense, True, CAMERA))
    ustart, ubone, uwv, index = hand_model.unique_skin(mesh)
    udense = skin_ref.dense_table(ustart, ubone, uwv, 17, torch.float32)
    assert torch.equal(skin_ref.skin(T, udense, True, CAMERA)[:, torch.from_numpy(index)], skin_ref.skin(T, dense, True, CAMERA))


def test_synthetic_table_has_the_rows_it_promises():
    start, bone, wv = skin_ref.synthetic_table()
    n = np.diff(start)
    assert len(start) == 71 and wv.shape == (start[-1], 4) and bone.min() == 0 and bone.max() == 16
    assert n[3] == 0 and n[40] == 0 and n[69] == 0 and n[5] == 17 and 1 not in bone
    assert list(bone[start[7]:start[8]]) == [2, 4, 4, 9] and list(bone[start[5]:start[6]][-2:]) == [16, 16]
    assert all(np.all(np.diff(bone[a:b]) >= 0) for a, b in zip(start[:-1], start[1:]))
    assert set(bone.tolist()) == set(range(17)) - {1}


@pytest.mark.parametrize("right_hand", (True, False))
@pytest.mark.parametrize("mode", ("model", "camera", "rand_f"))
def test_gradient_against_central_differences(mesh, mode, right_hand):
    """L(p) = <G, skin(FK(p))> in fp64, FK = HandTransformationMat.forward_torch: the autograd gradient against central
    differences over all 26 pose parameters at h = 2^-6 and h / 2.  The discrepancy is the differences' own second-order
    term, so it falls by 4 (the translation parameters enter linearly and contribute none); it stays below 1e-3 of the
    largest gradient entry (h^2 / 6 = 4e-5 times a third derivative of the size of the first: rotations)."""
    from spherehand_amd import hand_model, joint_angle
    from spherehand_amd.kinematicsTransformation import HandTransformationMat
    fk = HandTransformationMat([b["offset_matrix"].astype(np.float32) for b in mesh["bones"]]).double()
    start, bone, wv, _ = hand_model.unique_skin(mesh)
    dense = skin_ref.dense_table(start, bone, wv, 17)
    B = 2
    p0 = joint_angle.sample_poses(B, seed=5).double()
    gen = torch.Generator().manual_seed(3)
    G = torch.randn(B, dense.shape[1], 4, generator=gen, dtype=torch.float64)
    camera = None if mode == "model" else CAMERA
    rand_f = torch.tensor([0.93, 1.08], dtype=torch.float64) if mode == "rand_f" else None

    def L(p):
        return (skin_ref.skin(fk.forward_torch(p), dense, right_hand, camera, rand_f) * G).sum()

    p = p0.clone().requires_grad_(True)
    L(p).backward()
    analytic = p.grad.numpy()
    err = []
    for h in (2.0 ** -6, 2.0 ** -7):
        fd = np.zeros_like(analytic)
        for b in range(B):
            for k in range(26):
                up, dn = p0.clone(), p0.clone()
                up[b, k] += h
                dn[b, k] -= h
                with torch.no_grad():
                    fd[b, k] = (L(up).item() - L(dn).item()) / (2 * h)
        err.append(np.abs(fd - analytic).max())
    scale = np.abs(analytic).max()
    print("%s right_hand %s: |fd - autograd| %.3g at h = 2^-6, %.3g at h / 2: ratio %.2f; largest |gradient| %.3g"
          % (mode, right_hand, err[0], err[1], err[0] / err[1], scale))
    assert np.all(analytic != 0) and 3.5 < err[0] / err[1] < 4.5
    assert err[1] <= 1e-3 * scale


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    contract = text[text.index("Differentiable skinning of the mesh"):text.index("int shr_lbs_vertices_bwd(")]
    for cite in ("mesh/pointTransformation.py:39-46", ":84-99", "mesh/kinematicsTransformation.py:157-177"):
        assert cite in contract, cite
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23
    # host-side argument rules (every call below returns before a launch)
    A = 1 << 20                                                    # a 16-byte aligned stand-in for a device address
    lbs = [A, 2, 17, 70, A, A, A, 1, 1, 320.0, 320.0, 2.0, 2.0, None, A, None]
    bad = lambda i, val: lib.shr_lbs_vertices_bwd(*(lbs[:i] + [val] + lbs[i + 1:]))   # noqa: E731
    assert bad(1, 0) == 0 and bad(3, 0) == 0                       # B == 0, NV == 0: nothing to do
    for i in (0, 4, 5, 6, 14):
        assert bad(i, None) == -1, i
    assert bad(0, A + 8) == -1 and bad(6, A + 4) == -1 and bad(1, -1) == -1 and bad(2, 0) == -1 and bad(3, -1) == -1
    assert bad(1, (1 << 30) + 1) == -2
    for entry, last in ((lib.shr_pose_vertices_fwd, 15), (lib.shr_pose_vertices_bwd, 15)):
        args = [A, 2, A, A, 70, A, A, A, 1, 1, 320.0, 320.0, 2.0, 2.0, None, A, A, None]
        bad = lambda i, val: entry(*(args[:i] + [val] + args[i + 1:]))   # noqa: E731
        assert bad(1, 0) == 0 and bad(4, 0) == 0
        for i in (0, 2, 3, 5, 6, 7, 15):
            assert bad(i, None) == -1, i
        assert bad(7, A + 8) == -1 and bad(15, A + 8) == -1 and bad(2, A + 4) == -1 and bad(3, A + 4) == -1
        assert bad(1, -1) == -1 and bad(4, -1) == -1
        assert bad(1, (1 << 24) + 1) == -2 and bad(4, (1 << 30) + 1) == -2
    fwd = [A, 2, A, A, 70, A, A, A, 1, 1, 320.0, 320.0, 2.0, 2.0, None, A, A + 8, None]
    assert lib.shr_pose_vertices_fwd(*fwd) == -1                   # T given but not 16-byte aligned
    bwd = [A, 2, A, A, 70, A, A, A, 1, 1, 320.0, 320.0, 2.0, 2.0, None, A, None, None]
    assert lib.shr_pose_vertices_bwd(*bwd) == -1                   # grad_params NULL
    bwd[16] = A + 4
    assert lib.shr_pose_vertices_bwd(*bwd) == -1                   # ... or not 8-byte aligned


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


def test_units_compile_for_gfx950_without_scratch(tmp_path):
    """tests/test_depth_normals_cpu.py's reading of the code-object metadata.  pose_vertices.hip: two kernels, no scratch,
    no spills; the forward's LDS is the kLbsCrops x 17 matrices and the four sincos tables, the backward's the 51 gradient
    rows, the sincos table and the palm scratch; the backward's 16 waves fit a CU (<= 128 VGPRs).  lbs_project.hip keeps
    its two kernels (the backward took a flag, not a second instantiation).  DESIGN.md 4.4l has the figures."""
    sizes, kernels = _metadata("pose_vertices", tmp_path)
    assert len(sizes) == 2 and max(sizes) == 0, sizes
    assert len(kernels) == 2
    for name, k in kernels.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["vgpr_count"] <= 128, name
    fwd = next(k for n, k in kernels.items() if "pose_vertices_fwd_kernel" in n)
    bwd = next(k for n, k in kernels.items() if "pose_vertices_bwd_kernel" in n)
    assert fwd["group_segment_fixed_size"] == 4 * 17 * 64 + 4 * 23 * 12
    assert bwd["group_segment_fixed_size"] == 23 * 12 + 51 * 16 + 18 * 16
    sizes, kernels = _metadata("lbs_project", tmp_path)
    assert len(sizes) == 2 and max(sizes) == 0 and len(kernels) == 2, sizes
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4l"):design.index("### 4.5 ")]
    assert "pose_vertices_fwd_kernel" in section and "pose_vertices_bwd_kernel" in section


def test_modules_refuse_what_the_kernels_do_not_take(mesh):
    """No device here: the ops refuse CPU tensors with a RuntimeError; the module's tables, faces and rest vertices."""
    from spherehand_amd import hand_model, ops
    from spherehand_amd.render import MeshVertices
    assert MeshVertices.pixel_camera(640, 640) == (320.0, 320.0, 640 / 300, 640 / 300)
    assert MeshVertices.pixel_camera(64, 32) == (32.0, 16.0, 64 / 300, 32 / 300)
    mv = MeshVertices(mesh)
    assert mv.camera == MeshVertices.pixel_camera(640, 640) and mv.num_vertices == 1721
    faces = np.asarray(mesh["faces"], np.int64)
    assert mv.faces.dtype == np.int64 and mv.faces.shape == faces.shape and mv.faces.max() == 1720
    assert np.array_equal(mv.faces, mv.lbs.vertex_index[faces])
    rest = np.asarray(mesh["vertices"], np.float32)[:, :3] * np.array([-1, 1, 1], np.float32)
    assert mv.rest_vertices.shape == (1721, 3) and np.array_equal(mv.rest_vertices[mv.lbs.vertex_index], rest)
    full = MeshVertices(mesh, camera=None, right_hand=False, distinct=False)
    assert full.camera is None and full.num_vertices == 10144 and np.array_equal(full.faces, faces)
    assert np.array_equal(full.rest_vertices, np.asarray(mesh["vertices"], np.float32)[:, :3])
    T = torch.eye(4).repeat(2, 17, 1, 1).requires_grad_(True)
    lbs = mv.lbs
    with pytest.raises(RuntimeError):
        ops.SkinVertices.apply(T, lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv, True, None, None)
    off = torch.eye(4).repeat(17, 1, 1)
    with pytest.raises(RuntimeError):
        ops.PoseVertices.apply(torch.zeros(2, 26), off, off, lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv, True, None, None)
