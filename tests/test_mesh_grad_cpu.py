"""The differentiable mesh depth without a GPU: the torch restatement of its gradient (tests/mesh_grad_ref.py) against
finite differences and ATen's bilinear resize, the C ABI's new entries, the backward unit's resources, and the
DepthRender switch's size check."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_grad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("shr_mesh_depth_owner_fwd", "shr_mesh_depth_bwd", "shr_mesh_depth_bwd_workspace_bytes", "shr_lbs_project_bwd")


def _random_faces(rng, n):
    """n non-degenerate faces in pixel space, each with a source pixel strictly inside it (all weights in (0, 1))."""
    verts, pix = [], []
    while len(pix) < n:
        c = rng.uniform(50, 590, 2)
        p = c + rng.uniform(-20, 20, (3, 2))
        z = rng.uniform(200, 600, 3)
        x, y = np.round(c).astype(int)
        fv = np.concatenate([p, z[:, None]], 1).astype(np.float32)
        ok, bary = ref.clamp_decisions(fv[ref.sort_order(fv[None])[0]][None], np.array([x]), np.array([y]))
        P = fv.astype(np.float64)
        area = abs((P[1, 0] - P[0, 0]) * (P[2, 1] - P[0, 1]) - (P[2, 0] - P[0, 0]) * (P[1, 1] - P[0, 1]))
        # interior with a margin: a finite-difference step cannot flip a clamp decision
        if ok.all() and area > 40 and bary.min() > 0.05:
            verts.append(fv)
            pix.append((x, y))
    return np.stack(verts), np.array(pix)


def test_helper_gradient_matches_finite_differences():
    rng = np.random.default_rng(3)
    fv, pix = _random_faces(rng, 24)
    vertices = torch.from_numpy(fv.reshape(1, -1, 3)).double().requires_grad_(True)
    faces = np.arange(3 * len(fv)).reshape(-1, 3)
    face = (np.zeros(len(fv), np.int64), np.arange(len(fv)))
    zp = ref.face_zp(vertices, faces, face, pix[:, 0], pix[:, 1])
    g = torch.autograd.grad(zp.sum(), vertices)[0].numpy()
    v = fv.reshape(1, -1, 3).astype(np.float64)
    h = 1e-4
    fd = np.zeros_like(v)
    for i in range(v.shape[1]):
        for d in range(3):
            vp, vm = v.copy(), v.copy()
            vp[0, i, d] += h
            vm[0, i, d] -= h
            fp = ref.face_zp(torch.from_numpy(vp), faces, face, pix[:, 0], pix[:, 1]).sum().item()
            fm = ref.face_zp(torch.from_numpy(vm), faces, face, pix[:, 0], pix[:, 1]).sum().item()
            fd[0, i, d] = (fp - fm) / (2 * h)
    assert np.abs(g).max() > 1e-3
    np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-6 * np.abs(fd).max())


@pytest.mark.parametrize("S", [32, 64, 128, 256])
def test_helper_taps_reproduce_interpolate(S):
    img = torch.rand(2, 1, 640, 640, generator=torch.Generator().manual_seed(S)) * 100
    want = torch.nn.functional.interpolate(img, size=(S, S), mode="bilinear", align_corners=False)[:, 0].double()
    xs, ys, w = ref.tap_grid(S)
    got = (img[:, 0].double()[:, torch.from_numpy(ys), torch.from_numpy(xs)] * torch.from_numpy(w)).sum(-1)
    assert w.min() >= 0 and np.allclose(w.sum(-1), 1.0)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-4)


def test_new_symbols_are_declared_exported_and_loaded():
    from spherehand_amd import _lib, build
    import ctypes
    header = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    h = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(h, s), s
        assert s in _lib.SIGNATURES, s
    assert _lib.ABI_VERSION == 23 and _lib.lib().shr_abi_version() == 23


def test_backward_unit_uses_no_scratch(tmp_path):
    from spherehand_amd import build
    out = str(tmp_path / "mesh_depth_bwd.s")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", "mesh_depth_bwd.hip")],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) >= 4 and max(sizes) == 0, sizes
    # every store, atomic and cache write-back is a vector-memory or LDS instruction: none goes through the scalar cache
    mnemonics = {l.split()[0] for l in text.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))}
    scalar_writes = [m for m in mnemonics if m.startswith("s_") and ("store" in m or "atomic" in m or m.endswith("_wb"))]
    assert not scalar_writes, scalar_writes
    assert any(m.startswith("global_atomic") for m in mnemonics) and any(m.startswith("global_store") for m in mnemonics)


def test_depth_render_differentiable_switch_checks_sizes():
    from spherehand_amd import hand_model
    from spherehand_amd.render import DepthRasterization, DepthRender
    mesh = hand_model.load_mesh()
    r = DepthRender(mesh, 64, differentiable=True)
    assert r.differentiable
    assert not DepthRender(mesh, 64).differentiable
    for bad in (400, 321, 0):
        with pytest.raises(ValueError):
            DepthRender(mesh, bad, differentiable=True)
    DepthRender(mesh, 400)                       # the default path keeps every size
    with pytest.raises(ValueError):
        DepthRasterization(64, 32, mesh["faces"], differentiable=True)
    assert DepthRasterization(256, 256, mesh["faces"], differentiable=True).differentiable
