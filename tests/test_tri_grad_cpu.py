"""The triangle raster's backward at its own resolution without a GPU: the torch restatement (tests/tri_grad_ref.py)
against finite differences, the C ABI's new entries, the argument checks, the kernels' resources, and
TriangleDepthRaster's winding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_grad_ref
import tri_grad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("shr_tri_raster_owner_fwd", "shr_tri_raster_indexed_owner_fwd", "shr_tri_raster_bwd_workspace_bytes",
               "shr_tri_raster_indexed_bwd_workspace_bytes", "shr_tri_raster_bwd", "shr_tri_raster_indexed_bwd")


def test_helper_gradient_matches_finite_differences():
    """pixel_depth on faces whose pixel lies strictly inside (every weight in (0.05, 1)): autograd = central differences."""
    rng = np.random.default_rng(7)
    fv, pix = [], []
    while len(fv) < 16:
        c = rng.uniform(10, 50, 2)
        p = c + rng.uniform(-8, 8, (3, 2))
        f = np.concatenate([p, rng.uniform(20, 90, (3, 1))], 1).astype(np.float32)
        x, y = np.round(c).astype(int)
        ok, w = mesh_grad_ref.clamp_decisions(f[mesh_grad_ref.sort_order(f[None])[0]][None], np.array([x]), np.array([y]))
        if ok.all() and w.min() > 0.05:
            fv.append(f)
            pix.append((x, y))
    fv, pix = np.stack(fv), np.array(pix)
    verts, faces = ref.soup_as_indexed(fv[None])
    owner = np.full((1, 64, 64), -1, np.int32)
    keep = []
    for f, (x, y) in enumerate(pix):
        if owner[0, y, x] < 0:
            owner[0, y, x] = f
            keep.append(f)
    g = np.random.default_rng(1).standard_normal((1, 64, 64))
    v = torch.from_numpy(verts.astype(np.float64)).requires_grad_(True)
    (ref.pixel_depth(v, faces, owner) * torch.from_numpy(g)).sum().backward()
    fd = np.zeros_like(verts, np.float64)
    h = 1e-4
    for i in range(verts.shape[1]):
        for d in range(3):
            vp, vm = verts.astype(np.float64), verts.astype(np.float64)
            vp[0, i, d] += h
            vm[0, i, d] -= h
            fp = (ref.pixel_depth(torch.from_numpy(vp), faces, owner).numpy() * g).sum()
            fm = (ref.pixel_depth(torch.from_numpy(vm), faces, owner).numpy() * g).sum()
            fd[0, i, d] = (fp - fm) / (2 * h)
    assert len(keep) >= 8 and np.abs(fd).max() > 1e-3
    np.testing.assert_allclose(v.grad.numpy(), fd, rtol=1e-5, atol=1e-6 * np.abs(fd).max())


def test_new_symbols_are_declared_exported_and_loaded():
    from spherehand_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    h = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(h, s), s
        assert s in _lib.SIGNATURES, s
    assert _lib.ABI_VERSION == 23 and _lib.lib().shr_abi_version() == 23
    lib = _lib.lib()
    # workspace: crop maxima (256-byte rounded) + 3 x 8 bytes per accumulated point (a soup's 3 F corners)
    assert lib.shr_tri_raster_bwd_workspace_bytes(2, 10) == 256 + 2 * 30 * 24
    assert lib.shr_tri_raster_indexed_bwd_workspace_bytes(2, 10) == 256 + 2 * 10 * 24
    assert lib.shr_tri_raster_bwd_workspace_bytes(-1, 10) == -1


def test_entries_reject_bad_arguments_without_a_device():
    """Null pointers and bad sizes are refused before anything is launched (SHR_EINVAL / SHR_ETOOLARGE); B = 0 is a no-op."""
    from spherehand_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOLARGE = -1, -2
    assert lib.shr_tri_raster_owner_fwd(None, 0, 5, 8, 8, None, None, None) == 0
    assert lib.shr_tri_raster_owner_fwd(None, 1, 5, 8, 8, None, None, None) == EINVAL
    assert lib.shr_tri_raster_owner_fwd(16, 1, 5, 8, 0, 16, 16, None) == EINVAL
    assert lib.shr_tri_raster_owner_fwd(16, 1, 5, 70000, 8, 16, 16, None) == ETOOLARGE
    assert lib.shr_tri_raster_owner_fwd(16, 1, 5, 8, 8, 16, 20, None) == EINVAL                  # misaligned owner
    assert lib.shr_tri_raster_indexed_owner_fwd(16, None, 1, 4, 5, 8, 8, 16, 16, None) == EINVAL   # faces missing
    assert lib.shr_tri_raster_bwd(None, None, None, 0, 5, 8, 8, None, None, None) == 0
    assert lib.shr_tri_raster_bwd(16, 16, 16, 1, 5, 8, 8, 16, None, None) == EINVAL               # no workspace
    assert lib.shr_tri_raster_bwd(16, 16, 16, 70000, 5, 8, 8, 16, 16, None) == ETOOLARGE
    assert lib.shr_tri_raster_indexed_bwd(16, 16, 16, 16, 1, 0, 5, 8, 8, 16, 16, None) == EINVAL  # NV = 0
    assert lib.shr_tri_raster_indexed_bwd(16, 16, 16, 16, 1, 4, 5, 8, 8, 16, 24, None) == EINVAL  # misaligned workspace


def test_wrappers_check_their_inputs():
    """CPU tensors, non-contiguous tensors and wrong dtypes raise RuntimeError (the reference's CHECK_INPUT)."""
    from spherehand_amd import ops
    fv = torch.zeros(1, 4, 3, 3)
    verts, faces = torch.zeros(1, 12, 4), torch.arange(12, dtype=torch.int32).view(4, 3)
    own, g = torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8)
    calls = [lambda: ops.tri_raster_owner_fwd(8, 8, fv),
             lambda: ops.tri_raster_owner_fwd(8, 8, torch.zeros(1, 3, 4, 3).transpose(1, 2)),
             lambda: ops.tri_raster_owner_fwd(8, 8, fv.double()),
             lambda: ops.tri_raster_indexed_owner_fwd(8, 8, verts, faces),
             lambda: ops.tri_raster_indexed_owner_fwd(8, 8, verts, faces.long()),
             lambda: ops.tri_raster_bwd(fv, own, g),
             lambda: ops.tri_raster_indexed_bwd(verts, faces, own, g),
             lambda: ops.TriRaster.apply(fv.requires_grad_(True), 8, 8),
             lambda: ops.TriRasterIndexed.apply(verts[..., :3].requires_grad_(True), faces, 8, 8)]
    for k, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
        assert k >= 0


def _asm(unit, tmp_path):
    from spherehand_amd import build
    out = str(tmp_path / (unit + ".s"))
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", unit + ".hip")],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def _descriptors(text):
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                     for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")}
    return out


def test_backward_unit_uses_no_scratch_and_no_scalar_stores(tmp_path):
    text = _asm("mesh_depth_bwd", tmp_path)
    d = _descriptors(text)
    pixel = [n for n in d if "PixelTaps" in n]
    assert len(pixel) >= 6, sorted(d)               # max + sum for face soups and indexed meshes, LDS and global sums
    assert len([n for n in d if "mesh_bwd_finish_kernel" in n]) == 2
    sizes = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == len(d) and max(sizes) == 0, sizes
    mnemonics = {l.split()[0] for l in text.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))}
    scalar_writes = [m for m in mnemonics if m.startswith("s_") and ("store" in m or "atomic" in m or m.endswith("_wb"))]
    assert not scalar_writes, scalar_writes


def test_owner_raster_keeps_the_band_kernels_budget(tmp_path):
    """The owner band kernel (64-bit LDS cells): no scratch, LDS minima (ds_min_u64, not flat atomics), and no more VGPRs
    than the depth-only band kernel of the same input layout -- the same occupancy class (one 16-wave workgroup per CU)."""
    text = _asm("tri_raster", tmp_path)
    d = _descriptors(text)
    band = lambda idx, resize, owner: "_ZN3shr15tri_band_kernelILb%dELb%dELb%dEE" % (idx, resize, owner)
    for idx in (0, 1):
        own = [v for n, v in d.items() if n.startswith(band(idx, 0, 1))]
        plain = [v for n, v in d.items() if n.startswith(band(idx, 0, 0))]
        assert len(own) == 1 and len(plain) == 1
        assert own[0]["private_segment_fixed_size"] == 0
        assert own[0]["vgpr_count"] <= max(64, plain[0]["vgpr_count"]), (own, plain)
    assert max(int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)) == 0
    assert "ds_min_u64" in text and "flat_atomic" not in text


def test_owned_tap_and_weight_chain_live_in_one_header():
    """The backwards' shared statements about one face at one owned pixel -- the checked gather, the owned tap's fp32
    decisions and fp64 weights, the chain from the three weights to the corners' x, y -- are defined once under csrc/, in
    tri_tap.h, and the copies the units kept of each other are gone; no call of fixed_point_bwd is written once per RUNS."""
    csrc = os.path.join(ROOT, "spherehand_amd", "csrc")
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip"))}
    count = lambda pat: {n: len(re.findall(pat, t)) for n, t in texts.items() if re.search(pat, t)}   # noqa: E731
    assert count(r"\bbool tri_corners\(") == {"tri_tap.h": 1}
    assert count(r"\bfloat owned_tap\(") == {"tri_tap.h": 1}
    assert count(r"\bvoid weight_chain\(") == {"tri_tap.h": 1}
    assert count(r"\bstruct OwnedTap\b") == {"tri_tap.h": 1}
    assert count(r"kw \+= ") == {"tri_tap.h": 1}
    assert count(r"\.den = ") == {"tri_tap.h": 1}                      # the fp64 preamble: 2 x the signed area, once
    for gone in (r"\baa_corners\b", r"\binterp_corners\b", r"T\.den = ", r"\? fixed_point_bwd<"):
        assert not count(gone), gone
    # every unit of the family takes the header, and every caller of the gather, the tap and the chain is one of them
    for unit in ("mesh_depth_bwd.hip", "tri_interp.hip", "tri_antialias.hip"):
        assert '#include "tri_tap.h"' in texts[unit], unit
    assert set(count(r"\btri_corners\(")) == {"tri_tap.h", "mesh_depth_bwd.hip", "tri_interp.hip", "tri_antialias.hip"}
    assert set(count(r"\bowned_tap\(")) == {"tri_tap.h", "mesh_depth_bwd.hip", "tri_interp.hip"}
    assert set(count(r"\bweight_chain\(")) == {"tri_tap.h", "mesh_depth_bwd.hip", "tri_interp.hip"}
    assert count(r"\bint with_runs\(") == {"fixed_point.h": 1}
    assert count(r"\bint tri_raster_limits\(") == {"tri_raster.hip": 1} and len(re.findall(r"tri_raster_limits\(", texts["tri_raster.hip"])) == 5


def test_triangle_depth_raster_swaps_the_right_hands_winding():
    from spherehand_amd import hand_model
    from spherehand_amd.render import TriangleDepthRaster
    mesh = hand_model.load_mesh()
    faces = np.asarray(mesh["faces"])
    before = faces.copy()
    r, l = TriangleDepthRaster(640, 480, faces), TriangleDepthRaster(640, 480, faces, right_hand=False)
    assert np.array_equal(faces, before)
    assert np.array_equal(r.faces_i32.numpy(), faces[:, [1, 0, 2]]) and np.array_equal(l.faces_i32.numpy(), faces)
    assert r.faces_i32.dtype == torch.int32 and r.faces_i32.is_contiguous()
