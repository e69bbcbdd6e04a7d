"""The antialias pass over multi-channel maps without a GPU: the C ABI's new entries, their argument checks, the
wrappers' checks, and that the pass is stated once (tri_antialias.hip's kernel resources are checked by
tests/test_tri_aa_cpu.py)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("shr_tri_antialias_maps_fwd", "shr_tri_antialias_maps_bwd_workspace_bytes", "shr_tri_antialias_maps_bwd")


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
    # no pre-pass, no term of its own: the single-plane pass's workspace
    for B, NV in ((2, 10), (1, 1721), (256, 10144), (0, 5)):
        assert lib.shr_tri_antialias_maps_bwd_workspace_bytes(B, NV) == lib.shr_tri_antialias_bwd_workspace_bytes(B, NV)
    assert lib.shr_tri_antialias_maps_bwd_workspace_bytes(2, 10) == 256 + 2 * 10 * 24
    assert lib.shr_tri_antialias_maps_bwd_workspace_bytes(-1, 10) == -1


def test_entries_reject_bad_arguments_without_a_device():
    from spherehand_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOLARGE = -1, -2
    fwd, bwd = lib.shr_tri_antialias_maps_fwd, lib.shr_tri_antialias_maps_bwd
    far = 1 << 20                                                                                       # an `out` clear of values
    assert fwd(None, None, None, None, None, None, 0, 4, 2, 8, 8, 3, None, None) == 0                   # B = 0: a no-op
    assert fwd(None, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, far, None) == EINVAL                         # no values
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, None, None) == EINVAL                          # no out
    assert fwd(16, 16, 16, 16, None, 16, 1, 4, 2, 8, 8, 3, far, None) == EINVAL                         # faces missing
    assert fwd(16, 16, 16, 16, 16, None, 1, 4, 2, 8, 8, 3, far, None) == EINVAL                         # edges missing
    assert fwd(16, 16, 16, 20, 16, 16, 1, 4, 2, 8, 8, 3, far, None) == EINVAL                           # misaligned vertices
    assert fwd(16, 16, 16, 16, 16, 16, 1, 0, 2, 8, 8, 3, far, None) == EINVAL                           # NV = 0
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 0, 3, far, None) == EINVAL                           # H = 0
    assert fwd(16, 16, 16, 16, 16, 16, 70000, 4, 2, 8, 8, 3, far, None) == ETOOLARGE
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 70000, 8, 3, far, None) == ETOOLARGE
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 0, far, None) == EINVAL                           # C = 0
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, -3, far, None) == EINVAL
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 65, far, None) == ETOOLARGE                       # C = 65
    assert fwd(4096, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, 4096, None) == EINVAL                        # out == values
    assert fwd(4096, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, 4096 + 4 * 3 * 64 - 4, None) == EINVAL       # ... or overlapping it
    assert bwd(None, None, None, None, None, None, 0, 4, 2, 8, 8, 3, None, None, None, None, None) == 0
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, None, 16, 16, 16, None) == EINVAL              # no grad_out
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, 16, None, None, 16, None) == EINVAL            # no output at all
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, 16, 16, 16, None, None) == EINVAL              # no workspace
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, 16, 16, 16, 24, None) == EINVAL                # misaligned workspace
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 3, 16, 16, 20, 16, None) == EINVAL                # misaligned grad_vertices
    assert bwd(16, 16, 16, 16, 16, 16, 70000, 4, 2, 8, 8, 3, 16, 16, 16, 16, None) == ETOOLARGE
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 0, 16, 16, 16, 16, None) == EINVAL                # C = 0
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 65, 16, 16, 16, 16, None) == ETOOLARGE            # C = 65


def test_wrappers_check_their_inputs():
    """Shapes and types are checked before the device, so the messages can be told apart without one; a well-formed call
    on CPU tensors fails on the device alone."""
    from spherehand_amd import ops
    c, d = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8)
    own = torch.zeros(1, 8, 8, dtype=torch.int32)
    verts, faces = torch.zeros(1, 4, 4), torch.zeros(2, 3, dtype=torch.int32)
    edges = torch.zeros(2, 3, dtype=torch.int32)
    f = ops.tri_antialias_maps
    calls = [(lambda: f(c, d, own, verts, faces, edges), "CUDA"),                                   # device
             (lambda: f(c[0], d, own, verts, faces, edges), r"\[B,C,H,W\]"),                        # rank
             (lambda: f(c[:, 0], d, own, verts, faces, edges), r"\[B,C,H,W\]"),
             (lambda: f(c.double(), d, own, verts, faces, edges), "values must be torch.float32"),  # dtype
             (lambda: f(c, d, own.long(), verts, faces, edges), "owner must be torch.int32"),
             (lambda: f(c, d, own, verts, faces.long(), edges), "faces must be torch.int32"),
             (lambda: f(torch.zeros(1, 0, 8, 8), d, own, verts, faces, edges), "1 .. 64 channels"),  # C out of range
             (lambda: f(torch.zeros(1, 65, 8, 8), d, own, verts, faces, edges), "1 .. 64 channels"),
             (lambda: f(c, torch.zeros(1, 8, 9), own, verts, faces, edges), r"depth and owner must be \[B,H,W\]"),
             (lambda: f(c, d, torch.zeros(1, 3, 8, 8, dtype=torch.int32), verts, faces, edges),
              r"depth and owner must be \[B,H,W\]"),
             (lambda: f(c, d, own, torch.zeros(2, 4, 4), faces, edges), r"depth and owner must be \[B,H,W\]"),
             (lambda: f(c, d, own, verts[..., :3], faces, edges), r"vertices must be \[B,NV,4\]"),
             (lambda: f(c, d, own, verts, faces, edges[:1]), r"edges must be \[F,3\]"),
             (lambda: ops.tri_antialias_maps_bwd(c, d, own, verts, faces, edges, c), "CUDA"),
             (lambda: ops.tri_antialias_maps_bwd(c[0], d, own, verts, faces, edges, c), r"\[B,C,H,W\]"),
             (lambda: ops.TriAntialiasMaps.apply(c.clone().requires_grad_(True), d, own, verts, faces, edges), "CUDA"),
             (lambda: ops.TriAntialiasMaps.apply(c, d, own, torch.zeros(1, 4), faces, edges), r"\[B,NV,3\] or \[B,NV,4\]"),
             # the single-plane wrapper keeps its own errors on maps
             (lambda: ops.tri_antialias(c, d, own, verts, faces, edges), None)]
    for call, match in calls:
        with pytest.raises(RuntimeError, match=match):
            call()


def test_module_builds_the_depth_modules_tables():
    from spherehand_amd import hand_model
    from spherehand_amd.render import AntialiasedAttributeRaster, AntialiasedDepthRaster
    import numpy as np
    mesh = hand_model.load_mesh()
    faces, verts = np.asarray(mesh["faces"]), np.asarray(mesh["vertices"])
    before = faces.copy()
    for right in (True, False):
        a = AntialiasedAttributeRaster(640, 480, faces, right_hand=right, np_vertices=verts)
        d = AntialiasedDepthRaster(640, 480, faces, right_hand=right, np_vertices=verts)
        assert torch.equal(a.faces_i32, d.faces_i32) and torch.equal(a.edges_i32, d.edges_i32)
        assert a.clamp_max == 100.0 and (a.width, a.height) == (640, 480)
    assert np.array_equal(faces, before)
    with pytest.raises(RuntimeError):
        a(torch.zeros(4, 2), torch.zeros(4, 1))


def test_pair_decision_lives_in_one_file():
    """The pass is one unit: pair_blend, one pixel kernel template and one tap walker, each stated once under csrc/; the
    copies the pass, the raster's backward and the interpolation once kept of each other are gone."""
    csrc = os.path.join(ROOT, "spherehand_amd", "csrc")
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip"))}
    count = lambda pat: {n: len(re.findall(pat, t)) for n, t in texts.items() if re.search(pat, t)}   # noqa: E731
    assert count(r"PairBlend pair_blend\(") == {"tri_antialias.hip": 1}
    unit = texts["tri_antialias.hip"]
    for name in ("struct AAArgs", "struct PairBlend", "aa_sorts(", "aa_drawn(", "int aa_check("):
        assert name in unit, name
    # (the checked gather of a face's corners, once aa_corners here, is tri_tap.h's for every unit of the family)
    assert count(r"\bbool tri_corners\(") == {"tri_tap.h": 1} and "tri_corners(" in unit and not count(r"\baa_corners\b")
    assert "tri_antialias_maps.hip" not in texts and "tri_aa_pair.h" not in texts
    # one pixel kernel template and one tap walker of the pass, whatever their names
    assert count(r"__global__[^;{]*\baa_\w*pixel\w*\(") == {"tri_antialias.hip": 1}
    assert count(r"\bstruct AA\w*Taps\b") == {"tri_antialias.hip": 1}
    assert count(r"\baa_pixel_kernel\(") == {"tri_antialias.hip": 1} and count(r"\bstruct AATaps\b") == {"tri_antialias.hip": 1}
    # one bit bound and one pixel indexer for every fixed-point backward
    assert count(r"\bint fix_term_bits\(") == {"fixed_point.h": 1} and count(r"\bstruct PixelWalk\b") == {"fixed_point.h": 1}
    for gone in ("aa_maps_pixel_kernel", "AAMapsTaps", "each_pair", "raster_fix_bits", "interp_fix_bits", "aa_fix_bits",
                 "InterpWalk"):
        assert not count(r"\b%s\b" % gone), gone
