"""The antialias pass without a GPU: the edge table on the welded hand, the winding swap, the C ABI's new entries, the
argument checks, the new unit's kernel resources, and the fp64 restatement (tests/tri_aa_ref.py) against finite
differences of itself."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tri_aa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("shr_tri_antialias_fwd", "shr_tri_antialias_bwd_workspace_bytes", "shr_tri_antialias_bwd")


def _hand():
    from spherehand_amd import hand_model
    mesh = hand_model.load_mesh()
    return np.asarray(mesh["faces"]), np.asarray(mesh["vertices"])


def test_welded_hand_edge_table():
    """1 721 welded points; 5 101 edges: 5 031 shared by two faces, 63 boundary, 7 shared by three (-1 on both sides)."""
    from spherehand_amd import ops
    faces, verts = _hand()
    sw = faces[:, [1, 0, 2]]
    e = ops.tri_edge_table(sw, verts)
    assert e.shape == faces.shape and e.dtype == np.int32
    rows = np.ascontiguousarray(verts)
    _, weld = np.unique(rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel(), return_inverse=True)
    assert weld.max() + 1 == 1721
    assert np.array_equal(ops.tri_edge_table(sw, weld.ravel()), e)                  # ids or positions: the same table
    F = len(faces)
    f, k = np.nonzero(e >= 0)
    assert len(f) == 2 * 5031 and (e == -1).sum() == 63 + 3 * 7
    # symmetric: the face across edge k of f has f across the same undirected (welded) edge
    w = weld.ravel()[sw]
    for a, kk in zip(f, k):
        n = e[a, kk]
        assert n != a and 0 <= n < F
        ks = [j for j in range(3) if e[n, j] == a]
        assert len(ks) == 1
        j = ks[0]
        assert {w[a, kk], w[a, (kk + 1) % 3]} == {w[n, j], w[n, (j + 1) % 3]}
    # without welding the reference's separate corners share (almost) nothing: nearly every edge is a silhouette
    assert (ops.tri_edge_table(sw) == -1).sum() > 10000


def test_edge_table_small_cases():
    from spherehand_amd import ops
    sq = np.array([[0, 1, 2], [0, 2, 3]])
    assert ops.tri_edge_table(sq).tolist() == [[-1, -1, 1], [0, -1, -1]]
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])                      # edge (0, 1) shared by three faces
    assert ops.tri_edge_table(fan).tolist() == [[-1, -1, -1]] * 3
    assert ops.tri_edge_table(np.zeros((0, 3), np.int64)).shape == (0, 3)
    with pytest.raises(RuntimeError):
        ops.tri_edge_table(np.zeros((4, 2)))


def test_antialiased_raster_swaps_the_right_hands_winding():
    from spherehand_amd import ops
    from spherehand_amd.render import AntialiasedDepthRaster
    faces, verts = _hand()
    before = faces.copy()
    r = AntialiasedDepthRaster(640, 480, faces, np_vertices=verts)
    l = AntialiasedDepthRaster(640, 480, faces, right_hand=False, np_vertices=verts)
    assert np.array_equal(faces, before)
    assert np.array_equal(r.faces_i32.numpy(), faces[:, [1, 0, 2]]) and np.array_equal(l.faces_i32.numpy(), faces)
    assert np.array_equal(r.edges_i32.numpy(), ops.tri_edge_table(faces[:, [1, 0, 2]], verts))
    assert np.array_equal(l.edges_i32.numpy(), ops.tri_edge_table(faces, verts))
    assert not np.array_equal(r.edges_i32.numpy(), l.edges_i32.numpy())         # edge k joins the SWAPPED corners k, k + 1
    assert r.edges_i32.dtype == torch.int32 and r.edges_i32.is_contiguous() and r.clamp_max == 100.0


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
    assert lib.shr_tri_antialias_bwd_workspace_bytes(2, 10) == 256 + 2 * 10 * 24
    assert lib.shr_tri_antialias_bwd_workspace_bytes(-1, 10) == -1


def test_entries_reject_bad_arguments_without_a_device():
    from spherehand_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOLARGE = -1, -2
    fwd, bwd = lib.shr_tri_antialias_fwd, lib.shr_tri_antialias_bwd
    assert fwd(None, None, None, None, None, None, 0, 4, 2, 8, 8, None, None) == 0                  # B = 0: a no-op
    assert fwd(None, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 16, None) == EINVAL                         # no values
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, None, None) == EINVAL                         # no out
    assert fwd(16, 16, 16, 16, None, 16, 1, 4, 2, 8, 8, 16, None) == EINVAL                         # faces missing
    assert fwd(16, 16, 16, 16, 16, None, 1, 4, 2, 8, 8, 16, None) == EINVAL                         # edges missing
    assert fwd(16, 16, 16, 20, 16, 16, 1, 4, 2, 8, 8, 16, None) == EINVAL                           # misaligned vertices
    assert fwd(16, 16, 16, 16, 16, 16, 1, 0, 2, 8, 8, 16, None) == EINVAL                           # NV = 0
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 0, 16, None) == EINVAL                           # H = 0
    assert fwd(16, 16, 16, 16, 16, 16, 70000, 4, 2, 8, 8, 16, None) == ETOOLARGE
    assert fwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 70000, 8, 16, None) == ETOOLARGE
    assert bwd(None, None, None, None, None, None, 0, 4, 2, 8, 8, None, None, None, None, None) == 0
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, None, 16, 16, 16, None) == EINVAL             # no grad_out
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 16, None, None, 16, None) == EINVAL           # no output at all
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 16, 16, 16, None, None) == EINVAL             # no workspace
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 16, 16, 16, 24, None) == EINVAL               # misaligned workspace
    assert bwd(16, 16, 16, 16, 16, 16, 1, 4, 2, 8, 8, 16, 16, 20, 16, None) == EINVAL               # misaligned grad_vertices
    assert bwd(16, 16, 16, 16, 16, 16, 70000, 4, 2, 8, 8, 16, 16, 16, 16, None) == ETOOLARGE


def test_wrappers_check_their_inputs():
    from spherehand_amd import ops
    c, d = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8)
    own = torch.zeros(1, 8, 8, dtype=torch.int32)
    verts, faces = torch.zeros(1, 4, 4), torch.zeros(2, 3, dtype=torch.int32)
    edges = torch.zeros(2, 3, dtype=torch.int32)
    calls = [lambda: ops.tri_antialias(c, d, own, verts, faces, edges),
             lambda: ops.tri_antialias(c.double(), d, own, verts, faces, edges),
             lambda: ops.tri_antialias(c, d, own.long(), verts, faces, edges),
             lambda: ops.tri_antialias_bwd(c, d, own, verts, faces, edges, c),
             lambda: ops.TriAntialias.apply(c.requires_grad_(True), d, own, verts, faces, edges),
             lambda: ops.TriAntialias.apply(c, d, own, torch.zeros(1, 4), faces, edges),
             lambda: ops.TriRasterIndexedOwner.apply(verts[..., :3].requires_grad_(True), faces, 8, 8)]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()


def _asm(unit, tmp_path):
    from spherehand_amd import build
    out = str(tmp_path / (unit + ".s"))
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", unit + ".hip")],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_antialias_pass_uses_no_scratch_and_no_scalar_stores(tmp_path):
    """The merged unit (one plane and maps): every kernel of the one pass."""
    text = _asm("tri_antialias", tmp_path)
    meta = text[text.index("amdhsa.kernels:"):]
    d = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        d[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in ("vgpr_count", "private_segment_fixed_size")}
    # the one pass: the pixel kernel with C a run-time argument and with C = 1 at compile time (the single plane), the tap
    # walker with a run-time C alone -- no second set of instances
    assert len([n for n in d if "aa_pixel_kernel" in n]) == 4                 # (forward, value gradient) x (C, 1)
    assert len([n for n in d if "AATaps" in n]) == 3                          # maximum, LDS sums, global sums
    assert len(d) == 4 + 3 + 2                                                # ... and fixed_point.h's clear and conversion
    assert all(v["private_segment_fixed_size"] == 0 for v in d.values()), d
    # one 16-wave workgroup of the fixed-point passes per CU at least; the pixel kernels at full occupancy
    assert all(v["vgpr_count"] <= 64 for n, v in d.items() if "AATaps" in n or "aa_pixel" in n), d
    sizes = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == len(d) and max(sizes) == 0, sizes
    mnemonics = {l.split()[0] for l in text.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))}
    scalar_writes = [m for m in mnemonics if m.startswith("s_") and ("store" in m or "atomic" in m or m.endswith("_wb"))]
    assert not scalar_writes, scalar_writes


def _scene(seed):
    """Two steep front-facing triangles over background in 24 x 20 (one shares an edge with the other) and the owner /
    depth a raster gives them (inside: the nearer face; smaller index on ties)."""
    rng = np.random.default_rng(seed)
    W, H = 24, 20
    v = np.array([[4.3, 2.6, 20.0, 1], [9.7, 3.4, 20.0, 1], [6.2, 16.8, 20.0, 1], [15.1, 15.9, 30.0, 1],
                  [13.6, 3.1, 25.0, 1], [20.4, 9.3, 25.0, 1], [17.8, 17.2, 25.0, 1]])
    v[:, :2] += rng.uniform(-0.3, 0.3, (7, 2))
    faces = np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6]])
    # front-facing by the kernel's cull: flip any face the fp32 test calls a back face
    for f in range(len(faces)):
        if not ref.drawn(v[None].astype(np.float32), faces[f:f + 1])[0, 0]:
            faces[f, [0, 1]] = faces[f, [1, 0]]
    owner = np.full((1, H, W), -1, np.int32)
    depth = np.full((1, H, W), 1000.0, np.float32)
    gy, gx = np.mgrid[0:H, 0:W].astype(np.float64)
    for f in range(len(faces)):
        p = v[faces[f], :2]
        s = [(p[(k + 1) % 3, 0] - p[k, 0]) * (gy - p[k, 1]) - (p[(k + 1) % 3, 1] - p[k, 1]) * (gx - p[k, 0]) for k in range(3)]
        inside = (np.sign(s[0]) == np.sign(s[1])) & (np.sign(s[1]) == np.sign(s[2]))
        z = np.float32(v[faces[f], 2].mean())
        take = inside & (z < depth[0])
        owner[0][take], depth[0][take] = f, z
    from spherehand_amd import ops
    return v[None].astype(np.float32), faces, ops.tri_edge_table(faces), owner, depth


def test_restatement_gradient_matches_finite_differences():
    for seed in range(3):
        v, faces, edges, owner, depth = _scene(seed)
        rng = np.random.default_rng(seed + 10)
        c = np.where(owner >= 0, depth, np.float32(100.0)) + rng.uniform(-1, 1, owner.shape)
        g = rng.standard_normal(owner.shape)
        out, info = ref.antialias(c, depth, owner, v, faces, edges)
        assert info["pairs"] > 20 and not info["ambiguous"].any()
        assert edges[0].tolist().count(1) == 1 and edges[1].tolist().count(0) == 1   # the shared edge is not a silhouette
        gc, gv = ref.grads(c, depth, owner, v, faces, edges, g)
        f = lambda vv, cc: (ref.antialias(cc, depth, owner, vv, faces, edges)[0].numpy() * g).sum()   # noqa: E731
        h = 1e-6
        fd = np.zeros(v.shape)
        for i in range(v.shape[1]):
            for d in range(3):
                vp, vm = v.astype(np.float64), v.astype(np.float64)
                vp[0, i, d] += h
                vm[0, i, d] -= h
                fd[0, i, d] = (f(vp, c) - f(vm, c)) / (2 * h)
        assert np.abs(fd[..., :2]).max() > 1.0 and np.all(fd[..., 2:] == 0) and np.all(gv[..., 2:] == 0)
        np.testing.assert_allclose(gv, fd, rtol=1e-5, atol=1e-5 * np.abs(fd).max())
        # values: linear, so one difference per probe is exact up to rounding
        for (b, y, x) in list(zip(*np.nonzero(info["touched"])))[:12]:
            cp, cm = c.copy(), c.copy()
            cp[b, y, x] += 1e-3
            cm[b, y, x] -= 1e-3
            assert isclose_(gc[b, y, x], (f(v, cp) - f(v, cm)) / 2e-3)
        untouched = ~info["touched"]
        assert np.array_equal(gc[untouched], g[untouched]) and np.array_equal(out.numpy()[untouched], c[untouched])


def isclose_(a, b):
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))
