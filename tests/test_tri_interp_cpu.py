"""Vertex-attribute interpolation without a GPU: the C ABI's new entries and their argument checks, the wrappers'
checks, the unit's kernel resources, hand_model.dense_skin_weights, and the two restatements of
tests/tri_interp_ref.py -- against each other, against central differences, and the identity that interpolating the
vertices' own (x, y) gives back the pixel."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tri_interp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("shr_tri_interp_fwd", "shr_tri_interp_bwd_workspace_bytes", "shr_tri_interp_bwd")
U = 2.0 ** -24


def test_new_symbols_are_declared_exported_and_loaded():
    from spherehand_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    h = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(h, s), s
        assert s in _lib.SIGNATURES, s
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23                     # additions only
    q = lib.shr_tri_interp_bwd_workspace_bytes
    assert q(-1, 10, 3, 1, 1) == -1 and q(2, -1, 3, 1, 1) == -1 and q(2, 10, -1, 1, 1) == -1
    assert q(2, 10, 3, 0, 0) == 0
    # fixed_point.h's layout: 256 bytes of maxima + 24 bytes per accumulator point, per crop (vertices) and per crop and
    # group of three channels (attributes)
    assert q(2, 10, 3, 0, 1) == 256 + 2 * 10 * 24
    assert q(2, 10, 3, 1, 0) == 256 + 2 * 10 * 24 and q(2, 10, 4, 1, 0) == 256 + 2 * 2 * 10 * 24
    assert q(2, 10, 17, 1, 1) == q(2, 10, 17, 1, 0) + q(2, 10, 17, 0, 1)
    assert q(3, 10, 17, 1, 1) > q(2, 10, 17, 1, 1) and q(2, 11, 17, 1, 1) > q(2, 10, 17, 1, 1)
    assert q(2, 10, 19, 1, 1) > q(2, 10, 17, 1, 1) and q(2, 10, 64, 1, 0) > q(2, 10, 33, 1, 0)


def test_entries_reject_bad_arguments_without_a_device():
    from spherehand_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOLARGE = -1, -2
    fwd, bwd = lib.shr_tri_interp_fwd, lib.shr_tri_interp_bwd
    #          owner verts faces attr stride B NV F  W  H  C  out
    assert fwd(None, None, None, None, 0, 0, 4, 2, 8, 8, 3, None, None) == 0                 # B = 0: a no-op
    assert fwd(None, 16, 16, 16, 0, 1, 4, 2, 8, 8, 3, 16, None) == EINVAL                    # no owner
    assert fwd(16, 16, 16, None, 0, 1, 4, 2, 8, 8, 3, 16, None) == EINVAL                    # no attr
    assert fwd(16, 16, 16, 16, 0, 1, 4, 2, 8, 8, 3, None, None) == EINVAL                    # no out
    assert fwd(16, 16, None, 16, 0, 1, 4, 2, 8, 8, 3, 16, None) == EINVAL                    # faces missing
    assert fwd(16, 20, 16, 16, 0, 1, 4, 2, 8, 8, 3, 16, None) == EINVAL                      # misaligned vertices
    assert fwd(16, 16, 16, 16, 7, 1, 4, 2, 8, 8, 3, 16, None) == EINVAL                      # stride neither 0 nor NV * C
    assert fwd(16, 16, 16, 16, 0, 1, 0, 2, 8, 8, 3, 16, None) == EINVAL                      # NV = 0
    assert fwd(16, 16, 16, 16, 0, 1, 4, 2, 8, 0, 3, 16, None) == EINVAL                      # H = 0
    assert fwd(16, 16, 16, 16, 0, 1, 4, 2, 8, 8, 0, 16, None) == EINVAL                      # C = 0
    assert fwd(16, 16, 16, 16, 0, 1, 4, 2, 8, 8, 65, 16, None) == ETOOLARGE                  # C above the limit
    assert fwd(16, 16, 16, 16, 0, 70000, 4, 2, 8, 8, 3, 16, None) == ETOOLARGE
    assert fwd(16, 16, 16, 16, 0, 1, 4, 2, 70000, 8, 3, 16, None) == ETOOLARGE
    assert fwd(16, 16, 16, 16, 0, 1, 4, 2, 8, 70000, 3, 16, None) == ETOOLARGE
    #          owner verts faces attr stride B NV F W H C  grad_out grad_attr grad_verts ws
    assert bwd(None, None, None, None, 0, 0, 4, 2, 8, 8, 3, None, None, None, None, None) == 0
    assert bwd(16, 16, 16, 16, 12, 1, 4, 2, 8, 8, 3, None, 16, 16, 16, None) == EINVAL        # no grad_out
    assert bwd(16, 16, 16, 16, 12, 1, 4, 2, 8, 8, 3, 16, None, None, 16, None) == EINVAL      # no output at all
    assert bwd(16, 16, 16, 16, 12, 1, 4, 2, 8, 8, 3, 16, 16, 16, None, None) == EINVAL        # no workspace
    assert bwd(16, 16, 16, 16, 12, 1, 4, 2, 8, 8, 3, 16, 16, 16, 24, None) == EINVAL          # misaligned workspace
    assert bwd(16, 16, 16, 16, 12, 1, 4, 2, 8, 8, 3, 16, 16, 20, 16, None) == EINVAL          # misaligned grad_vertices
    assert bwd(16, 16, 16, 16, 12, 1, 4, 2, 8, 8, 65, 16, 16, 16, 16, None) == EINVAL         # (stride no longer NV * C)
    assert bwd(16, 16, 16, 16, 0, 1, 4, 2, 8, 8, 65, 16, 16, 16, 16, None) == ETOOLARGE
    assert bwd(16, 16, 16, 16, 0, 70000, 4, 2, 8, 8, 3, 16, 16, 16, 16, None) == ETOOLARGE
    assert bwd(16, 16, 16, 16, 0, 60000, 4, 2, 8, 8, 4, 16, 16, 16, 16, None) == ETOOLARGE    # B * ceil(C / 3) > 65535


def test_wrappers_check_their_inputs():
    from spherehand_amd import ops
    from spherehand_amd.render import MeshAttributeRaster
    a = torch.zeros(1, 4, 3)
    own = torch.zeros(1, 8, 8, dtype=torch.int32)
    verts, faces = torch.zeros(1, 4, 4), torch.zeros(2, 3, dtype=torch.int32)
    assert hasattr(ops, "TriInterpolate") and ops.TRI_INTERP_MAX_CHANNELS >= 64
    calls = [lambda: ops.tri_interpolate(a, own, verts, faces),                       # CPU tensors
             lambda: ops.tri_interpolate(a.double(), own, verts, faces),
             lambda: ops.tri_interpolate_bwd(a, own, verts, faces, torch.zeros(1, 3, 8, 8)),
             lambda: ops.TriInterpolate.apply(a.requires_grad_(True), own, verts, faces),
             lambda: ops.TriInterpolate.apply(a, own, torch.zeros(1, 4), faces),
             lambda: MeshAttributeRaster(8, 8, np.zeros((2, 3), np.int64))(torch.zeros(1, 4), a)]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    r = MeshAttributeRaster(640, 480, np.array([[0, 1, 2], [2, 1, 3]]))
    assert r.faces_i32.tolist() == [[1, 0, 2], [1, 2, 3]] and r.faces_i32.dtype == torch.int32
    assert MeshAttributeRaster(8, 8, np.array([[0, 1, 2]]), right_hand=False).faces_i32.tolist() == [[0, 1, 2]]


def test_dense_skin_weights():
    from spherehand_amd import hand_model
    mesh = hand_model.load_mesh()
    w = hand_model.dense_skin_weights(mesh)
    NV = len(mesh["vertices"])
    assert w.shape == (NV, 17) and w.dtype == np.float32 and w.flags["C_CONTIGUOUS"]
    want = np.zeros((NV, 17), np.float64)
    total = np.zeros(NV, np.float64)
    for b, bone in enumerate(mesh["bones"]):
        for v, c in zip(bone["weight_vertexid"], bone["weight_coeff"]):
            want[v, b] += c
            total[v] += c
    assert np.array_equal(w, want.astype(np.float32))
    np.testing.assert_allclose(w.astype(np.float64).sum(1), total, rtol=0, atol=17 * U)
    assert w.min() >= 0 and 0.99 < total.min() and total.max() < 1.01
    # sparse_skin's wv = float32(weight * vertex), entry by entry
    start, bone, wv = hand_model.sparse_skin(mesh)
    V = np.asarray(mesh["vertices"], np.float64)
    vid = np.repeat(np.arange(NV), np.diff(start))
    assert np.array_equal(wv, (want[vid, bone][:, None] * V[vid]).astype(np.float32))
    assert (w[vid, bone] > 0).all() and (w > 0).sum() == len(bone)


def _asm(unit, tmp_path):
    from spherehand_amd import build
    out = str(tmp_path / (unit + ".s"))
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", unit + ".hip")],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_interp_unit_stays_in_registers(tmp_path):
    text = _asm("tri_interp", tmp_path)
    meta = text[text.index("amdhsa.kernels:"):]
    d = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        d[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                   for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert len([n for n in d if "interp_fwd_kernel" in n]) == 2               # scalar and float4 attribute rows
    assert len([n for n in d if "InterpVertexTaps" in n]) == 5                # maxima x 2, LDS sums, global sums x 2
    assert len([n for n in d if "InterpAttrTaps" in n]) == 2                  # LDS sums, global sums
    assert any("interp_attr_max_kernel" in n for n in d) and any("interp_attr_finish_kernel" in n for n in d)
    assert all(v["private_segment_fixed_size"] == 0 for v in d.values()), d
    assert max(v["group_segment_fixed_size"] for v in d.values()) == 48 * 1024   # the accumulator stage, nothing else
    # the forward at full occupancy; a 16-wave workgroup of the fixed-point passes fits a CU (128 VGPRs per lane)
    assert all(v["vgpr_count"] <= 64 for n, v in d.items() if "interp_fwd" in n), d
    assert all(v["vgpr_count"] <= 128 for v in d.values()), d
    sizes = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == len(d) and max(sizes) == 0, sizes
    mnemonics = {l.split()[0] for l in text.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))}
    scalar_writes = [m for m in mnemonics if m.startswith("s_") and ("store" in m or "atomic" in m or m.endswith("_wb"))]
    assert not scalar_writes, scalar_writes


def _cells(seed, W=64, H=32, area=6.0, margin=0.05):
    """test_gradient_matches_central_differences' selection (tests/test_tri_grad_gpu.py): one face per 8 x 8 cell, area
    at least 6 px^2, every pixel centre at least 0.05 px from every edge; shared vertex list, z 20 .. 60.  Owners: the
    pixels strictly inside a face."""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    owner = np.full((1, H, W), -1, np.int32)
    for cy in range(4, H - 4, 8):
        for cx in range(4, W - 4, 8):
            while True:
                p = np.array([cx, cy], np.float64) + rng.uniform(-3.5, 3.5, (3, 2))
                cr = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1])
                if cr < 0:
                    p = p[[1, 0, 2]]
                if abs(cr) / 2 < area:
                    continue
                gx, gy = np.meshgrid(np.arange(cx - 5, cx + 6), np.arange(cy - 5, cy + 6))
                q = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64)
                dmin = np.inf
                for a in range(3):
                    e0, e1 = p[a], p[(a + 1) % 3]
                    t = np.clip(((q - e0) @ (e1 - e0)) / ((e1 - e0) @ (e1 - e0)), 0, 1)
                    dmin = min(dmin, np.linalg.norm(q - (e0 + t[:, None] * (e1 - e0)), axis=1).min())
                if dmin > margin:
                    break
            s = [(p[(k + 1) % 3, 0] - p[k, 0]) * (q[:, 1] - p[k, 1]) - (p[(k + 1) % 3, 1] - p[k, 1]) * (q[:, 0] - p[k, 0])
                 for k in range(3)]
            inside = (s[0] > 0) & (s[1] > 0) & (s[2] > 0)
            qi = q[inside].astype(int)
            owner[0, qi[:, 1], qi[:, 0]] = len(faces)
            faces.append([len(verts), len(verts) + 1, len(verts) + 2])
            verts += [list(pt) + [rng.uniform(20, 60), 1.0] for pt in p]
    return np.asarray(verts, np.float32)[None], np.asarray(faces, np.int64), owner


def _random_scene(seed, B=2, W=48, H=40, n=7):
    """A jittered grid mesh with shared vertices and an owner map of random faces (in range or -1): any owner is a
    legal input of the interpolation, clamped weights included."""
    rng = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:n, 0:n].astype(np.float64)
    faces = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, i * n + j + 1, (i + 1) * n + j, (i + 1) * n + j + 1
            faces += [[a, b, c], [b, d, c]]
    faces = np.array(faces)
    v = np.zeros((B, n * n, 4), np.float32)
    for bi in range(B):
        v[bi, :, 0] = gx.ravel() * (W - 1) / (n - 1) + rng.normal(0, 0.2 * W / n, n * n)
        v[bi, :, 1] = gy.ravel() * (H - 1) / (n - 1) + rng.normal(0, 0.2 * H / n, n * n)
        v[bi, :, 2] = rng.uniform(20, 80, n * n)
    # each pixel's owner: the face whose centroid is nearest (so most weights pass), some replaced at random
    cen = v[:, faces, :2].mean(2)                                                       # [B,F,2]
    py, px = np.mgrid[0:H, 0:W]
    owner = np.stack([np.argmin((cen[bi, :, 0, None, None] - px) ** 2 + (cen[bi, :, 1, None, None] - py) ** 2, 0)
                      for bi in range(B)]).astype(np.int32)
    swap = rng.random(owner.shape) < 0.1
    owner[swap] = rng.integers(-1, len(faces), swap.sum())
    return v, faces, owner


@pytest.mark.parametrize("shared", [False, True])
def test_the_two_restatements_agree(shared):
    for seed in range(3):
        v, faces, owner = _random_scene(seed)
        rng = np.random.default_rng(seed + 20)
        C = (1, 3, 17)[seed]
        attr = rng.standard_normal((v.shape[1], C) if shared else (v.shape[0], v.shape[1], C)).astype(np.float32)
        a, info = ref.interp32(attr, owner, v, faces, with_info=True)
        b = ref.interp64(torch.from_numpy(attr), owner, torch.from_numpy(v), faces).numpy()
        assert a.shape == b.shape == (v.shape[0], C) + owner.shape[1:]
        assert info["live"].sum() > 1000 and (~(info["w"] >= 0) | ~(info["w"] <= 1)).any(1).sum() > 50   # clamps occur
        assert np.array_equal(a[:, 0] == 0, b[:, 0] == 0) or C > 1
        assert np.all(a[np.broadcast_to((owner < 0)[:, None], a.shape)] == 0)
        # fp32 against fp64 of the same formula: the weights carry ~U X Y / |den| each (see the identity test); these
        # faces have |den| ~ 50 and X Y ~ 2000, attributes of order 1
        assert np.abs(a - b).max() < 2e-3 and np.abs(a - b).mean() < 1e-5, (np.abs(a - b).max(), np.abs(a - b).mean())


def test_restatement_gradient_matches_central_differences():
    """On faces of area >= 6 px^2 with every pixel at least 0.05 px from a clamp boundary a step of 1e-6 changes no
    decision: restatement (b)'s autograd gradient equals central differences of itself in fp64."""
    for seed in range(2):
        v, faces, owner = _cells(seed)
        rng = np.random.default_rng(seed + 5)
        C = 3 + seed
        attr = rng.standard_normal((1, v.shape[1], C))
        g = rng.standard_normal((1, C) + owner.shape[1:])
        assert (owner >= 0).sum() > 100
        ga, gv = ref.grads(attr, owner, v, faces, g)
        assert np.all(gv[..., 2:] == 0) and np.abs(gv[..., :2]).max() > 0.1 and np.abs(ga).max() > 0.1

        def f(vv, aa):
            return (ref.interp64(torch.from_numpy(aa), owner, torch.from_numpy(vv), faces).numpy() * g).sum()

        h = 1e-6
        v64 = v.astype(np.float64)
        for i in rng.choice(v.shape[1], 12, replace=False):
            for d in range(2):
                vp, vm = v64.copy(), v64.copy()
                vp[0, i, d] += h
                vm[0, i, d] -= h
                fd = (f(vp, attr) - f(vm, attr)) / (2 * h)
                assert abs(fd - gv[0, i, d]) <= 1e-5 * max(1.0, np.abs(gv).max()), (i, d, fd, gv[0, i, d])
            ch = int(rng.integers(C))
            ap, am = attr.copy(), attr.copy()
            ap[0, i, ch] += 1e-3
            am[0, i, ch] -= 1e-3
            assert abs((f(v64, ap) - f(v64, am)) / 2e-3 - ga[0, i, ch]) <= 1e-8 * max(1.0, np.abs(ga).max())


# The identity's bound, from the operation count (u = 2^-24; X, Y the largest |x|, |y| of the face's corners; a pixel
# whose three weights lie in [0, 1] is inside the face, so |x| <= X, |y| <= Y):
#   a weight w_k = (fi0 x + fi1 y) + fi2, fi_j = num_j / den.  In units of u X Y / |den|: the numerators' roundings give
#   2 (fi0: one subtraction, |y1 - y2| <= 2 Y, times x) + 2 (fi1) + 4 (fi2: two products and a subtraction of magnitude
#   2 X Y); the three divisions 2 + 2 + 2; the two products 2 + 2; the first addition 4; the last addition u |w| <= u
#   <= 4 u X Y / |den| (|den| is twice the area, at most 4 X Y): 26 in all.  (den's own error scales the three weights
#   alike and leaves c_k / s.)
#   wh_k = c_k / s with s = 1 + (at most 3 x 26 + roundings): sum_k |wh_k - w_k(exact)| <= (3 + 3) x 26 = 156, + 4 for
#   the roundings of s and of the three quotients: K = 160.
#   out - x = sum_k (wh_k - w_k) (x_k - x_0) + x_0 (sum_k wh_k - 1) + the roundings of three products and two additions:
#   |out - x| <= K u (X Y / |den|) extent + 16 u max(X, Y).
K_IDENTITY = 160


def test_identity_and_constant_on_the_hand(oracle):
    """Restatement (a) with the vertices' own (x, y) as attributes gives back the pixel wherever no weight was clamped,
    within the per-pixel bound above; with the constant 1 it gives 1 within 4 u at EVERY owned pixel.  The hand at the
    four sampled poses, 640 x 640; owners from the reference raster's depth (ref.cpu_owners).
    Counted here: 0.01 % of the 378 677 owned pixels have a clamped weight (pixel centres a rounding outside an edge
    that the column spans still cover), far under the cap of 25 %; the largest error is 0.05 px (on the smallest
    faces), 0.02 of its bound."""
    W = H = 640
    v, faces = ref.hand_verts(4, W, H)
    f64 = faces.astype(np.int64)
    depth = oracle.tri_raster_fwd(np.ascontiguousarray(v[:, f64, :3]), W, H)
    owner = ref.cpu_owners(depth, v, faces)
    fg = depth != np.float32(1000.0)
    assert fg.sum() > 4 * 40000 and np.array_equal(owner >= 0, fg)            # every drawn pixel found its face
    out, info = ref.interp32(v[..., :2].copy(), owner, v, faces, with_info=True)
    b, y, x, w, p = info["b"], info["y"], info["x"], info["w"], info["p"]
    assert info["live"].all() and len(b) == fg.sum()
    inside = ((w >= 0) & (w <= 1)).all(1)
    left_out = 1.0 - inside.mean()
    print("identity: %d owned pixels, %.2f %% left out (a clamped weight)" % (len(b), 100 * left_out))
    assert left_out <= 0.25, left_out
    X, Y = np.abs(p[..., 0]).max(1).astype(np.float64), np.abs(p[..., 1]).max(1).astype(np.float64)
    _, den, _ = ref.face_matrix32(p)
    ext = np.maximum(p[..., 0].max(1) - p[..., 0].min(1), p[..., 1].max(1) - p[..., 1].min(1)).astype(np.float64)
    bound = K_IDENTITY * U * X * Y / np.abs(den.astype(np.float64)) * ext + 16 * U * np.maximum(X, Y)
    got = out[b, :, y, x].astype(np.float64)
    err = np.maximum(np.abs(got[:, 0] - x), np.abs(got[:, 1] - y))
    ratio = (err / bound)[inside]
    print("identity: max error %.3g px, max error / bound %.3g, median bound %.3g px" %
          (err[inside].max(), ratio.max(), np.median(bound[inside])))
    assert ratio.max() <= 1.0, ratio.max()
    ones = ref.interp32(np.ones((v.shape[1], 1), np.float32), owner, v, faces)
    e1 = np.abs(ones[:, 0].astype(np.float64) - 1.0)
    assert e1[fg].max() <= 4 * U and np.all(ones[:, 0][~fg] == 0), e1[fg].max()
