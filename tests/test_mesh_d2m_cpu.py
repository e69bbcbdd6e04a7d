"""The mesh data-to-model distance without a device: the fp32 restatement of tests/mesh_d2m_ref.py against an fp64 brute
force written without the seven regions, the analytic fp64 gradient against central differences, the translation fit with
the restatement alone, the entries of the C ABI with their argument errors, and the unit's code-object metadata."""
import ctypes
import os
import re
import subprocess

import numpy as np

import mesh_d2m_ref as ref
from conftest import GOLDEN, ROOT

F32 = np.float32
ENTRIES = ("shr_mesh_d2m_workspace_bytes", "shr_mesh_d2m_fwd", "shr_mesh_d2m_bwd_workspace_bytes", "shr_mesh_d2m_bwd")

# The largest |restated dist - fp64 minimum| measured on the inputs below (x86-64, numpy; the seeds are fixed, so the
# figures repeat): the fp32 roundings of ap = p - a and of the corner differences scale with the coordinates (2^-24 x 30,
# x 640), not with the image.  The tests assert 4 x the measured value.
MEASURED = {"soup 30": 2.94e-6, "soup 640": 8.31e-5, "hand": 2.22e-6, "regions": 4.70e-6}


def restated(p, v, faces):
    """(dist fp32, face) of points p [N,3] by the restatement's sequence and serial rule"""
    a = v[faces[:, 0], :3]
    d2 = ref.tri_dist2_32(p[:, None, :] - a[None], (v[faces[:, 1], :3] - a)[None], (v[faces[:, 2], :3] - a)[None])
    d2 = np.where(d2 == d2, d2, F32(np.inf))
    f = d2.argmin(1)
    return np.sqrt(d2[np.arange(len(p)), f]), f


def against_brute(p, v, faces, name):
    p, v = np.asarray(p, F32), np.asarray(v, F32)
    d, f = restated(p, v, faces)
    brute = ref.brute64(p, v[faces][:, :, :3])
    best = brute.min(1)
    worst = float(np.abs(d - best).max())
    bar = 4 * MEASURED[name]
    print("%s: largest |dist - fp64 minimum| %.3g (measured %.3g, bar %.3g); chosen face above the minimum by at most %.3g"
          % (name, worst, MEASURED[name], bar, (brute[np.arange(len(p)), f] - best).max()))
    assert worst <= bar, name
    assert worst >= MEASURED[name] / 4, (name, "the measured figure is stale")
    assert (brute[np.arange(len(p)), f] - best).max() <= bar, name            # the chosen face is a minimiser


def distinct_faces(rs, NV, F):
    return np.stack([rs.permutation(NV)[:3] for _ in range(F)])


def test_restatement_against_brute_force_on_soups():
    rs = np.random.RandomState(0)
    for scale in (30, 640):
        v = np.ones((200, 4), F32)
        v[:, :3] = rs.uniform(0, scale, (200, 3))
        faces = distinct_faces(rs, 200, 400)
        p = rs.uniform(-0.2 * scale, 1.2 * scale, (3000, 3))
        against_brute(p, v, faces, "soup %d" % scale)


def test_restatement_against_brute_force_on_the_hand():
    rs = np.random.RandomState(0)
    v = np.load(os.path.join(GOLDEN, "g2_mesh.npz"))["verts"][0]
    faces = np.load(os.path.join(ROOT, "spherehand_amd", "data", "hand_model.npz"))["faces"].astype(np.int64)
    p = v[rs.randint(0, len(v), 2000), :3] + rs.uniform(-8, 8, (2000, 3))
    against_brute(p, v, faces, "hand")


def region_label(v, w):
    """A, B, AB, C, AC, BC, in = 0..6 from closest64's (v, w): the vertex and edge regions give exact 0 and 1"""
    return np.select([(v == 0) & (w == 0), (v == 1) & (w == 0), w == 0, (v == 0) & (w == 1), v == 0, v == 1 - w],
                     [0, 1, 2, 3, 4, 5], 6)


def test_restatement_in_each_of_the_seven_regions_on_both_sides():
    """points a + s ab + t ac + h n over a grid of (s, t) that reaches into every region, above and below the plane"""
    rs = np.random.RandomState(1)
    tri = rs.uniform(0, 40, (30, 3, 3))
    st = np.array([(s, t) for s in (-0.6, 0.2, 0.5, 1.4) for t in (-0.6, 0.2, 0.5, 1.4)])
    ps, labels = [], []
    for k in range(len(tri)):
        a, ab, ac = tri[k, 0], tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]
        n = np.cross(ab, ac)
        n /= np.linalg.norm(n)
        for h in (-3.0, 2.0):
            p = (a + st[:, :1] * ab + st[:, 1:] * ac + h * n).astype(F32)
            vv, ww = ref.closest64(ab.astype(F32), ac.astype(F32), p - tri[k, 0].astype(F32))
            labels.append(region_label(vv, ww) + (7 if h > 0 else 0))
            d = np.sqrt(ref.tri_dist2_32(p - tri[k, 0].astype(F32), ab.astype(F32), ac.astype(F32)))
            ps.append(np.abs(d - ref.brute64(p, tri[k:k + 1].astype(F32))[:, 0]))
    assert set(np.concatenate(labels)) == set(range(14))                       # every region, on both sides
    worst = float(np.concatenate(ps).max())
    print("regions: largest |dist - fp64| %.3g (measured %.3g, bar %.3g)" % (worst, MEASURED["regions"], 4 * MEASURED["regions"]))
    assert MEASURED["regions"] / 4 <= worst <= 4 * MEASURED["regions"]


def test_gradient_against_central_differences():
    """L(V) = sum gd_i min_f dist64(p_i, V) over the toy mesh moved off its observation, differentiated in all 45 vertex
    coordinates.  Central differences at h and h / 2: the analytic gradient's discrepancy falls by about 4 (second order).
    The points kept lie away from ties (the second face at least 0.05 farther), from saturation, and from the borders of
    the seven regions (the closest point is C1 there, not C2: a point that crosses one inside the stencil costs O(h)) --
    their face and region do not change under any of the displacements used."""
    rest, faces = ref.toy()
    rs = np.random.RandomState(4)
    obs = np.full((1, 32, 32), 1000.0, F32)
    obs[0, 4:28, 4:28] = rs.uniform(38, 58, (24, 24))
    v = ref.moved(rest, (1.5, -1.0, 2.0))
    faces64 = faces.astype(np.int64)
    dist, face = ref.forward32(obs, v, faces, fg_max=500.0, max_dist=50.0)
    gd = rs.standard_normal(obs.shape).astype(F32)
    b, i, j, p = ref.points32(obs, (1, 0, 1, 0), 500.0)
    h = 2.0 ** -9

    def state(V):
        tri = V[0][faces64][:, :, :3].astype(np.float64)
        d = ref.brute64(p, tri)
        f = d.argmin(1)
        vv, ww = ref.closest64(tri[f, 1] - tri[f, 0], tri[f, 2] - tri[f, 0], p.astype(np.float64) - tri[f, 0])
        return d, f, region_label(vv, ww)

    d0, f0, r0 = state(v.astype(np.float64))
    keep = np.sort(d0, 1)[:, 1] - d0.min(1) > 0.05
    for k in range(rest.shape[1]):
        for c in range(3):
            for s in (-2 * h, 2 * h):
                V = v.astype(np.float64)
                V[0, k, c] += s
                _, f, r = state(V)
                keep &= (f == f0) & (r == r0)
    assert keep.sum() > 150 and len(set(r0[keep])) >= 4 and np.array_equal(f0[keep], face[0, i, j][keep])
    mask = np.full(obs.shape, 1000.0, F32)
    mask[0, i[keep], j[keep]] = obs[0, i[keep], j[keep]]
    analytic = ref.grad64(mask, v, faces, dist, face, gd, fg_max=500.0, max_dist=50.0)[0]
    L = lambda V: float((gd[0, i[keep], j[keep]].astype(np.float64) * state(V)[0].min(1)[keep]).sum())   # noqa: E731
    err = []
    for step in (h, h / 2):
        fd = np.zeros_like(analytic)
        for k in range(rest.shape[1]):
            for c in range(3):
                up, dn = v.astype(np.float64), v.astype(np.float64)
                up[0, k, c] += step
                dn[0, k, c] -= step
                fd[k, c] = (L(up) - L(dn)) / (2 * step)
        err.append(np.abs(fd - analytic).max())
    print("central differences: |fd - analytic| %.3g at h = 2^-9, %.3g at h / 2: ratio %.2f; largest |gradient| %.3g"
          % (err[0], err[1], err[0] / err[1], np.abs(analytic).max()))
    assert np.abs(analytic).max() > 1 and 3.0 < err[0] / err[1] < 5.0


def test_translation_fit_with_the_restatement(oracle):
    """The toy mesh observed by its own depth at 32 x 32 (the reference raster on the CPU), started from a translation of
    (2.5, -1.5, 4): plain gradient descent on the three translation parameters, step 0.5, 24 steps, under the restated
    MeshDataToModelLoss.  The loss never rises and every component ends closer to the truth than it began, z included:
    (2.5, -1.5, 4) -> (2.11, -0.39, 0.79), the loss 1.361 -> 0.408.  The 24 steps are the fit's approach: a fixed step on a
    mean of |distance| overshoots once the points straddle the surface, and from about the 30th step the loss rises by
    small amounts from one step to the next while the translation goes on to (-0.02, 0.18, 0.09) at 80 steps, loss 0.049 --
    the remaining 0.18 px in y is the raster's depth at pixel centres against a surface that slopes between them."""
    rest, faces = ref.toy()
    S = ref.TOY_SIZE
    obs = oracle.tri_raster_fwd(np.ascontiguousarray(rest[:, faces.astype(np.int64), :3]), S, S)
    assert obs.shape == (1, S, S) and 350 < (obs < 99).sum() < 450
    assert (obs[obs < 99] < 40).any()                                          # the fin is seen
    t, losses = ref.fit(rest, faces, obs)
    print("fit: t = %s after %d steps, loss %.4f -> %.4f" % (t, len(losses), losses[0], losses[-1]))
    assert all(b <= a for a, b in zip(losses, losses[1:])), losses
    assert np.all(np.abs(t) < np.abs(np.asarray(ref.FIT_SHIFT))) and losses[-1] < 0.35 * losses[0]
    assert np.allclose(t, (2.11, -0.39, 0.79), atol=0.02)


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spherehand_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23
    inf = float("inf")
    # host-side argument rules (no launch: every call returns before one)
    assert lib.shr_mesh_d2m_workspace_bytes(3, 7) == 3 * 7 * 48 and lib.shr_mesh_d2m_workspace_bytes(-1, 7) == -1
    assert lib.shr_mesh_d2m_workspace_bytes(5, 0) == 0 and lib.shr_mesh_d2m_workspace_bytes(65535, 715827882) == 65535 * 715827882 * 48
    assert lib.shr_mesh_d2m_bwd_workspace_bytes(2, 5) == 256 + 2 * 5 * 3 * 8 and lib.shr_mesh_d2m_bwd_workspace_bytes(2, -1) == -1
    fwd = [16, 16, 16, 1, 5, 7, 9, 8, 1.0, 0.0, 1.0, 0.0, 99.0, 50.0, 16, 16, 16, None]
    bad = lambda i, val: lib.shr_mesh_d2m_fwd(*(fwd[:i] + [val] + fwd[i + 1:]))   # noqa: E731
    assert bad(3, 0) == 0                                                         # B == 0: a no-op
    assert bad(0, None) == -1 and bad(1, None) == -1 and bad(2, None) == -1 and bad(14, None) == -1 and bad(15, None) == -1
    assert bad(16, None) == -1 and bad(1, 8) == -1 and bad(16, 8) == -1 and bad(0, 18) == -1 and bad(15, 6) == -1
    assert bad(13, -1.0) == -1 and bad(13, float("nan")) == -1 and bad(4, 0) == -1 and bad(5, -1) == -1
    assert bad(6, 0) == -1 and bad(7, 0) == -1 and bad(3, -1) == -1
    assert bad(6, 2049) == -2 and bad(7, 2049) == -2 and bad(3, 65536) == -2
    assert bad(4, 715827883) == -2 and bad(5, 715827883) == -2                    # 3 NV, 3 F >= 2^31
    bwd = [16, 16, 16, 16, 16, 16, 1, 5, 7, 9, 8, 1.0, 0.0, 1.0, 0.0, 99.0, inf, 16, 16, None]
    bad = lambda i, val: lib.shr_mesh_d2m_bwd(*(bwd[:i] + [val] + bwd[i + 1:]))   # noqa: E731
    assert bad(6, 0) == 0
    for i in (0, 1, 2, 3, 4, 5, 17, 18):
        assert bad(i, None) == -1, i
    assert bad(1, 8) == -1 and bad(17, 8) == -1 and bad(18, 8) == -1 and bad(4, 18) == -1
    assert bad(16, -0.5) == -1 and bad(7, 0) == -1 and bad(8, -1) == -1 and bad(9, 0) == -1
    assert bad(9, 2049) == -2 and bad(10, 2049) == -2 and bad(6, 65536) == -2 and bad(7, 715827883) == -2


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_dist_transform_cpu.py's reading of the code-object metadata: every kernel of mesh_d2m.hip reports
    ScratchSize 0 and no spills; the search keeps its chunk of records, its point list and its counts in 14 400 bytes of
    static LDS and stays at or below 64 VGPRs (eight waves per SIMD; DESIGN.md 4.4j has the figures)."""
    from spherehand_amd import build
    out = str(tmp_path / "mesh_d2m.s")
    src = os.path.join(build.PKG, "csrc", "mesh_d2m.hip")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(s) for s in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == 9 and max(sizes) == 0, sizes
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
                                                          r"group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", block)}
    assert len(kernels) == 9
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
    one = lambda part: [k for n, k in kernels.items() if part in n]   # noqa: E731
    search, = one("d2m_search_kernel")
    records, = one("d2m_records_kernel")
    code = open(src).read()
    chunk = int(re.search(r"constexpr int kD2mChunk = (\d+);", code).group(1))
    tile = int(re.search(r"constexpr int kD2mTilePix = (\d+);", code).group(1))
    assert search["group_segment_fixed_size"] == chunk * 48 + tile * 2 + 64 == 14400 and search["vgpr_count"] <= 64
    assert records["group_segment_fixed_size"] == 0 and len(one("D2mTaps")) == 5
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "14 400" in design[design.index("### 4.4j"):design.index("### 4.5 ")]
