"""The nearest-site transform and the silhouette coverage term without a GPU: the restatements of tests/sil_cover_ref.py
against each other (the two-pass rule against the brute-force argmin, the fp64 gradient against central differences of the
frozen function, the scale-and-shift fit on the toy mesh and the degenerate minimum it removes), the header, loader and
exports, and the new unit's code-object resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dt_ref
import sil_cover_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("shr_dt_nearest_workspace_bytes", "shr_dt_nearest_fwd", "shr_sil_cover_fwd", "shr_sil_cover_bwd_workspace_bytes",
           "shr_sil_cover_bwd")


def _check_nearest(site, tag):
    H, W = site.shape
    want_d2, want = ref.nearest_brute(site)
    got_d2, got = ref.nearest_separable(site)
    assert got.dtype == np.int32 and got_d2.dtype == np.int32
    assert np.array_equal(got_d2, want_d2) and np.array_equal(got, want), tag
    assert np.array_equal(got_d2, dt_ref.dt_separable(site)), tag
    if site.any():
        idx = np.arange(H * W).reshape(H, W)
        assert np.array_equal(got[site], idx[site])                              # a site is its own nearest
        i, j = np.mgrid[0:H, 0:W]
        assert site.ravel()[got.ravel()].all()                                   # ... and every nearest is a site
        assert np.array_equal((i - got // W) ** 2 + (j - got % W) ** 2, got_d2)    # at the stated distance
    else:
        assert np.all(got == -1) and np.all(got_d2 == H * H + W * W)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (3, 13), (17, 19), (9, 33)])
def test_separable_equals_brute_force(H, W):
    for k, density in enumerate((0.0, 0.01, 0.1, 0.5, 1.0)):
        for seed in range(3):
            site = np.random.RandomState(100 * k + seed).rand(H, W) < density
            _check_nearest(site, (H, W, density, seed))
    i, j = np.mgrid[0:H, 0:W]
    _check_nearest((i + j) % 4 == 0, (H, W, "periodic"))                           # full of ties
    # the tie rules themselves: a site above and one below at the same distance -> the one above; left and right -> left
    if H >= 3:
        site = np.zeros((H, W), bool)
        site[0, 0] = site[2, 0] = True
        assert ref.nearest_separable(site)[1][1, 0] == 0 and ref.nearest_brute(site)[1][1, 0] == 0
    if W >= 3:
        site = np.zeros((H, W), bool)
        site[0, 0] = site[0, 2] = True
        assert ref.nearest_separable(site)[1][0, 1] == 0 and ref.nearest_brute(site)[1][0, 1] == 0


def _toy_case(s=0.75, t=(5.0, -3.0), seed=0):
    """the mitten at rest observed, the model scaled and moved: the inputs of the backward, all from the CPU"""
    rest, faces = ref.mitten()
    observed, _ = ref.render(rest, faces, ref.MITTEN_SIZE, ref.MITTEN_SIZE)
    v = ref.model(rest, s, t)
    depth, owner = ref.render(v, faces, ref.MITTEN_SIZE, ref.MITTEN_SIZE)
    d2, near = ref.transform(depth, 1000.0)
    rs = np.random.RandomState(seed)
    gd = rs.standard_normal(observed.shape).astype(np.float32)
    gd[rs.rand(*observed.shape) < 0.2] = 0
    return rest, faces, observed, v, depth, owner, d2, near, gd


def test_mitten_is_as_stated():
    rest, faces = ref.mitten()
    S, M = ref.MITTEN_SIZE, ref.MITTEN_MARGIN
    assert rest.shape == (1, 55, 4) and faces.shape == (56, 3) and len(faces) <= 200
    assert rest[0, :, :2].min() >= M and rest[0, :, :2].max() <= S - M
    ext = rest[0, :, :2].max(0) - rest[0, :, :2].min(0)
    assert abs(ext.max() / 2 - ref.MITTEN_HALF_EXTENT) < 1e-5
    fv = rest[0][faces][..., :2].astype(np.float64)
    drawn = (fv[:, 2, 1] - fv[:, 0, 1]) * (fv[:, 1, 0] - fv[:, 0, 0]) >= (fv[:, 1, 1] - fv[:, 0, 1]) * (fv[:, 2, 0] - fv[:, 0, 0])
    assert drawn.all()                                                           # the raster's cull draws every face
    depth, owner = ref.render(rest, faces, S, S)
    assert set(np.unique(owner)) == set(range(-1, 56)) and ((owner >= 0) == (depth < 1000)).all()
    assert depth[0, :M].min() == 1000 and depth[0, :, :M].min() == 1000 and depth[0, S - M + 1:].min() == 1000


def test_fp64_gradient_matches_central_differences():
    """cover_grad64 against central differences of the frozen function f(delta) = sum_p g_p |r_p - sum_v M[v,q_p] delta_v|,
    r_p = p - q_p (sil_cover_ref.frozen).  One coordinate of one vertex moved by +-h: a term is phi(h) = g |r - w h e| with
    |r| >= 1 (d2 >= 1 at a contributing pixel) and 0 <= w <= 1, whose third derivative is at most 3 w^3 / |r - w h e|^2
    <= 3 / (1 - h)^2, so the central difference of a term is off by at most |g| h^2 / (2 (1 - h)^2).  Rounding: each
    evaluation rounds a term at most 8 times and sums P terms, an error of at most (8 + P) 2^-53 sum_p |g_p| D_p with D_p
    the term's distance; twice that over 2 h.  Bound, for every vertex coordinate:
        sum_p |g_p| h^2 / (2 (1 - h)^2) + (8 + P) 2^-53 sum_p |g_p| (D_p + h) / h."""
    rest, faces, observed, v, depth, owner, d2, near, gd = _toy_case()
    S = ref.MITTEN_SIZE
    for max_dist in (np.inf, 7.25):
        grad = ref.cover_grad64(observed, ref.FIT_FG_MAX, d2, near, owner, v, faces, gd, max_dist)
        _, pixels = ref.pull_map(observed, ref.FIT_FG_MAX, d2, near, gd, max_dist)
        M = ref.weight_maps(owner, v, faces)
        b, y, x, q = pixels
        P = len(b)
        g_abs = np.abs(gd[b, y, x].astype(np.float64))
        D = np.sqrt(d2[b, y, x].astype(np.float64))
        assert P > 200 and D.min() >= 1 and (np.isfinite(max_dist) or D.max() > 7.25)
        h = 1e-4
        bound = g_abs.sum() * h * h / (2 * (1 - h) ** 2) + (8 + P) * 2.0 ** -53 * (g_abs * (D + h)).sum() / h
        worst = 0.0
        for vtx in range(v.shape[1]):
            for c in range(2):
                delta = np.zeros((1, v.shape[1], 2))
                delta[0, vtx, c] = h
                fd = (ref.frozen(delta, M, pixels, d2, gd, S) - ref.frozen(-delta, M, pixels, d2, gd, S)) / (2 * h)
                worst = max(worst, abs(fd - grad[0, vtx, c]))
        print("max_dist %s: %d pixels, fp64 gradient against central differences within %.3g (bound %.3g); largest "
              "|gradient| %.3g" % (max_dist, P, worst, bound, np.abs(grad).max()))
        assert np.abs(grad).max() > 1 and worst <= bound
    # a pixel beyond max_dist, a covered pixel, an unobserved pixel and a zero upstream gradient contribute nothing
    far = np.sqrt(d2.astype(np.float32)) > np.float32(7.25)
    keep = np.zeros(observed.shape, bool)
    keep[b, y, x] = True
    assert not (keep & far).any() and not (keep & (d2 == 0)).any() and not (keep & (gd == 0)).any()
    assert not (keep & ~(observed < ref.FIT_FG_MAX)).any()


def test_the_fit_on_the_restatement_and_the_degenerate_minimum():
    """The mitten observed at rest; the model from s = 0.6, t = (6, -4) px under both halves, sil_cover_ref's steps: it must
    end within |s - 1| <= 0.03 and |t| <= 0.5 px.  The first half alone, from s = 0.6 and t = 0 with every vertex inside the
    observation, has loss exactly 0 and gradient exactly 0 (dt_ref.sample32): the degenerate minimum.
    The fixture is favourable (sil_cover_ref.py says how the outline was placed): with the outline half a pixel off the
    covered pixel centres the two halves balance near s = 0.97, at the edge of the limit.  This shows that the pair grows
    the model back, not that the balance point is robust to the outline's sub-pixel position."""
    rest, faces = ref.mitten()
    observed, _ = ref.render(rest, faces, ref.MITTEN_SIZE, ref.MITTEN_SIZE)
    d2_obs = dt_ref.transform(observed, ref.FIT_FG_MAX)
    value, gxy = dt_ref.sample32(d2_obs, ref.model(rest, ref.FIT_S0, (0.0, 0.0)))
    assert np.all(value == 0) and np.all(gxy == 0)
    s, t, losses = ref.fit(rest, faces, observed, steps=3, t0=(0.0, 0.0), cover=False)
    assert s == float(np.float32(ref.FIT_S0)) and np.all(t == 0) and losses == [0.0, 0.0, 0.0]
    s, t, losses = ref.fit(rest, faces, observed)
    print("restated fit: s = %.4f, t = (%.3f, %.3f) px after %d steps; loss %.3f -> %.3f"
          % (s, t[0], t[1], ref.FIT_STEPS, losses[0], losses[-1]))
    assert losses[0] > 3 and losses[-1] < 0.1 * losses[0]
    assert abs(s - 1) <= 0.03 and float(np.hypot(t[0], t[1])) <= 0.5


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spherehand_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION == 23                                   # additions only
    # host-side argument rules (no launch: every call returns before one)
    assert lib.shr_dt_nearest_workspace_bytes(3, 5, 7) == 3 * 5 * 4 * 4
    assert lib.shr_dt_nearest_workspace_bytes(-1, 5, 7) == -1 and lib.shr_dt_nearest_workspace_bytes(1, 1, 1) == 16
    assert lib.shr_dt_nearest_fwd(None, 0, 5, 7, 1.0, None, None, None, None) == 0           # B == 0: a no-op
    assert lib.shr_dt_nearest_fwd(None, 1, 5, 7, 1.0, None, None, None, None) == -1          # NULL
    assert lib.shr_dt_nearest_fwd(16, 1, 5, 7, 1.0, 16, None, 16, None) == -1                # NULL nearest
    assert lib.shr_dt_nearest_fwd(16, 1, 5, 7, 1.0, 16, 16, 8, None) == -1                   # misaligned workspace
    assert lib.shr_dt_nearest_fwd(16, 1, 5, 7, 1.0, 16, 18, 16, None) == -1                  # misaligned nearest
    assert lib.shr_dt_nearest_fwd(16, 1, 2049, 7, 1.0, 16, 16, 16, None) == -2
    assert lib.shr_dt_nearest_fwd(16, 1, 7, 2049, 1.0, 16, 16, 16, None) == -2
    assert lib.shr_dt_nearest_fwd(16, 65536, 7, 7, 1.0, 16, 16, 16, None) == -2
    assert lib.shr_dt_nearest_fwd(16, 1, 0, 7, 1.0, 16, 16, 16, None) == -1
    assert lib.shr_sil_cover_fwd(None, 1.0, None, 0, 5, 7, 1.0, None, None) == 0             # B == 0
    assert lib.shr_sil_cover_fwd(None, 1.0, 16, 1, 5, 7, 1.0, 16, None) == -1                # NULL
    assert lib.shr_sil_cover_fwd(16, 1.0, 16, 1, 5, 7, -1.0, 16, None) == -1                 # max_dist < 0
    assert lib.shr_sil_cover_fwd(16, 1.0, 16, 1, 5, 7, float("nan"), 16, None) == -1
    assert lib.shr_sil_cover_fwd(16, 1.0, 16, 1, 5, 2049, 1.0, 16, None) == -2
    assert lib.shr_sil_cover_fwd(16, 1.0, 16, 1, 5, 7, 1.0, 18, None) == -1                  # misaligned
    assert lib.shr_sil_cover_bwd_workspace_bytes(-1, 5) == -1
    assert lib.shr_sil_cover_bwd_workspace_bytes(2, 100) == lib.shr_tri_raster_indexed_bwd_workspace_bytes(2, 100)
    ok = dict(observed=16, obs_fg_max=1.0, d2=16, nearest=16, owner=16, vertices=16, faces=16, grad_dist=16, B=1, NV=9, F=4,
              W=7, H=5, max_dist=1.0, grad_vertices=16, workspace=16, stream=None)

    def bwd(**kw):
        return lib.shr_sil_cover_bwd(*dict(ok, **kw).values())

    assert bwd(B=0) == 0                                                                      # a no-op
    for name in ("observed", "d2", "nearest", "owner", "vertices", "faces", "grad_dist", "grad_vertices", "workspace"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(vertices=8) == -1 and bwd(grad_vertices=8) == -1 and bwd(workspace=8) == -1    # 16-byte alignment
    assert bwd(nearest=18) == -1 and bwd(owner=18) == -1
    assert bwd(max_dist=-1.0) == -1 and bwd(max_dist=float("nan")) == -1
    assert bwd(NV=0) == -1 and bwd(F=-1) == -1 and bwd(W=0) == -1
    assert bwd(W=2049) == -2 and bwd(H=2049) == -2 and bwd(B=65536) == -2 and bwd(NV=1 << 30) == -2


def test_unit_compiles_for_gfx950_and_the_transform_has_no_scratch(tmp_path):
    """tests/test_dist_transform_cpu.py's reading of the code-object metadata: the three transform and forward kernels of
    sil_cover.hip report ScratchSize 0, no spills and no static LDS (the row pass asks for its LDS at the launch:
    kDnRowWaves rows of W 8-byte keys, 32 KB at the widest image); the walker's passes (fixed_point.h over CoverTaps) are
    there in both instantiations, and their registers and scratch are printed (DESIGN.md 4.4i records them)."""
    from spherehand_amd import build
    out = str(tmp_path / "sil_cover.s")
    src = os.path.join(build.PKG, "csrc", "sil_cover.hip")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        if ".name:" not in block:                                                # (amdhsa.version's list)
            continue
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                         for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                   "group_segment_fixed_size", "vgpr_count", "sgpr_count")}
    for kernel in ("dn_column_kernel", "dn_row_kernel", "sil_cover_fwd_kernel"):
        hits = [v for n, v in kernels.items() if kernel in n]
        assert len(hits) == 1, (kernel, list(kernels))
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"):
            assert hits[0][key] == 0, (kernel, key, hits[0])
    walkers = {n: v for n, v in kernels.items() if "CoverTaps" in n}
    assert len([n for n in walkers if "mesh_bwd_max_kernel" in n]) == 2
    assert len([n for n in walkers if "mesh_bwd_sum_kernel" in n]) == 3       # LDS, and global with and without runs
    for n, v in sorted(walkers.items()):
        print("%s: %d VGPRs, %d SGPRs, LDS %d B, scratch %d B, spills %d/%d"
              % (n, v["vgpr_count"], v["sgpr_count"], v["group_segment_fixed_size"], v["private_segment_fixed_size"],
                 v["vgpr_spill_count"], v["sgpr_spill_count"]))
    code = open(src).read()
    waves = int(re.search(r"constexpr int kDnRowWaves = (\d+);", code).group(1))
    side = int(re.search(r"constexpr int kDnMaxSide = (\d+);", code).group(1))
    assert "(size_t)kDnRowWaves * W * sizeof(long long)" in code and waves * side * 8 == 32768
    assert "getenv" not in code and "EXP_" not in code and "atomic" not in code.split("struct CoverTaps")[0]
    # the new kernels are not part of dist_transform.hip's code object
    assert "dn_" not in open(os.path.join(build.PKG, "csrc", "dist_transform.hip")).read()
