"""The silhouette distance transform and its sampler without a GPU: the restatements of tests/dt_ref.py against each other
(separable against brute force, fp32 against fp64, the fp64 gradient against central differences, the translation fit),
the header, loader and exports, and the new unit's code-object resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
ENTRIES = ("shr_dt_workspace_bytes", "shr_dt_fwd", "shr_dt_sample_fwd", "shr_dt_sample_bwd")


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (3, 13), (17, 19), (9, 33)])
def test_separable_equals_brute_force(H, W):
    for k, density in enumerate((0.0, 0.01, 0.1, 0.5)):
        for seed in range(3):
            site = np.random.RandomState(100 * k + seed).rand(H, W) < density
            want, got = ref.dt_brute(site), ref.dt_separable(site)
            assert got.dtype == np.int32 and np.array_equal(got, want), (H, W, density, seed)
            if site.any():
                assert np.all(got[site] == 0) and got.max() <= (H - 1) ** 2 + (W - 1) ** 2
    one = np.zeros((H, W), bool)
    one[H - 1, 0] = True                                         # one site in a corner: the far corner is the diagonal
    assert ref.dt_separable(one)[0, W - 1] == (H - 1) ** 2 + (W - 1) ** 2


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (17, 19), (2048, 1)])
def test_the_empty_image(H, W):
    empty = np.zeros((H, W), bool)
    for fn in (ref.dt_brute, ref.dt_separable):
        out = fn(empty)
        assert np.all(out == H * H + W * W)
    assert H * H + W * W > (H - 1) ** 2 + (W - 1) ** 2
    assert 2 * 2048 * 2048 < 2 ** 24 and np.float32(2 * 2048 * 2048 - 1) == 2 * 2048 * 2048 - 1    # exact in fp32
    # NaN and fg_max itself are not sites
    depth = np.array([[np.nan, 5.0], [4.999, 7.0]], np.float32)
    assert np.array_equal(ref.sites(depth, 5.0), [[False, False], [True, False]])


def _sampler_case(seed=0, H=37, W=41, N=4000):
    rs = np.random.RandomState(seed)
    d2 = ref.dt_separable(rs.rand(H, W) < 0.01)[None]
    p = np.stack([rs.uniform(-3, W + 2, N), rs.uniform(-3, H + 2, N)], -1)
    p[:200] = np.round(p[:200])                                  # integer coordinates
    p[200:220, 0], p[220:240, 1] = W - 1, H - 1
    p[240:260] = rs.uniform(0, 1, (20, 2)) * [1e-6, 1.0]           # the first cell, where 1 - fx rounds
    return d2, p[None].astype(np.float32)


def test_fp32_sampler_is_within_4_ulp_of_fp64():
    """value is a convex combination of four taps: two products and an add give top and bot (each product within u of
    itself, the add within u of top: 2 u top), two products and an add give the value (u (top uy + bot fy) + u value on
    top of the inherited 2 u): at most four roundings of terms no larger than the largest tap T, 4 u T.  (1 - f is exact
    for f a multiple of 2^-24, which xc - floor(xc) is from xc >= 1 on; in the first cell it is within u / 2.)  gx: the
    difference, the product and the add, 3 u T at most; gy = bot - top carries the two 2 u.  Bound: 4 u T for all three,
    u = 2^-24; T = the largest of the point's taps."""
    d2, p = _sampler_case()
    for max_dist in (np.inf, 6.5):
        v32, g32 = ref.sample32(d2, p, max_dist)
        v64, g64, T = ref.sample64(d2, p.astype(np.float64), max_dist)
        assert v32.dtype == np.float32 and g32.dtype == np.float32 and T.max() > 3
        ev = np.abs(v32.astype(np.float64) - v64) / T
        eg = np.abs(g32.astype(np.float64) - g64).max(-1) / T
        print("max_dist %s: value within %.3g u T, gradient within %.3g u T" % (max_dist, ev.max() / U, eg.max() / U))
        assert ev.max() <= 4 * U and eg.max() <= 4 * U
        if np.isfinite(max_dist):
            assert v32.max() <= max_dist * (1 + 4 * U) and (T == np.float32(max_dist)).any()      # saturated taps
    # clamped components and non-finite points
    out = np.array([[[-2.5, 3.25], [3.25, -0.5], [50.0, 3.5], [3.5, 40.0], [np.nan, 2], [2, np.inf], [40, 36]]], np.float32)
    v, g = ref.sample32(d2, out)
    assert np.all(g[0, [0, 2], 0] == 0) and np.all(g[0, [1, 3], 1] == 0) and np.all(v[0, 4:6] == 0) and np.all(g[0, 4:6] == 0)
    inside = np.array([[[0.0, 3.25], [3.25, 0.0], [50.0, 3.5], [3.5, 40.0], [0, 0], [0, 0], [40, 36]]], np.float32)
    assert np.array_equal(v[0, :4], ref.sample32(d2, inside)[0][0, :4])             # the border's value
    assert g[0, 6, 0] != 0 or g[0, 6, 1] != 0 or v[0, 6] == 0                        # x = W-1, y = H-1: not clamped
    gp = ref.sample_bwd32(g, np.full((1, 7), 0.5, np.float32), 4)
    assert gp.shape == (1, 7, 4) and np.all(gp[..., 2:] == 0) and np.array_equal(gp[..., :2], np.float32(0.5) * g)


def test_fp64_gradient_matches_central_differences():
    """Inside a cell the sampled function is bilinear: linear in x at fixed y and in y at fixed x, so a central difference
    is exact up to rounding: each of its two evaluations makes at most 8 fp64 roundings of terms <= T, and its coordinate
    p +- h is rounded to 2^-53 max(H, W), which the slope (at most T per pixel) carries into the value; over 2 h:
    |difference| <= (8 + max(H, W)) * 2^-53 * T / h."""
    d2, _ = _sampler_case(1)
    H, W = d2.shape[1:]
    rs = np.random.RandomState(5)
    cell = np.stack([rs.randint(0, W - 1, 3000), rs.randint(0, H - 1, 3000)], -1)
    p = (cell + rs.uniform(0.05, 0.95, (3000, 2)))[None]         # at least 0.05 from a cell border
    h = 1e-3
    _, g, T = ref.sample64(d2, p)
    worst = 0.0
    for d in range(2):
        e = np.zeros(2)
        e[d] = h
        fd = (ref.sample64(d2, p + e)[0] - ref.sample64(d2, p - e)[0]) / (2 * h)
        worst = max(worst, (np.abs(fd - g[..., d]) / np.maximum(T, 1e-300)).max())
    bound = (8 + max(H, W)) * 2.0 ** -53 / h
    print("fp64 gradient against central differences: within %.3g T (bound %.3g T); largest |gradient| %.3g"
          % (worst, bound, np.abs(g).max()))
    assert np.abs(g).max() > 0.5 and worst <= bound
    # outside the silhouette and away from its medial axis the gradient is a unit vector up to the bilinear
    # interpolation of a cone: its length is 1 within a few percent three pixels out
    far = T[0] > 6
    length = np.sqrt((g[0][far] ** 2).sum(-1))
    assert far.sum() > 100 and np.median(np.abs(length - 1)) < 0.02


@pytest.mark.parametrize("lr", [8.0, 16.0])
def test_translation_fit_on_the_restatement(lr):
    """The toy silhouette at 128 x 128, 1 500 points inside it moved by (25, 18) px, the translation fitted by plain
    gradient descent on the mean sampled distance alone, 50 steps: it ends under 0.5 px."""
    site = ref.toy_silhouette()
    assert site[:, :8].sum() == 0 and site[:8].sum() == 0
    d2 = ref.dt_separable(site)[None]
    p = ref.points_inside(site, 1500)
    assert ref.sample32(d2, p)[0].max() < 1                      # every point starts inside (a border pixel's cell reaches out)
    moved = p + np.array([25, 18], np.float32)
    assert moved[..., 0].max() < 127 and moved[..., 1].max() < 127
    t, losses = ref.fit(d2, moved, 50, lr)
    err = float(np.hypot(t[0] - 25, t[1] - 18))
    print("step %g: offset error %.4f px after 50 steps; loss %.4g -> %.4g" % (lr, err, losses[0], losses[-1]))
    assert losses[0] > 5 and err < 0.5 and losses[-1] < 0.1 * losses[0]


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spherehand_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    lib = _lib.lib()
    # host-side argument rules (no launch: every call returns before one)
    assert lib.shr_dt_workspace_bytes(3, 5, 7) == 3 * 5 * 4 * 4 and lib.shr_dt_workspace_bytes(-1, 5, 7) == -1
    assert lib.shr_dt_workspace_bytes(1, 1, 1) == 16                                  # rounded up to 16 bytes
    assert lib.shr_dt_fwd(None, 0, 5, 7, 1.0, None, None, None) == 0                  # B == 0: a no-op
    assert lib.shr_dt_fwd(None, 1, 5, 7, 1.0, None, None, None) == -1                 # NULL
    assert lib.shr_dt_fwd(16, 1, 5, 7, 1.0, 16, 8, None) == -1                        # misaligned workspace
    assert lib.shr_dt_fwd(16, 1, 2049, 7, 1.0, 16, 16, None) == -2
    assert lib.shr_dt_fwd(16, 1, 7, 2049, 1.0, 16, 16, None) == -2
    assert lib.shr_dt_fwd(16, 65536, 7, 7, 1.0, 16, 16, None) == -2
    assert lib.shr_dt_fwd(16, 1, 0, 7, 1.0, 16, 16, None) == -1
    assert lib.shr_dt_sample_fwd(16, 1, 1, 7, 16, 4, 2, 1.0, 16, 16, None) == -1      # H = 1
    assert lib.shr_dt_sample_fwd(16, 1, 7, 7, 16, 4, 1, 1.0, 16, 16, None) == -1      # C = 1
    assert lib.shr_dt_sample_fwd(16, 1, 7, 7, 16, 4, 2, -1.0, 16, 16, None) == -1     # max_dist < 0
    assert lib.shr_dt_sample_fwd(16, 1, 7, 7, 16, 4, 2, float("nan"), 16, 16, None) == -1
    assert lib.shr_dt_sample_fwd(16, 1, 7, 7, 16, 1 << 30, 2, 1.0, 16, 16, None) == -2
    assert lib.shr_dt_sample_fwd(16, 1, 7, 7, None, 4, 2, 1.0, 16, 16, None) == -1
    assert lib.shr_dt_sample_fwd(16, 1, 7, 7, None, 0, 2, 1.0, 16, 16, None) == 0     # N == 0: a no-op
    assert lib.shr_dt_sample_bwd(None, 16, 1, 4, 2, 16, None) == -1
    assert lib.shr_dt_sample_bwd(16, 16, 65536, 4, 2, 16, None) == -2
    assert lib.shr_dt_sample_bwd(None, None, 0, 4, 2, None, None) == 0


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_tri_normals_cpu.py's reading of the code-object metadata: the four kernels of dist_transform.hip report
    ScratchSize 0, no spills and no static LDS; the row pass asks for its LDS at the launch -- kDtRowWaves rows of W ints,
    32 KB at the widest image."""
    from spherehand_amd import build
    out = str(tmp_path / "dist_transform.s")
    src = os.path.join(build.PKG, "csrc", "dist_transform.hip")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(s) for s in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == 4 and max(sizes) == 0, sizes
    meta = text[text.index("amdhsa.kernels:"):]
    names = re.findall(r"\.name:\s+(\S+)", meta)
    for kernel in ("dt_column_kernel", "dt_row_kernel", "dt_sample_fwd_kernel", "dt_sample_bwd_kernel"):
        assert len([n for n in names if kernel in n]) == 1, names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"):
        vals = [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % key, meta)]
        assert len(vals) == 4 and max(vals) == 0, (key, vals)
    code = open(src).read()
    waves = int(re.search(r"constexpr int kDtRowWaves = (\d+);", code).group(1))
    side = int(re.search(r"constexpr int kDtMaxSide = (\d+);", code).group(1))
    assert "(size_t)kDtRowWaves * W * sizeof(int)" in code and waves * side * 4 == 32768
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "16·W B" in design[design.index("### 4.4h"):design.index("### 4.5 ")]
