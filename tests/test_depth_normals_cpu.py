"""The depth-image normals without a device: the fp32 restatement of tests/depth_normals_ref.py on exact planes, in every
case of the two differences, at steps, holes, NaN and inf; the fp64 restatement's autograd against central differences;
the plane fit with the restatement alone; the entries of the C ABI with their argument errors; the unit's code-object
metadata."""
import ctypes
import os
import re
import subprocess

import numpy as np
import torch

import depth_normals_ref as ref
from conftest import ROOT

F32 = np.float32
U = ref.U
ENTRIES = ("shr_depth_normals_fwd", "shr_depth_normals_bwd")
# max |fd - autograd| of test_gradient_against_central_differences at h / 2 = 2^-6 (x86-64, torch fp64; the seed is fixed,
# so the figure repeats).  The test asserts 4 x the measured value, and that the value is not stale.
MEASURED_FD = 4.98e-4


def plane(a, b, c, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (a * xx + b * yy + c)[None].astype(F32)


def unit64(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def test_exact_planes_at_both_scales():
    """z = a x + b y + c with dyadic coefficients: every difference and every product of N is exact, so the map is
    (a sy, b sx, -sx sy) / |.| at every pixel -- interior, border and corner alike -- to unit3's rounding, 4 u."""
    H, W = 48, 40
    from spherehand_amd.render import MeshDataToModelLoss
    ax, _, ay, _ = MeshDataToModelLoss.reference_grid(W, H)
    assert (ax, ay) == (7.5, 6.25)
    for scale in ((1.0, 1.0), (ax, ay)):
        for a, b in ((0.25, -0.5), (0.0, 0.0), (-1.5, 0.125), (0.0, 1.0)):
            out = ref.forward32(plane(a, b, 40.0, H, W), ref.FG_MAX, scale, ref.MAX_STEP)
            want = unit64([a * scale[1], b * scale[0], -scale[0] * scale[1]])
            err = np.abs(out["normals"].transpose(0, 2, 3, 1) - want).max()
            print("plane (%g, %g) scale %s: max |n - exact| %.3g u" % (a, b, scale, err / U))
            assert out["live"].all() and err <= 4 * U
            assert np.all(out["normals"][:, 2] < 0)
    out = ref.forward32(plane(0.0, 0.0, 40.0, H, W), ref.FG_MAX)
    assert np.all(out["normals"][0, :2] == 0) and np.all(out["normals"][0, 2] == -1)


def pixel_by_definition(d, i, j, fg_max, sx, sy, max_step):
    """the contract read pixel by pixel, scalar fp32: (dx, hx, dy, hy) or None for a pixel without a normal"""
    H, W = d.shape
    c = d[i, j]
    if not c < F32(fg_max):
        return None

    def axis(lo, hi):
        use = []
        for (y, x) in (lo, hi):
            ok = 0 <= y < H and 0 <= x < W
            if ok:
                with np.errstate(all="ignore"):
                    ok = bool(d[y, x] < F32(fg_max)) and bool(np.abs(F32(d[y, x] - c)) <= F32(max_step))
            use.append(ok)
        with np.errstate(all="ignore"):
            if use[0] and use[1]:
                return F32(d[hi] - d[lo]), 2
            if use[1]:
                return F32(d[hi] - c), 1
            if use[0]:
                return F32(c - d[lo]), 1
        return None

    x, y = axis((i, j - 1), (i, j + 1)), axis((i - 1, j), (i + 1, j))
    return None if x is None or y is None else x + y


def test_every_case_border_and_corner():
    """An image in which each of the 3 x 3 (horizontal, vertical) cases occurs, with pixels that lack a difference along
    one axis, checked pixel by pixel against the contract read as scalars; then the borders and corners of a full plane."""
    d = ref.random_depth(1, 19, 23, 5)[0]
    out = ref.forward32(d[None], ref.FG_MAX, (1.0, 0.5), ref.MAX_STEP)
    seen, none = {}, 0
    for i in range(d.shape[0]):
        for j in range(d.shape[1]):
            want = pixel_by_definition(d, i, j, ref.FG_MAX, 1.0, 0.5, ref.MAX_STEP)
            assert (want is not None) == bool(out["has"][0, i, j]), (i, j)
            if want is None:
                none += 1
                assert np.all(out["normals"][0, :, i, j] == 0)
                continue
            dx, hx, dy, hy = want
            case = (("both" if hx == 2 else ("r" if out["ur"][0, i, j] else "l")),
                    ("both" if hy == 2 else ("d" if out["ud"][0, i, j] else "u")))
            seen[case] = seen.get(case, 0) + 1
            same = lambda p, q: (np.isnan(p) and np.isnan(q)) or p == q   # noqa: E731
            assert same(out["dx"][0, i, j], dx) and same(out["dy"][0, i, j], dy), (i, j, case)
            assert out["wx"][0, i, j] == hx * 1.0 and out["wy"][0, i, j] == hy * 0.5, (i, j, case)
    print("cases:", seen, "without a normal:", none)
    assert len(seen) == 9 and min(seen.values()) >= 1 and none > 20
    assert (out["site"] & ~out["has"]).sum() >= 1          # a foreground pixel with no usable neighbour along an axis
    # a full plane: the four borders and the four corners take the one-sided forms
    p = plane(0.25, -0.5, 40.0, 6, 7)
    o = ref.forward32(p, ref.FG_MAX)
    for k in ("ul", "ur", "uu", "ud"):
        inner = {"ul": (slice(None), slice(1, None)), "ur": (slice(None), slice(0, -1)), "uu": (slice(1, None), slice(None)),
                 "ud": (slice(0, -1), slice(None))}[k]
        want = np.zeros((6, 7), bool)
        want[inner] = True
        assert np.array_equal(o[k][0], want), k
    assert np.all(o["dx"][0, :, 1:-1] == 0.5) and np.all(o["dx"][0, :, [0, -1]] == 0.25)
    assert np.all(o["dy"][0, 1:-1] == -1.0) and np.all(o["dy"][0, [0, -1]] == -0.5)
    assert np.all(o["wx"][0, :, 1:-1] == 2) and np.all(o["wx"][0, :, [0, -1]] == 1)
    assert np.all(o["wy"][0, 1:-1] == 2) and np.all(o["wy"][0, [0, -1]] == 1)
    for i, j in ((0, 0), (0, 6), (5, 0), (5, 6)):
        assert o["wx"][0, i, j] == 1 and o["wy"][0, i, j] == 1 and o["live"][0, i, j]
    # W == 1 or H == 1: no difference along one axis anywhere
    for shape in ((1, 9), (9, 1), (1, 1)):
        z = ref.forward32(np.full((1,) + shape, 40.0, F32), ref.FG_MAX)
        assert not z["has"].any() and np.all(z["normals"] == 0)


def test_steps_and_holes_never_mix_two_surfaces():
    H, W, k = 12, 16, 8
    a1, a2, b = 0.25, 0.5, -0.5
    d = plane(a1, b, 40.0, H, W)
    d[0, :, k:] = plane(a2, b, 60.0, H, W)[0, :, k:]           # a step of about 20 > max_step between columns k-1 and k
    d[0, 5, 3] = 100.0                                         # a hole of one background pixel in the left surface
    out = ref.forward32(d, ref.FG_MAX, (1.0, 1.0), ref.MAX_STEP)
    n = out["normals"][0].transpose(1, 2, 0)
    left, right = unit64([a1, b, -1.0]), unit64([a2, b, -1.0])
    assert np.all(n[5, 3] == 0) and out["live"].sum() == H * W - 1
    assert not out["ur"][0, :, k - 1].any() and not out["ul"][0, :, k].any()
    assert np.all(out["dx"][0, :, k - 1] == a1) and np.all(out["dx"][0, :, k] == a2)          # one-sided, own surface
    assert not out["ur"][0, 5, 2] and not out["ul"][0, 5, 4] and not out["ud"][0, 4, 3] and not out["uu"][0, 6, 3]
    assert out["dx"][0, 5, 2] == a1 and out["dx"][0, 5, 4] == a1 and out["dy"][0, 4, 3] == b and out["dy"][0, 6, 3] == b
    mask = np.ones((H, W), bool)
    mask[5, 3] = False
    assert np.abs(n[:, :k][mask[:, :k]] - left).max() <= 4 * U and np.abs(n[:, k:] - right).max() <= 4 * U
    # without the rule (max_step = inf) the two columns at the step do mix the surfaces
    mixed = ref.forward32(d, ref.FG_MAX)["normals"][0].transpose(1, 2, 0)
    assert np.abs(mixed[:, k - 1] - left).max() > 0.1 and np.abs(mixed[:, k] - right).max() > 0.1


def test_nan_and_inf_are_no_sites_and_poison_no_neighbour():
    H, W = 9, 11
    want = unit64([0.25, -0.5, -1.0])
    for bad in (np.nan, np.inf):
        for max_step in (ref.MAX_STEP, np.inf):
            d = plane(0.25, -0.5, 40.0, H, W)
            d[0, 4, 5] = bad
            d[0, 0, 0] = bad
            out = ref.forward32(d, ref.FG_MAX, (1.0, 1.0), max_step)
            n = out["normals"][0].transpose(1, 2, 0)
            assert not out["site"][0, 4, 5] and not out["site"][0, 0, 0]
            assert np.all(n[4, 5] == 0) and np.all(n[0, 0] == 0) and np.isfinite(n).all()
            assert out["live"].sum() == H * W - 2
            assert np.abs(n[out["live"][0]] - want).max() <= 4 * U
    # -inf is below every fg_max: a site by the rule, infinitely far from its neighbours.  A finite max_step cuts it off
    # (it has no normal, its neighbours go one-sided).  With max_step = inf it is a usable neighbour: the differences of
    # its four neighbours are infinite and the zero rule gives them 0, while its own central differences do not read it.
    # Nothing is ever NaN or inf in the output.
    d = plane(0.25, -0.5, 40.0, H, W)
    d[0, 4, 5] = -np.inf
    out = ref.forward32(d, ref.FG_MAX, (1.0, 1.0), ref.MAX_STEP)
    assert out["site"][0, 4, 5] and not out["has"][0, 4, 5] and out["live"].sum() == H * W - 1
    assert np.abs(out["normals"][0].transpose(1, 2, 0)[out["live"][0]] - want).max() <= 4 * U
    out = ref.forward32(d, ref.FG_MAX)
    dead = ~out["live"][0]
    assert dead.sum() == 4 and dead[4, 4] and dead[4, 6] and dead[3, 5] and dead[5, 5] and np.isfinite(out["normals"]).all()


def test_gradient_against_central_differences():
    """L(depth) = <g, normals64(depth)> on a smooth random height field with holes (values on a 2^-10 grid: +-h is exact
    in fp32).  Only pixels are perturbed for which +-2 h leaves every fp32 decision of the image unchanged.  Central
    differences at h and h / 2: the discrepancy to the autograd gradient falls by about 4 (second order)."""
    H, W, h = 24, 28, 2.0 ** -5
    d = ref.smooth_field(H, W, 3)
    dec = ref.forward32(d, ref.FG_MAX, (1.0, 1.0), ref.MAX_STEP)
    g = np.random.RandomState(7).standard_normal(dec["normals"].shape)
    analytic = ref.grad64(d, g, ref.FG_MAX, (1.0, 1.0), ref.MAX_STEP)[0]
    assert (~dec["site"]).sum() > 20 and (dec["has"] & ~(dec["ul"] & dec["ur"])).sum() > 40
    keep = []
    for i, j in np.argwhere(dec["site"][0]):
        same = True
        for s in (-2 * h, 2 * h):
            e = d.copy()
            e[0, i, j] += F32(s)
            o = ref.forward32(e, ref.FG_MAX, (1.0, 1.0), ref.MAX_STEP)
            same = same and all(np.array_equal(o[k], dec[k]) for k in ref.DECISIONS)
        if same:
            keep.append((i, j))
    assert len(keep) > 0.9 * dec["site"].sum()
    gt = torch.from_numpy(g)

    def L(z):
        return float((ref.normals64(torch.from_numpy(z), dec) * gt).sum())

    err = []
    for step in (h, h / 2):
        worst = 0.0
        for i, j in keep:
            up, dn = d.astype(np.float64), d.astype(np.float64)
            up[0, i, j] += step
            dn[0, i, j] -= step
            worst = max(worst, abs((L(up) - L(dn)) / (2 * step) - analytic[i, j]))
        err.append(worst)
    print("central differences over %d pixels: |fd - autograd| %.3g at h = 2^-5, %.3g at h / 2: ratio %.2f; largest "
          "|gradient| %.3g (measured %.3g)" % (len(keep), err[0], err[1], err[0] / err[1], np.abs(analytic).max(), MEASURED_FD))
    assert np.abs(analytic).max() > 0.5 and 3.5 < err[0] / err[1] < 4.5
    assert MEASURED_FD / 4 <= err[1] <= 4 * MEASURED_FD
    assert np.all(analytic[~dec["site"][0]] == 0) and np.all(analytic[ref.structural_zero(dec)[0]] == 0)


def test_plane_fit_with_the_restatement():
    """tilt_grid's plane observed at FIT_TARGET, from (0, 0): the model map is the restated depth normals of the model
    plane's exact depth, the observed map those of the target's, the loss NormalConsistencyLoss restated in fp64."""
    t, losses = ref.plane_fit(ref.restated_plane_map)
    print("plane fit: (a, b) = %s after %d steps, loss %.3g -> %.3g" % (t, len(losses), losses[0], losses[-1]))
    assert np.abs(t - np.asarray(ref.tn.FIT_TARGET)).max() <= 0.01
    assert all(b <= a + 1e-15 for a, b in zip(losses, losses[1:])) and losses[-1] < 1e-3 * losses[0]
    # the restated loss is the module's (CPU tensors): the same numbers
    from spherehand_amd.render import NormalConsistencyLoss
    m = ref.restated_plane_map(torch.tensor(0.1, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))
    o = ref.restated_plane_map(*(torch.tensor(v, dtype=torch.float64) for v in ref.tn.FIT_TARGET))
    m = torch.cat([m, torch.zeros_like(m)])                       # a crop without a common pixel: 0
    o = torch.cat([o, o])
    got = NormalConsistencyLoss()(m, o)
    assert torch.equal(got, ref.loss64(m, o)) and got[1] == 0 and got[0] > 0
    assert NormalConsistencyLoss().loss(m, o) == got.mean()


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spherehand_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    lib = _lib.lib()
    assert lib.shr_abi_version() == _lib.ABI_VERSION
    inf, nan = float("inf"), float("nan")
    # host-side argument rules (no launch: every call returns before one)
    fwd = [16, 1, 9, 8, 99.0, 1.0, 1.0, inf, 1 << 20, None]
    bad = lambda i, val: lib.shr_depth_normals_fwd(*(fwd[:i] + [val] + fwd[i + 1:]))   # noqa: E731
    assert bad(1, 0) == 0                                                              # B == 0: a no-op
    assert bad(0, None) == -1 and bad(8, None) == -1 and bad(0, 18) == -1 and bad(8, 18) == -1
    assert bad(8, 16) == -1 and bad(8, 16 + 9 * 8 * 4 - 4) == -1 and bad(0, (1 << 20) + 3 * 9 * 8 * 4 - 4) == -1   # overlap
    assert bad(1, -1) == -1 and bad(2, 0) == -1 and bad(3, 0) == -1
    assert bad(4, nan) == -1 and bad(7, nan) == -1 and bad(7, -0.5) == -1
    for i in (5, 6):
        assert bad(i, 0.0) == -1 and bad(i, -1.0) == -1 and bad(i, inf) == -1 and bad(i, nan) == -1, i
    assert bad(1, 65536) == -2 and bad(2, 65536) == -2 and bad(3, 65536) == -2
    bwd = [16, 1 << 20, 1, 9, 8, 99.0, 1.0, 1.0, 2.0, 1 << 21, None]
    bad = lambda i, val: lib.shr_depth_normals_bwd(*(bwd[:i] + [val] + bwd[i + 1:]))   # noqa: E731
    assert bad(2, 0) == 0
    assert bad(0, None) == -1 and bad(1, None) == -1 and bad(9, None) == -1 and bad(1, (1 << 20) + 2) == -1
    assert bad(9, 16) == -1 and bad(9, 1 << 20) == -1 and bad(9, (1 << 20) + 3 * 9 * 8 * 4 - 4) == -1             # overlap
    assert bad(5, nan) == -1 and bad(8, nan) == -1 and bad(8, -1.0) == -1 and bad(6, 0.0) == -1 and bad(7, inf) == -1
    assert bad(2, -1) == -1 and bad(3, 0) == -1 and bad(4, 0) == -1
    assert bad(2, 65536) == -2 and bad(3, 65536) == -2 and bad(4, 65536) == -2


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_mesh_d2m_cpu.py's reading of the code-object metadata: both kernels of depth_normals.hip report
    ScratchSize 0, no spills and no LDS; the backward stays at or below 64 VGPRs (eight waves per SIMD; DESIGN.md 4.4k
    has the figures)."""
    from spherehand_amd import build
    out = str(tmp_path / "depth_normals.s")
    src = os.path.join(build.PKG, "csrc", "depth_normals.hip")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(s) for s in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == 2 and max(sizes) == 0, sizes
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(x) for k, x in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
                                                          r"group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", block)}
    assert len(kernels) == 2
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["group_segment_fixed_size"] == 0 and k["vgpr_count"] <= 64, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "depth_normals_bwd_kernel" in design[design.index("### 4.4k"):design.index("### 4.5 ")]
