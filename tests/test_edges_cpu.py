"""CPU: the oracle against the EDGE fixtures (tests/golden/g_edges_sphere.npz, g_edges_d2m.npz), recorded by
tests/golden/make_goldens_edges.py from the running reference on scenes that sit on the rules: exact ties, a hit at
exactly 100.0, the 0.01 clamp, radii <= 0, the 99 threshold, points at a centre / on a surface / on the clamp at 50,
non-finite records.

Non-finite gradients: wherever the reference's gradient entry is finite, ours equals it at the same bar (an exact zero
stays an exact zero); where the reference's entry is NaN, ours is not compared.  Scenes whose reference gradient is NaN
in EVERY entry are listed by name below, and the list must equal what the fixtures show."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits, golden

# reference gradient NaN in every entry: nothing to compare there (a NaN depth pixel poisons the crop's mean)
ALL_NAN_GRADIENT_SCENES = ["a/nan_depth_pixel", "b/nan_depth_pixel"]
# q = r^2 - dx^2 - dy^2 exactly 0.01f has no construction on a pixel centre (no float squares to 0.01f; off the centre q
# is a multiple of an ulp of r^2 >> ulp(0.01)): the fixture holds its two fp32 neighbours, found at r = 0.1f and below
CLAMP_Q_FOUND = [False, True, True]


def sphere_groups():
    g = golden("g_edges_sphere.npz")
    for tag in g["groups"]:
        H, W = (int(x) for x in g[tag + "_hw"])
        yield g, str(tag), H, W


def d2m_groups():
    g = golden("g_edges_d2m.npz")
    for tag in g["groups"]:
        H, W = (int(x) for x in g[tag + "_hw"])
        yield g, str(tag), H, W


def check_gradient(name, ours, ref, rel, floor, fails):
    """ours against the reference's gradient of one scene where the reference is finite; its exact zeros exactly."""
    fin = np.isfinite(ref)
    if not fin.any():
        return
    tol = rel * np.abs(ref[fin]).max() + floor
    with np.errstate(invalid="ignore"):
        err = np.abs(ours[fin] - ref[fin])
    if not (err <= tol).all():        # (a NaN of ours where the reference is finite fails here)
        fails.append("%s: gradient err %s > %.3g\n ours %s\n ref %s" % (name, np.nanmax(err) if np.isfinite(err).any() else "nan",
                                                                        tol, ours.tolist(), ref.tolist()))
    zero = fin & (ref == 0)
    if not np.all(ours[zero] == 0):
        fails.append("%s: an exact zero of the reference is %s" % (name, ours[zero][ours[zero] != 0][:4]))


def check_depth(name, d, a, ref_d, ref_a, fails):
    """NaN pattern equal, bits equal elsewhere; owner equal on the foreground -- depth != 100.0, where torch.min's index
    is necessarily a hit (a miss is exactly 100).  Who owns a pixel AT 100.0 shows in the gradients, which are compared."""
    if not np.array_equal(np.isnan(d), np.isnan(ref_d)):
        fails.append("%s: NaN pattern differs at %d px" % (name, int((np.isnan(d) != np.isnan(ref_d)).sum())))
        return
    ok = ~np.isnan(ref_d)
    if not np.array_equal(bits(d)[ok], bits(ref_d)[ok]):
        fails.append("%s: depth bits differ at %d px" % (name, int((bits(d)[ok] != bits(ref_d)[ok]).sum())))
    fg = bits(ref_d) != bits(np.float32(100.0))
    if a is not None and not np.array_equal(a[fg], ref_a[fg]):
        fails.append("%s: owner differs at %d foreground px" % (name, int((a[fg] != ref_a[fg]).sum())))


def test_fixtures_record_version_and_scene_names():
    for name in ("g_edges_sphere.npz", "g_edges_d2m.npz"):
        g = golden(name)
        assert str(g["torch_version"])[0].isdigit()
        assert len(g["scene_names"]) == len(set(g["scene_names"])) > 40
    g = golden("g_edges_sphere.npz")
    assert list(g["clamp_q_found"]) == CLAMP_Q_FOUND
    names = set(g["scene_names"])
    assert {"a3/clamp_q_above", "b3/clamp_q_below", "a64/dup_front_j64", "b3/huge_x_r", "a3/r_below_1e6", "c3/hit100_twice"} <= names
    assert [int(g["b3_hw"][1]) % 4, int(g["a3_hw"][1]) % 4] == [2, 0]
    assert g["a64_spheres"].shape[1] == 64 and g["a3_spheres"].shape[1] == 3


def test_sphere_rules_the_scenes_pin():
    """What the reference does on each rule, read off the fixture: a regenerated fixture whose scene has drifted off its
    rule fails here."""
    g = golden("g_edges_sphere.npz")
    hundred = bits(np.float32(100.0))
    for tag in ("a3", "b3", "c3"):
        H, W = (int(x) for x in g[tag + "_hw"])
        names = [str(n) for n in g[tag + "_names"]]
        sc = lambda n: names.index(n)
        depth, arg, grad, up, sp = (g[tag + k] for k in ("_depth", "_argmin", "_grad", "_upstream", "_spheres"))
        own = np.where(bits(depth) != hundred, arg, 255)                # the owner where the depth is not the background's
        tv, tu = H - 3, W - 3                                           # the pixel the hit100 scenes aim at
        for n, owner in (("hit100_lower_misses", None), ("hit100_lower_deeper", 1), ("hit100_first", 0), ("hit100_twice", 1)):
            i = sc(n)
            assert bits(depth[i])[tv, tu] == hundred, (tag, n)        # the hit lands on exactly 100.0
            tie = [j for j in range(3) if sp[i, j, 2] == 102.0]
            if owner is None:                                           # a lower index misses: its background owns, no gradient
                assert arg[i, tv, tu] == 0 and all(grad[i, j, 2] == 0 for j in tie), (tag, n)
            else:                                                       # the tie sphere's only pixel: d/dz is that pixel's g
                assert arg[i, tv, tu] == owner and grad[i, owner, 2] == up[i, tv, tu], (tag, n)
                assert all(grad[i, j, 2] == 0 for j in tie if j != owner), (tag, n)
        # two identical spheres: bit-equal part maps, the first owns every pixel either could, the second gets nothing
        for n, first, second in (("dup_front", 0, 1), ("dup_front_late", 1, 2)):
            i = sc(n)
            assert np.array_equal(bits(sp[i, first]), bits(sp[i, second]))
            assert (own[i] == first).sum() > 4 and not (own[i] == second).any() and not grad[i, second].any(), (tag, n)
            assert grad[i, first].any()
        # mirrored spheres tie on the column x = 0: the lower index owns it, the two own as many pixels elsewhere
        for n, lo, hi in (("mirror_tie", 0, 1), ("mirror_tie_swapped", 0, 2)):
            i, uc = sc(n), W // 2
            assert (own[i][:, uc] == lo).sum() >= 2 and not (own[i][:, uc] == hi).any(), (tag, n)
            assert (own[i] == lo).sum() - (own[i][:, uc] == lo).sum() == (own[i] == hi).sum() > 0, (tag, n)
        assert depth[sc("all_behind_covering")].min() > 100.0 and np.all(bits(depth[sc("all_behind_partial")]) == hundred)
        assert np.all(bits(depth[sc("all_off_screen")]) == hundred)
        assert depth[sc("centre_behind_background")].min() < 100.0
        assert np.isnan(depth[sc("nan_x")]).all() and np.isnan(depth[sc("nan_r")]).all()
        nz = np.isnan(depth[sc("nan_z_twice")])
        assert set(arg[sc("nan_z_twice")][nz]) == {0, 1}               # the first NaN where both hit, the second where it alone does
        assert np.isneginf(depth[sc("minus_inf_z")]).any() and np.isneginf(depth[sc("inf_r")]).all()
        if tag != "c3":
            above, below = sc("clamp_q_above"), sc("clamp_q_below")
            assert arg[above, tv, tu] == 0 and depth[above, tv, tu] < 50.0 and bits(depth[below])[tv, tu] == hundred
            assert grad[sc("negative_radius")][0, 3] * grad[sc("negative_radius")][0, 2] != 0
            assert not grad[sc("zero_radius")][[0, 2]].any()


def test_sphere_depth_and_owner(oracle):
    fails = []
    for g, tag, H, W in sphere_groups():
        d, a = oracle.sphere_raster_fwd(g[tag + "_spheres"], H, W)
        for i, n in enumerate(g[tag + "_names"]):
            check_depth("%s/%s" % (tag, n), d[i], a[i], g[tag + "_depth"][i], g[tag + "_argmin"][i], fails)
            assert np.all(d[i][a[i] == 255] == 100.0)            # no owner: the background's value
    assert not fails, "\n".join(fails)


def test_sphere_gradients(oracle):
    """The bar of test_oracle_sphere.py::test_g3_gradients, 1e-6 * max|ref| + 1e-5, per scene."""
    fails = []
    for g, tag, H, W in sphere_groups():
        gs = oracle.sphere_raster_bwd(g[tag + "_spheres"], g[tag + "_upstream"])
        for i, n in enumerate(g[tag + "_names"]):
            check_gradient("%s/%s" % (tag, n), gs[i], g[tag + "_grad"][i], 1e-6, 1e-5, fails)
    assert not fails, "\n".join(fails)


def test_sphere_nan_radius_passes_no_gradient_to_x_and_y(oracle):
    """The deviation this fixture found: torch.clamp(min) passes no gradient for a NaN argument, so a NaN radius leaves
    d/dx = d/dy = 0 (d/dz finite, d/dr NaN), and a NaN x leaves d/dy = d/dr = 0."""
    g = golden("g_edges_sphere.npz")
    for tag in ("a3", "b3"):
        names = list(g[tag + "_names"])
        gs = oracle.sphere_raster_bwd(g[tag + "_spheres"], g[tag + "_upstream"])
        for scene, zero, nan in (("nan_r", [0, 1], 3), ("nan_x", [1, 3], 0)):
            row, ref = gs[names.index(scene)][1], g[tag + "_grad"][names.index(scene)][1]
            assert np.all(ref[zero] == 0) and np.isnan(ref[nan]) and np.isfinite(ref[2]) and ref[2] != 0
            assert np.all(row[zero] == 0) and np.isnan(row[nan]) and abs(row[2] - ref[2]) <= 1e-6 * abs(ref[2]) + 1e-5


def test_sphere_sse_of_the_fused_kernel(oracle):
    """The fixture's per-crop ((depth - target)^2).sum() and its gradient against the oracle's depth and backward, at the
    bars the fused kernel is held to (tools/fuzz.py): 1e-5 * max + 1e-3 and 2e-5 * max + 1e-3."""
    fails = []
    for g, tag, H, W in sphere_groups():
        sp, tgt = g[tag + "_spheres"], g[tag + "_target"]
        d = oracle.sphere_raster_fwd(sp, H, W, want_argmin=False)
        with np.errstate(invalid="ignore", over="ignore"):
            e = d.astype(np.float64) - tgt
            sse = (e * e).reshape(len(sp), -1).sum(1)
            gs = oracle.sphere_raster_bwd(sp, (2 * (d - tgt)).astype(np.float32))
        ref = g[tag + "_sse"].astype(np.float64)
        for i, n in enumerate(g[tag + "_names"]):
            name = "%s/%s sse" % (tag, n)
            if np.isfinite(ref[i]):
                if not abs(sse[i] - ref[i]) <= 1e-5 * ref[i] + 1e-3:
                    fails.append("%s: %r against %r" % (name, sse[i], ref[i]))
            elif not (np.isnan(sse[i]) == np.isnan(ref[i]) and (np.isnan(ref[i]) or sse[i] == ref[i])):
                fails.append("%s: %r against %r" % (name, sse[i], ref[i]))
            check_gradient(name, gs[i], g[tag + "_sse_grad"][i], 2e-5, 1e-3, fails)
    assert not fails, "\n".join(fails)


def test_restated_nan_inf_crops_are_in_the_fixture(oracle):
    """test_oracle_sphere.py::test_nan_and_inf_semantics' three crops, here against the reference's own output."""
    sp = np.array([[[0, 0, 10, 20], [np.nan, 0, 0, 5]],
                   [[0, 0, np.nan, 20], [50, 50, 0, 5]],
                   [[np.inf, 0, 0, 20], [0, 0, 5, 30]]], np.float32)
    g = golden("g_edges_sphere.npz")
    assert np.array_equal(bits(g["r2_spheres"]), bits(sp)) and list(g["r2_hw"]) == [16, 16]
    d, a = oracle.sphere_raster_fwd(sp, 16, 16)
    fails = []
    for i in range(3):
        check_depth("r2/%d" % i, d[i], a[i], g["r2_depth"][i], g["r2_argmin"][i], fails)
    assert not fails, "\n".join(fails)
    ref = g["r2_depth"]                                # the restated expectations hold for the reference itself
    assert np.isnan(ref[0]).all() and 0 < np.isnan(ref[1]).sum() < 256 and not np.isnan(ref[2]).any()


def test_data_to_model(oracle):
    """Loss at test_losses_gpu.py's golden bar (1e-5 relative), gradient at 1e-5 * max|ref| + 1e-9, zeros exact."""
    fails, all_nan = [], []
    for g, tag, H, W in d2m_groups():
        for i, n in enumerate(g[tag + "_names"]):
            name = "%s/%s" % (tag, n)
            dep, cen, rad = g[tag + "_depth"][i:i + 1], g[tag + "_centres"][i:i + 1], g[tag + "_radii"][i]
            loss = oracle.data_to_model_loss(dep, cen, rad)
            grad = oracle.data_to_model_bwd(dep, cen, rad)[0]              # the oracle's is the gradient of the mean
            ref, ref_grad = float(g[tag + "_loss"][i]), g[tag + "_grad"][i]
            if np.isnan(ref) or np.isnan(loss):
                if not (np.isnan(ref) and np.isnan(loss)):
                    fails.append("%s: loss %r against %r" % (name, loss, ref))
            elif not abs(loss - ref) <= 1e-5 * abs(ref):
                fails.append("%s: loss %r against %r" % (name, loss, ref))
            check_gradient(name, grad, ref_grad, 1e-5, 1e-9, fails)
            if np.isnan(ref_grad).all():
                all_nan.append(name)
    assert not fails, "\n".join(fails)
    assert all_nan == ALL_NAN_GRADIENT_SCENES


def test_data_to_model_rules_the_scenes_pin():
    """What the reference does on each rule, read off the fixture (so a regenerated fixture that stopped sitting on the
    rule fails here, not silently)."""
    g = golden("g_edges_d2m.npz")
    for tag in g["groups"]:
        H, W = (int(x) for x in g[tag + "_hw"])
        names = list(g[tag + "_names"])
        loss = dict(zip(names, g[tag + "_loss"] * (H * W)))
        grad = dict(zip(names, g[tag + "_grad"] * np.float32(H * W)))
        assert abs(loss["point_at_centre"] - 10.0) < 1e-4 and not grad["point_at_centre"].any()
        assert loss["point_on_surface"] == 0.0 and not grad["point_on_surface"].any()
        assert abs(loss["term_exactly_50"] - 50.0) < 1e-4 and abs(grad["term_exactly_50"][0, 2] - 1.0) < 1e-5   # kept on the clamp
        assert abs(grad["term_50_nearer"][0, 2] - 1.0) < 1e-5 and not grad["term_50_farther"].any()
        assert loss["depth_99"] > 0 and loss["depth_99_below"] > 0 and loss["depth_99_above"] == 0     # background = d > 99
        assert loss["depth_100"] == 0 and loss["all_background"] == 0
        first, late = grad["identical_spheres"], grad["identical_spheres_late"]
        assert first[0].any() and not first[1].any() and late[1].any() and not late[2].any()          # the first owns
        assert not grad["farther_than_1km"].any() and abs(loss["farther_than_1km"] - 50.0) < 1e-4
        assert abs(grad["near_centre_above"][0, 2] - 1.0) < 1e-5 and abs(grad["near_centre_below"][0, 2] + 1.0) < 1e-5   # inside: pushed away
    at, nearer, farther = g["collision_loss"]
    assert at == 0 and farther == 0 and 0 < nearer < 1e-5
    assert not g["collision_grad"][0].any() and not g["collision_grad"][2].any() and g["collision_grad"][1].any()


def test_fixtures_regenerate_bit_for_bit(tmp_path):
    if not os.path.isdir("/root/reference"):
        pytest.skip("no /root/reference here: the edge fixtures are regenerated in the container that has it")
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_goldens_edges.py"), "--out", str(tmp_path)], cwd=ROOT,
                          stdout=subprocess.DEVNULL)
    for name in ("g_edges_sphere.npz", "g_edges_d2m.npz"):
        old, new = golden(name), np.load(os.path.join(str(tmp_path), name))
        assert sorted(old.files) == sorted(new.files)
        for k in old.files:
            a, b = old[k], new[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert a.tobytes() == b.tobytes(), "%s: %s differs" % (name, k)
