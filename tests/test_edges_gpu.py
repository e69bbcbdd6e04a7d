"""GPU: the HIP kernels against the EDGE fixtures directly (tests/golden/g_edges_sphere.npz, g_edges_d2m.npz: the running
reference on exact ties, a hit at exactly 100.0, the 0.01 clamp, the 99 threshold, the clamp at 50, non-finite records;
tests/golden/make_goldens_edges.py).  Bars: depth bits and owners as tests/test_edges_cpu.py; sphere gradients at the
bar the GPU tests hold against the oracle, 1e-5 * max|ref| + 1e-4; the fused kernel at the fuzzer's, 1e-5 * max + 1e-3
(sse) and 2e-5 * max + 1e-3 (gradient); data -> model at 1e-5 relative (loss) and 1e-5 * max|ref| + 1e-9 (gradient).
An exact zero of the reference stays an exact zero; a NaN entry of the reference is not compared.

All scenes of one image size (and sphere count) are one batch per launch; the scenes that change a crop's path -- a
non-finite record, a record that is not tame, every sphere behind the background -- are also launched alone and must
give the bits they give inside the batch."""
import contextlib

import numpy as np
import pytest

from conftest import bits, golden
from test_edges_cpu import check_depth, check_gradient

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# What each forced path relies on in the launcher (csrc/sphere_raster.hip); test_forced_paths_are_what_they_say checks the
# arithmetic below against the fixtures' sizes, so a launcher change that turns a setting into a no-op has one place to fail.
#   general  shr_sphere_raster_fwd_ex: force_general makes `rows` 0 -> sphere_tile_fwd_kernel; shr_sphere_raster_bwd:
#            `argmin && !force_general` is false -> sphere_tile_bwd_kernel with or without an owner map.
#   box      launch_zbuf_fwd_t: lds = kHdrBytes + fwd_zbuf_bytes, raised to `least` = 8 rows; `box = lds < full` with
#            full = H rows: true for every fixture image (H = 10, 12, 16, 32 > 8).
#   fused    sphere_raster_mse_launch: `box = mse_box && box_fits` for mse_box >= 0, box_fits = W, H powers of two and
#            W >= 32: only the 32 x 32 group reaches sphere_zbuf_mse_box_kernel (mse_box = 1: half the LDS; a byte
#            value: that many bytes); every other group runs sphere_zbuf_mse_kernel whatever the setting.
SPHERE_PATHS = {"launcher": {}, "general": {"TUNE_FORCE_GENERAL": 1}, "box": {"TUNE_FWD_ZBUF_BYTES": 1}}
BOX_FORWARD_LEAST_ROWS = 8
MSE_BOX_SETTINGS = [-1, 0, 1, 20 * 1024]     # the launcher's choice, never, the box kernel at half the LDS, ... at 20 KB


def mse_box_fits(H, W):
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    return pow2(H) and pow2(W) and W >= 32


DEFAULTS = {"TUNE_FORCE_GENERAL": 0, "TUNE_FWD_ZBUF_BYTES": 0, "TUNE_MSE_BOX": -1, "TUNE_D2M_WAVES": 0, "TUNE_D2M_BAND_UNITS": 0}
ALONE_TOO = ("huge_x_r", "all_behind_covering", "all_behind_partial")     # ... and every scene with a non-finite record


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@contextlib.contextmanager
def tuning(**kw):
    from spherehand_amd import ops
    try:
        for k, v in kw.items():
            ops.set_tuning(getattr(ops, k), v)
        yield ops
    finally:
        for k, v in DEFAULTS.items():
            ops.set_tuning(getattr(ops, k), v)


def sphere_groups():
    g = golden("g_edges_sphere.npz")
    return g, [(str(t), int(g[t + "_hw"][0]), int(g[t + "_hw"][1])) for t in g["groups"]]


def nan_q_rows(sp, depth, argmin):
    """[N,J,4] mask of the entries the kernels' arithmetic does not give: d/dx, d/dy, d/dr of a record with a NaN in x, y
    or r THAT OWNS A PIXEL (the fixture's argmin names it where the depth is not the background's 100.0).  The
    reference's clamp(min) passes no gradient for the NaN q of such a record (0, or 0 * NaN = NaN); the backwards and the
    fused kernel form g / sqrt(q) = NaN for every pixel it owns -- the recorded deviation of DESIGN.md section 3 (edge
    scenes), which tests/test_edges_cpu.py holds the oracle to.  Such a record's d/dz, a NaN record that owns nothing
    (its exact zeros) and every other record of the crop are compared."""
    fg = bits(depth) != bits(np.float32(100.0))
    m = np.zeros(sp.shape, bool)
    for i in range(sp.shape[0]):
        for j in range(sp.shape[1]):
            if np.isnan(sp[i, j, [0, 1, 3]]).any() and (fg[i] & (argmin[i] == j)).any():
                m[i, j, [0, 1, 3]] = True
    return m


def run_sphere(ops, sp, up, H, W):
    s, u = dev(sp), dev(up)
    d, a = ops.sphere_raster_fwd(s, H, W, want_argmin=True)
    out = {"depth": d.cpu().numpy(), "owner": a.cpu().numpy(), "depth_only": ops.sphere_raster_fwd(s, H, W).cpu().numpy(),
           "grad_owner_map": ops.sphere_raster_bwd(s, u, a).cpu().numpy(), "grad_recomputed": ops.sphere_raster_bwd(s, u).cpu().numpy()}
    return out


@pytest.mark.parametrize("path", list(SPHERE_PATHS))
def test_sphere_forward_and_backward(path):
    g, groups = sphere_groups()
    fails = []
    with tuning(**SPHERE_PATHS[path]) as ops:
        for tag, H, W in groups:
            sp, up, names = g[tag + "_spheres"], g[tag + "_upstream"], [str(n) for n in g[tag + "_names"]]
            out = run_sphere(ops, sp, up, H, W)
            waived = nan_q_rows(sp, g[tag + "_depth"], g[tag + "_argmin"])
            for i, n in enumerate(names):
                name = "%s %s/%s" % (path, tag, n)
                check_depth(name, out["depth"][i], out["owner"][i], g[tag + "_depth"][i], g[tag + "_argmin"][i], fails)
                if not np.array_equal(bits(out["depth_only"][i]), bits(out["depth"][i])):
                    fails.append("%s: the depth-only launch differs" % name)
                ref = np.where(waived[i], np.nan, g[tag + "_grad"][i])
                # (the owner-map backward is the tile kernel under TUNE_FORCE_GENERAL, a z-buffer kernel otherwise)
                check_gradient(name + " recomputed", out["grad_recomputed"][i], ref, 1e-5, 1e-4, fails)
                check_gradient(name + " owner map", out["grad_owner_map"][i], ref, 1e-5, 1e-4, fails)
            for i, n in enumerate(names):
                if np.isfinite(sp[i]).all() and n not in ALONE_TOO:
                    continue
                one = run_sphere(ops, sp[i:i + 1], up[i:i + 1], H, W)
                for k, v in one.items():
                    same = np.array_equal(v[0], out[k][i]) if k == "owner" else np.array_equal(bits(v[0]), bits(out[k][i]))
                    if not same:
                        fails.append("%s %s/%s: %s alone differs from the batch\n %s\n %s" % (path, tag, n, k, v[0], out[k][i]))
    assert not fails, "\n".join(fails)


def test_forced_paths_are_what_they_say():
    """The sizes the comments at SPHERE_PATHS rely on: every image has more rows than the box forward's least z-buffer,
    and exactly one group is an image the fused box kernel takes."""
    g, groups = sphere_groups()
    assert all(H > BOX_FORWARD_LEAST_ROWS for _, H, W in groups)
    assert [tag for tag, H, W in groups if mse_box_fits(H, W)] == ["c3"]
    names = {str(n) for n in g["c3_names"]}
    assert {"dup_front", "mirror_tie", "hit100_lower_misses", "hit100_lower_deeper", "hit100_twice", "all_behind_covering",
            "all_behind_partial", "nan_x", "nan_z", "nan_r", "nan_z_twice", "inf_r", "minus_inf_z", "huge_x_r"} <= names


@pytest.mark.parametrize("mse_box", MSE_BOX_SETTINGS)
def test_fused_render_and_compare(mse_box):
    """Groups the box variant takes (32 x 32) run it under mse_box = 1 and 20 KB; the others run the whole-region kernel
    under every setting (labelled so in a failure)."""
    g, groups = sphere_groups()
    fails, ran, boxed = [], 0, 0
    with tuning(TUNE_MSE_BOX=mse_box) as ops:
        for tag, H, W in groups:
            sp, tgt, names = g[tag + "_spheres"], g[tag + "_target"], [str(n) for n in g[tag + "_names"]]
            if not ops.sphere_raster_mse_supported(dev(sp), dev(tgt), H, W):
                continue
            ran += 1
            box = mse_box > 0 and mse_box_fits(H, W)
            boxed += box

            def run(lo, hi):
                dep, sse, grad = ops.sphere_raster_mse(dev(sp[lo:hi]), dev(tgt[lo:hi]))
                return dep.cpu().numpy(), sse.double().cpu().numpy(), grad.cpu().numpy()
            dep, sse, grad = run(0, len(sp))
            ref_sse = g[tag + "_sse"].astype(np.float64)
            waived = nan_q_rows(sp, g[tag + "_depth"], g[tag + "_argmin"])
            for i, n in enumerate(names):
                name = "fused(%s kernel, TUNE_MSE_BOX %d) %s/%s" % ("box" if box else "whole-region", mse_box, tag, n)
                check_depth(name, dep[i], None, g[tag + "_depth"][i], None, fails)
                if np.isfinite(ref_sse[i]):
                    if not abs(sse[i] - ref_sse[i]) <= 1e-5 * ref_sse[i] + 1e-3:
                        fails.append("%s: sse %r against %r" % (name, sse[i], ref_sse[i]))
                elif not (np.isnan(sse[i]) == np.isnan(ref_sse[i]) and (np.isnan(ref_sse[i]) or sse[i] == ref_sse[i])):
                    fails.append("%s: sse %r against %r" % (name, sse[i], ref_sse[i]))
                check_gradient(name, grad[i], np.where(waived[i], np.nan, g[tag + "_sse_grad"][i]), 2e-5, 1e-3, fails)
                if not np.isfinite(sp[i]).all() or n in ALONE_TOO:
                    d1, s1, g1 = run(i, i + 1)
                    if not (np.array_equal(bits(d1[0]), bits(dep[i])) and np.array_equal(bits(np.float32(s1[0])), bits(np.float32(sse[i])))
                            and np.array_equal(bits(g1[0]), bits(grad[i]))):
                        fails.append("%s: alone differs from the batch" % name)
    assert ran >= 4          # the 20-, 16- and 32-pixel rows; 14-pixel rows are not the fused kernel's
    assert boxed == (1 if mse_box > 0 else 0)
    assert not fails, "\n".join(fails)


def d2m_batches():
    """[(tag, H, W, scene indices, radii)]: the scenes of one image size that share their radii are one batch."""
    g = golden("g_edges_d2m.npz")
    out = []
    for tag in g["groups"]:
        H, W = (int(x) for x in g[tag + "_hw"])
        rad = g[tag + "_radii"]
        keys = sorted({r.tobytes() for r in rad})
        for key in keys:
            idx = [i for i in range(len(rad)) if rad[i].tobytes() == key]
            out.append((str(tag), H, W, idx, rad[idx[0]]))
    return g, out


def check_d2m(name, loss_sum, grad_sum, ref_loss, ref_grad, count, fails):
    """loss_sum / grad_sum: the kernel's per-crop sum and its unit gradient; the fixture holds the mean over the crop."""
    loss = float(loss_sum) / count
    if np.isnan(ref_loss) or np.isnan(loss):
        if not (np.isnan(ref_loss) and np.isnan(loss)):
            fails.append("%s: loss %r against %r" % (name, loss, float(ref_loss)))
    elif not abs(loss - ref_loss) <= 1e-5 * abs(ref_loss):
        fails.append("%s: loss %r against %r" % (name, loss, float(ref_loss)))
    if grad_sum is not None:
        with np.errstate(invalid="ignore"):
            check_gradient(name, grad_sum / np.float32(count), ref_grad, 1e-5, 1e-9, fails)


@pytest.mark.parametrize("waves,units", [(0, 0), (4, 1), (16, 8)])
def test_data_to_model_kernel(waves, units):
    g, batches = d2m_batches()
    fails = []
    with tuning(TUNE_D2M_WAVES=waves, TUNE_D2M_BAND_UNITS=units) as ops:
        for tag, H, W, idx, rad in batches:
            dep, cen = g[tag + "_depth"][idx], g[tag + "_centres"][idx]
            names = [str(g[tag + "_names"][i]) for i in idx]
            loss, grad = [t.cpu().numpy() for t in ops.data_to_model(dev(dep), dev(cen), dev(rad), want_grad=True)]
            loss_only = ops.data_to_model(dev(dep), dev(cen), dev(rad)).cpu().numpy()
            for k, i in enumerate(idx):
                name = "d2m(%d,%d) %s/%s" % (waves, units, tag, names[k])
                check_d2m(name, loss[k], grad[k], g[tag + "_loss"][i], g[tag + "_grad"][i], H * W, fails)
                if not np.array_equal(bits(loss_only[k]), bits(loss[k])):
                    fails.append("%s: the loss-only launch gives %r, with the gradient %r" % (name, loss_only[k], loss[k]))
                if not (np.isfinite(dep[k]).all() and np.isfinite(cen[k]).all()):
                    l1, g1 = [t.cpu().numpy() for t in ops.data_to_model(dev(dep[k:k + 1]), dev(cen[k:k + 1]), dev(rad), want_grad=True)]
                    if not (np.array_equal(bits(l1[0]), bits(loss[k])) and np.array_equal(bits(g1[0]), bits(grad[k]))):
                        fails.append("%s: alone differs from the batch" % name)
    assert not fails, "\n".join(fails)


def test_data_to_model_two_step_path():
    """d2m_compact + data_to_model_from_points, where the path takes the image (rows of four pixels)."""
    from spherehand_amd import ops
    g, batches = d2m_batches()
    fails, ran = [], 0
    for tag, H, W, idx, rad in batches:
        dep, cen = g[tag + "_depth"][idx], g[tag + "_centres"][idx]
        if not ops.d2m_points_supported(dev(dep)):
            continue
        ran += 1
        ws = ops.d2m_compact(dev(dep))
        loss, grad = [t.cpu().numpy() for t in ops.data_to_model_from_points(ws, len(idx), H, W, dev(cen), dev(rad), None, True)]
        loss_only = ops.data_to_model_from_points(ws, len(idx), H, W, dev(cen), dev(rad)).cpu().numpy()
        for k, i in enumerate(idx):
            name = "two-step %s/%s" % (tag, g[tag + "_names"][i])
            check_d2m(name, loss[k], grad[k], g[tag + "_loss"][i], g[tag + "_grad"][i], H * W, fails)
            if not np.array_equal(bits(loss_only[k]), bits(loss[k])):
                fails.append("%s: the loss-only launch gives %r, with the gradient %r" % (name, loss_only[k], loss[k]))
    assert ran >= 1
    assert not fails, "\n".join(fails)


def test_data_to_model_module_autograd():
    """DataToModelLoss through autograd, one scene per call as the fixture recorded it (its loss is the crop's mean)."""
    from spherehand_amd.render import DataToModelLoss
    g, _ = d2m_batches()
    fails = []
    for tag in g["groups"]:
        H, W = (int(x) for x in g[tag + "_hw"])
        crits = {}
        for i, n in enumerate(g[tag + "_names"]):
            rad = g[tag + "_radii"][i]
            if rad.tobytes() not in crits:
                crits[rad.tobytes()] = DataToModelLoss(W, H, [float(r) for r in rad]).cuda()
            joints = dev(g[tag + "_centres"][i:i + 1]).requires_grad_(True)
            loss = crits[rad.tobytes()](dev(g[tag + "_depth"][i:i + 1]), joints)
            (loss * 3.0).backward()
            check_d2m("module %s/%s" % (tag, n), loss.item(), joints.grad.cpu().numpy()[0] / np.float32(3.0),
                      g[tag + "_loss"][i], g[tag + "_grad"][i], 1, fails)
    assert not fails, "\n".join(fails)


def test_collision_hinge_on_its_kink():
    """Two spheres exactly 6.0 apart (the hinge argument is exactly 0), one ulp nearer, one ulp farther: the case
    tools/fuzz.py's pl_case waives.  At and beyond the kink the loss and every gradient entry are exact zeros."""
    from spherehand_amd import ops
    from spherehand_amd.render import BoneLengthLoss
    g = golden("g_edges_d2m.npz")
    bc = BoneLengthLoss().cuda()
    for i, n in enumerate(g["collision_names"]):
        j = dev(g["collision_joints"][i:i + 1]).requires_grad_(True)
        col, _ = ops.PairLosses.apply(j, 41, 11, 6, float(g["collision_min_sq_dist"]), bc.joint_1.to(torch.int32),
                                      bc.joint_2.to(torch.int32), bc.min_length.reshape(-1).clone(), bc.max_length.reshape(-1).clone())
        col.backward()
        ref, ref_grad = float(g["collision_loss"][i]), g["collision_grad"][i]
        grad = j.grad.cpu().numpy()[0]
        assert abs(col.item() - ref) <= 1e-5 * max(1.0, abs(ref)), n              # test_losses_gpu.py's bar for this kernel
        assert np.abs(grad - ref_grad).max() <= 1e-5 * max(1.0, np.abs(ref_grad).max()), n
        if ref == 0:
            assert col.item() == 0 and not grad.any(), n
        else:
            assert col.item() > 0 and np.array_equal(grad != 0, ref_grad != 0), n
