"""tests/fixed_point_ref.py without a GPU: the per-tap terms of the three fp64 restatements scatter to their autograd
gradients, the restated bit count, the numpy emulation of fixed_point.h's passes meets the bound the design states
(and misses it where the unit is made wrong on purpose), and the fuzzer's two gradient families draw cases whose
reference terms are finite."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import fixed_point_ref as fx
import mesh_grad_ref
import tri_grad_ref
import tri_interp_ref
from conftest import ROOT
from tri_normals_ref import random_mesh


def _pow2(shape, seed, lo=-12, hi=12):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(lo, hi, shape))).astype(np.float32)


@pytest.fixture(scope="module")
def scene(oracle):
    """A small random mesh (981 vertices, 428 faces, two crops at 33 x 25), its raster and owners on the CPU, and the
    owner taps of its 16 x 16 resampling from a 33 x 33 raster."""
    W, H, S, src = 33, 25, 16, 33
    v, faces = random_mesh(2, W, H, 4, quirks=False)
    fv = np.ascontiguousarray(v[:, faces.astype(np.int64), :3])
    depth = oracle.tri_raster_fwd(fv, W, H)
    owner = tri_interp_ref.cpu_owners(depth, v, faces)
    assert (owner >= 0).sum() > 500
    raw = oracle.tri_raster_fwd(fv, src, src)
    own_src = tri_interp_ref.cpu_owners(raw, v, faces)
    xs, ys, wt = mesh_grad_ref.tap_grid(S, src)
    own4 = own_src[:, ys, xs]                                            # [B,S,S,4]
    own4 = np.where((raw[:, ys, xs] <= 100.0) & (wt != 0)[None], own4, -1).astype(np.int32)
    assert (own4 >= 0).sum() > 500
    return dict(W=W, H=H, S=S, src=src, v=v, faces=faces, owner=owner, own4=own4)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_scattered_terms_are_the_autograd_gradient(scene):
    s = scene
    B, NV = s["v"].shape[:2]
    g = _pow2((B, s["H"], s["W"]), 0, -3, 3)
    t, grad = fx.raster_terms(s["v"], s["faces"], s["owner"], g)
    assert t.D == 3 and t.NP == NV and np.abs(grad).max() > 0 and t.all_finite()
    assert _rel(t.sums(), grad) <= 1e-12
    want = tri_grad_ref.vertex_grad(torch.from_numpy(s["v"]), s["faces"], torch.from_numpy(s["owner"]), torch.from_numpy(g))
    assert np.array_equal(want[..., :3], grad)                           # (the helper changes no bit of the restatement)
    # a soup: the same terms on the corners
    fv = np.ascontiguousarray(s["v"][:, s["faces"].astype(np.int64), :3])
    sv, sf = tri_grad_ref.soup_as_indexed(fv)
    ts, gs = fx.raster_terms(sv, sf, s["owner"], g)
    assert _rel(ts.sums(), gs) <= 1e-12 and np.array_equal(np.sort(np.abs(ts.value)), np.sort(np.abs(t.value)))

    gm = _pow2((B, s["S"], s["S"]), 1, -3, 3)
    t, grad = fx.mesh_terms(s["v"], s["faces"], s["own4"], gm, s["src"])
    assert np.abs(grad).max() > 0 and _rel(t.sums(), grad) <= 1e-12
    assert len(t.value) == 9 * (s["own4"] >= 0).sum()                    # one row of nine terms per owner tap

    for C, shared in ((3, False), (17, True)):
        rng = np.random.default_rng(C)
        a = rng.standard_normal((NV, C) if shared else (B, NV, C)).astype(np.float32)
        go = _pow2((B, C, s["H"], s["W"]), C, -3, 3)
        tv, ta, (ga, gv) = fx.interp_terms(a, s["owner"], s["v"], s["faces"], go)
        wa, wv = tri_interp_ref.grads(a, s["owner"], s["v"], s["faces"], go)
        assert np.array_equal(wa, ga) and np.array_equal(wv[..., :2], gv)
        assert tv.D == 2 and ta.D == C and np.abs(gv).max() > 0
        assert _rel(tv.sums(), gv) <= 1e-12
        assert _rel(ta.sums().sum(0) if shared else ta.sums(), ga) <= 1e-12
        # an attribute term is wh_k grad_out[ch]: weights in [0, 1], so no term is larger than the largest gradient
        assert ta.largest().max() <= np.abs(go).max()


def test_restated_bit_count():
    assert fx.term_bits(3, 640, 640) == 41 and fx.term_bits(3, 1024, 700) == 40
    assert fx.term_bits(3, 1024, 682) == 41 and fx.term_bits(3, 1024, 683) == 40     # 3 W H = 2^21 - 2^11, 2^21 + 2^10
    assert fx.term_bits(12, 320, 320) == 41 and fx.term_bits(12, 418, 418) == 41 and fx.term_bits(12, 419, 419) == 40
    assert fx.term_bits(12, 16383, 16383) == 62 - 32 and fx.term_bits(3, 65535, 65535) == 62 - 34
    assert fx.term_bits(2, 1, 1) == 41 and fx.term_bits(1, 1, 1) == 41


def test_emulated_passes_meet_the_bound_and_a_wrong_unit_does_not(scene):
    """The bound is the design's own: fixed_point.h's passes restated in numpy on the reference's terms stay inside it
    across 24 binades of upstream gradient, at 41 bits and at fewer; an absolute constant in the unit (the unit of terms
    of order 1 whatever the crop's largest term) does not."""
    s = scene
    B = s["v"].shape[0]
    g = _pow2((B, s["H"], s["W"]), 2)
    t, _ = fx.raster_terms(s["v"], s["faces"], s["owner"], g)
    for bits in (41, 40, 28):
        assert fx.check_bound(t.emulate(bits), t, bits, "emulated raster") <= 1.0
    g[0, :, :] *= np.float32(2.0 ** 80)                                  # crop 0 alone is coarsened
    t2, _ = fx.raster_terms(s["v"], s["faces"], s["owner"], g)
    got = t2.emulate(41)
    fx.check_bound(got, t2, 41, "emulated raster, crop 0 x 2^80")
    assert np.array_equal(got[1], t.emulate(41)[1])
    # an absolute unit -- that of a crop whose largest term is of order 1 -- on the same terms 30 binades down: even the
    # exact sums rounded once to that unit are far outside the bound
    small = fx.Terms(t.value * 2.0 ** -30, t.crop, t.acc, t.B, t.NP, t.D)
    fx.check_bound(small.emulate(41), small, 41, "emulated raster x 2^-30")
    wrong = (np.rint(small.sums() / 2.0 ** -41) * 2.0 ** -41).astype(np.float32)
    with pytest.raises(AssertionError):
        fx.check_bound(wrong, small, 41, "an absolute unit")
    # non-finite terms: dropped or clamped, and named by the check
    bad = fx.Terms(np.concatenate([t.value, [np.nan, np.inf]]), np.concatenate([t.crop, [0, 0]]),
                   np.concatenate([t.acc, [0, 1]]), t.B, t.NP, t.D)
    assert not bad.all_finite() and np.isfinite(bad.emulate(41)).all()
    with pytest.raises(AssertionError):
        fx.check_bound(bad.emulate(41), bad, 41, "non-finite terms")


@pytest.fixture(scope="module")
def fuzz():
    spec = importlib.util.spec_from_file_location("shr_fuzz_cpu", os.path.join(ROOT, "tools", "fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("family", ["trigrad", "interp"])
def test_fuzz_draws_have_finite_reference_terms(fuzz, oracle, family):
    """The generator alone, owners from the CPU restatement: fewer than 5 % of a family's draws may be skipped for a
    reference term that is not finite (tests/test_fuzz_gpu.py holds the GPU run to the same cap)."""
    fuzz.rs = np.random.RandomState(7)
    n, skipped = 12, 0
    for _ in range(n):
        case = fuzz.grad_case_draw(family == "interp")
        fv = np.ascontiguousarray(case["verts"][:, case["faces"].astype(np.int64), :3])
        owner = tri_interp_ref.cpu_owners(oracle.tri_raster_fwd(fv, case["W"], case["H"]), case["verts"], case["faces"])
        skipped += not all(t.all_finite() for t in fuzz.grad_case_terms(case, owner).values())
    print("%s: %d of %d CPU draws skipped" % (family, skipped, n))
    assert skipped <= 0.05 * n
