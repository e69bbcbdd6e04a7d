"""The fixed-point gradient sums of the mesh backwards (spherehand_amd/csrc/fixed_point.h) at the edges of their design,
on the GPU: the per-accumulator error bound of tests/fixed_point_ref.py across 24 binades of upstream gradient and on
ill-conditioned faces, power-of-two equivariance bit for bit, the same bits from the LDS and the global staging on either
side of 2048 points, fewer than 41 bits on an image of more than 699 050 pixels, non-finite upstream gradients that stay
at their own faces, and a huge finite term that coarsens only its own crop.

Entries: shr_tri_raster_bwd, shr_tri_raster_indexed_bwd, shr_mesh_depth_bwd, shr_tri_interp_bwd (vertex and attribute
parts), shr_tri_antialias_maps_bwd (vertex and value parts).  Every bound test prints its worst err / bound; DESIGN.md
4.4c keeps the numbers."""
import numpy as np
import pytest
import torch

import fixed_point_ref as fx
import tri_aa_maps_ref
import tri_aa_ref
import tri_grad_ref
import tri_interp_ref
from conftest import bits, golden
from tri_normals_ref import QUIRKS, random_mesh

pytestmark = pytest.mark.gpu

NAN_QUIRK = 4                                        # QUIRKS[4] has the NaN corner: the one face no bound test takes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pow2(shape, seed, lo=-12, hi=12):
    """+- 2^U(lo, hi)"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(lo, hi, shape))).astype(np.float32)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).numpy()


def _mesh(B, W, H, seed, quirks):
    """tests/tri_normals_ref.py's random mesh (981 vertices: a folded grid and 300 free triangles); quirks: with the
    finite QUIRKS faces -- slivers, off-image, zero-depth, back-facing, 1e9 corners -- and without the NaN corner's."""
    v, faces = random_mesh(B, W, H, seed, quirks=quirks)
    if quirks:
        assert np.isnan(v[:, faces[len(faces) - len(QUIRKS) + NAN_QUIRK]]).any()
        faces = np.ascontiguousarray(np.delete(faces, len(faces) - len(QUIRKS) + NAN_QUIRK, 0))
        ref = v[:, faces.astype(np.int64).ravel(), :3]
        assert np.isfinite(ref).all() and np.abs(ref).max() == 1e9
    return v, faces


def _soup_of(v, faces):
    return np.ascontiguousarray(v[:, faces.astype(np.int64), :3])


def _close(got, want, rtol=1e-6, atol=1e-5):
    """tests/test_tri_grad_gpu.py's criterion"""
    err = np.abs(got - want) - (atol + rtol * np.abs(want))
    assert err.max() <= 0, (float(np.abs(got - want).max()), float(np.abs(want).max()))


def _same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the entries: (numpy in, numpy out) --------------------------------------------------------------------------------
def _owners(v, faces, W, H):
    from spherehand_amd import ops
    depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, dev(v), dev(faces))
    return depth, owner


def _indexed_bwd(v, faces, owner, g):
    from spherehand_amd import ops
    out = ops.tri_raster_indexed_bwd(dev(v), dev(faces), owner, dev(g)).cpu().numpy()
    assert np.all(out[..., 3] == 0)
    return out[..., :3]


def _soup_bwd(fv, owner, g):
    from spherehand_amd import ops
    return ops.tri_raster_bwd(dev(fv), owner, dev(g)).cpu().numpy().reshape(fv.shape[0], -1, 3)


def _interp_bwd(a, v, faces, owner, go):
    from spherehand_amd import ops
    ga, gv = ops.tri_interpolate_bwd(dev(a), owner, dev(v), dev(faces), dev(go))
    gv = gv.cpu().numpy()
    assert np.all(gv[..., 2:] == 0)
    return ga.cpu().numpy(), gv[..., :2]


def _mesh_owner(v, faces, S):
    from spherehand_amd import ops
    return ops.mesh_depth_owner_fwd(dev(v), dev(faces), S)[1]


def _mesh_bwd(v, faces, owner4, g):
    from spherehand_amd import ops
    out = ops.mesh_depth_bwd(dev(v), dev(faces), owner4, dev(g)).cpu().numpy()
    assert np.all(out[..., 3] == 0)
    return out[..., :3]


def _hands():
    """The hand as DepthRender has it: (its 1 721 distinct projected vertices [2,NU,4] -- LDS accumulators --, faces) and
    (g2_mesh.npz's 10 144 vertices -- global accumulators --, faces)."""
    from spherehand_amd import hand_model
    from spherehand_amd.render import DepthRender
    g = golden("g2_mesh.npz")
    r = DepthRender(hand_model.load_mesh(), 64).cuda()
    with torch.no_grad():
        verts = r.lbs(torch.from_numpy(g["T"][:2]).cuda(), r.camera, None).contiguous()
    return ((verts.cpu().numpy(), r.rasterizer.faces_i32.cpu().numpy()),
            (np.ascontiguousarray(g["verts"][:2]), g["faces_swapped"].astype(np.int32)))


# ---- the error bound across binades ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,seed", [(97, 61, 1), (128, 96, 0)])
def test_error_bound_across_binades(W, H, seed):
    """grad_out = +- 2^U(-12, 12) per pixel on the random mesh with the finite QUIRKS (the 1e9 corners' terms are some
    fifteen binades from the grid's): every accumulator within n_p M 2^(2 - bits) + 2^-23 |ref_p|."""
    from spherehand_amd import ops
    B = 2
    v, faces = _mesh(B, W, H, seed, quirks=True)
    _, owner = _owners(v, faces, W, H)
    own = owner.cpu().numpy()
    assert (own >= 0).sum() > 1000 and fx.term_bits(3, W, H) == 41
    g = _pow2((B, H, W), seed + 10)
    t, _ = fx.raster_terms(v, faces, own, g)
    assert np.log2(t.largest().max() / np.abs(t.value[t.value != 0]).min()) > 24          # the terms do span binades
    fx.check_bound(_indexed_bwd(v, faces, owner, g), t, 41, "tri_raster_indexed_bwd %dx%d" % (W, H))
    fv = _soup_of(v, faces)
    _, owner_s = ops.tri_raster_owner_fwd(W, H, dev(fv))
    assert torch.equal(owner_s, owner)
    ts, _ = fx.raster_terms(*tri_grad_ref.soup_as_indexed(fv), own, g)
    fx.check_bound(_soup_bwd(fv, owner, g), ts, 41, "tri_raster_bwd %dx%d" % (W, H))
    for C in (3, 17):
        a = _randn((B, v.shape[1], C), C + seed)
        go = _pow2((B, C, H, W), seed + 20 + C)
        tv, ta, _ = fx.interp_terms(a, own, v, faces, go)
        ga, gv = _interp_bwd(a, v, faces, owner, go)
        fx.check_bound(gv, tv, 41, "tri_interpolate_bwd vertices C=%d %dx%d" % (C, W, H))
        fx.check_bound(ga, ta, 41, "tri_interpolate_bwd attributes C=%d %dx%d" % (C, W, H))


def test_error_bound_across_binades_mesh_depth():
    """shr_mesh_depth_bwd at S = 64 from 640 x 640 on the hand (depths of both signs: faces that straddle z = 0 have
    terms many binades above the palm's), LDS and global accumulators."""
    S = 64
    for k, (v, faces) in enumerate(_hands()):
        owner4 = _mesh_owner(v, faces, S)
        g = _pow2((2, S, S), 30 + k)
        t, _ = fx.mesh_terms(v, faces, owner4.cpu().numpy(), g)
        assert len(t.value) > 9 * 2000 and fx.term_bits(12, S, S) == 41
        fx.check_bound(_mesh_bwd(v, faces, owner4, g), t, 41, "mesh_depth_bwd S=64 NV=%d" % v.shape[1])


# ---- power-of-two equivariance -----------------------------------------------------------------------------------------
def test_power_of_two_equivariance_bit_for_bit():
    """bwd(2^k g) has exactly the bits of 2^k bwd(g): the maximum, the unit, the integers and the conversion all scale
    exactly while nothing leaves the normal fp32 range -- any absolute constant in the unit or the passes breaks it."""
    from spherehand_amd import ops
    W, H, B, S = 97, 61, 2, 64
    v, faces = _mesh(B, W, H, 3, quirks=False)
    x, fc = dev(v), dev(faces)
    depth, owner = _owners(v, faces, W, H)
    fv = dev(_soup_of(v, faces))
    hv, hf = _hands()[0]
    hx, hfc = dev(hv), dev(hf)
    owner4 = _mesh_owner(hv, hf, S)
    attrs = {C: dev(_randn((B, v.shape[1], C), C)) for C in (3, 17)}
    ec = dev(ops.tri_edge_table(faces))
    vals = ops.tri_interpolate(attrs[3], owner, x, fc)
    g2, g3 = dev(_randn((B, H, W), 1)), dev(_randn((2, S, S), 2))
    gc = {C: dev(_randn((B, C, H, W), 3 + C)) for C in (3, 17)}

    def run(s):
        out = {"tri_raster_bwd": ops.tri_raster_bwd(fv, owner, g2 * s),
               "tri_raster_indexed_bwd": ops.tri_raster_indexed_bwd(x, fc, owner, g2 * s),
               "mesh_depth_bwd": ops.mesh_depth_bwd(hx, hfc, owner4, g3 * s)}
        for C in (3, 17):
            out["interp attr C=%d" % C], out["interp vertices C=%d" % C] = ops.tri_interpolate_bwd(attrs[C], owner, x, fc, gc[C] * s)
        out["aa_maps values"], out["aa_maps vertices"] = ops.tri_antialias_maps_bwd(vals, depth, owner, x, fc, ec, gc[3] * s)
        return {k: t.double().cpu().numpy() for k, t in out.items()}

    base = run(1.0)
    assert len(base) == 9
    for name, a in base.items():
        nz = np.abs(a[a != 0])
        assert len(nz) > 100 and nz.min() > 2.0 ** -60 and nz.max() < 2.0 ** 60, (name, len(nz))   # normal at every k
    for k in (-60, -13, 7, 60):
        got = run(2.0 ** k)
        for name, a in base.items():
            want = a * 2.0 ** k                                         # (fp64: exact)
            assert np.array_equal(got[name], want), (name, k, int((got[name] != want).sum()),
                                                     float(np.abs(got[name] - want).max() / 2.0 ** k))


# ---- LDS and global staging --------------------------------------------------------------------------------------------
PAD_NV = (2047, 2048, 2049, 4096)


def _padded(v, NV, seed):
    """v [B,n,4] + unreferenced vertices up to NV (finite, on the image: nothing marks them as padding)"""
    B, n = v.shape[:2]
    rng = np.random.default_rng(seed)
    pad = np.concatenate([rng.uniform(0, 60, (B, NV - n, 3)), np.ones((B, NV - n, 1))], -1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([v, pad], 1))


def test_lds_and_global_staging_give_the_same_bits_indexed():
    """One mesh of 981 referenced vertices padded to 2047, 2048 (LDS accumulators), 2049 and 4096 (global accumulators,
    runs of eight pixels): integer sums have no order, so the referenced vertices' gradients have the same bits, and the
    padding's are exactly zero."""
    from spherehand_amd import ops
    W, H, B, C, S = 128, 96, 2, 5, 64
    v, faces = _mesh(B, W, H, 6, quirks=False)
    n = v.shape[1]
    vm, faces_m = _mesh(B, 640, 640, 7, quirks=False)                    # the resampled depth takes a 640 x 640 raster
    a = _randn((B, n, C), 1)
    g, go, gm = _randn((B, H, W), 2), _randn((B, C, H, W), 3), _randn((B, S, S), 4)
    edges = ops.tri_edge_table(faces)
    res = {}
    for NV in PAD_NV:
        vp, vmp = _padded(v, NV, NV), _padded(vm, NV, NV + 1)
        ap = np.ascontiguousarray(np.concatenate([a, _randn((B, NV - n, C), NV)], 1))
        depth, owner = _owners(vp, faces, W, H)
        owner4 = _mesh_owner(vmp, faces_m, S)
        ga, gv = _interp_bwd(ap, vp, faces, owner, go)
        vals = ops.tri_interpolate(dev(ap), owner, dev(vp), dev(faces))
        gvals, gaa = ops.tri_antialias_maps_bwd(vals, depth, owner, dev(vp), dev(faces), dev(edges), dev(go))
        res[NV] = dict(owner=owner.cpu().numpy(), owner4=owner4.cpu().numpy(), depth=depth.cpu(), vals=vals.cpu(),
                       indexed=_indexed_bwd(vp, faces, owner, g), mesh=_mesh_bwd(vmp, faces_m, owner4, gm), attr=ga, vert=gv,
                       aa=gaa.cpu().numpy(), aa_values=gvals.cpu().numpy())
    first = res[PAD_NV[0]]
    for NV in PAD_NV:
        r = res[NV]
        assert np.array_equal(r["owner"], first["owner"]) and np.array_equal(r["owner4"], first["owner4"])
        assert _same_bits(r["aa_values"], first["aa_values"])
        for name in ("indexed", "mesh", "attr", "vert", "aa"):
            assert np.abs(r[name][:, :n]).max() > 0, (name, NV)
            assert _same_bits(r[name][:, :n], first[name][:, :n]), (name, NV, int((bits(r[name][:, :n]) != bits(first[name][:, :n])).sum()))
            assert np.all(r[name][:, n:] == 0), (name, NV)
    # the 2048-point result against the fp64 restatements
    NV = 2048
    r = res[NV]
    vp, vmp = _padded(v, NV, NV), _padded(vm, NV, NV + 1)
    ap = np.ascontiguousarray(np.concatenate([a, _randn((B, NV - n, C), NV)], 1))
    _close(r["indexed"], tri_grad_ref.vertex_grad(torch.from_numpy(vp), faces, torch.from_numpy(r["owner"]), torch.from_numpy(g))[..., :3])
    _, want_m = fx.mesh_terms(vmp, faces_m, r["owner4"], gm)
    _close(r["mesh"], want_m)
    wa, wv = tri_interp_ref.grads(ap, r["owner"], vp, faces, go)
    _close(r["attr"], wa)
    _close(r["vert"], wv[..., :2])
    # the antialias pass by its own test's rule (tests/test_tri_aa_maps_gpu.py): vertices of faces that own an ambiguous
    # pixel are left out, max err <= 2e-3 max |want|
    _, info = tri_aa_ref.antialias(r["vals"][:, 0], r["depth"], torch.from_numpy(r["owner"]), vp, faces, edges)
    _, wv = tri_aa_maps_ref.grads(r["vals"], r["depth"], torch.from_numpy(r["owner"]), vp, faces, edges, torch.from_numpy(go))
    skip = np.zeros(vp.shape[:2], bool)
    if info["ambiguous"].any():
        amb = np.unique(r["owner"][info["ambiguous"]])
        skip[:, np.unique(faces[amb[amb >= 0]])] = True
    scale = np.abs(wv).max()
    assert scale > 0 and np.abs(r["aa"][..., :2] - wv[..., :2])[~skip].max() <= 2e-3 * scale


def test_lds_and_global_staging_give_the_same_bits_soup():
    """3 F = 2046 corners (LDS) against 2049 (global, runs): one more face, off the image, and the first 682 faces'
    gradients keep their bits."""
    W, H, B = 128, 96, 2
    fv = tri_grad_ref.random_soup(B, 682, W, H, 8)
    fv[..., 2] = np.abs(fv[..., 2]) + 20.0
    off = np.broadcast_to(np.float32([[-50, -50, 30], [-40, -50, 30], [-50, -40, 30]]), (B, 1, 3, 3))
    fv2 = np.ascontiguousarray(np.concatenate([fv, off], 1))
    from spherehand_amd import ops
    g = _randn((B, H, W), 5)
    _, o1 = ops.tri_raster_owner_fwd(W, H, dev(fv))
    _, o2 = ops.tri_raster_owner_fwd(W, H, dev(fv2))
    assert torch.equal(o1, o2) and (o1 >= 0).sum().item() > 5000
    g1, g2 = _soup_bwd(fv, o1, g), _soup_bwd(fv2, o2, g)
    assert g1.shape[1] == 2046 and g2.shape[1] == 2049 and np.abs(g1).max() > 0
    assert _same_bits(g1, g2[:, :2046]) and np.all(g2[:, 2046:] == 0)
    sv, sf = tri_grad_ref.soup_as_indexed(fv2)
    _close(g2, tri_grad_ref.vertex_grad(torch.from_numpy(sv), sf, o2.cpu(), torch.from_numpy(g)))


# ---- fewer than 41 bits ------------------------------------------------------------------------------------------------
def test_fewer_than_41_bits_on_a_large_image():
    """1024 x 700: 3 W H > 2^21, so fix_term_bits gives 40.  One front-facing face covers the whole image -- every pixel
    sends to its three corners' accumulators -- behind 50 random faces; with grad_out = 1 its z terms all have one sign,
    the case in which a sum of 41-bit terms would come closest to wrapping."""
    from spherehand_amd import ops
    W, H, B = 1024, 700, 1
    assert fx.term_bits(3, W, H) == 40 and fx.term_bits(3, 640, 640) == 41
    front = tri_grad_ref.random_soup(B, 50, W, H, 9)
    front[..., 2] = np.abs(front[..., 2]) * 0.8 + 20.0                    # 20 .. 60
    big = np.float32([[[-50, -50, 70], [2400, -50, 90], [-50, 1600, 80]]])
    fv = np.ascontiguousarray(np.concatenate([front, np.broadcast_to(big, (B, 1, 3, 3))], 1))
    sv, sf = tri_grad_ref.soup_as_indexed(fv)
    v4 = np.ascontiguousarray(np.concatenate([sv, np.ones(sv.shape[:2] + (1,), np.float32)], -1))
    fi = sf.astype(np.int32)
    _, owner = ops.tri_raster_owner_fwd(W, H, dev(fv))
    _, owner_i = _owners(v4, fi, W, H)
    own = owner.cpu().numpy()
    assert torch.equal(owner, owner_i) and (own >= 0).all() and (own == 50).sum() > 0.9 * W * H
    a = _randn((B, v4.shape[1], 3), 1)
    for name, g in (("ones", np.ones((B, H, W), np.float32)), ("normal", _randn((B, H, W), 2))):
        t, _ = fx.raster_terms(sv, sf, own, g)
        assert t.counts().max() > 0.9 * W * H
        fx.check_bound(_soup_bwd(fv, owner, g), t, 40, "tri_raster_bwd 1024x700 %s" % name)
        fx.check_bound(_indexed_bwd(v4, fi, owner, g), t, 40, "tri_raster_indexed_bwd 1024x700 %s" % name)
        go = np.ascontiguousarray(np.broadcast_to(g[:, None], (B, 3, H, W))) if name == "ones" else _randn((B, 3, H, W), 3)
        tv, ta, _ = fx.interp_terms(a, own, v4, fi, go)
        ga, gv = _interp_bwd(a, v4, fi, owner, go)
        fx.check_bound(gv, tv, 40, "tri_interpolate_bwd vertices 1024x700 %s" % name)
        fx.check_bound(ga, ta, 40, "tri_interpolate_bwd attributes 1024x700 %s" % name)


# ---- non-finite and huge upstream gradients ----------------------------------------------------------------------------
def _two_owned_pixels(own):
    """two owned pixels of crop 0 with different owner faces: (y, x, face) twice"""
    y, x = np.nonzero(own[0] >= 0)
    i = 0
    other = np.nonzero(own[0, y, x] != own[0, y[0], x[0]])[0]
    j = int(other[len(other) // 2])
    return (y[i], x[i], own[0, y[i], x[i]]), (y[j], x[j], own[0, y[j], x[j]])


def _untouched(B, NP, crop0_points):
    keep = np.ones((B, NP), bool)
    keep[0, np.asarray(crop0_points, np.int64).ravel()] = False
    return keep


def test_non_finite_upstream_gradients_stay_at_their_faces():
    """A NaN at one owned pixel and +inf at another (faces f1, f2 of crop 0): the maximum pass leaves them out, the sums
    drop the NaN terms and clamp the infinite ones -- every output is finite, and every point that is not a corner of f1 or
    f2 has exactly the bits of the run with those two gradients set to 0."""
    W, H, B, C, S = 97, 61, 2, 4, 64
    v, faces = _mesh(B, W, H, 11, quirks=False)
    f64 = faces.astype(np.int64)
    _, owner = _owners(v, faces, W, H)
    (y1, x1, f1), (y2, x2, f2) = _two_owned_pixels(owner.cpu().numpy())
    assert f1 != f2
    g = _randn((B, H, W), 1)
    bad, zero = g.copy(), g.copy()
    bad[0, y1, x1], bad[0, y2, x2] = np.nan, np.inf
    zero[0, y1, x1] = zero[0, y2, x2] = 0.0
    keep = _untouched(B, v.shape[1], f64[[f1, f2]])

    def compare(got, want, keep, what):
        assert np.isfinite(got).all(), what
        assert np.abs(want[keep]).max() > 0 and _same_bits(got[keep], want[keep]), (what, int((bits(got[keep]) != bits(want[keep])).sum()))

    compare(_indexed_bwd(v, faces, owner, bad), _indexed_bwd(v, faces, owner, zero), keep, "tri_raster_indexed_bwd")
    fv = _soup_of(v, faces)
    keep_s = _untouched(B, 3 * len(faces), [[3 * f1, 3 * f1 + 1, 3 * f1 + 2], [3 * f2, 3 * f2 + 1, 3 * f2 + 2]])
    compare(_soup_bwd(fv, owner, bad), _soup_bwd(fv, owner, zero), keep_s, "tri_raster_bwd")
    # the interpolation: every channel of the two pixels (the attribute part's maximum pass sees the same gradients in
    # both runs)
    a = _randn((B, v.shape[1], C), 2)
    go = _randn((B, C, H, W), 3)
    gbad, gzero = go.copy(), go.copy()
    gbad[0, :, y1, x1], gbad[0, :, y2, x2] = np.nan, np.inf
    gzero[0, :, y1, x1] = gzero[0, :, y2, x2] = 0.0
    (ga, gv), (za, zv) = _interp_bwd(a, v, faces, owner, gbad), _interp_bwd(a, v, faces, owner, gzero)
    compare(gv, zv, keep, "tri_interpolate_bwd vertices")
    compare(ga, za, keep, "tri_interpolate_bwd attributes")
    # the resampled depth: an output pixel's four taps may have four owners
    hv, hf = _hands()[0]
    owner4 = _mesh_owner(hv, hf, S)
    o4 = owner4.cpu().numpy()
    ys, xs = np.nonzero((o4[0] >= 0).any(-1))
    pa, pb = (ys[0], xs[0]), (ys[len(ys) // 2], xs[len(ys) // 2])
    gm = _randn((2, S, S), 4)
    mbad, mzero = gm.copy(), gm.copy()
    mbad[0][pa], mbad[0][pb] = np.nan, np.inf
    mzero[0][pa] = mzero[0][pb] = 0.0
    fs = np.concatenate([o4[0][pa], o4[0][pb]])
    keep_m = _untouched(2, hv.shape[1], hf.astype(np.int64)[fs[fs >= 0]])
    compare(_mesh_bwd(hv, hf, owner4, mbad), _mesh_bwd(hv, hf, owner4, mzero), keep_m, "mesh_depth_bwd")


def test_a_huge_finite_term_coarsens_only_its_own_crop():
    """One pixel of crop 0 at grad = 2^80: crop 0's unit follows it and crop 0 still meets the bound with its own M;
    crop 1's gradient has the bits of crop 1 alone."""
    W, H, B, C = 97, 61, 2, 3
    v, faces = _mesh(B, W, H, 12, quirks=False)
    _, owner = _owners(v, faces, W, H)
    own = owner.cpu().numpy()
    (y1, x1, _), _ = _two_owned_pixels(own)
    g = _randn((B, H, W), 1)
    g[0, y1, x1] = np.float32(2.0 ** 80)
    t, _ = fx.raster_terms(v, faces, own, g)
    M = t.largest()
    assert M[0] > 2.0 ** 40 * M[1] > 0
    v1, o1 = np.ascontiguousarray(v[1:]), owner[1:].contiguous()
    got = _indexed_bwd(v, faces, owner, g)
    assert _same_bits(got[1], _indexed_bwd(v1, faces, o1, g[1:])[0]) and np.abs(got[1]).max() > 0
    fx.check_bound(got, t, 41, "tri_raster_indexed_bwd, one pixel of crop 0 at 2^80")
    fv = _soup_of(v, faces)
    got = _soup_bwd(fv, owner, g)
    assert _same_bits(got[1], _soup_bwd(fv[1:], o1, g[1:])[0])
    fx.check_bound(got, fx.raster_terms(*tri_grad_ref.soup_as_indexed(fv), own, g)[0], 41, "tri_raster_bwd, one pixel at 2^80")
    a = _randn((B, v.shape[1], C), 2)
    go = _randn((B, C, H, W), 3)
    go[0, 1, y1, x1] = np.float32(2.0 ** 80)
    tv, ta, _ = fx.interp_terms(a, own, v, faces, go)
    ga, gv = _interp_bwd(a, v, faces, owner, go)
    ga1, gv1 = _interp_bwd(np.ascontiguousarray(a[1:]), v1, faces, o1, go[1:])
    assert _same_bits(ga[1], ga1[0]) and _same_bits(gv[1], gv1[0])
    fx.check_bound(gv, tv, 41, "tri_interpolate_bwd vertices, one pixel at 2^80")
    fx.check_bound(ga, ta, 41, "tri_interpolate_bwd attributes, one pixel at 2^80")
