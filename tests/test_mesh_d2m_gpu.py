"""The mesh data-to-model distance on the GPU (ops.mesh_data_to_model, ops.mesh_data_to_model_bwd, ops.MeshDataToModel,
render.MeshDataToModelLoss) against the restatement of tests/mesh_d2m_ref.py, which measures every face for every point
(no cull): the forward's bits over partial waves, tiles and chunk seams, special inputs, inputs built against the cull,
the range checks with guard regions, the backward within the fixed-point sums' bound, determinism, batch independence,
autograd, graph capture, and the translation fit of tests/test_mesh_d2m_cpu.py through the module."""
import os

import numpy as np
import pytest
import torch

import fixed_point_ref as fpr
import mesh_d2m_ref as ref
from conftest import GOLDEN, ROOT, bits

pytestmark = pytest.mark.gpu

CHUNK = 256          # kD2mChunk (spherehand_amd/csrc/mesh_d2m.hip): test_chunk_constant pins it
F32 = np.float32
INF = float("inf")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_chunk_constant():
    import re
    code = open(os.path.join(ROOT, "spherehand_amd", "csrc", "mesh_d2m.hip")).read()
    assert int(re.search(r"constexpr int kD2mChunk = (\d+);", code).group(1)) == CHUNK


def soup(B, NV, F, H, W, seed, p2m=(1.0, 0.0, 1.0, 0.0), fg=0.6):
    """random vertices over the mapped image and z in [40, 60], random faces, an observation with about `fg` of its pixels
    data points at z in [35, 65]"""
    rs = np.random.RandomState(seed)
    ax, bx, ay, by = p2m
    v = np.ones((B, NV, 4), F32)
    v[..., 0] = rs.uniform(bx - 2, ax * W + bx + 2, (B, NV))
    v[..., 1] = rs.uniform(by - 2, ay * H + by + 2, (B, NV))
    v[..., 2] = rs.uniform(40, 60, (B, NV))
    faces = rs.randint(0, NV, (F, 3)).astype(np.int32)
    obs = rs.uniform(35, 65, (B, H, W)).astype(F32)
    obs[rs.rand(B, H, W) >= fg] = 1000.0
    return v, faces, obs


def run(obs, v, faces, p2m=(1.0, 0.0, 1.0, 0.0), fg_max=500.0, max_dist=INF):
    from spherehand_amd import ops
    d, f = ops.mesh_data_to_model(dev(obs), dev(v), dev(np.asarray(faces, np.int32).reshape(-1, 3)), p2m, fg_max, max_dist)
    torch.cuda.synchronize()
    return d.cpu().numpy(), f.cpu().numpy()


def same(obs, v, faces, p2m=(1.0, 0.0, 1.0, 0.0), fg_max=500.0, max_dist=INF, tag=""):
    """the GPU's maps equal the restatement's bit for bit -> (dist, face)"""
    want_d, want_f = ref.forward32(obs, v, faces, p2m, fg_max, max_dist)
    d, f = run(obs, v, faces, p2m, fg_max, max_dist)
    assert d.shape == want_d.shape and f.dtype == np.int32
    bad = (f != want_f) | (bits(d) != bits(want_d))
    assert not bad.any(), ("%s: %d pixels differ, first at %s: got (%r, %d) want (%r, %d)"
                           % (tag, bad.sum(), np.argwhere(bad)[0], d[bad][0], f[bad][0], want_d[bad][0], want_f[bad][0]))
    return d, f


def toy_case():
    """the toy mesh and its own depth at 33 x 33 from the triangle raster"""
    from spherehand_amd import ops
    rest, faces = ref.toy()
    obs = ops.tri_raster_indexed_fwd(33, 33, dev(rest), dev(faces)).cpu().numpy()
    return rest, faces, obs


# 1 x 1, 3 x 5: less than a wave; 9 x 67: 603 pixels, two rounds of the list, the second partial; 2 x 130: a row seam inside a wave;
# 33 x 33: 1089 pixels, two tiles
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (9, 67), (2, 130), (33, 33)])
def test_bits(H, W):
    if (H, W) == (33, 33):
        rest, faces, obs = toy_case()
        assert 300 < (obs < 99).sum() < 600
        for t in ((0, 0, 0), ref.FIT_SHIFT):
            d, f = same(obs, ref.moved(rest, t), faces, fg_max=ref.REF_FG_MAX, max_dist=50.0, tag="toy %s" % (t,))
        assert d.max() > 1 and len(np.unique(f)) > 6
        return
    p2m = (1.5, -2.0, 0.75, 1.0)
    v, faces, obs = soup(2, 40, 70, H, W, H * W, p2m, fg=0.8 if H * W > 1 else 1.0)
    d, f = same(obs, v, faces, p2m, tag="%d x %d" % (H, W))
    assert (f >= 0).sum() == (obs < 500).sum() > 0


@pytest.mark.parametrize("F", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_face_counts_cross_chunk_seams(F):
    v, faces, obs = soup(2, 90, F, 8, 8, 100 + F)
    if F > 1:                                                    # the face that wins most often goes last: past every seam
        won = ref.forward32(obs, v, faces, fg_max=500.0)[1]
        busiest = np.bincount(won[won >= 0], minlength=F).argmax()
        faces[[busiest, F - 1]] = faces[[F - 1, busiest]]
    d, f = same(obs, v, faces, tag="F = %d" % F)
    if F == 0:
        assert np.all(d == 0) and np.all(f == -1)
    if F > 1:
        assert (f == F - 1).any() and (f < min(F - 1, CHUNK)).any()


@pytest.mark.parametrize("kind", ["empty", "full", "single"])
def test_foreground(kind):
    v, faces, obs = soup(2, 30, 50, 9, 67, 5, fg=1.0)
    if kind == "empty":
        obs[:] = 1000.0
    elif kind == "single":
        keep = obs[1, 7, 66]
        obs[:] = np.nan
        obs[1, 7, 66] = keep                                    # (NaN: no data point)
    d, f = same(obs, v, faces, tag=kind)
    assert (f >= 0).sum() == {"empty": 0, "full": obs.size, "single": 1}[kind]


_HAND = {}


def hand_case():
    """all 3 382 faces of the hand at rest (tests/golden/g2_mesh.npz verts, 640 x 640 pixel space) under a 32 x 32
    observation mapped with ax = ay = 20: a pixel within 15 px of a vertex observes that vertex's z + [-6, 6]"""
    if not _HAND:
        v = np.load(os.path.join(GOLDEN, "g2_mesh.npz"))["verts"][:2].astype(F32)
        faces = np.load(os.path.join(ROOT, "spherehand_amd", "data", "hand_model.npz"))["faces"].astype(np.int32)
        rs = np.random.RandomState(11)
        obs = np.full((2, 32, 32), 1000.0, F32)
        gy, gx = np.meshgrid(np.arange(32) * 20.0, np.arange(32) * 20.0, indexing="ij")
        for b in range(2):
            d2 = (gx[..., None] - v[b, ::7, 0]) ** 2 + (gy[..., None] - v[b, ::7, 1]) ** 2
            near = d2.argmin(-1)
            hit = d2.min(-1) < 15.0 ** 2
            obs[b][hit] = (v[b, ::7, 2][near] + rs.uniform(-6, 6, near.shape))[hit]
        p2m = (20.0, 0.0, 20.0, 0.0)
        _HAND.update(v=v, faces=faces, obs=obs, p2m=p2m, want=ref.forward32(obs, v, faces, p2m, 500.0, INF))
    return _HAND


def test_the_hand():
    c = hand_case()
    assert (c["obs"] < 500).sum() > 60
    d, f = run(c["obs"], c["v"], c["faces"], c["p2m"])
    assert np.array_equal(f, c["want"][1]) and np.array_equal(bits(d), bits(c["want"][0]))
    assert len(np.unique(f)) > 40 and f.max() > 3000


def test_special_inputs():
    # one good face in the plane z = 50, a second one sharing its edge (16, 0)-(16, 16), then zero-area faces
    v = np.array([[[0, 0, 50, 1], [16, 0, 50, 1], [16, 16, 50, 1], [32, 0, 50, 1], [32, 16, 50, 1],
                   [3, 3, 40, 1], [5, 5, 40, 1], [7, 7, 40, 1], [np.nan, 2, 45, 1]]], F32)
    faces = np.array([[0, 1, 2], [1, 3, 2],          # two faces sharing the edge 1-2
                      [5, 6, 7], [5, 5, 5], [6, 7, 7],   # collinear, a point, two coincident corners
                      [0, 8, 2]], np.int32)             # a NaN vertex
    obs = np.full((1, 12, 24), 1000.0, F32)
    obs[0, 4, 8] = 50.0             # on face 0 (weights 1/2, 1/4, 1/4: exact): dist 0
    obs[0, 8, 16] = 47.0            # straight above the shared edge: faces 0 and 1 tie, the smaller index wins
    obs[0, 5, 5] = 41.0             # next to the zero-area faces (1 from the segment, 9 from the plane)
    obs[0, 3, 3] = 40.0             # on the degenerate faces' corner
    obs[0, 11, 23] = -np.inf        # a data point under a finite fg_max whose every distance is a NaN: 0 and -1
    obs[0, 0, 0] = np.nan           # no data point
    for max_dist in (0.0, 2.0, INF):
        d, f = same(obs, v, faces, max_dist=max_dist, tag="special, max_dist %r" % max_dist)
        assert d[0, 4, 8] == 0 and f[0, 4, 8] == 0
        assert f[0, 8, 16] == 0 and d[0, 8, 16] == min(3.0, max_dist)
        assert f[0, 5, 5] == 2 and d[0, 5, 5] == min(1.0, max_dist)
        assert f[0, 3, 3] == 2 and d[0, 3, 3] == 0
        assert f[0, 11, 23] == -1 and d[0, 11, 23] == 0 and f[0, 0, 0] == -1 and d[0, 0, 0] == 0
    d2 = ref.forward32(obs, v, faces, with_d2=True)[2]
    assert d2[0, 8, 16] == 9.0
    # the gradient: nothing from the pixels at distance 0 or without a face, the fourth float 0
    from spherehand_amd import ops
    d, f = run(obs, v, faces)
    g = ops.mesh_data_to_model_bwd(dev(obs), dev(v), dev(faces), dev(d), dev(f), dev(np.ones_like(obs)), fg_max=500.0)
    g = g.cpu().numpy()
    lone = obs.copy()
    lone[0, 4, 8] = lone[0, 3, 3] = lone[0, 11, 23] = 1000.0
    want = ref.grad64(lone, v, faces, d, f, np.ones_like(obs), fg_max=500.0)
    assert np.all(g[..., 3] == 0) and np.all(g[0, [3, 4, 8]] == 0)
    assert np.abs(g[..., :3] - want).max() < 1e-6 and np.abs(want).max() > 0.4


def test_cull_adversaries():
    """Built against the bounding-sphere cull; the restatement has none.
    far cluster: 300 tiny faces in a ball of radius 0.5 about (300, 300, 50) -- each a good seed and a tight bound -- and
    one LARGE face whose corner a lies at the far end: its sphere about a reaches over the points while the face itself
    passes them at a distance, on either side of the cluster's distance.
    near 640: coordinates of 630..640, faces a few tenths across, distances below 1: the roundings of |ap|^2 are largest
    relative to the distances."""
    rs = np.random.RandomState(3)
    c = np.array([300.0, 300.0, 50.0])
    tiny = c + rs.uniform(-0.5, 0.5, (300, 3))
    v = np.ones((2, 904, 4), F32)
    v[:, :900, :3] = (tiny[:, None, :] + rs.uniform(-0.01, 0.01, (300, 3, 3))).reshape(900, 3)
    # crop 0: the large face passes (0..30, 0..30) at z = 50 + 800: farther than the cluster; crop 1: at z = 60, nearer
    for b, z in ((0, 850.0), (1, 60.0)):
        v[b, 900:903, :3] = [[2000.0, 2000.0, z], [-2000.0, 10.0, z], [10.0, -2000.0, z]]
    faces = np.concatenate([np.arange(900).reshape(300, 3), [[900, 901, 902]]]).astype(np.int32)
    faces = faces[rs.permutation(301)]
    obs = rs.uniform(45, 55, (2, 6, 6)).astype(F32)
    d, f = same(obs, v, faces, (6.0, 0.0, 6.0, 0.0), tag="far cluster")
    large = int(np.nonzero(faces[:, 0] == 900)[0][0])
    assert np.all(f[0] != large) and np.all(f[1] == large) and d[0].min() > 350 and d[1].max() < 20
    # near 640
    NV, F = 1500, 3000
    v = np.ones((1, NV, 4), F32)
    v[0, :, :3] = rs.uniform(630, 640, (NV, 3))
    near = np.argsort(((v[0, :, None, :3] - v[0, None, :, :3]) ** 2).sum(-1), 1)[:, :8]
    faces = np.stack([rs.randint(0, NV, F)] * 3, 1)
    faces[:, 1] = near[faces[:, 0], rs.randint(1, 8, F)]
    faces[:, 2] = near[faces[:, 0], rs.randint(1, 8, F)]
    obs = rs.uniform(630, 640, (1, 16, 16)).astype(F32)
    d, f = same(obs, v, faces.astype(np.int32), (0.625, 630.0, 0.625, 630.0), fg_max=1000.0, tag="near 640")
    assert np.median(d) < 1 and len(np.unique(f)) > 50


def test_indices_from_memory_are_range_checked():
    """Face ids of -1, NV and INT_MIN in faces; in the backward face entries of -2, F and INT_MAX in a hand-made map: the
    result is the restatement's, which skips them, and the guard regions around every output stay as they were."""
    from spherehand_amd import _lib
    lib, p = _lib.lib(), lambda t: t.data_ptr()   # noqa: E731
    B, NV, F, H, W = 2, 60, 300, 9, 67
    v, faces, obs = soup(B, NV, F, H, W, 21)
    rs = np.random.RandomState(22)
    bad = rs.permutation(F)[:45]
    faces[bad[:15], rs.randint(0, 3, 15)] = -1
    faces[bad[15:30], rs.randint(0, 3, 15)] = NV
    faces[bad[30:], rs.randint(0, 3, 15)] = np.iinfo(np.int32).min
    want_d, want_f = ref.forward32(obs, v, faces, fg_max=500.0)
    assert not np.isin(want_f, bad).any()
    plain = ref.forward32(obs, v, soup(B, NV, F, H, W, 21)[1], fg_max=500.0)[1]
    assert (plain != want_f).sum() > 20                               # the skipped faces mattered
    G, n = 4096, B * H * W
    dist = torch.full((n + 2 * G,), -7.0, device="cuda")
    face = torch.full((n + 2 * G,), -77, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.shr_mesh_d2m_workspace_bytes(B, F), dtype=torch.uint8, device="cuda")
    tv, tf, to = dev(v), dev(faces), dev(obs)
    rc = lib.shr_mesh_d2m_fwd(p(to), p(tv), p(tf), B, NV, F, W, H, 1.0, 0.0, 1.0, 0.0, 500.0, INF, p(dist) + 4 * G,
                              p(face) + 4 * G, p(ws), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert (dist[:G] == -7).all() and (dist[-G:] == -7).all() and (face[:G] == -77).all() and (face[-G:] == -77).all()
    assert np.array_equal(bits(dist[G:-G].cpu().numpy().reshape(B, H, W)), bits(want_d))
    assert np.array_equal(face[G:-G].cpu().numpy().reshape(B, H, W), want_f)
    # the backward on a map with entries out of range
    fmap = want_f.copy()
    r = rs.rand(B, H, W)
    fmap[r < 0.05] = -2
    fmap[(r >= 0.05) & (r < 0.1)] = F
    fmap[(r >= 0.1) & (r < 0.15)] = np.iinfo(np.int32).max
    fmap[(r >= 0.15) & (r < 0.2)] = bad[rs.randint(0, 45, ((r >= 0.15) & (r < 0.2)).sum())]   # in range, ids out of range
    gd = rs.standard_normal((B, H, W)).astype(F32)
    terms = fpr.Terms.from_taps(*ref.taps64(obs, v, faces, want_d, fmap, gd, fg_max=500.0), B, NV)
    full = fpr.Terms.from_taps(*ref.taps64(obs, v, faces, want_d, want_f, gd, fg_max=500.0), B, NV)
    assert np.abs(terms.sums() - full.sums()).max() > 1e-2
    out = torch.full((B * NV * 4 + 2 * G,), -7.0, device="cuda")
    ws = torch.empty(lib.shr_mesh_d2m_bwd_workspace_bytes(B, NV), dtype=torch.uint8, device="cuda")
    td, tm, tg = dev(want_d), dev(fmap), dev(gd)
    rc = lib.shr_mesh_d2m_bwd(p(to), p(tv), p(tf), p(td), p(tm), p(tg), B, NV, F, W, H, 1.0, 0.0, 1.0, 0.0,
                              500.0, INF, p(out) + 4 * G, p(ws), None)
    torch.cuda.synchronize()
    assert rc == 0 and (out[:G] == -7).all() and (out[-G:] == -7).all()
    got = out[G:-G].cpu().numpy().reshape(B, NV, 4)
    assert np.all(got[..., 3] == 0)
    fpr.check_bound(got[..., :3], terms, fpr.term_bits(3, W, H), "indices out of range")


def bwd_case(name):
    """(obs, v, faces, p2m, fg_max, dist, face, gd): toy -- 15 vertices, the LDS sums; hand -- 10 144, global sums in runs"""
    rs = np.random.RandomState(len(name))
    if name == "toy":
        rest, faces, obs = toy_case()
        obs = np.repeat(obs, 3, 0)
        v = np.concatenate([ref.moved(rest, t) for t in (ref.FIT_SHIFT, (-1.0, 2.0, -3.0), (0.0, 0.0, 9.0))])
        p2m, fg_max = (1.0, 0.0, 1.0, 0.0), ref.REF_FG_MAX
        dist, face = ref.forward32(obs, v, faces, p2m, fg_max, 8.0)
    else:
        c = hand_case()
        obs, v, faces, p2m, fg_max = c["obs"], c["v"], c["faces"], c["p2m"], 500.0
        dist, face = ref.forward32(obs, v, faces, p2m, fg_max, 8.0)
    gd = rs.standard_normal(obs.shape).astype(F32)
    gd[rs.rand(*obs.shape) < 0.2] = 0
    return obs, v, faces, p2m, fg_max, dist, face, gd


def gpu_bwd(case, sl=slice(None), max_dist=8.0):
    from spherehand_amd import ops
    obs, v, faces, p2m, fg_max, dist, face, gd = case
    return ops.mesh_data_to_model_bwd(dev(obs[sl]), dev(v[sl]), dev(faces), dev(dist[sl]), dev(face[sl]), dev(gd[sl]), p2m,
                                      fg_max, max_dist)


@pytest.mark.parametrize("name", ["toy", "hand"])
def test_backward_values(name):
    case = bwd_case(name)
    obs, v, faces, p2m, fg_max, dist, face, gd = case
    B, NV = v.shape[:2]
    d, f = run(obs, v, faces, p2m, fg_max, 8.0)
    assert np.array_equal(bits(d), bits(dist)) and np.array_equal(f, face)
    assert (dist == 8).any() and ((dist > 0) & (dist < 8)).sum() > 50          # saturated pixels: constants
    got = gpu_bwd(case).cpu().numpy()
    assert got.shape == (B, NV, 4) and np.all(got[..., 3] == 0) and np.all(bits(got[..., 3]) == 0)
    terms = fpr.Terms.from_taps(*ref.taps64(obs, v, faces, dist, face, gd, p2m, fg_max, 8.0), B, NV)
    fpr.check_bound(got[..., :3], terms, fpr.term_bits(3, obs.shape[2], obs.shape[1]), name)
    untouched = terms.counts().sum(-1) == 0
    assert (untouched.any() or name == "toy") and np.all(got[untouched] == 0) and np.abs(got).max() > 0


@pytest.mark.parametrize("name", ["toy", "hand"])
def test_deterministic_and_batch_independent(name):
    from spherehand_amd import ops
    case = bwd_case(name)
    obs, v, faces, p2m, fg_max = case[:5]
    B = v.shape[0]
    five = lambda a: np.concatenate([a] * 3)[:5]   # noqa: E731
    big = tuple(five(a) if k not in (2, 3, 4) else a for k, a in enumerate(case))
    fwd = lambda c, sl: ops.mesh_data_to_model(dev(c[0][sl]), dev(c[1][sl]), dev(faces), p2m, fg_max, 8.0)   # noqa: E731
    a, b = fwd(big, slice(None)), fwd(big, slice(None))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    ga, gb = gpu_bwd(big), gpu_bwd(big)
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)) and ga.abs().max() > 0
    for k in range(5):
        one = fwd(big, slice(k, k + 1))
        assert torch.equal(one[0][0].view(torch.int32), a[0][k].view(torch.int32)) and torch.equal(one[1][0], a[1][k]), k
        assert torch.equal(gpu_bwd(big, slice(k, k + 1))[0].view(torch.int32), ga[k].view(torch.int32)), k
    assert B <= 5


def test_through_autograd_and_the_module():
    from spherehand_amd import ops
    from spherehand_amd.render import MeshDataToModelLoss
    obs, v, faces, p2m, fg_max, dist, face, _ = bwd_case("toy")
    w = torch.tensor([0.5, -1.25, 2.0], device="cuda")[:, None, None]
    want = None
    for width in (4, 3):
        x = dev(v[..., :width]).requires_grad_(True)
        d, f = ops.MeshDataToModel.apply(dev(obs), x, dev(faces), p2m, fg_max, 8.0)
        assert np.array_equal(bits(d.detach().cpu().numpy()), bits(dist)) and np.array_equal(f.cpu().numpy(), face)
        assert not f.requires_grad
        (d * w).sum().backward()
        if want is None:
            want = ops.mesh_data_to_model_bwd(dev(obs), dev(v), dev(faces), dev(dist), dev(face),
                                              w.expand(3, 33, 33).contiguous(), p2m, fg_max, 8.0)
        assert x.grad.shape == x.shape
        assert torch.equal(x.grad.view(torch.int32), want[..., :width].contiguous().view(torch.int32)) and x.grad.abs().max() > 0
    term = MeshDataToModelLoss(33, 33, faces).cuda()
    assert term.fg_max == ref.REF_FG_MAX == 99.00000762939453 and term.max_dist == 50.0
    x = dev(v).requires_grad_(True)
    loss = term(dev(obs), x)
    want_loss, want_grad = ref.loss_and_grad(obs, v, faces)
    assert abs(loss.item() - want_loss) <= 2.0 ** -20 * want_loss and want_loss > 0.5
    loss.backward()
    assert np.abs(x.grad.cpu().numpy()[..., :3] - want_grad).max() <= 2.0 ** -20 * np.abs(want_grad).max()
    d, f = term.distances(dev(obs), dev(v))
    assert np.array_equal(bits(d.cpu().numpy()), bits(ref.forward32(obs, v, faces, p2m, ref.REF_FG_MAX, 50.0)[0]))
    # the reference's grid and background rule: d > 99 is background, so 99 is a data point, 99.5 and 100 are not
    grid = MeshDataToModelLoss.reference_grid(4, 2)
    assert grid == (75.0, -150.0, 150.0, -150.0)
    term = MeshDataToModelLoss(4, 2, faces, grid).cuda()
    img = np.array([[[99.0, 99.5, 100.0, 50.0], [np.nextafter(F32(99), F32(0)), np.nextafter(F32(99), F32(200)), 1000.0, 0.0]]], F32)
    d, f = term.distances(dev(img), dev(v[:1]))
    assert np.array_equal(f.cpu().numpy() >= 0, ~(img > 99)) and (f.cpu().numpy() >= 0).sum() == 4
    assert np.array_equal(bits(d.cpu().numpy()), bits(ref.forward32(img, v[:1], faces, grid, ref.REF_FG_MAX, 50.0)[0]))
    with pytest.raises(RuntimeError, match="observed"):
        term(dev(obs), dev(v))
    with pytest.raises(RuntimeError, match="max_dist"):
        ops.mesh_data_to_model(dev(obs), dev(v), dev(faces), max_dist=-1.0)
    with pytest.raises(RuntimeError, match="vertices"):
        ops.mesh_data_to_model(dev(obs), dev(v[:1]), dev(faces))
    with pytest.raises(RuntimeError, match="face"):
        ops.mesh_data_to_model_bwd(dev(obs), dev(v), dev(faces), dev(dist), dev(face).float(), dev(dist))


def test_graph_capture():
    """forward + backward captured once on one stream, replayed after the inputs change in place: the eager bits"""
    from spherehand_amd import ops
    obs, v, faces, p2m, fg_max = bwd_case("toy")[:5]
    base, seen = dev(v), dev(obs)
    x = base.clone().requires_grad_(True)
    o = seen.clone()
    tf = dev(faces)
    w = torch.tensor([0.5, -1.25, 2.0], device="cuda")[:, None, None]

    def step():
        d, f = ops.MeshDataToModel.apply(o, x, tf, p2m, fg_max, 8.0)
        g, = torch.autograd.grad((d * w).sum(), x)
        return d.detach(), f, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step()
    for shift in (0.0, 3.25, -7.5):
        with torch.no_grad():
            x.copy_(base + torch.tensor([shift, -0.5 * shift, 0.25 * shift, 0.0], device="cuda"))
            o.copy_(torch.where(seen < 99, seen + 0.125 * shift, seen))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in cap]
        eager = step()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, eager)), shift
    assert got[2].abs().max().item() > 0


def test_the_translation_fit_through_the_module():
    """tests/test_mesh_d2m_cpu.py's fit with MeshDataToModelLoss and torch's autograd: the same assertions, and the loss of
    every step within a bound of the restated trajectory's.  The bound carries the difference dt of the two translations
    through the steps: a step adds lr (E + L dt), E the fixed-point bound of the summed gradient (fixed_point_ref's, over
    every accumulator) plus its fp32 roundings, L = sum over the contributing points of |grad_dist| / dist the gradient's
    Lipschitz constant in the translation where the faces do not switch (a unit vector at distance d turns at 1 / d);
    the distance is 1-Lipschitz in the translation, so the losses differ by at most |dt| and the fp32 mean's 2^-20."""
    from spherehand_amd import ops
    from spherehand_amd.render import MeshDataToModelLoss
    rest, faces = ref.toy()
    S = ref.TOY_SIZE
    observed = ops.tri_raster_indexed_fwd(S, S, dev(rest), dev(faces))
    obs = observed.cpu().numpy()
    term = MeshDataToModelLoss(S, S, faces).cuda()
    r = dev(rest)
    t = torch.tensor(ref.FIT_SHIFT, device="cuda", requires_grad=True)
    losses = []
    for _ in range(ref.FIT_STEPS):
        loss = term(observed, torch.cat([r[..., :3] + t, r[..., 3:]], -1))
        g, = torch.autograd.grad(loss, t)
        losses.append(loss.item())
        with torch.no_grad():
            t -= ref.FIT_LR * g
    t = t.detach().cpu().numpy()
    # the restated trajectory with its carried bound
    tc, dt, bits_ = np.asarray(ref.FIT_SHIFT, F32), 0.0, fpr.term_bits(3, S, S)
    for k in range(ref.FIT_STEPS):
        v = ref.moved(rest, tc)
        dist, face = ref.forward32(obs, v, faces, fg_max=ref.REF_FG_MAX, max_dist=50.0)
        want = float(dist.astype(np.float64).mean())
        tol = dt + 2.0 ** -20 * want
        print("step %2d: loss %.6f, restated %.6f, difference %.3g, bound %.3g" % (k, losses[k], want, abs(losses[k] - want), tol))
        assert abs(losses[k] - want) <= tol, k
        gd = np.full(dist.shape, F32(1.0 / dist.size), F32)
        terms = fpr.Terms.from_taps(*ref.taps64(obs, v, faces, dist, face, gd, fg_max=ref.REF_FG_MAX, max_dist=50.0), 1, rest.shape[1])
        g = terms.sums().sum((0, 1))
        E = np.linalg.norm(terms.bound(bits_).sum((0, 1))) + 2.0 ** -20 * np.abs(terms.sums()).sum()
        live = (dist > 0) & (dist < 50) & (face >= 0)
        L = float((gd[live].astype(np.float64) / dist[live]).sum())
        dt = dt + ref.FIT_LR * (E + L * dt) + 2.0 ** -22 * (np.abs(tc).max() + ref.FIT_LR * np.abs(g).max())
        tc = (tc - F32(ref.FIT_LR) * g.astype(F32)).astype(F32)
    print("fit: GPU t = %s, restated t = %s, loss %.4f -> %.4f" % (t, tc, losses[0], losses[-1]))
    assert all(b <= a for a, b in zip(losses, losses[1:]))
    assert np.all(np.abs(t) < np.abs(np.asarray(ref.FIT_SHIFT)))
