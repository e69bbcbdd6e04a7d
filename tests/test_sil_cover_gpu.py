"""The nearest-site transform and the silhouette coverage term on the GPU (ops.nearest_site_transform, ops.sil_cover,
ops.sil_cover_bwd, ops.SilhouetteCover, render.SilhouetteCoverage) against the restatements of tests/sil_cover_ref.py:
the transform's bits, batch independence, the forward's bits and the backward within the fixed-point sums' bound, the
range checks, determinism, autograd, graph capture, argument errors, and the toy mesh grown back from s = 0.6 by the two
halves together where the first half alone does not move."""
import numpy as np
import pytest
import torch

import dt_ref
import sil_cover_ref as ref
from conftest import bits

pytestmark = pytest.mark.gpu

FG_MAX = ref.FG_MAX
OBS_FG_MAX = ref.FIT_FG_MAX


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_WANT = {}


def want_transform(H, W):
    """the restatement of patterns(H, W), computed once"""
    if (H, W) not in _WANT:
        _WANT[(H, W)] = ref.transform(ref.patterns(H, W), FG_MAX)
    return _WANT[(H, W)]


# (2, 2048): the widest image -- the row pass's largest LDS request, 32 KB, and the key's fields at their limits
@pytest.mark.parametrize("H,W", ref.SHAPES + [(2, 2048)])
def test_transform_bits(H, W):
    from spherehand_amd import ops
    depth = ref.patterns(H, W)
    want_d2, want = want_transform(H, W)
    d2, nearest = ops.nearest_site_transform(dev(depth), FG_MAX)
    assert d2.dtype == torch.int32 and nearest.dtype == torch.int32 and d2.shape == nearest.shape == (13, H, W)
    assert torch.equal(d2, ops.distance_transform(dev(depth), FG_MAX))
    d2, nearest = d2.cpu().numpy(), nearest.cpu().numpy()
    for k in range(len(depth)):
        bad = nearest[k] != want[k]
        assert not bad.any(), ("pattern %d: %d pixels differ, first at %s: got %d want %d"
                               % (k, bad.sum(), np.argwhere(bad)[0], nearest[k][bad][0], want[k][bad][0]))
        assert np.array_equal(d2[k], want_d2[k]), k
        if H * W <= 67 * 65:
            brute_d2, brute = ref.nearest_brute(dt_ref.sites(depth[k], FG_MAX))
            assert np.array_equal(nearest[k], brute) and np.array_equal(d2[k], brute_d2), k
    assert np.all(nearest[0] == -1) and np.all(nearest[11] == -1)
    assert np.array_equal(nearest[1], np.arange(H * W).reshape(H, W))          # a site is its own nearest
    assert np.all(nearest[2] == 0) and np.all(nearest[5] == H * W - 1)


@pytest.mark.parametrize("H,W", [(67, 65), (3, 130)])
def test_images_do_not_leak_and_batch_independent(H, W):
    from spherehand_amd import ops
    p = ref.patterns(H, W)
    want_d2, want = want_transform(H, W)
    trio = np.stack([p[9], p[0], p[5]])                      # an empty image between two different non-empty ones
    d2, nearest = ops.nearest_site_transform(dev(trio), FG_MAX)
    assert np.array_equal(nearest.cpu().numpy(), np.stack([want[9], want[0], want[5]]))
    assert np.array_equal(d2.cpu().numpy(), np.stack([want_d2[9], want_d2[0], want_d2[5]]))
    one = ops.nearest_site_transform(dev(trio[:1]), FG_MAX)
    assert torch.equal(one[0][0], d2[0]) and torch.equal(one[1][0], nearest[0])
    empty = ops.nearest_site_transform(torch.zeros(0, H, W, device="cuda"), FG_MAX)
    assert empty[0].shape == (0, H, W) and empty[1].shape == (0, H, W) and empty[1].dtype == torch.int32


# ---- the coverage term ----------------------------------------------------------------------------------------------------
_CASES = {}


def case(name):
    """The inputs of the coverage term, rendered on the GPU once and downloaded, with the restated transform of the render:
    toy    the mitten at 64 x 64 observed at rest; the models: scaled and moved three ways (55 vertices: the LDS sums)
    hand   tri_normals_ref.hand(2, 100, 190) in a 128 x 128 crop, observed from the same hand moved by (25, 18)
           (10 144 vertices: the sums in global memory, runs)"""
    if name in _CASES:
        return _CASES[name]
    from spherehand_amd import ops
    if name == "toy":
        rest, faces = ref.mitten()
        W = H = ref.MITTEN_SIZE
        v = np.concatenate([ref.model(rest, s, t) for s, t in ((0.75, (5.0, -3.0)), (0.6, (6.0, -4.0)), (1.1, (-4.0, 2.5)))])
        seen = np.repeat(rest, 3, 0)
    else:
        import tri_normals_ref
        v, faces = tri_normals_ref.hand(2, 100, 190)[:2]
        W = H = 128
        seen = v.copy()
        seen[..., 0] += np.float32(25.0)
        seen[..., 1] += np.float32(18.0)
        assert seen[0, :, 0].max() < 127 and seen[0, :, 1].max() < 127        # (the second pose reaches past the crop)
    faces = np.ascontiguousarray(faces, np.int32)
    observed = ops.tri_raster_indexed_fwd(W, H, dev(seen), dev(faces)).cpu().numpy()
    depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, dev(v), dev(faces))
    depth, owner = depth.cpu().numpy(), owner.cpu().numpy()
    d2, nearest = ref.transform(depth, 1000.0)
    rs = np.random.RandomState(len(name))
    gd = rs.standard_normal(observed.shape).astype(np.float32)
    gd[rs.rand(*observed.shape) < 0.2] = 0
    c = dict(v=v, faces=faces, observed=observed, depth=depth, owner=owner, d2=d2, nearest=nearest, gd=gd, W=W, H=H)
    _CASES[name] = c
    return c


def gpu_bwd(c, max_dist, sl=slice(None), **replace):
    """ops.sil_cover_bwd on the crops `sl` of a case, some of its inputs replaced"""
    from spherehand_amd import ops
    g = lambda k: replace.get(k, c[k])   # noqa: E731
    return ops.sil_cover_bwd(dev(g("observed")[sl]), OBS_FG_MAX, dev(g("d2")[sl]), dev(g("nearest")[sl]), dev(g("owner")[sl]),
                             dev(g("v")[sl]), dev(g("faces")), dev(g("gd")[sl]), max_dist)


def check_grad(got, want, m, W, H, tag):
    """|got - want| <= 2^-23 |want| + 3 W H 2^-40 m, m the crop's largest |term| (fixed_point.h: the unit puts the largest
    term below 2^41, so a term rounds by at most m 2^-41, an accumulator takes at most 3 W H terms, the conversion to fp32
    adds 2^-24 relative; both doubled)"""
    got = got.astype(np.float64)
    assert np.all(got[..., 2:] == 0) and np.all(bits(got[..., 2:].astype(np.float32)) == 0), tag
    err = np.abs(got[..., :2] - want)
    bound = 2.0 ** -23 * np.abs(want) + 3 * W * H * 2.0 ** -40 * m[:, None, None]
    print("%s: largest error %.3g, %.3g of its bound; largest |gradient| %.3g, largest term %.3g"
          % (tag, err.max(), (err / np.maximum(bound, 1e-300)).max(), np.abs(want).max(), m.max()))
    assert (err <= bound).all(), tag
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("name", ["toy", "hand"])
def test_forward_bits_and_backward_values(name):
    from spherehand_amd import ops
    c = case(name)
    d2g, nearg = ops.nearest_site_transform(dev(c["depth"]), 1000.0)
    assert np.array_equal(d2g.cpu().numpy(), c["d2"]) and np.array_equal(nearg.cpu().numpy(), c["nearest"])
    seen = c["observed"] < OBS_FG_MAX
    assert (seen & (c["d2"] > 0)).sum() > 200 and (np.sqrt(c["d2"][seen]) > 7.25).any()
    for max_dist in (float("inf"), 7.25):
        dist = ops.sil_cover(dev(c["observed"]), OBS_FG_MAX, d2g, max_dist).cpu().numpy()
        want = ref.cover32(c["observed"], OBS_FG_MAX, c["d2"], max_dist)
        assert np.array_equal(bits(dist), bits(want)), max_dist
        assert np.all(dist[~seen] == 0) and dist.max() == (np.float32(max_dist) if np.isfinite(max_dist) else want.max())
        got = gpu_bwd(c, max_dist).cpu().numpy()
        grad, m = ref.cover_grad64(c["observed"], OBS_FG_MAX, c["d2"], c["nearest"], c["owner"], c["v"], c["faces"], c["gd"],
                                   max_dist, with_max=True)
        assert got.shape == c["v"].shape[:2] + (4,)
        check_grad(got, grad, m, c["W"], c["H"], "%s, max_dist %s" % (name, max_dist))


@pytest.mark.parametrize("name", ["toy", "hand"])
def test_indices_from_memory_are_range_checked(name):
    """some nearest entries -1 or H W, some owner entries -1 or F, one face with a vertex id of NV: the result is the
    restatement's, which skips those pixels"""
    c = case(name)
    B, H, W = c["d2"].shape
    NV, F = c["v"].shape[1], len(c["faces"])
    rs = np.random.RandomState(7)
    nearest, owner, faces = c["nearest"].copy(), c["owner"].copy(), c["faces"].copy()
    used = nearest[0][(c["observed"][0] < OBS_FG_MAX) & (c["d2"][0] > 0) & (nearest[0] >= 0)]   # crop 0's pulled-on pixels
    r = rs.rand(B, H, W)
    nearest[r < 0.05] = -1
    nearest[(r >= 0.05) & (r < 0.1)] = H * W
    r = rs.rand(B, H, W)
    owner[(r < 0.05) & (owner >= 0)] = -1
    owner[(r >= 0.05) & (r < 0.1) & (owner >= 0)] = F
    busiest = np.bincount(c["owner"][0].ravel()[used], minlength=F).argmax()     # a face that is pulled on
    faces[busiest, 1] = NV
    got = gpu_bwd(c, float("inf"), nearest=nearest, owner=owner, faces=faces).cpu().numpy()
    grad, m = ref.cover_grad64(c["observed"], OBS_FG_MAX, c["d2"], nearest, owner, c["v"], faces, c["gd"], with_max=True)
    plain = ref.cover_grad64(c["observed"], OBS_FG_MAX, c["d2"], c["nearest"], c["owner"], c["v"], c["faces"], c["gd"])
    assert np.abs(grad - plain).max() > 1e-3                                   # the skipped pixels mattered
    check_grad(got, grad, m, W, H, "%s, indices out of range" % name)


@pytest.mark.parametrize("name", ["toy", "hand"])
def test_deterministic_and_batch_independent(name):
    c = case(name)
    B = c["v"].shape[0]
    a, b = gpu_bwd(c, 7.25), gpu_bwd(c, 7.25)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for k in range(B):
        one = gpu_bwd(c, 7.25, slice(k, k + 1))
        assert torch.equal(one[0].view(torch.int32), a[k].view(torch.int32)), k
    # an image whose render is empty: nearest -1 everywhere, a zero gradient
    empty = gpu_bwd(c, float("inf"), nearest=np.full_like(c["nearest"], -1))
    assert (empty == 0).all()


def toy_module():
    from spherehand_amd.render import SilhouetteCoverage
    c = case("toy")
    term = SilhouetteCoverage(c["W"], c["H"], c["faces"], OBS_FG_MAX, max_dist=9.5, right_hand=False).cuda()
    count = term.observe(dev(c["observed"]))
    assert np.array_equal(count.cpu().numpy(), (c["observed"] < OBS_FG_MAX).sum((1, 2)).astype(np.float32))
    return c, term, count


def test_through_autograd_and_a_wider_view():
    from spherehand_amd import ops
    c, term, count = toy_module()
    w = torch.tensor([0.5, -1.25, 2.0], device="cuda")
    v = dev(c["v"]).requires_grad_(True)
    out = term(v)
    assert out.shape == (3,)
    (out * w).sum().backward()
    d2 = dev(c["d2"])
    dist = ops.sil_cover(dev(c["observed"]), OBS_FG_MAX, d2, 9.5)
    assert torch.equal(out.detach(), dist.sum((1, 2)) / count)
    gd = (w / count)[:, None, None].expand(3, c["H"], c["W"]).contiguous()
    want = ops.sil_cover_bwd(dev(c["observed"]), OBS_FG_MAX, d2, dev(c["nearest"]), dev(c["owner"]), dev(c["v"]),
                             dev(c["faces"]), gd, 9.5)
    assert torch.equal(v.grad.view(torch.int32), want.view(torch.int32)) and v.grad.abs().max() > 0
    assert abs(term.loss(dev(c["v"])).item() - out.mean().item()) < 1e-6
    # a [B,NV,6] tensor: its first three components are taken; a view of its first four goes through .contiguous(); either
    # way the gradient comes back in the shape that was given
    for take in (lambda t: t, lambda t: t[..., :4], lambda t: t[..., :3]):
        wide = torch.zeros(3, c["v"].shape[1], 6, device="cuda")
        wide[..., :4] = dev(c["v"])
        wide.requires_grad_(True)
        (term(take(wide)) * w).sum().backward()
        assert wide.grad.shape == wide.shape
        assert torch.equal(wide.grad[..., :4].view(torch.int32), want.view(torch.int32)) and (wide.grad[..., 2:] == 0).all()


def test_graph_capture():
    """forward + backward captured once on one stream, replayed after the vertices change in place: the eager bits"""
    c, term, _ = toy_module()
    base = dev(c["v"])
    x = base.clone().requires_grad_(True)
    w = torch.tensor([0.5, -1.25, 2.0], device="cuda")

    def step():
        out = term(x)
        g, = torch.autograd.grad((out * w).sum(), x)
        return out.detach(), g

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
            x.copy_(base + torch.tensor([shift, -0.5 * shift, 0.0, 0.0], device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in cap]
        eager = step()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, eager)), shift
    assert got[1].abs().max().item() > 0


def test_argument_errors():
    from spherehand_amd import _lib, ops
    from spherehand_amd.render import SilhouetteCoverage
    c = case("toy")
    H, W = c["H"], c["W"]
    obs, d2, near, owner = dev(c["observed"]), dev(c["d2"]), dev(c["nearest"]), dev(c["owner"])
    v, faces, gd = dev(c["v"]), dev(c["faces"]), dev(c["gd"])
    bwd = lambda **kw: ops.sil_cover_bwd(*dict(dict(observed=obs, obs_fg_max=OBS_FG_MAX, d2=d2, nearest=near, owner=owner,   # noqa: E731
                                                    vertices=v, faces=faces, grad_dist=gd, max_dist=1.0), **kw).values())
    term = SilhouetteCoverage(W, H, c["faces"], OBS_FG_MAX, right_hand=False).cuda()
    seen = SilhouetteCoverage(W, H, c["faces"], OBS_FG_MAX, right_hand=False).cuda()
    seen.observe(obs)
    calls = [(lambda: ops.nearest_site_transform(obs.cpu(), FG_MAX), "depth"),
             (lambda: ops.nearest_site_transform(obs.transpose(1, 2), FG_MAX), "depth"),
             (lambda: ops.nearest_site_transform(obs.double(), FG_MAX), "depth"),
             (lambda: ops.nearest_site_transform(obs[0], FG_MAX), "depth"),
             (lambda: ops.nearest_site_transform(torch.zeros(1, 2049, 2, device="cuda"), FG_MAX), "shr_dt_nearest_fwd"),
             (lambda: ops.sil_cover(obs.cpu(), OBS_FG_MAX, d2), "observed"),
             (lambda: ops.sil_cover(obs.double(), OBS_FG_MAX, d2), "observed"),
             (lambda: ops.sil_cover(obs[0], OBS_FG_MAX, d2[0]), "observed"),
             (lambda: ops.sil_cover(obs, OBS_FG_MAX, d2.float()), "d2"),
             (lambda: ops.sil_cover(obs, OBS_FG_MAX, d2[:1].contiguous()), "d2"),
             (lambda: ops.sil_cover(obs, OBS_FG_MAX, d2, -1.0), "max_dist"),
             (lambda: ops.sil_cover(obs, OBS_FG_MAX, d2, float("nan")), "max_dist"),
             (lambda: bwd(nearest=near.float()), "nearest"),
             (lambda: bwd(nearest=near[:, :5].contiguous()), "nearest"),
             (lambda: bwd(owner=owner.cpu()), "owner"),
             (lambda: bwd(owner=owner.transpose(1, 2)), "owner"),
             (lambda: bwd(grad_dist=gd.double()), "grad_dist"),
             (lambda: bwd(grad_dist=gd[:1].contiguous()), "grad_dist"),
             (lambda: bwd(vertices=v[..., :3].contiguous()), "vertices"),
             (lambda: bwd(vertices=v[:1].contiguous()), "vertices"),
             (lambda: bwd(faces=faces.long()), "faces"),
             (lambda: bwd(max_dist=-2.0), "max_dist"),
             (lambda: ops.SilhouetteCover.apply(v[..., :2], faces, owner, d2, near, obs, OBS_FG_MAX), "vertices"),
             (lambda: term(v), "observe"),
             (lambda: term.observe(obs[:, :5]), "observe"),
             (lambda: seen(v[..., :2]), "vertices"),
             (lambda: seen(v[0]), "vertices")]
    for call, word in calls:
        with pytest.raises(RuntimeError, match=word):
            call()
    # the C calls' codes (include/spherehand_hip.h); every one of these returns before a launch
    lib, p = _lib.lib(), lambda t: t.data_ptr()
    ws = torch.empty(lib.shr_dt_nearest_workspace_bytes(3, H, W) + 16, dtype=torch.uint8, device="cuda")
    o1, o2 = torch.empty_like(d2), torch.empty_like(near)
    depth = dev(c["depth"])
    assert lib.shr_dt_nearest_fwd(p(depth), 3, H, W, 1000.0, p(o1), p(o2), p(ws), None) == 0
    assert torch.equal(o1, d2) and torch.equal(o2, near)
    assert lib.shr_dt_nearest_fwd(p(depth), 3, H, W, 1000.0, p(o1), p(o2), p(ws) + 4, None) == -1
    assert lib.shr_dt_nearest_fwd(p(depth), 3, H, W, 1000.0, p(o1), None, p(ws), None) == -1
    assert lib.shr_dt_nearest_fwd(p(depth), 3, H, 2049, 1000.0, p(o1), p(o2), p(ws), None) == -2
    assert lib.shr_dt_nearest_fwd(None, 0, H, W, 1000.0, None, None, None, None) == 0
    assert lib.shr_sil_cover_fwd(p(obs), OBS_FG_MAX, p(d2), 3, H, W, -1.0, p(gd), None) == -1
    assert lib.shr_sil_cover_fwd(p(obs), OBS_FG_MAX, None, 3, H, W, 1.0, p(gd), None) == -1
    out = torch.empty_like(v)
    ws = torch.empty(lib.shr_sil_cover_bwd_workspace_bytes(3, v.shape[1]) + 16, dtype=torch.uint8, device="cuda")
    args = [p(obs), OBS_FG_MAX, p(d2), p(near), p(owner), p(v), p(faces), p(gd), 3, v.shape[1], len(c["faces"]), W, H, 1.0,
            p(out), p(ws), None]
    bad = lambda i, val: lib.shr_sil_cover_bwd(*(args[:i] + [val] + args[i + 1:]))   # noqa: E731
    assert bad(15, p(ws) + 8) == -1 and bad(3, None) == -1 and bad(13, float("nan")) == -1 and bad(11, 2049) == -2
    assert bad(8, 0) == 0
    torch.cuda.synchronize()


def gpu_fit(rest, faces, observed, cover, s0, t0, steps):
    """sil_cover_ref.fit on the GPU: plain gradient descent on (s, t) under SilhouetteDistance.loss (+ SilhouetteCoverage.loss)"""
    from spherehand_amd.render import SilhouetteCoverage, SilhouetteDistance
    S = ref.MITTEN_SIZE
    first = SilhouetteDistance(OBS_FG_MAX).cuda()
    first.observe(observed)
    second = SilhouetteCoverage(S, S, faces, OBS_FG_MAX, right_hand=False).cuda()
    second.observe(observed)
    r = dev(rest)[0]
    c = r[:, :2].mean(0)
    s = torch.tensor(s0, device="cuda", requires_grad=True)
    t = torch.tensor(t0, device="cuda", requires_grad=True)
    losses = []
    for _ in range(steps):
        v = torch.cat([c + s * (r[:, :2] - c) + t, r[:, 2:]], -1)[None]
        loss = first.loss(v) + second.loss(v) if cover else first.loss(v)
        gs, gt = torch.autograd.grad(loss, (s, t))
        losses.append(loss.item())
        with torch.no_grad():
            s -= ref.FIT_LR_S * gs
            t -= ref.FIT_LR_T * gt
    return s.item(), t.detach().cpu().numpy(), losses


def test_the_pair_grows_the_mitten_back_and_the_first_half_alone_does_not():
    """The mitten observed at rest (rendered by TriangleDepthRaster).  The first half alone, from s = 0.6 and t = 0: every
    vertex lies inside the observation, the loss is 0 and s stays at 0.6 exactly -- the degenerate minimum.  Both halves
    from s = 0.6, t = (6, -4), sil_cover_ref's steps: the GPU fit must end within the restated fit's |s - 1| + 1 / R and
    |t| + 0.5 px, R = 19.1 px the mitten's half extent -- a margin of one pixel of silhouette quantisation, a judgement:
    coverage is decided at pixel centres, and two fits that differ by roundings may settle one quantum apart.
    What this shows and what it does not: the fixture is favourable.  The mitten's outline was placed a tenth of a pixel
    outside the covered pixel centres so that the two halves balance at s = 0.993; with the outline half a pixel off the
    centres they balance near s = 0.97, the edge of the restated fit's own limit.  The assertions show that the pair grows
    a model back that the first half alone leaves where it is, not that the balance point is robust to the outline's
    sub-pixel position."""
    from spherehand_amd.render import TriangleDepthRaster
    rest, faces = ref.mitten()
    S = ref.MITTEN_SIZE
    observed = TriangleDepthRaster(S, S, faces, right_hand=False).cuda()(dev(rest))
    obs = observed.cpu().numpy()
    assert 1000 < (obs < OBS_FG_MAX).sum() < 1600 and obs.max() == 1000
    s, t, losses = gpu_fit(rest, faces, observed, False, ref.FIT_S0, (0.0, 0.0), 5)
    assert s == float(np.float32(ref.FIT_S0)) and np.all(t == 0) and losses == [0.0] * 5
    want_s, want_t, want_losses = ref.fit(rest, faces, obs)
    s, t, losses = gpu_fit(rest, faces, observed, True, ref.FIT_S0, ref.FIT_T0, ref.FIT_STEPS)
    print("fit: GPU s = %.4f, t = (%.3f, %.3f) px, loss %.3f -> %.3f; restatement s = %.4f, t = (%.3f, %.3f) px, loss %.3f -> %.3f"
          % (s, t[0], t[1], losses[0], losses[-1], want_s, want_t[0], want_t[1], want_losses[0], want_losses[-1]))
    assert abs(want_s - 1) <= 0.03 and float(np.hypot(*want_t)) <= 0.5
    assert losses[0] > 3 and abs(losses[0] - want_losses[0]) < 1e-3
    assert abs(s - 1) <= abs(want_s - 1) + 1 / ref.MITTEN_HALF_EXTENT
    assert float(np.hypot(*t)) <= float(np.hypot(*want_t)) + 0.5
