"""Vertex normals and normal maps on the GPU (ops.tri_vertex_normals, ops.TriVertexNormals, ops.unit3_maps,
ops.Unit3Maps, render.MeshNormalRaster): the forward's bits against the fp32 restatement, the gradients against the fp64
restatement's autograd (tests/tri_normals_ref.py), determinism, batch independence and graph capture, the module's
claims, the tilt fit and the argument checks.

Gradient bound: the kernels evaluate in fp64 and round once, 2^-24; a factor 4 for the fp64 summation order:
max |difference| <= 2^-22 x the crop's largest gradient component."""
import numpy as np
import pytest
import torch

import tri_normals_ref as ref
from conftest import bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    """Bit for bit, a NaN for a NaN.  Which NaN an operation returns (sign, payload) is not part of IEEE 754, and the
    two sides need not agree: the device code evaluates a b - c d as a b + (-c) d (a negated multiply and an add: exact
    for numbers), which can hand a NaN on with its sign turned where numpy's subtraction keeps it."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (bits(got) != bits(want)))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        print("%d of %d differ; first at %s: got %r (%08x), want %r (%08x)"
              % (bad.sum(), bad.size, i, got[i], bits(got)[i], want[i], bits(want)[i]))
    return not bad.any()


def _tables(faces, NV, weld=None):
    from spherehand_amd import ops
    return ops.tri_vertex_tables(faces, NV, weld).to("cuda")


def _cases():
    """(name, points [B,NV,4], faces, weld, gradient faces: the same without NaN / 1e9 corners)"""
    v, f = ref.random_mesh(3, 40, 30, 1)
    fan_v, fan_f = ref.fan_mesh(3, 2)
    co_v, co_f = ref.coincident_mesh(2)
    gv, gf = ref.random_mesh(2, 40, 30, 3, quirks=False)
    sv, sf = ref.soup_of(gv[:, :81], gf[:128])                     # the folded grid as a soup, welded by position bits
    return [("random + quirks", v, f, None, ref.finite_part(v, f)),
            ("fan, isolated vertices", fan_v, fan_f, None, fan_f),
            ("coincident zero-area faces", co_v, co_f, None, co_f),
            ("soup welded by bits", sv, sf, sv[0, :, :3], sf),
            ("one vertex, no face", np.ones((2, 1, 4), np.float32), np.zeros((0, 3), np.int32), None,
             np.zeros((0, 3), np.int32))]


@pytest.mark.parametrize("case", range(5))
def test_forward_bits(case):
    from spherehand_amd import ops
    name, v, f, weld, _ = _cases()[case]
    n, N = ops.tri_vertex_normals(dev(v), dev(f), _tables(f, v.shape[1], weld), want_raw=True)
    only = ops.tri_vertex_normals(dev(v), dev(f), _tables(f, v.shape[1], weld))
    N32, n32, live = ref.normals32(v, f, weld)
    n, N = n.cpu().numpy(), N.cpu().numpy()
    assert same_bits(N[..., :3], N32), name
    assert same_bits(n[..., :3], n32), name
    assert np.all(n[..., 3] == 0) and np.all(N[..., 3] == 0) and np.array_equal(bits(only.cpu().numpy()), bits(n))
    assert not np.isnan(n).any()
    if case == 0:
        assert live.any() and (~live).any() and np.isnan(N).any()
    if case == 1:
        assert np.all(n[:, -3:] == 0) and live[:, 0].all()            # the isolated vertices; the hub of 64 faces
    if case == 2:
        assert np.all(n[:, :3] == 0) and live[:, 3:].all()
    if case == 3:
        # every face stores its own corners: copies of a position have the same bits
        keys = [r.tobytes() for r in v[0, :, :3]]
        a = keys.index(keys[-1])
        assert a != len(keys) - 1 and np.array_equal(bits(n[:, a]), bits(n[:, -1]))


def test_empty_batch_returns_cleanly():
    from spherehand_amd import ops
    v, f, _, _, _ = ref.random_mesh(1, 40, 30, 1) + (None, None, None)
    T = _tables(f, v.shape[1])
    e = torch.zeros(0, v.shape[1], 4, device="cuda")
    assert ops.tri_vertex_normals(e, dev(f), T).shape == (0, v.shape[1], 4)
    assert ops.tri_vertex_normals_bwd(e, dev(f), T, e).shape == (0, v.shape[1], 4)
    m = torch.zeros(0, 3, 5, 7, device="cuda")
    assert ops.unit3_maps(m).shape == m.shape and ops.unit3_maps_bwd(m, m).shape == m.shape


def test_forward_bits_on_the_hand_at_both_weldings():
    from spherehand_amd import ops
    v, faces, rest, index, first = ref.hand(2)
    n, N = ops.tri_vertex_normals(dev(v), dev(faces), _tables(faces, v.shape[1], rest), want_raw=True)
    N32, n32, live = ref.normals32(v, faces, rest)
    assert live.all()
    n, N = n.cpu().numpy()[..., :3], N.cpu().numpy()[..., :3]
    assert np.array_equal(bits(N), bits(N32)) and np.array_equal(bits(n), bits(n32))
    assert np.array_equal(bits(n), bits(n[:, first][:, index]))                         # copies are bit-identical
    fd = index[faces.astype(np.int64)].astype(np.int32)
    nd = ops.tri_vertex_normals(dev(v[:, first]), dev(fd), _tables(fd, len(first))).cpu().numpy()[..., :3]
    assert np.array_equal(bits(n), bits(nd[:, index]))                                  # ... and the distinct run's bits


def _check_grad(got, want, what):
    for b in range(want.shape[0]):
        top = np.abs(want[b]).max()
        err = np.abs(got[b].astype(np.float64) - want[b]).max()
        print("%s crop %d: max |diff| %.3g, largest component %.3g, ratio %.3g u" % (what, b, err, top, err / max(top, 1e-300) / U))
        assert err <= 4 * U * top, (what, b, err, top)


@pytest.mark.parametrize("case", range(5))
def test_gradient(case):
    from spherehand_amd import ops
    name, v, _, weld, f = _cases()[case]
    if case == 0:
        v = np.where(np.isfinite(v), v, np.float32(0))              # (the NaN corner's face is not in f; its vertex stays)
    g = np.random.default_rng(case).standard_normal(v.shape).astype(np.float32)
    got = ops.tri_vertex_normals_bwd(dev(v), dev(f), _tables(f, v.shape[1], weld), dev(g)).cpu().numpy()
    want = ref.normals_grad(v, f, weld, g)
    assert np.all(got[..., 3] == 0)
    _check_grad(got[..., :3], want, name)
    if case == 1:
        assert np.all(got[:, -3:] == 0) and np.abs(got[:, 0]).max() > 0
    if case == 2:
        assert np.all(got[:, :3] == 0) and np.abs(got[:, 3:, :3]).max() > 0
    if case == 4:
        assert np.all(got == 0)
    # autograd, three components in and out
    p3 = dev(v[..., :3]).requires_grad_(True)
    out = ops.TriVertexNormals.apply(p3, dev(f), _tables(f, v.shape[1], weld))
    gp, = torch.autograd.grad((out * dev(g)).sum(), p3)
    assert gp.shape == p3.shape and np.array_equal(bits(gp.cpu().numpy()), bits(got[..., :3]))


def test_gradient_on_the_hand():
    from spherehand_amd import ops
    v, faces, rest, index, first = ref.hand(2)
    g = np.random.default_rng(9).standard_normal(v.shape).astype(np.float32)
    got = ops.tri_vertex_normals_bwd(dev(v), dev(faces), _tables(faces, v.shape[1], rest), dev(g)).cpu().numpy()
    _check_grad(got[..., :3], ref.normals_grad(v, faces, rest, g), "hand, welded")
    fd = index[faces.astype(np.int64)].astype(np.int32)
    vd, gd = v[:, first], g[:, first]
    got = ops.tri_vertex_normals_bwd(dev(vd), dev(fd), _tables(fd, len(first)), dev(gd)).cpu().numpy()
    _check_grad(got[..., :3], ref.normals_grad(vd, fd, None, gd), "hand, distinct")


def _maps(B, H, W, seed):
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal((B, 3, H, W)) * rng.choice([1e-3, 1.0, 50.0], (B, 1, H, W))).astype(np.float32)
    m[:, :, ::3, ::5] = 0                                            # background pixels
    m[0, :, 1, 1] = [1e-41, 0, 0]                                    # a subnormal pixel (its square underflows: 0)
    m[0, :, 2, 3] = [3e-21, 1e-22, 0]                                # a subnormal sum of squares
    m[0, :, 2, 2] = [np.inf, 1, 2]                                   # an inf pixel
    m[0, :, 3, 3] = [2e19, 2e19, 0]                                  # finite, the sum of squares is not
    return m


@pytest.mark.parametrize("B,H,W", [(2, 29, 37), (1, 480, 640)])
def test_unit3_maps(B, H, W):
    from spherehand_amd import ops
    m = _maps(B, H, W, B)
    want, live = ref.unit3_maps32(m)
    x = dev(m)
    out = ops.unit3_maps(x)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert np.all(want[0, :, 1, 1] == 0) and np.all(want[0, :, 2, 2] == 0) and np.all(want[0, :, 3, 3] == 0)
    assert live[0, 2, 3] and not live[0, 0, 0]
    # an unaligned view takes the scalar kernel: the same bits
    flat = torch.zeros(m.size + 1, device="cuda")
    flat[1:] = x.reshape(-1)
    assert torch.equal(ops.unit3_maps(flat[1:].view(B, 3, H, W)), out)
    fin = np.where(np.isfinite(m), m, np.float32(0))
    g = np.random.default_rng(5).standard_normal(m.shape).astype(np.float32)
    mt = torch.from_numpy(fin).double().requires_grad_(True)
    (ref.unit3_maps64(mt) * torch.from_numpy(g).double()).sum().backward()
    xs = dev(fin).requires_grad_(True)
    got, = torch.autograd.grad((ops.Unit3Maps.apply(xs) * dev(g)).sum(), xs)
    _check_grad(got.cpu().numpy(), mt.grad.numpy(), "unit3 %dx%d" % (W, H))
    _, live = ref.unit3_maps32(fin)
    assert np.all(got.cpu().numpy().transpose(0, 2, 3, 1)[~live] == 0)
    # out overlapping maps: SHR_EINVAL
    with pytest.raises(RuntimeError, match="shr_unit3_maps_fwd"):
        ops.unit3_maps(x, out=x)
    buf = torch.zeros(m.size + 4, device="cuda")
    with pytest.raises(RuntimeError, match="shr_unit3_maps_fwd"):
        ops.unit3_maps(buf[:m.size].view(B, 3, H, W), out=buf[4:].view(B, 3, H, W))


def test_bitwise_reproducible_batch_independent_and_capturable():
    from spherehand_amd import ops
    v, f = ref.random_mesh(3, 40, 30, 4, quirks=False)
    sv, sf = ref.soup_of(v, f)
    g = np.random.default_rng(1).standard_normal(sv.shape).astype(np.float32)
    x, fc, gg = dev(sv), dev(sf), dev(g)
    T = _tables(sf, sv.shape[1], sv[0, :, :3] * 0 + np.arange(sv.shape[1])[:, None] // 3 % 50)   # an arbitrary welding
    m, gm = dev(_maps(3, 29, 37, 2)), torch.randn(3, 3, 29, 37, generator=torch.Generator().manual_seed(3)).cuda()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))

    def both(sl):
        p, q = x[sl].contiguous(), gg[sl].contiguous()
        return (ops.tri_vertex_normals(p, fc, T), ops.tri_vertex_normals_bwd(p, fc, T, q),
                ops.unit3_maps(m[sl].contiguous()), ops.unit3_maps_bwd(m[sl].contiguous(), gm[sl].contiguous()))

    full, again = both(slice(0, 3)), both(slice(0, 3))
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(full, again))
    assert full[1].abs().max().item() > 0
    for i in range(3):
        one = both(slice(i, i + 1))
        assert all(torch.equal(p[0].view(torch.int32), q[i].view(torch.int32)) for p, q in zip(one, full)), i
    # forward + backward captured into a graph, replayed twice with changed inputs: the eager bits
    xs, ms = x.clone().requires_grad_(True), m.clone().requires_grad_(True)

    def step():
        n = ops.TriVertexNormals.apply(xs, fc, T)
        o = ops.Unit3Maps.apply(ms)
        gx, gmaps = torch.autograd.grad((n * gg).sum() + (o * gm).sum(), (xs, ms))
        return n.detach(), o.detach(), gx, gmaps

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step()
    for scale in (1.0, 1.5, 0.75):
        with torch.no_grad():
            xs.copy_(x * scale + (scale - 1.0))
            ms.copy_(m * scale)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in cap]
        eager = step()
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(got, eager)), scale
    assert torch.equal(got[0], ops.tri_vertex_normals(xs.detach(), fc, T))


def test_module_on_the_hand():
    from spherehand_amd import ops
    from spherehand_amd.render import AntialiasedDepthRaster, MeshNormalRaster, TriangleDepthRaster
    W, H = 320, 240
    v, faces, rest, _, _ = ref.hand(2, W, H)
    x = dev(v)
    r = MeshNormalRaster(W, H, faces, right_hand=False, np_vertices=rest).cuda()
    xs = x.clone().requires_grad_(True)
    maps, depth = r(xs)
    assert torch.equal(depth.view(torch.int32), TriangleDepthRaster(W, H, faces, right_hand=False).cuda()(x).view(torch.int32))
    _, owner = ops.tri_raster_indexed_owner_fwd(W, H, x, dev(faces))
    own = owner.cpu().numpy()
    mp = maps.detach().cpu().numpy().transpose(0, 2, 3, 1)
    assert (own >= 0).sum() > 1000 and np.all(mp[own < 0] == 0)
    length = np.sqrt((mp.astype(np.float64) ** 2).sum(-1))[own >= 0]
    print("owned pixels: |length - 1| max %.3g u" % (np.abs(length - 1).max() / U))
    assert np.abs(length - 1).max() <= 4 * U
    # the orientation claim: in the raster's own winding every owner face has n_f.z >= 0 (it points away from the
    # camera), and the module's normals, from the turned faces, have z <= 0 on those faces
    used = np.unique(own[own >= 0])
    for b in range(2):
        ub = np.unique(own[b][own[b] >= 0])
        nz = ref.face_normals32(v[b:b + 1], faces[ub])[0][0, :, 2]
        assert np.all(nz >= 0) and (nz > 0).any(), nz.min()
        nt = ref.face_normals32(v[b:b + 1], faces[ub][:, [0, 2, 1]])[0][0, :, 2]
        assert np.array_equal(nt, -nz)
    assert len(used) > 100 and (mp[..., 2][own >= 0] < 0).mean() > 0.9
    # a loss on the map alone reaches z
    g = torch.randn(maps.shape, generator=torch.Generator().manual_seed(1)).cuda()
    gx, = torch.autograd.grad((maps * g).sum(), xs)
    assert gx.shape == xs.shape and gx[..., 2].abs().max().item() > 0 and torch.isfinite(gx).all() and (gx[..., 3] == 0).all()
    # antialias = True: AntialiasedDepthRaster's depth bits; blended outline pixels are shorter than 1
    ra = MeshNormalRaster(W, H, faces, right_hand=False, np_vertices=rest, antialias=True).cuda()
    ma, da = ra(x)
    want = AntialiasedDepthRaster(W, H, faces, right_hand=False, np_vertices=rest).cuda()(x)
    assert torch.equal(da.view(torch.int32), want.view(torch.int32))
    la = (ma.double() ** 2).sum(1).sqrt()
    assert ((la > 0.01) & (la < 0.99)).sum().item() > 10
    # `points`: metric normals from other points of the same mesh, and the gradient goes to them
    pts = (x[..., :3] * torch.tensor([0.5, 0.5, 1.0], device="cuda")).requires_grad_(True)
    mm, _ = r(x, pts)
    gp, = torch.autograd.grad((mm * g).sum(), pts)
    assert gp.shape == pts.shape and gp.abs().max().item() > 0 and not torch.equal(mm, maps.detach())


def test_fronto_parallel_square_is_exactly_minus_z():
    from spherehand_amd import ops
    from spherehand_amd.render import MeshNormalRaster
    v = np.array([[[3.3, 4.1, 57, 1], [40.7, 4.1, 57, 1], [3.3, 35.2, 57, 1], [40.7, 35.2, 57, 1]]], np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    maps, _ = MeshNormalRaster(48, 40, faces, right_hand=False).cuda()(dev(v))
    _, owner = ops.tri_raster_indexed_owner_fwd(48, 40, dev(v), dev(faces))
    own = owner.cpu().numpy()[0] >= 0
    mp = maps.cpu().numpy()[0]
    assert own.sum() > 500
    assert np.all(mp[0][own] == 0) and np.all(mp[1][own] == 0) and np.all(mp[2][own] == -1)
    assert np.all(mp[:, ~own] == 0)


def test_tilt_fit_matches_the_restatement():
    """A 5 x 5 grid over 48 x 48, z = a x + b y + 50; the target map at (0.3, -0.2); Adam with the cosine schedule, 100
    steps, from (0, 0), through MeshNormalRaster; the same run on restatement (b) (tests/test_tri_normals_cpu.py shows it
    within 0.01 of the target): the end points agree to 1e-3."""
    from spherehand_amd import ops
    from spherehand_amd.render import MeshNormalRaster
    v0, faces = ref.tilt_grid(0.0, 0.0)
    r = MeshNormalRaster(48, 48, faces, right_hand=False).cuda()
    _, owner = ops.tri_raster_indexed_owner_fwd(48, 48, v0.float().cuda().contiguous(), dev(faces))
    own = owner.cpu().numpy()
    assert (own >= 0).all()
    got = ref.tilt_fit(lambda v: r(v)[0], torch.float32, "cuda")
    want = ref.tilt_fit(lambda v: ref.module64(v, own, faces), torch.float64)
    print("tilt fit: GPU", got, "restatement", want, "target", ref.FIT_TARGET)
    assert np.abs(got - want).max() <= 1e-3, (got, want)


def test_wrappers_reject_bad_inputs():
    from spherehand_amd import ops
    from spherehand_amd.render import MeshNormalRaster
    v, f = ref.random_mesh(2, 40, 30, 0, quirks=False)
    x, fc = dev(v), dev(f)
    NV = v.shape[1]
    T = _tables(f, NV)
    host = ops.tri_vertex_tables(f, NV)
    g = torch.zeros_like(x)
    m = torch.zeros(2, 3, 8, 9, device="cuda")
    assert ops.tri_vertex_normals(x, fc, T).shape == (2, NV, 4)
    calls = [(lambda: ops.tri_vertex_normals(x.cpu(), fc, T), "points"),
             (lambda: ops.tri_vertex_normals(x.double(), fc, T), "points"),
             (lambda: ops.tri_vertex_normals(x[..., :3].contiguous(), fc, T), "points"),
             (lambda: ops.tri_vertex_normals(x.transpose(0, 1), fc, T), "points"),
             (lambda: ops.tri_vertex_normals(x, fc.long(), T), "faces"),
             (lambda: ops.tri_vertex_normals(x, fc.cpu(), T), "faces"),
             (lambda: ops.tri_vertex_normals(x, fc, host), "tables"),                       # numpy tables
             (lambda: ops.tri_vertex_normals(x, fc, None), "tables"),
             (lambda: ops.tri_vertex_normals(x, fc[:-1].contiguous(), T), "tables"),       # built for other faces
             (lambda: ops.tri_vertex_normals(x[:, :-1].contiguous(), fc, T), "tables"),    # ... another NV
             (lambda: ops.tri_vertex_normals_bwd(x, fc, T, g[:1].contiguous()), "grad_normals"),
             (lambda: ops.tri_vertex_normals_bwd(x, fc, T, g.double()), "grad_normals"),
             (lambda: ops.tri_vertex_normals_bwd(x, fc, T, g.cpu()), "grad_normals"),
             (lambda: ops.TriVertexNormals.apply(x[0], fc, T), "vertices"),
             (lambda: ops.unit3_maps(m.cpu()), "maps"),
             (lambda: ops.unit3_maps(m.double()), "maps"),
             (lambda: ops.unit3_maps(m[:, :2].contiguous()), "maps"),
             (lambda: ops.unit3_maps(m[0]), "maps"),
             (lambda: ops.unit3_maps(m, out=m[:1].contiguous()), "out"),
             (lambda: ops.unit3_maps_bwd(m, m.double()), "grad_out"),
             (lambda: ops.unit3_maps_bwd(m, m[:1].contiguous()), "grad_out"),
             (lambda: MeshNormalRaster(40, 30, f, right_hand=False).cuda()(x[0]), "vertices"),
             (lambda: MeshNormalRaster(40, 30, f, right_hand=False).cuda()(x, x[:1]), "points")]
    for call, word in calls:
        with pytest.raises(RuntimeError, match=word):
            call()
