"""The triangle raster at its own resolution with a backward (ops.TriRaster / ops.TriRasterIndexed /
render.TriangleDepthRaster) on the GPU: the depth is depth_rasterization.forward's bit for bit at any W x H, the owners
made the pixels' depths, the gradients equal the torch restatement's autograd (tests/tri_grad_ref.py) and central
differences of the forward, the backward is bitwise reproducible, batch independent and capturable, and it fits a
mesh by render-and-compare."""
import numpy as np
import pytest
import torch

import tri_grad_ref as ref
from conftest import bits, golden

pytestmark = pytest.mark.gpu

SIZES = ((640, 640), (640, 480), (320, 640), (64, 32), (1, 1))     # (W, H)
QUIRKS = np.array([
    [[-0.5, -0.7, 5], [-0.2, 3.0, 5], [-0.1, -0.6, 5]], [[2, 2, 0], [2, 9, 4], [9, 2, 4]], [[5, 5, 3], [5, 9, 3], [5, 7, 3]],
    [[1, 1, 3], [4, 4, 3], [7, 7, 3]], [[np.nan, 1, 3], [4, 2, 3], [7, 9, 3]], [[3, 12, 2], [12, 3, 2], [3, 3, -2]],
    [[-40, -30, 7], [60, -20, 7], [10, 70, 7]], [[-0.7, 7.1, 5], [-3.2, 14.3, 7], [-9.4, 7.6, 6]],
    [[1e9, 3, 2], [2, 1e9, 2], [3, 3, 2]], [[2, -1e9, 2], [9, 1e9, 2], [4, 3, 2]],
], np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hand_soup(B):
    """[B,3382,3,3]: g2_mesh.npz's four hand crops (depths of both signs), the fifth their first reversed in x."""
    fv = golden("g2_mesh.npz")["face_vertices"]
    out = [fv[i % 4] for i in range(B)]
    if B > 4:
        out[4] = out[4] * np.float32([-1, 1, 1]) + np.float32([640, 0, 0])
    return np.ascontiguousarray(np.stack(out) if B else fv[:0], np.float32)


_random_soup = ref.random_soup          # (tests/tri_grad_ref.py: tests/test_fixed_point_gpu.py draws the same soups)


def _check_owner_raster(fv, W, H):
    """owner forward (soup and indexed) against depth_rasterization.forward: depth bits, owners, recomputed depths."""
    import depth_rasterization
    from spherehand_amd import ops
    B, F = fv.shape[:2]
    want = depth_rasterization.forward(W, H, dev(fv))
    depth, owner = ops.tri_raster_owner_fwd(W, H, dev(fv))
    assert depth.shape == (B, H, W) and owner.shape == (B, H, W) and owner.dtype == torch.int32
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want.cpu().numpy())), (B, F, W, H)
    verts, faces = ref.soup_as_indexed(fv)
    v4 = np.concatenate([verts, np.ones(verts.shape[:2] + (1,), np.float32)], -1) if F else np.ones((B, 1, 4), np.float32)
    di, oi = ops.tri_raster_indexed_owner_fwd(W, H, dev(v4), dev(faces.astype(np.int32)))
    assert torch.equal(di, depth) and torch.equal(oi, owner)
    d, own = depth.cpu().numpy(), owner.cpu().numpy()
    assert np.array_equal(own == -1, d == 1000.0)
    assert own.size == 0 or (own.min() >= -1 and own.max() < max(F, 0))
    if (own >= 0).any():
        (b, y, x), zp = ref.pixel_zp32(verts, faces, own)
        assert np.array_equal(bits(zp), bits(d[b, y, x]))
    return own


@pytest.mark.parametrize("band", [-1, 0, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_depth_bits_and_owners(W, H, band):
    """band -1: the default plan (the LDS band kernel wherever it fits); 0: the two-pass global-atomic kernel; 8: bands
    of at most 8 rows (faces straddle many bands)."""
    from spherehand_amd import ops
    ops.set_tuning(ops.TUNE_TRI_BAND, band)
    try:
        for B in (0, 1, 5):
            _check_owner_raster(_hand_soup(B), W, H)
            _check_owner_raster(_random_soup(B, 300, W, H, seed=B + W), W, H)
            _check_owner_raster(np.zeros((B, 0, 3, 3), np.float32), W, H)
        for fv in (QUIRKS[None], QUIRKS[None, ::-1], QUIRKS[None, :, [1, 0, 2], :]):
            _check_owner_raster(np.ascontiguousarray(fv), W, H)
    finally:
        ops.set_tuning(ops.TUNE_TRI_BAND, -1)


@pytest.mark.parametrize("band", [-1, 0])
def test_coincident_faces_go_to_the_smaller_index(band):
    from spherehand_amd import ops
    rng = np.random.default_rng(5)
    F = 40
    fv = np.concatenate([rng.uniform(50, 590, (1, F, 1, 2)) + rng.uniform(-60, 60, (1, F, 3, 2)),
                         rng.uniform(20, 90, (1, F, 3, 1))], -1).astype(np.float32)
    both = np.concatenate([fv[:, ::-1], fv], 1)                     # face F + i repeats face F - 1 - i
    ops.set_tuning(ops.TUNE_TRI_BAND, band)
    try:
        d1, o1 = ops.tri_raster_owner_fwd(640, 480, dev(fv))
        d2, o2 = ops.tri_raster_owner_fwd(640, 480, dev(both))
    finally:
        ops.set_tuning(ops.TUNE_TRI_BAND, -1)
    assert torch.equal(d1, d2) and (o1 >= 0).sum().item() > 1000
    o1, o2 = o1.cpu().numpy(), o2.cpu().numpy()
    assert np.array_equal(o2[o1 >= 0], F - 1 - o1[o1 >= 0])        # the reversed copy comes first: the smaller index
    assert np.array_equal(o2 < 0, o1 < 0)


def _hand_verts(B=4, W=640, H=480):
    """g2_mesh.npz's hand vertices [B,10144,4] moved to z = 212 .. 475 (well-conditioned depths), their x, y (-110 .. 528,
    165 .. 650) mapped onto a W x H image, and its faces (right hand's winding).  Crops 4 .. 6 repeat crop 0 mirrored in x."""
    g = golden("g2_mesh.npz")
    v = g["verts"].copy()
    v = np.concatenate([v, v[:1], v[:1], v[:1]])[:B]
    v[4:, :, 0] = 420.0 - v[4:, :, 0]
    v[..., 0] = (v[..., 0] + 110.0) * (W / 640.0)
    v[..., 1] = (v[..., 1] - 165.0) * (H / 490.0)
    v[..., 2] += 300.0
    return np.ascontiguousarray(v, np.float32), g["faces_swapped"].astype(np.int32)


def _close(got, want, rtol=1e-6, atol=1e-5):
    err = np.abs(got - want) - (atol + rtol * np.abs(want))
    assert err.max() <= 0, (float(np.abs(got - want).max()), float(np.abs(want).max()))


@pytest.mark.parametrize("W,H", [(640, 480), (64, 32), (320, 640)])
def test_gradient_matches_the_helper(W, H):
    from spherehand_amd import ops
    v, faces = _hand_verts(3, W, H)
    soup = np.ascontiguousarray(v[:, faces.astype(np.int64), :3])
    rnd = _random_soup(2, 300, W, H, seed=W)
    rnd[..., 2] = np.abs(rnd[..., 2]) + 20.0
    for fv in (soup, rnd):
        x = dev(fv)
        depth, owner = ops.tri_raster_owner_fwd(W, H, x)
        g = torch.randn(depth.shape, generator=torch.Generator().manual_seed(W + H)).cuda()
        got = ops.tri_raster_bwd(x, owner, g).cpu().numpy()
        verts, fidx = ref.soup_as_indexed(fv)
        want = ref.vertex_grad(torch.from_numpy(verts), fidx, owner, g).reshape(fv.shape)
        assert np.abs(want).max() > 0
        _close(got, want)
    # the indexed entry on the hand's shared vertices
    x, fc = dev(v), dev(faces)
    depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, x, fc)
    g = torch.randn(depth.shape, generator=torch.Generator().manual_seed(1)).cuda()
    got = ops.tri_raster_indexed_bwd(x, fc, owner, g).cpu().numpy()
    assert np.all(got[..., 3] == 0)
    _close(got[..., :3], ref.vertex_grad(torch.from_numpy(v), faces, owner, g)[..., :3])


def test_indexed_gradient_is_the_soup_gradient_scattered():
    from spherehand_amd import ops
    v, faces = _hand_verts(4)
    f64 = faces.astype(np.int64)
    x, fc = dev(v), dev(faces)
    soup = dev(v[:, f64, :3])
    for W, H in ((640, 640), (640, 480)):
        d_i, o_i = ops.tri_raster_indexed_owner_fwd(W, H, x, fc)
        d_s, o_s = ops.tri_raster_owner_fwd(W, H, soup)
        assert torch.equal(d_i, d_s) and torch.equal(o_i, o_s)
        g = torch.randn(d_i.shape, generator=torch.Generator().manual_seed(W + H)).cuda()
        gi = ops.tri_raster_indexed_bwd(x, fc, o_i, g).double().cpu()
        gs = ops.tri_raster_bwd(soup, o_s, g).double().cpu()               # [B,F,3,3]
        scat = torch.zeros(v.shape[0], v.shape[1], 3, dtype=torch.float64).index_add_(
            1, torch.from_numpy(f64.reshape(-1)), gs.reshape(v.shape[0], -1, 3))
        # the same fixed-point terms in the same unit: the two differ by the fp32 roundings of the soup's corners only
        scale = gs.abs().max().item()
        assert scale > 0
        np.testing.assert_allclose(gi[..., :3].numpy(), scat.numpy(), rtol=1e-6, atol=1e-6 * scale)


def test_gradient_matches_central_differences():
    """Faces whose pixels are all interior -- every pixel centre at least 0.05 px from every edge, separate cells, no
    overlaps -- so a step of 2e-3 px changes no coverage and no clamp: the kernel's gradient of <g, depth> equals central
    differences of the kernel's own forward."""
    from spherehand_amd import ops
    rng = np.random.default_rng(3)
    W, H = 64, 32
    faces = []
    for cy in range(4, H - 4, 8):
        for cx in range(4, W - 4, 8):
            while True:
                p = np.array([cx, cy], np.float64) + rng.uniform(-3.5, 3.5, (3, 2))
                if (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1]) < 0:
                    p = p[[1, 0, 2]]
                area = abs((p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1])) / 2
                if area < 6:
                    continue
                gx, gy = np.meshgrid(np.arange(cx - 5, cx + 6), np.arange(cy - 5, cy + 6))
                q = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64)
                dmin = np.inf
                for a in range(3):
                    e0, e1 = p[a], p[(a + 1) % 3]
                    t = np.clip(((q - e0) @ (e1 - e0)) / ((e1 - e0) @ (e1 - e0)), 0, 1)
                    dmin = min(dmin, np.linalg.norm(q - (e0 + t[:, None] * (e1 - e0)), axis=1).min())
                if dmin > 0.05:
                    break
            faces.append(np.concatenate([p, rng.uniform(20, 60, (3, 1))], 1))
    fv = np.asarray(faces, np.float32)[None]
    for flip in (False, True):                                  # (the culling rule's winding is the kernel's to decide)
        f = fv[:, :, [1, 0, 2]] if flip else fv
        _, owner = ops.tri_raster_owner_fwd(W, H, dev(f))
        if len(np.unique(owner.cpu().numpy())) > fv.shape[1] // 2:
            fv = np.ascontiguousarray(f)
            break
    x = dev(fv)
    depth, owner = ops.tri_raster_owner_fwd(W, H, x)
    live = np.unique(owner.cpu().numpy())
    assert len(live) > fv.shape[1] // 2 + 1
    g = torch.rand(depth.shape, generator=torch.Generator().manual_seed(2)).cuda() + 0.5
    got = ops.tri_raster_bwd(x, owner, g).double().cpu().numpy()

    def loss(a):
        d, o = ops.tri_raster_owner_fwd(W, H, dev(a))
        assert torch.equal(o, owner)                           # coverage held
        return (d.double() * g.double()).sum().item()

    h = 2e-3
    fd = np.zeros(fv.shape, np.float64)
    for f in live[live >= 0][:10]:
        for k in range(3):
            for c in range(3):
                ap, am = fv.copy(), fv.copy()
                ap[0, f, k, c] += np.float32(h)
                am[0, f, k, c] -= np.float32(h)
                fd[0, f, k, c] = (loss(ap) - loss(am)) / float(ap[0, f, k, c] - am[0, f, k, c])
        np.testing.assert_allclose(got[0, f], fd[0, f], rtol=2e-2, atol=2e-2 * np.abs(fd[0, f]).max())
    assert np.abs(fd).max() > 0.1


def test_backward_is_bitwise_reproducible_batch_independent_and_capturable():
    from spherehand_amd import ops
    W, H = 640, 480
    v, faces = _hand_verts(7, W, H)
    x, fc = dev(v), dev(faces)
    soup = dev(v[:, faces.astype(np.int64), :3])
    g = torch.randn(7, H, W, generator=torch.Generator().manual_seed(4)).cuda()

    def both(xb, sb, gb):
        _, oi = ops.tri_raster_indexed_owner_fwd(W, H, xb, fc)
        _, os_ = ops.tri_raster_owner_fwd(W, H, sb)
        return ops.tri_raster_indexed_bwd(xb, fc, oi, gb), ops.tri_raster_bwd(sb, os_, gb)

    a, b = both(x, soup, g), both(x, soup, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].abs().max().item() > 0
    for i in (0, 3, 6):
        one = both(x[i:i + 1].contiguous(), soup[i:i + 1].contiguous(), g[i:i + 1].contiguous())
        assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i]), i
    # autograd through the Functions, captured into a graph and replayed
    xs = x.clone().requires_grad_(True)

    def step():
        d = ops.TriRasterIndexed.apply(xs, fc, W, H)
        return d.detach(), torch.autograd.grad((d * g).sum(), xs)[0]

    d_eager, g_eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d_cap, g_cap = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d_cap, d_eager) and torch.equal(g_cap, g_eager)
    assert torch.equal(g_eager, a[0])
    with torch.no_grad():
        xs.copy_(x.flip(0))
    graph.replay()
    d2, g2 = step()
    torch.cuda.synchronize()
    assert torch.equal(d_cap, d2) and torch.equal(g_cap, g2)


def test_triangle_depth_raster_module():
    """TriangleDepthRaster: the forward-only raster's bits with and without grad, three- and four-wide vertices, and the
    face-soup Function agrees with the indexed one."""
    import depth_rasterization
    from spherehand_amd import hand_model, ops
    from spherehand_amd.render import TriangleDepthRaster
    mesh = hand_model.load_mesh()
    g2 = golden("g2_mesh.npz")
    r = TriangleDepthRaster(640, 480, mesh["faces"]).cuda()
    assert np.array_equal(r.faces_i32.cpu().numpy(), g2["faces_swapped"])
    v = dev(g2["verts"])
    want = depth_rasterization.forward(640, 480, dev(g2["face_vertices"]))
    assert torch.equal(r(v), want) and torch.equal(r(v[..., :3]), want)
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(3)).cuda()
    grads = []
    for width in (4, 3):
        vg = v[..., :width].clone().requires_grad_(True)
        d = r(vg)
        assert d.grad_fn is not None and torch.equal(d.detach(), want)
        (torch.clamp(d, max=100.0) * g).sum().backward()
        grads.append(vg.grad[..., :3])
    assert torch.equal(grads[0], grads[1])
    fv = dev(g2["face_vertices"]).requires_grad_(True)
    d = ops.TriRaster.apply(fv, 640, 480)
    assert torch.equal(d.detach(), want)
    (d * g).sum().backward()
    assert fv.grad.shape == fv.shape and torch.isfinite(fv.grad).all() and fv.grad.abs().max().item() > 0


def test_render_and_compare_fits_a_mesh():
    """640 x 480: the target is the hand rendered from a perturbed mesh (every vertex's depth moved by N(0, 3)); 30 Adam
    steps (lr 0.5) on the depths of the vertices, starting from the unperturbed mesh, on the MSE of the raw depths clamped
    at 100 as the reference clamps them.  The gradient holds coverage fixed, and so does a fit of the depths alone."""
    from spherehand_amd import hand_model
    from spherehand_amd.render import TriangleDepthRaster
    mesh = hand_model.load_mesh()
    v, _ = _hand_verts(2)
    v[..., 2] -= 200.0                                          # z = 12 .. 275: the clamp at 100 cuts the far side
    r = TriangleDepthRaster(640, 480, mesh["faces"]).cuda()
    xy, z0 = dev(v[..., :2]), dev(v[..., 2:3])
    noise = torch.randn(z0.shape, generator=torch.Generator().manual_seed(8)).cuda() * 3.0
    with torch.no_grad():
        target = torch.clamp(r(torch.cat([xy, z0 + noise], -1)), max=100.0)
    z = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr=0.5)

    def mse():
        return ((torch.clamp(r(torch.cat([xy, z], -1)), max=100.0) - target) ** 2).mean()

    with torch.no_grad():
        loss0 = mse().item()
    for _ in range(30):
        opt.zero_grad()
        loss = mse()
        loss.backward()
        opt.step()
    with torch.no_grad():
        loss1 = mse().item()
    print("fit: loss %.4g -> %.4g" % (loss0, loss1))
    assert torch.isfinite(z).all() and loss0 > 0.1
    assert loss1 < loss0 / 4, (loss0, loss1)
