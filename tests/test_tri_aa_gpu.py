"""The antialias pass on the GPU (ops.tri_antialias, ops.TriAntialias, render.AntialiasedDepthRaster): the forward and
both gradients against the fp64 restatement (tests/tri_aa_ref.py) on the hand and on random meshes, central differences
of the forward, bitwise copies away from the outline, determinism, batch independence and graph capture, continuity
under a sub-pixel sweep, and render-and-compare fits of a translation, which the raster alone cannot do."""
import numpy as np
import pytest
import torch

import tri_aa_ref as ref
from conftest import bits, golden

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hand(B=3, W=640, H=480):
    """g2_mesh.npz's hand vertices [B,10144,4] at z = 12 .. 275 (the clamp at 100 cuts the far side), x, y mapped onto W x H (crops 3 .. : crop 0 mirrored in
    x, a left hand for the cull), its faces (right hand's winding) and the welded edge table."""
    from spherehand_amd import hand_model, ops
    g = golden("g2_mesh.npz")
    v = g["verts"].copy()
    v = np.concatenate([v, v[:1], v[:1]])[:B]
    v[3:, :, 0] = 420.0 - v[3:, :, 0]
    v[..., 0] = (v[..., 0] + 110.0) * (W / 640.0)
    v[..., 1] = (v[..., 1] - 165.0) * (H / 490.0)
    v[..., 2] += 100.0
    faces = g["faces_swapped"].astype(np.int32)
    edges = ops.tri_edge_table(faces, np.asarray(hand_model.load_mesh()["vertices"]))
    return np.ascontiguousarray(v, np.float32), faces, edges


def _grid_mesh(B, W, H, seed):
    """A jittered, folded height field over the image: shared vertices, faces of both windings (the cull opens holes
    and inner silhouettes), depths 20 .. 80."""
    rng = np.random.default_rng(seed)
    n = 9
    gy, gx = np.mgrid[0:n, 0:n].astype(np.float64)
    faces = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, i * n + j + 1, (i + 1) * n + j, (i + 1) * n + j + 1
            faces += [[a, b, c], [b, d, c]]
    faces = np.array(faces)
    flip = rng.random(len(faces)) < 0.2
    faces[flip] = faces[flip][:, [1, 0, 2]]
    v = np.zeros((B, n * n, 4), np.float32)
    for bi in range(B):
        v[bi, :, 0] = gx.ravel() * (W - 1) / (n - 1) * 0.8 + 0.1 * W + rng.normal(0, 0.25 * W / n, n * n)
        v[bi, :, 1] = gy.ravel() * (H - 1) / (n - 1) * 0.8 + 0.1 * H + rng.normal(0, 0.25 * H / n, n * n)
        v[bi, :, 2] = rng.uniform(20, 80, n * n)
    from spherehand_amd import ops
    return v, faces.astype(np.int32), ops.tri_edge_table(faces)


def _run(v, faces, edges, W, H, values=None):
    from spherehand_amd import ops
    x, fc, ec = dev(v), dev(faces), dev(edges)
    depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, x, fc)
    c = torch.clamp(depth, max=100.0) if values is None else values
    return x, fc, ec, depth, owner, c.contiguous(), ops.tri_antialias(c.contiguous(), depth, owner, x, fc, ec)


def _check_forward(v, faces, edges, W, H):
    x, fc, ec, depth, owner, c, out = _run(v, faces, edges, W, H)
    want, info = ref.antialias(c.cpu(), depth.cpu(), owner.cpu(), v, faces, edges)
    got, want, cn = out.cpu().numpy(), want.numpy(), c.cpu().numpy()
    # per pixel: 2e-4 |c_f - c_o| + 1e-5 for each of its (up to four) pairs; |c_f - c_o| <= the 3 x 3 range of values
    pad = np.pad(cn, ((0, 0), (1, 1), (1, 1)), mode="edge")
    rng = np.max([np.abs(pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] - cn) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
    tol = 4 * (2e-4 * rng + 1e-5)
    keep = ~info["ambiguous"]
    blended = info["gain"].sum()
    assert blended > 0 and info["ambiguous"].sum() < 1e-3 * blended, (info["ambiguous"].sum(), blended)
    bad = keep & (np.abs(got - want) > tol)
    assert not bad.any(), (bad.sum(), np.abs(got - want)[bad].max())
    # a pixel that gains nothing is a bitwise copy
    same = ~info["gain"] & keep
    assert np.array_equal(bits(got[same]), bits(cn[same]))
    return blended


@pytest.mark.parametrize("W,H", [(640, 480), (640, 640), (97, 61)])
def test_forward_matches_the_restatement_on_the_hand(W, H):
    v, faces, edges = _hand(4, W, H)
    assert _check_forward(v, faces, edges, W, H) > 100


@pytest.mark.parametrize("W,H,seed", [(128, 96, 0), (97, 61, 1), (256, 256, 2)])
def test_forward_matches_the_restatement_on_random_meshes(W, H, seed):
    v, faces, edges = _grid_mesh(3, W, H, seed)
    assert _check_forward(v, faces, edges, W, H) > 50


def _square(shift=(0.0, 0.0), z=50.0, size=20.0, at=(21.37, 22.61)):
    """Two triangles of a constant-z square (corners in a shared vertex list) in pixel space, front-facing for the cull."""
    x0, y0 = at[0] + shift[0], at[1] + shift[1]
    v = np.array([[x0, y0, z, 1], [x0 + size, y0, z, 1], [x0 + size, y0 + size, z, 1], [x0, y0 + size, z, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    if not ref.drawn(v[None], faces[:1])[0, 0]:
        faces = faces[:, [1, 0, 2]]
    return v, faces.astype(np.int32)


def test_shared_diagonal_is_not_a_silhouette():
    from spherehand_amd import ops
    v, faces = _square()
    edges = ops.tri_edge_table(faces)
    assert (edges >= 0).sum() == 2
    x, fc, ec, depth, owner, c, out = _run(v[None], faces, edges, 64, 64)
    own = owner.cpu().numpy()[0]
    assert set(np.unique(own)) == {-1, 0, 1}
    # pixels where the two faces meet (and no background is near) are untouched
    diag = np.zeros_like(own, bool)
    diag[:, :-1] |= (own[:, :-1] >= 0) & (own[:, 1:] >= 0) & (own[:, :-1] != own[:, 1:])
    diag[:-1, :] |= (own[:-1, :] >= 0) & (own[1:, :] >= 0) & (own[:-1, :] != own[1:, :])
    inner = diag & (np.abs(np.arange(64)[None] - 31.4) < 6) & (np.abs(np.arange(64)[:, None] - 32.6) < 6)
    assert inner.sum() > 4
    o, cn = out.cpu().numpy()[0], c.cpu().numpy()[0]
    assert np.array_equal(bits(o[inner]), bits(cn[inner]))
    # ... while the outline blends; with an unwelded table the diagonal would blend too (equal values: no change)
    assert (o != cn).sum() > 40


def _centre_gap(v, faces):
    """The smallest distance, over every edge of `faces` (vertices v [NV,>=2]), between a crossing of an integer row
    (column) and the nearest pixel centre on it."""
    gap = np.inf
    for f in faces:
        for a in range(3):
            p, q = v[f[a]].astype(np.float64), v[f[(a + 1) % 3]].astype(np.float64)
            for i, j in ((1, 0), (0, 1)):           # crossings of rows (x at integer y), then of columns
                if p[i] == q[i]:
                    continue
                r = np.arange(np.ceil(min(p[i], q[i])), np.floor(max(p[i], q[i])) + 1)
                c = p[j] + (r - p[i]) * (q[j] - p[j]) / (q[i] - p[i])
                if len(c):
                    gap = min(gap, np.abs(c - np.round(c)).min())
    return gap


def _grad_case(v, faces, edges, W, H, seed):
    x, fc, ec, depth, owner, c, out = _run(v, faces, edges, W, H)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).cuda()
    from spherehand_amd import ops
    gvals, gverts = ops.tri_antialias_bwd(c, depth, owner, x, fc, ec, g)
    return x, fc, ec, depth, owner, c, g, gvals, gverts


@pytest.mark.parametrize("case", ["hand", "grid"])
def test_gradients_match_the_restatement(case):
    W, H = (640, 480) if case == "hand" else (128, 96)
    v, faces, edges = _hand(3, W, H) if case == "hand" else _grid_mesh(2, W, H, 5)
    x, fc, ec, depth, owner, c, g, gvals, gverts = _grad_case(v, faces, edges, W, H, 3)
    _, info = ref.antialias(c.cpu(), depth.cpu(), owner.cpu(), v, faces, edges)
    wc, wv = ref.grads(c.cpu(), depth.cpu(), owner.cpu(), v, faces, edges, g.cpu())
    gc, gv = gvals.cpu().numpy(), gverts.cpu().numpy()
    keep = ~info["ambiguous"]
    assert np.abs(gc[keep] - wc[keep]).max() <= 1e-4, np.abs(gc[keep] - wc[keep]).max()
    untouched = ~info["touched"]
    assert np.array_equal(bits(gc[untouched]), bits(g.cpu().numpy()[untouched]))
    assert np.all(gv[..., 2:] == 0)
    # vertex terms: every vertex of a pair near a threshold is left out of the comparison
    if info["ambiguous"].any():
        amb_faces = np.unique(owner.cpu().numpy()[info["ambiguous"]])
        amb_faces = amb_faces[amb_faces >= 0]
        skip = np.zeros(v.shape[:2], bool)
        skip[:, np.unique(faces[amb_faces])] = True
    else:
        skip = np.zeros(v.shape[:2], bool)
    scale = np.abs(wv).max()
    assert scale > 1.0
    err = np.abs(gv[..., :2] - wv[..., :2])[~skip]
    assert err.max() <= 2e-3 * scale, (err.max(), scale)


def test_gradients_match_central_differences():
    """Steep and shallow edges away from 45 degrees and from pixel centres: a step of 1e-3 px changes no decision, and the
    kernel's vertex gradient of <g, out> equals central differences of the kernel's forward, with nonzero x and y."""
    from spherehand_amd import ops
    W, H = 48, 40
    v0 = np.array([[[8.31, 5.27, 30, 1], [13.62, 33.71, 30, 1], [38.43, 21.19, 40, 1], [30.17, 4.42, 35, 1]]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    if not ref.drawn(v0, faces[:1])[0, 0]:
        faces = faces[:, [1, 0, 2]]
    rng = np.random.default_rng(11)
    v = v0
    while _centre_gap(v[0], faces) < 0.01:               # every crossing at least 0.01 px from a pixel centre
        v = v0.copy()
        v[0, :, :2] += rng.uniform(-0.2, 0.2, (4, 2)).astype(np.float32)
    faces = faces.astype(np.int32)
    edges = ops.tri_edge_table(faces)
    x, fc, ec, depth, owner, c, g, gvals, gverts = _grad_case(v, faces, edges, W, H, 7)
    g = g.abs() + 0.5
    _, gverts = ops.tri_antialias_bwd(c, depth, owner, x, fc, ec, g)
    got = gverts.cpu().numpy()[0]

    def loss(a):
        d, o = ops.tri_raster_indexed_owner_fwd(W, H, dev(a), fc)
        assert torch.equal(o, owner)
        return (ops.tri_antialias(c, depth, owner, dev(a), fc, ec).double() * g.double()).sum().item()

    h = 1e-3
    fd = np.zeros((4, 2))
    for i in range(4):
        for d in range(2):
            ap, am = v.copy(), v.copy()
            ap[0, i, d] += np.float32(h)
            am[0, i, d] -= np.float32(h)
            fd[i, d] = (loss(ap) - loss(am)) / float(ap[0, i, d] - am[0, i, d])
    assert np.abs(fd[:, 0]).max() > 1 and np.abs(fd[:, 1]).max() > 1
    np.testing.assert_allclose(got[:, :2], fd, rtol=2e-2, atol=2e-2 * np.abs(fd).max())


def test_deterministic_batch_independent_and_capturable():
    from spherehand_amd import ops
    from spherehand_amd.render import AntialiasedDepthRaster
    W, H = 640, 480
    v, faces, edges = _hand(5, W, H)
    x, fc, ec, depth, owner, c, g, gvals, gverts = _grad_case(v, faces, edges, W, H, 4)
    a = ops.tri_antialias_bwd(c, depth, owner, x, fc, ec, g)
    assert torch.equal(a[0], gvals) and torch.equal(a[1], gverts) and gverts.abs().max().item() > 0
    for i in (0, 2, 4):
        sl = lambda t: t[i:i + 1].contiguous()   # noqa: E731
        one = ops.tri_antialias_bwd(sl(c), sl(depth), sl(owner), sl(x), fc, ec, sl(g))
        assert torch.equal(one[0][0], gvals[i]) and torch.equal(one[1][0], gverts[i]), i
        assert torch.equal(ops.tri_antialias(sl(c), sl(depth), sl(owner), sl(x), fc, ec)[0],
                           ops.tri_antialias(c, depth, owner, x, fc, ec)[i])
    # the module's forward and backward, captured into a graph and replayed
    from spherehand_amd import hand_model
    mesh = hand_model.load_mesh()
    r = AntialiasedDepthRaster(W, H, mesh["faces"], np_vertices=np.asarray(mesh["vertices"])).cuda()
    assert torch.equal(r.edges_i32.cpu(), torch.from_numpy(edges))
    xs = x.clone().requires_grad_(True)

    def step():
        d = r(xs)
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
    assert torch.equal(d_eager, ops.tri_antialias(c, depth, owner, x, fc, ec))
    with torch.no_grad():
        xs.copy_(x.flip(0))
    graph.replay()
    d2, g2 = step()
    torch.cuda.synchronize()
    assert torch.equal(d_cap, d2) and torch.equal(g_cap, g2)


def test_output_is_continuous_under_a_subpixel_sweep():
    """A steep constant-z triangle over background swept in x by 0.01 px across two pixel centres: between samples no
    output pixel moves by more than step x |c_f - c_o| (plus rounding).  Its corners lie outside the image, so that every
    row holds one span between two steep edges (within a pixel of a corner the pairs of two edges meet)."""
    from spherehand_amd import ops
    W, H = 32, 32
    base = np.array([[10.37, -8.23, 40, 1], [14.91, 45.64, 40, 1], [3.13, 41.42, 40, 1]], np.float32)
    faces = np.array([[0, 1, 2]])
    if not ref.drawn(base[None], faces)[0, 0]:
        faces = faces[:, [1, 0, 2]]
    faces = faces.astype(np.int32)
    edges = ops.tri_edge_table(faces)
    fc, ec = dev(faces), dev(edges)
    step, outs, shifts = 0.01, [], []
    for k in range(231):
        dx = -1.1 + step * k
        v = base.copy()
        v[:, 0] += np.float32(dx)
        if _centre_gap(v, faces) < 1e-3:       # an edge within 1e-3 px of a centre: the raster's coverage rounding decides
            continue
        x = dev(v[None])
        depth, owner = ops.tri_raster_indexed_owner_fwd(W, H, x, fc)
        outs.append(ops.tri_antialias(torch.clamp(depth, max=100.0), depth, owner, x, fc, ec).cpu().numpy()[0])
        shifts.append(dx)
    assert len(outs) > 150
    dc = 100.0 - 40.0
    for a, b, sa, sb in zip(outs[:-1], outs[1:], shifts[:-1], shifts[1:]):
        jump = np.abs(b - a).max()
        assert jump <= (sb - sa) * dc * 1.0001 + 1e-3, (sa, sb, jump)


def _fit(r, target, v0, steps, lr):
    t = torch.zeros(2, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([t], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps)
    pad = torch.zeros(v0.shape[-1] - 2, device="cuda")
    for _ in range(steps):
        opt.zero_grad()
        loss = ((r(v0 + torch.cat([t, pad])) - target) ** 2).mean()
        loss.backward()
        opt.step()
        sched.step()
    return t.detach().cpu().numpy()


def test_translation_has_no_gradient_without_the_pass_and_fits_with_it():
    """A constant-z square shifted by (+2.3, -1.7) px: through TriangleDepthRaster + clamp its x/y gradient is zero; through
    AntialiasedDepthRaster 100 Adam steps on a 2-vector translation recover the shift within 0.1 px."""
    from spherehand_amd.render import AntialiasedDepthRaster, TriangleDepthRaster
    shift = np.array([2.3, -1.7])
    v, faces = _square()
    vt, _ = _square(tuple(shift))
    plain = TriangleDepthRaster(64, 64, faces, right_hand=False).cuda()
    aa = AntialiasedDepthRaster(64, 64, faces, right_hand=False, np_vertices=v).cuda()
    v0 = dev(v[None])
    t = torch.zeros(2, device="cuda", requires_grad=True)
    with torch.no_grad():
        target_plain = torch.clamp(plain(dev(vt[None])), max=100.0)
    loss = ((torch.clamp(plain(v0 + torch.cat([t, torch.zeros(2, device="cuda")])), max=100.0) - target_plain) ** 2).mean()
    loss.backward()
    assert loss.item() > 1 and t.grad.abs().max().item() < 1e-6
    with torch.no_grad():
        target = aa(dev(vt[None]))
    got = _fit(aa, target, v0, 100, 0.3)
    print("square fit:", got, "want", shift)
    assert np.abs(got - shift).max() < 0.1, got


def test_translation_fit_on_the_posed_hand():
    from spherehand_amd import hand_model
    from spherehand_amd.render import AntialiasedDepthRaster
    mesh = hand_model.load_mesh()
    v, _, _ = _hand(1, 640, 480)
    shift = np.array([2.3, -1.7], np.float32)
    aa = AntialiasedDepthRaster(640, 480, mesh["faces"], np_vertices=np.asarray(mesh["vertices"])).cuda()
    vt = v.copy()
    vt[..., :2] += shift
    with torch.no_grad():
        target = aa(dev(vt))
    got = _fit(aa, target, dev(v), 100, 0.3)
    print("hand fit:", got, "want", shift)
    assert np.abs(got - shift).max() < 0.25, got


def test_silhouette_is_a_differentiable_mask():
    from spherehand_amd import hand_model
    from spherehand_amd.render import AntialiasedDepthRaster
    mesh = hand_model.load_mesh()
    v, _, _ = _hand(2, 640, 480)
    aa = AntialiasedDepthRaster(640, 480, mesh["faces"], np_vertices=np.asarray(mesh["vertices"])).cuda()
    x = dev(v).requires_grad_(True)
    m = aa.silhouette(x)
    own = aa._raster(x.detach())[2]
    hard = (own >= 0).float()
    assert torch.isfinite(m).all()
    assert 0 < (m != hard).sum().item() < 0.2 * (own >= 0).sum().item()
    m.sum().backward()
    assert x.grad[..., :2].abs().max().item() > 0 and torch.all(x.grad[..., 2:] == 0)
