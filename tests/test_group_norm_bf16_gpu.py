"""The bf16 GroupNorm+ReLU kernel pair on the GPU: against the fp64 restatement (tests/gn_bf16_ref.py) on identical bf16
inputs, against the fp32 kernels bit for bit, and inside the hourglass under autocast.

Bounds (y and dx, elementwise): |got - ref| <= 2^-8 |ref| + 2 e32, e32 = tests/test_group_norm_gpu.py's bar for the same
quantity (y: 2e-6 max(1, max|ref|), 5e-6 with a folded bias; dx: 2e-5 and 5e-5 likewise): the value in front of the
store is the fp32 kernels' value, within e32 of the reference, and one round-to-nearest-even to 8 significant bits adds
at most 2^-8 of it (bf16's unit roundoff: half an ulp at the lower end of a binade).  A store that truncates misses
it (tests/test_group_norm_bf16_cpu.py).  dgamma, dbeta and the bias gradient are fp32 outputs and meet the fp32
bars.  Input condition, not a tolerance: the reference's fp64 pre-activation has no element within 1e-5 of zero (a
ReLU decision that differs between fp32 and fp64 is no arithmetic error but moves a group sum by O(1/M)); the seed of
a case is the first of 0..7 that satisfies it."""
import numpy as np
import pytest

import gn_bf16_ref as ref
from gn_bf16_ref import SHAPES, bits, case, clear_seed

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REL = 2.0 ** -8
MARGIN = 1e-5


def _cl(t):
    return t.cuda().to(memory_format=torch.channels_last)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _check_elementwise(got, want, e32, name):
    err = np.abs(got - want)
    bar = REL * np.abs(want) + 2 * e32 * max(1.0, np.abs(want).max())
    worst = float((err / bar).max())
    print("%s: worst error / bound %.3f, max |ref| %.4g" % (name, worst, np.abs(want).max()))
    assert worst <= 1.0, name


def _check_fp32(got, want, tol, name):
    err = float(np.abs(got - want).max())
    print("%s: max error %.3g, bar %.3g" % (name, err, tol * max(1.0, np.abs(want).max())))
    assert err <= tol * max(1.0, np.abs(want).max()), name


def _run_direct(N, C, H, W, G, with_pre, seed):
    from spherehand_amd import ops
    x, gamma, beta, pre, dy = case(N, C, H, W, G, seed, with_pre)
    xg = _cl(x).requires_grad_(True)
    gn = torch.nn.GroupNorm(G, C).cuda()
    with torch.no_grad():
        gn.weight.copy_(gamma); gn.bias.copy_(beta)
    pg = None if pre is None else pre.cuda().requires_grad_(True)
    assert ops.group_norm_relu_supported(xg, G)
    y = ops.group_norm_relu(xg, gn, pg)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    (y.float() * _cl(dy).float()).sum().backward()
    assert xg.grad.dtype == torch.bfloat16 and gn.weight.grad.dtype == torch.float32 and gn.bias.grad.dtype == torch.float32
    out = {"y": y.detach(), "dx": xg.grad, "dgamma": gn.weight.grad, "dbeta": gn.bias.grad}
    if pg is not None:
        assert pg.grad.dtype == torch.float32
        out["dpre"] = pg.grad
    return (x, gamma, beta, pre, dy), out


@pytest.mark.parametrize("with_pre", [False, True])
@pytest.mark.parametrize("N,C,H,W,G", SHAPES)
def test_kernels_match_the_fp64_reference(N, C, H, W, G, with_pre):
    seed = clear_seed(N, C, H, W, G, with_pre, MARGIN)
    assert seed is not None
    (x, gamma, beta, pre, dy), out = _run_direct(N, C, H, W, G, with_pre, seed)
    r = ref.reference(bits(x), gamma.numpy(), beta.numpy(), G, 1e-5, None if pre is None else pre.numpy(), bits(dy))
    assert np.abs(r["pre"]).min() > MARGIN
    ey, eg = (5e-6, 5e-5) if with_pre else (2e-6, 2e-5)
    _check_elementwise(_np(out["y"]), r["y"], ey, "y")
    _check_elementwise(_np(out["dx"]), r["dx"], eg, "dx")
    for k in ("dgamma", "dbeta") + (("dpre",) if with_pre else ()):
        _check_fp32(_np(out[k]), r[k], eg, k)


@pytest.mark.parametrize("N,C,H,W,G", SHAPES)
def test_conv_then_kernels_under_autocast(N, C, H, W, G):
    """ops.conv_then_group_norm_relu under autocast: the bias-free bf16 convolution feeds the bf16 kernels, conv.bias
    (fp32) rides as pre_bias.  The reference takes the convolution's own bf16 output (the identical input of the
    kernels); the weight gradient, which comes from a bf16 MIOpen convolution, is held against the torch autocast
    composition's own distance from fp64 on the same inputs, x 2.
    The convolution's input and weights are small integers (x in -2..2, w in -1..1, 288 products: |sum| < 256), so the
    bf16 convolution is exact and its output IS the fp64 composition's: the input condition then covers the whole
    composition, and the weight gradient's distance from fp64 measures rounding, not ReLU decisions (one decision that
    differs moves an entry of dW by a whole product x * dy * gamma * rstd, a hundred times the rounding noise, and
    would make the comparison of two maxima a matter of chance)."""
    from spherehand_amd import ops
    Cin, k = 32, 3
    found = None
    for seed in range(8):
        g = torch.Generator().manual_seed(1000 + seed)
        conv = torch.nn.Conv2d(Cin, C, k, padding=1).cuda().to(memory_format=torch.channels_last)
        gn = torch.nn.GroupNorm(G, C).cuda()
        with torch.no_grad():
            conv.weight.copy_(_cl(torch.randint(-1, 2, (C, Cin, k, k), generator=g).float()))
            conv.bias.copy_(torch.randn(C, generator=g) * 2)
            gn.weight.copy_(torch.randn(C, generator=g)); gn.bias.copy_(torch.randn(C, generator=g) * 0.5)
        x = _cl(torch.randint(-2, 3, (N, Cin, H, W), generator=g).float())
        dy = torch.randn(N, C, H, W, generator=g).bfloat16()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            z = torch.nn.functional.conv2d(x, conv.weight, None, 1, 1)
        assert z.dtype == torch.bfloat16
        with torch.no_grad():
            assert torch.equal(z.double(), torch.nn.functional.conv2d(x.double(), conv.weight.double(), None, 1, 1))
        r = ref.reference(bits(z.cpu()), gn.weight.detach().cpu().numpy(), gn.bias.detach().cpu().numpy(), G, gn.eps,
                          conv.bias.detach().cpu().numpy(), bits(dy))
        if np.abs(r["pre"]).min() > MARGIN:
            found = seed
            break
    assert found is not None

    def run(fused):
        ops.FUSED_GROUP_NORM_RELU = fused
        try:
            for p in list(conv.parameters()) + list(gn.parameters()):
                p.grad = None
            xin = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = ops.conv_then_group_norm_relu(xin, conv, gn)
            (y.float() * _cl(dy).float()).sum().backward()
            return y.detach(), {n: p.grad.clone() for n, p in (("dW", conv.weight), ("dbias", conv.bias),
                                                               ("dgamma", gn.weight), ("dbeta", gn.bias))}
        finally:
            ops.FUSED_GROUP_NORM_RELU = True

    y, grads = run(True)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert all(v.dtype == torch.float32 for v in grads.values())
    _check_elementwise(_np(y), r["y"], 5e-6, "y")
    for name, key in (("dgamma", "dgamma"), ("dbeta", "dbeta"), ("dbias", "dpre")):
        _check_fp32(_np(grads[name]), r[key], 5e-5, name)
    # the weight gradient: fp64 composition on the same inputs, and torch's own autocast composition
    cd, gd = torch.nn.Conv2d(Cin, C, k, padding=1).cuda().double(), torch.nn.GroupNorm(G, C).cuda().double()
    cd.load_state_dict({n_: v.double() for n_, v in conv.state_dict().items()})
    gd.load_state_dict({n_: v.double() for n_, v in gn.state_dict().items()})
    (torch.relu(gd(cd(x.double().contiguous()))) * dy.cuda().double()).sum().backward()
    _, grads_t = run(False)
    err = (grads["dW"].double() - cd.weight.grad).abs().max().item()
    err_t = (grads_t["dW"].double() - cd.weight.grad).abs().max().item()
    print("dW: max error %.3g, torch autocast's own %.3g, max |ref| %.3g" % (err, err_t, cd.weight.grad.abs().max().item()))
    assert err <= 2 * err_t


@pytest.mark.parametrize("with_pre", [False, True])
@pytest.mark.parametrize("N,C,H,W,G", SHAPES)
def test_bit_for_bit_the_fp32_kernels_then_one_rounding(N, C, H, W, G, with_pre):
    """The header's claim: every sum is taken in the fp32 kernels' order, so y and dx are the fp32 kernels' values on
    the widened input rounded once to nearest even, and the fp32 outputs are theirs exactly."""
    from spherehand_amd import ops
    (x, gamma, beta, pre, dy), out = _run_direct(N, C, H, W, G, with_pre, 3)
    x32 = _cl(x.float()).requires_grad_(True)
    pg = None if pre is None else pre.cuda().requires_grad_(True)
    w, b = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    y32 = ops.GroupNormReLU.apply(x32, w, b, G, 1e-5, pg)
    (y32 * _cl(dy).float()).sum().backward()
    assert torch.equal(out["y"].view(torch.int16), y32.detach().bfloat16().view(torch.int16))
    assert torch.equal(out["dx"].view(torch.int16), x32.grad.bfloat16().view(torch.int16))
    assert torch.equal(out["dgamma"], w.grad) and torch.equal(out["dbeta"], b.grad)
    if with_pre:
        assert torch.equal(out["dpre"], pg.grad)


def test_two_calls_give_equal_bits():
    for (N, C, H, W, G), with_pre in ((SHAPES[1], True), (SHAPES[5], False)):
        _, a = _run_direct(N, C, H, W, G, with_pre, 0)
        _, b = _run_direct(N, C, H, W, G, with_pre, 0)
        for k in a:
            assert torch.equal(a[k].view(torch.int16) if a[k].dtype == torch.bfloat16 else a[k].view(torch.int32),
                               b[k].view(torch.int16) if b[k].dtype == torch.bfloat16 else b[k].view(torch.int32)), k


def test_bf16_activations_stay_on_the_kernels():
    """Without the feature group_norm_relu_supported answers False for bf16 and the pair falls back to torch."""
    from spherehand_amd import ops
    x = _cl(torch.randn(2, 64, 8, 8).bfloat16())
    gn = torch.nn.GroupNorm(16, 64).cuda()
    assert ops.group_norm_relu_supported(x, 16)
    called = []
    orig = torch.nn.functional.group_norm
    torch.nn.functional.group_norm = lambda *a, **k: called.append(1) or orig(*a, **k)
    try:
        y = ops.group_norm_relu(x, gn)
    finally:
        torch.nn.functional.group_norm = orig
    assert y.dtype == torch.bfloat16 and not called


def test_unsupported_bf16_shape_falls_back_to_torch():
    from spherehand_amd import ops
    x = torch.randn(2, 48, 8, 8).bfloat16().cuda()                        # C % 32 != 0
    gn = torch.nn.GroupNorm(4, 48).cuda()
    assert not ops.group_norm_relu_supported(x, 4)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(ops.group_norm_relu(x, gn), torch.relu(gn(x)))


def test_hourglass_under_autocast_with_and_without_the_kernels(monkeypatch):
    """The whole network, 6 crops @ 64^2, outputs and all parameter gradients of out.square().mean(): fp32 with the
    kernels, bf16 autocast on torch ops only, bf16 autocast with the bf16 kernels.  The kernels' distance from fp32 in
    relative max-norm (outputs; gradients) is at most 2 x torch's own autocast distance + 1e-6 -- the factor covers the
    two paths rounding at different points of the residual adds.  During the fused run F.group_norm raises: no pair of
    the network may fall back."""
    from spherehand_amd import ops
    from spherehand_amd.hourglass import create_hourglass_network
    torch.manual_seed(1)
    net = create_hourglass_network(82, 1).cuda().to(memory_format=torch.channels_last)
    x = _cl(torch.randn(6, 1, 64, 64))

    def run(amp, fused):
        ops.FUSED_GROUP_NORM_RELU = fused
        try:
            net.zero_grad(set_to_none=True)
            if amp:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out, _ = net(x)
                assert out[0].dtype == torch.bfloat16
            else:
                out, _ = net(x)
            o = out[0].float()
            o.square().mean().backward()
            grads = {k: p.grad.clone() for k, p in net.named_parameters()}
            assert all(g.dtype == torch.float32 for g in grads.values())
            return o.detach(), grads
        finally:
            ops.FUSED_GROUP_NORM_RELU = True

    base_o, base_g = run(False, True)
    torch_o, torch_g = run(True, False)

    def refuse(*a, **k):
        raise AssertionError("a GroupNorm+ReLU pair fell back to torch's group_norm")
    monkeypatch.setattr(torch.nn.functional, "group_norm", refuse)
    fused_o, fused_g = run(True, True)
    monkeypatch.undo()

    def dist(o, g):
        gmax = max(v.abs().max().item() for v in base_g.values())
        return ((o - base_o).abs().max().item() / base_o.abs().max().item(),
                max((g[k] - base_g[k]).abs().max().item() for k in base_g) / gmax)
    (fo, fg), (to, tg) = dist(fused_o, fused_g), dist(torch_o, torch_g)
    print("distance from fp32, outputs: kernels %.3g, torch autocast %.3g; gradients: kernels %.3g, torch autocast %.3g"
          % (fo, to, fg, tg))
    assert fo <= 2 * to + 1e-6 and fg <= 2 * tg + 1e-6
