"""The bf16 GroupNorm+ReLU pair without a GPU: the restatement's rounding against torch's, its fp64 forward and backward
against torch's fp64 group_norm + relu + autograd, the new unit's code-object resources, the host-side argument codes of
its two entries and the engine's `amp` option."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import gn_bf16_ref as ref
from gn_bf16_ref import SHAPES, bits, case, clear_seed

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("shr_group_norm_relu_bf16_fwd", "shr_group_norm_relu_bf16_bwd")


def _torch_bits(a32):
    return torch.from_numpy(a32).bfloat16().view(torch.int16).numpy().view(np.uint16)


def test_rounding_equals_torch():
    """2^16 patterns that hold every tie (lower half 0x8000 under an even and under an odd upper half) with their two
    neighbours, across all exponents; the largest finite fp32 and the values around the largest bf16; denormals; +-0,
    +-inf; NaNs (torch keeps a NaN a NaN, whichever: compared as NaN, everything else bit for bit)."""
    rs = np.random.RandomState(0)
    upper = rs.randint(0, 1 << 16, 1 << 14).astype(np.uint32)
    upper[:512] = np.arange(512, dtype=np.uint32) << 7                       # every exponent, even upper halves
    upper[512:1024] = (np.arange(512, dtype=np.uint32) << 7) | 1             # ... and odd ones
    sweep = np.concatenate([(upper << 16) | low for low in (0x7fff, 0x8000, 0x8001, rs.randint(0, 1 << 16))]).astype(np.uint32)
    assert sweep.size == 1 << 16
    ties = sweep[(sweep & 0xffff) == 0x8000]
    assert ((ties >> 16) & 1 == 0).any() and ((ties >> 16) & 1 == 1).any()
    special = np.array([0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0x7f7f7fff, 0x7f7f8000,      # largest finite, around bf16's
                        0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff, 0x807f8000,   # denormals
                        0x00000000, 0x80000000, 0x7f800000, 0xff800000], np.uint32)
    bits = np.concatenate([sweep, special])
    a = bits.view(np.float32)
    finite_or_inf = ~np.isnan(a)
    got, want = ref.bf16_round(a), _torch_bits(a)
    assert np.array_equal(got[finite_or_inf], want[finite_or_inf])
    assert np.isnan(ref.bf16_widen(got[~finite_or_inf])).all() and np.isnan(ref.bf16_widen(want[~finite_or_inf])).all()
    nans = np.array([0x7fc00000, 0x7f800001, 0xffc12345, 0x7f80ffff, 0xff800100], np.uint32).view(np.float32)
    assert np.isnan(ref.bf16_widen(ref.bf16_round(nans))).all() and np.isnan(ref.bf16_widen(_torch_bits(nans))).all()
    assert np.array_equal(ref.bf16_round(nans) >> 15, nans.view(np.uint32) >> 31)            # the sign stays
    assert ref.bf16_round(np.float32(3.4028235e38))[()] == 0x7f80 and ref.bf16_round(np.float32(np.inf))[()] == 0x7f80
    # widening inverts rounding on every bf16 value, and truncation is a different function
    every = np.arange(1 << 16, dtype=np.uint16)
    keep = ~np.isnan(ref.bf16_widen(every))
    assert np.array_equal(ref.bf16_round(ref.bf16_widen(every))[keep], every[keep])
    assert (ref.bf16_truncate(a[finite_or_inf]) != got[finite_or_inf]).mean() > 0.3


@pytest.mark.parametrize("with_pre", [False, True])
@pytest.mark.parametrize("N,C,H,W,G", SHAPES)
def test_reference_matches_torch_fp64(N, C, H, W, G, with_pre):
    seed = clear_seed(N, C, H, W, G, with_pre)
    assert seed is not None                        # every shape of the GPU test has a seed that clears the margin
    x, gamma, beta, pre, dy = case(N, C, H, W, G, seed, with_pre)
    r = ref.reference(bits(x), gamma.numpy(), beta.numpy(), G, 1e-5, None if pre is None else pre.numpy(), bits(dy))
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pd = None if pre is None else pre.double().requires_grad_(True)
    z = torch.nn.functional.group_norm(xd if pd is None else xd + pd.view(1, -1, 1, 1), G, gd, bd, 1e-5)
    y = torch.relu(z)
    (y * dy.double()).sum().backward()
    pairs = [(r["pre"], z.detach()), (r["y"], y.detach()), (r["dx"], xd.grad), (r["dgamma"], gd.grad), (r["dbeta"], bd.grad)]
    if pd is not None:
        pairs.append((r["dpre"], pd.grad))
    for mine, theirs in pairs:
        t = theirs.numpy()
        assert np.abs(mine - t).max() <= 1e-12 * max(1.0, np.abs(t).max())
    assert r["dx"].shape == (N, C, H, W) and r["mean"].shape == (N, G)


def test_a_truncating_store_misses_the_bound():
    """The reference's y stored by truncation instead of rounding: the GPU test's elementwise bound
    (2^-8 |ref| + 2 e32) refuses it and accepts the rounded one, so a kernel that truncates cannot pass there."""
    N, C, H, W, G = SHAPES[0]
    x, gamma, beta, pre, dy = case(N, C, H, W, G, clear_seed(N, C, H, W, G, False), False)
    r = ref.reference(bits(x), gamma.numpy(), beta.numpy(), G, 1e-5)
    y32 = r["y"].astype(np.float32)
    bar = 2.0 ** -8 * np.abs(r["y"]) + 2 * 2e-6 * max(1.0, np.abs(r["y"]).max())
    assert (np.abs(ref.bf16_widen(ref.bf16_round(y32)).astype(np.float64) - r["y"]) <= bar).all()
    assert (np.abs(ref.bf16_widen(ref.bf16_truncate(y32)).astype(np.float64) - r["y"]) > bar).any()


def test_header_loader_library_and_argument_codes():
    from spherehand_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spherehand_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert _lib.SIGNATURES[ENTRIES[0]] == _lib.SIGNATURES["shr_group_norm_relu_fwd"]
    assert _lib.SIGNATURES[ENTRIES[1]] == _lib.SIGNATURES["shr_group_norm_relu_bwd"]
    lib = _lib.lib()
    fwd, bwd = lib.shr_group_norm_relu_bf16_fwd, lib.shr_group_norm_relu_bf16_bwd
    p = 4096                                       # an aligned non-NULL address (no call below reaches a launch)
    # forward: x, pre_bias, gamma, beta, N, C, HW, G, eps, y, mean, rstd, stream
    assert fwd(None, None, None, None, 0, 64, 64, 16, 1e-5, None, None, None, None) == 0          # N == 0: a no-op
    for k in (0, 2, 3, 9, 10, 11):                                                                    # NULL
        a = [p, p, p, p, 2, 64, 64, 16, 1e-5, p, p, p, None]
        a[k] = None
        assert fwd(*a) == -1, k
    assert fwd(p, None, p, p, -1, 64, 64, 16, 1e-5, p, p, p, None) == -1
    assert fwd(p, None, p, p, 2, 64, 0, 16, 1e-5, p, p, p, None) == -1
    for C, G in ((48, 4), (64, 32), (64, 1), (64, 0), (0, 4), (64, 6)):                              # outside gn_supported
        assert lib.shr_group_norm_relu_supported(C, G) == 0
        assert fwd(p, None, p, p, 2, C, 64, G, 1e-5, p, p, p, None) == -1, (C, G)
    for k in (0, 1, 2, 3, 9):                                                                         # off 16 bytes
        a = [p, p, p, p, 2, 64, 64, 16, 1e-5, p, p, p, None]
        a[k] = p + 8
        assert fwd(*a) == -1, k
    assert fwd(p, None, p, p, 65536, 64, 64, 16, 1e-5, p, p, p, None) == -2
    # backward: x, pre_bias, dy, gamma, beta, mean, rstd, N, C, HW, G, dx, dg_part, db_part, dp_part, dgamma, dbeta, dpre, stream
    ok = [p, p, p, p, p, p, p, 2, 64, 64, 16, p, p, p, p, None, None, None, None]
    assert bwd(*([None] * 7 + [0, 64, 64, 16] + [None] * 8)) == 0
    for k in (0, 2, 3, 4, 5, 6, 11, 12, 13):
        a = list(ok)
        a[k] = None
        assert bwd(*a) == -1, k
    for k in (0, 1, 2, 3, 4, 11, 12, 13, 14):
        a = list(ok)
        a[k] = p + 8
        assert bwd(*a) == -1, k
    a = list(ok); a[1] = None                       # pre_bias and dpre_partial come together
    assert bwd(*a) == -1
    a = list(ok); a[14] = None
    assert bwd(*a) == -1
    a = list(ok); a[8] = 48
    assert bwd(*a) == -1
    a = list(ok); a[7] = 65536
    assert bwd(*a) == -2


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_dist_transform_cpu.py's reading of the code-object metadata: the two kernels of
    group_norm_relu_bf16.hip report ScratchSize 0 and no spills; every access to an activation is 16 bytes wide."""
    from spherehand_amd import build
    out = str(tmp_path / "group_norm_relu_bf16.s")
    src = os.path.join(build.PKG, "csrc", "group_norm_relu_bf16.hip")
    assert src in build.sources()
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(s) for s in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == 2 and max(sizes) == 0, sizes
    meta = text[text.index("amdhsa.kernels:"):]
    names = re.findall(r"\.name:\s+(\S+)", meta)
    for kernel in ("group_norm_relu_bf16_fwd_kernel", "group_norm_relu_bf16_bwd_kernel"):
        assert len([n for n in names if kernel in n]) == 1, names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        vals = [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % key, meta)]
        assert len(vals) == 2 and max(vals) == 0, (key, vals)
    stores = re.findall(r"global_store_(\w+)", text)
    assert stores.count("dwordx4") >= 2 and "short" not in stores and "dwordx2" not in stores, stores
    # the fp32 unit's kernels are untouched and the parameter-gradient kernel exists once, there
    assert "group_norm_param_grad_kernel" not in text


def test_engine_refuses_an_unknown_amp_value(tmp_path):
    from spherehand_amd.engine import Engine
    o = SimpleNamespace(amp='fp16', model_dir=str(tmp_path))
    with pytest.raises(ValueError):
        Engine(o)
    from spherehand_amd.criterion import HeatmapEstimationNetwork
    with pytest.raises(ValueError):
        HeatmapEstimationNetwork(16, 0.01, 41, 1, amp_dtype=torch.float16)
    from spherehand_amd.run_engine import build_parser
    assert build_parser().parse_args([]).amp is None and build_parser().parse_args(["--amp", "bf16"]).amp == "bf16"
