"""Tensor-level entry points over the C ABI (device memory + stream plumbing only).

Every function takes CUDA(HIP) fp32 contiguous tensors, allocates its outputs
with torch, and enqueues the hand-written HIP kernels on torch's CURRENT stream.
Preconditions mirror the reference extension's CHECK_INPUT
(mesh/cuda_kernel/depth_rasterization_cuda.cpp:11-19): a violation raises
RuntimeError.
"""
import numpy as np
import torch

from . import _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


# (device index) -> hipStream_t of torch's current stream, and the current device index.  The two private accessors
# are 13 us per call cheaper than the public spelling (see _stream); a torch build without them (CPU-only wheels, a
# rename) falls back to the public one -- importing this module never fails for that.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda d: torch.cuda.current_stream(d).cuda_stream)
_cur_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def _stream():
    """torch's current HIP stream on the current device, as the integer the C ABI takes.  (The public spelling
    torch.cuda.current_stream().cuda_stream builds a Stream object through three Python layers: 13 us per call, six
    calls per pose -> depth -> pose iteration -- a third of its eager time, tools/prof_eager.py.)"""
    return _raw_stream(_cur_device())


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device):
    """Device guard for the launches below: a no-op when `device` is already current (one process
    per GPU: always), torch.cuda.device(...) otherwise."""
    if device.index is None or device.index == _cur_device():
        return _NO_SWITCH
    return torch.cuda.device(device)


def _check_input(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s" % (name, dtype))


RASTER_OWNER_TOUCHED_ROWS = 1   # shr_sphere_raster_fwd_ex flag (include/spherehand_hip.h)


def sphere_raster_fwd(spheres, H, W, want_argmin=False, flags=0):
    """spheres [N,J,4] (x,y,z,r) -> depth [N,H,W] (and uint8 argmin [N,H,W]).  flags = RASTER_OWNER_TOUCHED_ROWS:
    the owner bytes of rows no sphere touches stay unwritten (all sphere_raster_bwd needs)."""
    _check_input(spheres, "spheres")
    if spheres.dim() != 3 or spheres.shape[2] != 4:
        raise RuntimeError("spheres must be [N,J,4]")
    N, J, _ = spheres.shape
    with _on(spheres.device):
        depth = torch.empty((N, H, W), dtype=torch.float32, device=spheres.device)
        arg = torch.empty((N, H, W), dtype=torch.uint8, device=spheres.device) if want_argmin else None
        _lib.check(_lib.lib().shr_sphere_raster_fwd_ex(_ptr(spheres), N, J, H, W, _ptr(depth), _ptr(arg), int(flags),
                                                       _stream()), "shr_sphere_raster_fwd")
    return (depth, arg) if want_argmin else depth


def sphere_raster_bwd(spheres, grad_depth, argmin=None):
    """grad_depth [N,H,W] (+ the forward's uint8 owner map, or None to recompute
    the owners) -> grad_spheres [N,J,4]."""
    _check_input(spheres, "spheres")
    _check_input(grad_depth, "grad_depth")
    N, J, _ = spheres.shape
    if grad_depth.dim() != 3 or grad_depth.shape[0] != N:
        raise RuntimeError("grad_depth must be [N,H,W]")
    H, W = grad_depth.shape[1], grad_depth.shape[2]
    if argmin is not None:
        _check_input(argmin, "argmin", torch.uint8)
        if argmin.shape != grad_depth.shape:
            raise RuntimeError("argmin must be [N,H,W]")
    with _on(spheres.device):
        out = torch.empty((N, J, 4), dtype=torch.float32, device=spheres.device)
        _lib.check(_lib.lib().shr_sphere_raster_bwd(_ptr(spheres), _ptr(grad_depth), _ptr(argmin), N, J, H, W,
                                                    _ptr(out), _stream()), "shr_sphere_raster_bwd")
    return out


TUNE_FWD_LDS_BYTES, TUNE_FWD_OWNER_LDS_BYTES, TUNE_BWD_LDS_BYTES, TUNE_FORCE_GENERAL, TUNE_FWD_WAVES = 1, 2, 3, 4, 5
TUNE_FWD_SHARES, TUNE_BWD_SHARES, TUNE_D2M_WAVES, TUNE_D2M_BAND_UNITS, TUNE_PERSISTENT, TUNE_FWD_ZBUF_BYTES = 6, 7, 8, 9, 10, 11
TUNE_BWD_WAVES, TUNE_MSE_BOX, TUNE_FWD_RUN_TABLE, TUNE_D2M_TILED, TUNE_TRI_BAND, TUNE_MESH_BAND = 12, 13, 14, 15, 16, 17
TUNE_MESH_LATTICE = 18


def set_tuning(key, value):
    """Launch-shape / test hook (shr_set_tuning); never changes results."""
    _lib.check(_lib.lib().shr_set_tuning(int(key), int(value)), "shr_set_tuning")


class SphereDepthRaster(torch.autograd.Function):
    """depth[N,H,W] = min over the J spheres of a crop (SURVEY 8b "new
    differentiable op").  Differentiable w.r.t. spheres[N,J,4] = (x,y,z,r).
    The forward saves its uint8 owner map (1 byte/pixel) for the backward -- written on the rows the backward
    will look at only (RASTER_OWNER_TOUCHED_ROWS: the map never leaves this Function)."""

    @staticmethod
    def forward(ctx, spheres, H, W):
        spheres = spheres.contiguous()
        if ctx.needs_input_grad[0]:
            depth, owner = sphere_raster_fwd(spheres, H, W, want_argmin=True, flags=RASTER_OWNER_TOUCHED_ROWS)
            ctx.save_for_backward(spheres, owner)
        else:
            depth = sphere_raster_fwd(spheres, H, W)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        spheres, owner = ctx.saved_tensors
        return sphere_raster_bwd(spheres, grad_depth.contiguous(), owner), None, None


def _check_index(index, n, m, name):
    if index.dtype != torch.int32 or index.dim() != 1 or index.numel() != n or not index.is_cuda or not index.is_contiguous():
        raise RuntimeError("%s must be a contiguous int32 CUDA tensor with one entry per crop" % name)
    # PRECONDITION (not checked here -- reading the values back would synchronise the stream): every entry is an
    # image number in [0, m).  The kernels index the image stack with it unchecked; MutualProjectionLoss builds
    # and caches its index tensors once per (B, V, device), in range by construction.


def sphere_raster_mse_supported(spheres, target, H, W):
    """True when shr_sphere_raster_mse takes these buffers (16-byte rows, image fits the kernel)."""
    return (W % 4 == 0 and spheres.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 0
            and _lib.lib().shr_sphere_raster_mse_regions(int(H), int(W)) > 0)


def sphere_raster_mse(spheres, target, target_index=None, want_depth=True):
    """spheres [N,J,4], target [M,H,W] (crop n compares with image target_index[n], or n)
    -> (depth [N,H,W] or None, sse [N], grad_spheres [N,J,4]) with sse[n] = sum over the
    crop of (depth - target)^2 and grad_spheres = d sse[n] / d (x,y,z,r): the fused
    render-and-compare kernel, no owner map / gradient image in HBM."""
    _check_input(spheres, "spheres")
    _check_input(target, "target")
    if spheres.dim() != 3 or spheres.shape[2] != 4 or target.dim() != 3:
        raise RuntimeError("spheres must be [N,J,4] and target [M,H,W]")
    N, J, _ = spheres.shape
    H, W = target.shape[1:]
    if target_index is None and target.shape[0] != N:
        raise RuntimeError("target must hold one image per crop unless target_index is given")
    if target_index is not None:
        _check_index(target_index, N, target.shape[0], "target_index")
    R = _lib.lib().shr_sphere_raster_mse_regions(int(H), int(W))
    if R <= 0:
        raise RuntimeError("image rows too wide for the fused kernel (compose sphere_raster_fwd / _bwd)")
    with _on(spheres.device):
        depth = torch.empty((N, H, W), dtype=torch.float32, device=spheres.device) if want_depth else None
        sse = torch.empty((N, R), dtype=torch.float32, device=spheres.device)
        grad = torch.empty((N, R, J, 4), dtype=torch.float32, device=spheres.device)
        _lib.check(_lib.lib().shr_sphere_raster_mse(_ptr(spheres), N, J, H, W, _ptr(target), _ptr(target_index),
                                                    _ptr(depth), _ptr(sse), _ptr(grad), _stream()),
                   "shr_sphere_raster_mse")
        if R > 1:
            sse, grad = sse.sum(1), grad.sum(1)
        else:
            sse, grad = sse.view(N), grad.view(N, J, 4)
    return depth, sse, grad


class SphereRasterSSE(torch.autograd.Function):
    """(spheres [N,J,4], target [M,H,W], target_index [N] int32 or None) -> (sse [N], depth
    [N,H,W]): per-crop sum of squared differences between the rendered spheres and an
    observed depth image, with the rendered depth as a second, non-differentiable output.
    The backward only scales the gradient the fused kernel already produced."""

    @staticmethod
    def forward(ctx, spheres, target, target_index=None):
        spheres = spheres.contiguous()
        depth, sse, grad = sphere_raster_mse(spheres, target.contiguous(), target_index)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(depth)
        ctx.set_materialize_grads(False)    # no zero image for the depth output's "gradient"
        return sse, depth

    @staticmethod
    def backward(ctx, grad_sse, _grad_depth):
        (grad,) = ctx.saved_tensors
        if grad_sse is None:
            return None, None, None
        return grad * grad_sse.view(-1, 1, 1), None, None


D2M_TWO_STEP = True   # data->model: compact the images once + search the point lists (False: the streaming kernel)


def data_to_model(depth, centres, radii, want_grad=False, depth_index=None):
    """depth [N,H,W], centres [N,J,3], radii [J] -> loss_sum [N] (and the unit
    gradient d loss_sum[n]/d centres [N,J,3]).  With depth_index [N] int32, depth is
    [M,H,W] and crop n reads image depth_index[n].
    Two paths by stack size (d2m_two_step_pays): the two-step path returns ONE integer sum per crop; the streaming
    kernel returns R = shr_data_to_model_parts partial sums per crop (R = 2 from 192x192 pixels on), each an exact
    integer sum, ADDED here in fp32.  The two agree bit for bit where R = 1 and to one fp32 rounding of the crop's
    total where R = 2 -- a crop's value may move by that rounding with the batch size that selects the path."""
    _check_input(depth, "depth")
    _check_input(centres, "centres")
    _check_input(radii, "radii")
    if depth.dim() != 3 or centres.dim() != 3 or centres.shape[2] != 3:
        raise RuntimeError("depth must be [N,H,W] and centres [N,J,3]")
    if depth_index is None and centres.shape[0] != depth.shape[0]:
        raise RuntimeError("depth must be [N,H,W] and centres [N,J,3]")
    N, (H, W) = centres.shape[0], depth.shape[1:]
    J = centres.shape[1]
    if radii.numel() != J:
        raise RuntimeError("radii must have J entries")
    if depth_index is not None:
        _check_index(depth_index, N, depth.shape[0], "depth_index")
    if N > 0 and d2m_two_step_pays(depth, shared=depth_index is not None and N >= 2 * depth.shape[0]):
        # compact every image once, search the point lists (the same integer sums, see csrc/data_to_model.hip)
        ws = d2m_compact(depth)
        return data_to_model_from_points(ws, depth.shape[0], H, W, centres, radii, depth_index, want_grad)
    lib = _lib.lib()
    R = lib.shr_data_to_model_parts(N, int(H), int(W))     # large crops: R partial results per crop, added here
    with _on(depth.device):
        loss_sum = torch.empty((N, R), dtype=torch.float32, device=depth.device)
        grad = torch.empty((N, R, J, 3), dtype=torch.float32, device=depth.device) if want_grad else None
        _lib.check(lib.shr_data_to_model_partial(_ptr(depth), _ptr(depth_index), _ptr(centres), 3, _ptr(radii), N, J, H, W, R,
                                                 _ptr(loss_sum), _ptr(grad), _stream()), "shr_data_to_model_partial")
        if R > 1:
            loss_sum = loss_sum.sum(1)
            grad = grad.sum(1) if want_grad else None
        else:
            loss_sum = loss_sum.view(N)
            grad = grad.view(N, J, 3) if want_grad else None
    return (loss_sum, grad) if want_grad else loss_sum


D2M_TWO_STEP_MIN_PIXELS = 1 << 23   # (384 images @128x128 = 6.3 M pixels: the two paths tie there -- 52 vs 55 us at 1152 crops)


def d2m_points_supported(depth):
    """True when the two-step data->model path takes this image stack [M,H,W] (16-byte rows, at most 2^28 pixels)."""
    return depth.dim() == 3 and depth.shape[0] > 0 and depth.data_ptr() % 16 == 0 and \
        _lib.lib().shr_data_to_model_points_bytes(int(depth.shape[0]), int(depth.shape[1]), int(depth.shape[2])) > 0


def d2m_two_step_pays(depth, shared=False):
    """The two-step path costs a launch more than the streaming kernel and wins where the streaming kernel is bound by
    its VALU work (large images compared with several sphere sets); small stacks stay with one launch.  shared: the
    stand-alone term with every image searched by at least two crops -- the compaction is paid once per image, the
    search per crop: from half the size on (1152 crops on 384 images @128x128: 46 against 56 us; the fused loss, which
    has other launches to feed, gains nothing there and keeps the full threshold)."""
    least = D2M_TWO_STEP_MIN_PIXELS // 2 if shared else D2M_TWO_STEP_MIN_PIXELS
    return D2M_TWO_STEP and depth.numel() >= least and d2m_points_supported(depth)


MV_OVERLAP = True        # MutualProjectionLossFused: render-and-compare beside the point search (see there)
SAME_VIEW_SPLIT = True   # ... and, for the same-view pairs only, the compare on those pairs alone (see there)
# The side stream and its 'projection done' event are kept per (device, caller's stream): two callers on different
# streams of one device (two training loops in one process) get a side stream and an event each, so neither orders the
# other's work.  One caller stream = one pair, reused call after call (creating them costs ~20 us).
_SIDE = {}


def _side_key(dev):
    d = dev.index if dev.index is not None else _cur_device()
    return (d, _raw_stream(d))


def _side_stream(dev):
    k = _side_key(dev)
    if k not in _SIDE:
        _SIDE[k] = torch.cuda.Stream(device=dev)
    return _SIDE[k]


_SIDE_EVENT = {}


def _side_event(dev):
    """One reusable event per (device, caller's stream) for the 'projection done' edge between the two streams."""
    k = _side_key(dev)
    if k not in _SIDE_EVENT:
        _SIDE_EVENT[k] = torch.cuda.Event()
    return _SIDE_EVENT[k]


def d2m_points_workspace(depth):
    """An UNFILLED workspace (uint8 tensor) for the point lists of depth [M,H,W] (shr_data_to_model_points_bytes)."""
    _check_input(depth, "depth")
    M, H, W = depth.shape
    nbytes = _lib.lib().shr_data_to_model_points_bytes(int(M), int(H), int(W))
    if nbytes <= 0 or depth.data_ptr() % 16:
        raise RuntimeError("image not taken by the two-step data->model path (rows of 4 pixels, 16-byte aligned)")
    with _on(depth.device):
        return torch.empty(nbytes, dtype=torch.uint8, device=depth.device)


def d2m_compact(depth):
    """depth [M,H,W] -> workspace (uint8 tensor): every image's foreground pixels as tile-sorted point records, for
    data_to_model_from_points (shr_data_to_model_compact)."""
    ws = d2m_points_workspace(depth)
    M, H, W = depth.shape
    with _on(depth.device):
        _lib.check(_lib.lib().shr_data_to_model_compact(_ptr(depth), M, H, W, _ptr(ws), _stream()), "shr_data_to_model_compact")
    return ws


def d2m_points_parts(N):
    """Partial results per crop of the point-list search: ONE.  The regions of an image enter its list in the order
    their workgroups arrive, so the groups a part would own change from run to run; a crop's total is an integer sum
    over all its points and does not (bit-reproducible), several float partials added afterwards would only be equal
    to a rounding.  The launcher gives a crop's workgroup more waves when there are few crops."""
    return 1


def data_to_model_from_points(ws, M, H, W, centres, radii, depth_index=None, want_grad=False, centre_stride=None, parts=None):
    """The search step: centres [N,J,3] (or the rasterizer's [N,J,4] records with centre_stride=4) against the point
    lists of images depth_index[n] (or n) -> loss_sum [N] (and grad_centres [N,J,3])."""
    N, J = centres.shape[0], centres.shape[1]
    stride = int(centres.shape[2]) if centre_stride is None else centre_stride
    P = d2m_points_parts(N) if parts is None else parts
    lib = _lib.lib()
    with _on(centres.device):
        loss = torch.empty((N, P), dtype=torch.float32, device=centres.device)
        grad = torch.empty((N, P, J, 3), dtype=torch.float32, device=centres.device) if want_grad else None
        _lib.check(lib.shr_data_to_model_from_points(_ptr(ws), int(M), _ptr(depth_index), _ptr(centres), stride, _ptr(radii), N, J,
                                                     int(H), int(W), P, _ptr(loss), _ptr(grad), _stream()),
                   "shr_data_to_model_from_points")
        if P > 1:
            loss = loss.sum(1)
            grad = grad.sum(1) if want_grad else None
        else:
            loss = loss.view(N)
            grad = grad.view(N, J, 3) if want_grad else None
    return (loss, grad) if want_grad else loss


class DataToModel(torch.autograd.Function):
    """mean over ALL N*H*W pixels of the clamped point-to-sphere-surface distance
    (mesh/render.py:123-142).  The kernel emits the unit gradient with the loss;
    backward only scales it."""

    @staticmethod
    def forward(ctx, depth, centres, radii, depth_index=None):
        depth = depth.contiguous()
        centres = centres.contiguous()
        count = float(centres.shape[0] * depth.shape[-2] * depth.shape[-1])   # pixels of the N crops
        if ctx.needs_input_grad[1]:
            loss_sum, grad = data_to_model(depth, centres, radii, want_grad=True, depth_index=depth_index)
            ctx.save_for_backward(grad)
            ctx.count = count
        else:
            loss_sum = data_to_model(depth, centres, radii, depth_index=depth_index)
        return (loss_sum.double().sum() / count).float()

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return None, grad * (grad_out / ctx.count), None, None


class MutualProjectionLossFused(torch.autograd.Function):
    """(cam, inv_cam [B,V,4,4], joints [B,V,J,3], observed [B*V,H,W], radii [J], index [B*V*V] int32 (pair -> observed
    image), diag_index [B*V] int32 (the same-view pairs' numbers), is_mv, ..., diag_target [B*V] int32 = index[diag_index]) ->
    (loss, projected depth [B*V*V,H,W]): MutualProjectionLoss (mesh/multiview_utility.py:90-130) as FIVE launches
    -- view projection, (compaction of the observed images into point lists,) fused render-and-compare, data->model,
    and the assembly kernel that weights, adds and pulls both sphere gradients back to the joints (the whole backward
    is done in the forward: the losses are plain sums) -- plus one scaling in backward.  The unfused wiring needed
    ~35 small torch launches around the same three kernels.
    points_ws: a point-list workspace of these very observed images (d2m_points_workspace); points_fresh = it is
    still to be filled (done here, by the call that also projects the views: shr_mv_project_compact)."""

    @staticmethod
    def forward(ctx, cam, inv_cam, joints, observed, radii, index, diag_index, is_mv, d2m_weight, points_ws=None,
                points_fresh=False, diag_target=None, want_depth=True, order=None, order_target=None):
        cam, inv_cam, joints = (t.detach().contiguous().float() for t in (cam, inv_cam, joints))
        observed, radii = observed.contiguous().float(), radii.contiguous().float()
        for t, name in ((cam, "camera_poses"), (inv_cam, "inv_camera_poses"), (joints, "joints"), (observed, "depth_maps"),
                        (radii, "radii")):
            _check_input(t, name)
        B, V, J = joints.shape[0], joints.shape[1], joints.shape[2]
        H, W = observed.shape[-2], observed.shape[-1]
        N = B * V * V
        lib = _lib.lib()
        if diag_index.dtype != torch.int32:
            diag_index = diag_index.to(torch.int32)
        if diag_target is None and not is_mv:
            diag_target = index.index_select(0, diag_index.long())
        Rm = lib.shr_sphere_raster_mse_regions(int(H), int(W))
        dev = joints.device
        if N == 0 or J == 0:     # (the entry points return at once on an empty batch: nothing would write the outputs)
            if ctx.needs_input_grad[2]:
                ctx.save_for_backward(torch.zeros((B, V, J, 3), dtype=torch.float32, device=dev))
            depth = torch.full((N, H, W), 100.0, dtype=torch.float32, device=dev)
            ctx.mark_non_differentiable(depth)
            ctx.set_materialize_grads(False)
            return torch.zeros((), dtype=torch.float32, device=dev), depth
        # every observed image is compared with V sphere sets (mesh/multiview_utility.py:99): compacted once into a
        # point list (points_ws: the caller's -- MutualProjectionLoss keeps the lists while it is handed the same
        # observations again: a second hourglass stack, a fitting loop)
        two_step = points_ws is not None or d2m_two_step_pays(observed)
        if two_step and points_ws is None:
            points_ws, points_fresh = d2m_points_workspace(observed), True
        with _on(dev):
            spheres = torch.empty((N, J, 4), dtype=torch.float32, device=dev)
            # want_depth = False (MutualProjectionLoss.return_projections off: a training loop that never looks at the
            # projections): the fused kernel writes no depth map -- half of its HBM bytes -- and the same-view mode
            # launches no plain forward at all; an empty tensor stands in for the projections.
            depth = torch.empty((N, H, W) if want_depth else (0, H, W), dtype=torch.float32, device=dev)
            dptr = _ptr(depth) if want_depth else None
            # Two streams where the stack is large enough for the two-step path (MV_OVERLAP; same bits either way):
            #   caller's stream   view projection -> render-and-compare (the LONG kernel: nothing it waits for crosses
            #                     a queue) [-> the plain forward of all pairs in the same-view split]
            #   side stream       compaction of the observed images (needs nothing from this call) -> [projection
            #                     done] -> point search
            # Round 4 had projection + compaction on the caller's stream and the render-and-compare kernel on the
            # side: it started 12 us after the compaction's end (cross-queue dependency) and the join cost another 11
            # on the critical path (rocprofv3 timeline, tools/timeline_mvloss.sh).
            overlap = MV_OVERLAP and two_step
            main = side = None
            s_main = _stream()
            s_d2m = s_main
            if overlap:
                main, side = torch.cuda.current_stream(dev), _side_stream(dev)
                side.wait_stream(main)
                s_d2m = side.cuda_stream
            if two_step and points_fresh and not overlap:
                _lib.check(lib.shr_mv_project_compact(_ptr(cam), _ptr(inv_cam), _ptr(joints), _ptr(radii), B, V, J,
                                                      _ptr(spheres), _ptr(observed), int(observed.shape[0]), H, W,
                                                      _ptr(points_ws), s_main), "shr_mv_project_compact")
            else:
                if two_step and points_fresh:
                    _lib.check(lib.shr_data_to_model_compact(_ptr(observed), int(observed.shape[0]), H, W, _ptr(points_ws), s_d2m),
                               "shr_data_to_model_compact")
                _lib.check(lib.shr_mutual_project_fwd(_ptr(cam), _ptr(inv_cam), _ptr(joints), _ptr(radii), B, V, J,
                                                      _ptr(spheres), s_main), "shr_mutual_project_fwd")
            if overlap:
                ev = _side_event(dev)
                ev.record(main)
                side.wait_event(ev)               # the point search reads the projected records
            # Same-view pairs only (what the reference trains with after its first 1500 iterations,
            # network/engine.py:361): E = B*V pairs enter the loss, all V*V projections are still returned.  The pairs
            # are SELECTED by index inside the kernels (diag_index: pair e = crop diag_index[e] of the batch; diag_target:
            # its observed image) -- no gather of their records in front (two torch launches and 16 us until round 4).
            if is_mv:
                E, cidx, cen_index = N, index, None
            else:
                E, cidx, cen_index = B * V, diag_target, diag_index
            # On a large stack the compare runs on those pairs alone (no depth output) and the plain forward kernel
            # renders all N projections behind it (SAME_VIEW_SPLIT).
            split = (overlap or not want_depth) and not is_mv and SAME_VIEW_SPLIT
            Em = E if split else N
            # the partial results of the two terms: ONE allocation, addressed by offsets (four torch.empty calls and
            # their tensors were ~10 us of host time per step)
            Rd = d2m_points_parts(E) if two_step else lib.shr_data_to_model_parts(E, int(H), int(W))
            n_gsp, n_gd2m, n_sse, n_d2m = Em * Rm * J * 4, E * Rd * J * 3, Em * Rm, E * Rd
            scratch = torch.empty(n_gsp + n_gd2m + n_sse + n_d2m, dtype=torch.float32, device=dev)
            loss = torch.empty(1, dtype=torch.float32, device=dev)    # (its own: the result must not pin the scratch)
            p_gsp = scratch.data_ptr()                          # (16-byte aligned: the allocation's start)
            p_gd2m = p_gsp + 4 * n_gsp
            p_sse = p_gd2m + 4 * n_gd2m
            p_d2m = p_sse + 4 * n_sse
            if split:
                _lib.check(lib.shr_sphere_raster_mse_indexed(_ptr(spheres), _ptr(diag_index), E, J, H, W, _ptr(observed),
                                                             _ptr(index), None, p_sse, p_gsp, s_main),
                           "shr_sphere_raster_mse_indexed")
                if want_depth:
                    _lib.check(lib.shr_sphere_raster_fwd_ex(_ptr(spheres), N, J, H, W, dptr, None, 0, s_main),
                               "shr_sphere_raster_fwd_ex")
            elif is_mv and order is not None:
                # all pairs, in the XCD-aware launch order (multiview_utility._indices): the same slots, the same bits
                _lib.check(lib.shr_sphere_raster_mse_ordered(_ptr(spheres), _ptr(order), N, J, H, W, _ptr(observed), _ptr(index),
                                                             dptr, p_sse, p_gsp, s_main), "shr_sphere_raster_mse_ordered")
            else:
                _lib.check(lib.shr_sphere_raster_mse(_ptr(spheres), N, J, H, W, _ptr(observed), _ptr(index), dptr,
                                                     p_sse, p_gsp, s_main), "shr_sphere_raster_mse")
            if two_step:
                ws = points_ws
                # (ordered: workgroup = crop; with several parts per crop blockIdx.x = crop * parts + part and the XCD
                # placement the order was built for no longer holds -- the batch's own order then)
                if is_mv and order is not None and Rd == 1:
                    _lib.check(lib.shr_data_to_model_from_points_ordered(_ptr(ws), int(observed.shape[0]), _ptr(order_target),
                                                                         _ptr(order), _ptr(spheres), 4, _ptr(radii), E, J, H, W,
                                                                         Rd, p_d2m, p_gd2m, s_d2m), "shr_data_to_model_from_points_ordered")
                else:
                    _lib.check(lib.shr_data_to_model_from_points_indexed(_ptr(ws), int(observed.shape[0]), _ptr(cidx), _ptr(cen_index),
                                                                         _ptr(spheres), 4, _ptr(radii), E, J, H, W, Rd, p_d2m,
                                                                         p_gd2m, s_d2m), "shr_data_to_model_from_points")
                if overlap:
                    # the join: everything the side stream wrote into `scratch` / read from `spheres` is ordered before
                    # the assembly kernel on the caller's stream -- and before the caching allocator can hand either
                    # block to a later allocation of that stream (which is why no record_stream() is needed)
                    main.wait_stream(side)
            else:
                cen = spheres if is_mv else spheres.index_select(0, diag_index.long())
                _lib.check(lib.shr_data_to_model_partial(_ptr(observed), _ptr(cidx), _ptr(cen), 4, _ptr(radii), E, J, H, W, Rd,
                                                         p_d2m, p_gd2m, s_main), "shr_data_to_model_partial")
            want = ctx.needs_input_grad[2]
            gj = torch.empty((B, V, J, 3), dtype=torch.float32, device=dev) if want else None
            _lib.check(lib.shr_mv_loss_combine(_ptr(cam), _ptr(inv_cam), p_sse, p_gsp, Rm, p_d2m, p_gd2m, Rd,
                                               B, V, J, H, W, 1 if is_mv else (2 if split else 0), float(d2m_weight), _ptr(loss), _ptr(gj),
                                               _stream()), "shr_mv_loss_combine")
        if want:
            ctx.save_for_backward(gj)
        ctx.mark_non_differentiable(depth)
        ctx.set_materialize_grads(False)
        return loss.view(()), depth

    @staticmethod
    def backward(ctx, g_loss, _g_depth):
        if g_loss is None:
            return (None,) * 15
        (gj,) = ctx.saved_tensors
        return (None, None, gj * g_loss) + (None,) * 12


class MutualProject(torch.autograd.Function):
    """(cam, inv_cam [B,V,4,4], joints [B,V,J,3], radii [J]) -> spheres [B,V,V,J,4]:
    every view's joints expressed in every view (mesh/multiview_utility.py:13-30,
    :62-72).  Differentiable w.r.t. joints only (the transforms are detached in
    the reference, :68)."""

    @staticmethod
    def forward(ctx, cam, inv_cam, joints, radii):
        cam, inv_cam, joints, radii = (t.contiguous().float() for t in (cam, inv_cam, joints, radii))
        for t, name in ((cam, "camera_poses"), (inv_cam, "inv_camera_poses"), (joints, "joints"), (radii, "radii")):
            _check_input(t, name)
        B, V, J = joints.shape[0], joints.shape[1], joints.shape[2]
        if cam.shape != (B, V, 4, 4) or inv_cam.shape != (B, V, 4, 4) or joints.shape[3] != 3:
            raise RuntimeError("expected cam/inv_cam [B,V,4,4] and joints [B,V,J,3]")
        with _on(joints.device):
            out = torch.empty((B, V, V, J, 4), dtype=torch.float32, device=joints.device)
            _lib.check(_lib.lib().shr_mutual_project_fwd(_ptr(cam), _ptr(inv_cam), _ptr(joints), _ptr(radii), B, V, J,
                                                         _ptr(out), _stream()), "shr_mutual_project_fwd")
        ctx.save_for_backward(cam, inv_cam)
        return out

    @staticmethod
    def backward(ctx, grad_spheres):
        cam, inv_cam = ctx.saved_tensors
        g = grad_spheres.contiguous()
        B, V, _, J, _ = g.shape
        with _on(g.device):
            out = torch.empty((B, V, J, 3), dtype=torch.float32, device=g.device)
            _lib.check(_lib.lib().shr_mutual_project_bwd(_ptr(cam), _ptr(inv_cam), _ptr(g), B, V, J, _ptr(out),
                                                         _stream()), "shr_mutual_project_bwd")
        return None, None, out, None


def tri_raster_fwd(width, height, face_vertices):
    """face_vertices [B,F,3,3] (pixel-space x,y,z) -> depth [B,height,width],
    background 1000: depth_rasterization.forward (mesh/cuda_kernel)."""
    _check_input(face_vertices, "vertices")
    if face_vertices.dim() < 2:
        raise RuntimeError("vertices must be [B,F,3,3]")
    B, F = face_vertices.shape[0], face_vertices.shape[1]
    if face_vertices.numel() != B * F * 9:
        raise RuntimeError("vertices must hold 9 floats per face ([B,F,3,3])")
    with _on(face_vertices.device):
        depth = torch.empty((B, height, width), dtype=torch.float32, device=face_vertices.device)
        _lib.check(_lib.lib().shr_tri_raster_fwd(_ptr(face_vertices), B, F, width, height, _ptr(depth), _stream()),
                   "shr_tri_raster_fwd")
    return depth


def tri_raster_indexed_fwd(width, height, vertices, faces):
    """vertices [B,NV,4] + faces [F,3] int32 -> depth [B,height,width] (gather fused)."""
    _check_input(vertices, "vertices")
    _check_input(faces, "faces", torch.int32)
    if vertices.dim() != 3 or vertices.shape[2] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("vertices must be [B,NV,4] and faces [F,3]")
    B, NV = vertices.shape[0], vertices.shape[1]
    with _on(vertices.device):
        depth = torch.empty((B, height, width), dtype=torch.float32, device=vertices.device)
        _lib.check(_lib.lib().shr_tri_raster_indexed_fwd(_ptr(vertices), _ptr(faces), B, NV, faces.shape[0], width,
                                                         height, _ptr(depth), _stream()),
                   "shr_tri_raster_indexed_fwd")
    return depth


def lbs_project(T, skin_vertex_start, skin_bone, skin_wv, right_hand=True, camera=None, rand_f=None):
    """T [B,NB,4,4] -> skinned (and, with camera=(cx,cy,fx,fy), projected) vertices [B,NV,4]."""
    _check_input(T, "bone_transformations")
    _check_input(skin_vertex_start, "skin_vertex_start", torch.int32)
    _check_input(skin_bone, "skin_bone", torch.int32)
    _check_input(skin_wv, "skin_wv")
    if rand_f is not None:
        _check_input(rand_f, "rand_f")
    B, NB = T.shape[0], T.shape[1]
    NV = skin_vertex_start.numel() - 1
    cx, cy, fx, fy = camera if camera is not None else (0.0, 0.0, 1.0, 1.0)
    with _on(T.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=T.device)
        _lib.check(_lib.lib().shr_lbs_project(_ptr(T), B, NB, NV, _ptr(skin_vertex_start), _ptr(skin_bone),
                                              _ptr(skin_wv), int(bool(right_hand)), int(camera is not None),
                                              cx, cy, fx, fy, _ptr(rand_f), _ptr(out), _stream()), "shr_lbs_project")
    return out


class KeypointSpheres(torch.autograd.Function):
    """T[B,NB,4,4] -> the rasterizer's records spheres[B,J,4] = (+-p.x, p.y, p.z, radii[j]), p = T[bone[j]] @ wv[j]: the
    key-point skinning + cat of HandBallPrimitiveRender (mesh/render.py:65-88) as one launch per direction; gradient
    w.r.t. T (the radii are buffers in the reference).  Tables: pointTransformation.LinearBlendSkinning.kp_*."""

    @staticmethod
    def forward(ctx, T, bone, wv, radii, bone_start, bone_points, right_hand):
        T = T.contiguous().float()
        _check_input(T, "transformation matrices")
        if T.dim() != 4 or T.shape[2:] != (4, 4):
            raise RuntimeError("transformation matrices must be [B,NB,4,4]")
        B, NB, J = T.shape[0], T.shape[1], bone.shape[0]
        if bone_start.shape[0] != NB + 1 or wv.shape != (J, 4) or radii.numel() != J:
            raise RuntimeError("key-point tables do not match the bones")
        with _on(T.device):
            sph = torch.empty((B, J, 4), dtype=torch.float32, device=T.device)
            _lib.check(_lib.lib().shr_keypoint_spheres_fwd(_ptr(T), B, NB, J, _ptr(bone), _ptr(wv), _ptr(radii),
                                                           int(bool(right_hand)), _ptr(sph), _stream()),
                       "shr_keypoint_spheres_fwd")
        ctx.save_for_backward(wv, bone_start, bone_points)
        ctx.dims = (B, NB, J, int(bool(right_hand)))
        return sph

    @staticmethod
    def backward(ctx, grad_spheres):
        wv, bone_start, bone_points = ctx.saved_tensors
        B, NB, J, right = ctx.dims
        g = grad_spheres.contiguous().float()
        with _on(g.device):
            gT = torch.zeros((B, NB, 4, 4), dtype=torch.float32, device=g.device) if B == 0 else \
                torch.empty((B, NB, 4, 4), dtype=torch.float32, device=g.device)
            _lib.check(_lib.lib().shr_keypoint_spheres_bwd(_ptr(g), B, NB, J, _ptr(bone_start), _ptr(bone_points),
                                                           _ptr(wv), right, _ptr(gT), _stream()),
                       "shr_keypoint_spheres_bwd")
        return gT, None, None, None, None, None, None


class ForwardKinematics(torch.autograd.Function):
    """params [B,26] -> bone transforms [B,17,4,4] (mesh/kinematicsTransformation.py:169-177),
    analytic backward; offset / offset_inv [17,4,4] are constants."""

    @staticmethod
    def forward(ctx, params, offset, offset_inv):
        params = params.contiguous().float()
        for t, name in ((params, "parameters"), (offset, "offset"), (offset_inv, "offset_inv")):
            _check_input(t, name)
        if params.dim() != 2 or params.shape[1] != 26:
            raise RuntimeError("parameters must be [B,26]")
        B = params.shape[0]
        with _on(params.device):
            T = torch.empty((B, 17, 4, 4), dtype=torch.float32, device=params.device)
            _lib.check(_lib.lib().shr_fk_fwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), _ptr(T), _stream()),
                       "shr_fk_fwd")
        ctx.save_for_backward(params, offset, offset_inv)
        return T

    @staticmethod
    def backward(ctx, grad_T):
        params, offset, offset_inv = ctx.saved_tensors
        g = grad_T.contiguous().float()
        B = params.shape[0]
        with _on(params.device):
            out = torch.empty((B, 26), dtype=torch.float32, device=params.device)
            _lib.check(_lib.lib().shr_fk_bwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), _ptr(g), _ptr(out),
                                             _stream()), "shr_fk_bwd")
        return out, None, None


class PoseSpheres(torch.autograd.Function):
    """params [B,26] -> the rasterizer's records spheres [B,J,4]: ForwardKinematics followed by KeypointSpheres as ONE
    launch per direction (shr_pose_spheres_fwd / _bwd): the bone transforms stay in LDS.  The fit chain
    HandBallPrimitiveRender(HandTransformationMat(pose)) (mesh/render.py:81-88 over
    mesh/kinematicsTransformation.py:169-177); records and gradient are bit-identical to the two Functions chained."""

    @staticmethod
    def forward(ctx, params, offset, offset_inv, bone, wv, radii, bone_start, bone_points, right_hand):
        params = params.contiguous().float()
        for t, name in ((params, "parameters"), (offset, "offset"), (offset_inv, "offset_inv"), (wv, "key-points"),
                        (radii, "radii")):
            _check_input(t, name)
        if params.dim() != 2 or params.shape[1] != 26:
            raise RuntimeError("parameters must be [B,26]")
        B, J = params.shape[0], bone.shape[0]
        if bone_start.shape[0] != 18 or wv.shape != (J, 4) or radii.numel() != J:
            raise RuntimeError("key-point tables do not match the 17 bones")
        with _on(params.device):
            sph = torch.empty((B, J, 4), dtype=torch.float32, device=params.device)
            _lib.check(_lib.lib().shr_pose_spheres_fwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone), _ptr(wv),
                                                       _ptr(radii), int(bool(right_hand)), _ptr(sph), None, _stream()),
                       "shr_pose_spheres_fwd")
        ctx.save_for_backward(params, offset, offset_inv, wv, bone_start, bone_points)
        ctx.dims = (B, J, int(bool(right_hand)))
        return sph

    @staticmethod
    def backward(ctx, grad_spheres):
        params, offset, offset_inv, wv, bone_start, bone_points = ctx.saved_tensors
        B, J, right = ctx.dims
        g = grad_spheres.contiguous().float()
        with _on(g.device):
            out = torch.empty((B, 26), dtype=torch.float32, device=g.device)
            _lib.check(_lib.lib().shr_pose_spheres_bwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone_start),
                                                       _ptr(bone_points), _ptr(wv), right, _ptr(g), _ptr(out), _stream()),
                       "shr_pose_spheres_bwd")
        return out, None, None, None, None, None, None, None, None


class PoseDepthRaster(torch.autograd.Function):
    """params [B,26] -> depth [B,H,W]: PoseSpheres followed by SphereDepthRaster as ONE autograd node (two launches per
    direction; an eager fitting loop pays the Python / autograd cost of one Function instead of two).  Same kernels,
    same bits as the two Functions chained."""

    @staticmethod
    def forward(ctx, params, offset, offset_inv, bone, wv, radii, bone_start, bone_points, right_hand, H, W):
        params = params.contiguous().float()
        _check_input(params, "parameters")
        if params.dim() != 2 or params.shape[1] != 26:
            raise RuntimeError("parameters must be [B,26]")
        B, J = params.shape[0], bone.shape[0]
        if bone_start.shape[0] != 18 or wv.shape != (J, 4) or radii.numel() != J:
            raise RuntimeError("key-point tables do not match the 17 bones")
        lib, right = _lib.lib(), int(bool(right_hand))
        want = ctx.needs_input_grad[0]
        with _on(params.device):
            s = _stream()
            sph = torch.empty((B, J, 4), dtype=torch.float32, device=params.device)
            depth = torch.empty((B, H, W), dtype=torch.float32, device=params.device)
            owner = torch.empty((B, H, W), dtype=torch.uint8, device=params.device) if want else None
            _lib.check(lib.shr_pose_spheres_fwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone), _ptr(wv),
                                                _ptr(radii), right, _ptr(sph), None, s), "shr_pose_spheres_fwd")
            _lib.check(lib.shr_sphere_raster_fwd_ex(_ptr(sph), B, J, H, W, _ptr(depth), _ptr(owner),
                                                    RASTER_OWNER_TOUCHED_ROWS if want else 0, s), "shr_sphere_raster_fwd")
        if want:
            ctx.save_for_backward(params, offset, offset_inv, wv, bone_start, bone_points, sph, owner)
            ctx.dims = (B, J, right, H, W)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        params, offset, offset_inv, wv, bone_start, bone_points, sph, owner = ctx.saved_tensors
        B, J, right, H, W = ctx.dims
        g = grad_depth.contiguous()
        lib = _lib.lib()
        with _on(g.device):
            s = _stream()
            gs = torch.empty((B, J, 4), dtype=torch.float32, device=g.device)
            out = torch.empty((B, 26), dtype=torch.float32, device=g.device)
            _lib.check(lib.shr_sphere_raster_bwd(_ptr(sph), _ptr(g), _ptr(owner), B, J, H, W, _ptr(gs), s), "shr_sphere_raster_bwd")
            _lib.check(lib.shr_pose_spheres_bwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone_start),
                                                _ptr(bone_points), _ptr(wv), right, _ptr(gs), _ptr(out), s), "shr_pose_spheres_bwd")
        return (out,) + (None,) * 10


def mesh_depth_fwd(vertices, faces, out_size, src_size=640, clamp_max=100.0):
    """vertices [B,NV,4] (src_size pixel space) + faces [F,3] int32 -> depth [B,S,S]: triangle
    raster at src_size, clamp(max), bilinear resize to S, fused (only the sampled pixels)."""
    _check_input(vertices, "vertices")
    _check_input(faces, "faces", torch.int32)
    if vertices.dim() != 3 or vertices.shape[2] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("vertices must be [B,NV,4] and faces [F,3]")
    B, NV = vertices.shape[0], vertices.shape[1]
    with _on(vertices.device):
        depth = torch.empty((B, out_size, out_size), dtype=torch.float32, device=vertices.device)
        _lib.check(_lib.lib().shr_mesh_depth_fwd(_ptr(vertices), _ptr(faces), B, NV, faces.shape[0], src_size, out_size,
                                                 clamp_max, _ptr(depth), _stream()), "shr_mesh_depth_fwd")
    return depth


def mesh_render_fwd(T, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f, faces, out_size, src_size=640,
                    clamp_max=100.0):
    """DepthRender.forward as one call (shr_mesh_render_fwd): T [B,NB,4,4] -> depth [B,S,S].  One launch where the fused
    kernel applies (integer src_size / S, lattice <= 128 x 128); otherwise skinning and raster through a vertex workspace."""
    _check_input(T, "bone_transformations")
    _check_input(skin_vertex_start, "skin_vertex_start", torch.int32)
    _check_input(skin_bone, "skin_bone", torch.int32)
    _check_input(skin_wv, "skin_wv")
    _check_input(faces, "faces", torch.int32)
    if rand_f is not None:
        _check_input(rand_f, "rand_f")
    if T.dim() != 4 or T.shape[2:] != (4, 4) or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("T must be [B,NB,4,4] and faces [F,3]")
    B, NB = T.shape[0], T.shape[1]
    NV = skin_vertex_start.numel() - 1
    cx, cy, fx, fy = camera
    with _on(T.device):
        depth = torch.empty((B, out_size, out_size), dtype=torch.float32, device=T.device)
        ws = torch.empty((B, NV, 4), dtype=torch.float32, device=T.device)     # (the caching allocator: no launch; unused
        #                                                                         when the fused kernel takes the call)
        _lib.check(_lib.lib().shr_mesh_render_fwd(_ptr(T), B, NB, NV, _ptr(skin_vertex_start), _ptr(skin_bone), _ptr(skin_wv),
                                                  int(bool(right_hand)), cx, cy, fx, fy, _ptr(rand_f), _ptr(faces),
                                                  faces.shape[0], src_size, out_size, clamp_max, _ptr(ws), _ptr(depth),
                                                  _stream()), "shr_mesh_render_fwd")
    return depth


def mesh_owner_supported(out_size, src_size=640):
    """True for the sizes the differentiable mesh path takes: square S with 0 < S <= src_size / 2 (S = 32 .. 320)."""
    return isinstance(out_size, int) and 0 < out_size and 2 * out_size <= src_size


def mesh_depth_owner_fwd(vertices, faces, out_size, src_size=640, clamp_max=100.0):
    """mesh_depth_fwd's depth [B,S,S] (the same bits) + owner [B,S,S,4] int32: the face of each of the output pixel's
    four bilinear taps (y0x0, y0x1, y1x0, y1x1), -1 for background, zero-weight or clamped taps."""
    _check_input(vertices, "vertices")
    _check_input(faces, "faces", torch.int32)
    if vertices.dim() != 3 or vertices.shape[2] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("vertices must be [B,NV,4] and faces [F,3]")
    if not mesh_owner_supported(out_size, src_size):
        raise RuntimeError("the differentiable mesh path takes square sizes 0 < S <= %d, not %r" % (src_size // 2, out_size))
    B, NV = vertices.shape[0], vertices.shape[1]
    with _on(vertices.device):
        depth = torch.empty((B, out_size, out_size), dtype=torch.float32, device=vertices.device)
        owner = torch.empty((B, out_size, out_size, 4), dtype=torch.int32, device=vertices.device)
        _lib.check(_lib.lib().shr_mesh_depth_owner_fwd(_ptr(vertices), _ptr(faces), B, NV, faces.shape[0], src_size,
                                                       out_size, clamp_max, _ptr(depth), _ptr(owner), _stream()),
                   "shr_mesh_depth_owner_fwd")
    return depth, owner


def mesh_depth_bwd(vertices, faces, owner, grad_depth, src_size=640):
    """d<grad_depth, depth>/d vertices [B,NV,4] = (du, dv, dz, 0) through the owner taps (coverage held fixed);
    deterministic fixed-point sums."""
    _check_input(vertices, "vertices")
    _check_input(faces, "faces", torch.int32)
    _check_input(owner, "owner", torch.int32)
    _check_input(grad_depth, "grad_depth")
    B, NV = vertices.shape[0], vertices.shape[1]
    S = grad_depth.shape[-1]
    if grad_depth.shape != (B, S, S) or owner.shape != (B, S, S, 4) or vertices.shape != (B, NV, 4):
        raise RuntimeError("grad_depth [B,S,S], owner [B,S,S,4] and vertices [B,NV,4] do not match")
    lib = _lib.lib()
    with _on(vertices.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=vertices.device)
        ws = torch.empty((max(1, lib.shr_mesh_depth_bwd_workspace_bytes(B, NV)),), dtype=torch.uint8,
                         device=vertices.device)
        _lib.check(lib.shr_mesh_depth_bwd(_ptr(vertices), _ptr(faces), _ptr(owner), _ptr(grad_depth), B, NV,
                                          faces.shape[0], src_size, S, _ptr(out), _ptr(ws), _stream()),
                   "shr_mesh_depth_bwd")
    return out


def lbs_project_bwd(grad_vertices, NB, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f=None):
    """lbs_project's backward (project = 1): grad_vertices [B,NV,4] -> grad_T [B,NB,4,4] (rand_f gets none)."""
    _check_input(grad_vertices, "grad_vertices")
    _check_input(skin_vertex_start, "skin_vertex_start", torch.int32)
    _check_input(skin_bone, "skin_bone", torch.int32)
    _check_input(skin_wv, "skin_wv")
    if rand_f is not None:
        _check_input(rand_f, "rand_f")
    B, NV = grad_vertices.shape[0], grad_vertices.shape[1]
    if NV != skin_vertex_start.numel() - 1 or grad_vertices.shape[2] != 4:
        raise RuntimeError("grad_vertices must be [B,NV,4] with the skin table's NV")
    cx, cy, fx, fy = camera
    with _on(grad_vertices.device):
        grad_T = torch.empty((B, NB, 4, 4), dtype=torch.float32, device=grad_vertices.device)
        _lib.check(_lib.lib().shr_lbs_project_bwd(_ptr(grad_vertices), B, NB, NV, _ptr(skin_vertex_start), _ptr(skin_bone),
                                                  _ptr(skin_wv), int(bool(right_hand)), cx, cy, fx, fy, _ptr(rand_f),
                                                  _ptr(grad_T), _stream()), "shr_lbs_project_bwd")
    return grad_T


def _skin_tables(skin_vertex_start, skin_bone, skin_wv, rand_f):
    _check_input(skin_vertex_start, "skin_vertex_start", torch.int32)
    _check_input(skin_bone, "skin_bone", torch.int32)
    _check_input(skin_wv, "skin_wv")
    if rand_f is not None:
        _check_input(rand_f, "rand_f")
    if skin_wv.dim() != 2 or skin_wv.shape[1] != 4 or skin_bone.numel() != skin_wv.shape[0] or skin_vertex_start.numel() < 1:
        raise RuntimeError("the skin table is skin_vertex_start [NV+1], skin_bone [NS], skin_wv [NS,4]")
    return skin_vertex_start.numel() - 1


def lbs_vertices_bwd(grad_vertices, NB, skin_vertex_start, skin_bone, skin_wv, right_hand, camera=None, rand_f=None):
    """lbs_project's backward in either mode (camera=None: the skinned points): grad_vertices [B,NV,4] -> grad_T
    [B,NB,4,4]; with a camera the bits of lbs_project_bwd.  rand_f gets none."""
    _check_input(grad_vertices, "grad_vertices")
    NV = _skin_tables(skin_vertex_start, skin_bone, skin_wv, rand_f)
    if grad_vertices.dim() != 3 or tuple(grad_vertices.shape[1:]) != (NV, 4):
        raise RuntimeError("grad_vertices must be [B,NV,4] with the skin table's NV")
    B = grad_vertices.shape[0]
    cx, cy, fx, fy = camera if camera is not None else (0.0, 0.0, 1.0, 1.0)
    with _on(grad_vertices.device):
        make = torch.zeros if B == 0 or NV == 0 else torch.empty
        grad_T = make((B, NB, 4, 4), dtype=torch.float32, device=grad_vertices.device)
        _lib.check(_lib.lib().shr_lbs_vertices_bwd(_ptr(grad_vertices), B, NB, NV, _ptr(skin_vertex_start), _ptr(skin_bone),
                                                   _ptr(skin_wv), int(bool(right_hand)), int(camera is not None), cx, cy,
                                                   fx, fy, _ptr(rand_f), _ptr(grad_T), _stream()), "shr_lbs_vertices_bwd")
    return grad_T


class SkinVertices(torch.autograd.Function):
    """T [B,NB,4,4] (or [B,NB,1,4,4]) -> the mesh's vertices [B,NV,4]: lbs_project (LinearBlendSkinning.forward,
    mesh/pointTransformation.py:39-46, and with camera=(cx,cy,fx,fy) OthographicalProjection.forward, :84-99), the same
    bits, with the backward to T (shr_lbs_vertices_bwd).  camera=None: the skinned points in model space.  rand_f and
    the tables get no gradient."""

    @staticmethod
    def forward(ctx, T, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f):
        _check_input(T, "transformation matrices")
        if T.dim() == 5 and T.shape[2] == 1:
            T = T.squeeze(2)
        if T.dim() != 4 or T.shape[2:] != (4, 4):
            raise RuntimeError("transformation matrices must be [B,NB,4,4]")
        _skin_tables(skin_vertex_start, skin_bone, skin_wv, rand_f)
        camera = None if camera is None else tuple(float(c) for c in camera)
        verts = lbs_project(T, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f)
        ctx.save_for_backward(skin_vertex_start, skin_bone, skin_wv, rand_f)
        ctx.meta = (T.shape[1], bool(right_hand), camera)
        return verts

    @staticmethod
    def backward(ctx, grad_vertices):
        start, bone, wv, rand_f = ctx.saved_tensors
        NB, right_hand, camera = ctx.meta
        g = grad_vertices.contiguous().float()
        return (lbs_vertices_bwd(g, NB, start, bone, wv, right_hand, camera, rand_f),) + (None,) * 6


class PoseVertices(torch.autograd.Function):
    """params [B,26] -> the mesh's vertices [B,NV,4]: ForwardKinematics followed by SkinVertices as ONE launch per
    direction (shr_pose_vertices_fwd / _bwd): the bone transforms stay in LDS.  Vertices and pose gradient are
    bit-identical to the two Functions chained.  camera=None: model space.  rand_f and the tables get no gradient."""

    @staticmethod
    def forward(ctx, params, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f):
        for t, name in ((params, "parameters"), (offset, "offset"), (offset_inv, "offset_inv")):
            _check_input(t, name)
        if params.dim() != 2 or params.shape[1] != 26:
            raise RuntimeError("parameters must be [B,26]")
        if tuple(offset.shape) != (17, 4, 4) or tuple(offset_inv.shape) != (17, 4, 4):
            raise RuntimeError("offset and offset_inv must be [17,4,4]")
        NV = _skin_tables(skin_vertex_start, skin_bone, skin_wv, rand_f)
        B = params.shape[0]
        camera = None if camera is None else tuple(float(c) for c in camera)
        cx, cy, fx, fy = camera if camera is not None else (0.0, 0.0, 1.0, 1.0)
        right, project = int(bool(right_hand)), int(camera is not None)
        with _on(params.device):
            verts = torch.empty((B, NV, 4), dtype=torch.float32, device=params.device)
            _lib.check(_lib.lib().shr_pose_vertices_fwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), NV,
                                                        _ptr(skin_vertex_start), _ptr(skin_bone), _ptr(skin_wv), right,
                                                        project, cx, cy, fx, fy, _ptr(rand_f), _ptr(verts), None, _stream()),
                       "shr_pose_vertices_fwd")
        ctx.save_for_backward(params, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, rand_f)
        ctx.meta = (B, NV, right, project, cx, cy, fx, fy)
        return verts

    @staticmethod
    def backward(ctx, grad_vertices):
        params, offset, offset_inv, start, bone, wv, rand_f = ctx.saved_tensors
        B, NV, right, project, cx, cy, fx, fy = ctx.meta
        g = grad_vertices.contiguous().float()
        with _on(g.device):
            make = torch.zeros if B == 0 or NV == 0 else torch.empty
            out = make((B, 26), dtype=torch.float32, device=g.device)
            _lib.check(_lib.lib().shr_pose_vertices_bwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), NV, _ptr(start),
                                                        _ptr(bone), _ptr(wv), right, project, cx, cy, fx, fy, _ptr(rand_f),
                                                        _ptr(g), _ptr(out), _stream()), "shr_pose_vertices_bwd")
        return (out,) + (None,) * 8


def _ik_tables(params, offset, offset_inv, bone, wv, name="parameters"):
    for t, what in ((params, name), (offset, "offset"), (offset_inv, "offset_inv"), (wv, "key-points")):
        _check_input(t, what)
    _check_input(bone, "key-point bones", torch.int32)
    if params.dim() != 2 or params.shape[1] != 26:
        raise RuntimeError("%s must be [B,26]" % name)
    if tuple(offset.shape) != (17, 4, 4) or tuple(offset_inv.shape) != (17, 4, 4):
        raise RuntimeError("offset and offset_inv must be [17,4,4]")
    J = bone.shape[0]
    if bone.dim() != 1 or tuple(wv.shape) != (J, 4) or not 1 <= J <= 64:
        raise RuntimeError("key-point tables must be bone [J] and wv [J,4] with 1 <= J <= 64")
    return params.shape[0], J


def _ik_weights(weights, stiffness, B, J):
    """(weights or None, weight_stride, stiffness or None) as the entries take them."""
    stride = 0
    if weights is not None:
        _check_input(weights, "weights")
        if tuple(weights.shape) == (B, J):
            stride = J
        elif tuple(weights.shape) != (J,):
            raise RuntimeError("weights must be [J] or [B,J]")
    if stiffness is not None:
        _check_input(stiffness, "stiffness")
        if tuple(stiffness.shape) != (26,):
            raise RuntimeError("stiffness must be [26]")
    return weights, stride, stiffness


def pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand=True):
    """params [B,26] -> (keypoints [B,J,4], jac [B,3J,26]): ops.PoseSpheres' xyz bit for bit (w = 1) and their derivative,
    row 3 j + c = d keypoint j component c / d params, in the frame PoseSpheres outputs (shr_pose_keypoints_jacobian)."""
    B, J = _ik_tables(params, offset, offset_inv, bone, wv)
    with _on(params.device):
        kp = torch.empty((B, J, 4), dtype=torch.float32, device=params.device)
        jac = torch.empty((B, 3 * J, 26), dtype=torch.float32, device=params.device)
        _lib.check(_lib.lib().shr_pose_keypoints_jacobian(_ptr(params), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone),
                                                          _ptr(wv), int(bool(right_hand)), _ptr(kp), _ptr(jac), _stream()),
                   "shr_pose_keypoints_jacobian")
    return kp, jac


def pose_ik(target, params0, offset, offset_inv, bone, wv, right_hand=True, weights=None, stiffness=None, iters=12,
            lambda0=1e-3):
    """Levenberg-Marquardt refinement of params0 [B,26] towards the keypoints target [B,J,3] (shr_pose_ik_fwd has the
    iteration): -> (params [B,26], cost0 [B], cost [B]).  weights [J] or [B,J], stiffness [26]: optional, each >= 0."""
    B, J = _ik_tables(params0, offset, offset_inv, bone, wv, "start parameters")
    _check_input(target, "target keypoints")
    if tuple(target.shape) != (B, J, 3):
        raise RuntimeError("target keypoints must be [B,J,3]")
    if int(iters) < 0 or not float(lambda0) > 0:
        raise RuntimeError("iters must be >= 0 and lambda0 > 0")
    weights, stride, stiffness = _ik_weights(weights, stiffness, B, J)
    with _on(params0.device):
        params = torch.empty((B, 26), dtype=torch.float32, device=params0.device)
        cost0 = torch.empty((B,), dtype=torch.float32, device=params0.device)
        cost = torch.empty((B,), dtype=torch.float32, device=params0.device)
        _lib.check(_lib.lib().shr_pose_ik_fwd(_ptr(target), _ptr(params0), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone),
                                              _ptr(wv), int(bool(right_hand)), _ptr(weights), stride, _ptr(stiffness),
                                              int(iters), float(lambda0), _ptr(params), _ptr(cost0), _ptr(cost), _stream()),
                   "shr_pose_ik_fwd")
    return params, cost0, cost


def pose_ik_bwd(params, grad_params, offset, offset_inv, bone, wv, right_hand=True, weights=None, stiffness=None):
    """grad_target [B,J,3] = w_j J_j (J^T W J + diag(mu))^-1 grad_params at `params` (shr_pose_ik_bwd); zeros for a crop
    whose matrix is not positive definite."""
    B, J = _ik_tables(params, offset, offset_inv, bone, wv)
    _check_input(grad_params, "parameter gradient")
    if tuple(grad_params.shape) != (B, 26):
        raise RuntimeError("parameter gradient must be [B,26]")
    weights, stride, stiffness = _ik_weights(weights, stiffness, B, J)
    with _on(params.device):
        out = torch.empty((B, J, 3), dtype=torch.float32, device=params.device)
        _lib.check(_lib.lib().shr_pose_ik_bwd(_ptr(params), _ptr(grad_params), B, _ptr(offset), _ptr(offset_inv), J,
                                              _ptr(bone), _ptr(wv), int(bool(right_hand)), _ptr(weights), stride,
                                              _ptr(stiffness), _ptr(out), _stream()), "shr_pose_ik_bwd")
    return out


class PoseFromKeypoints(torch.autograd.Function):
    """target keypoints [B,J,3], start pose [B,26] -> pose [B,26]: the solver pose_ik as a differentiable node.  Backward
    is the implicit-function gradient in Gauss-Newton form (pose_ik_bwd), to `target` only: the start pose, the weights
    and the stiffness get none."""

    @staticmethod
    def forward(ctx, target, params0, offset, offset_inv, bone, wv, right_hand, weights, stiffness, iters, lambda0):
        params, _, _ = pose_ik(target, params0, offset, offset_inv, bone, wv, right_hand, weights, stiffness, iters, lambda0)
        ctx.save_for_backward(params, offset, offset_inv, bone, wv, weights, stiffness)
        ctx.right_hand = bool(right_hand)
        return params

    @staticmethod
    def backward(ctx, grad_params):
        params, offset, offset_inv, bone, wv, weights, stiffness = ctx.saved_tensors
        g = pose_ik_bwd(params, grad_params.contiguous().float(), offset, offset_inv, bone, wv, ctx.right_hand, weights,
                        stiffness)
        return (g,) + (None,) * 10


class MeshDepthRaster(torch.autograd.Function):
    """vertices [B,NV,4] (pixel space) -> depth [B,S,S] of the fused raster + clamp + resize, differentiable w.r.t.
    (u, v, z) of the vertices.  Same contract as SphereDepthRaster: the gradient routes to each tap's owner face and
    holds coverage fixed (no edge, silhouette or visibility gradient)."""

    @staticmethod
    def forward(ctx, vertices, faces, out_size, src_size, clamp_max):
        vertices = vertices.contiguous()
        depth, owner = mesh_depth_owner_fwd(vertices, faces, out_size, src_size, clamp_max)
        ctx.save_for_backward(vertices, faces, owner)
        ctx.src_size = src_size
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        vertices, faces, owner = ctx.saved_tensors
        g = mesh_depth_bwd(vertices, faces, owner, grad_depth.contiguous().float(), ctx.src_size)
        return g, None, None, None, None


class MeshDepthRender(torch.autograd.Function):
    """DepthRender.forward, differentiable w.r.t. T [B,NB,4,4]: skinning + camera into the distinct vertices
    (lbs_project), then the owner-recording raster + clamp + resize; the depth is bit-identical to mesh_render_fwd.
    Backward: owner taps -> vertex gradient -> skinning + camera backward.  Same contract as SphereDepthRaster: coverage
    held fixed, no edge, silhouette or visibility gradient; rand_f (a random draw) gets none."""

    @staticmethod
    def forward(ctx, T, rand_f, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, faces, out_size,
                src_size=640, clamp_max=100.0):
        T = T.contiguous().float()
        verts = lbs_project(T, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f)
        depth, owner = mesh_depth_owner_fwd(verts, faces, out_size, src_size, clamp_max)
        ctx.save_for_backward(verts, owner, rand_f, skin_vertex_start, skin_bone, skin_wv, faces)
        ctx.meta = (T.shape[1], right_hand, camera, src_size)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        verts, owner, rand_f, start, bone, wv, faces = ctx.saved_tensors
        NB, right_hand, camera, src_size = ctx.meta
        gv = mesh_depth_bwd(verts, faces, owner, grad_depth.contiguous().float(), src_size)
        grad_T = lbs_project_bwd(gv, NB, start, bone, wv, right_hand, camera, rand_f)
        return (grad_T,) + (None,) * 10


def _soup_shape(face_vertices):
    _check_input(face_vertices, "face_vertices")
    if face_vertices.dim() != 4 or tuple(face_vertices.shape[2:]) != (3, 3):
        raise RuntimeError("face_vertices must be [B,F,3,3]")
    return face_vertices.shape[0], face_vertices.shape[1]


def _indexed_shape(vertices, faces):
    _check_input(vertices, "vertices")
    _check_input(faces, "faces", torch.int32)
    if vertices.dim() != 3 or vertices.shape[2] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("vertices must be [B,NV,4] and faces [F,3]")
    return vertices.shape[0], vertices.shape[1], faces.shape[0]


def tri_raster_owner_fwd(width, height, face_vertices):
    """tri_raster_fwd's depth [B,height,width] (the same bits) + owner [B,height,width] int32: the face whose offered
    depth is the pixel's (ties to the smaller index), -1 for background."""
    B, F = _soup_shape(face_vertices)
    with _on(face_vertices.device):
        depth = torch.empty((B, height, width), dtype=torch.float32, device=face_vertices.device)
        owner = torch.empty((B, height, width), dtype=torch.int32, device=face_vertices.device)
        _lib.check(_lib.lib().shr_tri_raster_owner_fwd(_ptr(face_vertices), B, F, width, height, _ptr(depth), _ptr(owner),
                                                       _stream()), "shr_tri_raster_owner_fwd")
    return depth, owner


def tri_raster_indexed_owner_fwd(width, height, vertices, faces):
    """tri_raster_indexed_fwd's depth [B,height,width] (the same bits) + owner [B,height,width] int32 (as above)."""
    B, NV, F = _indexed_shape(vertices, faces)
    with _on(vertices.device):
        depth = torch.empty((B, height, width), dtype=torch.float32, device=vertices.device)
        owner = torch.empty((B, height, width), dtype=torch.int32, device=vertices.device)
        _lib.check(_lib.lib().shr_tri_raster_indexed_owner_fwd(_ptr(vertices), _ptr(faces), B, NV, F, width, height,
                                                               _ptr(depth), _ptr(owner), _stream()),
                   "shr_tri_raster_indexed_owner_fwd")
    return depth, owner


def _check_pixel_grad(owner, grad_depth, B):
    _check_input(owner, "owner", torch.int32)
    _check_input(grad_depth, "grad_depth")
    if grad_depth.dim() != 3 or grad_depth.shape[0] != B or owner.shape != grad_depth.shape:
        raise RuntimeError("grad_depth and owner must both be [B,H,W] with the vertices' B")
    return grad_depth.shape[2], grad_depth.shape[1]


def tri_raster_bwd(face_vertices, owner, grad_depth):
    """d<grad_depth, depth>/d face_vertices [B,F,3,3] through each pixel's owner face (coverage held fixed);
    deterministic fixed-point sums."""
    B, F = _soup_shape(face_vertices)
    W, H = _check_pixel_grad(owner, grad_depth, B)
    lib = _lib.lib()
    with _on(face_vertices.device):
        out = torch.empty((B, F, 3, 3), dtype=torch.float32, device=face_vertices.device)
        ws = torch.empty((max(16, lib.shr_tri_raster_bwd_workspace_bytes(B, F)),), dtype=torch.uint8,
                         device=face_vertices.device)
        _lib.check(lib.shr_tri_raster_bwd(_ptr(face_vertices), _ptr(owner), _ptr(grad_depth), B, F, W, H, _ptr(out), _ptr(ws),
                                          _stream()), "shr_tri_raster_bwd")
    return out


def tri_raster_indexed_bwd(vertices, faces, owner, grad_depth):
    """d<grad_depth, depth>/d vertices [B,NV,4] = (du, dv, dz, 0) through each pixel's owner face (coverage held
    fixed); deterministic fixed-point sums."""
    B, NV, F = _indexed_shape(vertices, faces)
    W, H = _check_pixel_grad(owner, grad_depth, B)
    lib = _lib.lib()
    with _on(vertices.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=vertices.device)
        ws = torch.empty((max(16, lib.shr_tri_raster_indexed_bwd_workspace_bytes(B, NV)),), dtype=torch.uint8,
                         device=vertices.device)
        _lib.check(lib.shr_tri_raster_indexed_bwd(_ptr(vertices), _ptr(faces), _ptr(owner), _ptr(grad_depth), B, NV, F, W, H,
                                                  _ptr(out), _ptr(ws), _stream()), "shr_tri_raster_indexed_bwd")
    return out


class TriRaster(torch.autograd.Function):
    """depth_rasterization.forward with a backward: face_vertices [B,F,3,3] (pixel-space x, y, z) -> raw depth
    [B,height,width], background 1000, the same bits.  Differentiable w.r.t. face_vertices: each pixel's gradient goes
    to the face that owns its depth, coverage held fixed (no edge, silhouette or visibility gradient)."""

    @staticmethod
    def forward(ctx, face_vertices, width, height):
        face_vertices = face_vertices.contiguous()
        depth, owner = tri_raster_owner_fwd(width, height, face_vertices)
        ctx.save_for_backward(face_vertices, owner)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        face_vertices, owner = ctx.saved_tensors
        return tri_raster_bwd(face_vertices, owner, grad_depth.contiguous().float()), None, None


def vertices4(vertices):
    """vertices [B,NV,3 or 4] -> (the contiguous [B,NV,4] the kernels take, a zero appended to three components; whether
    the input had four): the Functions below hand the gradient back in the width they were given."""
    if vertices.dim() != 3 or vertices.shape[-1] not in (3, 4):
        raise RuntimeError("vertices must be [B,NV,3] or [B,NV,4]")
    width4 = vertices.shape[-1] == 4
    return (vertices.contiguous() if width4 else torch.nn.functional.pad(vertices, (0, 1)).contiguous()), width4


def _grad_as_given(ctx, gverts):
    return gverts if gverts is None or ctx.width4 else gverts[..., :3]


def _tri_indexed_forward(ctx, vertices, faces, width, height):
    v4, ctx.width4 = vertices4(vertices)
    depth, owner = tri_raster_indexed_owner_fwd(width, height, v4, faces)
    ctx.save_for_backward(v4, faces, owner)
    return depth, owner


def _tri_indexed_backward(ctx, grad_depth):
    v4, faces, owner = ctx.saved_tensors
    g = tri_raster_indexed_bwd(v4, faces, owner, grad_depth.contiguous().float())
    return _grad_as_given(ctx, g), None, None, None


class TriRasterIndexed(torch.autograd.Function):
    """TriRaster on an indexed mesh: vertices [B,NV,3 or 4] (pixel space) + faces [F,3] int32 -> raw depth
    [B,height,width], the bits of tri_raster_indexed_fwd; differentiable w.r.t. vertices[..., :3]."""

    @staticmethod
    def forward(ctx, vertices, faces, width, height):
        return _tri_indexed_forward(ctx, vertices, faces, width, height)[0]

    @staticmethod
    def backward(ctx, grad_depth):
        return _tri_indexed_backward(ctx, grad_depth)


class TriRasterIndexedOwner(torch.autograd.Function):
    """TriRasterIndexed that also returns the owners: (raw depth [B,height,width], differentiable w.r.t.
    vertices[..., :3] exactly as TriRasterIndexed, owner [B,height,width] int32, not differentiable) -- one owner forward
    for both the raster's backward and the antialias pass (TriAntialias)."""

    @staticmethod
    def forward(ctx, vertices, faces, width, height):
        depth, owner = _tri_indexed_forward(ctx, vertices, faces, width, height)
        ctx.mark_non_differentiable(owner)
        return depth, owner

    @staticmethod
    def backward(ctx, grad_depth, _grad_owner):
        return _tri_indexed_backward(ctx, grad_depth)


def tri_edge_table(faces, weld=None):
    """The antialias pass's edge table (host, numpy): faces [F,3] (as the raster takes them: after the right hand's
    winding swap) -> edges [F,3] int32.  Edge k of face f joins corners k and (k + 1) % 3; edges[f,k] is the other face
    that shares this undirected edge, -1 when no other face shares it or when three or more do (a boundary).  Corners
    are matched on welded ids: `weld` None (the faces' own ids), an integer array [NV] (vertex -> point id), or a float
    array [NV,C] of positions (vertices with bit-identical rows are one point)."""
    f = np.asarray(faces.cpu().numpy() if isinstance(faces, torch.Tensor) else faces).astype(np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise RuntimeError("faces must be [F,3]")
    if weld is not None:
        w = np.asarray(weld.cpu().numpy() if isinstance(weld, torch.Tensor) else weld)
        if w.dtype.kind == "f":
            rows = np.ascontiguousarray(w.reshape(len(w), -1))
            _, w = np.unique(rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel(),
                             return_inverse=True)
        w = np.asarray(w, np.int64).ravel()
        if len(f) and (f.min() < 0 or f.max() >= len(w)):
            raise RuntimeError("faces index outside the welded vertices")
        f = w[f]
    F = len(f)
    a, b = f, f[:, [1, 2, 0]]
    key = np.stack([np.minimum(a, b), np.maximum(a, b)], -1).reshape(-1, 2)      # row 3 f + k: edge k of face f
    _, grp, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    grp = grp.ravel()
    edges = np.full(3 * F, -1, np.int64)
    two = np.nonzero(cnt[grp] == 2)[0]
    order = two[np.argsort(grp[two], kind="stable")]                         # the two rows of each group, adjacent
    first, second = order[0::2], order[1::2]
    edges[first], edges[second] = second // 3, first // 3
    return edges.reshape(F, 3).astype(np.int32)


def _aa_shape(values, depth, owner, vertices, faces, edges):
    _check_input(values, "values")
    _check_input(depth, "depth")
    _check_input(owner, "owner", torch.int32)
    B, NV, F = _indexed_shape(vertices, faces)
    _check_input(edges, "edges", torch.int32)
    if values.dim() != 3 or values.shape[0] != B or depth.shape != values.shape or owner.shape != values.shape:
        raise RuntimeError("values, depth and owner must all be [B,H,W] with the vertices' B")
    if tuple(edges.shape) != (F, 3):
        raise RuntimeError("edges must be [F,3]")
    return B, NV, F, values.shape[2], values.shape[1]


def _aa_call_fwd(entry, tensors, *dims):
    """One of the two forward entries of the pass (dims: B, NV, F, W, H and, for maps, C) on (values, depth, owner,
    vertices, faces, edges), already checked."""
    with _on(tensors[0].device):
        out = torch.empty_like(tensors[0])
        _lib.check(getattr(_lib.lib(), entry)(*[_ptr(t) for t in tensors], *dims, _ptr(out), _stream()), entry)
    return out


def _aa_call_bwd(entry, tensors, grad_out, want_values, want_vertices, *dims):
    """One of the two backward entries of the pass, as _aa_call_fwd: (grad_values or None, grad_vertices or None)."""
    if not (want_values or want_vertices):
        return None, None
    lib, values, (B, NV) = _lib.lib(), tensors[0], dims[:2]
    with _on(values.device):
        gvals = torch.empty_like(values) if want_values else None
        gverts = torch.empty((B, NV, 4), dtype=torch.float32, device=values.device) if want_vertices else None
        ws = torch.empty((max(16, getattr(lib, entry + "_workspace_bytes")(B, NV)),), dtype=torch.uint8,
                         device=values.device) if want_vertices else None
        _lib.check(getattr(lib, entry)(*[_ptr(t) for t in tensors], *dims, _ptr(grad_out), _ptr(gvals), _ptr(gverts),
                                       _ptr(ws), _stream()), entry)
    return gvals, gverts


def tri_antialias(values, depth, owner, vertices, faces, edges):
    """The antialias pass (include/spherehand_hip.h, shr_tri_antialias_fwd): values [B,H,W] blended across the
    silhouette edges of the owner faces -> [B,H,W]; depth, owner from tri_raster_indexed_owner_fwd, vertices [B,NV,4]
    pixel space, faces [F,3] int32, edges [F,3] int32 (tri_edge_table)."""
    dims = _aa_shape(values, depth, owner, vertices, faces, edges)
    return _aa_call_fwd("shr_tri_antialias_fwd", (values, depth, owner, vertices, faces, edges), *dims)


def tri_antialias_bwd(values, depth, owner, vertices, faces, edges, grad_out, want_values=True, want_vertices=True):
    """tri_antialias's backward: (grad_values [B,H,W] or None, grad_vertices [B,NV,4] = (d/dx, d/dy, 0, 0) or None);
    the vertex sums are deterministic fixed point."""
    dims = _aa_shape(values, depth, owner, vertices, faces, edges)
    _check_input(grad_out, "grad_out")
    if grad_out.shape != values.shape:
        raise RuntimeError("grad_out must be [B,H,W] as values")
    return _aa_call_bwd("shr_tri_antialias_bwd", (values, depth, owner, vertices, faces, edges), grad_out, want_values,
                        want_vertices, *dims)


def _aa_forward(ctx, fwd, values, depth, owner, vertices, faces, edges):
    v4, ctx.width4 = vertices4(vertices)
    values, depth, owner = values.contiguous(), depth.contiguous(), owner.contiguous()
    out = fwd(values, depth, owner, v4, faces, edges)
    ctx.save_for_backward(values, depth, owner, v4, faces, edges)
    return out


def _aa_backward(ctx, bwd, grad_out):
    values, depth, owner, v4, faces, edges = ctx.saved_tensors
    gvals, gverts = bwd(values, depth, owner, v4, faces, edges, grad_out.contiguous().float(), ctx.needs_input_grad[0],
                        ctx.needs_input_grad[3])
    return gvals, None, None, _grad_as_given(ctx, gverts), None, None


class TriAntialias(torch.autograd.Function):
    """tri_antialias with a backward: (values [B,H,W], depth, owner, vertices [B,NV,3 or 4] pixel space, faces, edges)
    -> the antialiased values.  Differentiable w.r.t. values and vertices[..., :2] (the z gradient is zero); depth and
    owner get none."""

    @staticmethod
    def forward(ctx, values, depth, owner, vertices, faces, edges):
        return _aa_forward(ctx, tri_antialias, values, depth, owner, vertices, faces, edges)

    @staticmethod
    def backward(ctx, grad_out):
        return _aa_backward(ctx, tri_antialias_bwd, grad_out)


TRI_INTERP_MAX_CHANNELS = 64   # include/spherehand_hip.h, shr_tri_interp_fwd


def _interp_shape(attr, owner, vertices, faces):
    _check_input(attr, "attr")
    _check_input(owner, "owner", torch.int32)
    B, NV, F = _indexed_shape(vertices, faces)
    if owner.dim() != 3 or owner.shape[0] != B:
        raise RuntimeError("owner must be [B,H,W] with the vertices' B")
    if attr.dim() not in (2, 3) or attr.shape[-2] != NV or (attr.dim() == 3 and attr.shape[0] != B):
        raise RuntimeError("attr must be [B,NV,C] or [NV,C] with the vertices' B and NV")
    C = attr.shape[-1]
    if not 1 <= C <= TRI_INTERP_MAX_CHANNELS:
        raise RuntimeError("attr must have 1 .. %d channels" % TRI_INTERP_MAX_CHANNELS)
    if not (attr.device == owner.device == vertices.device == faces.device):
        raise RuntimeError("attr, owner, vertices and faces must be on one device")
    return B, NV, F, owner.shape[2], owner.shape[1], C, (NV * C if attr.dim() == 3 else 0)


def tri_interpolate(attr, owner, vertices, faces):
    """Vertex attributes interpolated over the owner map (include/spherehand_hip.h, shr_tri_interp_fwd): attr [B,NV,C]
    or [NV,C] (shared by all crops), owner [B,H,W] int32 from tri_raster_indexed_owner_fwd, vertices [B,NV,4] pixel
    space and faces [F,3] int32 as the raster took them -> maps [B,C,H,W], 0 at background pixels."""
    B, NV, F, W, H, C, stride = _interp_shape(attr, owner, vertices, faces)
    with _on(owner.device):
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=owner.device)
        _lib.check(_lib.lib().shr_tri_interp_fwd(_ptr(owner), _ptr(vertices), _ptr(faces), _ptr(attr), stride, B, NV, F, W,
                                                 H, C, _ptr(out), _stream()), "shr_tri_interp_fwd")
    return out


def tri_interpolate_bwd(attr, owner, vertices, faces, grad_out, want_attr=True, want_vertices=True):
    """tri_interpolate's backward: (grad_attr [B,NV,C] -- per crop, also for shared attributes -- or None,
    grad_vertices [B,NV,4] = (d/dx, d/dy, 0, 0) or None); deterministic fixed-point sums."""
    B, NV, F, W, H, C, stride = _interp_shape(attr, owner, vertices, faces)
    _check_input(grad_out, "grad_out")
    if tuple(grad_out.shape) != (B, C, H, W):
        raise RuntimeError("grad_out must be [B,C,H,W]")
    if not (want_attr or want_vertices):
        return None, None
    lib = _lib.lib()
    with _on(owner.device):
        gattr = torch.empty((B, NV, C), dtype=torch.float32, device=owner.device) if want_attr else None
        gverts = torch.empty((B, NV, 4), dtype=torch.float32, device=owner.device) if want_vertices else None
        nbytes = lib.shr_tri_interp_bwd_workspace_bytes(B, NV, C, int(want_attr), int(want_vertices))
        ws = torch.empty((max(16, nbytes),), dtype=torch.uint8, device=owner.device)
        _lib.check(lib.shr_tri_interp_bwd(_ptr(owner), _ptr(vertices), _ptr(faces), _ptr(attr), stride, B, NV, F, W, H, C,
                                          _ptr(grad_out), _ptr(gattr), _ptr(gverts), _ptr(ws), _stream()),
                   "shr_tri_interp_bwd")
    return gattr, gverts


class TriInterpolate(torch.autograd.Function):
    """tri_interpolate with a backward: (attr [B,NV,C] or [NV,C], owner, vertices [B,NV,3 or 4] pixel space, faces) ->
    maps [B,C,H,W].  Differentiable w.r.t. attr (shared attributes get the sum over the crops) and vertices[..., :2]
    (the z gradient is zero); coverage and owner are held fixed."""

    @staticmethod
    def forward(ctx, attr, owner, vertices, faces):
        v4, ctx.width4 = vertices4(vertices)
        attr, owner = attr.contiguous(), owner.contiguous()
        out = tri_interpolate(attr, owner, v4, faces)
        ctx.save_for_backward(attr, owner, v4, faces)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        attr, owner, v4, faces = ctx.saved_tensors
        gattr, gverts = tri_interpolate_bwd(attr, owner, v4, faces, grad_out.contiguous().float(),
                                            ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        if gattr is not None and attr.dim() == 2:
            gattr = gattr.sum(0)
        return gattr, None, _grad_as_given(ctx, gverts), None


def _aa_maps_shape(values, depth, owner, vertices, faces, edges):
    # shapes and types first, then where the tensors live: the messages name what is wrong with the call
    for t, name, dtype in ((values, "values", torch.float32), (depth, "depth", torch.float32),
                           (owner, "owner", torch.int32), (vertices, "vertices", torch.float32),
                           (faces, "faces", torch.int32), (edges, "edges", torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("%s must be a torch.Tensor" % name)
        if t.dtype != dtype:
            raise RuntimeError("%s must be %s" % (name, dtype))
    if values.dim() != 4:
        raise RuntimeError("values must be [B,C,H,W] (tri_antialias takes one plane [B,H,W])")
    if vertices.dim() != 3 or vertices.shape[2] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("vertices must be [B,NV,4] and faces [F,3]")
    B, C, H, W = values.shape
    NV, F = vertices.shape[1], faces.shape[0]
    if not 1 <= C <= TRI_INTERP_MAX_CHANNELS:
        raise RuntimeError("values must have 1 .. %d channels" % TRI_INTERP_MAX_CHANNELS)
    if vertices.shape[0] != B or tuple(depth.shape) != (B, H, W) or tuple(owner.shape) != (B, H, W):
        raise RuntimeError("depth and owner must be [B,H,W] of values [B,C,H,W], with the vertices' B")
    if tuple(edges.shape) != (F, 3):
        raise RuntimeError("edges must be [F,3]")
    for t, name, dtype in ((values, "values", torch.float32), (depth, "depth", torch.float32),
                           (owner, "owner", torch.int32), (edges, "edges", torch.int32)):
        _check_input(t, name, dtype)
    _indexed_shape(vertices, faces)
    if not (values.device == depth.device == owner.device == vertices.device == faces.device == edges.device):
        raise RuntimeError("values, depth, owner, vertices, faces and edges must be on one device")
    return B, NV, F, W, H, C


def tri_antialias_maps(values, depth, owner, vertices, faces, edges):
    """The antialias pass over multi-channel maps (include/spherehand_hip.h, shr_tri_antialias_maps_fwd): values
    [B,C,H,W] (tri_interpolate's maps, 1 <= C <= 64) -> [B,C,H,W], every channel the bits of tri_antialias on that plane,
    with each pair decided once for all channels; the other arguments as tri_antialias takes them."""
    dims = _aa_maps_shape(values, depth, owner, vertices, faces, edges)
    return _aa_call_fwd("shr_tri_antialias_maps_fwd", (values, depth, owner, vertices, faces, edges), *dims)


def tri_antialias_maps_bwd(values, depth, owner, vertices, faces, edges, grad_out, want_values=True, want_vertices=True):
    """tri_antialias_maps's backward: (grad_values [B,C,H,W] or None, grad_vertices [B,NV,4] = (d/dx, d/dy, 0, 0) or
    None); the vertex sums are deterministic fixed point."""
    dims = _aa_maps_shape(values, depth, owner, vertices, faces, edges)
    _check_input(grad_out, "grad_out")
    if grad_out.shape != values.shape or grad_out.device != values.device:
        raise RuntimeError("grad_out must be [B,C,H,W] as values, on their device")
    return _aa_call_bwd("shr_tri_antialias_maps_bwd", (values, depth, owner, vertices, faces, edges), grad_out,
                        want_values, want_vertices, *dims)


class TriAntialiasMaps(torch.autograd.Function):
    """tri_antialias_maps with a backward: (values [B,C,H,W], depth, owner, vertices [B,NV,3 or 4] pixel space, faces,
    edges) -> the antialiased maps.  Differentiable w.r.t. values and vertices[..., :2] (the z gradient is zero); depth
    and owner get none."""

    @staticmethod
    def forward(ctx, values, depth, owner, vertices, faces, edges):
        return _aa_forward(ctx, tri_antialias_maps, values, depth, owner, vertices, faces, edges)

    @staticmethod
    def backward(ctx, grad_out):
        return _aa_backward(ctx, tri_antialias_maps_bwd, grad_out)


class TriVertexTables:
    """The incidence tables of the vertex normals (include/spherehand_hip.h, shr_tri_vertex_normals_fwd), all int32; a
    corner is the integer 3 f + k.  NV, F: what they were built for.
        point[NV]                    vertex -> welded point id in [0, NP)
        inc_start[NP+1], inc[NI]     welded incidence: the corners whose vertex welds to the point, ascending
        copy_start[NP+1], copy[NV]   the vertices that weld to the point, ascending
        own_start[NV+1], own[NO]     own-id incidence: the corners with faces[f,k] == v, ascending
    tri_vertex_tables returns them as numpy arrays; .to(device) gives the torch tensors the entry points take."""
    FIELDS = ("point", "inc_start", "inc", "copy_start", "copy", "own_start", "own")

    def __init__(self, NV, F, **arrays):
        self.NV, self.F = int(NV), int(F)
        for name in self.FIELDS:
            setattr(self, name, arrays[name])

    @property
    def NP(self):
        return len(self.inc_start) - 1

    def arrays(self):
        return tuple(getattr(self, name) for name in self.FIELDS)

    def to(self, device):
        return TriVertexTables(self.NV, self.F, **{
            name: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.int32))).to(device)
            for name, a in zip(self.FIELDS, self.arrays())})


def _csr(keys, n, items):
    """items grouped by key (stable: ascending items stay ascending within a key) -> (start [n+1], items) int32"""
    order = np.argsort(keys, kind="stable")
    start = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(keys, minlength=n), out=start[1:])
    return start.astype(np.int32), np.asarray(items)[order].astype(np.int32)


def tri_vertex_tables(faces, NV, weld=None):
    """The vertex normals' tables (host, numpy, built once): faces [F,3] as the raster takes them (after the right hand's
    winding swap), NV vertices -> TriVertexTables.  `weld` as tri_edge_table takes it: None (every vertex its own point),
    an integer array [NV] (vertex -> point id; ids are renumbered densely), or a float array [NV,C] of positions
    (vertices with bit-identical rows are one point).  Faces with a vertex id outside [0, NV) appear in no table.
    Without welding the three tables coincide: inc == own and copy is the identity."""
    f = np.asarray(faces.cpu().numpy() if isinstance(faces, torch.Tensor) else faces).astype(np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise RuntimeError("faces must be [F,3]")
    NV = int(NV)
    if NV <= 0:
        raise RuntimeError("NV must be positive")
    if weld is None:
        point = np.arange(NV, dtype=np.int64)
    else:
        w = np.asarray(weld.cpu().numpy() if isinstance(weld, torch.Tensor) else weld)
        if len(w) != NV:
            raise RuntimeError("weld must have NV rows")
        if w.dtype.kind == "f":
            rows = np.ascontiguousarray(w.reshape(len(w), -1))
            w = rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()
        _, point = np.unique(np.asarray(w).ravel(), return_inverse=True)
        point = np.asarray(point, np.int64).ravel()
    NP = int(point.max()) + 1
    valid = np.all((f >= 0) & (f < NV), axis=1)
    corners = np.nonzero(np.repeat(valid, 3))[0]
    vid = f.ravel()[corners]
    own_start, own = _csr(vid, NV, corners)
    inc_start, inc = _csr(point[vid], NP, corners)
    copy_start, copy = _csr(point, NP, np.arange(NV))
    return TriVertexTables(NV, len(f), point=point.astype(np.int32), inc_start=inc_start, inc=inc, copy_start=copy_start,
                           copy=copy, own_start=own_start, own=own)


def _normals_shape(points, faces, tables):
    _check_input(points, "points")
    _check_input(faces, "faces", torch.int32)
    if points.dim() != 3 or points.shape[2] != 4 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("points must be [B,NV,4] and faces [F,3]")
    B, NV, F = points.shape[0], points.shape[1], faces.shape[0]
    if not isinstance(tables, TriVertexTables):
        raise RuntimeError("tables must be a TriVertexTables (tri_vertex_tables(...).to(device))")
    for name, t in zip(tables.FIELDS, tables.arrays()):
        _check_input(t, "tables." + name, torch.int32)
        if t.dim() != 1 or t.device != points.device:
            raise RuntimeError("tables.%s must be one-dimensional, on the points' device" % name)
    if faces.device != points.device:
        raise RuntimeError("points, faces and tables must be on one device")
    NP = tables.NP
    if tables.NV != NV or tables.F != F or NP < 1 or tables.point.numel() != NV or tables.copy.numel() != NV or \
            tables.copy_start.numel() != NP + 1 or tables.own_start.numel() != NV + 1:
        raise RuntimeError("tables do not match faces [F,3] and the points' NV (built for NV = %d, F = %d)"
                           % (tables.NV, tables.F))
    return B, NV, F, NP, tables.inc.numel(), tables.own.numel()


def tri_vertex_normals(points, faces, tables, want_raw=False):
    """Area-weighted vertex normals (include/spherehand_hip.h, shr_tri_vertex_normals_fwd): points [B,NV,4] (x, y, z, -),
    faces [F,3] int32, tables from tri_vertex_tables(...).to(device) -> unit normals [B,NV,4] = (n, 0); with want_raw
    also the unnormalised sums [B,NV,4] = (N, 0).  The normals of the faces' own winding: never flipped."""
    B, NV, F, NP, NI, _ = _normals_shape(points, faces, tables)
    T = tables
    with _on(points.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=points.device)
        raw = torch.empty_like(out) if want_raw else None
        _lib.check(_lib.lib().shr_tri_vertex_normals_fwd(_ptr(points), _ptr(faces), _ptr(T.point), _ptr(T.inc_start),
                                                         _ptr(T.inc), _ptr(T.copy_start), _ptr(T.copy), B, NV, F, NP, NI,
                                                         _ptr(out), _ptr(raw), _stream()), "shr_tri_vertex_normals_fwd")
    return (out, raw) if want_raw else out


def tri_vertex_normals_bwd(points, faces, tables, grad_normals):
    """tri_vertex_normals's backward: grad_normals [B,NV,4] (the fourth component is not read) -> grad_points [B,NV,4] =
    (d/dx, d/dy, d/dz, 0); fp64 gathers in a fixed order, bitwise reproducible."""
    B, NV, F, NP, NI, NO = _normals_shape(points, faces, tables)
    _check_input(grad_normals, "grad_normals")
    if grad_normals.shape != points.shape or grad_normals.device != points.device:
        raise RuntimeError("grad_normals must be [B,NV,4] as points, on their device")
    T, lib = tables, _lib.lib()
    with _on(points.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=points.device)
        ws = torch.empty((max(16, lib.shr_tri_vertex_normals_bwd_workspace_bytes(B, NP)),), dtype=torch.uint8,
                         device=points.device)
        _lib.check(lib.shr_tri_vertex_normals_bwd(_ptr(points), _ptr(faces), _ptr(T.point), _ptr(T.inc_start), _ptr(T.inc),
                                                  _ptr(T.copy_start), _ptr(T.copy), _ptr(T.own_start), _ptr(T.own), B, NV,
                                                  F, NP, NI, NO, _ptr(grad_normals), _ptr(out), _ptr(ws), _stream()),
                   "shr_tri_vertex_normals_bwd")
    return out


class TriVertexNormals(torch.autograd.Function):
    """tri_vertex_normals with a backward: (points [B,NV,3 or 4], faces [F,3] int32, tables) -> unit normals [B,NV,4] =
    (n, 0).  Differentiable w.r.t. points[..., :3], the zero rule held fixed; the gradient comes back in the width
    given."""

    @staticmethod
    def forward(ctx, points, faces, tables):
        p4, ctx.width4 = vertices4(points)
        ctx.tables = tables
        ctx.save_for_backward(p4, faces)
        return tri_vertex_normals(p4, faces, tables)

    @staticmethod
    def backward(ctx, grad_normals):
        p4, faces = ctx.saved_tensors
        g = tri_vertex_normals_bwd(p4, faces, ctx.tables, grad_normals.contiguous().float())
        return _grad_as_given(ctx, g), None, None


def _unit3_shape(maps, name="maps"):
    _check_input(maps, name)
    if maps.dim() != 4 or maps.shape[1] != 3:
        raise RuntimeError("%s must be [B,3,H,W]" % name)
    return maps.shape[0], maps.shape[3], maps.shape[2]


def unit3_maps(maps, out=None):
    """Per-pixel unit normalisation of three planes (include/spherehand_hip.h, shr_unit3_maps_fwd): maps [B,3,H,W] ->
    [B,3,H,W], each pixel's (m0, m1, m2) divided by its length; a pixel whose sum of squares is 0 or not finite gets 0.
    `out`: where to write (not overlapping maps)."""
    B, W, H = _unit3_shape(maps)
    if out is not None:
        _check_input(out, "out")
        if out.shape != maps.shape or out.device != maps.device:
            raise RuntimeError("out must be [B,3,H,W] as maps, on their device")
    with _on(maps.device):
        if out is None:
            out = torch.empty_like(maps)
        _lib.check(_lib.lib().shr_unit3_maps_fwd(_ptr(maps), B, W, H, _ptr(out), _stream()), "shr_unit3_maps_fwd")
    return out


def unit3_maps_bwd(maps, grad_out):
    """unit3_maps's backward: grad_maps [B,3,H,W] = (g - o (o . g)) / |m| per pixel, 0 where the forward wrote 0."""
    B, W, H = _unit3_shape(maps)
    _check_input(grad_out, "grad_out")
    if grad_out.shape != maps.shape or grad_out.device != maps.device:
        raise RuntimeError("grad_out must be [B,3,H,W] as maps, on their device")
    with _on(maps.device):
        out = torch.empty_like(maps)
        _lib.check(_lib.lib().shr_unit3_maps_bwd(_ptr(maps), _ptr(grad_out), B, W, H, _ptr(out), _stream()),
                   "shr_unit3_maps_bwd")
    return out


class Unit3Maps(torch.autograd.Function):
    """unit3_maps with a backward: maps [B,3,H,W] -> unit maps, differentiable w.r.t. maps."""

    @staticmethod
    def forward(ctx, maps):
        maps = maps.contiguous()
        ctx.save_for_backward(maps)
        return unit3_maps(maps)

    @staticmethod
    def backward(ctx, grad_out):
        maps, = ctx.saved_tensors
        return unit3_maps_bwd(maps, grad_out.contiguous().float())


def distance_transform(depth, fg_max):
    """The exact squared Euclidean distance transform of the foreground (include/spherehand_hip.h, shr_dt_fwd): depth
    [B,H,W] fp32 -> int32 [B,H,W], each pixel's squared distance to the nearest pixel with depth < fg_max; H H + W W
    everywhere in an image that has none."""
    _check_input(depth, "depth")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise RuntimeError("depth must be [B,H,W] with H, W >= 1")
    B, H, W = depth.shape
    lib = _lib.lib()
    with _on(depth.device):
        d2 = torch.empty((B, H, W), dtype=torch.int32, device=depth.device)
        ws = torch.empty((max(16, lib.shr_dt_workspace_bytes(B, H, W)),), dtype=torch.uint8, device=depth.device)
        _lib.check(lib.shr_dt_fwd(_ptr(depth), B, H, W, float(fg_max), _ptr(d2), _ptr(ws), _stream()), "shr_dt_fwd")
    return d2


def _dt_sample_shape(d2, points):
    _check_input(d2, "d2", torch.int32)
    _check_input(points, "points")
    if d2.dim() != 3 or d2.shape[1] < 2 or d2.shape[2] < 2:
        raise RuntimeError("d2 must be [B,H,W] with H, W >= 2")
    if points.dim() != 3 or points.shape[2] < 2 or points.shape[0] != d2.shape[0] or points.device != d2.device:
        raise RuntimeError("points must be [B,N,C] with C >= 2 and d2's B, on its device")
    return d2.shape[0], d2.shape[1], d2.shape[2], points.shape[1], points.shape[2]


def dt_sample(d2, points, max_dist=float("inf")):
    """Bilinear samples of min(sqrt(d2), max_dist) at points [B,N,C] = (x, y, ...) in pixel coordinates
    (include/spherehand_hip.h, shr_dt_sample_fwd) -> (value [B,N], grad_xy [B,N,2] = d value / d (x, y)).  Points outside
    the image sample its border with zero gradient in the clamped component; non-finite points give zeros."""
    B, H, W, N, C = _dt_sample_shape(d2, points)
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise RuntimeError("max_dist must be >= 0 (inf: no saturation), not %r" % (max_dist,))
    with _on(d2.device):
        value = torch.empty((B, N), dtype=torch.float32, device=d2.device)
        grad_xy = torch.empty((B, N, 2), dtype=torch.float32, device=d2.device)
        _lib.check(_lib.lib().shr_dt_sample_fwd(_ptr(d2), B, H, W, _ptr(points), N, C, max_dist, _ptr(value),
                                                _ptr(grad_xy), _stream()), "shr_dt_sample_fwd")
    return value, grad_xy


def dt_sample_bwd(grad_xy, grad_value, C):
    """dt_sample's backward: grad_xy [B,N,2] (the forward's), grad_value [B,N] -> grad_points [B,N,C], components 0 and 1
    = grad_value * grad_xy, the others 0."""
    _check_input(grad_xy, "grad_xy")
    _check_input(grad_value, "grad_value")
    if grad_xy.dim() != 3 or grad_xy.shape[2] != 2 or grad_value.shape != grad_xy.shape[:2] or \
            grad_value.device != grad_xy.device:
        raise RuntimeError("grad_xy must be [B,N,2] and grad_value [B,N], on one device")
    if C < 2:
        raise RuntimeError("C must be >= 2")
    B, N = grad_value.shape
    with _on(grad_xy.device):
        out = torch.empty((B, N, C), dtype=torch.float32, device=grad_xy.device)
        _lib.check(_lib.lib().shr_dt_sample_bwd(_ptr(grad_xy), _ptr(grad_value), B, N, C, _ptr(out), _stream()),
                   "shr_dt_sample_bwd")
    return out


class DistanceSample(torch.autograd.Function):
    """dt_sample with a backward: (points [B,N,C], d2 [B,H,W] int32, max_dist) -> distances [B,N], differentiable w.r.t.
    points[..., :2] (the bilinear cell's own slope: piecewise constant, zero in a clamped component)."""

    @staticmethod
    def forward(ctx, points, d2, max_dist=float("inf")):
        points = points.contiguous()
        value, grad_xy = dt_sample(d2, points, max_dist)
        ctx.C = points.shape[2]
        ctx.save_for_backward(grad_xy)
        return value

    @staticmethod
    def backward(ctx, grad_value):
        grad_xy, = ctx.saved_tensors
        return dt_sample_bwd(grad_xy, grad_value.contiguous().float(), ctx.C), None, None


def nearest_site_transform(depth, fg_max):
    """distance_transform with its argument (include/spherehand_hip.h, shr_dt_nearest_fwd): depth [B,H,W] fp32 ->
    (d2 int32 [B,H,W], the bits of distance_transform; nearest int32 [B,H,W]: i' W + j' of the nearest pixel with
    depth < fg_max, the smallest such index among equally near ones, -1 everywhere in an image that has none)."""
    _check_input(depth, "depth")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise RuntimeError("depth must be [B,H,W] with H, W >= 1")
    B, H, W = depth.shape
    lib = _lib.lib()
    with _on(depth.device):
        d2 = torch.empty((B, H, W), dtype=torch.int32, device=depth.device)
        nearest = torch.empty((B, H, W), dtype=torch.int32, device=depth.device)
        ws = torch.empty((max(16, lib.shr_dt_nearest_workspace_bytes(B, H, W)),), dtype=torch.uint8, device=depth.device)
        _lib.check(lib.shr_dt_nearest_fwd(_ptr(depth), B, H, W, float(fg_max), _ptr(d2), _ptr(nearest), _ptr(ws), _stream()),
                   "shr_dt_nearest_fwd")
    return d2, nearest


def _cover_max_dist(max_dist):
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise RuntimeError("max_dist must be >= 0 (inf: no saturation), not %r" % (max_dist,))
    return max_dist


def _cover_shape(observed, d2):
    _check_input(observed, "observed")
    _check_input(d2, "d2", torch.int32)
    if observed.dim() != 3 or observed.shape[1] < 1 or observed.shape[2] < 1:
        raise RuntimeError("observed must be [B,H,W] with H, W >= 1")
    if d2.shape != observed.shape or d2.device != observed.device:
        raise RuntimeError("d2 must be [B,H,W] as observed, on its device")
    return observed.shape


def sil_cover(observed, obs_fg_max, d2, max_dist=float("inf")):
    """The coverage distance (include/spherehand_hip.h, shr_sil_cover_fwd): observed [B,H,W] fp32, d2 [B,H,W] int32 the
    transform of the RENDERED depth -> dist [B,H,W] = min(sqrt(d2), max_dist) where observed < obs_fg_max, 0 elsewhere."""
    B, H, W = _cover_shape(observed, d2)
    max_dist = _cover_max_dist(max_dist)
    with _on(observed.device):
        dist = torch.empty((B, H, W), dtype=torch.float32, device=observed.device)
        _lib.check(_lib.lib().shr_sil_cover_fwd(_ptr(observed), float(obs_fg_max), _ptr(d2), B, H, W, max_dist, _ptr(dist),
                                                _stream()), "shr_sil_cover_fwd")
    return dist


def sil_cover_bwd(observed, obs_fg_max, d2, nearest, owner, vertices, faces, grad_dist, max_dist=float("inf")):
    """sil_cover's backward to the vertices (include/spherehand_hip.h, shr_sil_cover_bwd): d2, nearest from
    nearest_site_transform of the rendered depth, owner [B,H,W] int32, vertices [B,NV,4] and faces [F,3] int32 as
    tri_raster_indexed_owner_fwd gave and took them, grad_dist [B,H,W] -> grad_vertices [B,NV,4] = (du, dv, 0, 0): every
    uncovered observed pixel pulls its nearest rendered pixel's owner face towards itself; deterministic fixed-point
    sums."""
    B, H, W = _cover_shape(observed, d2)
    max_dist = _cover_max_dist(max_dist)
    _check_input(nearest, "nearest", torch.int32)
    _check_input(owner, "owner", torch.int32)
    _check_input(grad_dist, "grad_dist")
    Bv, NV, F = _indexed_shape(vertices, faces)
    for t, name in ((nearest, "nearest"), (owner, "owner"), (grad_dist, "grad_dist")):
        if t.shape != observed.shape or t.device != observed.device:
            raise RuntimeError("%s must be [B,H,W] as observed, on its device" % name)
    if Bv != B or vertices.device != observed.device or faces.device != observed.device:
        raise RuntimeError("vertices must be [B,NV,4] with observed's B, vertices and faces on its device")
    lib = _lib.lib()
    with _on(observed.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=observed.device)
        ws = torch.empty((max(16, lib.shr_sil_cover_bwd_workspace_bytes(B, NV)),), dtype=torch.uint8,
                         device=observed.device)
        _lib.check(lib.shr_sil_cover_bwd(_ptr(observed), float(obs_fg_max), _ptr(d2), _ptr(nearest), _ptr(owner),
                                         _ptr(vertices), _ptr(faces), _ptr(grad_dist), B, NV, F, W, H, max_dist, _ptr(out),
                                         _ptr(ws), _stream()), "shr_sil_cover_bwd")
    return out


class SilhouetteCover(torch.autograd.Function):
    """sil_cover with a backward: (vertices [B,NV,3 or 4] pixel space, faces, owner, d2, nearest, observed, obs_fg_max,
    max_dist) -> dist [B,H,W].  owner, d2 and nearest are those of the render of these vertices
    (tri_raster_indexed_owner_fwd, nearest_site_transform).  Differentiable w.r.t. vertices[..., :2] only: the nearest
    rendered pixel and its weights are held fixed (the z gradient is zero)."""

    @staticmethod
    def forward(ctx, vertices, faces, owner, d2, nearest, observed, obs_fg_max, max_dist=float("inf")):
        v4, ctx.width4 = vertices4(vertices)
        observed = observed.contiguous()
        dist = sil_cover(observed, obs_fg_max, d2, max_dist)
        ctx.obs_fg_max, ctx.max_dist = obs_fg_max, max_dist
        ctx.save_for_backward(v4, faces, owner, d2, nearest, observed)
        return dist

    @staticmethod
    def backward(ctx, grad_dist):
        v4, faces, owner, d2, nearest, observed = ctx.saved_tensors
        g = sil_cover_bwd(observed, ctx.obs_fg_max, d2, nearest, owner, v4, faces, grad_dist.contiguous().float(),
                          ctx.max_dist)
        return _grad_as_given(ctx, g), None, None, None, None, None, None, None


def _d2m_args(observed, vertices, faces, pixel_to_model, max_dist):
    _check_input(observed, "observed")
    if observed.dim() != 3 or observed.shape[1] < 1 or observed.shape[2] < 1:
        raise RuntimeError("observed must be [B,H,W] with H, W >= 1")
    Bv, NV, F = _indexed_shape(vertices, faces)
    if Bv != observed.shape[0] or NV < 1 or vertices.device != observed.device or faces.device != observed.device:
        raise RuntimeError("vertices must be [B,NV,4] with observed's B and NV >= 1, vertices and faces on its device")
    try:
        ax, bx, ay, by = (float(t) for t in pixel_to_model)
    except (TypeError, ValueError):
        raise RuntimeError("pixel_to_model must be four numbers (ax, bx, ay, by): x = ax j + bx, y = ay i + by")
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise RuntimeError("max_dist must be >= 0 (inf: no saturation), not %r" % (max_dist,))
    return observed.shape[0], observed.shape[1], observed.shape[2], NV, F, (ax, bx, ay, by), max_dist


def mesh_data_to_model(observed, vertices, faces, pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf")):
    """The mesh data-to-model distance (include/spherehand_hip.h, shr_mesh_d2m_fwd): observed [B,H,W] fp32, vertices
    [B,NV,4] fp32 in model space, faces [F,3] int32 as given, pixel_to_model = (ax, bx, ay, by) -> (dist [B,H,W] fp32, face
    [B,H,W] int32): at every pixel with observed < fg_max the distance from (ax j + bx, ay i + by, observed) to the closest
    point of the closest triangle, saturated at max_dist, and that triangle's row in faces; 0 and -1 elsewhere."""
    B, H, W, NV, F, p2m, max_dist = _d2m_args(observed, vertices, faces, pixel_to_model, max_dist)
    lib = _lib.lib()
    with _on(observed.device):
        dist = torch.empty((B, H, W), dtype=torch.float32, device=observed.device)
        face = torch.empty((B, H, W), dtype=torch.int32, device=observed.device)
        ws = torch.empty((max(16, lib.shr_mesh_d2m_workspace_bytes(B, F)),), dtype=torch.uint8, device=observed.device)
        _lib.check(lib.shr_mesh_d2m_fwd(_ptr(observed), _ptr(vertices), _ptr(faces), B, NV, F, W, H, *p2m, float(fg_max),
                                        max_dist, _ptr(dist), _ptr(face), _ptr(ws), _stream()), "shr_mesh_d2m_fwd")
    return dist, face


def mesh_data_to_model_bwd(observed, vertices, faces, dist, face, grad_dist, pixel_to_model=(1.0, 0.0, 1.0, 0.0),
                           fg_max=1000.0, max_dist=float("inf")):
    """mesh_data_to_model's backward (include/spherehand_hip.h, shr_mesh_d2m_bwd): dist, face its outputs, grad_dist
    [B,H,W] -> grad_vertices [B,NV,4] = (d/dx, d/dy, d/dz, 0): every data point with 0 < dist < max_dist pushes the three
    corners of its face away from itself (a descent step pulls them towards it) with the closest point's weights;
    deterministic fixed-point sums."""
    B, H, W, NV, F, p2m, max_dist = _d2m_args(observed, vertices, faces, pixel_to_model, max_dist)
    _check_input(dist, "dist")
    _check_input(face, "face", torch.int32)
    _check_input(grad_dist, "grad_dist")
    for t, name in ((dist, "dist"), (face, "face"), (grad_dist, "grad_dist")):
        if t.shape != observed.shape or t.device != observed.device:
            raise RuntimeError("%s must be [B,H,W] as observed, on its device" % name)
    lib = _lib.lib()
    with _on(observed.device):
        out = torch.empty((B, NV, 4), dtype=torch.float32, device=observed.device)
        ws = torch.empty((max(16, lib.shr_mesh_d2m_bwd_workspace_bytes(B, NV)),), dtype=torch.uint8, device=observed.device)
        _lib.check(lib.shr_mesh_d2m_bwd(_ptr(observed), _ptr(vertices), _ptr(faces), _ptr(dist), _ptr(face), _ptr(grad_dist),
                                        B, NV, F, W, H, *p2m, float(fg_max), max_dist, _ptr(out), _ptr(ws), _stream()),
                   "shr_mesh_d2m_bwd")
    return out


class MeshDataToModel(torch.autograd.Function):
    """mesh_data_to_model with a backward: (observed [B,H,W], vertices [B,NV,3 or 4] model space, faces [F,3] int32,
    pixel_to_model, fg_max, max_dist) -> dist [B,H,W].  Differentiable w.r.t. vertices[..., :3]; the closest face of every
    point and the closest point's weights on it are held fixed (the envelope rule: the distance is a minimum over both)."""

    @staticmethod
    def forward(ctx, observed, vertices, faces, pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf")):
        v4, ctx.width4 = vertices4(vertices)
        observed = observed.contiguous()
        dist, face = mesh_data_to_model(observed, v4, faces, pixel_to_model, fg_max, max_dist)
        ctx.args = (tuple(pixel_to_model), fg_max, max_dist)
        ctx.save_for_backward(observed, v4, faces, dist, face)
        ctx.mark_non_differentiable(face)
        return dist, face

    @staticmethod
    def backward(ctx, grad_dist, _grad_face):
        observed, v4, faces, dist, face = ctx.saved_tensors
        g = mesh_data_to_model_bwd(observed, v4, faces, dist, face, grad_dist.contiguous().float(), *ctx.args)
        return None, _grad_as_given(ctx, g), None, None, None, None


def _icp_args(observed, vertices, faces, params, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, pixel_to_model,
              max_dist, name="parameters"):
    B, H, W, NV, F, p2m, max_dist = _d2m_args(observed, vertices, faces, pixel_to_model, max_dist)
    _icp_pose_args(params, B, observed.device, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, NV, name)
    return B, H, W, NV, F, p2m, max_dist


def _icp_pose_args(params, B, dev, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, NV, name="parameters"):
    for t, what in ((params, name), (offset, "offset"), (offset_inv, "offset_inv")):
        _check_input(t, what)
    if tuple(params.shape) != (B, 26) or params.device != dev:
        raise RuntimeError("%s must be [B,26] with observed's B, on its device" % name)
    if tuple(offset.shape) != (17, 4, 4) or tuple(offset_inv.shape) != (17, 4, 4):
        raise RuntimeError("offset and offset_inv must be [17,4,4]")
    if _skin_tables(skin_vertex_start, skin_bone, skin_wv, None) != NV:
        raise RuntimeError("the skin table must have the vertices' NV rows")


def pose_icp_normal(observed, vertices, faces, dist, face, params, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv,
                    right_hand=True, pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf")):
    """The Gauss-Newton normal equations of 1/2 sum dist^2 of the mesh data-to-model distance with respect to the pose
    (include/spherehand_hip.h, shr_pose_icp_normal): dist, face = mesh_data_to_model(observed, vertices, ...) and vertices
    those of `params` in model space (PoseVertices with camera=None; NOT checked) -> (A [B,26,26] fp64, g [B,26] fp64,
    cost [B] fp64 = sum dist^2 over all pixels, count [B] int32 = the contributing points)."""
    B, H, W, NV, F, p2m, max_dist = _icp_args(observed, vertices, faces, params, offset, offset_inv, skin_vertex_start,
                                              skin_bone, skin_wv, pixel_to_model, max_dist)
    _check_input(dist, "dist")
    _check_input(face, "face", torch.int32)
    for t, name in ((dist, "dist"), (face, "face")):
        if t.shape != observed.shape or t.device != observed.device:
            raise RuntimeError("%s must be [B,H,W] as observed, on its device" % name)
    lib = _lib.lib()
    dev = observed.device
    with _on(dev):
        A = torch.empty((B, 26, 26), dtype=torch.float64, device=dev)
        g = torch.empty((B, 26), dtype=torch.float64, device=dev)
        cost = torch.empty((B,), dtype=torch.float64, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(16, lib.shr_pose_icp_normal_workspace_bytes(B, W, H)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.shr_pose_icp_normal(_ptr(observed), _ptr(vertices), _ptr(faces), _ptr(dist), _ptr(face), _ptr(params),
                                           _ptr(offset), _ptr(offset_inv), _ptr(skin_vertex_start), _ptr(skin_bone),
                                           _ptr(skin_wv), int(bool(right_hand)), B, NV, F, W, H, *p2m, float(fg_max), max_dist,
                                           _ptr(A), _ptr(g), _ptr(cost), _ptr(count), _ptr(ws), _stream()),
                   "shr_pose_icp_normal")
    return A, g, cost, count


def _lm_prior_args(prior, stiffness, B):
    """The stiffness term's arguments as every Levenberg-Marquardt step takes them: prior [B,26] and stiffness [26], or None."""
    if prior is not None:
        _check_input(prior, "prior")
        if tuple(prior.shape) != (B, 26):
            raise RuntimeError("prior must be [B,26]")
    if stiffness is not None:
        _check_input(stiffness, "stiffness")
        if tuple(stiffness.shape) != (26,):
            raise RuntimeError("stiffness must be [26]")


def pose_lm_begin(params0, lambda0=1e-3):
    """Start a Levenberg-Marquardt loop on the device (shr_pose_lm_begin): params0 [B,26] -> (state, trial [B,26]): the
    opaque per-crop state pose_lm_step takes and the first pose to evaluate, params0."""
    _check_input(params0, "start parameters")
    if params0.dim() != 2 or params0.shape[1] != 26:
        raise RuntimeError("start parameters must be [B,26]")
    if not float(lambda0) > 0:
        raise RuntimeError("lambda0 must be > 0")
    B = params0.shape[0]
    lib = _lib.lib()
    with _on(params0.device):
        state = torch.empty((max(1, lib.shr_pose_lm_state_bytes(B) // 8),), dtype=torch.float64, device=params0.device)
        trial = torch.empty((B, 26), dtype=torch.float32, device=params0.device)
        _lib.check(lib.shr_pose_lm_begin(_ptr(params0), B, float(lambda0), _ptr(state), _ptr(trial), _stream()),
                   "shr_pose_lm_begin")
    return state, trial


def pose_lm_step(state, A, g, cost_data, trial, prior=None, stiffness=None, solve=True, out=None):
    """One step of the loop (shr_pose_lm_step): A [B,26,26], g [B,26], cost_data [B] fp64 of the pose `trial` [B,26] ->
    (trial_out [B,26] or None without `solve`, params [B,26], cost [B], cost0 [B]).  prior [B,26] (default: the start
    pose) and stiffness [26] add sum_i stiffness_i (p_i - prior_i)^2.  cost0 is written by the first step after
    pose_lm_begin only.  out = (trial_out, params, cost, cost0): buffers to write instead of new ones."""
    _check_input(trial, "trial")
    B = trial.shape[0]
    if trial.dim() != 2 or trial.shape[1] != 26:
        raise RuntimeError("trial must be [B,26]")
    for t, name, shape in ((state, "state", None), (A, "A", (B, 26, 26)), (g, "g", (B, 26)), (cost_data, "cost_data", (B,))):
        _check_input(t, name, torch.float64)
        if (shape is not None and tuple(t.shape) != shape) or t.device != trial.device:
            raise RuntimeError("%s must be %s fp64 on trial's device" % (name, shape))
    lib = _lib.lib()
    if state.numel() * 8 < lib.shr_pose_lm_state_bytes(B):
        raise RuntimeError("state is pose_lm_begin's, for the same B")
    _lm_prior_args(prior, stiffness, B)
    with _on(trial.device):
        if out is None:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=trial.device)   # noqa: E731
            out = (new(B, 26) if solve else None, new(B, 26), new(B), new(B))
        trial_out, params, cost, cost0 = out
        _lib.check(lib.shr_pose_lm_step(_ptr(state), _ptr(A), _ptr(g), _ptr(cost_data), _ptr(trial), _ptr(prior),
                                        _ptr(stiffness), int(bool(solve)), B, _ptr(trial_out) if solve else None, _ptr(params),
                                        _ptr(cost), _ptr(cost0), _stream()), "shr_pose_lm_step")
    return (trial_out if solve else None), params, cost, cost0


def pose_icp(observed, params0, faces, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, right_hand=True,
             pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
             stiffness=None, prior=None):
    """Fit the pose to an observed depth image through the mesh: `iters` Levenberg-Marquardt iterations on
    sum dist^2 + sum_i stiffness_i (p_i - prior_i)^2 from params0 [B,26], dist the mesh data-to-model distance of
    mesh_data_to_model saturated at max_dist -> (params [B,26], cost0 [B], cost [B]).  Each of the iters + 1 evaluations
    is shr_pose_vertices_fwd (model space) -> shr_mesh_d2m_fwd -> shr_pose_icp_normal -> shr_pose_lm_step on torch's
    current stream, into buffers allocated once before the loop; nothing returns to the host: capturable in a graph.
    iters = 0 returns params0 and cost = cost0."""
    _check_input(observed, "observed")
    _check_input(faces, "faces", torch.int32)
    if observed.dim() != 3 or observed.shape[1] < 1 or observed.shape[2] < 1 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("observed must be [B,H,W] with H, W >= 1 and faces [F,3]")
    dev = observed.device
    B, H, W = observed.shape
    NV, F = _skin_tables(skin_vertex_start, skin_bone, skin_wv, None), faces.shape[0]
    verts = torch.empty((B, NV, 4), dtype=torch.float32, device=dev)
    _, _, _, _, _, p2m, max_dist = _icp_args(observed, verts, faces, params0, offset, offset_inv, skin_vertex_start, skin_bone,
                                             skin_wv, pixel_to_model, max_dist, "start parameters")
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    state, trial = pose_lm_begin(params0, lambda0)
    _lm_prior_args(prior, stiffness, B)
    lib = _lib.lib()
    right, fg_max = int(bool(right_hand)), float(fg_max)
    with _on(dev):
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
        dist, face = f32(B, H, W), torch.empty((B, H, W), dtype=torch.int32, device=dev)
        A, g, cost_data, count = f64(B, 26, 26), f64(B, 26), f64(B), torch.empty((B,), dtype=torch.int32, device=dev)
        params, cost0, cost = f32(B, 26), f32(B), f32(B)
        ws_d2m = torch.empty((max(16, lib.shr_mesh_d2m_workspace_bytes(B, F)),), dtype=torch.uint8, device=dev)
        ws_icp = torch.empty((max(16, lib.shr_pose_icp_normal_workspace_bytes(B, W, H)),), dtype=torch.uint8, device=dev)
        stream = _stream()
        for it in range(iters + 1):
            _lib.check(lib.shr_pose_vertices_fwd(_ptr(trial), B, _ptr(offset), _ptr(offset_inv), NV, _ptr(skin_vertex_start),
                                                 _ptr(skin_bone), _ptr(skin_wv), right, 0, 0.0, 0.0, 1.0, 1.0, None,
                                                 _ptr(verts), None, stream), "shr_pose_vertices_fwd")
            _lib.check(lib.shr_mesh_d2m_fwd(_ptr(observed), _ptr(verts), _ptr(faces), B, NV, F, W, H, *p2m, fg_max, max_dist,
                                            _ptr(dist), _ptr(face), _ptr(ws_d2m), stream), "shr_mesh_d2m_fwd")
            _lib.check(lib.shr_pose_icp_normal(_ptr(observed), _ptr(verts), _ptr(faces), _ptr(dist), _ptr(face), _ptr(trial),
                                               _ptr(offset), _ptr(offset_inv), _ptr(skin_vertex_start), _ptr(skin_bone),
                                               _ptr(skin_wv), right, B, NV, F, W, H, *p2m, fg_max, max_dist, _ptr(A), _ptr(g),
                                               _ptr(cost_data), _ptr(count), _ptr(ws_icp), stream), "shr_pose_icp_normal")
            solve = int(it < iters)
            _lib.check(lib.shr_pose_lm_step(_ptr(state), _ptr(A), _ptr(g), _ptr(cost_data), _ptr(trial), _ptr(prior),
                                            _ptr(stiffness), solve, B, _ptr(trial) if solve else None, _ptr(params), _ptr(cost),
                                            _ptr(cost0), stream), "shr_pose_lm_step")
    return params, cost0, cost


def _views_args(view, B, dev, name="view"):
    _check_input(view, name)
    if view.dim() != 4 or view.shape[0] != B or view.shape[1] < 1 or tuple(view.shape[2:]) != (4, 4) or view.device != dev:
        raise RuntimeError("%s must be [B,V,4,4] with V >= 1, on the other tensors' device" % name)
    if B * view.shape[1] > 65535:
        raise RuntimeError("B * V must be at most 65535")
    return view.shape[1]


def view_vertices(vertices, view):
    """Model-space vertices [B,NV,4] taken into every view's frame (include/spherehand_hip.h, shr_view_vertices_fwd):
    view [B,V,4,4] rigid, x_v = R x + t -> [B,V,NV,4] fp32, the 4th float copied."""
    _check_input(vertices, "vertices")
    if vertices.dim() != 3 or vertices.shape[2] != 4 or vertices.shape[1] < 1:
        raise RuntimeError("vertices must be [B,NV,4] with NV >= 1")
    B, NV = vertices.shape[0], vertices.shape[1]
    V = _views_args(view, B, vertices.device)
    with _on(vertices.device):
        out = torch.empty((B, V, NV, 4), dtype=torch.float32, device=vertices.device)
        _lib.check(_lib.lib().shr_view_vertices_fwd(_ptr(vertices), _ptr(view), B, V, NV, _ptr(out), _stream()),
                   "shr_view_vertices_fwd")
    return out


def _icp_views_args(observed, view, name="observed"):
    _check_input(observed, name)
    if observed.dim() != 4 or observed.shape[2] < 1 or observed.shape[3] < 1:
        raise RuntimeError("%s must be [B,V,H,W] with H, W >= 1" % name)
    B, V, H, W = observed.shape
    if _views_args(view, B, observed.device) != V:
        raise RuntimeError("view must be [B,V,4,4] with observed's B and V")
    return B, V, H, W


def pose_icp_normal_views(observed, view_verts, faces, dist, face, view, params, offset, offset_inv, skin_vertex_start, skin_bone,
                          skin_wv, right_hand=True, pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf")):
    """pose_icp_normal summed over V views of every sample (include/spherehand_hip.h, shr_pose_icp_normal_views): observed,
    dist, face [B,V,H,W], view_verts [B,V,NV,4] = view_vertices(vertices of `params`, view), dist and face the maps of
    mesh_data_to_model on the B V crops, view [B,V,4,4] rigid (NOT checked) -> (A [B,26,26], g [B,26], cost [B] fp64 over
    all pixels of all views, count [B] int32)."""
    B, V, H, W = _icp_views_args(observed, view)
    _check_input(view_verts, "view vertices")
    if view_verts.dim() != 4 or tuple(view_verts.shape[:2]) != (B, V) or view_verts.shape[3] != 4:
        raise RuntimeError("view vertices must be [B,V,NV,4]")
    _, _, _, NV, F, p2m, max_dist = _d2m_args(observed.view(B * V, H, W), view_verts.view(B * V, view_verts.shape[2], 4), faces,
                                              pixel_to_model, max_dist)
    _icp_pose_args(params, B, observed.device, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, NV)
    _check_input(dist, "dist")
    _check_input(face, "face", torch.int32)
    for t, name in ((dist, "dist"), (face, "face")):
        if t.shape != observed.shape or t.device != observed.device:
            raise RuntimeError("%s must be [B,V,H,W] as observed, on its device" % name)
    lib = _lib.lib()
    dev = observed.device
    with _on(dev):
        A = torch.empty((B, 26, 26), dtype=torch.float64, device=dev)
        g = torch.empty((B, 26), dtype=torch.float64, device=dev)
        cost = torch.empty((B,), dtype=torch.float64, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(16, lib.shr_pose_icp_normal_views_workspace_bytes(B, V, W, H)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.shr_pose_icp_normal_views(_ptr(observed), _ptr(view_verts), _ptr(faces), _ptr(dist), _ptr(face), _ptr(view),
                                                 _ptr(params), _ptr(offset), _ptr(offset_inv), _ptr(skin_vertex_start),
                                                 _ptr(skin_bone), _ptr(skin_wv), int(bool(right_hand)), B, V, NV, F, W, H, *p2m,
                                                 float(fg_max), max_dist, _ptr(A), _ptr(g), _ptr(cost), _ptr(count), _ptr(ws),
                                                 _stream()), "shr_pose_icp_normal_views")
    return A, g, cost, count


def pose_icp_views(observed, view, params0, faces, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, right_hand=True,
                   pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                   stiffness=None, prior=None):
    """pose_icp on V depth views of every sample: ONE pose params0 [B,26] in the model frame fitted to observed [B,V,H,W],
    view [B,V,4,4] rigid taking the model frame to view v's (x_v = R x + t); each iteration is one Levenberg-Marquardt step
    on the sum of all views' costs -> (params [B,26], cost0 [B], cost [B]).  Each of the iters + 1 evaluations is
    shr_pose_vertices_fwd (model space) -> shr_view_vertices_fwd -> shr_mesh_d2m_fwd (B V crops) ->
    shr_pose_icp_normal_views -> shr_pose_lm_step on torch's current stream, into buffers allocated once before the loop;
    nothing returns to the host: capturable in a graph.  iters = 0 returns params0 and cost = cost0."""
    _check_input(faces, "faces", torch.int32)
    B, V, H, W = _icp_views_args(observed, view)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces must be [F,3]")
    dev = observed.device
    NV, F = _skin_tables(skin_vertex_start, skin_bone, skin_wv, None), faces.shape[0]
    verts = torch.empty((B, NV, 4), dtype=torch.float32, device=dev)
    vverts = torch.empty((B, V, NV, 4), dtype=torch.float32, device=dev)
    _, _, _, _, _, p2m, max_dist = _d2m_args(observed.view(B * V, H, W), vverts.view(B * V, NV, 4), faces, pixel_to_model, max_dist)
    _icp_pose_args(params0, B, dev, offset, offset_inv, skin_vertex_start, skin_bone, skin_wv, NV, "start parameters")
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    state, trial = pose_lm_begin(params0, lambda0)
    _lm_prior_args(prior, stiffness, B)
    lib = _lib.lib()
    right, fg_max = int(bool(right_hand)), float(fg_max)
    with _on(dev):
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
        dist, face = f32(B, V, H, W), torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
        A, g, cost_data, count = f64(B, 26, 26), f64(B, 26), f64(B), torch.empty((B,), dtype=torch.int32, device=dev)
        params, cost0, cost = f32(B, 26), f32(B), f32(B)
        ws_d2m = torch.empty((max(16, lib.shr_mesh_d2m_workspace_bytes(B * V, F)),), dtype=torch.uint8, device=dev)
        ws_icp = torch.empty((max(16, lib.shr_pose_icp_normal_views_workspace_bytes(B, V, W, H)),), dtype=torch.uint8, device=dev)
        stream = _stream()
        for it in range(iters + 1):
            _lib.check(lib.shr_pose_vertices_fwd(_ptr(trial), B, _ptr(offset), _ptr(offset_inv), NV, _ptr(skin_vertex_start),
                                                 _ptr(skin_bone), _ptr(skin_wv), right, 0, 0.0, 0.0, 1.0, 1.0, None,
                                                 _ptr(verts), None, stream), "shr_pose_vertices_fwd")
            _lib.check(lib.shr_view_vertices_fwd(_ptr(verts), _ptr(view), B, V, NV, _ptr(vverts), stream), "shr_view_vertices_fwd")
            _lib.check(lib.shr_mesh_d2m_fwd(_ptr(observed), _ptr(vverts), _ptr(faces), B * V, NV, F, W, H, *p2m, fg_max, max_dist,
                                            _ptr(dist), _ptr(face), _ptr(ws_d2m), stream), "shr_mesh_d2m_fwd")
            _lib.check(lib.shr_pose_icp_normal_views(_ptr(observed), _ptr(vverts), _ptr(faces), _ptr(dist), _ptr(face), _ptr(view),
                                                     _ptr(trial), _ptr(offset), _ptr(offset_inv), _ptr(skin_vertex_start),
                                                     _ptr(skin_bone), _ptr(skin_wv), right, B, V, NV, F, W, H, *p2m, fg_max,
                                                     max_dist, _ptr(A), _ptr(g), _ptr(cost_data), _ptr(count), _ptr(ws_icp),
                                                     stream), "shr_pose_icp_normal_views")
            solve = int(it < iters)
            _lib.check(lib.shr_pose_lm_step(_ptr(state), _ptr(A), _ptr(g), _ptr(cost_data), _ptr(trial), _ptr(prior),
                                            _ptr(stiffness), solve, B, _ptr(trial) if solve else None, _ptr(params), _ptr(cost),
                                            _ptr(cost0), stream), "shr_pose_lm_step")
    return params, cost0, cost


def _weight_arg(value, name):
    """A term's weight as a float: finite and >= 0."""
    value = float(value)
    if not (value >= 0.0 and value < float("inf")):
        raise RuntimeError("%s must be finite and >= 0, not %r" % (name, value))
    return value


def _new_normal(B, dev):
    """(A [B,26,26], g [B,26], cost [B]) fp64, uninitialised: what a *_normal entry writes."""
    return (torch.empty((B, 26, 26), dtype=torch.float64, device=dev), torch.empty((B, 26), dtype=torch.float64, device=dev),
            torch.empty((B,), dtype=torch.float64, device=dev))


def _accumulate_args(accumulate_into, B, dev, where="the parameters' device"):
    """accumulate_into = (A, g, cost) of the other terms, checked; None: new buffers (call under _on(dev))."""
    if accumulate_into is None:
        return None
    A, g, cost = accumulate_into
    for t, name, shape in ((A, "A", (B, 26, 26)), (g, "g", (B, 26)), (cost, "cost", (B,))):
        _check_input(t, name, torch.float64)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("accumulate_into's %s must be %s fp64 on %s" % (name, shape, where))
    return A, g, cost


def _sphere_icp_args(observed, view, params, offset, offset_inv, bone, wv, radii, pixel_to_model, max_dist, name="parameters"):
    B, V, H, W = _icp_views_args(observed, view)
    Bp, J = _ik_tables(params, offset, offset_inv, bone, wv, name)
    _check_input(radii, "radii")
    if tuple(radii.shape) != (J,):
        raise RuntimeError("radii must be [J], one per key-point")
    if Bp != B or any(t.device != observed.device for t in (params, offset, offset_inv, bone, wv, radii)):
        raise RuntimeError("%s must be [B,26] with observed's B, every tensor on observed's device" % name)
    try:
        p2m = tuple(float(t) for t in pixel_to_model)
        ax, bx, ay, by = p2m
    except (TypeError, ValueError):
        raise RuntimeError("pixel_to_model must be four numbers (ax, bx, ay, by): x = ax j + bx, y = ay i + by")
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise RuntimeError("max_dist must be >= 0 (inf: no saturation), not %r" % (max_dist,))
    return B, V, H, W, J, p2m, max_dist


def sphere_icp_normal(observed, view, params, offset, offset_inv, bone, wv, radii, right_hand=True,
                      pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), want_maps=False):
    """The Gauss-Newton normal equations of the sphere model against observed depth (include/spherehand_hip.h,
    shr_sphere_icp_normal): observed [B,V,H,W], view [B,V,4,4] rigid (NOT checked), params [B,26], the key-point tables of
    pose_keypoints_jacobian and radii [J] -> (A [B,26,26], g [B,26], cost [B] fp64 over all pixels of all views, count [B]
    int32, moments [B,J,12] fp64); with want_maps also (dist [B,V,H,W] fp32, owner [B,V,H,W] int32).  Three launches:
    shr_pose_keypoints_jacobian -> shr_view_vertices_fwd -> shr_sphere_icp_normal; every data point meets every sphere, so
    there is no search to run first."""
    B, V, H, W, J, p2m, max_dist = _sphere_icp_args(observed, view, params, offset, offset_inv, bone, wv, radii, pixel_to_model,
                                                    max_dist)
    lib = _lib.lib()
    dev = observed.device
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        centres = torch.empty((B, V, J, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.shr_view_vertices_fwd(_ptr(kp), _ptr(view), B, V, J, _ptr(centres), _stream()), "shr_view_vertices_fwd")
        A, g, cost = _new_normal(B, dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        moments = torch.empty((B, J, 12), dtype=torch.float64, device=dev)
        dist = torch.empty((B, V, H, W), dtype=torch.float32, device=dev) if want_maps else None
        owner = torch.empty((B, V, H, W), dtype=torch.int32, device=dev) if want_maps else None
        ws = torch.empty((max(16, lib.shr_sphere_icp_normal_workspace_bytes(B, V, J, W, H)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.shr_sphere_icp_normal(_ptr(observed), _ptr(centres), _ptr(radii), _ptr(view), _ptr(jac), B, V, J, W, H,
                                             *p2m, float(fg_max), max_dist, _ptr(A), _ptr(g), _ptr(cost), _ptr(count),
                                             _ptr(moments), _ptr(dist), _ptr(owner), _ptr(ws), _stream()),
                   "shr_sphere_icp_normal")
    return (A, g, cost, count, moments) + ((dist, owner) if want_maps else ())


def sphere_icp(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand=True,
               pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
               stiffness=None, prior=None):
    """Fit the pose to V observed depth views through the SPHERE model: `iters` Levenberg-Marquardt iterations on
    sum dist^2 + sum_i stiffness_i (p_i - prior_i)^2 from params0 [B,26], dist = min_j | |p - c_j| - r_j | saturated at
    max_dist, over all views -> (params [B,26], cost0 [B], cost [B]).  observed [B,V,H,W], view [B,V,4,4] rigid taking the
    model frame to view v's.  Each of the iters + 1 evaluations is shr_pose_keypoints_jacobian -> shr_view_vertices_fwd
    (NV := J) -> shr_sphere_icp_normal -> shr_pose_lm_step on torch's current stream, into buffers allocated once before
    the loop; nothing returns to the host: capturable in a graph.  iters = 0 returns params0 and cost = cost0."""
    return sphere_icp_priors(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand, pixel_to_model, fg_max,
                             max_dist, iters, lambda0, stiffness, prior, render_weight=0.0)

def _sphere_render_args(max_resid, background, weight, name="weight"):
    max_resid, background, weight = float(max_resid), float(background), float(weight)
    if not max_resid >= 0.0:
        raise RuntimeError("max_resid must be >= 0 (inf: no saturation), not %r" % (max_resid,))
    if not abs(background) < float("inf"):
        raise RuntimeError("background must be finite, not %r" % (background,))
    return max_resid, background, _weight_arg(weight, name)


def sphere_render_normal(observed, view, params, offset, offset_inv, bone, wv, radii, right_hand=True,
                         pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_resid=float("inf"), background=100.0,
                         weight=1.0, accumulate_into=None, want_maps=False):
    """The Gauss-Newton normal equations of the RENDERED sphere model against observed depth, the model-to-data term
    (include/spherehand_hip.h, shr_sphere_render_normal): sphere_icp_normal's arguments -> (A [B,26,26], g [B,26], cost [B]
    fp64 over all pixels of all views, count [B] int32, moments [B,J,12] fp64); with want_maps also (depth [B,V,H,W] fp32,
    owner [B,V,H,W] int32), the render and its owners.  A, g and cost are `weight` x the term's; count and moments are the
    term's own.  accumulate_into = (A, g, cost) of sphere_icp_normal at the same pose: weight x the term is ADDED to them in
    place (with weight = 0 they are not touched) and they are the A, g, cost returned.  Three launches:
    shr_pose_keypoints_jacobian -> shr_view_vertices_fwd -> shr_sphere_render_normal."""
    B, V, H, W, J, p2m, _ = _sphere_icp_args(observed, view, params, offset, offset_inv, bone, wv, radii, pixel_to_model, 0.0)
    max_resid, background, weight = _sphere_render_args(max_resid, background, weight)
    dev = observed.device
    into = _accumulate_args(accumulate_into, B, dev, "observed's device")
    lib = _lib.lib()
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        centres = torch.empty((B, V, J, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.shr_view_vertices_fwd(_ptr(kp), _ptr(view), B, V, J, _ptr(centres), _stream()), "shr_view_vertices_fwd")
        A, g, cost = into or _new_normal(B, dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        moments = torch.empty((B, J, 12), dtype=torch.float64, device=dev)
        depth = torch.empty((B, V, H, W), dtype=torch.float32, device=dev) if want_maps else None
        owner = torch.empty((B, V, H, W), dtype=torch.int32, device=dev) if want_maps else None
        ws = torch.empty((max(16, lib.shr_sphere_render_normal_workspace_bytes(B, V, J, W, H)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.shr_sphere_render_normal(_ptr(observed), _ptr(centres), _ptr(radii), _ptr(view), _ptr(jac), B, V, J, W, H,
                                                *p2m, float(fg_max), background, max_resid, weight,
                                                int(accumulate_into is not None), _ptr(A), _ptr(g), _ptr(cost), _ptr(count),
                                                _ptr(moments), _ptr(depth), _ptr(owner), _ptr(ws), _stream()),
                   "shr_sphere_render_normal")
    return (A, g, cost, count, moments) + ((depth, owner) if want_maps else ())


def sphere_icp_render(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand=True,
                      pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                      stiffness=None, prior=None, render_weight=1.0, max_resid=float("inf"), background=100.0):
    """sphere_icp with the model-to-data term: `iters` Levenberg-Marquardt iterations on
    sum dist^2 + render_weight sum min(|D - O'|, max_resid)^2 + sum_i stiffness_i (p_i - prior_i)^2, D the sphere render of
    the pose (background where no sphere is hit), O' the observation with its background set to `background`, over all
    pixels of all views -> (params [B,26], cost0 [B], cost [B]).  Each of the iters + 1 evaluations is sphere_icp's with
    shr_sphere_render_normal(accumulate = 1) after shr_sphere_icp_normal, on torch's current stream, into buffers allocated
    once before the loop; nothing returns to the host: capturable in a graph.  render_weight = 0 issues no launch of the
    new entry: sphere_icp bit for bit."""
    return sphere_icp_priors(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand, pixel_to_model, fg_max,
                             max_dist, iters, lambda0, stiffness, prior, render_weight, max_resid, background)

def _sphere_prior_args(B, V, J, dev, keypoints, confidence, kp_weight, kp_max, limits, limit_weight):
    kp_weight, kp_max, limit_weight = float(kp_weight), float(kp_max), float(limit_weight)
    kp_weight, limit_weight = _weight_arg(kp_weight, "kp_weight"), _weight_arg(limit_weight, "limit_weight")
    if not kp_max >= 0.0:
        raise RuntimeError("kp_max must be >= 0 (inf: no saturation), not %r" % (kp_max,))
    if confidence is not None and keypoints is None:
        raise RuntimeError("confidence without keypoints")
    if keypoints is not None:
        _check_input(keypoints, "keypoints")
        if tuple(keypoints.shape) != (B, V, J, 3) or keypoints.device != dev:
            raise RuntimeError("keypoints must be [B,V,J,3], in each view's frame, on observed's device")
    if confidence is not None:
        _check_input(confidence, "confidence")
        if tuple(confidence.shape) != (B, V, J) or confidence.device != dev:
            raise RuntimeError("confidence must be [B,V,J] on observed's device")
    lower = upper = None
    if limits is not None:
        try:
            lower, upper = limits
        except (TypeError, ValueError):
            raise RuntimeError("limits must be (lower [26], upper [26])")
        for t, name in ((lower, "lower"), (upper, "upper")):
            _check_input(t, name)
            if tuple(t.shape) != (26,) or t.device != dev:
                raise RuntimeError("limits' %s must be [26] on observed's device" % name)
    return kp_weight, kp_max, limit_weight, lower, upper


def sphere_prior_normal(view, params, offset, offset_inv, bone, wv, right_hand=True, keypoints=None, confidence=None,
                        kp_weight=1.0, kp_max=float("inf"), limits=None, limit_weight=0.0, accumulate_into=None):
    """The normal equations of the sphere fit's keypoint and joint-limit terms (include/spherehand_hip.h,
    shr_sphere_prior_normal): view [B,V,4,4], params [B,26], the key-point tables of pose_keypoints_jacobian, keypoints
    [B,V,J,3] in each view's frame (None: no keypoint term), confidence [B,V,J] >= 0 (None: 1), limits = (lower [26],
    upper [26]) (None: no limit term) -> (A [B,26,26], g [B,26], cost [B] fp64, count [B,2] int32: pairs with rows and limit
    rows, moments [B,J,12] fp64).  A, g and cost carry kp_weight and limit_weight; count and moments are the terms' own.
    accumulate_into = (A, g, cost) of the image terms at the same pose: the terms are ADDED to them in place (with no
    weighted term they are not touched) and they are the A, g, cost returned.  Three launches:
    shr_pose_keypoints_jacobian -> shr_view_vertices_fwd -> shr_sphere_prior_normal."""
    Bp, J = _ik_tables(params, offset, offset_inv, bone, wv, "parameters")
    dev = params.device
    B, V = Bp, (view.shape[1] if torch.is_tensor(view) and view.dim() == 4 else 0)
    _views_args(view, B, dev)
    if any(t.device != dev for t in (offset, offset_inv, bone, wv)):
        raise RuntimeError("every tensor must be on the parameters' device")
    kp_weight, kp_max, limit_weight, lower, upper = _sphere_prior_args(B, V, J, dev, keypoints, confidence, kp_weight, kp_max,
                                                                       limits, limit_weight)
    into = _accumulate_args(accumulate_into, B, dev)
    lib = _lib.lib()
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        centres = torch.empty((B, V, J, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.shr_view_vertices_fwd(_ptr(kp), _ptr(view), B, V, J, _ptr(centres), _stream()), "shr_view_vertices_fwd")
        A, g, cost = into or _new_normal(B, dev)
        count = torch.empty((B, 2), dtype=torch.int32, device=dev)
        moments = torch.empty((B, J, 12), dtype=torch.float64, device=dev)
        _lib.check(lib.shr_sphere_prior_normal(_ptr(centres), _ptr(view), _ptr(jac), _ptr(params), _ptr(keypoints),
                                               _ptr(confidence), kp_weight, kp_max, _ptr(lower), _ptr(upper), limit_weight,
                                               B, V, J, int(accumulate_into is not None), _ptr(A), _ptr(g), _ptr(cost),
                                               _ptr(count), _ptr(moments), None, _stream()), "shr_sphere_prior_normal")
    return A, g, cost, count, moments


def _sphere_collision_args(J, dev, pairs, weight, name="weight"):
    """(pair_a, pair_b, pair_min, K, weight): pairs = (a [K] int32, b [K] int32, m [K] fp32) on `dev`, or None (K = 0).
    hand_model.collision_table validates the table where it is built; the entry skips a bad pair."""
    weight = _weight_arg(weight, name)
    if pairs is None:
        return None, None, None, 0, weight
    try:
        a, b, m = pairs
    except (TypeError, ValueError):
        raise RuntimeError("pairs must be (a [K] int32, b [K] int32, min_dist [K] float32)")
    _check_input(a, "pairs' a", torch.int32)
    _check_input(b, "pairs' b", torch.int32)
    _check_input(m, "pairs' min_dist")
    K = a.shape[0] if a.dim() == 1 else -1
    if K < 0 or tuple(b.shape) != (K,) or tuple(m.shape) != (K,) or any(t.device != dev for t in (a, b, m)):
        raise RuntimeError("pairs must be three [K] tensors on the parameters' device")
    if K > 4096:
        raise RuntimeError("at most 4096 pairs, not %d" % K)
    if K == 0:
        return None, None, None, 0, weight
    return a, b, m, K, weight


def sphere_collision_normal(params, offset, offset_inv, bone, wv, right_hand=True, pairs=None, weight=1.0,
                            accumulate_into=None):
    """The normal equations of the sphere fit's collision term (include/spherehand_hip.h, shr_sphere_collision_normal):
    params [B,26], the key-point tables of pose_keypoints_jacobian, pairs = (a [K] int32, b [K] int32, m [K] fp32), the
    table of hand_model.collision_table (None: no pair) -> (A [B,26,26], g [B,26], cost [B] fp64, count [B] int32: the pairs
    with rows, penetration [B,K] fp64: h = m - |c_a - c_b| at an active pair, 0 elsewhere).  A, g and cost carry `weight`;
    count and penetration are the term's own.  The term is view-independent: it reads the model-frame keypoints.
    accumulate_into = (A, g, cost) of the other terms at the same pose: weight x the term is ADDED to them in place (with
    weight = 0 or no pair they are not touched) and they are the A, g, cost returned.  Two launches:
    shr_pose_keypoints_jacobian -> shr_sphere_collision_normal."""
    B, J = _ik_tables(params, offset, offset_inv, bone, wv, "parameters")
    dev = params.device
    if any(t.device != dev for t in (offset, offset_inv, bone, wv)):
        raise RuntimeError("every tensor must be on the parameters' device")
    pa, pb, pm, K, weight = _sphere_collision_args(J, dev, pairs, weight)
    into = _accumulate_args(accumulate_into, B, dev)
    lib = _lib.lib()
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        A, g, cost = into or _new_normal(B, dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        penetration = torch.empty((B, K), dtype=torch.float64, device=dev)
        _lib.check(lib.shr_sphere_collision_normal(_ptr(kp), _ptr(jac), _ptr(pa), _ptr(pb), _ptr(pm), weight, B, J, K,
                                                   int(accumulate_into is not None), _ptr(A), _ptr(g), _ptr(cost), _ptr(count),
                                                   _ptr(penetration) if K else None, None, _stream()),
                   "shr_sphere_collision_normal")
    return A, g, cost, count, penetration


def _pose_vae_args(J, dev, blob, weight, latent_weight, name="weight"):
    """(blob, weight, latent_weight) of the pose-VAE term: the blob of pose_vae.pack_fit_weights on `dev`."""
    weight, latent_weight = float(weight), float(latent_weight)
    weight, latent_weight = _weight_arg(weight, name), _weight_arg(latent_weight, "latent_weight")
    if J != 41:
        raise RuntimeError("the pose-VAE term is built for the hand's 41 spheres, not %d" % J)
    _check_input(blob, "the pose-VAE blob")
    if blob.dim() != 1 or blob.shape[0] != _lib.lib().shr_pose_vae_blob_floats() or blob.device != dev:
        raise RuntimeError("the pose-VAE blob must be pose_vae.pack_fit_weights' [%d] on the parameters' device"
                           % _lib.lib().shr_pose_vae_blob_floats())
    return blob, weight, latent_weight


def _pose_prior_args(J, dev, pose_prior):
    """The loops' pose_prior = (blob, weight, latent_weight) checked, or None where the loop issues no launch of the entry
    (no prior, or weight 0)."""
    if pose_prior is None:
        return None
    try:
        blob, weight, latent_weight = pose_prior
    except (TypeError, ValueError):
        raise RuntimeError("pose_prior must be (blob, weight, latent_weight)")
    blob, weight, latent_weight = _pose_vae_args(J, dev, blob, weight, latent_weight, "pose_prior's weight")
    return (blob, weight, latent_weight) if weight > 0.0 else None


def pose_vae_normal(params, offset, offset_inv, bone, wv, right_hand, blob, weight, latent_weight=0.0, accumulate_into=None):
    """The normal equations of the sphere fit's pose-VAE prior (include/spherehand_hip.h, shr_pose_vae_normal): params
    [B,26], the key-point tables of pose_keypoints_jacobian (J = 41), blob = pose_vae.pack_fit_weights(module) ->
    (A [B,26,26], g [B,26], cost [B] fp64, residual [B,123] fp64: r = c - 100 recon(c / 100) in mm, latent [B,32] fp64: mu,
    relu_mask [B,32] int32: the 1024 ReLU decisions of the value column, the header's bit order).  A, g and cost carry
    `weight` and the latent rows `latent_weight` on top; residual, latent and relu_mask are the term's own.
    accumulate_into = (A, g, cost) of the other terms at the same pose: weight x the term is ADDED to them in place and they
    are the A, g, cost returned.  With weight = 0 the three are not touched (without accumulate_into they come back
    uninitialised).  Two launches: shr_pose_keypoints_jacobian -> shr_pose_vae_normal."""
    B, J = _ik_tables(params, offset, offset_inv, bone, wv, "parameters")
    dev = params.device
    if any(t.device != dev for t in (offset, offset_inv, bone, wv)):
        raise RuntimeError("every tensor must be on the parameters' device")
    blob, weight, latent_weight = _pose_vae_args(J, dev, blob, weight, latent_weight)
    into = _accumulate_args(accumulate_into, B, dev)
    lib = _lib.lib()
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        A, g, cost = into or _new_normal(B, dev)
        residual = torch.empty((B, 123), dtype=torch.float64, device=dev)
        latent = torch.empty((B, 32), dtype=torch.float64, device=dev)
        relu_mask = torch.empty((B, 32), dtype=torch.int32, device=dev)
        _lib.check(lib.shr_pose_vae_normal(_ptr(kp), _ptr(jac), _ptr(blob), blob.shape[0], weight, latent_weight, B, J,
                                           int(accumulate_into is not None), _ptr(A), _ptr(g), _ptr(cost), _ptr(residual),
                                           _ptr(latent), _ptr(relu_mask), None, _stream()), "shr_pose_vae_normal")
    return A, g, cost, residual, latent, relu_mask


class _FrameTerms:
    """One evaluation of the per-frame terms of the sphere fit at a trial pose, for the loops (sphere_icp_priors and through
    it sphere_icp and sphere_icp_render, the sequence loops, sphere_icp_calibrate).  The constructor checks the terms'
    arguments in the loops' order and decides which terms carry a weight; allocate() makes, once, the buffers every evaluation
    writes -- kp, jac, centres, A, g, cost_data, the row counters and the image terms' shared workspace --; evaluate() issues
    shr_pose_keypoints_jacobian -> shr_view_vertices_fwd -> the data term (shr_sphere_icp_normal, or with group_size
    shr_sphere_icp_radii_normal) -> render -> keypoints and limits -> collision -> pose-VAE, each later term with
    accumulate = 1 and none for a term without a weight.  Afterwards A, g and cost_data hold the frame's equations."""

    def __init__(self, observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand, pixel_to_model, fg_max, max_dist,
                 render_weight=0.0, max_resid=float("inf"), background=100.0, keypoints=None, confidence=None, kp_weight=0.0,
                 kp_max=float("inf"), limits=None, limit_weight=0.0, collision=None, collision_weight=0.0, pose_prior=None,
                 group_size=None):
        if group_size is None:
            B, V, H, W, J, p2m, max_dist = _sphere_icp_args(observed, view, params0, offset, offset_inv, bone, wv, radii,
                                                            pixel_to_model, max_dist, "start parameters")
            self.N = self.G = None
        else:                                                  # radii [G,J]: the start of the groups' tables
            B, V, H, W, J, self.N, self.G, p2m, max_dist = _sphere_radii_args(
                observed, view, params0, offset, offset_inv, bone, wv, radii, group_size, pixel_to_model, max_dist,
                "start parameters")
        self.max_resid, self.background, self.render_weight = _sphere_render_args(max_resid, background, render_weight,
                                                                                  "render_weight")
        self.dev = dev = observed.device
        self.kp_weight, self.kp_max, self.limit_weight, self.lower, self.upper = _sphere_prior_args(
            B, V, J, dev, keypoints, confidence, kp_weight, kp_max, limits, limit_weight)
        self.priors = (keypoints is not None and self.kp_weight > 0.0) or (self.lower is not None and self.limit_weight > 0.0)
        self.pairs = _sphere_collision_args(J, dev, collision, collision_weight, "collision_weight")
        self.collide = self.pairs[3] > 0 and self.pairs[4] > 0.0
        self.vae = _pose_prior_args(J, dev, pose_prior)
        self.dims, self.p2m, self.fg_max, self.max_dist = (B, V, J, W, H), p2m, float(fg_max), max_dist
        self.right = int(bool(right_hand))
        self.tables = (offset, offset_inv, bone, wv)
        self.observed, self.view, self.radii, self.keypoints, self.confidence = observed, view, radii, keypoints, confidence

    def allocate(self):
        """The evaluation's buffers (call under _on(self.dev))."""
        B, V, J, W, H = self.dims
        lib, dev = _lib.lib(), self.dev
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        rows = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)    # noqa: E731
        self.kp, self.jac, self.centres = f32(B, J, 4), f32(B, 3 * J, 26), f32(B, V, J, 4)
        self.A, self.g, self.cost_data = _new_normal(B, dev)
        self.count = rows(B)
        if self.G is not None:
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
            self.C, self.R, self.gs = f64(B, 26, J), f64(self.G, J, J), f64(self.G, J)
            ws_bytes = lib.shr_sphere_icp_radii_normal_workspace_bytes(B, V, J, W, H)
        else:
            ws_bytes = lib.shr_sphere_icp_normal_workspace_bytes(B, V, J, W, H)
        if self.render_weight > 0.0:
            # (one workspace: the two entries' formulas agree, and each writes it before it reads it)
            ws_bytes = max(ws_bytes, lib.shr_sphere_render_normal_workspace_bytes(B, V, J, W, H))
            self.model_rows = rows(B)
        if self.priors:
            self.prior_rows = rows(B, 2)
        if self.collide:
            self.pair_rows = rows(B)
        self.ws = torch.empty((max(16, ws_bytes),), dtype=torch.uint8, device=dev)

    def evaluate(self, trial, stream, radii=None):
        """The frame's terms at trial [B,26]; radii: the trial tables [G,J] of a fit with group_size."""
        B, V, J, W, H = self.dims
        lib = _lib.lib()
        offset, offset_inv, bone, wv = self.tables
        observed, view, kp, jac, centres = self.observed, self.view, self.kp, self.jac, self.centres
        A, g, cost_data = self.A, self.g, self.cost_data
        _lib.check(lib.shr_pose_keypoints_jacobian(_ptr(trial), B, _ptr(offset), _ptr(offset_inv), J, _ptr(bone), _ptr(wv),
                                                   self.right, _ptr(kp), _ptr(jac), stream), "shr_pose_keypoints_jacobian")
        _lib.check(lib.shr_view_vertices_fwd(_ptr(kp), _ptr(view), B, V, J, _ptr(centres), stream), "shr_view_vertices_fwd")
        if self.G is None:
            _lib.check(lib.shr_sphere_icp_normal(_ptr(observed), _ptr(centres), _ptr(self.radii), _ptr(view), _ptr(jac), B, V, J, W,
                                                 H, *self.p2m, self.fg_max, self.max_dist, _ptr(A), _ptr(g), _ptr(cost_data),
                                                 _ptr(self.count), None, None, None, _ptr(self.ws), stream),
                       "shr_sphere_icp_normal")
        else:
            _lib.check(lib.shr_sphere_icp_radii_normal(_ptr(observed), _ptr(centres), _ptr(radii), _ptr(view), _ptr(jac), B, V, J,
                                                       W, H, self.N, *self.p2m, self.fg_max, self.max_dist, _ptr(A), _ptr(g),
                                                       _ptr(cost_data), _ptr(self.count), _ptr(self.C), _ptr(self.R),
                                                       _ptr(self.gs), None, None, None, _ptr(self.ws), stream),
                       "shr_sphere_icp_radii_normal")
        if self.render_weight > 0.0:
            _lib.check(lib.shr_sphere_render_normal(_ptr(observed), _ptr(centres), _ptr(self.radii), _ptr(view), _ptr(jac), B, V, J,
                                                    W, H, *self.p2m, self.fg_max, self.background, self.max_resid,
                                                    self.render_weight, 1, _ptr(A), _ptr(g), _ptr(cost_data),
                                                    _ptr(self.model_rows), None, None, None, _ptr(self.ws), stream),
                       "shr_sphere_render_normal")
        if self.priors:
            _lib.check(lib.shr_sphere_prior_normal(_ptr(centres), _ptr(view), _ptr(jac), _ptr(trial), _ptr(self.keypoints),
                                                   _ptr(self.confidence), self.kp_weight, self.kp_max, _ptr(self.lower),
                                                   _ptr(self.upper), self.limit_weight, B, V, J, 1, _ptr(A), _ptr(g),
                                                   _ptr(cost_data), _ptr(self.prior_rows), None, None, stream),
                       "shr_sphere_prior_normal")
        if self.collide:                                       # (kp: the trial's keypoints in the MODEL frame)
            pair_a, pair_b, pair_min, K, collision_weight = self.pairs
            _lib.check(lib.shr_sphere_collision_normal(_ptr(kp), _ptr(jac), _ptr(pair_a), _ptr(pair_b), _ptr(pair_min),
                                                       collision_weight, B, J, K, 1, _ptr(A), _ptr(g), _ptr(cost_data),
                                                       _ptr(self.pair_rows), None, None, stream), "shr_sphere_collision_normal")
        if self.vae is not None:
            blob, weight, latent_weight = self.vae
            _lib.check(lib.shr_pose_vae_normal(_ptr(kp), _ptr(jac), _ptr(blob), blob.shape[0], weight, latent_weight, B, J, 1,
                                               _ptr(A), _ptr(g), _ptr(cost_data), None, None, None, None, stream),
                       "shr_pose_vae_normal")


def sphere_icp_priors(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand=True,
                      pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                      stiffness=None, prior=None, render_weight=1.0, max_resid=float("inf"), background=100.0,
                      keypoints=None, confidence=None, kp_weight=1.0, kp_max=float("inf"), limits=None, limit_weight=0.0,
                      collision=None, collision_weight=0.0, pose_prior=None):
    """sphere_icp_render with the keypoint and joint-limit terms: `iters` Levenberg-Marquardt iterations on
    sphere_icp_render's energy + kp_weight sum w min(|k - c|, kp_max)^2 + limit_weight sum_i h_i^2, k the predicted
    keypoints [B,V,J,3] in each view's frame with confidence w [B,V,J] (None: 1), c the sphere centres in that frame, h_i the
    distance of parameter i beyond limits = (lower [26], upper [26]) -> (params [B,26], cost0 [B], cost [B]).  Each of the
    iters + 1 evaluations is sphere_icp_render's with shr_sphere_prior_normal(accumulate = 1) after the render entry, on
    torch's current stream, into buffers allocated once before the loop; nothing returns to the host: capturable in a
    graph.  With no weighted term (both weights 0, or neither keypoints nor limits) it issues no launch of the new entry:
    sphere_icp_render bit for bit.
    collision = (a [K] int32, b [K] int32, m [K] fp32), hand_model.collision_table's pairs, with collision_weight > 0 adds
    collision_weight sum_k max(m_k - |c_a - c_b|, 0)^2 over the model-frame centres: shr_sphere_collision_normal
    (accumulate = 1) after the prior entry in every evaluation.  Without a weighted collision term no launch of it is
    issued and the loop is what it is without the two arguments, bit for bit.
    pose_prior = (blob, weight, latent_weight), the pose-VAE prior (pose_vae_normal) with weight > 0, adds
    weight (sum r^2 + latent_weight sum mu^2): shr_pose_vae_normal (accumulate = 1) after the collision entry in every
    evaluation.  With pose_prior = None or weight = 0 no launch of it is issued: the loop without the argument, bit for bit."""
    terms = _FrameTerms(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand, pixel_to_model, fg_max, max_dist,
                        render_weight, max_resid, background, keypoints, confidence, kp_weight, kp_max, limits, limit_weight,
                        collision, collision_weight, pose_prior)
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    B, dev = terms.dims[0], terms.dev
    state, trial = pose_lm_begin(params0, lambda0)
    _lm_prior_args(prior, stiffness, B)
    lib = _lib.lib()
    with _on(dev):
        terms.allocate()
        params, cost0, cost = (torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((B, 26), (B,), (B,)))
        stream = _stream()
        for it in range(iters + 1):
            terms.evaluate(trial, stream)
            solve = int(it < iters)
            _lib.check(lib.shr_pose_lm_step(_ptr(state), _ptr(terms.A), _ptr(terms.g), _ptr(terms.cost_data), _ptr(trial),
                                            _ptr(prior), _ptr(stiffness), solve, B, _ptr(trial) if solve else None, _ptr(params),
                                            _ptr(cost), _ptr(cost0), stream), "shr_pose_lm_step")
    return params, cost0, cost

def _sphere_temporal_args(B, dev, seq_len, temporal_weight, ts_max, frame_weight):
    try:
        T = int(seq_len)
    except (TypeError, ValueError):
        raise RuntimeError("seq_len must be an integer >= 1")
    if T < 1 or B % T != 0:
        raise RuntimeError("seq_len must be >= 1 and divide the %d frames of the batch, not %r" % (B, seq_len))
    temporal_weight, ts_max = float(temporal_weight), float(ts_max)
    temporal_weight = _weight_arg(temporal_weight, "temporal_weight")
    if not ts_max >= 0.0:
        raise RuntimeError("ts_max must be >= 0 (inf: no saturation), not %r" % (ts_max,))
    if frame_weight is not None:
        _check_input(frame_weight, "frame_weight")
        if tuple(frame_weight.shape) != (B,) or frame_weight.device != dev:
            raise RuntimeError("frame_weight must be [B] on the parameters' device")
    return T, temporal_weight, ts_max


def sphere_temporal_normal(params, offset, offset_inv, bone, wv, seq_len, right_hand=True, temporal_weight=1.0,
                           ts_max=float("inf"), frame_weight=None, accumulate_into=None):
    """The normal equations of the sphere fit's temporal term (include/spherehand_hip.h, shr_sphere_temporal_normal):
    params [B,26], B = S seq_len frames with the frames of a sequence adjacent, the key-point tables of
    pose_keypoints_jacobian -> (A [B,26,26] the diagonal blocks, g [B,26], E [B,26,26] the off-diagonal blocks (frame t's rows,
    frame t + 1's columns; +0 for the last frame of a sequence), cost [B] fp64 (a pair's cost at its later frame), count [B]
    int32: the spheres with rows of the pair ending at the frame).  The term is temporal_weight frame_weight[t]
    sum_j min(|c_j(t + 1) - c_j(t)|, ts_max)^2 over the model-frame centres; frame_weight [B] >= 0 (None: 1) weighs the pair
    (t, t + 1) at t.  accumulate_into = (A, g, cost) of the per-frame terms at the same poses: the term is ADDED to them in
    place (a frame without a weighted pair is not touched) and they are the A, g, cost returned; E is always new.  Two
    launches: shr_pose_keypoints_jacobian -> shr_sphere_temporal_normal."""
    B, J = _ik_tables(params, offset, offset_inv, bone, wv, "parameters")
    dev = params.device
    if any(t.device != dev for t in (offset, offset_inv, bone, wv)):
        raise RuntimeError("every tensor must be on the parameters' device")
    T, temporal_weight, ts_max = _sphere_temporal_args(B, dev, seq_len, temporal_weight, ts_max, frame_weight)
    into = _accumulate_args(accumulate_into, B, dev)
    lib = _lib.lib()
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        A, g, cost = into or _new_normal(B, dev)
        E = torch.empty((B, 26, 26), dtype=torch.float64, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.shr_sphere_temporal_normal(_ptr(kp), _ptr(jac), _ptr(frame_weight), temporal_weight, ts_max, B, T, J,
                                                  int(accumulate_into is not None), _ptr(A), _ptr(g), _ptr(E), _ptr(cost),
                                                  _ptr(count), None, _stream()), "shr_sphere_temporal_normal")
    return A, g, E, cost, count


def _lm_band_begin(entry, params0, seq_len, lambda0):
    """pose_lm_seq_begin / pose_lm_seq2_begin: `entry` names the C entry, whose state size is shr_<entry>_state_bytes."""
    _check_input(params0, "start parameters")
    if params0.dim() != 2 or params0.shape[1] != 26:
        raise RuntimeError("start parameters must be [B,26]")
    if not float(lambda0) > 0:
        raise RuntimeError("lambda0 must be > 0")
    B = params0.shape[0]
    T = _sphere_temporal_args(B, params0.device, seq_len, 0.0, 0.0, None)[0]
    lib = _lib.lib()
    with _on(params0.device):
        state = torch.empty((max(1, getattr(lib, "shr_%s_state_bytes" % entry)(B) // 8),), dtype=torch.float64,
                            device=params0.device)
        trial = torch.empty((B, 26), dtype=torch.float32, device=params0.device)
        _lib.check(getattr(lib, "shr_%s_begin" % entry)(_ptr(params0), B, T, float(lambda0), _ptr(state), _ptr(trial), _stream()),
                   "shr_%s_begin" % entry)
    return state, trial


def _lm_band_step(entry, state, A, g, E, F, cost_data, trial, seq_len, prior, stiffness, solve, out, workspace):
    """pose_lm_seq_step / pose_lm_seq2_step: `entry` names the C entry; F = () for the entry that takes none, else a 1-tuple."""
    _check_input(trial, "trial")
    B = trial.shape[0]
    if trial.dim() != 2 or trial.shape[1] != 26:
        raise RuntimeError("trial must be [B,26]")
    T = _sphere_temporal_args(B, trial.device, seq_len, 0.0, 0.0, None)[0]
    if E is None and T > 1:
        raise RuntimeError("E is needed with seq_len > 1")
    for t, name, shape in ((state, "state", None), (A, "A", (B, 26, 26)), (g, "g", (B, 26)), (E, "E", (B, 26, 26))) + \
            tuple((f, "F", (B, 26, 26)) for f in F) + ((cost_data, "cost_data", (B,)),):
        if t is None:
            continue
        _check_input(t, name, torch.float64)
        if (shape is not None and tuple(t.shape) != shape) or t.device != trial.device:
            raise RuntimeError("%s must be %s fp64 on trial's device" % (name, shape))
    lib = _lib.lib()
    if state.numel() * 8 < getattr(lib, "shr_%s_state_bytes" % entry)(B):
        raise RuntimeError("state is %s_begin's, for the same B" % entry)
    _lm_prior_args(prior, stiffness, B)
    S = B // T
    with _on(trial.device):
        if out is None:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=trial.device)   # noqa: E731
            out = (new(B, 26) if solve else None, new(B, 26), new(S), new(S))
        if workspace is None and solve:
            workspace = torch.empty((max(1, getattr(lib, "shr_%s_workspace_bytes" % entry)(B) // 8),), dtype=torch.float64,
                                    device=trial.device)
        trial_out, params, cost, cost0 = out
        _lib.check(getattr(lib, "shr_%s_step" % entry)(_ptr(state), _ptr(A), _ptr(g), _ptr(E), *(_ptr(f) for f in F),
                                                       _ptr(cost_data), _ptr(trial), _ptr(prior), _ptr(stiffness),
                                                       int(bool(solve)), B, T, _ptr(trial_out) if solve else None, _ptr(params),
                                                       _ptr(cost), _ptr(cost0), _ptr(workspace) if solve else None, _stream()),
                   "shr_%s_step" % entry)
    return (trial_out if solve else None), params, cost, cost0


def pose_lm_seq_begin(params0, seq_len, lambda0=1e-3):
    """pose_lm_begin for sequences (shr_pose_lm_seq_begin): params0 [B,26], B = S seq_len -> (state, trial [B,26])."""
    return _lm_band_begin("pose_lm_seq", params0, seq_len, lambda0)


def pose_lm_seq_step(state, A, g, E, cost_data, trial, seq_len, prior=None, stiffness=None, solve=True, out=None, workspace=None):
    """One step of the sequence loop (shr_pose_lm_seq_step): A [B,26,26], g [B,26], E [B,26,26] (None with seq_len 1),
    cost_data [B] fp64 of the poses `trial` [B,26] -> (trial_out [B,26] or None without `solve`, params [B,26], cost [S],
    cost0 [S]), S = B / seq_len: one decision, one lambda and one cost per sequence, the step from the block-tridiagonal
    solve.  prior, stiffness, out: pose_lm_step's; workspace: shr_pose_lm_seq_workspace_bytes(B) bytes to use instead of a
    new buffer."""
    return _lm_band_step("pose_lm_seq", state, A, g, E, (), cost_data, trial, seq_len, prior, stiffness, solve, out, workspace)


def sphere_icp_sequence(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand=True,
                        pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                        stiffness=None, prior=None, render_weight=1.0, max_resid=float("inf"), background=100.0,
                        keypoints=None, confidence=None, kp_weight=1.0, kp_max=float("inf"), limits=None, limit_weight=0.0,
                        collision=None, collision_weight=0.0, temporal_weight=1.0, ts_max=float("inf"), frame_weight=None,
                        pose_prior=None):
    """sphere_icp_priors over SEQUENCES: the B = S seq_len frames are S sequences of seq_len consecutive frames (adjacent in
    the batch), fitted jointly by `iters` Levenberg-Marquardt iterations on the sum over a sequence's frames of
    sphere_icp_priors' energy + temporal_weight sum_t frame_weight[t] sum_j min(|c_j(t + 1) - c_j(t)|, ts_max)^2, c the
    model-frame sphere centres -> (params [B,26], cost0 [S], cost [S]): one cost, one lambda and one accept decision per
    sequence.  Each of the iters + 1 evaluations is sphere_icp_priors' launches, then shr_sphere_temporal_normal
    (accumulate = 1), then shr_pose_lm_seq_step (the block-tridiagonal solve) in place of shr_pose_lm_step, on torch's
    current stream, into buffers allocated once before the loop; nothing returns to the host: capturable in a graph.
    Without a weighted temporal term (temporal_weight = 0 or seq_len = 1) no launch of the temporal entry is issued and E
    is zero; with seq_len = 1 the loop is sphere_icp_priors bit for bit."""
    return _sphere_sequence_loop(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand, pixel_to_model,
                                 fg_max, max_dist, iters, lambda0, stiffness, prior, render_weight, max_resid, background,
                                 keypoints, confidence, kp_weight, kp_max, limits, limit_weight, collision, collision_weight,
                                 temporal_weight, ts_max, frame_weight, 0.0, float("inf"), None, pose_prior=pose_prior)


def _sphere_accel_args(B, dev, accel_weight, acc_max, triple_weight):
    accel_weight, acc_max = float(accel_weight), float(acc_max)
    accel_weight = _weight_arg(accel_weight, "accel_weight")
    if not acc_max >= 0.0:
        raise RuntimeError("acc_max must be >= 0 (inf: no saturation), not %r" % (acc_max,))
    if triple_weight is not None:
        _check_input(triple_weight, "triple_weight")
        if tuple(triple_weight.shape) != (B,) or triple_weight.device != dev:
            raise RuntimeError("triple_weight must be [B] on the parameters' device")
    return accel_weight, acc_max


def sphere_accel_normal(params, offset, offset_inv, bone, wv, seq_len, right_hand=True, accel_weight=1.0, acc_max=float("inf"),
                        triple_weight=None, accumulate_into=None, accumulate_E_into=None):
    """The normal equations of the sphere fit's constant-velocity term (include/spherehand_hip.h, shr_sphere_accel_normal):
    params [B,26], B = S seq_len frames with the frames of a sequence adjacent, the key-point tables of
    pose_keypoints_jacobian -> (A [B,26,26] the diagonal blocks, g [B,26], E [B,26,26] (frame t's rows, frame t + 1's
    columns), F [B,26,26] (frame t's rows, frame t + 2's columns; +0 for the last two frames of a sequence), cost [B] fp64 (a
    triple's cost at its last frame), count [B] int32: the spheres with rows of the triple ending at the frame).  The term is
    accel_weight triple_weight[k] sum_j min(|c_j(k - 1) - 2 c_j(k) + c_j(k + 1)|, acc_max)^2 over the model-frame centres;
    triple_weight [B] >= 0 (None: 1) weighs the triple centred at k.  accumulate_into = (A, g, cost) of the other terms at
    the same poses: the term is ADDED to them in place (a frame without a weighted triple is not touched) and they are the
    A, g, cost returned.  accumulate_E_into = E of shr_sphere_temporal_normal at the same poses: the term's E is added to
    it in place.  F is always new.  Two launches: shr_pose_keypoints_jacobian -> shr_sphere_accel_normal."""
    B, J = _ik_tables(params, offset, offset_inv, bone, wv, "parameters")
    dev = params.device
    if any(t.device != dev for t in (offset, offset_inv, bone, wv)):
        raise RuntimeError("every tensor must be on the parameters' device")
    T = _sphere_temporal_args(B, dev, seq_len, 0.0, 0.0, None)[0]
    accel_weight, acc_max = _sphere_accel_args(B, dev, accel_weight, acc_max, triple_weight)
    if accumulate_into is not None:
        A, g, cost = accumulate_into
    E = accumulate_E_into
    for t, name, shape in (() if accumulate_into is None else ((A, "A", (B, 26, 26)), (g, "g", (B, 26)), (cost, "cost", (B,)))) + \
            (() if E is None else ((E, "E", (B, 26, 26)),)):
        _check_input(t, name, torch.float64)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("the %s to accumulate into must be %s fp64 on the parameters' device" % (name, shape))
    lib = _lib.lib()
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        if accumulate_into is None:
            A, g, cost = _new_normal(B, dev)
        if E is None:
            E = torch.empty((B, 26, 26), dtype=torch.float64, device=dev)
        F = torch.empty((B, 26, 26), dtype=torch.float64, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.shr_sphere_accel_normal(_ptr(kp), _ptr(jac), _ptr(triple_weight), accel_weight, acc_max, B, T, J,
                                               int(accumulate_into is not None), int(accumulate_E_into is not None), _ptr(A),
                                               _ptr(g), _ptr(E), _ptr(F), _ptr(cost), _ptr(count), None, _stream()),
                   "shr_sphere_accel_normal")
    return A, g, E, F, cost, count


def pose_lm_seq2_begin(params0, seq_len, lambda0=1e-3):
    """pose_lm_seq_begin for the block-pentadiagonal step (shr_pose_lm_seq2_begin): params0 [B,26], B = S seq_len ->
    (state, trial [B,26])."""
    return _lm_band_begin("pose_lm_seq2", params0, seq_len, lambda0)


def pose_lm_seq2_step(state, A, g, E, F, cost_data, trial, seq_len, prior=None, stiffness=None, solve=True, out=None,
                      workspace=None):
    """pose_lm_seq_step with the second off-diagonal blocks F [B,26,26] (frame t's rows, frame t + 2's columns) after E
    (shr_pose_lm_seq2_step): the step is from the block-PENTAdiagonal solve.  F None: no second band, and every output is
    pose_lm_seq_step's bit for bit.  state: pose_lm_seq2_begin's; workspace: shr_pose_lm_seq2_workspace_bytes(B) bytes to use
    instead of a new buffer."""
    return _lm_band_step("pose_lm_seq2", state, A, g, E, (F,), cost_data, trial, seq_len, prior, stiffness, solve, out, workspace)


def pose_lm_covariance(A, E, F, seq_len, stiffness=None, jac=None, workspace=None):
    """The marginal covariances of the sequence fit (include/spherehand_hip.h, shr_pose_lm_seq2_covariance): A [B,26,26], E
    and F [B,26,26] fp64 (or None: F None no second band, E None no coupling at all), B = S seq_len -> (cov [B,26,26] fp64,
    the diagonal blocks of the inverse of the UNDAMPED block-pentadiagonal matrix with diagonal blocks A_t + diag(stiffness);
    sphere_cov [B,J,3,3] fp64 = Jc_j cov Jc_j^T per sphere with jac [B,3J,26] (pose_keypoints_jacobian's), None without;
    status [S] int32: 0, or 1 + the first frame whose pivot is not positive and finite -- that sequence's cov and sphere_cov
    are NaN on all its frames).  The Gauss-Newton (Laplace) covariance per unit of residual variance; all fp64 in a stated
    order, bitwise reproducible.  workspace: shr_pose_lm_seq2_covariance_workspace_bytes(B) bytes to use instead of a new
    buffer.  One launch, two with jac, on torch's current stream; the six stored values per sphere are expanded to the
    symmetric 3 x 3 in torch."""
    _check_input(A, "A", torch.float64)
    if A.dim() != 3 or tuple(A.shape[1:]) != (26, 26):
        raise RuntimeError("A must be [B,26,26]")
    B, dev = A.shape[0], A.device
    T = _sphere_temporal_args(B, dev, seq_len, 0.0, 0.0, None)[0]
    for t, name in ((E, "E"), (F, "F")):
        if t is None:
            continue
        _check_input(t, name, torch.float64)
        if tuple(t.shape) != (B, 26, 26) or t.device != dev:
            raise RuntimeError("%s must be [B,26,26] fp64 on A's device" % name)
    if stiffness is not None:
        _check_input(stiffness, "stiffness")
        if tuple(stiffness.shape) != (26,) or stiffness.device != dev:
            raise RuntimeError("stiffness must be [26] on A's device")
    J = 1
    if jac is not None:
        _check_input(jac, "jac")
        if jac.dim() != 3 or jac.shape[0] != B or jac.shape[2] != 26 or jac.shape[1] % 3 != 0 or jac.shape[1] == 0 or jac.device != dev:
            raise RuntimeError("jac must be [B,3J,26] on A's device")
        J = jac.shape[1] // 3
    lib = _lib.lib()
    need = lib.shr_pose_lm_seq2_covariance_workspace_bytes(B)
    if workspace is not None and workspace.numel() * workspace.element_size() < need:
        raise RuntimeError("workspace must hold shr_pose_lm_seq2_covariance_workspace_bytes(B) = %d bytes" % need)
    with _on(dev):
        cov = torch.empty((B, 26, 26), dtype=torch.float64, device=dev)
        six = None if jac is None else torch.empty((B, J, 6), dtype=torch.float64, device=dev)
        status = torch.empty((B // T,), dtype=torch.int32, device=dev)
        if workspace is None:
            workspace = torch.empty((max(1, need // 8),), dtype=torch.float64, device=dev)
        _lib.check(lib.shr_pose_lm_seq2_covariance(_ptr(A), _ptr(E), _ptr(F), _ptr(stiffness), _ptr(jac), B, T, J, _ptr(cov),
                                                   _ptr(six), _ptr(status), _ptr(workspace), _stream()),
                   "shr_pose_lm_seq2_covariance")
        sphere_cov = None
        if six is not None:                                  # (no index tensor: nothing goes from the host to the device)
            xx, xy, xz, yy, yz, zz = six.unbind(-1)
            sphere_cov = torch.stack((xx, xy, xz, xy, yy, yz, xz, yz, zz), -1).view(B, J, 3, 3)
    return cov, sphere_cov, status


def _window_prior_args(prior, S, T, dev, active):
    """(Lambda [S,52,52], eta [S,52], offset [S] fp64, point [S,52] fp32) of pose_window_marginalize, and active [S] int32 or
    None, checked for a batch of S sequences on `dev`"""
    try:
        Lambda, eta, offset, point = prior
    except (TypeError, ValueError):
        raise RuntimeError("the window prior is (Lambda, eta, offset, point)")
    for t, name, shape, dtype in ((Lambda, "Lambda", (S, 52, 52), torch.float64), (eta, "eta", (S, 52), torch.float64),
                                  (offset, "offset", (S,), torch.float64), (point, "point", (S, 52), torch.float32)):
        _check_input(t, name, dtype)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("%s must be %s on the parameters' device" % (name, shape))
    if active is not None:
        _check_input(active, "active", torch.int32)
        if tuple(active.shape) != (S,) or active.device != dev:
            raise RuntimeError("active must be [S] int32 on the parameters' device")
    return Lambda, eta, offset, point, active


def pose_window_marginalize(A, g, E, F, cost_data, trial, seq_len, prior=None, stiffness=None):
    """The frame that leaves a sliding window folded into a Gaussian prior on the next two frames (include/spherehand_hip.h,
    shr_pose_window_marginalize): the DEPARTING system A [B,26,26], g [B,26], E, F [B,26,26] (or None), cost_data [B] fp64
    at the poses trial [B,26] fp32, B = S seq_len, of which frames 0 ... min(seq_len, 3) - 1 are read; prior [B,26] and
    stiffness [26] apply to frame 0 only -> (Lambda [S,52,52], eta [S,52], offset [S] fp64, point [S,52] fp32 the trial poses
    of frames 1 and 2, status [S] int32: 1 where frame 0's matrix has a pivot that is not positive and finite -- that
    sequence's record is then an exact +0).  All fp64 in a stated order, bitwise reproducible; one launch on torch's current
    stream."""
    _check_input(trial, "trial")
    if trial.dim() != 2 or trial.shape[1] != 26:
        raise RuntimeError("trial must be [B,26]")
    B, dev = trial.shape[0], trial.device
    T = _sphere_temporal_args(B, dev, seq_len, 0.0, 0.0, None)[0]
    for t, name, shape in ((A, "A", (B, 26, 26)), (g, "g", (B, 26)), (E, "E", (B, 26, 26)), (F, "F", (B, 26, 26)),
                           (cost_data, "cost_data", (B,))):
        if t is None and name in ("E", "F"):
            continue
        _check_input(t, name, torch.float64)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("%s must be %s fp64 on trial's device" % (name, shape))
    if prior is not None:
        _check_input(prior, "prior")
        if tuple(prior.shape) != (B, 26) or prior.device != dev:
            raise RuntimeError("prior must be [B,26] on trial's device")
    if stiffness is not None:
        _check_input(stiffness, "stiffness")
        if tuple(stiffness.shape) != (26,) or stiffness.device != dev:
            raise RuntimeError("stiffness must be [26] on trial's device")
    S = B // T
    lib = _lib.lib()
    with _on(dev):
        Lambda = torch.empty((S, 52, 52), dtype=torch.float64, device=dev)
        eta = torch.empty((S, 52), dtype=torch.float64, device=dev)
        offset = torch.empty((S,), dtype=torch.float64, device=dev)
        point = torch.empty((S, 52), dtype=torch.float32, device=dev)
        status = torch.empty((S,), dtype=torch.int32, device=dev)
        _lib.check(lib.shr_pose_window_marginalize(_ptr(A), _ptr(g), _ptr(E), _ptr(F), _ptr(cost_data), _ptr(trial), _ptr(prior),
                                                   _ptr(stiffness), B, T, _ptr(Lambda), _ptr(eta), _ptr(offset), _ptr(point),
                                                   _ptr(status), None, _stream()), "shr_pose_window_marginalize")
    return Lambda, eta, offset, point, status


def pose_window_prior_normal(trial, Lambda, eta, offset, point, seq_len, into=None, E=None, active=None):
    """The normal equations of the prior a sliding window carries (include/spherehand_hip.h, shr_pose_window_prior_normal):
    trial [B,26] fp32, B = S seq_len, and pose_window_marginalize's record -> (A [B,26,26], g [B,26], E [B,26,26], cost [B]
    fp64).  The term is (d^T Lambda d + 2 eta^T d) + offset with d = trial(frames 0, 1) - point; it touches frames 0 and 1 of
    a sequence and E of frame 0 alone.  into = (A, g, cost) of the other terms at the same poses: the term is ADDED to them
    in place and they are returned; without it the three are new, +0 on the frames the term does not reach.  E: the other
    terms' E to add to in place; without it a new one, +0 outside the term.  active [S] int32: a sequence with 0 has no term
    and is left alone.  One launch on torch's current stream."""
    _check_input(trial, "trial")
    if trial.dim() != 2 or trial.shape[1] != 26:
        raise RuntimeError("trial must be [B,26]")
    B, dev = trial.shape[0], trial.device
    T = _sphere_temporal_args(B, dev, seq_len, 0.0, 0.0, None)[0]
    Lambda, eta, offset, point, active = _window_prior_args((Lambda, eta, offset, point), B // T, T, dev, active)
    if into is not None:
        A, g, cost = into
    for t, name, shape in (() if into is None else ((A, "A", (B, 26, 26)), (g, "g", (B, 26)), (cost, "cost", (B,)))) + \
            (() if E is None else ((E, "E", (B, 26, 26)),)):
        _check_input(t, name, torch.float64)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("the %s to accumulate into must be %s fp64 on trial's device" % (name, shape))
    add_E = int(E is not None)
    lib = _lib.lib()
    with _on(dev):
        if into is None:                                     # (an inactive sequence and frames >= 2 are not written: +0)
            A = torch.zeros((B, 26, 26), dtype=torch.float64, device=dev)
            g = torch.zeros((B, 26), dtype=torch.float64, device=dev)
            cost = torch.zeros((B,), dtype=torch.float64, device=dev)
        if E is None:
            E = torch.zeros((B, 26, 26), dtype=torch.float64, device=dev)
        _lib.check(lib.shr_pose_window_prior_normal(_ptr(trial), _ptr(Lambda), _ptr(eta), _ptr(offset), _ptr(point), _ptr(active),
                                                    B, T, int(into is not None), add_E, _ptr(A), _ptr(g), _ptr(E), _ptr(cost),
                                                    None, _stream()), "shr_pose_window_prior_normal")
    return A, g, E, cost


def _sphere_sequence_loop(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand, pixel_to_model, fg_max,
                          max_dist, iters, lambda0, stiffness, prior, render_weight, max_resid, background, keypoints, confidence,
                          kp_weight, kp_max, limits, limit_weight, collision, collision_weight, temporal_weight, ts_max,
                          frame_weight, accel_weight, acc_max, triple_weight, window_prior=None, pose_prior=None):
    """The loop of sphere_icp_sequence, sphere_icp_trajectory and sphere_icp_window.  pose_prior: sphere_icp_priors', a
    per-frame term: shr_pose_vae_normal (accumulate = 1) follows the collision entry.  Without a weighted acceleration term
    (accel_weight = 0 or seq_len < 3) it is sphere_icp_sequence's: shr_pose_lm_seq_begin / _step, no F; with one,
    shr_sphere_accel_normal follows the first-difference entry and the step is shr_pose_lm_seq2_begin / _step's.
    window_prior = (Lambda, eta, offset, point) of pose_window_marginalize (None: no prior, no launch): the carried prior's
    entry shr_pose_window_prior_normal (accumulate = 1) follows shr_sphere_accel_normal in every evaluation."""
    terms = _FrameTerms(observed, view, params0, offset, offset_inv, bone, wv, radii, right_hand, pixel_to_model, fg_max, max_dist,
                        render_weight, max_resid, background, keypoints, confidence, kp_weight, kp_max, limits, limit_weight,
                        collision, collision_weight, pose_prior)
    (B, _, J, _, _), dev = terms.dims, terms.dev
    T, temporal_weight, ts_max = _sphere_temporal_args(B, dev, seq_len, temporal_weight, ts_max, frame_weight)
    temporal = T > 1 and temporal_weight > 0.0
    accel_weight, acc_max = _sphere_accel_args(B, dev, accel_weight, acc_max, triple_weight)
    accel = T > 2 and accel_weight > 0.0
    if window_prior is not None:
        window_prior = _window_prior_args(window_prior, B // T, T, dev, None)
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    state, trial = (pose_lm_seq2_begin if accel else pose_lm_seq_begin)(params0, T, lambda0)
    _lm_prior_args(prior, stiffness, B)
    lib = _lib.lib()
    S = B // T
    with _on(dev):
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
        terms.allocate()
        kp, jac, A, g, cost_data = terms.kp, terms.jac, terms.A, terms.g, terms.cost_data
        E = torch.zeros((B, 26, 26), dtype=torch.float64, device=dev)       # (stays zero without a term between frames)
        F = f64(B, 26, 26) if accel else None
        temporal_rows = torch.empty((B,), dtype=torch.int32, device=dev) if temporal else None
        accel_rows = torch.empty((B,), dtype=torch.int32, device=dev) if accel else None
        params, cost0, cost = f32(B, 26), f32(S), f32(S)
        seq_ws = f64(max(1, (lib.shr_pose_lm_seq2_workspace_bytes if accel else lib.shr_pose_lm_seq_workspace_bytes)(B) // 8))
        stream = _stream()
        for it in range(iters + 1):
            terms.evaluate(trial, stream)
            if temporal:
                _lib.check(lib.shr_sphere_temporal_normal(_ptr(kp), _ptr(jac), _ptr(frame_weight), temporal_weight, ts_max, B, T,
                                                          J, 1, _ptr(A), _ptr(g), _ptr(E), _ptr(cost_data), _ptr(temporal_rows),
                                                          None, stream), "shr_sphere_temporal_normal")
            if accel:                                          # (without the first-difference entry E is this entry's alone)
                _lib.check(lib.shr_sphere_accel_normal(_ptr(kp), _ptr(jac), _ptr(triple_weight), accel_weight, acc_max, B, T, J,
                                                       1, int(temporal), _ptr(A), _ptr(g), _ptr(E), _ptr(F), _ptr(cost_data),
                                                       _ptr(accel_rows), None, stream), "shr_sphere_accel_normal")
            if window_prior is not None:                       # (E of frame 0: written where no entry above has written it)
                _lib.check(lib.shr_pose_window_prior_normal(_ptr(trial), *(_ptr(t) for t in window_prior), B, T, 1,
                                                            int(temporal or accel), _ptr(A), _ptr(g), _ptr(E), _ptr(cost_data),
                                                            None, stream), "shr_pose_window_prior_normal")
            solve = int(it < iters)
            tail = (_ptr(cost_data), _ptr(trial), _ptr(prior), _ptr(stiffness), solve, B, T, _ptr(trial) if solve else None,
                    _ptr(params), _ptr(cost), _ptr(cost0), _ptr(seq_ws) if solve else None, stream)
            if accel:
                _lib.check(lib.shr_pose_lm_seq2_step(_ptr(state), _ptr(A), _ptr(g), _ptr(E), _ptr(F), *tail), "shr_pose_lm_seq2_step")
            else:
                _lib.check(lib.shr_pose_lm_seq_step(_ptr(state), _ptr(A), _ptr(g), _ptr(E), *tail), "shr_pose_lm_seq_step")
    return params, cost0, cost


def sphere_icp_trajectory(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand=True,
                          pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                          stiffness=None, prior=None, render_weight=1.0, max_resid=float("inf"), background=100.0,
                          keypoints=None, confidence=None, kp_weight=1.0, kp_max=float("inf"), limits=None, limit_weight=0.0,
                          collision=None, collision_weight=0.0, temporal_weight=1.0, ts_max=float("inf"), frame_weight=None,
                          accel_weight=1.0, acc_max=float("inf"), triple_weight=None, pose_prior=None):
    """sphere_icp_sequence with the constant-velocity term: the energy of a sequence gains
    accel_weight sum_k triple_weight[k] sum_j min(|c_j(k - 1) - 2 c_j(k) + c_j(k + 1)|, acc_max)^2 over its triples of
    consecutive frames -> (params [B,26], cost0 [S], cost [S]).  Each of the iters + 1 evaluations is sphere_icp_sequence's
    launches up to shr_sphere_temporal_normal, then shr_sphere_accel_normal (accumulate = 1; accumulate_E = 1 iff the
    first-difference entry was launched in this evaluation), then shr_pose_lm_seq2_step (the block-pentadiagonal solve), on
    torch's current stream, into buffers allocated once before the loop; nothing returns to the host: capturable in a
    graph.  Without a weighted acceleration term (accel_weight = 0 or seq_len < 3) no launch of the entry is issued and F is
    not formed: the loop is then sphere_icp_sequence's own, launch for launch."""
    return _sphere_sequence_loop(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand, pixel_to_model,
                                 fg_max, max_dist, iters, lambda0, stiffness, prior, render_weight, max_resid, background,
                                 keypoints, confidence, kp_weight, kp_max, limits, limit_weight, collision, collision_weight,
                                 temporal_weight, ts_max, frame_weight, accel_weight, acc_max, triple_weight,
                                 pose_prior=pose_prior)


def sphere_icp_window(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand=True,
                      pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                      stiffness=None, prior=None, render_weight=1.0, max_resid=float("inf"), background=100.0,
                      keypoints=None, confidence=None, kp_weight=1.0, kp_max=float("inf"), limits=None, limit_weight=0.0,
                      collision=None, collision_weight=0.0, temporal_weight=1.0, ts_max=float("inf"), frame_weight=None,
                      accel_weight=1.0, acc_max=float("inf"), triple_weight=None, window_prior=None, pose_prior=None):
    """sphere_icp_trajectory over a sliding window that carries its marginalised past: window_prior = (Lambda [S,52,52],
    eta [S,52], offset [S] fp64, point [S,52] fp32), pose_window_marginalize's record, adds
    (d^T Lambda d + 2 eta^T d) + offset, d = (p_0, p_1) - point, to the energy of each sequence (a record that a failed pivot
    left +0 adds nothing) -> (params [B,26], cost0 [S], cost [S]).  Each evaluation is
    sphere_icp_trajectory's launches with shr_pose_window_prior_normal (accumulate = 1; accumulate_E = 1 iff an entry before
    it wrote E in this evaluation) after shr_sphere_accel_normal; the step is unchanged, the prior's blocks being blocks of
    the same block-pentadiagonal system.  window_prior = None: no launch is added, and the loop is sphere_icp_trajectory's
    launch for launch and bit for bit."""
    return _sphere_sequence_loop(observed, view, params0, offset, offset_inv, bone, wv, radii, seq_len, right_hand, pixel_to_model,
                                 fg_max, max_dist, iters, lambda0, stiffness, prior, render_weight, max_resid, background,
                                 keypoints, confidence, kp_weight, kp_max, limits, limit_weight, collision, collision_weight,
                                 temporal_weight, ts_max, frame_weight, accel_weight, acc_max, triple_weight, window_prior,
                                 pose_prior)


PoseLmSharedMaxK = 64        # shared parameters of a group at most (shr_pose_lm_shared_step)


def _pose_lm_shared_args(B, group_size, K):
    try:
        N, K = int(group_size), int(K)
    except (TypeError, ValueError):
        raise RuntimeError("group_size and the number of shared parameters must be integers")
    if N < 1 or B % N != 0:
        raise RuntimeError("group_size must be >= 1 and divide the %d frames of the batch, not %r" % (B, group_size))
    if not 0 <= K <= PoseLmSharedMaxK:
        raise RuntimeError("0 to %d shared parameters are taken, not %d" % (PoseLmSharedMaxK, K))
    return N, K, B // N


def pose_lm_shared_begin(params0, shape0, group_size, lambda0=1e-3):
    """pose_lm_begin for groups of frames that share parameters (shr_pose_lm_shared_begin): params0 [B,26], B = G group_size,
    shape0 [G,K] fp32 (None: K = 0, no shared block) -> (state, trial [B,26], trial_shape [G,K] or None)."""
    _check_input(params0, "start parameters")
    if params0.dim() != 2 or params0.shape[1] != 26:
        raise RuntimeError("start parameters must be [B,26]")
    if not float(lambda0) > 0:
        raise RuntimeError("lambda0 must be > 0")
    B = params0.shape[0]
    if shape0 is not None:
        _check_input(shape0, "start shape")
        if shape0.dim() != 2 or shape0.device != params0.device:
            raise RuntimeError("start shape must be [G,K] on the start parameters' device")
    N, K, G = _pose_lm_shared_args(B, group_size, 0 if shape0 is None else shape0.shape[1])
    if shape0 is not None and shape0.shape[0] != G:
        raise RuntimeError("start shape must be [%d,K], one row per group" % G)
    lib = _lib.lib()
    dev = params0.device
    with _on(dev):
        state = torch.empty((max(1, lib.shr_pose_lm_shared_state_bytes(B, G, K) // 8),), dtype=torch.float64, device=dev)
        trial = torch.empty((B, 26), dtype=torch.float32, device=dev)
        trial_shape = torch.empty((G, K), dtype=torch.float32, device=dev) if K else None
        _lib.check(lib.shr_pose_lm_shared_begin(_ptr(params0), _ptr(shape0) if K else None, B, N, K, float(lambda0), _ptr(state),
                                                _ptr(trial), _ptr(trial_shape) if K else None, _stream()),
                   "shr_pose_lm_shared_begin")
    return state, trial, trial_shape


def pose_lm_shared_step(state, A, g, C, R, gs, cost_data, trial, trial_shape, group_size, prior=None, stiffness=None,
                        shape_prior=None, shape_stiffness=None, solve=True, out=None, workspace=None):
    """One step of the loop over groups with shared parameters (shr_pose_lm_shared_step): A [B,26,26], g [B,26],
    cost_data [B] fp64 of the poses `trial` [B,26] and, of the shared parameters `trial_shape` [G,K], the coupling
    C [B,26,K], the shared block R [G,K,K] (lower triangle read) and its gradient gs [G,K], fp64 -> (trial_out [B,26],
    trial_shape_out [G,K] -- both None without `solve` --, params [B,26], shape [G,K], cost [G], cost0 [G]), G = B /
    group_size: one decision, one lambda and one cost per group, the step from the Schur complement on the shared block.
    prior, stiffness: pose_lm_step's; shape_prior [G,K] (default: the start shape) and shape_stiffness [K] >= 0 add
    sum_k shape_stiffness_k (shape_k - shape_prior_k)^2 to a group's cost.  C = R = gs = trial_shape = None: K = 0, no shared
    block; the shape outputs are then None and with group_size 1 every output is pose_lm_step's bit for bit.
    out = (trial_out, trial_shape_out, params, shape, cost, cost0): buffers to write instead of new ones; workspace:
    shr_pose_lm_shared_workspace_bytes(B, G, K) bytes to use instead of a new buffer."""
    _check_input(trial, "trial")
    B = trial.shape[0]
    if trial.dim() != 2 or trial.shape[1] != 26:
        raise RuntimeError("trial must be [B,26]")
    dev = trial.device
    shared = (C, R, gs, trial_shape)
    if any(t is None for t in shared) and not all(t is None for t in shared):
        raise RuntimeError("C, R, gs and trial_shape are given together or not at all")
    if trial_shape is not None:
        _check_input(trial_shape, "trial_shape")
        if trial_shape.dim() != 2 or trial_shape.device != dev:
            raise RuntimeError("trial_shape must be [G,K] on trial's device")
    N, K, G = _pose_lm_shared_args(B, group_size, 0 if trial_shape is None else trial_shape.shape[1])
    if K == 0 and trial_shape is not None:
        C = R = gs = trial_shape = None
    for t, name, shape in ((state, "state", None), (A, "A", (B, 26, 26)), (g, "g", (B, 26)), (C, "C", (B, 26, K)),
                           (R, "R", (G, K, K)), (gs, "gs", (G, K)), (cost_data, "cost_data", (B,))):
        if t is None:
            continue
        _check_input(t, name, torch.float64)
        if (shape is not None and tuple(t.shape) != shape) or t.device != dev:
            raise RuntimeError("%s must be %s fp64 on trial's device" % (name, shape))
    if trial_shape is not None and tuple(trial_shape.shape) != (G, K):
        raise RuntimeError("trial_shape must be [%d,%d]" % (G, K))
    lib = _lib.lib()
    if state.numel() * 8 < lib.shr_pose_lm_shared_state_bytes(B, G, K):
        raise RuntimeError("state is pose_lm_shared_begin's, for the same B, group_size and K")
    for t, name, shape in ((prior, "prior", (B, 26)), (stiffness, "stiffness", (26,)), (shape_prior, "shape_prior", (G, K)),
                           (shape_stiffness, "shape_stiffness", (K,))):
        if t is None:
            continue
        _check_input(t, name)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("%s must be %s on trial's device" % (name, list(shape)))
    if K == 0:
        shape_prior = shape_stiffness = None
    with _on(dev):
        if out is None:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
            out = (new(B, 26) if solve else None, new(G, K) if solve and K else None, new(B, 26), new(G, K) if K else None,
                   new(G), new(G))
        if workspace is None:
            workspace = torch.empty((max(1, lib.shr_pose_lm_shared_workspace_bytes(B, G, K) // 8),), dtype=torch.float64,
                                    device=dev)
        elif workspace.numel() * workspace.element_size() < lib.shr_pose_lm_shared_workspace_bytes(B, G, K):
            raise RuntimeError("workspace is too small for this B, group_size and K")
        trial_out, trial_shape_out, params, shape, cost, cost0 = out
        _lib.check(lib.shr_pose_lm_shared_step(
            _ptr(state), _ptr(A), _ptr(g), _ptr(C) if K else None, _ptr(R) if K else None, _ptr(gs) if K else None,
            _ptr(cost_data), _ptr(trial), _ptr(trial_shape) if K else None, _ptr(prior), _ptr(stiffness), _ptr(shape_prior),
            _ptr(shape_stiffness), int(bool(solve)), B, N, K, _ptr(trial_out) if solve else None,
            _ptr(trial_shape_out) if solve and K else None, _ptr(params), _ptr(shape) if K else None, _ptr(cost), _ptr(cost0),
            _ptr(workspace), _stream()), "shr_pose_lm_shared_step")
    return (trial_out if solve else None), (trial_shape_out if solve and K else None), params, (shape if K else None), cost, cost0


def _sphere_radii_args(observed, view, params, offset, offset_inv, bone, wv, radii, group_size, pixel_to_model, max_dist,
                       name="parameters"):
    _check_input(radii, "radii")
    if radii.dim() != 2:
        raise RuntimeError("radii must be [G,J], one table per group of frames")
    one = radii[0] if radii.shape[0] else radii.new_empty((radii.shape[1],))
    B, V, H, W, J, p2m, max_dist = _sphere_icp_args(observed, view, params, offset, offset_inv, bone, wv, one, pixel_to_model,
                                                    max_dist, name)
    N, _, G = _pose_lm_shared_args(B, group_size, J)
    if radii.shape[0] != G:
        raise RuntimeError("radii must be [%d,%d]: %d frames in groups of %d" % (G, J, B, N))
    return B, V, H, W, J, N, G, p2m, max_dist


def sphere_icp_radii_normal(observed, view, params, offset, offset_inv, bone, wv, radii, group_size, right_hand=True,
                            pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), want_maps=False):
    """sphere_icp_normal with the sphere radii among the unknowns (shr_sphere_icp_radii_normal): radii [G,J], one table per
    group of group_size adjacent frames, B = G group_size -> (A [B,26,26], g [B,26], cost [B] fp64, count [B] int32,
    C [B,26,J], R [G,J,J], gs [G,J] fp64 -- what pose_lm_shared_step takes beside A and g --, moments [B,J,16] fp64: the
    twelve of sphere_icp_normal, then sum u and sum d); with want_maps also (dist, owner).  A group with a radius that is not
    finite or not > 0 has cost = +inf and zero equations."""
    B, V, H, W, J, N, G, p2m, max_dist = _sphere_radii_args(observed, view, params, offset, offset_inv, bone, wv, radii,
                                                            group_size, pixel_to_model, max_dist)
    lib = _lib.lib()
    dev = observed.device
    with _on(dev):
        kp, jac = pose_keypoints_jacobian(params, offset, offset_inv, bone, wv, right_hand)
        centres = torch.empty((B, V, J, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.shr_view_vertices_fwd(_ptr(kp), _ptr(view), B, V, J, _ptr(centres), _stream()), "shr_view_vertices_fwd")
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
        (A, g, cost), C, R, gs, moments = _new_normal(B, dev), f64(B, 26, J), f64(G, J, J), f64(G, J), f64(B, J, 16)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        dist = torch.empty((B, V, H, W), dtype=torch.float32, device=dev) if want_maps else None
        owner = torch.empty((B, V, H, W), dtype=torch.int32, device=dev) if want_maps else None
        ws = torch.empty((max(16, lib.shr_sphere_icp_radii_normal_workspace_bytes(B, V, J, W, H)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.shr_sphere_icp_radii_normal(_ptr(observed), _ptr(centres), _ptr(radii), _ptr(view), _ptr(jac), B, V, J, W,
                                                   H, N, *p2m, float(fg_max), max_dist, _ptr(A), _ptr(g), _ptr(cost), _ptr(count),
                                                   _ptr(C), _ptr(R), _ptr(gs), _ptr(moments), _ptr(dist), _ptr(owner), _ptr(ws),
                                                   _stream()), "shr_sphere_icp_radii_normal")
    return (A, g, cost, count, C, R, gs, moments) + ((dist, owner) if want_maps else ())


def sphere_icp_calibrate(observed, view, params0, offset, offset_inv, bone, wv, radii0, group_size, right_hand=True,
                         pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=1000.0, max_dist=float("inf"), iters=10, lambda0=1e-3,
                         stiffness=None, prior=None, shape_stiffness=None, shape_prior=None, keypoints=None, confidence=None,
                         kp_weight=1.0, kp_max=float("inf"), limits=None, limit_weight=0.0, collision=None,
                         collision_weight=0.0):
    """Calibrate the sphere radii to the hand in the frames: sphere_icp_priors' loop without the render term, the radii [G,J]
    of every group of group_size adjacent frames fitted with the frames' poses -> (params [B,26], radii [G,J], cost0 [G],
    cost [G]).  `iters` Levenberg-Marquardt iterations from (params0 [B,26], radii0 [G,J]) on the group's energy
    sum over its frames of (sum dist^2 + sum_i stiffness_i (p_i - prior_i)^2 + the keypoint, limit and collision terms of
    sphere_icp_priors) + sum_j shape_stiffness_j (r_j - shape_prior_j)^2, shape_prior [G,J] (default radii0).  Each of the
    iters + 1 evaluations is shr_pose_keypoints_jacobian -> shr_view_vertices_fwd -> shr_sphere_icp_radii_normal with the
    trial radii -> shr_sphere_prior_normal / shr_sphere_collision_normal (accumulate = 1: they do not depend on the radii
    and add to A, g and the cost only) -> shr_pose_lm_shared_step, on torch's current stream, into buffers allocated once
    before the loop; nothing returns to the host: capturable in a graph.  The collision table is NOT rebuilt from the trial
    radii.  iters = 0 returns the starts and cost = cost0."""
    terms = _FrameTerms(observed, view, params0, offset, offset_inv, bone, wv, radii0, right_hand, pixel_to_model, fg_max,
                        max_dist, keypoints=keypoints, confidence=confidence, kp_weight=kp_weight, kp_max=kp_max, limits=limits,
                        limit_weight=limit_weight, collision=collision, collision_weight=collision_weight, group_size=group_size)
    (B, _, J, _, _), N, G, dev = terms.dims, terms.N, terms.G, terms.dev
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    for t, name, shape in ((prior, "prior", (B, 26)), (stiffness, "stiffness", (26,)), (shape_prior, "shape_prior", (G, J)),
                           (shape_stiffness, "shape_stiffness", (J,))):
        if t is None:
            continue
        _check_input(t, name)
        if tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError("%s must be %s on observed's device" % (name, list(shape)))
    state, trial, trial_shape = pose_lm_shared_begin(params0, radii0, N, lambda0)
    lib = _lib.lib()
    with _on(dev):
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        terms.allocate()
        params, radii, cost0, cost = f32(B, 26), f32(G, J), f32(G), f32(G)
        lm_ws = torch.empty((max(1, lib.shr_pose_lm_shared_workspace_bytes(B, G, J) // 8),), dtype=torch.float64, device=dev)
        stream = _stream()
        for it in range(iters + 1):
            terms.evaluate(trial, stream, trial_shape)
            solve = int(it < iters)
            _lib.check(lib.shr_pose_lm_shared_step(
                _ptr(state), _ptr(terms.A), _ptr(terms.g), _ptr(terms.C), _ptr(terms.R), _ptr(terms.gs), _ptr(terms.cost_data),
                _ptr(trial), _ptr(trial_shape), _ptr(prior), _ptr(stiffness), _ptr(shape_prior), _ptr(shape_stiffness), solve, B,
                N, J, _ptr(trial) if solve else None, _ptr(trial_shape) if solve else None, _ptr(params), _ptr(radii), _ptr(cost),
                _ptr(cost0), _ptr(lm_ws), stream), "shr_pose_lm_shared_step")
    return params, radii, cost0, cost


def _depth_normals_args(depth, scale, max_step):
    _check_input(depth, "depth")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise RuntimeError("depth must be [B,H,W] with H, W >= 1")
    try:
        sx, sy = (float(t) for t in scale)
    except (TypeError, ValueError):
        raise RuntimeError("scale must be two numbers (sx, sy): the model-space width of a pixel step in x and in y")
    return depth.shape[0], depth.shape[1], depth.shape[2], sx, sy, float(max_step)


def depth_normals(depth, fg_max, scale=(1.0, 1.0), max_step=float("inf"), out=None):
    """The unit normal map of a depth image (include/spherehand_hip.h, shr_depth_normals_fwd): depth [B,H,W] fp32 ->
    [B,3,H,W].  A pixel with depth < fg_max gets the normalised (dx wy, dy wx, -(wx wy)) of its central -- at a border, a
    hole or a depth step above max_step one-sided -- differences over widths of scale = (sx, sy) model units per pixel;
    every other pixel, and one with no usable neighbour along an axis, gets (0, 0, 0).  z <= 0: towards the camera.
    The entry refuses a scale that is not positive and finite, a NaN fg_max or max_step, a negative max_step, and an
    `out` ([B,3,H,W], where to write) that overlaps depth."""
    B, H, W, sx, sy, max_step = _depth_normals_args(depth, scale, max_step)
    if out is not None:
        _check_input(out, "out")
        if tuple(out.shape) != (B, 3, H, W) or out.device != depth.device:
            raise RuntimeError("out must be [B,3,H,W] for depth [B,H,W], on its device")
    with _on(depth.device):
        if out is None:
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
        _lib.check(_lib.lib().shr_depth_normals_fwd(_ptr(depth), B, W, H, float(fg_max), sx, sy, max_step, _ptr(out),
                                                    _stream()), "shr_depth_normals_fwd")
    return out


def depth_normals_bwd(depth, grad_normals, fg_max, scale=(1.0, 1.0), max_step=float("inf"), out=None):
    """depth_normals's backward (include/spherehand_hip.h, shr_depth_normals_bwd): grad_normals [B,3,H,W] -> grad_depth
    [B,H,W], the exact derivative with the forward's decisions held fixed; 0 at every pixel that is no site.  `out`: where
    to write (overlapping neither input)."""
    B, H, W, sx, sy, max_step = _depth_normals_args(depth, scale, max_step)
    _check_input(grad_normals, "grad_normals")
    if tuple(grad_normals.shape) != (B, 3, H, W) or grad_normals.device != depth.device:
        raise RuntimeError("grad_normals must be [B,3,H,W] for depth [B,H,W], on its device")
    if out is not None:
        _check_input(out, "out")
        if out.shape != depth.shape or out.device != depth.device:
            raise RuntimeError("out must be [B,H,W] as depth, on its device")
    with _on(depth.device):
        if out is None:
            out = torch.empty_like(depth)
        _lib.check(_lib.lib().shr_depth_normals_bwd(_ptr(depth), _ptr(grad_normals), B, W, H, float(fg_max), sx, sy,
                                                    max_step, _ptr(out), _stream()), "shr_depth_normals_bwd")
    return out


class DepthNormals(torch.autograd.Function):
    """depth_normals with a backward: (depth [B,H,W], fg_max, scale, max_step) -> normals [B,3,H,W], differentiable
    w.r.t. depth; which pixels have a normal and which neighbours each uses are held fixed."""

    @staticmethod
    def forward(ctx, depth, fg_max, scale=(1.0, 1.0), max_step=float("inf")):
        depth = depth.contiguous()
        ctx.args = (fg_max, tuple(scale), max_step)
        ctx.save_for_backward(depth)
        return depth_normals(depth, *ctx.args)

    @staticmethod
    def backward(ctx, grad_normals):
        depth, = ctx.saved_tensors
        return depth_normals_bwd(depth, grad_normals.contiguous().float(), *ctx.args), None, None, None


def hand_synth(params, offset, offset_inv, rng_state, rand_scale, lbs, faces, camera, out_size, depth_scale, noise,
               sigma_xy, sigma_z, heat=None, src_size=640, clamp_max=100.0):
    """HandSynthesizer.forward in ONE launch (shr_hand_synth_fwd), or None where that kernel does not apply (the caller
    then takes synth_pose / mesh_render_post / heatmap_render).  lbs: the mesh's SparseSkinning (tables + right_hand);
    heat: None (depth only) or (kp_start, kp_bone_i32, kp_wv, hm, (hcx, hcy, hfx, hfy), sigma, inv_k, uv_scale, d_scale).
    Returns (draws [6,B], depth [B,S,S], uv_hm, d_hm, xyz) -- the last three None without `heat`."""
    params = params.contiguous().float()
    B = params.shape[0]
    NV, F = lbs.skin_vertex_start.numel() - 1, faces.shape[0]
    J, hm = (heat[0].numel() - 1, int(heat[3])) if heat is not None else (0, 1)
    lib = _lib.lib()
    if params.dim() != 2 or params.shape[1] != 26 or not lib.shr_hand_synth_one_launch(17, NV, F, src_size, out_size, J, hm):
        return None
    _check_input(params, "parameters")
    _check_input(rng_state, "rng_state", torch.int64)
    dev = params.device
    cx, cy, fx, fy = camera
    with _on(dev):
        draws = torch.empty((6, B), dtype=torch.float32, device=dev)
        depth = torch.empty((B, out_size, out_size), dtype=torch.float32, device=dev)
        uv = d = xyz = None
        hargs = (0, None, None, None, 1, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
        if heat is not None:
            kp_start, kp_bone, kp_wv, _, hcam, hsigma, inv_k, uv_scale, d_scale = heat
            uv = torch.empty((B, J, hm, hm), dtype=torch.float32, device=dev)
            d = torch.empty((B, J, hm, hm), dtype=torch.float32, device=dev)
            xyz = torch.empty((B, J, 4), dtype=torch.float32, device=dev)
            hargs = (J, _ptr(kp_start), _ptr(kp_bone), _ptr(kp_wv), hm, hcam[0], hcam[1], hcam[2], hcam[3], float(hsigma),
                     float(uv_scale), float(d_scale), inv_k[0], inv_k[1], inv_k[2], inv_k[3])
        _lib.check(lib.shr_hand_synth_fwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), _ptr(rng_state), float(rand_scale), NV,
                                          _ptr(lbs.skin_vertex_start), _ptr(lbs.skin_bone), _ptr(lbs.skin_wv),
                                          int(bool(lbs.right_hand)), cx, cy, fx, fy, _ptr(faces), F, src_size, out_size,
                                          clamp_max, float(depth_scale), int(bool(noise)), float(sigma_xy), float(sigma_z),
                                          *hargs, _ptr(draws), _ptr(depth), _ptr(uv), _ptr(d), _ptr(xyz), _stream()),
                   "shr_hand_synth_fwd")
    return draws, depth, uv, d, xyz


def synth_pose(params, offset, offset_inv, rng_state, rand_scale):
    """pose [B,26] -> (diag(s) T [B,17,4,4], draws [6,B]): forward kinematics, RandScale and the samples' random draws in
    one launch (shr_synth_pose_fwd).  draws = s_x, s_y, s_z, focal jitter, and the two uint32 noise keys (as float bits);
    rng_state: int64 [2] = (seed, call counter) on the device (read only here)."""
    params = params.contiguous().float()
    for t, name in ((params, "parameters"), (offset, "offset"), (offset_inv, "offset_inv")):
        _check_input(t, name)
    _check_input(rng_state, "rng_state", torch.int64)
    if params.dim() != 2 or params.shape[1] != 26 or rng_state.numel() < 3:
        raise RuntimeError("parameters must be [B,26] and rng_state int64 [>= 3] (seed, call counter, ticket)")
    B = params.shape[0]
    with _on(params.device):
        T = torch.empty((B, 17, 4, 4), dtype=torch.float32, device=params.device)
        draws = torch.empty((6, B), dtype=torch.float32, device=params.device)
        _lib.check(_lib.lib().shr_synth_pose_fwd(_ptr(params), B, _ptr(offset), _ptr(offset_inv), _ptr(rng_state),
                                                 float(rand_scale), _ptr(T), _ptr(draws), _stream()), "shr_synth_pose_fwd")
    return T, draws


def mesh_render_post(T, skin_vertex_start, skin_bone, skin_wv, right_hand, camera, rand_f, faces, out_size, depth_scale,
                     noise_keys=None, sigma_xy=0.5, sigma_z=0.05, rng_state=None, src_size=640, clamp_max=100.0):
    """DepthRender + `* depth_scale` + DepthNoise as one call (shr_mesh_render_post_fwd): T [B,NB,4,4] -> [B,S,S].
    noise_keys: the samples' stream keys ([2,B] float32 view of uint32: synth_pose's draws[4:6]) or None = no noise;
    rng_state: the generator state whose call counter the launch advances (None: left alone)."""
    _check_input(T, "bone_transformations")
    _check_input(faces, "faces", torch.int32)
    if T.dim() != 4 or T.shape[2:] != (4, 4) or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("T must be [B,NB,4,4] and faces [F,3]")
    B, NB = T.shape[0], T.shape[1]
    NV = skin_vertex_start.numel() - 1
    cx, cy, fx, fy = camera
    lib = _lib.lib()
    with _on(T.device):
        depth = torch.empty((B, out_size, out_size), dtype=torch.float32, device=T.device)
        ws = dws = None
        if not lib.shr_mesh_render_one_launch(NB, NV, faces.shape[0], src_size, out_size):
            ws = torch.empty((B, NV, 4), dtype=torch.float32, device=T.device)
            dws = torch.empty_like(depth)
        _lib.check(lib.shr_mesh_render_post_fwd(_ptr(T), B, NB, NV, _ptr(skin_vertex_start), _ptr(skin_bone), _ptr(skin_wv),
                                                int(bool(right_hand)), cx, cy, fx, fy, _ptr(rand_f), _ptr(faces),
                                                faces.shape[0], src_size, out_size, clamp_max, float(depth_scale),
                                                _ptr(noise_keys), float(sigma_xy), float(sigma_z), _ptr(rng_state),
                                                _ptr(ws), _ptr(dws), _ptr(depth), _stream()), "shr_mesh_render_post_fwd")
    return depth


def heatmap_render(T, kp_start, kp_bone, kp_wv, right_hand, camera, rand_f, S, sigma, inv_k, uv_scale=1.0, d_scale=1.0):
    """Hand3DHeatmapRender in one launch (shr_heatmap_render_fwd): T [B,NB,4,4] -> (uv_hm [B,J,S,S] * uv_scale,
    d_hm [B,J,S,S] * d_scale, xyz [B,J,4]); kp_*: the key-points' CSR skin table (one entry each for the hand)."""
    _check_input(T, "bone_transformations")
    B, NB = T.shape[0], T.shape[1]
    J = kp_start.numel() - 1
    cx, cy, fx, fy = camera
    a00, a03, a11, a13 = inv_k
    with _on(T.device):
        uv = torch.empty((B, J, S, S), dtype=torch.float32, device=T.device)
        d = torch.empty((B, J, S, S), dtype=torch.float32, device=T.device)
        xyz = torch.empty((B, J, 4), dtype=torch.float32, device=T.device)
        _lib.check(_lib.lib().shr_heatmap_render_fwd(_ptr(T), B, NB, J, _ptr(kp_start), _ptr(kp_bone), _ptr(kp_wv),
                                                     int(bool(right_hand)), cx, cy, fx, fy, _ptr(rand_f), int(S), float(sigma),
                                                     float(uv_scale), float(d_scale), a00, a03, a11, a13, _ptr(uv), _ptr(d),
                                                     _ptr(xyz), _stream()), "shr_heatmap_render_fwd")
    return uv, d, xyz


def group_norm_relu_supported(x, num_groups):
    """True when the NHWC GroupNorm+ReLU kernels take this activation (CUDA fp32 or bf16, channels-last)."""
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 4 and x.shape[0] > 0
            and x.is_contiguous(memory_format=torch.channels_last)
            and bool(_lib.lib().shr_group_norm_relu_supported(int(x.shape[1]), int(num_groups))))


class GroupNormReLU(torch.autograd.Function):
    """relu(group_norm(x + pre_bias, G, weight, bias, eps)) on channels-last activations
    (network/hourglass.py:28-31), one kernel per direction.  `pre_bias` [C] (optional) is the bias of the
    convolution that produced x: the convolution is then run WITHOUT its bias, and this op's backward returns
    the bias gradient with dx (two launches and one reduction less per convolution).
    bf16 x (the hourglass under autocast): the bf16 kernel pair -- y, the saved x, dy and dx are bf16 channels-last,
    the parameters (fp32 master copies), mean, rstd and the parameter gradients fp32; the arithmetic is fp32.
    No autocast decorator: the Function reads x.dtype itself and takes the parameters as they are."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, pre_bias=None):
        N, C, H, W = x.shape
        weight, bias = weight.float().contiguous(), bias.float().contiguous()
        pre = None if pre_bias is None else pre_bias.float().contiguous()
        fwd = _lib.lib().shr_group_norm_relu_bf16_fwd if x.dtype == torch.bfloat16 else _lib.lib().shr_group_norm_relu_fwd
        with _on(x.device):
            y = torch.empty_like(x, memory_format=torch.channels_last)
            mean = torch.empty((N, num_groups), dtype=torch.float32, device=x.device)
            rstd = torch.empty((N, num_groups), dtype=torch.float32, device=x.device)
            _lib.check(fwd(_ptr(x), _ptr(pre), _ptr(weight), _ptr(bias), N, C, H * W, num_groups, float(eps), _ptr(y),
                           _ptr(mean), _ptr(rstd), _stream()), "shr_group_norm_relu_fwd")
        ctx.save_for_backward(x, weight, bias, mean, rstd, pre)
        ctx.num_groups = num_groups
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd, pre = ctx.saved_tensors
        N, C, H, W = x.shape
        dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        bwd = _lib.lib().shr_group_norm_relu_bf16_bwd if x.dtype == torch.bfloat16 else _lib.lib().shr_group_norm_relu_bwd
        k = 2 if pre is None else 3
        with _on(x.device):
            dx = torch.empty_like(x, memory_format=torch.channels_last)
            part = torch.empty((k, N, C), dtype=torch.float32, device=x.device)     # per-sample partials (workspace)
            dgb = torch.empty((k, C), dtype=torch.float32, device=x.device)
            _lib.check(bwd(_ptr(x), _ptr(pre), _ptr(dy), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(rstd), N, C, H * W,
                           ctx.num_groups, _ptr(dx), _ptr(part[0]), _ptr(part[1]),
                           _ptr(part[2]) if pre is not None else None, _ptr(dgb[0]), _ptr(dgb[1]),
                           _ptr(dgb[2]) if pre is not None else None, _stream()), "shr_group_norm_relu_bwd")
        return dx, dgb[0], dgb[1], None, None, (dgb[2] if pre is not None else None)


FUSED_GROUP_NORM_RELU = True    # False: always torch's group_norm + relu (A/B measurements)


def group_norm_relu(x, gn, pre_bias=None):
    """F.relu(gn(x + pre_bias)) for an nn.GroupNorm `gn`: the NHWC kernels when they apply, torch otherwise."""
    if FUSED_GROUP_NORM_RELU and gn.affine and group_norm_relu_supported(x, gn.num_groups):
        return GroupNormReLU.apply(x, gn.weight, gn.bias, gn.num_groups, gn.eps, pre_bias)
    if pre_bias is not None:
        x = x + pre_bias.view(1, -1, 1, 1)
    return torch.nn.functional.relu(gn(x))


def conv_then_group_norm_relu(x, conv, gn):
    """relu(gn(conv(x))) with the convolution's bias folded into the normalisation kernel when that kernel will
    take conv's output (NHWC fp32 or bf16 on the GPU, supported channel counts): conv runs bias-free.  Under CUDA
    autocast to bf16 the convolution's output is bf16 whatever x is; it then feeds the bf16 kernels and conv.bias
    (fp32) rides as their pre_bias."""
    # (F.conv2d below bypasses conv.forward: only for a plain zero-padded convolution without hooks or
    # parametrizations; the kernel reads the bias 16 bytes at a time)
    plain = (conv.padding_mode == 'zeros' and not conv._forward_hooks and not conv._forward_pre_hooks
             and not getattr(conv, 'parametrizations', None) and conv.bias is not None
             and conv.bias.data_ptr() % 16 == 0 and conv.bias.is_contiguous())
    if (FUSED_GROUP_NORM_RELU and gn.affine and plain and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16)
            and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and bool(_lib.lib().shr_group_norm_relu_supported(int(conv.out_channels), int(gn.num_groups)))):
        y = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
        if y.dtype == torch.bfloat16:      # (a one-channel input leaves the layout to the solver: one copy, not torch's path)
            y = y.contiguous(memory_format=torch.channels_last)
        if group_norm_relu_supported(y, gn.num_groups):
            return GroupNormReLU.apply(y, gn.weight, gn.bias, gn.num_groups, gn.eps, conv.bias)
        return torch.nn.functional.relu(gn(y + conv.bias.view(1, -1, 1, 1)))
    return group_norm_relu(conv(x), gn)


def heatmap_paint(uvd, S, sigma, inv_k, uv_scale=1.0, d_scale=1.0):
    """uvd [B,J,4] heat-map-space key-points -> (uv_hm [B,J,S,S] * uv_scale, d_hm [B,J,S,S] * d_scale,
    xyz [B,J,4] = inv_k @ uvd): HeatmapRender + InverseOthographicalProjection in one launch."""
    _check_input(uvd, "uvd_points")
    if uvd.dim() != 3 or uvd.shape[2] != 4:
        raise RuntimeError("uvd_points must be [B,J,4]")
    B, J = uvd.shape[0], uvd.shape[1]
    a00, a03, a11, a13 = (float(inv_k[0][0]), float(inv_k[0][3]), float(inv_k[1][1]), float(inv_k[1][3]))
    with _on(uvd.device):
        uv = torch.empty((B, J, S, S), dtype=torch.float32, device=uvd.device)
        d = torch.empty((B, J, S, S), dtype=torch.float32, device=uvd.device)
        xyz = torch.empty((B, J, 4), dtype=torch.float32, device=uvd.device)
        _lib.check(_lib.lib().shr_heatmap_paint(_ptr(uvd), B * J, int(S), float(sigma), float(uv_scale), float(d_scale),
                                                a00, a03, a11, a13, _ptr(uv), _ptr(d), _ptr(xyz), _stream()),
                   "shr_heatmap_paint")
    return uv, d, xyz


def depth_noise(depth, sigma_xy, sigma_z, generator=None):
    """DepthNoise on [B,H,W] scaled depth: one torch.randn([3,B,H,W]) + one launch."""
    _check_input(depth, "depth")
    B, H, W = depth.shape
    with _on(depth.device):
        normal3 = torch.randn((3, B, H, W), dtype=torch.float32, device=depth.device, generator=generator)
        out = torch.empty_like(depth)
        _lib.check(_lib.lib().shr_depth_noise(_ptr(depth), _ptr(normal3), B, H, W, float(sigma_xy), float(sigma_z),
                                              _ptr(out), _stream()), "shr_depth_noise")
    return out


def soft_argmax_supported(hm, J):
    """True when the soft-argmax kernels take this raw network output (CUDA fp32 [N,2J,h,w], pixels
    linear in memory: NCHW or channels-last, also as a batch slice)."""
    if not (hm.is_cuda and hm.dtype == torch.float32 and hm.dim() == 4 and hm.shape[1] == 2 * J and hm.shape[0] > 0):
        return False
    h, w = hm.shape[2], hm.shape[3]
    if hm.stride(2) != w * hm.stride(3) or hm.stride(3) < 1 or hm.stride(1) < 1:
        return False
    return bool(_lib.lib().shr_soft_argmax_supported(int(J), int(h), int(w)))


class SoftArgmaxXYZ(torch.autograd.Function):
    """hm [N,2J,h,w] (uv heat-maps | depth heat-maps) -> xyz [N,J,3]: RecoverXYZCoordinateFromHeatmap
    (network/util_modules.py:164-201) in one launch per direction."""

    @staticmethod
    def forward(ctx, hm, J, cx, cy, fx, fy, depth_scale_inv):
        N, _, h, w = hm.shape
        with _on(hm.device):
            xyz = torch.empty((N, J, 3), dtype=torch.float32, device=hm.device)
            _lib.check(_lib.lib().shr_soft_argmax_fwd(_ptr(hm), hm.stride(0), hm.stride(1), hm.stride(3), N, J, h, w,
                                                      float(cx), float(cy), float(fx), float(fy), float(depth_scale_inv),
                                                      _ptr(xyz), _stream()), "shr_soft_argmax_fwd")
        ctx.save_for_backward(hm)
        ctx.args = (J, cx, cy, fx, fy, depth_scale_inv)
        return xyz

    @staticmethod
    def backward(ctx, grad_xyz):
        (hm,) = ctx.saved_tensors
        J, cx, cy, fx, fy, ds = ctx.args
        N, _, h, w = hm.shape
        grad_xyz = grad_xyz.contiguous()
        with _on(hm.device):
            grad_hm = torch.empty_strided(hm.shape, hm.stride(), dtype=torch.float32, device=hm.device)
            _lib.check(_lib.lib().shr_soft_argmax_bwd(_ptr(hm), hm.stride(0), hm.stride(1), hm.stride(3), N, J, h, w,
                                                      float(cx), float(cy), float(fx), float(fy), float(ds),
                                                      _ptr(grad_xyz), _ptr(grad_hm), _stream()), "shr_soft_argmax_bwd")
        return grad_hm, None, None, None, None, None, None


class PairLosses(torch.autograd.Function):
    """(joints [B,P,3] with P >= J: the first J points of a sample are its sphere centres, as the reference's
    `joints.view(B, -1, 3)` indexing implies) -> (collision loss, bone-length loss) of mesh/render.py:145-206
    with the reference's reductions (sum; mean of the two hinges over [B,K]).  One launch; the backward only
    scales the unit gradients the kernel already produced."""

    @staticmethod
    def forward(ctx, joints, J, num_palm, per_finger, min_dist_sq, bone_a, bone_b, bone_min_sq, bone_max_sq):
        joints = joints.contiguous()
        B, P = joints.shape[0], joints.shape[1]
        K = bone_a.numel()
        with _on(joints.device):
            sums = torch.empty((3, B), dtype=torch.float32, device=joints.device)
            grads = torch.empty((3, B, J, 3), dtype=torch.float32, device=joints.device)
            _lib.check(_lib.lib().shr_pair_losses(_ptr(joints), P * 3, B, J, int(num_palm), int(per_finger),
                                                  float(min_dist_sq), _ptr(bone_a), _ptr(bone_b), _ptr(bone_min_sq),
                                                  _ptr(bone_max_sq), K, _ptr(sums[0]), _ptr(sums[1]), _ptr(sums[2]),
                                                  _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _stream()),
                       "shr_pair_losses")
        ctx.save_for_backward(grads)
        ctx.meta = (B, P, J, K)
        tot = sums.sum(dim=1)
        return tot[0], (tot[1] + tot[2]) / float(B * K)

    @staticmethod
    def backward(ctx, g_coll, g_bone):
        (grads,) = ctx.saved_tensors
        B, P, J, K = ctx.meta
        g = grads[0] * g_coll + (grads[1] + grads[2]) * (g_bone / float(B * K))
        if P > J:
            full = torch.zeros((B, P, 3), dtype=torch.float32, device=g.device)
            full[:, :J] = g
            g = full
        return g, None, None, None, None, None, None, None, None


class MultiviewConsistency(torch.autograd.Function):
    """(camera_poses [B,V,4,4], joints [B,V,J,3]) -> MSELoss(median over the views, canonical points): the
    reference's MultiviewConsistencyLoss without heat-map weights (mesh/multiview_utility.py:138-167), one launch;
    the backward only scales the unit gradient the kernel already produced."""

    @staticmethod
    def forward(ctx, camera_poses, joints):
        cam = camera_poses.detach().contiguous().float()
        joints = joints.contiguous().float()
        _check_input(cam, "camera_poses")
        _check_input(joints, "joints")
        B, V, J = joints.shape[0], joints.shape[1], joints.shape[2]
        if cam.shape != (B, V, 4, 4) or joints.dim() != 4 or joints.shape[3] != 3:
            raise RuntimeError("expected camera_poses [B,V,4,4] and joints [B,V,J,3]")
        want = ctx.needs_input_grad[1]
        with _on(joints.device):
            sums = torch.empty(B, dtype=torch.float32, device=joints.device)
            grad = torch.empty((B, V, J, 3), dtype=torch.float32, device=joints.device) if want else None
            _lib.check(_lib.lib().shr_mv_consistency(_ptr(cam), _ptr(joints), B, V, J, _ptr(sums), _ptr(grad), _stream()),
                       "shr_mv_consistency")
        if want:
            ctx.save_for_backward(grad)
        ctx.count = float(B * V * J * 3)
        return sums.sum() / ctx.count

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return None, grad * (g / ctx.count)


def mv_consistency_supported(camera_poses, joints):
    return (joints.is_cuda and camera_poses.is_cuda and joints.dim() == 4 and joints.shape[-1] == 3
            and joints.shape[1] <= 8 and joints.shape[2] <= 64 and joints.dtype == torch.float32)


def depth_resample(depth, sample_ratio, kernel_size, generator=None):
    """DepthResample on [N,H,W] scaled depth: one torch.rand + one launch -> [N,1,H,W]."""
    _check_input(depth, "depth")
    N, H, W = depth.shape
    with _on(depth.device):
        uniform = torch.rand((N, H, W), dtype=torch.float32, device=depth.device, generator=generator)
        out = torch.empty((N, 1, H, W), dtype=torch.float32, device=depth.device)
        _lib.check(_lib.lib().shr_depth_resample(_ptr(depth), _ptr(uniform), N, H, W, float(sample_ratio),
                                                 int(kernel_size), _ptr(out), _stream()), "shr_depth_resample")
    return out
