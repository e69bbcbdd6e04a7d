"""A numpy restatement of the pose-VAE prior of the sphere fit (spherehand_amd/csrc/pose_vae.hip; include/spherehand_hip.h,
the section of shr_pose_vae_normal), on tests/pose_ik_ref.py's chain, which it does not change (test helper; not a conftest):

    weights        the shipped network's arrays in a dtype
    unpack_mask    relu_mask [B,32] uint32 -> [B,4,256] bool in the header's bit order (pack_mask inverts it)
    forward        the value and the 26 tangents through the network as one matrix, in the given dtype: r, J_r, mu, mu' and
                   every ReLU input; the ReLU decisions are its own or GIVEN
    normal         A, g, cost (weighted) from those rows, every sum in fp64 by a matrix product -- no order of the kernel's
    inputs         (c [B,41,3], jac [B,123,26]) of a pose on the fp64 chain
    cases          the inputs of the GPU tests, on which the fp32 bars are measured
    translation    how the residual of plausible poses grows under a global translation

The network works on x = c / 100; the contract takes that quotient in fp32 (`x=`), the fp64 function of the CPU tests in fp64."""
import numpy as np
import torch

import pose_ik_ref as ik

EPS = 1e-5
GN_LAYERS = ("base.1", "base.4", "decoder.1", "decoder.4")


def weights(dtype=np.float64):
    from spherehand_amd import pose_vae
    with np.load(pose_vae.DEFAULT_WEIGHTS) as z:
        return {k: z[k].astype(dtype) for k in z.files}


def unpack_mask(words):
    """[B,32] uint32 (or int32) -> [B,4,256] bool: unit u = 256 layer + channel is bit u & 31 of word u >> 5."""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, 32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(-1, 4, 256).astype(bool)


def pack_mask(mask):
    m = np.asarray(mask, bool).reshape(-1, 32, 32).astype(np.uint32)
    return (m << np.arange(32, dtype=np.uint32)[None, None, :]).sum(-1).astype(np.uint32)


def _linear(W, b, M):
    H = np.matmul(W[None], M)                 # [B,out,27]
    H[:, :, 0] += b[None]
    return H


def _gn_relu(H, gamma, beta, given):
    """GroupNorm(16 groups of 16, biased variance, eps 1e-5) and ReLU of value and tangents -> (out, y the ReLU input of
    the value column [B,256], the decisions used [B,256])."""
    B = H.shape[0]
    dt = H.dtype
    h = H[:, :, 0].reshape(B, 16, 16)
    m = h.mean(2, keepdims=True)
    d = h - m
    rs = 1 / np.sqrt((d * d).mean(2, keepdims=True) + dt.type(EPS))
    hh = d * rs
    y = hh.reshape(B, 256) * gamma[None] + beta[None]
    t = H[:, :, 1:].reshape(B, 16, 16, -1)
    m1 = t.mean(2, keepdims=True)
    m2 = (hh[..., None] * t).mean(2, keepdims=True)
    yt = (gamma.reshape(1, 16, 16) * rs)[..., None] * ((t - m1) - hh[..., None] * m2)
    on = (y > 0) if given is None else given
    out = np.concatenate([y[:, :, None], yt.reshape(B, 256, -1)], 2)
    return np.where(on[:, :, None], out, dt.type(0)), y, on


def forward(c, jac, dtype=np.float64, mask=None, x=None, W=None):
    """c [B,41,3] mm and jac [B,123,26] -> dict of r [B,123] and J_r [B,123,26] (fp64 from the dtype's network outputs, as
    the entry forms its rows), mu [B,32], dmu [B,32,26], relu_in [B,4,256] (the value column's ReLU inputs, dtype), mask
    [B,4,256] the decisions used: its own, or GIVEN (`mask`).  x [B,123]: the network's input where it is not c / 100 in
    the dtype (the contract's fp32 quotient)."""
    dtype = np.dtype(dtype)
    W = weights(dtype) if W is None else W
    c = np.asarray(c)[..., :3].reshape(-1, 123)
    B = c.shape[0]
    x = (c.astype(dtype) / dtype.type(100)) if x is None else np.asarray(x).reshape(B, 123).astype(dtype)
    jac = np.asarray(jac).reshape(B, 123, 26)
    M = np.concatenate([x[:, :, None], jac.astype(dtype)], 2)
    relu_in, used = [], []

    def hidden(M, lin, gn, layer):
        out, y, on = _gn_relu(_linear(W[lin + ".weight"], W[lin + ".bias"], M), W[gn + ".weight"], W[gn + ".bias"],
                              None if mask is None else mask[:, layer])
        relu_in.append(y)
        used.append(on)
        return out

    M = hidden(M, "base.0", "base.1", 0)
    M = hidden(M, "base.3", "base.4", 1)
    L = _linear(W["mu.weight"], W["mu.bias"], M)
    M = hidden(L, "decoder.0", "decoder.1", 2)
    M = hidden(M, "decoder.3", "decoder.4", 3)
    R = _linear(W["decoder.6.weight"], W["decoder.6.bias"], M)
    r = 100.0 * (x.astype(np.float64) - R[:, :, 0].astype(np.float64))
    Jr = jac.astype(np.float64) - R[:, :, 1:].astype(np.float64)
    return dict(r=r, J=Jr, mu=L[:, :, 0].astype(np.float64), dmu=L[:, :, 1:].astype(np.float64), recon=R[:, :, 0],
                relu_in=np.stack(relu_in, 1), mask=np.stack(used, 1), x=x)


def normal(f, weight=1.0, latent_weight=0.0):
    """(A [B,26,26], g [B,26], cost [B]) fp64 of forward()'s dict: weight (S + lw S_l), ... with the weights rounded to fp32
    as the entry takes them."""
    w, lw = float(np.float32(weight)), float(np.float32(latent_weight))
    A = np.einsum("bia,bic->bac", f["J"], f["J"])
    g = np.einsum("bi,bia->ba", f["r"], f["J"])
    cost = (f["r"] * f["r"]).sum(1)
    if lw > 0:
        A = A + lw * np.einsum("bka,bkc->bac", f["dmu"], f["dmu"])
        g = g + lw * np.einsum("bk,bka->ba", f["mu"], f["dmu"])
        cost = cost + lw * (f["mu"] * f["mu"]).sum(1)
    return w * A, w * g, w * cost


def inputs(chain, p):
    """(c [B,41,3], jac [B,123,26]) numpy in the chain's dtype."""
    k, j = chain.jacobian(torch.as_tensor(p))
    return k.numpy(), j.numpy()


def term(model, p, weight, latent_weight=0.0):
    """(A, g, cost) torch fp64 of the term at pose p on the model's chain, in the chain's dtype."""
    c, j = model.chain.jacobian(p)
    dt = np.float32 if model.dtype == torch.float32 else np.float64
    f = forward(c.numpy(), j.numpy(), dt)
    return tuple(torch.as_tensor(t) for t in normal(f, weight, latent_weight)) + (f,)


def combined(model, view, observed, p, p2m, vae=None, tab=None, collision_weight=0.0, **prior):
    """(A, g, cost, f) at pose p: sphere_collision_ref.combined plus the term, one sum per entry; vae = (weight,
    latent_weight) or None; f is forward()'s dict, None where the loop issues no launch of the entry."""
    import sphere_collision_ref as cref
    A, g, cost, _ = cref.combined(model, view, observed, p, p2m, tab, collision_weight, **prior)
    if vae is None or not vae[0] > 0:
        return A, g, cost, None
    a, gg, c, f = term(model, p, *vae)
    return A + a, g + gg, cost + c, f


def solve(model, view, observed, params0, p2m, vae=None, tab=None, collision_weight=0.0, iters=10, lambda0=1e-3, stiffness=None,
          prior=None, **terms):
    """The loop of ops.sphere_icp_priors with the term in model.dtype -> (params, cost0, cost, lm); lm.masks: per evaluation
    the [B,4,256] ReLU decisions (None without the term)."""
    import pose_icp_ref as ref
    start = params0.float().double() if model.dtype == torch.float32 else params0.double()
    lm = ref.LM(start, lambda0, model.dtype)
    lm.masks = []
    trial = lm.trial
    for it in range(iters + 1):
        A, g, cost, f = combined(model, view, observed, trial, p2m, vae, tab, collision_weight, **terms)
        lm.masks.append(None if f is None else torch.as_tensor(f["mask"]))
        out = lm.step(A, g, cost, trial, prior, stiffness, solve=it < iters)
        trial = out if out is not None else trial
    return lm.p, lm.cost0, lm.cost, lm


# ---- the GPU tests' inputs ----------------------------------------------------------------------------------------------
_CACHE = {}


def poses():
    """[8,26] fp32: the rest pose, six of joint_angle.sample_poses(64, seed=3), and one pose at pose_limits()."""
    from spherehand_amd import joint_angle
    s = np.asarray(joint_angle.sample_poses(64, seed=3), np.float32).reshape(64, 26)
    lo, hi = (np.asarray(t, np.float32).reshape(26) for t in joint_angle.pose_limits())
    edge = np.where(np.arange(26) % 2 == 0, lo, hi).astype(np.float32)
    edge = np.where(np.isfinite(edge), edge, 0).astype(np.float32)
    return np.concatenate([np.zeros((1, 26), np.float32), s[:6], edge[None]], 0)


def cached_cases(mesh):
    """[{name, right_hand, params [B,26] fp32, c, jac (the fp64 chain's, rounded to fp32: what the entry is handed up to
    the chain's own fp32 error)}]: both hands, B in {0, 1, 3, 5} -- once per process."""
    if "cases" not in _CACHE:
        P = poses()
        out = []
        for name, right, rows in (("right1", True, [0]), ("right3", True, [1, 2, 7]), ("right5", True, [0, 3, 4, 5, 7]),
                                  ("left3", False, [6, 7, 0]), ("left5", False, [1, 2, 3, 4, 5]), ("empty", True, [])):
            p = P[rows].reshape(-1, 26)
            chain = ik.Chain(mesh, right_hand=right)
            if len(rows):
                c, j = inputs(chain, p.astype(np.float64))
            else:
                c, j = np.zeros((0, 41, 3)), np.zeros((0, 123, 26))
            out.append(dict(name=name, right_hand=right, params=p, c=c.astype(np.float32), jac=j.astype(np.float32)))
        _CACHE["cases"] = out
    return _CACHE["cases"]


# ---- the study ----------------------------------------------------------------------------------------------------------
STUDY_WEIGHTS = (0.0, 0.01, 0.1, 1.0, 10.0)
STUDY_LATENT_WEIGHTS = (0.0, 100.0)


def study_frames(mesh, family, weights=STUDY_WEIGHTS, latent_weights=(0.0,), poses=slice(None), W=48, H=40, iters=10, sigma=5.0):
    """The frame fitter's rows of the study by THIS FILE's fp64 loop on the CPU (4.4s's set-up: the 20 poses of 4.4q, one view,
    keypoints with sigma mm of noise, the other terms at their defaults; `blind` drops the hidden finger's keypoints):
    [{weight, latent_weight, mean, hidden}]."""
    import pose_icp_ref as ref
    import pose_icp_views_ref as vref
    import sphere_collision_ref as cref
    import sphere_icp_ref as sref
    import sphere_prior_ref as pref
    import sphere_render_icp_ref as rref
    model = sref.Spheres(mesh, None, True)
    p2m = ref.grid(W, H)
    p, p0 = (t[poses] for t in rref.study_poses(family))
    view = vref.views(p.shape[0], ("identity",))
    obs = rref.render64(model, view, p, W, H, p2m)
    k = pref.targets(model, view, p, sigma, seed=3)
    finger = hidden_finger(model, p)
    if family == "blind":
        k[:, :, finger] = np.nan
    lo, hi = pref.limits()
    terms = dict(keypoints=k, confidence=None, kp_weight=pref.DEFAULT_KP_WEIGHT, kp_max=pref.DEFAULT_KP_MAX, lower=lo, upper=hi,
                 limit_weight=pref.DEFAULT_LIMIT_WEIGHT)
    rows = []
    for w in weights:
        for lw in (latent_weights if w > 0 else (0.0,)):
            q = solve(model, view, obs, p0, p2m, (w, lw), cref.table(mesh), cref.DEFAULT_COLLISION_WEIGHT, iters, 1e-3,
                      torch.as_tensor(ref.STIFFNESS), **terms)[0]
            fe = (model.centres(q) - model.centres(p)).detach().norm(dim=-1)
            rows.append(dict(weight=w, latent_weight=lw, mean=fe.mean().item(), hidden=fe[:, finger].mean().item()))
    return rows


def hidden_finger(model, p):
    """The spheres the index finger's three flexes move."""
    import sphere_render_icp_ref as rref
    c0 = model.centres(p).detach()
    q = p.clone()
    q[:, rref.FINGER + 1:rref.FINGER + 4] += 0.5
    return np.nonzero((model.centres(q).detach() - c0).norm(dim=-1).max(0).values.numpy() > 1e-9)[0]


def study(mesh, W=48, H=40, S=3, T=8, N=12, win=4, iters=10, sigma=5.0, weights=STUDY_WEIGHTS, latent_weights=STUDY_LATENT_WEIGHTS,
          families=("noise", "blind"), out=print):
    """The table of DESIGN.md 4.4zzz, through the library's classes on a GPU (the three loops have no common restatement):
    4.4t / u / z's set-up (S sequences, one view, keypoints with sigma mm of noise, `noise` and `blind`; `blind` hides the index
    finger in some frames: no keypoints there, the start extended) for
        frame    SphereCollisionPoseFitter on the S T frames, each on its own
        traj     SphereTrajectoryPoseFitter over sequences of T frames
        tracker  SphereWindowTracker.track, windows of `win` over N frames, the smoothed poses
    over the prior's weight x latent_weight: the mean keypoint error, the jitter, the hidden finger's error in its frames.
    Then the rms of r under a global translation (translation())."""
    import pose_icp_ref as ref
    import pose_icp_views_ref as vref
    import sphere_icp_ref as sref
    import sphere_prior_ref as pref
    import sphere_render_icp_ref as rref
    import sphere_sequence_ref as qref
    import sphere_trajectory_ref as tref
    from spherehand_amd.render import PoseVaePrior, SphereCollisionPoseFitter, SphereTrajectoryPoseFitter, SphereWindowTracker
    model = sref.Spheres(mesh, None, True)
    p2m = ref.grid(W, H)
    rows = []
    for family in families:
        for kind, n in (("frame", T), ("traj", T), ("tracker", N)):
            p, p0, hidden = tref.study_sequences(family, S, n)
            B = S * n
            view = vref.views(B, ("identity",))
            obs = rref.render64(model, view, p, W, H, p2m)
            k = pref.targets(model, view, p, sigma, seed=3)
            finger = hidden_finger(model, p)
            if family == "blind":
                k[np.ix_(np.nonzero(hidden.numpy())[0], [0], finger)] = np.nan
            dev = lambda t: torch.as_tensor(np.asarray(t)).float().cuda().contiguous()   # noqa: E731
            obs_d, p0_d, view_d, k_d = dev(obs), dev(p0), dev(view), dev(k)
            for w in weights:
                for lw in (latent_weights if w > 0 else (0.0,)):
                    kw = dict(pixel_to_model=p2m, iters=iters, stiffness=np.asarray(ref.STIFFNESS, np.float32),
                              pose_prior=PoseVaePrior(weight=w, latent_weight=lw) if w > 0 else None)
                    if kind == "frame":
                        q = SphereCollisionPoseFitter(mesh, W, H, **kw).cuda().solve(obs_d, p0_d, view_d, keypoints=k_d)[0]
                    elif kind == "traj":
                        q = SphereTrajectoryPoseFitter(mesh, W, H, T, **kw).cuda().solve(obs_d, p0_d, view_d, keypoints=k_d)[0]
                    else:
                        per = lambda t: t.view((S, N) + tuple(t.shape[1:]))   # noqa: E731
                        q = SphereWindowTracker(mesh, W, H, win, **kw).cuda().track(per(obs_d), per(p0_d), per(view_d),
                                                                                    per(k_d))[0].reshape(B, 26)
                    q = q.double().cpu()
                    err, jit = sref.keypoint_error(model, q, p), qref.jitter(model, q, p, n)
                    row = dict(family=family, kind=kind, weight=w, latent_weight=lw, mean=err.mean().item(), jitter=jit.mean().item())
                    if family == "blind":
                        fe = (model.centres(q) - model.centres(p)).detach().norm(dim=-1)[:, finger].mean(1)
                        row["hidden"] = fe[hidden].mean().item()
                    rows.append(row)
                    out("%-5s %-7s w %-5g lw %-4g: error %.2f mm, jitter %.2f mm%s"
                        % (family, kind, w, lw, row["mean"], row["jitter"],
                           "" if "hidden" not in row else "; the hidden finger in its frames %.2f mm" % row["hidden"]))
    out("rms of r under a translation along x (mm -> mm): %s" % translation(mesh))
    return rows


def translation(mesh, shifts=(0.0, 10.0, 30.0, 100.0), n=64, seed=3):
    """{shift mm: rms of r in mm over n sampled poses with every centre moved by `shift` along x} -- the VAE saw the
    global pose in training, so the residual of a plausible pose is not invariant."""
    from spherehand_amd import joint_angle
    p = np.asarray(joint_angle.sample_poses(n, seed=seed), np.float64).reshape(n, 26)
    c, j = inputs(ik.Chain(mesh), p)
    out = {}
    for s in shifts:
        f = forward(c + np.array([s, 0.0, 0.0]), j)
        out[s] = float(np.sqrt((f["r"] ** 2).mean()))
    return out


if __name__ == "__main__":
    from spherehand_amd import hand_model
    study(hand_model.load_mesh())
