"""A restatement of the constant-velocity term of the sphere model's sequence fit and of the block-pentadiagonal step
(spherehand_amd/csrc/sphere_accel.hip and lm_seq2.hip; include/spherehand_hip.h, the section of shr_sphere_accel_normal and
shr_pose_lm_seq2_step), on top of tests/sphere_sequence_ref.py and its family, none of which it changes (test helper; not a
conftest):

    decide         per (triple, sphere): a, n2, valid, the cost term and whether it has rows -- the header's rules in numpy
                   fp64 on fp32 centres; arrays are indexed by the triple's CENTRE frame
    energy         the torch expression of the cost per frame (a triple's cost at its last frame), differentiable in p
    normal         A, g, E, F, cost, count by AUTOGRAD: the Jacobian of a sequence's stacked residuals with respect to all
                   of its 26 T parameters, H = J^T W J cut into blocks; nothing about +Jc, -2 Jc, +Jc is stated
    chain          A, g, E, F, cost, count in the header's summation order, operation for operation, GIVEN the entry's own
                   fp32 centres and Jacobian: what the entry gives
    block_solve    shr_pose_lm_seq2_step's block Cholesky with bandwidth two, forward and back substitution word for word
    dense_solve    the 26 T x 26 T system assembled densely and solved by numpy.linalg.solve: the independent check
    Seq2LM         shr_pose_lm_seq2_begin / _step: sphere_sequence_ref.SeqLM with F; without F it IS SeqLM's step
    combined/solve the loop of ops.sphere_icp_trajectory on sphere_sequence_ref.combined
    study          DESIGN.md 4.4u's table

dtype is the chain's, as in sphere_icp_ref."""
import numpy as np
import torch

import pose_icp_ref as ref
import pose_icp_views_ref as vref
import sphere_collision_ref as cref
import sphere_icp_ref as sref
import sphere_prior_ref as pref
import sphere_render_icp_ref as rref
import sphere_sequence_ref as qref

INF = float("inf")
# render.SphereTrajectoryPoseFitter's defaults
DEFAULT_TEMPORAL_WEIGHT, DEFAULT_ACCEL_WEIGHT, DEFAULT_ACC_MAX = 0.0, 0.1, 20.0


def _weights(B, T, triple_weight):
    """[B] fp64: the weight of the triple CENTRED at b, 0 where b is the first or last frame of its sequence or the weight is
    not > 0."""
    fw = np.ones(B, np.float32) if triple_weight is None else np.asarray(triple_weight, np.float32)
    t = np.arange(B) % T
    with np.errstate(invalid="ignore"):
        live = (t >= 1) & (t <= T - 2) & (fw > 0)
    return np.where(live, fw.astype(np.float64), 0.0), live


def decide(centres32, T, acc_max=INF, triple_weight=None):
    """dict over [B,J] indexed by the triple's CENTRE frame: a [B,J,3] = (c(b - 1) + c(b + 1)) - 2 c(b), n2, valid (the triple
    has a weight and n2 is no NaN), act (rows: n2 < cap2), term (min(n2, cap2), 0 where not valid); fw [B], live [B]."""
    c = np.asarray(centres32, np.float32)[..., :3].astype(np.float64)
    B = c.shape[0]
    fw, live = _weights(B, T, triple_weight)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.roll(c, 1, axis=0) + np.roll(c, -1, axis=0)) - 2.0 * c
        n2 = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        cap2 = np.float64(np.float32(acc_max)) * np.float64(np.float32(acc_max))
        valid = live[:, None] & ~np.isnan(n2)
        act = valid & (n2 < cap2)
        term = np.where(valid, np.where(act, n2, cap2), 0.0)
    return dict(a=a, n2=n2, valid=valid, act=act, term=term, fw=fw, live=live, cap2=cap2)


def _to_last(x, B, T, zero):
    """a per-triple value indexed by the centre frame, moved to the triple's LAST frame; `zero` at a sequence's first two"""
    return np.where(np.arange(B) % T >= 2, np.roll(x, 1), zero)


def energy(model, p, T, accel_weight=1.0, acc_max=INF, triple_weight=None, held=None):
    """cost [B] as a torch expression of p: the triple centred at b - 1 pays at frame b, w sum_j min(n2, cap2), the set with
    rows decided at p itself or held (decide()'s dict)."""
    c = model.centres(p).double()
    B = c.shape[0]
    d = decide(c.detach().numpy(), T, acc_max, triple_weight) if held is None else held
    a = (torch.roll(c, 1, 0) + torch.roll(c, -1, 0)) - 2.0 * c
    n2 = (a * a).sum(-1)
    cap = torch.full_like(n2, float(min(d["cap2"], 1.7e308)))
    t = torch.where(torch.as_tensor(d["act"]), n2, torch.where(torch.as_tensor(d["valid"]), cap, torch.zeros_like(n2)))
    w = float(np.float32(accel_weight)) * torch.as_tensor(d["fw"])
    triple = w * t.sum(1)                                      # at the centre frame
    return torch.roll(triple, 1, 0) * torch.as_tensor((np.arange(B) % T >= 2).astype(np.float64))


def normal(model, p, T, accel_weight=1.0, acc_max=INF, triple_weight=None, centres32=None, chain_residual=False):
    """dict of A, E, F [B,26,26], g [B,26], cost [B], count [B] by autograd through the chain: per sequence the Jacobian of the
    stacked residuals a of the spheres with rows with respect to the sequence's [T,26] parameters.  centres32: the centres
    the rows are decided on (the kernel's own), default the model's rounded once.  chain_residual: the chain's own a in g
    (whose gradient g then is) instead of the contract's."""
    B = p.shape[0]
    aw = float(np.float32(accel_weight))
    c32 = model.centres(p.to(model.dtype)).detach().float().numpy() if centres32 is None else np.asarray(centres32, np.float32)
    d = decide(c32, T, acc_max, triple_weight)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)        # noqa: E731
    A, g, E, F = z(B, 26, 26), z(B, 26), z(B, 26, 26), z(B, 26, 26)
    for s in range(B // T if aw > 0 else 0):
        rows_ = slice(s * T, s * T + T)
        act = torch.as_tensor(d["act"][rows_])
        if not bool(act.any()):
            continue
        w = (aw * torch.as_tensor(d["fw"][rows_]))[:, None, None].expand(T, act.shape[1], 3)[act]

        def resid(P):
            c = model.centres(P).double()
            return ((torch.roll(c, 1, 0) + torch.roll(c, -1, 0)) - 2.0 * c)[act]   # [N,3] of the (triple, sphere) with rows

        P = p[rows_].detach().to(model.dtype)
        Jr = torch.autograd.functional.jacobian(resid, P).double().reshape(-1, T * 26)
        r = torch.as_tensor(d["a"][rows_])[act].reshape(-1)    # the contract's a: fp64 on the fp32 centres
        if chain_residual:
            r = resid(P).detach().double().reshape(-1)
        H = (Jr * w.reshape(-1, 1)).t() @ Jr
        G = Jr.t() @ (w.reshape(-1) * r)
        for t in range(T):
            A[s * T + t] = H[26 * t:26 * t + 26, 26 * t:26 * t + 26]
            g[s * T + t] = G[26 * t:26 * t + 26]
            if t < T - 1:
                E[s * T + t] = H[26 * t:26 * t + 26, 26 * t + 26:26 * t + 52]
            if t < T - 2:
                F[s * T + t] = H[26 * t:26 * t + 26, 26 * t + 52:26 * t + 78]
    cost = torch.as_tensor(_to_last(aw * d["fw"] * d["term"].sum(1), B, T, 0.0))
    count = torch.as_tensor(_to_last(d["act"].sum(1), B, T, 0))
    return dict(A=A, g=g, E=E, F=F, cost=cost, count=count, decided=d)


def _gram(x, y):
    """[26,26]: ((x0 y0 + x1 y1) + x2 y2) per entry, x, y [3,26]"""
    return (x[0][:, None] * y[0][None] + x[1][:, None] * y[1][None]) + x[2][:, None] * y[2][None]


def chain(centres32, jac32, T, accel_weight=1.0, acc_max=INF, triple_weight=None, into=None, into_E=None):
    """(A, g, E, F, cost, count) numpy fp64 in the header's order, operation for operation.  Frame b belongs to the triples
    centred at b - 1 (P), b (M) and b + 1 (N); the sums run over the spheres with rows, ascending, from 0, three separate
    chains: A = (w_P P + (4 w_M) M) + w_N N, g = (w_P GP - (2 w_M) GM) + w_N GN, E = (0 - (2 w_M) XM) - (2 w_N) XN, F = w_N FN.
    into = (A, g, cost): the term is added (accumulate = 1), frames without a weighted triple untouched; into_E: E likewise
    (accumulate_E = 1)."""
    d = decide(centres32, T, acc_max, triple_weight)
    q = np.asarray(jac32).astype(np.float64)
    B, J = d["act"].shape
    q = q.reshape(B, J, 3, 26)
    aw = np.float64(np.float32(accel_weight))
    used = aw > 0
    A, g, cost = (np.zeros((B, 26, 26)), np.zeros((B, 26)), np.zeros(B)) if into is None else (np.array(t, np.float64) for t in into)
    E = np.zeros((B, 26, 26)) if into_E is None else np.array(into_E, np.float64)
    F = np.zeros((B, 26, 26))
    count = np.zeros(B, np.int64)
    for b in range(B):
        t = b % T
        bp, bn = b - 1, (b + 1) % B                            # (live is False where these leave the sequence)
        use_p, use_m, use_n = (bool(used and d["live"][i]) for i in (bp, b, bn))
        if t >= 2:
            count[b] = d["act"][bp].sum()
        wp, wm, wn = (aw * d["fw"][i] if use else 0.0 for i, use in ((bp, use_p), (b, use_m), (bn, use_n)))
        z = lambda: np.zeros((26, 26))                         # noqa: E731
        P, M, N, XM, XN, FN = z(), z(), z(), z(), z(), z()
        GP, GM, GN, C = np.zeros(26), np.zeros(26), np.zeros(26), np.float64(0.0)
        for j in range(J):
            own = q[b, j]
            dot = lambda a: (own[0] * a[0] + own[1] * a[1]) + own[2] * a[2]   # noqa: E731
            if use_p and d["act"][bp, j]:
                P = P + _gram(own, own)
                GP = GP + dot(d["a"][bp, j])
            if use_m and d["act"][b, j]:
                M = M + _gram(own, own)
                GM = GM + dot(d["a"][b, j])
                XM = XM + _gram(own, q[b + 1, j])
            if use_n and d["act"][bn, j]:
                N = N + _gram(own, own)
                GN = GN + dot(d["a"][bn, j])
                XN = XN + _gram(own, q[b + 1, j])
                FN = FN + _gram(own, q[b + 2, j])
            if use_p:
                C = C + d["term"][bp, j]
        if use_n:
            F[b] = wn * FN
        if use_m or use_n:
            mine_E = (0.0 - (2.0 * wm) * XM) - (2.0 * wn) * XN
            E[b] = mine_E if into_E is None else E[b] + mine_E
        if into is not None and not (use_p or use_m or use_n):
            continue
        mine_A, mine_g = (wp * P + (4.0 * wm) * M) + wn * N, (wp * GP - (2.0 * wm) * GM) + wn * GN
        if into is None:
            A[b], g[b], cost[b] = mine_A, mine_g, wp * C
        else:
            A[b], g[b] = A[b] + mine_A, g[b] + mine_g
            if use_p:
                cost[b] = cost[b] + wp * C
    return A, g, E, F, cost, count


# ---- the solve ----------------------------------------------------------------------------------------------------------
def _cholesky(M, lam, Wt, Vt):
    """lm_band.h's lm_band_cholesky: column by column, the diagonal damped first, W_{t-1}'s outer product subtracted entry by
    entry (m ascending), then V_{t-2}'s, then the columns' own.  (L, ok)."""
    n = M.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        v = M[k:, k].copy()
        v[0] = v[0] + lam * v[0]
        for X in (Wt, Vt):
            if X is not None:
                for m in range(n):
                    v = v - X[m, k:] * X[m, k]
        for m in range(k):
            v = v - L[k:, m] * L[k, m]
        d = v[0]
        if not (d > 0 and d < np.inf):
            return L, False
        root = np.sqrt(d)
        L[k:, k] = v / root
        L[k, k] = root
    return L, True


def _rows(L, Xt):
    """Xt[k, i] = X[i, k]: column i := the solution z of L z = that column, all columns side by side"""
    n = L.shape[0]
    Xt = Xt.copy()
    for k in range(n):
        v = Xt[k].copy()
        for m in range(k):
            v = v - L[k, m] * Xt[m]
        Xt[k] = v / L[k, k]
    return Xt


def block_solve(A, g, E, F, lam, mu, p, prior, T):
    """delta [T,26] (None where a pivot is not positive and finite) of ONE sequence: the header's block Cholesky with
    bandwidth two, forward over t, then block forward and back substitution, every sum in index order, the W term before
    the V term.  A, E, F [T,26,26] (F None: no second band), g, p, prior [T,26] fp64."""
    A, g, E, p, prior, mu = (np.asarray(t, np.float64) for t in (A, g, E, p, prior, mu))
    band2 = F is not None
    F = np.asarray(F, np.float64) if band2 else None
    n = 26
    Ls, Wts, Vts, ys = [], [], [None] * T, []
    for t in range(T):
        M = A[t].copy()
        M[np.arange(n), np.arange(n)] += mu
        Wp = Wts[t - 1] if t > 0 else None                     # W_{t-1}
        V1 = Vts[t - 1] if band2 and t > 0 else None           # V_{t-1}
        V2 = Vts[t - 2] if band2 and t > 1 else None           # V_{t-2}
        with np.errstate(all="ignore"):
            L, ok = _cholesky(M, lam, Wp, V2)
        if not ok:
            return None
        rhs = -(g[t] + mu * (p[t] - prior[t]))
        for X, y in ((Wp, ys[t - 1] if t > 0 else None), (V2, ys[t - 2] if t > 1 else None)):
            if X is not None:
                c = np.zeros(n)
                for k in range(n):
                    c = c + X[k] * y[k]
                rhs = rhs - c
        y, acc = np.zeros(n), np.zeros(n)
        for k in range(n):
            y[k] = (rhs[k] - acc[k]) / L[k, k]
            acc[k + 1:] = acc[k + 1:] + L[k + 1:, k] * y[k]
        Ls.append(L)
        ys.append(y)
        if t < T - 1:
            R = E[t].copy()                                    # R[k, i] = (E_t^T - V_{t-1} W_{t-1}^T)[i, k]
            if band2 and t > 0:
                for k in range(n):
                    c = np.zeros(n)
                    for m in range(n):
                        c = c + V1[m] * Wp[m, k]
                    R[k] = E[t][k] - c
            Wts.append(_rows(L, R))
        if band2 and t < T - 2:
            Vts[t] = _rows(L, F[t])
    x = np.zeros((T, n))
    for t in range(T - 1, -1, -1):
        z = ys[t].copy()
        if t < T - 1:
            c = np.zeros(n)
            for i in range(n):
                c = c + Wts[t][:, i] * x[t + 1, i]
            z = z - c
        if band2 and t < T - 2:
            c = np.zeros(n)
            for i in range(n):
                c = c + Vts[t][:, i] * x[t + 2, i]
            z = z - c
        acc = np.zeros(n)
        L = Ls[t]
        for k in range(n - 1, -1, -1):
            x[t, k] = (z[k] - acc[k]) / L[k, k]
            acc[:k] = acc[:k] + L[k, :k] * x[t, k]
    return x


def dense_system(A, g, E, F, lam, mu, p, prior, T):
    """(H [26T,26T], rhs [26T]): sphere_sequence_ref.dense_system's with the blocks (t, t + 2) = F_t and (t + 2, t) = F_t^T"""
    H, rhs = qref.dense_system(A, g, E, lam, mu, p, prior, T)
    if F is not None:
        F = np.asarray(F, np.float64)
        for t in range(T - 2):
            H[26 * t:26 * t + 26, 26 * t + 52:26 * t + 78] = F[t]
            H[26 * t + 52:26 * t + 78, 26 * t:26 * t + 26] = F[t].T
    return H, rhs


def dense_solve(A, g, E, F, lam, mu, p, prior, T):
    H, rhs = dense_system(A, g, E, F, lam, mu, p, prior, T)
    return np.linalg.solve(H, rhs).reshape(T, 26)


class Seq2LM(qref.SeqLM):
    """shr_pose_lm_seq2_begin / shr_pose_lm_seq2_step: sphere_sequence_ref.SeqLM's bookkeeping with the accepted F kept beside
    E.  Without F the step IS SeqLM's; with F the step is block_solve per sequence, the kernel's recurrences word for word."""

    def __init__(self, params0, T, lambda0=1e-3, dtype=torch.float64):
        super().__init__(params0, T, lambda0, dtype)
        self.F = torch.zeros_like(self.E)

    def step(self, A, g, E, F, cost_data, trial, prior=None, stiffness=None, solve=True):
        if F is None:
            return super().step(A, g, E, cost_data, trial, prior, stiffness, solve)
        super().step(A, g, E, cost_data, trial, prior, stiffness, solve=False)
        T, S = self.T, self.S
        af = self.history[-1].repeat_interleave(T)
        self.F = torch.where(af[:, None, None], F.double(), self.F)
        if not solve:
            return None
        pr = (self.p0 if prior is None else prior.double()).numpy()
        mu = np.zeros(26) if stiffness is None else torch.as_tensor(stiffness).double().numpy()
        delta = np.zeros((S * T, 26))
        ok = np.ones(S, bool)
        for s in range(S):
            sl = slice(s * T, s * T + T)
            x = block_solve(self.A[sl].numpy(), self.g[sl].numpy(), self.E[sl].numpy(), self.F[sl].numpy(), float(self.lam[s]), mu,
                            self.p[sl].numpy(), pr[sl], T)
            ok[s] = x is not None
            if x is not None:
                delta[sl] = x
        self.ok = torch.as_tensor(ok)
        self.trial = (self.p + torch.as_tensor(delta)).float().double()   # the trial is fp32 by contract, whatever the chain
        return self.trial


def combined(model, view, observed, p, p2m, T, tab=None, collision_weight=0.0, temporal_weight=0.0, ts_max=INF, frame_weight=None,
             accel_weight=0.0, acc_max=INF, triple_weight=None, rows="autograd", **prior):
    """(A, g, E, F, cost, accel) at poses p: sphere_sequence_ref.combined plus the acceleration term; F and `accel` (normal()'s
    dict) are None where the loop issues no launch of the entry.  rows = "chain": both temporal terms from the header's
    chains on the model's own Jacobian instead of autograd's blocks (the CPU tests hold the two equal to 1e-13; the study
    uses it, autograd's 26 T columns per row being most of its run time)."""
    accel = T > 2 and accel_weight > 0
    if rows == "autograd":
        A, g, E, cost, _ = qref.combined(model, view, observed, p, p2m, T, tab, collision_weight, temporal_weight, ts_max,
                                         frame_weight, **prior)
        if not accel:
            return A, g, E, None, cost, None
        n = normal(model, p, T, accel_weight, acc_max, triple_weight)
        return A + n["A"], g + n["g"], E + n["E"], n["F"], cost + n["cost"], n
    A, g, cost, _ = cref.combined(model, view, observed, p, p2m, tab, collision_weight, **prior)
    E, F, n = torch.zeros_like(A), None, None
    if (T > 1 and temporal_weight > 0) or accel:
        pm = p.to(model.dtype)
        jac = model.chain.jacobian(pm)[1].detach().numpy()
        c32 = model.centres(pm).detach().float().numpy()
    if T > 1 and temporal_weight > 0:
        a, b, e, c, _ = qref.chain(c32, jac, T, temporal_weight, ts_max, frame_weight)
        A, g, E, cost = A + torch.as_tensor(a), g + torch.as_tensor(b), torch.as_tensor(e), cost + torch.as_tensor(c)
    if accel:
        a, b, e, f, c, _ = chain(c32, jac, T, accel_weight, acc_max, triple_weight)
        A, g, E, cost = A + torch.as_tensor(a), g + torch.as_tensor(b), E + torch.as_tensor(e), cost + torch.as_tensor(c)
        F, n = torch.as_tensor(f), dict(decided=decide(c32, T, acc_max, triple_weight))
    return A, g, E, F, cost, n


def solve(model, view, observed, params0, p2m, T, tab=None, collision_weight=0.0, temporal_weight=0.0, ts_max=INF,
          frame_weight=None, accel_weight=0.0, acc_max=INF, triple_weight=None, iters=10, lambda0=1e-3, stiffness=None,
          prior=None, rows="autograd", **terms):
    """The loop of ops.sphere_icp_trajectory in model.dtype -> (params [B,26], cost0 [S], cost [S], lm); lm.rowed: per
    evaluation the [B,J] bool of the spheres with acceleration rows (None without the term)."""
    start = params0.float().double() if model.dtype == torch.float32 else params0.double()
    lm = Seq2LM(start, T, lambda0, model.dtype)
    lm.rowed = []
    trial = lm.trial
    for it in range(iters + 1):
        A, g, E, F, cost, n = combined(model, view, observed, trial, p2m, T, tab, collision_weight, temporal_weight, ts_max,
                                       frame_weight, accel_weight, acc_max, triple_weight, rows, **terms)
        lm.rowed.append(None if n is None else torch.as_tensor(n["decided"]["act"]))
        out = lm.step(A, g, E, F, cost, trial, prior, stiffness, solve=it < iters)
        trial = out if out is not None else trial
    return lm.p, lm.cost0, lm.cost, lm


# ---- the study ----------------------------------------------------------------------------------------------------------
TURN_FRAME = 4            # the frame of T = 8 at which the `turn` family's truth changes direction


def study_sequences(family, S=3, T=8):
    """(p*, p0, hidden [S T] bool).  `noise`, `blind`: sphere_sequence_ref.study_sequences'.  `turn`: the truth of sequence s
    interpolates through THREE poses of pose_icp_ref.poses(3 S, 41), pose 3 s at frame 0, 3 s + 1 at frame TURN_FRAME and
    3 s + 2 at frame T - 1, linearly in the 26 parameters on either side: a truth that does accelerate, at the kink.  The
    starts are sequence_poses' noise on it."""
    if family != "turn":
        return qref.study_sequences(family, S, T)
    p, _ = ref.poses(3 * S, 41)
    star = torch.zeros(S, T, 26, dtype=torch.float64)
    for t in range(T):
        if t <= TURN_FRAME:
            lam = t / TURN_FRAME
            star[:, t] = p[0::3] * (1 - lam) + p[1::3] * lam
        else:
            lam = (t - TURN_FRAME) / (T - 1 - TURN_FRAME)
            star[:, t] = p[1::3] * (1 - lam) + p[2::3] * lam
    star = star.reshape(S * T, 26)
    gen = torch.Generator().manual_seed(41 + 1000)
    p0 = star + ref.SIGMA_ANGLE * torch.randn(S * T, 26, generator=gen, dtype=torch.float64)
    p0[:, 3:6] = star[:, 3:6] + ref.SIGMA_MM * torch.randn(S * T, 3, generator=gen, dtype=torch.float64)
    return star, p0, torch.zeros(S * T, dtype=torch.bool)


def accel_of(model, p, T):
    """mean over the triples and j of |c_j(k - 1) - 2 c_j(k) + c_j(k + 1)| of poses p, mm (fp64)"""
    c = model.to(torch.float64).centres(p.double())
    B, J = c.shape[:2]
    c = c.view(B // T, T, J, 3)
    return (c[:, :-2] + c[:, 2:] - 2 * c[:, 1:-1]).norm(dim=-1).mean()


def study(mesh, W=48, H=40, S=3, T=8, iters=10, sigma=5.0, accel_weights=(0.01, 0.1, 1.0, 10.0), temporal_weights=(0.0, 0.1),
          caps=(INF, 20.0), families=("noise", "blind", "turn"), out=print):
    """The table of DESIGN.md 4.4u: 4.4t's set-up unchanged (S sequences of T frames, one view, 4.4s's defaults for the other
    terms, keypoints with sigma mm of noise drawn per frame, the `noise` and `blind` families) plus the `turn` family, over
    accel_weight x temporal_weight x acc_max: the mean keypoint error, the frame-to-frame jitter and, for `blind`, the
    hidden finger's error in its frames.  `frames` is the frame-by-frame fit (T = 1) and `seq` SphereSequencePoseFitter at
    its defaults, 4.4t's baselines."""
    model = sref.Spheres(mesh, None, True)
    p2m = ref.grid(W, H)
    mu = torch.as_tensor(ref.STIFFNESS)
    lo, hi = pref.limits()
    tab = cref.table(mesh)
    B = S * T
    view = vref.views(B, ("identity",))
    rows_out = []
    grid = [("traj", tw, qref.DEFAULT_TS_MAX, aw, cap, T) for cap in caps for tw in temporal_weights for aw in accel_weights]
    for family in families:
        p, p0, hidden = study_sequences(family, S, T)
        obs = rref.render64(model, view, p, W, H, p2m)
        k = pref.targets(model, view, p, sigma, seed=3)
        finger = None
        if family == "blind":
            c0 = model.centres(p).detach()
            q = p.clone()
            q[:, rref.FINGER + 1:rref.FINGER + 4] += 0.5
            finger = np.nonzero((model.centres(q).detach() - c0).norm(dim=-1).max(0).values.numpy() > 1e-9)[0]
            k[np.ix_(np.nonzero(hidden.numpy())[0], [0], finger)] = np.nan
        terms = dict(keypoints=k, confidence=None, kp_weight=pref.DEFAULT_KP_WEIGHT, kp_max=pref.DEFAULT_KP_MAX, lower=lo,
                     upper=hi, limit_weight=pref.DEFAULT_LIMIT_WEIGHT)
        start, jit0 = sref.keypoint_error(model, p0, p), qref.jitter(model, p0, p, T)
        out("%s: start keypoint error %.2f mm, jitter %.2f mm; the truth moves %.2f mm per frame and sphere and accelerates by "
            "%.2f mm" % (family, start.mean(), jit0.mean(), qref.jitter(model, p, p[:1].expand_as(p), T).mean(),
                         accel_of(model, p, T)))
        base = (("frames", 0.0, INF, 0.0, INF, 1), ("seq", qref.DEFAULT_TEMPORAL_WEIGHT, qref.DEFAULT_TS_MAX, 0.0, INF, T))
        for name, tw, ts, aw, cap, TT in base + tuple(grid):
            q, c0, c, _ = solve(model, view, obs, p0, p2m, TT, tab, cref.DEFAULT_COLLISION_WEIGHT, tw, ts, None, aw, cap, None,
                                iters, 1e-3, mu, None, "chain", **terms)
            err, jit = sref.keypoint_error(model, q, p), qref.jitter(model, q, p, T)
            ratio = c0 / c.clamp(min=1e-300)
            row = dict(family=family, name=name, temporal_weight=tw, accel_weight=aw, acc_max=cap, start=start.mean().item(),
                       mean=err.mean().item(), median=err.median().item(), jitter0=jit0.mean().item(), jitter=jit.mean().item(),
                       ratio_median=ratio.median().item(), ratio_worst=ratio.min().item())
            if family == "blind":
                fe = (model.centres(q) - model.centres(p)).detach().norm(dim=-1)[:, finger].mean(1)
                row["hidden"] = fe[hidden].mean().item()
            rows_out.append(row)
            out("  %-6s accel %-5g temporal %-4g acc_max %-4g: error %.2f -> %.2f (%.2f) mm, jitter %.2f -> %.2f mm, cost0/cost "
                "%.3g (worst %.3g)%s" % (name, aw, tw, cap, row["start"], row["mean"], row["median"], row["jitter0"],
                                         row["jitter"], row["ratio_median"], row["ratio_worst"],
                                         "" if "hidden" not in row else "; the hidden finger in its frames %.2f mm" % row["hidden"]))
    return rows_out


if __name__ == "__main__":
    import sys
    from spherehand_amd import hand_model
    kw = {}
    if len(sys.argv) > 1:
        kw["families"] = (sys.argv[1],)
    study(hand_model.load_mesh(), **kw)
