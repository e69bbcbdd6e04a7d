"""A restatement of the two entries of the sliding-window tracker (spherehand_amd/csrc/lm_window.hip; include/spherehand_hip.h,
the section of shr_pose_window_marginalize), on top of lm_scripts_ref and sphere_trajectory_ref, none of which it changes
(test helper; not a conftest):

    marginalize      the header's steps word for word on ONE sequence: sphere_trajectory_ref's _cholesky at lambda = 0 and its
                     _rows, then the five products, each a chain from 0 subtracted once
    dense_marginalize   the Schur complement by numpy.linalg.solve on the dense 78 x 78 (52 x 52) departing matrix: the
                     independent check
    prior_normal     the carried prior's normal equations, word for word; prior_dense by matmul
    reference        both marginalisations of a whole batch, their distance per sequence, the status
    compare          the ONE comparator of the CPU and the GPU tests (records); compare_prior the same for the prior's term
    chain            the equivalence: marginalise-and-slide on a quadratic energy against the full-batch solve
    cases            the inputs of the GPU tests

Equations are torch fp64 on the CPU or numpy, A [B,26,26], g [B,26], E, F [B,26,26] or None, cost [B], B = S T; trial, prior
[B,26] and mu [26] fp32-representable."""
import numpy as np
import torch

import lm_scripts_ref as lref
import sphere_trajectory_ref as tref

N26, N52 = 26, 52
MARGIN = lref.MARGIN
NAN = float("nan")


def _np(t, dtype=np.float64):
    if t is None:
        return None
    t = np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    return t if dtype is None else t.astype(dtype)


def _gram(X, Y):
    """out[a][b] = sum_k X[k][a] Y[k][b]: a chain from 0, k ascending, all 26 terms"""
    c = np.zeros((X.shape[1], Y.shape[1]))
    for k in range(X.shape[0]):
        c = c + X[k][:, None] * Y[k][None, :]
    return c


def _mirror(z):
    """the lower triangle, mirrored"""
    return np.tril(z) + np.tril(z, -1).T


VARIANTS = ("E untransposed", "F dropped", "eta uncorrected", "offset without y.y", "stiffness on frame 1", "NaN on failure")


def marginalize(A, g, E, F, cost, trial, prior=None, mu=None, variant=None):
    """(Lambda [52,52], eta [52], offset, point [52] fp32, status) of ONE sequence: A [T,26,26], g [T,26], E, F [T,26,26] or
    None, cost [T] fp64, trial [T,26], prior [T,26] or None, mu [26] or None.  variant: one of the wrong versions (VARIANTS)
    the comparator has to tell from the right one."""
    T = A.shape[0]
    band1 = E is not None and T >= 2
    two = band1 and T >= 3
    band2 = two and F is not None
    trial = _np(trial, np.float32)
    point = np.zeros(N52, np.float32)
    for t in (1, 2):
        if t < T:
            point[N26 * (t - 1):N26 * t] = trial[t]
    Lambda, eta = np.zeros((N52, N52)), np.zeros(N52)
    muv = np.zeros(N26) if mu is None else _np(mu, np.float32).astype(np.float64)
    d = np.zeros(N26) if prior is None else trial[0].astype(np.float64) - _np(prior, np.float32)[0].astype(np.float64)
    M = A[0].copy()
    if mu is not None:
        M[np.arange(N26), np.arange(N26)] += muv
    with np.errstate(all="ignore"):
        L, ok = tref._cholesky(M, 0.0, None, None)
    if not ok:
        if variant == "NaN on failure":
            return Lambda + NAN, eta + NAN, NAN, point, 1
        return Lambda, eta, 0.0, point, 1
    b0 = g[0] + muv * d
    sq = muv * (d * d)
    y = tref._rows(L, b0[:, None])[:, 0]
    c = cost[0]
    for i in range(N26):
        c = c + sq[i]
    if T >= 2:
        c = c + cost[1]
    if T >= 3:
        c = c + cost[2]
    yy = 0.0
    for k in range(N26):
        yy = yy + y[k] * y[k]
    offset = c if variant == "offset without y.y" else c - yy
    if band1:
        XE = tref._rows(L, E[0].T.copy() if variant == "E untransposed" else E[0])
        XF = tref._rows(L, F[0]) if band2 and variant != "F dropped" else None
        l11 = A[1] - _gram(XE, XE)
        if variant == "stiffness on frame 1":
            l11[np.arange(N26), np.arange(N26)] += muv
        Lambda[:N26, :N26] = _mirror(l11)
        eta[:N26] = g[1] if variant == "eta uncorrected" else g[1] - _gram(XE, y[:, None])[:, 0]
        if two:
            l12, l22, e2 = E[1], A[2], g[2]
            if XF is not None:
                l12, l22 = E[1] - _gram(XE, XF), A[2] - _gram(XF, XF)
                if variant != "eta uncorrected":
                    e2 = g[2] - _gram(XF, y[:, None])[:, 0]
            Lambda[:N26, N26:], Lambda[N26:, :N26] = l12, l12.T
            Lambda[N26:, N26:] = _mirror(l22)
            eta[N26:] = e2
    return Lambda, eta, offset, point, 0


def dense_marginalize(A, g, E, F, cost, trial, prior=None, mu=None):
    """(Lambda, eta, offset) of ONE sequence by numpy.linalg.solve on the dense departing matrix of its first min(T, 3)
    frames; the contract's special cases (T == 1, E None: +0) as stated."""
    T = A.shape[0]
    n = min(T, 3)
    band1 = E is not None and T >= 2
    muv = np.zeros(N26) if mu is None else _np(mu, np.float32).astype(np.float64)
    d = np.zeros(N26) if prior is None else (_np(trial, np.float32)[0].astype(np.float64) - _np(prior, np.float32)[0].astype(np.float64))
    H, b = np.zeros((N26 * n, N26 * n)), np.zeros(N26 * n)
    for t in range(n):
        sl = slice(N26 * t, N26 * t + N26)
        H[sl, sl], b[sl] = _mirror(A[t]), g[t]
        if band1 and t + 1 < n:
            H[sl, N26 * t + N26:N26 * t + N52] = E[t]
            H[N26 * t + N26:N26 * t + N52, sl] = E[t].T
    if band1 and F is not None and n == 3:
        H[:N26, N52:], H[N52:, :N26] = F[0], F[0].T
    H[np.arange(N26), np.arange(N26)] += muv
    b[:N26] += muv * d
    total = float(np.sum(cost[:n])) + float(np.sum(muv * d * d))
    M0, b0 = H[:N26, :N26], b[:N26]
    offset = total - b0 @ np.linalg.solve(M0, b0)
    Lambda, eta = np.zeros((N52, N52)), np.zeros(N52)
    if band1:
        C = H[N26:, :N26]                                      # the coupling of frames 1, 2 to frame 0
        m = N26 * (n - 1)
        Lambda[:m, :m] = H[N26:, N26:] - C @ np.linalg.solve(M0, C.T)
        eta[:m] = b[N26:] - C @ np.linalg.solve(M0, b0)
    return Lambda, eta, offset


def _seq(X, s, T):
    return None if X is None else X[s * T:s * T + T]


def reference(A, g, E, F, cost, trial, T, prior=None, mu=None, variant=None):
    """dict over a batch of S = B / T sequences: Lambda [S,52,52], eta [S,52], offset [S], point [S,52] fp32, status [S] by the
    restatement; dense_Lambda, dense_eta, dense_offset by numpy.linalg.solve (a failed sequence's: the restatement's +0);
    gap [S,3]: the largest |restatement - dense| of the sequence's Lambda, eta and offset, 0 where it fails; size [S,3] the
    largest |dense| entry of each."""
    A, g, E, F, cost = (_np(X) for X in (A, g, E, F, cost))
    trial, prior = _np(trial, np.float32), _np(prior, np.float32)
    S = A.shape[0] // T
    out = dict(Lambda=np.zeros((S, N52, N52)), eta=np.zeros((S, N52)), offset=np.zeros(S), point=np.zeros((S, N52), np.float32),
               status=np.zeros(S, np.int32), gap=np.zeros((S, 3)), size=np.zeros((S, 3)), T=T)
    out.update(dense_Lambda=np.zeros((S, N52, N52)), dense_eta=np.zeros((S, N52)), dense_offset=np.zeros(S))
    for s in range(S):
        eq = tuple(_seq(X, s, T) for X in (A, g, E, F, cost, trial, prior))
        L, e, c, p, st = marginalize(*eq, mu, variant)
        out["Lambda"][s], out["eta"][s], out["offset"][s], out["point"][s], out["status"][s] = L, e, c, p, st
        if st:
            continue
        dl, de, dc = dense_marginalize(*eq, mu)
        out["dense_Lambda"][s], out["dense_eta"][s], out["dense_offset"][s] = dl, de, dc
        out["gap"][s] = [np.abs(L - dl).max(), np.abs(e - de).max(), abs(c - dc)]
        out["size"][s] = [np.abs(dl).max(), np.abs(de).max(), abs(dc)]
    return out


def compare(got, want, out=None):
    """The differences between a run (Lambda [S,52,52], eta [S,52], offset [S], point [S,52], status [S]) and reference()'s
    dict, as a list of strings (empty: none).  Per sequence, every sequence:
        status, point    equal (point: the bits of the fp32 trial poses)
        a failed one     every Lambda, eta and offset entry an exact +0 (not -0, not a NaN)
        Lambda, eta, offset   the largest |got - restatement| of the sequence <= MARGIN x the largest |restatement - dense| of
                         that quantity (gap): both are fp64 in one stated order, so bits are expected and the reference's own
                         distance is all that is allowed; Lambda bit-symmetric
    out: a dict that receives `exact` (sequences that match the restatement bit for bit), `live` (the sequences that
    factorise) and `ratio`, the largest error / bar seen where the bar is not 0."""
    Lam, eta, off, point, status = (_np(t, None) for t in got)
    out = {} if out is None else out
    out.update(exact=0, live=0, ratio=out.get("ratio", 0.0))
    bad = []
    for s in range(want["status"].shape[0]):
        if int(status[s]) != int(want["status"][s]):
            bad.append("sequence %d: status %d, %d is due" % (s, status[s], want["status"][s]))
            continue
        if not np.array_equal(np.asarray(point[s], np.float32).view(np.int32), want["point"][s].view(np.int32)):
            bad.append("sequence %d: point is not the trial poses of frames 1 and 2" % s)
        triples = (("Lambda", Lam[s], want["Lambda"][s], want["gap"][s, 0]), ("eta", eta[s], want["eta"][s], want["gap"][s, 1]),
                   ("offset", np.asarray(off[s]), np.asarray(want["offset"][s]), want["gap"][s, 2]))
        if want["status"][s]:
            for name, v, _, _ in triples:
                v = np.asarray(v, np.float64)
                if not (np.array_equal(v, np.zeros_like(v)) and not np.signbit(v).any()):
                    bad.append("sequence %d fails: %s is not +0 throughout" % (s, name))
            continue
        out["live"] += 1
        same = True
        for name, v, w, gap in triples:
            with np.errstate(invalid="ignore"):
                err = np.abs(v - w)
            err = float(np.where(np.isnan(err), np.inf, err).max())
            same = same and np.array_equal(v, w)
            if err > MARGIN * gap:
                bad.append("sequence %d: %s off by %.3g (bar %.3g = %g x %.3g)" % (s, name, err, MARGIN * gap, MARGIN, gap))
            if gap > 0:
                out["ratio"] = max(out["ratio"], err / (MARGIN * gap))
        if not np.array_equal(Lam[s], Lam[s].T):
            bad.append("sequence %d: Lambda is not bit-symmetric" % s)
        out["exact"] += int(same)
    return bad


# ---- the carried prior's term -------------------------------------------------------------------------------------------
def prior_normal(trial, Lambda, eta, offset, point, T, A, g, E, cost, accumulate, accumulate_E, active=None, variant=None):
    """(A, g, E, cost) after shr_pose_window_prior_normal on copies of the given buffers (whatever they hold: what the entry
    does not touch stays), word for word.  E may be None with T == 1.  variant "point not subtracted": d = trial."""
    trial, point = _np(trial, np.float32), _np(point, np.float32)
    Lambda, eta, offset = _np(Lambda), _np(eta), _np(offset)
    A, g, cost = _np(A).copy(), _np(g).copy(), _np(cost).copy()
    E = None if E is None else _np(E).copy()
    S = trial.shape[0] // T
    n = N26 if T == 1 else N52
    for q in range(S):
        if active is not None and int(_np(active, None)[q]) == 0:
            continue
        first = q * T
        d = trial[first:first + n // N26].reshape(-1).astype(np.float64)
        if variant != "point not subtracted":
            d = d - point[q, :n].astype(np.float64)
        ld = np.zeros(n)
        for j in range(n):
            ld = ld + Lambda[q, :n, j] * d[j]
        for t in range(n // N26):
            o, b = N26 * t, first + t
            blk = np.tril(Lambda[q, o:o + N26, o:o + N26])
            low = np.tril(A[b]) + blk if accumulate else blk
            A[b] = low + np.tril(low, -1).T
            mine = ld[o:o + N26] + eta[q, o:o + N26]
            g[b] = g[b] + mine if accumulate else mine
        if T >= 2:
            mine = Lambda[q, :N26, N26:]
            E[first] = E[first] + mine if accumulate_E else mine
        quad = lin = 0.0
        for i in range(n):
            quad = quad + d[i] * ld[i]
        for i in range(n):
            lin = lin + eta[q, i] * d[i]
        c = (quad + 2.0 * lin) + offset[q]
        cost[first] = cost[first] + c if accumulate else c
        if T >= 2 and not accumulate:
            cost[first + 1] = 0.0
    return A, g, E, cost


def prior_dense(trial, Lambda, eta, offset, point, T):
    """(A, g, E, cost) of the term alone by matmul, +0 where it has nothing: the independent check of prior_normal"""
    trial, point = _np(trial, np.float32).astype(np.float64), _np(point, np.float32).astype(np.float64)
    Lambda, eta, offset = _np(Lambda), _np(eta), _np(offset)
    B = trial.shape[0]
    S, n = B // T, (N26 if T == 1 else N52)
    A, g, E, cost = np.zeros((B, N26, N26)), np.zeros((B, N26)), np.zeros((B, N26, N26)), np.zeros(B)
    for q in range(S):
        d = trial[q * T:q * T + n // N26].reshape(-1) - point[q, :n]
        L = Lambda[q, :n, :n]
        grad = L @ d + eta[q, :n]
        cost[q * T] = d @ L @ d + 2.0 * eta[q, :n] @ d + offset[q]
        for t in range(n // N26):
            A[q * T + t], g[q * T + t] = L[N26 * t:N26 * t + N26, N26 * t:N26 * t + N26], grad[N26 * t:N26 * t + N26]
        if T >= 2:
            E[q * T] = L[:N26, N26:]
    return A, g, E, cost


def compare_prior(got, want, dense, T, out=None):
    """The differences between a run's (A, g, E, cost) and prior_normal's on the same buffers, as a list of strings.  `dense`
    is prior_dense's term alone and the restated term alone (prior_normal with accumulate = 0 on zeros): per sequence the
    bar is MARGIN x their largest distance, per quantity; bits are expected.  A stays bit-symmetric on the frames written."""
    names = ("A", "g", "E", "cost")
    term, alone = dense
    out = {} if out is None else out
    out.update(exact=out.get("exact", 0), ratio=out.get("ratio", 0.0))
    bad = []
    B = want[0].shape[0]
    for q in range(B // T):
        sl = slice(q * T, q * T + T)
        same = True
        for name, v, w, td, ta in zip(names, got, want, term, alone):
            if w is None:
                continue
            v = _np(v)
            gap = float(np.abs(td[sl] - ta[sl]).max())
            with np.errstate(invalid="ignore"):
                err = np.abs(v[sl] - w[sl])
            err = float(np.where(np.isnan(err), np.inf, err).max())
            same = same and np.array_equal(v[sl], w[sl])
            if err > MARGIN * gap:
                bad.append("sequence %d: %s off by %.3g (bar %.3g = %g x %.3g)" % (q, name, err, MARGIN * gap, MARGIN, gap))
            if gap > 0:
                out["ratio"] = max(out["ratio"], err / (MARGIN * gap))
        a = _np(got[0])[q * T:q * T + min(T, 2)]
        if not np.array_equal(a, a.transpose(0, 2, 1)):
            bad.append("sequence %d: A is not bit-symmetric" % q)
        out["exact"] += int(same)
    return bad


# ---- the equivalence -------------------------------------------------------------------------------------------------------
def restated_entries():
    """(marginalize, prior) as chain() calls them, by the restatement; the GPU test passes the two entries instead.
    marginalize(A, g, E, F, cost, trial, T) -> (Lambda, eta, offset, point, status), batch arrays, numpy;
    prior(trial, Lambda, eta, offset, point, T, A, g, E, cost) -> (A, g, E, cost), accumulate = accumulate_E = 1."""
    def marg(A, g, E, F, cost, trial, T):
        r = reference(A, g, E, F, cost, trial, T)
        return r["Lambda"], r["eta"], r["offset"], r["point"], r["status"]

    def prior(trial, Lambda, eta, offset, point, T, A, g, E, cost):
        return prior_normal(trial, Lambda, eta, offset, point, T, A, g, E, cost, 1, 1)
    return marg, prior


def _dense_of(A, g, E, F, T):
    """(H [26T,26T], g [26T]) of ONE sequence, undamped"""
    z = np.zeros((T, N26))
    H = tref.dense_system(A, z, E, F, 0.0, np.zeros(N26), z, z, T)[0]
    return H, g.reshape(-1)


def chain(entries, U=2, T=8, leave=5, seed=21, step=0.05):
    """Marginalise-and-slide on a QUADRATIC energy against its full-batch solve: lm_scripts_ref.banded_system(U, T, band = 2)
    is, per sequence, f(x) = x^T H x + 2 g^T x + c over the 26 T unknowns.  Frames 0 ... leave - 1 are marginalised one after
    the other, each time from the first three frames of what is left: the blocks of those frames that the marginalisation
    consumes (A_0, E_0, F_0, g_0 and A_1, E_1, A_2, g_1, g_2) are taken out of the remaining energy and live on in the prior
    alone.  Every departing system is evaluated at a trial pose of its own, fp32 and DIFFERENT from the point of the prior it
    carries (a random walk of `step` per frame), so the prior enters through `entries`' prior term with d != 0, and the
    energy that is left through its exact gradient there.  The last T - leave frames' system with the last prior is solved
    densely in numpy.
    -> dict: x [U,T-leave,26] the minimiser of the remaining frames (absolute poses), Z [U,26n,26n] the inverse of the final
    matrix, energy [U] its minimum; x_dense, Z_dense, energy_dense the same from the dense 26 T system (numpy.linalg.solve);
    bar_x, bar_Z, bar_energy [U]: MARGIN x the distance of two dense routes over all 26 T unknowns, numpy.linalg.solve against
    numpy.linalg.inv.  The solve route is linearised at the origin; the inv route, like every window, at the trial poses p the
    chain ends with: x = p - inv(H) (g + H p), the minimum c(p) - g(p)^T inv(H) g(p) -- a step from a pose 0.3 away carries the
    rounding of that step, which the origin's route does not have.  For Z, inv(H) and solve(H, I) are one LAPACK call and
    differ in no bit, so the inv route is the inverse of the dense Schur complement of the frames that left."""
    marg, prior = entries
    A, g, E, F, cost = (_np(X) for X in lref.banded_system(U, T, band=2, seed=seed))
    rng = np.random.RandomState(seed)
    n = T - leave
    out = dict(x=np.zeros((U, n, N26)), Z=np.zeros((U, N26 * n, N26 * n)), energy=np.zeros(U))
    out.update(x_dense=np.zeros((U, n, N26)), Z_dense=np.zeros((U, N26 * n, N26 * n)), energy_dense=np.zeros(U),
               bar_x=np.zeros(U), bar_Z=np.zeros(U), bar_energy=np.zeros(U), status=[])
    # the remaining energy, linearised at the origin: per sequence blocks rA, rg, rE, rF over the frames left and a constant
    rA, rg, rE, rF = A.reshape(U, T, N26, N26).copy(), g.reshape(U, T, N26).copy(), E.reshape(U, T, N26, N26).copy(), \
        F.reshape(U, T, N26, N26).copy()
    rc = cost.reshape(U, T).sum(1)
    record, pose = None, (0.3 * rng.randn(U, T, N26)).astype(np.float32)

    def evaluate(k, m):
        """the first m frames of what is left from frame k on, at the trial poses: (A, g, E, F, cost) [U m, ...] of the blocks
        among those frames alone, the constant with the first frame"""
        dA, dE, dF = rA[:, k:k + m].copy(), rE[:, k:k + m].copy(), rF[:, k:k + m].copy()
        dE[:, m - 1:] = 0.0
        dF[:, max(m - 2, 0):] = 0.0
        dg, dc = np.zeros((U, m, N26)), np.zeros((U, m))
        for u in range(U):
            H, g0 = _dense_of(dA[u], rg[u, k:k + m], dE[u], dF[u], m)
            p = pose[u, k:k + m].astype(np.float64).reshape(-1)
            dg[u] = (g0 + H @ p).reshape(m, N26)
            dc[u, 0] = rc[u] + 2.0 * g0 @ p + p @ H @ p
        return tuple(X.reshape((U * m,) + X.shape[2:]) for X in (dA, dg, dE, dF, dc))

    for k in range(leave):
        m = min(3, T - k)
        pose[:, k:] = (pose[:, k:].astype(np.float64) + step * rng.randn(U, T - k, N26)).astype(np.float32)
        dA, dg, dE, dF, dc = evaluate(k, m)
        trial = pose[:, k:k + m].reshape(U * m, N26)
        if record is not None:
            dA, dg, dE, dc = prior(trial, *record, m, dA, dg, dE, dc)
        record = marg(dA, dg, dE, dF, dc, trial, m)
        out["status"].append(np.asarray(record[4]).copy())
        record = record[:4]
        # what the marginalisation consumed leaves the remaining energy
        rA[:, k:k + m], rg[:, k:k + m] = 0.0, 0.0
        rE[:, k:k + m - 1], rF[:, k] = 0.0, 0.0
        rc[:] = 0.0
    pose[:, leave:] = (pose[:, leave:].astype(np.float64) + step * rng.randn(U, n, N26)).astype(np.float32)
    fA, fg, fE, fF, fc = evaluate(leave, n)
    trial = pose[:, leave:].reshape(U * n, N26)
    fA, fg, fE, fc = prior(trial, *record, n, fA, fg, fE, fc)
    fA, fg, fE, fc = (_np(X) for X in (fA, fg, fE, fc))
    for u in range(U):
        sl = slice(u * n, u * n + n)
        H, gg = _dense_of(fA[sl], fg[sl], fE[sl], fF[sl], n)
        delta = np.linalg.solve(H, -gg)
        out["x"][u] = trial[sl].astype(np.float64) + delta.reshape(n, N26)
        out["Z"][u] = np.linalg.solve(H, np.eye(N26 * n))
        out["energy"][u] = fc[sl].sum() + gg @ delta
    for u in range(U):                                         # the dense side, two routes
        H, gg = _dense_of(A[u * T:u * T + T], g[u * T:u * T + T], E[u * T:u * T + T], F[u * T:u * T + T], T)
        c = float(cost[u * T:u * T + T].sum())
        sl, hd = slice(N26 * leave, N26 * T), slice(0, N26 * leave)
        xs, Zs = np.linalg.solve(H, -gg), np.linalg.solve(H, np.eye(N26 * T))
        p = pose[u].astype(np.float64).reshape(-1)
        Zi = np.linalg.inv(H)
        gp = gg + H @ p
        xi = p - Zi @ gp
        ei = (c + 2.0 * gg @ p + p @ H @ p) - gp @ Zi @ gp
        Zc = np.linalg.inv(H[sl, sl] - H[sl, hd] @ np.linalg.solve(H[hd, hd], H[hd, sl]))
        out["x_dense"][u], out["Z_dense"][u], out["energy_dense"][u] = xs[sl].reshape(n, N26), Zs[sl, sl], c + gg @ xs
        out["bar_x"][u] = MARGIN * np.abs(xs[sl] - xi[sl]).max()
        out["bar_Z"][u] = MARGIN * np.abs(Zs[sl, sl] - Zc).max()
        out["bar_energy"][u] = MARGIN * abs((c + gg @ xs) - ei)
    return out


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------
SWEEP_T = (1, 2, 3, 5)
SWEEP = tuple((band, own, mu, w) for band in (1, 2) for own in (40, 6) for mu in (0.0, 1e-3, 0.5) for w in (1.0, 1e4))


def stiffness(mu):
    """[26] fp32-representable, or None for 0"""
    return None if not mu else torch.full((26,), float(mu)).float()


def poses(B, seed, prior=True):
    """(trial [B,26], prior [B,26] or None) fp32: lm_scripts_ref's draw"""
    gen = torch.Generator().manual_seed(seed)
    p = (0.3 * torch.randn(B, 26, generator=gen, dtype=torch.float64)).float()
    pr = (p.double() + 0.05 * torch.randn(B, 26, generator=gen, dtype=torch.float64)).float() if prior else None
    return p, pr


def random_stiffness(seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.5 * torch.rand(26, generator=gen, dtype=torch.float64)).float()


def system(S, T, band, own=40, weight=1.0, seed=7):
    """(A, g, E, F or None, cost) of S sequences; band 2 draws lm_scripts_ref.system's 12 rows per pair and triple"""
    A, g, E, F, cost = lref.banded_system(S, T, own=own, weight=weight, seed=seed, band=band, pair=12 if band == 2 else 30)
    return A, g, E, (F if band == 2 else None), cost


def shape_cases():
    """[(name, T, (A, g, E, F, cost), trial, prior, mu)]: S in {1, 3, 65} x T in {1, 2, 3, 5} x band 1 and 2, a prior and a
    stiffness in turn; then F = None on a band-2 system and E = None (F given), at T = 3 and 5."""
    out, n = [], 0
    for S in (1, 3, 65):
        for T in SWEEP_T:
            for band in (1, 2):
                trial, prior = poses(S * T, 900 + n, prior=n % 3 != 0)
                mu = None if n % 2 else random_stiffness(40 + n)
                out.append(("S=%d T=%d band=%d" % (S, T, band), T, system(S, T, band, seed=900 + n), trial, prior, mu))
                n += 1
    for T in (3, 5):
        A, g, E, F, cost = system(3, T, 2, seed=950 + T)
        trial, prior = poses(3 * T, 950 + T)
        out.append(("F=None T=%d" % T, T, (A, g, E, None, cost), trial, prior, random_stiffness(7)))
        out.append(("E=None T=%d" % T, T, (A, g, None, F, cost), trial, prior, random_stiffness(8)))
    return out


def record_of(S, seed, T=3):
    """a prior record (Lambda, eta, offset, point) of S sequences, numpy: the restated marginalisation of a band-2 system"""
    A, g, E, F, cost = system(S, 3, 2, seed=seed)
    trial, _ = poses(3 * S, seed)
    r = reference(A, g, E, F, cost, trial, 3)
    assert not r["status"].any()
    return r["Lambda"], r["eta"], r["offset"], r["point"]


def prior_cases():
    """[(name, T, record, trial, (A, g, E, cost), accumulate, accumulate_E, active)]: S in {1, 3, 65} x T in {1, 2, 3, 5},
    the flags in every combination over the cases, `active` None or with a 0 in the middle (S = 3: sequence 1)"""
    out, n = [], 0
    for S in (1, 3, 65):
        for T in SWEEP_T:
            for acc, acc_E in ((0, 0), (1, 1), (1, 0), (0, 1)):
                if (n + T) % 2 and (acc, acc_E) in ((1, 0), (0, 1)) and S != 3:
                    n += 1
                    continue                                   # (the mixed flags on every T at S = 3, on every other T elsewhere)
                A, g, E, _, cost = system(S, T, 1, seed=970 + n)
                trial, _ = poses(S * T, 970 + n, prior=False)
                active = None
                if S >= 3 and n % 2 == 0:
                    active = torch.ones(S, dtype=torch.int32)
                    active[S // 2] = 0
                out.append(("S=%d T=%d accumulate=%d accumulate_E=%d%s" % (S, T, acc, acc_E, "" if active is None else " active"),
                            T, record_of(S, 980 + n), trial, (A, g, E, cost), acc, acc_E, active))
                n += 1
    return out


PIVOT_T = 3


def pivot_case(band):
    """(broken eqs, good eqs, trial, prior, mu): three sequences of T = 3 whose MIDDLE one's M_0 fails in column 25 alone
    (lm_scripts_ref.break_column on frame 0 at lambda = 0), beside the batch without the failure"""
    kind = "seq2" if band == 2 else "seq"
    A, g, E, F, cost = system(3, PIVOT_T, band, seed=401)
    mu = random_stiffness(5)
    eqs = (A, g, E, F) if band == 2 else (A, g, E)
    broken = lref.break_column(kind, eqs, 1, PIVOT_T, 0, 0.0, mu.double().numpy())
    trial, prior = poses(3 * PIVOT_T, 402)
    return (broken[0], g, E, F, cost), (A, g, E, F, cost), trial, prior, mu


# ---- the study -------------------------------------------------------------------------------------------------------------
def study(mesh, W=48, H=40, S=3, N=12, win=4, iters=10, sigma=5.0, families=("noise", "blind"), out=print):
    """The table of DESIGN.md 4.4z: 4.4t/u's set-up and `noise` and `blind` families (S streams, one view, keypoints with
    `sigma` mm of noise; `blind` drops the index finger's keypoints in frames BLIND_FRAMES and starts it extended there)
    extended to N frames, fitted in fp64 by sphere_trajectory_ref's loop with SphereTrajectoryPoseFitter's defaults:
        tracker   windows of `win` frames that slide by one frame and carry the marginalised past (the restated entries)
        window    the same sliding windows WITHOUT the prior
        frames    the frame-by-frame fit
        batch     the full-batch trajectory fit over all N frames
    Every new frame starts from the family's noisy start pose.  Per row: the keypoint error and the jitter of the SMOOTHED
    poses (a frame's pose when it left its window, the last window's at the end; for `frames` and `batch` their result) and
    of the FILTERED poses (its pose after the first fit it was part of), for `blind` the hidden finger's error in its frames,
    and the mean sigma of the NEWEST frame of every window after the first (lm_covariance_ref's restated marginals of the
    window's accepted equations, with the prior's blocks and with them taken out again)."""
    import lm_covariance_ref as vcov
    import pose_icp_ref as ref
    import pose_icp_views_ref as vref
    import sphere_collision_ref as cref
    import sphere_icp_ref as sref
    import sphere_prior_ref as pref
    import sphere_render_icp_ref as rref
    import sphere_sequence_ref as qref
    model = sref.Spheres(mesh, None, True)
    p2m = ref.grid(W, H)
    mu = torch.as_tensor(ref.STIFFNESS)
    lo, hi = pref.limits()
    tab = cref.table(mesh)
    B = S * N
    view = vref.views(B, ("identity",))
    tw, ts, aw, cap = tref.DEFAULT_TEMPORAL_WEIGHT, qref.DEFAULT_TS_MAX, tref.DEFAULT_ACCEL_WEIGHT, tref.DEFAULT_ACC_MAX
    cw = cref.DEFAULT_COLLISION_WEIGHT
    rows_out = []

    def frames_of(k, m):
        return [s * N + k + j for s in range(S) for j in range(m)]

    for family in families:
        p, p0, hidden = tref.study_sequences(family, S, N)
        obs = rref.render64(model, view, p, W, H, p2m)
        kp = pref.targets(model, view, p, sigma, seed=3)
        finger = None
        if family == "blind":
            c0 = model.centres(p).detach()
            q = p.clone()
            q[:, rref.FINGER + 1:rref.FINGER + 4] += 0.5
            finger = np.nonzero((model.centres(q).detach() - c0).norm(dim=-1).max(0).values.numpy() > 1e-9)[0]
            kp[np.ix_(np.nonzero(hidden.numpy())[0], [0], finger)] = np.nan

        def terms(idx):
            return dict(keypoints=kp[idx], confidence=None, kp_weight=pref.DEFAULT_KP_WEIGHT, kp_max=pref.DEFAULT_KP_MAX, lower=lo,
                        upper=hi, limit_weight=pref.DEFAULT_LIMIT_WEIGHT)

        def fit(idx, start, T, record):
            """sphere_trajectory_ref.solve's loop on the frames idx, the carried prior's restated term added to every evaluation"""
            lm = tref.Seq2LM(start.double(), T, 1e-3, model.dtype)
            trial = lm.trial
            t_w, a_w = (tw, aw) if T > 1 else (0.0, 0.0)
            for it in range(iters + 1):
                A, g, E, F, cost, _ = tref.combined(model, view[idx], obs[idx], trial, p2m, T, tab, cw, t_w, ts, None, a_w, cap, None,
                                                    "chain", **terms(idx))
                if record is not None:
                    A, g, E, cost = (torch.as_tensor(X) for X in prior_normal(trial.float(), *record, T, A, g, E, cost, 1, 1))
                step = lm.step(A, g, E, F, cost, trial, None, mu, solve=it < iters)
                trial = step if step is not None else trial
            return lm

        def departing(k, lm, start, record):
            """the restated marginalisation of frame k at the window's fitted poses: every term that involves it, from the
            restated entries alone"""
            n = min(win, 3)
            first = frames_of(k, 1)
            q = lm.p.view(S, win, 26)
            A0, g0, c0, _ = cref.combined(model, view[first], obs[first], q[:, 0], p2m, tab, cw, **terms(first))
            qs = q[:, :n].reshape(S * n, 26)
            A, g, cost = np.zeros((S * n, 26, 26)), np.zeros((S * n, 26)), np.zeros(S * n)
            A[0::n], g[0::n], cost[0::n] = A0.numpy(), g0.numpy(), c0.numpy()
            pm = qs.to(model.dtype)
            jac = model.chain.jacobian(pm)[1].detach().numpy()
            c32 = model.centres(pm).detach().float().numpy()
            at = lambda t: np.tile((np.arange(n) == t).astype(np.float32), S)   # noqa: E731
            E, F = np.zeros((S * n, 26, 26)), None
            if n > 1 and tw > 0:
                A, g, E, cost, _ = qref.chain(c32, jac, n, tw, ts, at(0), (A, g, cost))
            if n > 2 and aw > 0:
                A, g, E, F, cost, _ = tref.chain(c32, jac, n, aw, cap, at(1), (A, g, cost), E)
            if record is not None:
                A, g, E, cost = prior_normal(qs.float(), *record, n, A, g, E, cost, 1, 1)
            r = reference(A, g, E, F, cost, qs.float(), n, start.view(S, win, 26)[:, :n].reshape(S * n, 26).float(), mu.float())
            return (r["Lambda"], r["eta"], r["offset"], r["point"]), r["status"]

        def newest_sigma(lm, record):
            """the newest frame's mean sigma from the window's accepted equations, and with the prior's blocks taken out"""
            A, E, F = lm.A.clone(), lm.E.clone(), lm.F.clone()
            jac = model.chain.jacobian(lm.p.to(model.dtype))[1].detach().float().numpy()
            with_prior = vcov.sigma_of(vcov.reference(A, E, F, win, mu.float())["cov"], jac).reshape(S, win, -1)[:, -1].mean()
            L = torch.as_tensor(record[0])
            A[0::win] -= L[:, :26, :26]
            A[1::win] -= L[:, 26:, 26:]
            E[0::win] -= L[:, :26, 26:]
            without = vcov.sigma_of(vcov.reference(A, E, F, win, mu.float())["cov"], jac).reshape(S, win, -1)[:, -1].mean()
            return float(with_prior), float(without)

        def slide(carry):
            smoothed, filtered = torch.zeros(S, N, 26, dtype=torch.float64), torch.zeros(S, N, 26, dtype=torch.float64)
            start = p0.view(S, N, 26)[:, :win].reshape(S * win, 26).float().double()
            lm = fit(frames_of(0, win), start, win, None)
            filtered[:, :win] = lm.p.view(S, win, 26)
            failed, sig = 0, []
            record = None
            for k in range(N - win):
                if carry:
                    record, status = departing(k, lm, start, record)
                    failed += int(status.sum())
                q = lm.p.view(S, win, 26)
                smoothed[:, k] = q[:, 0]
                start = torch.cat((q[:, 1:], p0.view(S, N, 26)[:, k + win:k + win + 1].float().double()), 1).reshape(S * win, 26)
                lm = fit(frames_of(k + 1, win), start, win, record)
                filtered[:, k + win] = lm.p.view(S, win, 26)[:, -1]
                if carry:
                    sig.append(newest_sigma(lm, record))
            smoothed[:, N - win:] = lm.p.view(S, win, 26)
            return smoothed.reshape(B, 26), filtered.reshape(B, 26), failed, (np.mean(sig, 0) if sig else None)

        results = {}
        results["tracker"] = slide(True)
        results["window"] = slide(False)
        everything = list(range(B))
        q = fit(everything, p0.float().double(), 1, None).p
        results["frames"] = (q, q, 0, None)
        q = fit(everything, p0.float().double(), N, None).p
        results["batch"] = (q, q, 0, None)
        for name, (sm, fl, failed, sig) in results.items():
            row = dict(family=family, name=name, failed=failed)
            for label, q in (("smoothed", sm), ("filtered", fl)):
                row[label] = float(sref.keypoint_error(model, q, p).mean())
                row[label + "_jitter"] = float(qref.jitter(model, q, p, N).mean())
                if finger is not None:
                    fe = (model.centres(q) - model.centres(p)).detach().norm(dim=-1)[:, finger].mean(1)
                    row[label + "_hidden"] = float(fe[hidden].mean())
            if sig is not None:
                row["sigma_with"], row["sigma_without"] = float(sig[0]), float(sig[1])
            rows_out.append(row)
            text = "  %-6s %-8s: smoothed error %.2f mm, jitter %.2f mm; filtered error %.2f mm, jitter %.2f mm" % (
                family, name, row["smoothed"], row["smoothed_jitter"], row["filtered"], row["filtered_jitter"])
            if finger is not None:
                text += "; the hidden finger in its frames %.2f mm smoothed, %.2f mm filtered" % (row["smoothed_hidden"], row["filtered_hidden"])
            if sig is not None:
                text += "; the newest frame's mean sigma %.3f mm with the prior, %.3f mm without; %d failed pivots" % (
                    row["sigma_with"], row["sigma_without"], failed)
            out(text)
    return rows_out


if __name__ == "__main__":
    from spherehand_amd import hand_model
    study(hand_model.load_mesh())
