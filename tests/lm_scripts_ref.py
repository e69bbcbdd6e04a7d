"""Scripts for the three structured Levenberg-Marquardt steps (shr_pose_lm_seq_step, shr_pose_lm_seq2_step and
shr_pose_lm_shared_step; include/spherehand_hip.h), on top of sphere_sequence_ref, sphere_trajectory_ref and sphere_radii_ref,
none of which it changes (test helper; not a conftest).  `kind` is "seq", "seq2" or "shared"; a UNIT is a sequence of n = T
frames or a group of n = N frames, and U = B / n.

    banded_system    A, g, E, F, cost of U sequences from a stacked Jacobian: positive semi-definite by construction
    arrow_system     A, g, C, R, gs, cost of U groups from a stacked Jacobian over (pose_b | sigma)
    first_bad_pivot  replays the restated _cholesky recurrences of one unit: the first (t, k) whose pivot is not positive
    break_coupling / break_column   make a unit's pivot fail at a chosen frame, through the coupling or in one column
    block_scripts    hand-made multi-step inputs in pose_icp_ref.lm_scripts()'s format
    Restated         the stepper of the restatement (SeqLM, Seq2LM, SharedLM or a subclass); drive() runs any stepper
    reference        the restatement on the very trials a run took, with the word-for-word block solve, the dense solve and
                     their distance per step and unit
    compare          the ONE comparator of the CPU and the GPU tests
    pivot_cases, conditioning_cases, long_chain    the inputs of the GPU tests, stated and checked on the CPU

Equations ("eqs") are (A, g, E) | (A, g, E, F) | (A, g, C, R, gs), torch fp64 on the CPU; a step is eqs + (cost_data, solve).
A script is (lambda0, start, prior, stiffness, steps): start, prior and stiffness are tensors for the sequences and pairs
(pose part, shape part) for the groups; prior and stiffness may be None."""
import numpy as np
import torch

import sphere_radii_ref as sref
import sphere_sequence_ref as qref
import sphere_trajectory_ref as tref

KINDS = ("seq", "seq2", "shared")
INF, NAN = float("inf"), float("nan")
EPS32 = 2.0 ** -23
MARGIN = 4.0               # what the project gives a reference's own distance (sa_case, C_BAR)
_MOD = dict(seq=qref, seq2=tref, shared=sref)
_LM = dict(seq=qref.SeqLM, seq2=tref.Seq2LM, shared=sref.SharedLM)
f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)          # noqa: E731
f32 = lambda t: t.float().double()                             # noqa: E731  (what an fp32 argument of the ABI can hold)


def _rnd(seed):
    gen = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64), gen


# ---- systems ------------------------------------------------------------------------------------------------------------
def banded_system(U, T, own=40, weight=1.0, seed=7, band=1, pair=30, small=0.05, residual=0.1):
    """(A [B,26,26], g [B,26], E, F [B,26,26], cost [B]) fp64.  Per sequence a stacked Jacobian over its 26 T unknowns: `own`
    rows per frame that touch frame t only; `pair` rows per (t, t + 1), (-J, J + small N); with band = 2 `pair` rows per
    (t, t + 1, t + 2), (J, -2 J, J); the coupling rows scaled by sqrt(weight).  H = J^T J cut into A_t, E_t (zero at the
    last frame) and F_t (zero at the last two); g = J^T r with r ~ N(0, residual); cost = |r|^2 / T per frame."""
    rnd, _ = _rnd(seed)
    B, sw = U * T, float(np.sqrt(weight))
    A, E, F, g, cost = f64(B, 26, 26), f64(B, 26, 26), f64(B, 26, 26), f64(B, 26), f64(B)
    for u in range(U):
        rows = []

        def add(t, parts):
            r = f64(parts[0].shape[0], 26 * T)
            for i, P in enumerate(parts):
                r[:, 26 * (t + i):26 * (t + i + 1)] = P
            rows.append(r)

        for t in range(T):
            if own:
                add(t, [rnd(own, 26)])
            if t < T - 1:
                J = rnd(pair, 26)
                add(t, [-sw * J, sw * (J + small * rnd(pair, 26))])
            if band == 2 and t < T - 2:
                J = rnd(pair, 26)
                add(t, [sw * J, -2.0 * sw * J, sw * J])
        Jd = torch.cat(rows) if rows else f64(0, 26 * T)
        r = residual * rnd(Jd.shape[0])
        H = Jd.t() @ Jd
        H, G = 0.5 * (H + H.t()), Jd.t() @ r
        for t in range(T):
            sl = slice(26 * t, 26 * t + 26)
            A[u * T + t], g[u * T + t], cost[u * T + t] = H[sl, sl], G[sl], (r * r).sum() / T
            if t < T - 1:
                E[u * T + t] = H[sl, 26 * t + 26:26 * t + 52]
            if t < T - 2:
                F[u * T + t] = H[sl, 26 * t + 52:26 * t + 78]
    return A, g, E, F, cost


def arrow_system(U, N, K, own=40, weight=1.0, seed=7, pair=30, residual=0.1):
    """(A [B,26,26], g [B,26], C [B,26,K], R [U,K,K], gs [U,K], cost [B]) fp64.  Per frame `own` rows over its pose only and
    `pair` rows over (pose_b | sigma), the latter scaled by sqrt(weight): A_b, C_b and the frame's share of R and gs are the
    blocks of J^T J and J^T r.  With own = 0 and 30 N < 26 N + K the group's system is singular but for the damping."""
    rnd, _ = _rnd(seed)
    B, sw = U * N, float(np.sqrt(weight))
    Jo, Jp, Js = rnd(B, own, 26), sw * rnd(B, pair, 26), sw * rnd(B, pair, K)
    ro, rp = residual * rnd(B, own), residual * rnd(B, pair)
    A = Jo.transpose(1, 2) @ Jo + Jp.transpose(1, 2) @ Jp
    A = 0.5 * (A + A.transpose(1, 2))
    C = Jp.transpose(1, 2) @ Js
    R = (Js.transpose(1, 2) @ Js).view(U, N, K, K).sum(1)
    R = 0.5 * (R + R.transpose(1, 2))
    g = (Jo * ro[:, :, None]).sum(1) + (Jp * rp[:, :, None]).sum(1)
    gs = (Js * rp[:, :, None]).sum(1).view(U, N, K).sum(1)
    return A, g, C, R, gs, (ro * ro).sum(1) + (rp * rp).sum(1)


def system(kind, U, n, K=None, **kw):
    """eqs + (cost,) of `kind`.  seq2 draws 12 rows per pair and per triple instead of 30: fewer rows than unknowns without
    own rows, as 30 per pair alone are for seq."""
    if kind == "shared":
        return arrow_system(U, n, K, **kw)
    if kind == "seq2":
        kw.setdefault("pair", 12)
    A, g, E, F, cost = banded_system(U, n, band=2 if kind == "seq2" else 1, **kw)
    return (A, g, E, cost) if kind == "seq" else (A, g, E, F, cost)


def _per_frame(kind):
    """which of the eqs are per frame (the others are per unit)"""
    return dict(seq=(1, 1, 1), seq2=(1, 1, 1, 1), shared=(1, 1, 1, 0, 0))[kind]


def unit_of(kind, eqs, u, n):
    """the eqs of unit u alone, numpy"""
    return tuple((e[u * n:u * n + n] if f else e[u]).numpy() for e, f in zip(eqs, _per_frame(kind)))


def with_unit(kind, eqs, u, n, other, v=None):
    """a copy of eqs with unit u replaced by unit v (default u) of `other`"""
    v = u if v is None else v
    out = tuple(e.clone() for e in eqs)
    for o, e, f in zip(out, other, _per_frame(kind)):
        if f:
            o[u * n:u * n + n] = e[v * n:v * n + n]
        else:
            o[u] = e[v]
    return out


# ---- pivots -------------------------------------------------------------------------------------------------------------
def _traced(mod, call):
    """call() with mod._cholesky's results recorded, in call order"""
    seen, orig = [], mod._cholesky

    def spy(*a):
        out = orig(*a)
        seen.append(out)
        return out

    mod._cholesky = spy
    try:
        result = call()
    finally:
        mod._cholesky = orig
    return result, seen


def _solve_unit(kind, eq, lam, mu, nu, p, prior, sigma=None, sprior=None):
    """the word-for-word solve of one unit -> flat delta (26 n [+ K]) or None"""
    n = eq[0].shape[0]
    if kind == "seq":
        x = qref.block_solve(eq[0], eq[1], eq[2], lam, mu, p, prior, n)
    elif kind == "seq2":
        x = tref.block_solve(eq[0], eq[1], eq[2], eq[3], lam, mu, p, prior, n)
    else:
        x = sref.schur_solve(eq[0], eq[1], eq[2], eq[3], eq[4], lam, mu, nu, p, prior, sigma, sprior)
        x = None if x is None else np.concatenate([x[0].reshape(-1), x[1]])
    return None if x is None else np.asarray(x).reshape(-1)


def _dense_unit(kind, eq, lam, mu, nu, p, prior, sigma=None, sprior=None):
    n = eq[0].shape[0]
    if kind == "seq":
        return qref.dense_solve(eq[0], eq[1], eq[2], lam, mu, p, prior, n).reshape(-1)
    if kind == "seq2":
        return tref.dense_solve(eq[0], eq[1], eq[2], eq[3], lam, mu, p, prior, n).reshape(-1)
    x = sref.dense_solve(eq[0], eq[1], eq[2], eq[3], eq[4], lam, mu, nu, p, prior, sigma, sprior)
    return np.concatenate([x[0].reshape(-1), x[1]])


def _factors(kind, eq, lam, mu, nu=None):
    """the (L, ok) of every _cholesky call of one unit's solve: frame t is call t; the groups' Schur block is call N"""
    n = eq[0].shape[0]
    mu = np.zeros(26) if mu is None else np.asarray(mu, np.float64)
    z = np.zeros((n, 26))
    if kind == "shared":
        K = eq[2].shape[2]
        nu = np.zeros(K) if nu is None else np.asarray(nu, np.float64)
        return _traced(sref, lambda: _solve_unit(kind, eq, lam, mu, nu, z, z, np.zeros(K), np.zeros(K)))[1]
    return _traced(_MOD[kind], lambda: _solve_unit(kind, eq, lam, mu, None, z, z))[1]


def first_bad_pivot(kind, eq, lam, mu=None, nu=None):
    """(t, k) of the first pivot that is not positive and finite when the restated recurrences run on one unit's equations
    (unit_of's), None where all are.  t is the frame; for a group t = N is the Schur block."""
    for t, (L, ok) in enumerate(_factors(kind, eq, lam, mu, nu)):
        if not ok:
            return t, int(np.argmax(np.diagonal(L) == 0))
    return None


def break_coupling(kind, eqs, u, n, t, factor=1.5, second=False):
    """a copy of eqs in which unit u's coupling INTO frame t is scaled: E_{t-1} (F_{t-2} with `second`), so that D_t goes
    indefinite and no earlier frame changes; for a group every C_b, so that the Schur block does."""
    out = tuple(e.clone() for e in eqs)
    if kind == "shared":
        out[2][u * n:u * n + n] *= factor
    elif second:
        out[3][u * n + t - 2] *= factor
    else:
        out[2][u * n + t - 1] *= factor
    return out


def break_column(kind, eqs, u, n, t, lam, mu=None, nu=None):
    """a copy of eqs in which unit u's frame t fails in column 25 ONLY: A_t[25,25], which no other pivot reads, lowered by
    1.5 x the last pivot of D_t, which becomes -0.5 x itself."""
    L, ok = _factors(kind, unit_of(kind, eqs, u, n), lam, mu, nu)[t]
    assert ok
    out = tuple(e.clone() for e in eqs)
    out[0][u * n + t, 25, 25] -= 1.5 * L[25, 25] ** 2 / (1.0 + lam)
    return out


# ---- scripts ------------------------------------------------------------------------------------------------------------
# totals per unit and step, of the roles of script 0: all accepted | accepted, rejected twice, accepted again | a cost that
# is not finite in a MIDDLE frame | a pivot that fails on steps 0 to 2 (through the coupling, then in column 25 of the last
# frame), next to good units
ROLES = ((1000.0, 900.0, 800.0, 700.0, 600.0, 500.0, 400.0),
         (1000.0, 1100.0, 1200.0, 900.0, 1300.0, 800.0, 700.0),
         (NAN, 500.0, INF, 400.0, 300.0, 350.0, 200.0),
         (500.0, 400.0, 450.0, 300.0, 250.0, 200.0, 150.0))
SOLVES = (True, True, True, False, True, True, False)          # a step without a solve in the middle and at the end
LOW = ((1000.0, 900.0, 800.0, 700.0, 600.0, 500.0), (1000.0, 1100.0, 1200.0, 1300.0, 900.0, 800.0))
HIGH = ((1000.0, 1100.0, 1200.0, 900.0, 1300.0, 800.0), (1000.0, 900.0, 800.0, 700.0, 600.0, 500.0))


def _frame_costs(totals, n, step):
    """[U n]: a unit's total spread over its frames with weights 1 +- 0.5 that swap every step, so that a frame's own cost
    goes up where its unit's goes down; a total that is not finite sits in the MIDDLE frame alone."""
    out = []
    for tot in totals:
        w = np.array([1.0 + 0.5 * (-1) ** (t + step) for t in range(n)])
        c = (1000.0 if not np.isfinite(tot) else tot) * w / w.sum()
        if not np.isfinite(tot):
            c[n // 2] = tot
        out.append(c)
    return torch.as_tensor(np.concatenate(out))


def _start(kind, U, n, K, seed, prior, stiff):
    rnd, gen = _rnd(seed)
    p0 = f32(0.3 * rnd(U * n, 26))
    pr = f32(p0 + 0.05 * rnd(U * n, 26)) if prior else None
    mu = f32(0.5 * torch.rand(26, generator=gen, dtype=torch.float64)) if stiff else None
    if kind != "shared":
        return p0, pr, mu
    s0 = f32(10.0 + rnd(U, K))
    spr = f32(s0 + 0.5 * rnd(U, K)) if prior else None
    nu = f32(1e-2 * torch.rand(K, generator=gen, dtype=torch.float64)) if stiff else None
    return (p0, s0), (None if pr is None else (pr, spr)), (None if mu is None else (mu, nu))


def _script(kind, n, K, totals, solves, lam0, own, prior, stiff, seed, bad=None):
    U = len(totals)
    start, pr, st = _start(kind, U, n, K, seed, prior, stiff)
    mu, nu = (st if kind == "shared" else (st, None)) if st is not None else (None, None)
    steps = []
    for i, solve in enumerate(solves):
        *eqs, _ = system(kind, U, n, K, own=own, seed=seed + 1 + i)
        eqs = tuple(eqs)
        if bad is not None and i < 3:
            if i == 1:
                eqs = break_column(kind, eqs, bad, n, n - 1, lam0, mu, nu)
            else:
                eqs = break_coupling(kind, eqs, bad, n, max(1, n // 2), 2.0 if kind == "shared" else 1.5)   # (K = 1 needs the 2)
        steps.append(eqs + (_frame_costs([t[i] for t in totals], n, i), solve))
    return lam0, start, pr, st, steps


def block_scripts(kind, n, K=41, U=4):
    """The scripts of `kind` with n frames per unit (K shared parameters), U units per batch of script 0:
      script 0.., lambda0 1e-3, a prior different from the start and a stiffness, 7 steps, the fourth and the last without a
        solve: ROLES in batches of U units (cyclically filled), every step with equations of its own, so that a re-solve
        after a reject has to come from the KEPT ones
      then lambda0 2e-9, two units, no prior, no stiffness, own = 6: accepted steps run into the lower clamp next to a unit
        that is rejected three times
      then lambda0 5e5, two units, a stiffness alone: rejected steps run into the upper clamp next to a unit that descends
    The cost gaps (100 and more) are far above the stiffness terms (below 1) and rounding, so the decisions are exact."""
    scripts = []
    for first in range(0, len(ROLES), U):
        roles = [(first + i) % len(ROLES) for i in range(U)]
        scripts.append(_script(kind, n, K, [ROLES[r] for r in roles], SOLVES, 1e-3, 40, True, True, 100 + first,
                               bad=roles.index(3) if 3 in roles else None))
    scripts.append(_script(kind, n, K, LOW, (True,) * 6, 2e-9, 6, False, False, 200))
    scripts.append(_script(kind, n, K, HIGH, (True,) * 6, 5e5, 40, False, True, 300))
    return scripts


# (n, K, U) of the scripts the tests run.  T = 2 of seq2: every frame is one of the last two, F is all zero.
SCRIPT_SHAPES = dict(seq=((2, None, 4), (3, None, 4), (8, None, 4)), seq2=((3, None, 4), (4, None, 4), (6, None, 4), (2, None, 4)),
                     shared=((3, 41, 2), (1, 64, 3), (5, 1, 2)))


# ---- steppers -----------------------------------------------------------------------------------------------------------
def split(kind, x):
    """(pose part, shape part) of a script's start, prior or stiffness"""
    if x is None:
        return None, None
    return x if kind == "shared" else (x, None)


class Restated:
    """the restatement (or a subclass of it) behind the steppers' interface: step(eqs, cost, trial, shape, solve) -> dict of
    trial_out, shape_out (None without a solve), params, shape, cost, cost0"""

    def __init__(self, kind, script, n, cls=None):
        lam0, start, prior, stiff, _ = script
        self.kind, self.n = kind, n
        (p0, s0), (self.prior, self.sprior), (self.mu, self.nu) = split(kind, start), split(kind, prior), split(kind, stiff)
        cls = _LM[kind] if cls is None else cls
        self.lm = cls(p0, s0, n, lam0) if kind == "shared" else cls(p0, n, lam0)

    def step(self, eqs, cost, trial, shape, solve):
        lm = self.lm
        if self.kind == "shared":
            t, s = lm.step(*eqs, cost, trial, shape, self.prior, self.mu, self.sprior, self.nu, solve)
        else:
            t, s = lm.step(*eqs, cost, trial, self.prior, self.mu, solve), None
        return dict(trial_out=None if t is None else t.clone(), shape_out=None if s is None else s.clone(), params=lm.p.clone(),
                    shape=lm.s.clone() if self.kind == "shared" else None, cost=lm.cost.clone(), cost0=lm.cost0.clone())


def drive(stepper, kind, script):
    """the stepper on a script: the trial of a step is what the last step WITH a solve wrote (the start first)"""
    trial, shape = split(kind, script[1])
    out = []
    for *eqs, cost, solve in script[4]:
        rec = stepper.step(tuple(eqs), cost, trial, shape, solve)
        out.append(rec)
        if solve:
            trial, shape = rec["trial_out"], rec["shape_out"]
    return out


def kept(kind, lm):
    """the eqs a restatement holds: those of the last accepted trial"""
    if kind == "shared":
        return lm.A, lm.g, lm.C, lm.R, lm.gs
    return (lm.A, lm.g, lm.E) if kind == "seq" else (lm.A, lm.g, lm.E, lm.F)


def state_solve(kind, lm, n, prior, mu, sprior=None, nu=None, dense=False):
    """(delta [B,26], dshape [U,K] or None, ok [U]) from the KEPT state of a restatement, per unit by the word-for-word
    block solve (zero where a pivot fails) or, `dense`, by numpy.linalg.solve of the assembled system"""
    B = lm.p.shape[0]
    U = B // n
    K = lm.K if kind == "shared" else 0
    prior = lm.p0 if prior is None else prior
    mu = np.zeros(26) if mu is None else mu.numpy()
    nu = np.zeros(K) if nu is None else nu.numpy()
    sprior = (lm.s0 if sprior is None else sprior) if kind == "shared" else None
    eqs = kept(kind, lm)
    delta, ds, ok = f64(B, 26), f64(U, K), torch.ones(U, dtype=torch.bool)
    for u in range(U):
        sl = slice(u * n, u * n + n)
        args = (kind, unit_of(kind, eqs, u, n), float(lm.lam[u]), mu, nu, lm.p[sl].numpy(), prior[sl].numpy())
        if kind == "shared":
            args += (lm.s[u].numpy(), sprior[u].numpy())
        x = (_dense_unit if dense else _solve_unit)(*args)
        if x is None:
            ok[u] = False
            continue
        delta[sl], ds[u] = torch.as_tensor(x[:26 * n]).view(n, 26), torch.as_tensor(x[26 * n:])
    return delta, (ds if kind == "shared" else None), ok


def reference(kind, script, n, got, cls=None):
    """The restatement on the trials that the run `got` (drive()'s records) took: per step Restated's record, and with a
    solve also
        ok [U], bad {u: (t, k)}    the units whose step is formed, and where the others' first pivot fails
        gap [U]                    the largest |block - dense| of the unit's step, 0 where its pivot fails
        rel [U]                    gap / the largest |dense|
        trial_block, trial_dense (shape_block, shape_dense)    the fp32 trials of those two solves
    and always lam [U], accept [U].  The GPU's own trial_out goes to the kernel and to the restatement alike, so that one
    rounding cannot grow into a different decision."""
    ref_ = Restated(kind, script, n, cls)
    lm = ref_.lm
    trial, shape = split(kind, script[1])
    out = []
    for i, (*eqs, cost, solve) in enumerate(script[4]):
        rec = ref_.step(tuple(eqs), cost, trial, shape, solve)
        rec.update(lam=lm.lam.clone(), accept=lm.history[-1].clone())
        if solve:
            xb, sb, ok = state_solve(kind, lm, n, ref_.prior, ref_.mu, ref_.sprior, ref_.nu)
            xd, sd, _ = state_solve(kind, lm, n, ref_.prior, ref_.mu, ref_.sprior, ref_.nu, dense=True)
            xd, sd = torch.where(ok.repeat_interleave(n)[:, None], xd, f64(1)), (None if sd is None else torch.where(ok[:, None], sd, f64(1)))
            U = ok.shape[0]
            gap, size = (xb - xd).abs().view(U, -1).amax(1), xd.abs().view(U, -1).amax(1)
            if sd is not None and sd.shape[1]:
                gap, size = torch.maximum(gap, (sb - sd).abs().amax(1)), torch.maximum(size, sd.abs().amax(1))
            bad = {u: first_bad_pivot(kind, unit_of(kind, kept(kind, lm), u, n), float(lm.lam[u]),
                                      None if ref_.mu is None else ref_.mu.numpy(), None if ref_.nu is None else ref_.nu.numpy())
                   for u in range(U) if not ok[u]}
            rec.update(ok=ok, bad=bad, gap=gap, rel=gap / size.clamp(min=1e-300), trial_block=f32(lm.p + xb), trial_dense=f32(lm.p + xd))
            if kind == "shared":
                rec.update(shape_block=f32(lm.s + sb), shape_dense=f32(lm.s + sd))
            assert torch.equal(ok, lm.ok), (ok, lm.ok)
            trial, shape = got[i]["trial_out"], got[i]["shape_out"]
        out.append(rec)
    return out


def bars_of(want):
    """per step the [U] distance of the reference's own two solves (None without a solve): compare()'s `bars`"""
    return [w.get("gap") for w in want]


def compare(got, want, bars, out=None):
    """The differences between a run and the reference on the same trials, as a list of strings (empty: none).  Per step
        params (shape)       equal bits: they are fp32 trials, or kept poses that were
        cost; cost0 after the first step    rtol 2^-23, a NaN or an infinity its own equal
        trial_out (shape_out)    |got - want| <= 2^-23 |want| + 1e-12 + 4 |block - dense| of that unit and step (`bars`);
                             a unit whose pivot fails: the kept pose, bit for bit, on ALL its frames
    out: a dict that receives the largest error / bar seen, and the error and bar there."""
    bad = []
    worst = dict(ratio=0.0, err=0.0, bar=0.0) if out is None else out
    worst.setdefault("ratio", 0.0)
    for i, (g, w, gap) in enumerate(zip(got, want, bars)):
        for name in ("params", "shape"):
            if w[name] is not None and not torch.equal(g[name].double(), w[name]):
                bad.append("step %d: %s differs in %d entries" % (i, name, int((g[name].double() != w[name]).sum())))
        names = ("cost", "cost0") if i == 0 else ("cost",)
        for name in names:
            if not torch.allclose(g[name].double(), w[name], rtol=EPS32, atol=0.0, equal_nan=True):
                bad.append("step %d: %s %s against %s" % (i, name, g[name].tolist(), w[name].tolist()))
        if w["trial_out"] is None:
            continue
        U = w["ok"].shape[0]
        for name in ("trial_out", "shape_out"):
            if w[name] is None:
                continue
            a, b = g[name].double().view(U, -1), w[name].view(U, -1)
            bar = EPS32 * b.abs() + 1e-12 + MARGIN * gap[:, None]
            bar = torch.where(w["ok"][:, None], bar, torch.zeros_like(bar))
            err = (a - b).abs()
            err = torch.where(torch.isnan(err), torch.full_like(err, INF), err)
            if bool((err > bar).any()):
                over = (err - bar).nan_to_num(posinf=INF)
                u = int(over.amax(1).argmax())
                j = int(over[u].argmax())
                bad.append("step %d: %s of unit %d off by %.3g (bar %.3g)%s" % (
                    i, name, u, err[u, j], bar[u, j], "" if w["ok"][u] else ": its pivot fails, the kept pose is due"))
            live = w["ok"][:, None].expand_as(err)
            if bool(live.any()):
                ratio = (err / bar.clamp(min=1e-300))[live]
                j = int(ratio.argmax())
                if float(ratio[j]) >= worst["ratio"]:
                    worst.update(ratio=float(ratio[j]), err=float(err[live][j]), bar=float(bar[live][j]))
    return bad


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------
PIVOT_SHAPE = dict(seq=(4, None), seq2=(4, None), shared=(3, 5))       # n, K; three units, the middle one fails


def pivot_cases(kind):
    """[(name, script, bad_script's good twin, (t, k or None))]: two-step scripts of three units, lambda0 1e-3, a stiffness.
    In step 0 the MIDDLE unit's pivot fails at frame t (t = N: the groups' Schur block) -- through the coupling alone at
    every t from 1, in column 25 alone at t = 1, and in column 25 of the LAST frame -- and in the twin it does not; step 1
    is a good step with equations of its own and half the cost, accepted by all."""
    n, K = PIVOT_SHAPE[kind]
    lam0, U, u = 1e-3, 3, 1
    start, _, st = _start(kind, U, n, K, 400, False, True)
    mu, nu = split(kind, st)
    *good, cost = system(kind, U, n, K, seed=401)
    *after, _ = system(kind, U, n, K, seed=402)
    good, after = tuple(good), tuple(after)
    broken = []
    if kind == "shared":
        broken.append(("the Schur block through C", break_coupling(kind, good, u, n, n), (n, None)))
        broken += [("column 25 of frame %d" % t, break_column(kind, good, u, n, t, lam0, mu, nu), (t, 25)) for t in (1, n - 1)]
    else:
        broken += [("E into frame %d" % t, break_coupling(kind, good, u, n, t), (t, None)) for t in range(1, n)]
        if kind == "seq2":
            broken += [("F into frame %d" % t, break_coupling(kind, good, u, n, t, 2.4, True), (t, None)) for t in range(2, n)]
        broken += [("column 25 of frame %d" % t, break_column(kind, good, u, n, t, lam0, mu, nu), (t, 25)) for t in (1, n - 1)]
    mk = lambda first: (lam0, start, None, st, [first + (cost, True), after + (0.5 * cost, True)])   # noqa: E731
    return [(name, mk(eqs), mk(good), where) for name, eqs, where in broken]


CONDITIONING = tuple((own, lam0, w) for own in (40, 6, 0) for lam0 in (2e-10, 1e-3, 1e6) for w in (1.0, 1e4))
CONDITIONING_SHAPE = dict(seq=(5, None), seq2=(5, None), shared=(4, 41))


def conditioning_cases(kind):
    """[((own, lambda0, weight), script)]: one step of two units, no stiffness, at T = 5 (N = 4, K = 41).  lambda0 2e-10 is
    clamped up to 1e-9 by the first step.  Without own rows the damping alone makes the system definite."""
    n, K = CONDITIONING_SHAPE[kind]
    out = []
    for j, (own, lam0, w) in enumerate(CONDITIONING):
        start, _, _ = _start(kind, 2, n, K, 500 + j, False, False)
        *eqs, cost = system(kind, 2, n, K, own=own, weight=w, seed=600 + j)
        out.append(((own, lam0, w), (lam0, start, None, None, [tuple(eqs) + (cost, True)])))
    return out


def condition_number(kind, script, n):
    """the largest 2-norm condition number over the units of the damped dense system of a one-step script's step"""
    lam0, start, _, _, steps = script
    lam = min(max(float(np.float32(lam0)), 1e-9), 1e6)
    p0, s0 = split(kind, start)
    *eqs, _, _ = steps[0]
    worst = 0.0
    for u in range(p0.shape[0] // n):
        eq = unit_of(kind, eqs, u, n)
        z = np.zeros((n, 26))
        if kind == "shared":
            K = eq[2].shape[2]
            H, _ = sref.dense_system(*eq, lam, np.zeros(26), np.zeros(K), z, z, np.zeros(K), np.zeros(K))
        elif kind == "seq":
            H, _ = qref.dense_system(*eq, lam, np.zeros(26), z, z, n)
        else:
            H, _ = tref.dense_system(*eq, lam, np.zeros(26), z, z, n)
        worst = max(worst, float(np.linalg.cond(H)))
    return worst


LONG_CHAINS = ((3, 64), (65, 2))


def long_chain(kind, U, T):
    """a one-step script of U well-conditioned sequences of T frames whose LAST sequence has the first one's inputs"""
    start, _, mu = _start(kind, U, T, None, 700 + T, False, True)
    *eqs, cost = system(kind, U, T, seed=701 + T)
    eqs = with_unit(kind, tuple(eqs), U - 1, T, tuple(eqs), 0)
    start, cost = start.clone(), cost.clone()
    start[(U - 1) * T:], cost[(U - 1) * T:] = start[:T], cost[:T]
    return 1e-3, start, None, mu, [eqs + (cost, True)]
