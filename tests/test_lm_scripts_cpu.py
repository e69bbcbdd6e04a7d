"""CPU: the scripts of tests/lm_scripts_ref.py are what they claim, the three forms of the reference (the restatement's step,
the word-for-word block solve, the dense solve) agree on every step of them, and the comparator that the GPU tests use tells
six deliberately wrong steps from the right one.  No kernel runs here."""
import functools

import numpy as np
import pytest
import torch

import lm_scripts_ref as ref

SHAPES = [(kind,) + shape for kind in ref.KINDS for shape in ref.SCRIPT_SHAPES[kind]]
LAMBDA_MIN, LAMBDA_MAX = 1e-9, 1e6


@functools.lru_cache(maxsize=None)
def runs(kind, n, K, U):
    """[(script, got, want)]: the restatement driven on its own trials, and reference() on them"""
    out = []
    for script in ref.block_scripts(kind, n, K, U):
        got = ref.drive(ref.Restated(kind, script, n), kind, script)
        out.append((script, got, ref.reference(kind, script, n, got)))
    return out


def letters(want, u):
    return "".join("A" if bool(w["accept"][u]) else "R" for w in want)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_scripts_cover_what_they_claim(kind):
    """Counted from the restatements' histories, per kind over SCRIPT_SHAPES: accepted, rejected-twice and accepted-again units;
    a cost that is not finite in a middle frame; a solve after a reject, whose equations differ from the call's; both clamps
    at n > 1; a step without a solve in the middle and at the end; a unit whose pivot fails next to units whose does not, at
    t > 0, in column 25 and in the last frame (the groups: in a frame's factor and in the Schur block); a prior that is not the
    start, with a stiffness.  Every unit of every step with a solve is compared: nothing is skipped."""
    seen = set()
    for n, K, U in ref.SCRIPT_SHAPES[kind]:
        here = set()
        for script, got, want in runs(kind, n, K, U):
            lam0, start, prior, stiff, steps = script
            assert len(steps) >= 6
            units = want[0]["accept"].shape[0]
            solves = [bool(s[-1]) for s in steps]
            if not solves[-1] and False in solves[1:-1]:
                here.add("no solve in the middle and at the end")
            if prior is not None and stiff is not None:
                p0, pr = ref.split(kind, start)[0], ref.split(kind, prior)[0]
                assert float((p0 - pr).abs().min()) > 0 and float(ref.split(kind, stiff)[0].max()) > 0.1
                here.add("prior and stiffness")
            for u in range(units):
                h = letters(want, u)
                if "ARRA" in h:
                    here.add("accepted, rejected twice, accepted again")
                if set(h) == {"A"}:
                    here.add("all accepted")
            for i, (w, s) in enumerate(zip(want, steps)):
                cost = s[-2].view(units, n)
                odd = ~torch.isfinite(cost)
                if bool(odd.any()):
                    assert bool((odd.sum(1) <= 1).all()) and bool(odd[:, n // 2].any())
                    here.add("nan" if bool(torch.isnan(cost).any()) else "inf")
                if n > 1 and bool((w["lam"] == LAMBDA_MIN).any()):
                    here.add("lower clamp")
                if n > 1 and bool((w["lam"] == LAMBDA_MAX).any()):
                    here.add("upper clamp")
                if w["trial_out"] is None:
                    continue
                assert w["ok"].shape == (units,) and w["gap"].shape == (units,)          # every unit is compared
                if bool((~w["accept"]).any()):
                    assert all(not torch.equal(s[2], earlier[2]) for earlier in steps[:i])    # the call's E (C) is no kept one
                    here.add("solve after a reject")
                if w["bad"]:
                    assert bool(w["ok"].any()), "a failing unit stands next to good ones"
                    here.add("bad pivot next to good units")
                    for t, k in w["bad"].values():
                        here.add("fails at t > 0" if 0 < t < max(n, 2) else "fails at t = 0")
                        if k == 25:
                            here.add("fails in column 25")
                        if t == n - 1:
                            here.add("fails in the last frame")
                        if kind == "shared" and t == n:
                            here.add("fails in the Schur block")
        print("%s n %d K %s U %d: %s" % (kind, n, K, U, sorted(here)))
        every = {"no solve in the middle and at the end", "prior and stiffness", "accepted, rejected twice, accepted again",
                 "all accepted", "nan", "inf", "solve after a reject", "bad pivot next to good units", "fails in column 25",
                 "fails in the last frame"}
        if n > 1:
            every |= {"lower clamp", "upper clamp"}
        every |= {"fails in the Schur block"} if kind == "shared" else {"fails at t > 0"}
        assert every <= here, (kind, n, K, U, sorted(every - here))
        seen |= here
    assert "fails at t > 0" in seen or kind == "shared"


@pytest.mark.parametrize("kind", ref.KINDS)
def test_pivot_cases_fail_where_they_say(kind):
    """pivot_cases: the replayed recurrences fail first at the frame (and column) the case names, in the middle unit only; the
    twin and the second step have no bad pivot at all, and the second step is accepted by every unit."""
    n, K = ref.PIVOT_SHAPE[kind]
    names, cases = [], ref.pivot_cases(kind)
    twin = cases[0][2]
    assert all(all(torch.equal(a, b) for a, b in zip(c[2][4][0][:-1], twin[4][0][:-1])) for c in cases)      # one twin for all
    twin_want = ref.reference(kind, twin, n, ref.drive(ref.Restated(kind, twin, n), kind, twin))
    assert not twin_want[0]["bad"] and not twin_want[1]["bad"]
    for name, script, _, (t, k) in cases:
        got = ref.drive(ref.Restated(kind, script, n), kind, script)
        want = ref.reference(kind, script, n, got)
        assert list(want[0]["bad"]) == [1] and want[0]["bad"][1][0] == t and k in (None, want[0]["bad"][1][1]), (name, want[0]["bad"])
        assert not want[1]["bad"] and bool(want[1]["accept"].all()) and bool(want[0]["accept"].all())
        assert torch.equal(want[0]["trial_out"][n:2 * n], ref.split(kind, script[1])[0][n:2 * n])
        names.append("%s -> %s" % (name, want[0]["bad"][1]))
    print(kind, names)
    ts = [c[3][0] for c in cases]
    assert set(range(1, n)) <= set(ts) and 25 in [c[3][1] for c in cases] and n - 1 in ts


def agree(want):
    """the three forms within compare()'s bar, step by step -> the largest relative |block - dense|"""
    worst = 0.0
    for i, w in enumerate(want):
        if w["trial_out"] is None:
            continue
        U = w["ok"].shape[0]
        pairs = [(w["trial_out"], w["trial_block"], w["trial_dense"])]
        if w["shape_out"] is not None:
            pairs.append((w["shape_out"], w["shape_block"], w["shape_dense"]))
        for a, b, c in pairs:
            a, b, c = a.view(U, -1), b.view(U, -1), c.view(U, -1)
            bar = ref.EPS32 * a.abs() + 1e-12 + ref.MARGIN * w["gap"][:, None]
            for x, y in ((a, b), (a, c), (b, c)):
                assert bool(((x - y).abs() <= bar).all()), (i, float(((x - y).abs() - bar).max()))
        worst = max(worst, float(w["rel"].max()))
    return worst


@pytest.mark.parametrize("kind", ref.KINDS)
def test_three_forms_of_the_reference_agree(kind):
    """The restatement's step (LAPACK for the sequences), the word-for-word block solve and numpy.linalg.solve of the dense
    system agree within the comparator's bar on every step of every script, of pivot_cases, conditioning_cases and
    long_chain; the relative |block - dense| per kind is printed, with the condition numbers that conditioning_cases span."""
    worst = 0.0
    for n, K, U in ref.SCRIPT_SHAPES[kind]:
        worst = max([worst] + [agree(want) for _, _, want in runs(kind, n, K, U)])
    print("%s scripts: the largest relative |block - dense| %.3g" % (kind, worst))
    n = ref.CONDITIONING_SHAPE[kind][0]
    conds, rels = [], []
    for (own, lam0, w), script in ref.conditioning_cases(kind):
        want = ref.reference(kind, script, n, ref.drive(ref.Restated(kind, script, n), kind, script))
        assert bool(want[0]["ok"].all()) and bool(want[0]["accept"].all())
        conds.append(ref.condition_number(kind, script, n))
        rels.append(agree(want))
        print("%s own %2d lambda0 %-7g weight %-6g: condition number %.3g, relative |block - dense| %.3g, largest step %.3g"
              % (kind, own, lam0, w, conds[-1], rels[-1], float((want[0]["trial_dense"] - ref.split(kind, script[1])[0]).abs().max())))
    print("%s conditioning: condition numbers %.3g to %.3g, relative |block - dense| %.3g to %.3g"
          % (kind, min(conds), max(conds), min(rels), max(rels)))
    assert min(conds) < 1e3 and max(conds) > 1e9
    if kind != "shared":
        for U, T in ref.LONG_CHAINS:
            script = ref.long_chain(kind, U, T)
            want = ref.reference(kind, script, T, ref.drive(ref.Restated(kind, script, T), kind, script))
            assert bool(want[0]["ok"].all()) and torch.equal(want[0]["trial_out"][:T], want[0]["trial_out"][-T:])
            assert float((want[0]["trial_out"] - script[1]).abs().max()) > 1e-3
            print("%s S %d T %d: relative |block - dense| %.3g" % (kind, U, T, agree(want)))


# ---- the comparator discriminates ---------------------------------------------------------------------------------------
NEQ = dict(seq=3, seq2=4, shared=5)
COUPLING = dict(seq=("E",), seq2=("E", "F"), shared=("C",))
VARIANTS = {1: "takes E / F / C from the call, not the kept ones", 2: "decides per frame", 3: "no W W^T at the last frame",
            4: "a bad pivot keeps only its own frame", 5: "lambda x 0.3 on the first accepted step", 6: "no prior for t > 0"}


def applies(kind, n, variant):
    if variant == 3:
        return kind != "shared"
    if variant in (2, 6):
        return n > 1
    if variant == 4:
        return n > 1 or kind == "shared"
    return True


def wrong(kind, n, variant):
    """the restatement of `kind` with one deliberate mistake (0: none); its solve is state_solve's, the word-for-word one"""
    base = ref._LM[kind]
    mod = ref._MOD[kind]

    class Wrong(base):
        def book(self, eqs, cost, trial, shape, prior, mu, sprior, nu):
            if kind == "shared":
                base.step(self, *eqs, cost, trial, shape, prior, mu, sprior, nu, False)
            else:
                base.step(self, *eqs, cost, trial, prior, mu, False)

        def book_per_frame(self, eqs, cost, trial, shape, prior, mu, sprior, nu):
            B = trial.shape[0]
            U = B // n
            pr = self.p0 if prior is None else prior
            frame = cost + (0.0 if mu is None else (mu * (trial - pr) ** 2).sum(1))
            if kind == "shared" and nu is not None:
                frame = frame.clone()
                frame[::n] += (nu * (shape - (self.s0 if sprior is None else sprior)) ** 2).sum(1)
            if not hasattr(self, "fcost"):
                self.fcost = torch.full((B,), ref.INF, dtype=torch.float64)
            acc = torch.isfinite(frame) & (frame < self.fcost)
            first = acc[::n]
            self.fcost = torch.where(acc, frame, self.fcost)
            self.p = torch.where(acc[:, None], trial, self.p)
            self.A, self.g = torch.where(acc[:, None, None], eqs[0], self.A), torch.where(acc[:, None], eqs[1], self.g)
            for name, e in zip(COUPLING[kind], eqs[2:]):
                setattr(self, name, torch.where(acc[:, None, None], e, getattr(self, name)))
            if kind == "shared":
                self.R, self.gs = torch.where(first[:, None, None], eqs[3], self.R), torch.where(first[:, None], eqs[4], self.gs)
                self.s = torch.where(first[:, None], shape, self.s)
            self.cost = self.fcost.view(U, n).sum(1)
            factor = torch.where(first, torch.where(self.moved, 0.3, 1.0), 10.0).double()
            self.lam = (self.lam * factor).clamp(LAMBDA_MIN, LAMBDA_MAX)
            self.moved = self.moved | first
            self.history.append(first.clone())
            if self.fresh:
                self.cost0, self.fresh = frame.view(U, n).sum(1), False

        def step(self, *args):
            eqs, rest = tuple(e.double() for e in args[:NEQ[kind]]), args[NEQ[kind]:]
            if kind == "shared":
                cost, trial, shape, prior, mu, sprior, nu, solve = rest
            else:
                (cost, trial, prior, mu, solve), shape, sprior, nu = rest, None, None, None
            trial = trial.double()
            if variant == 6 and prior is not None:
                late = (torch.arange(trial.shape[0]) % n > 0)[:, None]
                prior = torch.where(late, self.p0, prior)
            moved = self.moved.clone()
            (self.book_per_frame if variant == 2 else self.book)(eqs, cost, trial, shape, prior, mu, sprior, nu)
            if variant == 5:
                first = self.history[-1] & ~moved
                self.lam = torch.where(first, (self.lam * 0.3).clamp(LAMBDA_MIN, LAMBDA_MAX), self.lam)
            if not solve:
                return (None, None) if kind == "shared" else None
            kept = [getattr(self, name) for name in COUPLING[kind]]
            if variant == 1:
                for name, e in zip(COUPLING[kind], eqs[2:]):
                    setattr(self, name, e)
            orig, frame_ = mod._cholesky, [0]

            def no_last_outer(M, lam, Wt, *Vt):                # frame 0 of a unit is the call without a W
                frame_[0] = 0 if Wt is None else frame_[0] + 1
                return orig(M, lam, None, *((None,) * len(Vt))) if frame_[0] == n - 1 else orig(M, lam, Wt, *Vt)

            if variant == 3:
                mod._cholesky = no_last_outer
            try:
                delta, ds, ok = ref.state_solve(kind, self, n, prior, mu, sprior, nu)
            finally:
                mod._cholesky = orig
            if variant == 4:
                eq_kept = ref.kept(kind, self)
                pr = self.p0 if prior is None else prior
                m = torch.zeros(26, dtype=torch.float64) if mu is None else mu
                for u in np.nonzero(~ok.numpy())[0]:
                    t, _ = ref.first_bad_pivot(kind, ref.unit_of(kind, eq_kept, u, n), float(self.lam[u]), m.numpy(),
                                               None if nu is None else nu.numpy())
                    for b in range(u * n, u * n + n):
                        if b != u * n + t:                     # every other frame takes a step of its own
                            M = self.A[b] + torch.diag(m)
                            M = M + float(self.lam[u]) * torch.diag(torch.diagonal(M))
                            delta[b] = torch.linalg.solve(M, -(self.g[b] + m * (self.p[b] - pr[b])))
            for name, e in zip(COUPLING[kind], kept):
                setattr(self, name, e)
            self.ok = ok
            self.trial = ref.f32(self.p + delta)
            if kind != "shared":
                return self.trial
            self.trial_shape = ref.f32(self.s + ds)
            return self.trial, self.trial_shape

    return Wrong


@pytest.mark.parametrize("kind,n,K,U", SHAPES)
def test_comparator_flags_each_wrong_step(kind, n, K, U):
    """Each script run through the six wrong variants of the restatement, as the GPU tests run the kernels: the variant's
    own trials go to the right restatement, and compare() must name a difference -- for every variant that applies to the
    shape, on at least one script (a variant can only show where a script has its edge: a reject, a bad pivot, a prior).
    Variant 0, the right step formed by the word-for-word solve instead of LAPACK, passes on every script."""
    scripts = ref.block_scripts(kind, n, K, U)
    for variant in (0,) + tuple(VARIANTS):
        if variant and not applies(kind, n, variant):
            continue
        flagged = []
        for j, script in enumerate(scripts):
            got = ref.drive(ref.Restated(kind, script, n, wrong(kind, n, variant)), kind, script)
            want = ref.reference(kind, script, n, got)
            diff = ref.compare(got, want, ref.bars_of(want))
            if diff:
                flagged.append((j, diff[0]))
                break                                          # (one script is enough; the others only take time)
        print("%s n %d variant %d (%s): %s" % (kind, n, variant, VARIANTS.get(variant, "none"), flagged))
        assert bool(flagged) == bool(variant), (variant, flagged)
