"""The sliding-window tracker's two entries without a device: the entries in the C ABI with their argument rules, the unit's
code-object metadata, and the restatement (tests/lm_window_ref.py) with what keeps it honest -- the restated marginalisation
equals the Schur complement by numpy.linalg.solve on the dense departing matrix over a conditioning sweep, marginalise-and-slide
on a quadratic energy equals the full-batch solve of the newest frames and their covariance, the special cases of the contract,
and the comparators tell wrong variants from the right one.  The GPU tests (tests/test_lm_window_gpu.py) hold the kernels to the
same restatement with the same comparators."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lm_scripts_ref as lref
import lm_window_ref as wref
from conftest import ROOT
from test_pose_ik_cpu import _metadata

ENTRIES = ("shr_pose_window_marginalize_workspace_bytes", "shr_pose_window_marginalize",
           "shr_pose_window_prior_normal_workspace_bytes", "shr_pose_window_prior_normal")
EPS = 2.0 ** -52


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert _lib.ABI_VERSION == 23 and h.shr_abi_version() == 23        # additions only
    contract = text[text.index("The sliding window: marginalise"):text.index("long long shr_pose_window_marginalize_workspace_bytes(")]
    for cite in ("DEPARTING SYSTEM", "FRAME 0 ONLY", "LOWER triangle", "column recurrence", "row recurrence", "subtracted ONCE",
                 "Lambda_12 = E_1 - X_E^T X_F", "y.y", "bit-symmetric", "frame 1's rows and frame 2's columns", "exact +0",
                 "point is still written", "no atomics", "capturable in a hipGraph", "65535", "NOT", "never relinearised",
                 "(Lambda d)_i + eta_i", "NEVER touched", "active [S]"):
        assert cite in contract, cite
    assert text.index("shr_pose_lm_seq2_covariance(") < text.index("shr_pose_window_marginalize(")      # after the covariance
    lib = _lib.lib()
    for wb in (lib.shr_pose_window_marginalize_workspace_bytes, lib.shr_pose_window_prior_normal_workspace_bytes):
        assert [wb(*a) for a in ((0, 1), (6, 3), (-1, 3), (6, -1))] == [0, 0, -1, -1]
    P = 1 << 20                                                    # an aligned stand-in for a device address
    #       0 A 1 g 2 E 3 F 4 cost 5 trial 6 prior 7 stiffness | 8 B 9 T | 10 Lambda 11 eta 12 offset 13 point 14 status 15 ws 16 stream
    args = [P] * 8 + [6, 3] + [P] * 5 + [None, None]
    call = lambda i, val, base=args: lib.shr_pose_window_marginalize(*(base[:i] + [val] + base[i + 1:]))   # noqa: E731
    assert call(8, 0) == 0                                         # the no-op
    for i in (0, 1, 4, 5, 10, 11, 12, 13, 14):
        assert call(i, None) == -1, i
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14):
        assert call(i, P + 2) == -1, i
    for i in (0, 1, 2, 3, 4, 10, 11, 12):                          # fp64 buffers: 8 bytes
        assert call(i, P + 4) == -1, i
    assert call(8, -3) == -1 and call(9, 0) == -1 and call(9, 4) == -1
    assert call(8, 65536 * 3) == -2
    none = list(args)
    none[8] = 0
    assert call(9, 0, none) == -1                                  # the rules come before the no-op
    optional = list(args)                                          # E, F, prior and stiffness may be NULL
    for i in (2, 3, 6, 7):
        optional[i] = None
    assert call(8, 0, optional) == 0
    #       0 trial 1 Lambda 2 eta 3 offset 4 point 5 active | 6 B 7 T 8 accumulate 9 accumulate_E | 10 A 11 g 12 E 13 cost 14 ws 15 stream
    args = [P] * 6 + [6, 3, 1, 1] + [P] * 4 + [None, None]
    call = lambda i, val, base=args: lib.shr_pose_window_prior_normal(*(base[:i] + [val] + base[i + 1:]))   # noqa: E731
    assert call(6, 0) == 0
    for i in (0, 1, 2, 3, 4, 10, 11, 12, 13):
        assert call(i, None) == -1, i
    for i in (0, 1, 2, 3, 4, 5, 10, 11, 12, 13):
        assert call(i, P + 2) == -1, i
    for i in (1, 2, 3, 10, 11, 12, 13):
        assert call(i, P + 4) == -1, i
    assert call(6, -3) == -1 and call(7, 0) == -1 and call(7, 4) == -1 and call(6, 65536 * 3) == -2
    for i in (8, 9):
        assert call(i, 2) == -1 and call(i, -1) == -1, i
    none = list(args)
    none[6] = 0
    assert call(8, 2, none) == -1 and call(7, 0, none) == -1
    frames = list(args)                                            # E may be NULL with T == 1 alone; active may be NULL
    frames[5], frames[6], frames[7], frames[12] = None, 0, 1, None
    assert call(6, 0, frames) == 0


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """lm_window.hip: two kernels, no scratch, no spills, no matrix-core instruction (its accumulation order is not the
    contract's).  marginalize: L [26 x 26], X [26 x 53] and 26 cost terms in fp64, 16 640 bytes; prior: d and Lambda d, 832
    bytes.  DESIGN.md 4.4z tables the figures.  The unit includes lm_solve.h alone."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4z"):design.index("### 4.5 ")]
    sizes, kernels = _metadata("lm_window", tmp_path)
    assert sizes == [0] * 2 and len(kernels) == 2
    # LDS exact; (VGPRs, SGPRs) as built, the ceilings a few above: they only catch a change of code that costs registers
    want = {"marginalize": ((676 + 26 * 53 + 26) * 8, 26, 68), "prior": (2 * 52 * 8, 16, 50)}
    seen = set()
    for name, k in kernels.items():
        print(name, k)
        which = re.search(r"pose_window_([a-z]+)_kernel", name).group(1)
        seen.add(which)
        lds, vgpr, sgpr = want[which]
        assert "pose_window_%s_kernel" % which in section
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        assert k["group_segment_fixed_size"] == lds, which
        assert k["vgpr_count"] <= vgpr + 6 and k["sgpr_count"] <= sgpr + 8, which
    assert seen == set(want)
    assert want["marginalize"][0] == 16640 and want["prior"][0] == 832
    assert "16 640" in section and "832" in section
    assert "v_mfma" not in open(str(tmp_path / "lm_window.s")).read()
    text = open(os.path.join(ROOT, "spherehand_amd", "csrc", "lm_window.hip")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["lm_solve.h"]


def test_restatement_equals_the_dense_schur_complement():
    """Over T in {1, 2, 3, 5} x band {1, 2} x own rows {40, 6} x mu {0, 1e-3, 0.5} x weight {1, 1e4}: where M_0 factorises,
    the largest |restatement - dense| entry of Lambda, eta and the offset is within 78 kappa(M_0) 2^-52 of the largest
    magnitude that enters it -- both are backward-stable solves with M_0 followed by one product of at most 78 terms and one
    subtraction, so each carries a forward error of the order n kappa eps of the OPERANDS of that subtraction (C M_0^-1 C^T
    beside the blocks of frames 1 and 2; the costs beside b_0^T M_0^-1 b_0), which can be far larger than the result.
    Nothing is taken from the measured values, which the table printed here (DESIGN.md 4.4z's) shows orders below."""
    seen = 0
    for T in wref.SWEEP_T:
        rels, conds = [], []
        for i, (band, own, mu, w) in enumerate(wref.SWEEP):
            A, g, E, F, cost = wref.system(1, T, band, own, w, seed=600 + i)
            trial, prior = wref.poses(T, 600 + i)
            m = wref.stiffness(mu)
            want = wref.reference(A, g, E, F, cost, trial, T, prior, m)
            if want["status"][0]:
                assert own < 26 and mu == 0.0 and (T < 3 or band == 1 and T < 2), (T, band, own, mu, w)
                continue
            a, gg, e, f = (None if X is None else X.numpy() for X in (A, g, E, F))
            M0 = np.tril(a[0]) + np.tril(a[0], -1).T + np.diag(np.zeros(26) if m is None else m.double().numpy())
            kappa = float(np.linalg.cond(M0))
            n = min(T, 3)
            C = np.zeros((26 * (n - 1), 26))
            if n >= 2:
                C[:26] = e[0].T
            if n == 3 and f is not None:
                C[26:] = f[0].T
            d = trial[0].double().numpy() - prior[0].double().numpy()
            b0 = gg[0] + (0.0 if m is None else m.double().numpy() * d)
            inv = np.linalg.inv(M0)
            scale = (max(np.abs(a[:n]).max(), np.abs(e[:n]).max(), np.abs(C @ inv @ C.T).max() if n >= 2 else 0.0),
                     max(np.abs(gg[:n]).max(), np.abs(C @ inv @ b0).max() if n >= 2 else 0.0),
                     max(np.abs(cost.numpy()[:n]).sum(), abs(b0 @ inv @ b0)))
            for k in range(3):
                assert want["gap"][0, k] <= 78 * kappa * EPS * scale[k], (T, band, own, mu, w, k, want["gap"][0, k], kappa)
            rels.append(want["gap"][0] / np.maximum(want["size"][0], 1e-300))
            conds.append(kappa)
            seen += 1
        rels = np.array(rels)
        print("T=%d: %2d cases, |restatement - dense| / largest entry: Lambda %.1e ... %.1e, eta %.1e ... %.1e, offset %.1e ... %.1e;"
              " condition numbers of M_0 %.1e ... %.1e" % (T, len(rels), rels[:, 0].min(), rels[:, 0].max(), rels[:, 1].min(),
                                                             rels[:, 1].max(), rels[:, 2].min(), rels[:, 2].max(), min(conds), max(conds)))
    assert seen >= 88          # 96 cases; only mu = 0 with fewer own rows than unknowns and too few coupling rows fails


def test_special_cases():
    """T == 1 and E None: an exact +0 prior with the offset of the contract; F None is F = 0 and T == 2 is the leading block
    of T == 3 with E_1, A_2 and F gone, bit for bit (a product with an exact zero adds nothing); Lambda is bit-symmetric and
    positive semi-definite (the Schur complement of a Gram matrix); a prior pose and a stiffness move eta and the offset only
    through b_0, and only frame 0's."""
    A, g, E, F, cost = (X.numpy() for X in wref.system(1, 3, 2, seed=811))
    trial, prior = (X.numpy() for X in wref.poses(3, 811))
    mu = wref.random_stiffness(3).numpy()
    L, e, c, p, st = wref.marginalize(A, g, E, F, cost, trial, prior, mu)
    assert st == 0 and np.array_equal(L, L.T) and np.linalg.eigvalsh(L).min() > -1e-12 * np.abs(L).max()
    assert np.array_equal(p, trial[1:].reshape(-1))
    for eqs in ((A[:1], g[:1], E[:1], F[:1], cost[:1], trial[:1], prior[:1]), (A, g, None, F, cost, trial, prior)):
        L0, e0, c0, p0, st0 = wref.marginalize(*eqs, mu)
        assert st0 == 0 and not L0.any() and not e0.any() and not np.signbit(L0).any() and np.isfinite(c0) and c0 != 0.0
    assert not wref.marginalize(A[:1], g[:1], E[:1], F[:1], cost[:1], trial[:1], prior[:1], mu)[3].any()
    zero = wref.marginalize(A, g, E, np.zeros_like(F), cost, trial, prior, mu)
    none = wref.marginalize(A, g, E, None, cost, trial, prior, mu)
    assert all(np.array_equal(a, b) for a, b in zip(zero, none))
    assert np.array_equal(none[0][26:, 26:], np.tril(A[2]) + np.tril(A[2], -1).T) and np.array_equal(none[0][:26, 26:], E[1])
    two = wref.marginalize(A[:2], g[:2], E[:2], F[:2], cost[:2], trial[:2], prior[:2], mu)
    assert np.array_equal(two[0][:26, :26], L[:26, :26]) and np.array_equal(two[1][:26], e[:26])
    assert not two[0][26:].any() and not two[0][:, 26:].any() and not two[1][26:].any() and not two[3][26:].any()
    assert two[2] != c                                             # frame 2's cost is not in it
    plain = wref.marginalize(A, g, E, F, cost, trial, None, None)
    moved = wref.marginalize(A, g, E, F, cost, trial, prior, None)     # a prior pose without a stiffness: nothing
    assert all(np.array_equal(a, b) for a, b in zip(plain, moved))
    other = prior.copy()
    other[1:] += 1.0                                               # the prior poses of frames 1 and 2 are not read
    assert all(np.array_equal(a, b) for a, b in zip(wref.marginalize(A, g, E, F, cost, trial, other, mu), (L, e, c, p, st)))


def test_marginalise_and_slide_is_the_full_batch_solve():
    """lm_window_ref.chain in fp64 on a quadratic: banded_system(U = 2, T = 8, band = 2), frames 0 ... 4 marginalised one after
    the other, each prior entering the next departing system through the restated prior entry at a trial pose different from
    its point; the last three frames' solution equals the dense 208-unknown solve's, the inverse of the final 78 x 78 the
    dense inverse's last block, each within MARGIN x the distance of two dense routes (solve against inv; lm_window_ref.chain
    says how the two are linearised).  The energy's minimum is reported: one number against one number is no bar.  A chain
    whose prior term forgets to subtract the point misses by orders: d != 0 is exercised."""
    out = wref.chain(wref.restated_entries())
    assert all(not s.any() for s in out["status"]) and len(out["status"]) == 5
    for key in ("x", "Z", "energy"):
        err = np.abs(out[key] - out[key + "_dense"]).reshape(2, -1).max(1)
        print("%-6s |chain - dense| %s; bar (4 x |solve - inv|) %s; largest entry %.3g"
              % (key, err, out["bar_" + key], np.abs(out[key + "_dense"]).max()))
        if key != "energy":
            assert (out["bar_" + key] > 0).all() and (err <= out["bar_" + key]).all(), (key, err, out["bar_" + key])
    marg, prior = wref.restated_entries()
    shifted = wref.chain((marg, lambda trial, L, e, o, p, T, A, g, E, cost:
                          wref.prior_normal(trial, L, e, o, p, T, A, g, E, cost, 1, 1, variant="point not subtracted")))
    assert (np.abs(shifted["x"] - out["x_dense"]).reshape(2, -1).max(1) > 1e6 * out["bar_x"]).all()


def _as_got(want):
    return tuple(want[k].copy() for k in ("Lambda", "eta", "offset", "point", "status"))


@pytest.mark.parametrize("band", (1, 2))
@pytest.mark.parametrize("T", (1, 2, 3, 5))
def test_comparator_tells_wrong_variants(band, T):
    """The comparator passes the restatement and the dense Schur complement, and names every wrong variant on every shape
    it applies to: E_0 untransposed (T >= 2), the F term dropped from Lambda_22 and Lambda_12 (band 2, T >= 3), eta without
    its Schur correction (T >= 2), the offset without -y.y, the stiffness applied to frame 1 (T >= 2), one entry off by 1e-3
    of itself (which also breaks the symmetry), a point that is not the trial's, a wrong status, a failed sequence that
    returns NaN instead of +0 or keeps its values."""
    S = 2
    A, g, E, F, cost = wref.system(S, T, band, seed=840 + T)
    trial, prior = wref.poses(S * T, 840 + T)
    mu = wref.random_stiffness(6)
    want = wref.reference(A, g, E, F, cost, trial, T, prior, mu)
    out = {}
    assert wref.compare(_as_got(want), want, out) == [] and out["exact"] == out["live"] == S
    mirrored = np.tril(want["dense_Lambda"]) + np.tril(want["dense_Lambda"], -1).transpose(0, 2, 1)
    assert wref.compare((mirrored, want["dense_eta"], want["dense_offset"], want["point"], want["status"]), want) == []
    applies = {"E untransposed": T >= 2, "F dropped": band == 2 and T >= 3, "eta uncorrected": T >= 2,
               "offset without y.y": True, "stiffness on frame 1": T >= 2}
    for name, on in applies.items():
        if not on:
            continue
        w = wref.reference(A, g, E, F, cost, trial, T, prior, mu, variant=name)
        bad = wref.compare(_as_got(w), want)
        assert len(bad) >= S and all("off by" in b for b in bad), (name, bad)            # every sequence is named
    if T >= 2:
        got = _as_got(want)
        got[0][0, 3, 5] *= 1.0 + 1e-3
        assert any("off by" in b or "symmetric" in b for b in wref.compare(got, want))
        got = _as_got(want)
        got[3][1, 4] = np.nextafter(got[3][1, 4], np.float32(9))
        assert any("point" in b for b in wref.compare(got, want))
    got = _as_got(want)
    got[4][1] = 1
    assert any("status" in b for b in wref.compare(got, want))
    kind = "seq2" if band == 2 else "seq"
    eqs = (A, g, E, F) if band == 2 else (A, g, E)
    broken = lref.break_column(kind, eqs, 1, T, 0, 0.0, mu.double().numpy())
    w = wref.reference(broken[0], g, E, F, cost, trial, T, prior, mu)
    assert w["status"].tolist() == [0, 1] and not w["Lambda"][1].any() and w["offset"][1] == 0.0
    assert wref.compare(_as_got(w), w) == []
    nan = wref.reference(broken[0], g, E, F, cost, trial, T, prior, mu, variant="NaN on failure")
    bad = wref.compare(_as_got(nan), w)
    assert len(bad) == 3 and all("not +0" in b for b in bad), bad
    kept = _as_got(want)
    kept[4][1] = 1                                                 # the good batch's values under the failing status
    assert any("not +0" in b for b in wref.compare(kept, w))
    assert any("status" in b for b in wref.compare(_as_got(want), w))


@pytest.mark.parametrize("T", (1, 2, 3, 5))
def test_prior_term_restated_against_matmul(T):
    """The restated prior term against d^T Lambda d + 2 eta^T d + offset and its derivatives by matmul: within 104 eps of the
    absolute sums (two orders of a 52-term double sum differ by at most 52 eps of it each); accumulate adds exactly one
    fp64 number per entry, writes both triangles, and leaves frames >= 2, E but frame 0's, and an inactive sequence alone;
    the comparator names a point that is not subtracted."""
    S = 3
    record = wref.record_of(S, 860 + T)
    Lam, eta, offset, point = record
    trial, _ = wref.poses(S * T, 861 + T, prior=False)
    zeros = (np.zeros((S * T, 26, 26)), np.zeros((S * T, 26)), np.zeros((S * T, 26, 26)), np.zeros(S * T))
    alone = wref.prior_normal(trial, *record, T, *zeros, 0, 0)
    dense = wref.prior_dense(trial, *record, T)
    n = 26 if T == 1 else 52
    for q in range(S):
        d = np.abs(trial.numpy()[q * T:q * T + n // 26].reshape(-1).astype(np.float64) - point[q, :n])
        bound = 104 * EPS * (np.abs(Lam[q, :n, :n]) @ d + np.abs(eta[q, :n]))
        for t in range(n // 26):
            assert (np.abs(alone[1][q * T + t] - dense[1][q * T + t]) <= bound[26 * t:26 * t + 26]).all()
            assert np.array_equal(alone[0][q * T + t], dense[0][q * T + t])
        assert abs(alone[3][q * T] - dense[3][q * T]) <= 208 * EPS * (d @ np.abs(Lam[q, :n, :n]) @ d + 2 * np.abs(eta[q, :n]) @ d
                                                                         + abs(offset[q]))
    assert wref.compare_prior(alone, alone, (dense, alone), T) == []
    eqs = wref.system(S, T, 1, seed=870 + T)
    A, g, E, cost = (eqs[i].numpy() for i in (0, 1, 2, 4))
    active = np.array([1, 0, 1], np.int32)
    got = wref.prior_normal(trial, *record, T, A, g, E, cost, 1, 1, active)
    for q in range(S):
        sl = slice(q * T, q * T + T)
        if not active[q]:
            assert all(np.array_equal(v[sl], w[sl]) for v, w in zip(got, (A, g, E, cost)))
            continue
        m = min(T, 2)
        low = np.tril(A[sl][:m]) + np.tril(alone[0][sl][:m])
        assert np.array_equal(got[0][sl][:m], low + np.tril(low, -1).transpose(0, 2, 1))
        assert np.array_equal(got[1][sl][:m], g[sl][:m] + alone[1][sl][:m]) and got[3][q * T] == cost[q * T] + alone[3][q * T]
        assert np.array_equal(got[0][sl][m:], A[sl][m:]) and np.array_equal(got[1][sl][m:], g[sl][m:])
        assert np.array_equal(got[3][sl][1:], cost[sl][1:]) and np.array_equal(got[2][sl][1:], E[sl][1:])
        if T >= 2:
            assert np.array_equal(got[2][q * T], E[q * T] + Lam[q, :26, 26:])
    wrong = wref.prior_normal(trial, *record, T, *zeros, 0, 0, variant="point not subtracted")
    bad = wref.compare_prior(wrong, alone, (dense, alone), T)
    assert len(bad) >= S and all("off by" in b for b in bad), bad


def test_gpu_cases_are_what_they_say():
    """The inputs of the GPU tests: every shape case factorises (a dense Cholesky of M_0 agrees), S, T, bands and the NULL
    cases are all there; the prior cases carry every flag combination and an `active` with a 0 in the middle; the pivot cases
    fail in the middle sequence alone, in column 25 of frame 0."""
    shapes = wref.shape_cases()
    for name, T, (A, g, E, F, cost), trial, prior, mu in shapes:
        for s in range(A.shape[0] // T):
            M0 = A[s * T].numpy() + np.diag(np.zeros(26) if mu is None else mu.double().numpy())
            np.linalg.cholesky(M0)
    seen = {(A.shape[0] // T, T, F is not None) for _, T, (A, g, E, F, cost), _, _, _ in shapes if E is not None}
    assert {(S, T) for S, T, _ in seen} == {(S, T) for S in (1, 3, 65) for T in (1, 2, 3, 5)}
    assert any(E is None for _, _, (A, g, E, F, c), _, _, _ in shapes) and any(p is None for _, _, _, _, p, _ in shapes)
    assert any(m is None for *_, m in shapes) and any(m is not None for *_, m in shapes)
    priors = wref.prior_cases()
    assert {(c[5], c[6]) for c in priors} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c[3].shape[0] // c[1], c[1]) for c in priors} == {(S, T) for S in (1, 3, 65) for T in (1, 2, 3, 5)}
    mids = [c for c in priors if c[7] is not None]
    assert mids and all(int(c[7][c[7].shape[0] // 2]) == 0 and int(c[7].sum()) == c[7].shape[0] - 1 for c in mids)
    for band in (1, 2):
        bad, good, trial, prior, mu = wref.pivot_case(band)
        assert wref.reference(*bad, trial, wref.PIVOT_T, prior, mu)["status"].tolist() == [0, 1, 0]
        assert not wref.reference(*good, trial, wref.PIVOT_T, prior, mu)["status"].any()
        kind, eqs = ("seq2", bad[:4]) if band == 2 else ("seq", bad[:3])
        assert lref.first_bad_pivot(kind, lref.unit_of(kind, eqs, 1, wref.PIVOT_T), 0.0, mu.double().numpy()) == (0, 25)


def test_study_on_one_short_stream():
    """What DESIGN.md 4.4z's study shows with a clear margin, on one `blind` stream of five frames at W = 3 and two iterations
    (seconds): no pivot fails; the tracker's smoothed poses are more than 10 % better than the frame-by-frame fit's (5.6 against
    7.3 mm here); the prior barely reaches the newest frame -- its sigma is not larger with the prior and within 1 % of the
    one without (2.959 against 2.964 mm); and the hidden finger is NOT remembered: it stays more than 20 mm off with the prior
    and within 10 % of where the same windows leave it without (37.06 against 37.11 mm)."""
    from spherehand_amd import hand_model
    rows = wref.study(hand_model.load_mesh(), S=1, N=5, win=3, iters=2, families=("blind",), out=lambda s: None)
    by = {r["name"]: r for r in rows}
    assert set(by) == {"tracker", "window", "frames", "batch"}
    t, w, f = by["tracker"], by["window"], by["frames"]
    assert t["failed"] == 0
    assert t["smoothed"] < 0.9 * f["smoothed"], (t, f)
    assert t["sigma_with"] <= t["sigma_without"] * (1 + 1e-9) and t["sigma_with"] > 0.99 * t["sigma_without"], t
    assert t["smoothed_hidden"] > 20.0 and abs(t["smoothed_hidden"] - w["smoothed_hidden"]) < 0.1 * w["smoothed_hidden"], (t, w)
    assert f["smoothed"] == f["filtered"] and by["batch"]["smoothed"] == by["batch"]["filtered"]
