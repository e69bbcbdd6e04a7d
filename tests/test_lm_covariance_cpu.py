"""The marginal covariances of the sequence fit without a device: the entry in the C ABI with its argument rules, the unit's
code-object metadata, and the restatement (tests/lm_covariance_ref.py) with what keeps it honest -- the selected inversion
equals numpy.linalg.inv of the dense 26 T x 26 T matrix over a conditioning sweep, the special cases of the contract, the
comparator tells wrong variants from the right one, a broken coupling fails at the frame it enters, and what the study
 shows.  The GPU tests (tests/test_lm_covariance_gpu.py) hold the kernels to the same restatement with the
same comparator."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lm_covariance_ref as cref
import lm_scripts_ref as lref
from conftest import ROOT
from test_pose_ik_cpu import _metadata

ENTRIES = ("shr_pose_lm_seq2_covariance_workspace_bytes", "shr_pose_lm_seq2_covariance")
EPS = 2.0 ** -52


def test_header_loader_and_library_have_the_entries():
    from spherehand_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "spherehand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    contract = text[text.index("The uncertainty of the sequence fit"):text.index("long long shr_pose_lm_seq2_covariance_workspace_bytes(")]
    for cite in ("UNDAMPED", "lambda = 0", "LOWER triangle", "W product subtracted first", "m ascending", "Z_{t+1,t}", "Z_{t+2,t}",
                 "N_t^T N_t", "bit-symmetric", "xx xy xz yy yz zz", "1 + t", "ALL that sequence's frames", "no atomics",
                 "capturable in a hipGraph", "16 320 B", "65535", "NOT"):
        assert cite in contract, cite
    assert text.index("int shr_pose_lm_seq2_step(") < text.index("shr_pose_lm_seq2_covariance(")     # after the sequence steps
    lib = _lib.lib()
    wb = lib.shr_pose_lm_seq2_covariance_workspace_bytes
    assert [wb(B) for B in (0, 1, 6, -1)] == [0, 16320, 6 * 16320, -1]
    P = 1 << 20                                                    # an aligned stand-in for a device address
    #       0 A 1 E 2 F 3 stiffness 4 jac | 5 B 6 T 7 J | 8 cov 9 sphere_cov 10 status 11 workspace 12 stream
    args = [P, P, P, P, P, 6, 3, 41, P, P, P, P, None]
    call = lambda i, val, base=args: lib.shr_pose_lm_seq2_covariance(*(base[:i] + [val] + base[i + 1:]))   # noqa: E731
    assert call(5, 0) == 0                                         # the no-op
    for i in (0, 8, 10, 11):
        assert call(i, None) == -1, i
    assert call(4, None) == -1 and call(9, None) == -1             # exactly one of jac and sphere_cov
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        assert call(i, P + 2) == -1, i
    for i in (0, 1, 2, 8, 9):                                      # fp64 buffers: 8 bytes
        assert call(i, P + 4) == -1, i
    assert call(11, P + 8) == -1                                   # the workspace: 16 bytes
    assert call(5, -3) == -1 and call(6, 0) == -1 and call(6, 4) == -1 and call(7, 0) == -1
    assert call(5, 65536 * 3) == -2 and call(7, 65) == -2
    none = list(args)
    none[5] = 0
    for i, val, rc in ((6, 0, -1), (7, 65, -2), (7, 0, -1)):       # the rules come before the no-op
        assert call(i, val, none) == rc
    optional = list(args)                                          # E, F, stiffness and the pair (jac, sphere_cov) may be NULL
    for i in (1, 2, 3, 4, 9):
        optional[i] = None
    assert call(5, 0, optional) == 0


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """lm_covariance.hip: two kernels, no scratch, no spills, no matrix-core instruction (its accumulation order is not the
    contract's).  chain: nine [26 x 26] fp64 blocks, 48 672 bytes, three sequences per CU by LDS; project: Z in fp64 and the
    frame's 192 x 26 fp32 Jacobian, 25 376 bytes.  DESIGN.md 4.4y tables the figures.  The unit includes lm_solve.h alone."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4y"):design.index("### 4.5 ")]
    sizes, kernels = _metadata("lm_covariance", tmp_path)
    assert sizes == [0] * 2 and len(kernels) == 2
    # LDS exact; (VGPRs, SGPRs) as built, the ceilings a few above: they only catch a change of code that costs registers
    want = {"chain": (9 * 676 * 8, 32, 94), "project": (676 * 8 + 192 * 26 * 4, 33, 28)}
    seen = set()
    for name, k in kernels.items():
        print(name, k)
        which = re.search(r"pose_lm_seq2_covariance_([a-z]+)_kernel", name).group(1)
        seen.add(which)
        lds, vgpr, sgpr = want[which]
        assert "pose_lm_seq2_covariance_%s_kernel" % which in section
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        assert k["group_segment_fixed_size"] == lds, which
        assert k["vgpr_count"] <= vgpr + 6 and k["sgpr_count"] <= sgpr + 8, which
    assert seen == set(want)
    assert want["chain"][0] == 48672 and want["project"][0] == 25376
    assert "48 672" in section and "25 376" in section
    assert "v_mfma" not in open(str(tmp_path / "lm_covariance.s")).read()
    text = open(os.path.join(ROOT, "spherehand_amd", "csrc", "lm_covariance.hip")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["lm_solve.h"]


def seq(eqs, s, T):
    return tuple(None if X is None else cref._np(X[s * T:s * T + T]) for X in eqs)


def test_restatement_equals_the_dense_inverse():
    """Over kind x T in {1, 2, 3, 5, 8} x own rows {40, 6, 0} x mu {0, 1e-3, 0.5} x weight {1, 1e4}: where the sequence
    factorises at lambda = 0, the largest |restatement - dense| entry is within 26 T kappa 2^-52 of the largest entry -- both
    inverses are backward stable, so each carries a forward error of the order n kappa eps (n = 26 T unknowns, kappa the
    2-norm condition number of the dense matrix); nothing is taken from the measured values, which the table printed here
    (DESIGN.md 4.4y's) shows two to six orders below.  T = 1: against inv(A + diag mu) itself."""
    seen = 0
    for kind in cref.KINDS:
        for T in cref.SWEEP_T:
            rels, conds = [], []
            for i, (own, mu, w) in enumerate(cref.SWEEP):
                eqs = cref.equations(kind, 1, T, own, w, seed=600 + i)
                m = cref.stiffness(mu)
                want = cref.reference(*eqs, T, m)
                if want["status"][0]:
                    assert own < 26 and mu == 0.0, (kind, T, own, mu, w)       # only a matrix nothing makes definite fails
                    continue
                kappa = float(np.linalg.cond(cref.dense_matrix(*seq(eqs, 0, T), cref._np(m))))
                rel = want["gap"][0] / want["size"][0]
                assert rel <= 26 * T * kappa * EPS, (kind, T, own, mu, w, rel, kappa)
                rels.append(rel), conds.append(kappa)
                if T == 1:
                    M = cref._np(eqs[0][0]) + np.diag(np.zeros(26) if m is None else m.double().numpy())
                    assert np.abs(want["cov"][0] - np.linalg.inv(M)).max() <= 26 * kappa * EPS * want["size"][0]
                seen += 1
            print("%-4s T=%d: %2d cases, |restatement - dense| / largest entry %.1e ... %.1e, condition numbers %.1e ... %.1e"
                  % (kind, T, len(rels), min(rels), max(rels), min(conds), max(conds)))
    assert seen >= 140          # 180 cases; at most the 40 with mu = 0 and fewer own rows than unknowns fail


@pytest.mark.parametrize("kind", cref.KINDS)
def test_special_cases(kind):
    """E = F = 0 is T independent frames and F None is F = 0, bit for bit (a product with an exact zero adds nothing); the
    result is bit-symmetric and positive definite; a frame's marginal is no smaller than its conditional covariance: Z_tt -
    N_t^T N_t is positive semi-definite, and zero for the last frame."""
    T = 4
    A, E, F = cref.equations(kind, 2, T, seed=811)
    mu = cref._np(cref.random_stiffness(3))
    for s in range(2):
        a, e, f = seq((A, E, F), s, T)
        Z, bad = cref.selected(a, e, f, mu)
        assert bad is None and np.array_equal(Z, Z.transpose(0, 2, 1))
        for t in range(T):
            assert np.linalg.eigvalsh(Z[t]).min() > 0
        zero = cref.selected(a, np.zeros_like(a), np.zeros_like(a), mu)[0]
        for t in range(T):
            assert np.array_equal(zero[t], cref.selected(a[t:t + 1], None, None, mu)[0][0])
        assert np.array_equal(zero, cref.selected(a, None, None, mu)[0])
        assert np.array_equal(cref.selected(a, e, np.zeros_like(a), mu)[0], cref.selected(a, e, None, mu)[0])
        cond = cref.selected(a, e, f, mu, variant="conditional")[0]
        for t in range(T - 1):
            assert np.linalg.eigvalsh(Z[t] - cond[t]).min() > -1e-12 * np.abs(Z[t]).max()
        assert np.array_equal(Z[T - 1], cond[T - 1])                       # the last frame's N^T N is its marginal


def test_marginal_over_a_sphere_is_the_dense_projection():
    """C_j = Jc_j Z_tt Jc_j^T in the header's order against the matmul of the dense inverse's block: per entry within
    |Jc_a|_1 |Jc_b|_1 (|restatement - dense| + 2 x 52 eps max |Z|) -- the projection is linear in Z, and two orders of a
    26 x 26 double sum differ by at most 52 eps of the absolute sum each."""
    for kind, T, J in (("seq", 3, 41), ("seq2", 5, 64), ("seq2", 1, 1)):
        eqs = cref.equations(kind, 2, T, seed=820 + T)
        jac = cref.jacobian(2 * T, J)
        want = cref.reference(*eqs, T, cref.random_stiffness(4), jac)
        assert not want["status"].any()
        q = np.abs(jac.double().numpy()).reshape(2 * T, J, 3, 26).sum(-1)
        for b in range(2 * T):
            s = b // T
            bound = np.stack([q[b, :, a] * q[b, :, c] for a, c in cref.PAIRS], 1) * (want["gap"][s] + 104 * EPS * want["size"][s])
            assert (np.abs(want["sphere_cov"][b] - want["dense_sphere"][b]) <= bound).all()
        C = cref.expand(want["sphere_cov"])
        assert np.array_equal(C, C.swapaxes(-1, -2)) and np.linalg.eigvalsh(C).min() > 0


def _as_got(want):
    return want["cov"].copy(), None if want["sphere_cov"] is None else want["sphere_cov"].copy(), want["status"].copy()


@pytest.mark.parametrize("kind", cref.KINDS)
@pytest.mark.parametrize("T", (1, 2, 3, 5))
def test_comparator_tells_wrong_variants(kind, T):
    """The comparator passes the restatement and the dense inverse, and names every wrong variant on every shape it applies
    to: the conditional covariance N^T N alone (T >= 2), the V terms dropped (seq2, T >= 3), E untransposed (T >= 2), the
    damped matrix (lambda = 1e-3) inverted, one entry off by 1e-3 of itself (which also breaks the symmetry), a wrong status,
    a missing sphere_cov, and a failed sequence that poisons only its own frame (T >= 2)."""
    S = 2
    eqs = cref.equations(kind, S, T, seed=840 + T)
    mu, jac = cref.random_stiffness(6), cref.jacobian(S * T, 41)
    want = cref.reference(*eqs, T, mu, jac)
    out = {}
    assert cref.compare(_as_got(want), want, out) == [] and out["exact"] == out["live"] == S
    mirrored = np.tril(want["dense_cov"]) + np.tril(want["dense_cov"], -1).transpose(0, 2, 1)     # (numpy's inverse is not bit-symmetric)
    assert cref.compare((mirrored, want["dense_sphere"], want["status"]), want) == []
    assert cref.compare((want["cov"], cref.expand(want["sphere_cov"]), want["status"]), want) == []      # the 3 x 3 form
    wrong = {}
    if T >= 2:
        wrong["conditional"] = cref.reference(*eqs, T, mu, jac, variant="conditional")
        wrong["E untransposed"] = cref.reference(eqs[0], eqs[1].transpose(1, 2).contiguous(), eqs[2], T, mu, jac)
    if kind == "seq2" and T >= 3:
        wrong["V dropped"] = cref.reference(*eqs, T, mu, jac, variant="no_v")
    wrong["damped"] = cref.reference(*eqs, T, mu, jac, lam=1e-3)
    for name, w in wrong.items():
        bad = cref.compare(_as_got(w), want)
        assert len(bad) >= S and all("off by" in b for b in bad), (name, bad)        # every sequence is named
    got = _as_got(want)
    got[0][0, 3, 5] *= 1.0 + 1e-3
    assert any("off by" in b or "symmetric" in b for b in cref.compare(got, want))
    got = _as_got(want)
    got[2][1] = 1
    assert any("status" in b for b in cref.compare(got, want))
    assert cref.compare((want["cov"], None, want["status"]), want) != []
    if T >= 2:
        for second in ((False, True) if kind == "seq2" and T >= 3 else (False,)):
            t = T - 1
            broken = cref.broken(kind, eqs, T, 1, t, second)
            w = cref.reference(*broken, T, mu, jac)
            assert w["status"].tolist() == [0, 1 + t]
            assert cref.compare(_as_got(w), w) == []
            got = _as_got(want)                                    # the good batch's values, NaN at the failing frame alone
            got[0][T + t], got[1][T + t], got[2][1] = np.nan, np.nan, 1 + t
            bad = cref.compare(got, w)
            assert bad and all("no NaN" in b for b in bad), bad
            assert any("status" in b for b in cref.compare(_as_got(want), w))


@pytest.mark.parametrize("kind", cref.KINDS)
def test_a_broken_coupling_fails_at_its_frame(kind):
    """lm_scripts_ref.break_coupling with factor 3 at lambda = 0 and the default own rows: the middle sequence fails exactly
    at frame t for every t >= 1 through E and every t >= 2 through F, the restated recurrences (first_bad_pivot) name that
    frame, and the other sequences factorise.  These are the GPU tests' pivot cases."""
    T = cref.PIVOT_T
    cases = [c for c in cref.pivot_cases() if c[1] == kind]
    assert len(cases) == (T - 1) + ((T - 2) if kind == "seq2" else 0)
    mu = cref.random_stiffness(5)
    for name, _, bad_eqs, good_eqs, t in cases:
        want = cref.reference(*bad_eqs, T, mu)
        assert want["status"].tolist() == [0, 1 + t, 0], name
        assert lref.first_bad_pivot(kind, cref.unit(bad_eqs, 1, T), 0.0, mu.double().numpy())[0] == t, name
        assert lref.first_bad_pivot(kind, cref.unit(good_eqs, 1, T), 0.0, mu.double().numpy()) is None
        assert np.isnan(want["cov"][T:2 * T]).all() and not np.isnan(want["cov"][:T]).any()
        good = cref.reference(*good_eqs, T, mu)
        assert not good["status"].any()
        for s in (0, 2):
            assert np.array_equal(want["cov"][s * T:s * T + T], good["cov"][s * T:s * T + T])


def test_gpu_cases_are_what_they_say():
    """The inputs of the GPU tests: every shape case, long chain and conditioning case factorises at lambda = 0 (a dense
    Cholesky agrees), the conditioning cases are the sweep's factorisable ones for both kinds, and the long chains' last
    sequence repeats the first."""
    cond = cref.conditioning_cases()
    assert len(cond) >= 24 and {c[1] for c in cond} == set(cref.KINDS)
    assert any("weight=10000" in c[0] and "own=0" in c[0] for c in cond) and any("own=6" in c[0] for c in cond)
    for name, kind, T, eqs, mu, J in cref.shape_cases() + cond:
        S = eqs[0].shape[0] // T
        for s in range(S):
            a, e, f = seq(eqs, s, T)
            assert cref.factor(a, e, f, cref._np(mu))[3] is None, (name, s)
            np.linalg.cholesky(cref.dense_matrix(a, e, f, cref._np(mu)))
    shapes = [(T, J) for _, _, T, _, _, J in cref.shape_cases()]
    assert {t for t, _ in shapes} == {1, 2, 3, 4, 6} and {j for _, j in shapes} == {1, 41, 64}
    for name, kind, T, eqs, mu, J in cref.long_cases():
        assert all(X is None or torch.equal(X[-T:], X[:T]) for X in eqs), name
    assert sorted((e[0].shape[0] // T, T) for _, _, T, e, _, _ in cref.long_cases()) == [(2, 64), (65, 2), (65, 2)]


def test_study_singles_out_the_hidden_finger():
    """What DESIGN.md 4.4y's study shows, on one sequence and three iterations (seconds): in the `blind` family the hidden
    finger's sigma in its hidden frames is more than four times the other spheres' there and more than four times its own in
    the visible frames; the temporal coupling does not reach those frames (the sequence's marginal and the frame's own are
    within 1 %: acc_max cuts the term exactly there); and sigma is NOT a bound -- the finger is further off than it, in
    another basin."""
    from spherehand_amd import hand_model
    rows = cref.study(hand_model.load_mesh(), S=1, iters=3, families=("blind",), out=lambda s: None)
    by = {r["name"]: r for r in rows}
    assert set(by) == {"traj", "cut", "frames"}
    for r in rows:
        assert r["hidden"] > 4.0 * r["others"] and r["hidden"] > 4.0 * r["visible"], r
        assert r["hidden_error"] > r["hidden"], r
        assert r["rank"] > 0.0, r
    assert abs(by["traj"]["hidden"] - by["cut"]["hidden"]) < 0.01 * by["traj"]["hidden"]
