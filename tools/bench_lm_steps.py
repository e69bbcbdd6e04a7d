"""The Levenberg-Marquardt step entries of THIS build beside the PARENT commit's library (--parent-lib), loaded in one process:
what a change that restates their shared text (lm_solve.h, lm_state.h, lm_band.h) must not slow down.  HIP events on the
launching stream, through the C ABI (no Python op in the loop), every entry with the solve:
  lm_step      shr_pose_lm_step, 256 crops: one wave per crop
  seq_step     shr_pose_lm_seq_step: one wave per sequence, a latency chain of its frames
  seq2_step    shr_pose_lm_seq2_step with F
  seq2_no_F    the same entry with F = NULL, which hands the call to shr_pose_lm_seq_step
  shared_step  shr_pose_lm_shared_step at K = 41: four launches, parallel over the frames
the sequence and shared steps for 256 frames as 32 units of 8 frames and as 8 units of 32 (tools/bench_sphere_trajectory.py's
and tools/bench_sphere_radii.py's shapes).  The equations are synthetic: seeded, well-conditioned SPD diagonal blocks with
small E, F and C, so that no pivot fails; the kernels' loops do not depend on the values.  Each library begins its own
states; the first step of a state accepts, every later one evaluates the same trial again and rejects, in both libraries
alike.  Every shape is run from both libraries before anything is timed, and trial_out of the same step of both is
compared bit for bit; then alternated, three rounds, the odd ones in
reverse order (every round is printed; the summary is the median, the spread is max - min over the rounds).  The condition,
per entry and shape: this build's median is not above the parent library's by more than the run-to-run spread (the larger
of the two); the tool exits with status 1 where it is missed, and says so where no parent library was given (status 0:
nothing to hold)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spherehand_amd import _lib  # noqa: E402

ROUNDS = 3
B, K = 256, 41
ENTRIES = ("shr_pose_lm_state_bytes", "shr_pose_lm_begin", "shr_pose_lm_step", "shr_pose_lm_seq_state_bytes",
           "shr_pose_lm_seq_workspace_bytes", "shr_pose_lm_seq_begin", "shr_pose_lm_seq_step", "shr_pose_lm_seq2_state_bytes",
           "shr_pose_lm_seq2_workspace_bytes", "shr_pose_lm_seq2_begin", "shr_pose_lm_seq2_step",
           "shr_pose_lm_shared_state_bytes", "shr_pose_lm_shared_workspace_bytes", "shr_pose_lm_shared_begin",
           "shr_pose_lm_shared_step")


def load_parent(path):
    """The parent commit's library beside this build's: its own handle, the entries' signatures set from this loader's (the
    ABI is the same)."""
    h = ctypes.CDLL(os.path.abspath(path))
    for name in ENTRIES:
        getattr(h, name).argtypes, getattr(h, name).restype = _lib.SIGNATURES[name]
    return h


def equations(gen):
    """Seeded stand-ins for a fit's equations: A = M M^T / 26 + I per frame, E, F and C of entries ~ 0.05, R = M M^T / K + I
    per group (sized for the smaller grouping), g, gs and positive costs."""
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    M, Ms = rnd(B, 26, 26), rnd(B // 8, K, K)
    eq = dict(A=M @ M.transpose(1, 2) / 26 + torch.eye(26, dtype=torch.float64), g=rnd(B, 26), E=0.05 * rnd(B, 26, 26),
              F=0.05 * rnd(B, 26, 26), C=0.05 * rnd(B, 26, K), R=Ms @ Ms.transpose(1, 2) / K + torch.eye(K, dtype=torch.float64),
              gs=rnd(B // 8, K), cost=rnd(B).abs() + 1.0)
    eq = {k: v.contiguous().cuda() for k, v in eq.items()}
    eq["start"] = (0.1 * torch.randn(B, 26, generator=gen)).cuda()
    eq["shape0"] = (10.0 + torch.rand(B // 8, K, generator=gen)).cuda()
    eq["mu"] = torch.tensor([1.0] * 3 + [0.0] * 3 + [1.0] * 20).cuda()
    eq["nu"] = torch.full((K,), 0.5).cuda()
    return eq


def runs_of(h, eq, s0):
    """{label: fn(stream)} of one library: its own states (begun here), trials, outputs and workspaces."""
    p = lambda t: t.data_ptr()  # noqa: E731
    f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    f64 = lambda n: torch.empty(max(1, n // 8), dtype=torch.float64, device="cuda")  # noqa: E731
    A, g, E, F, C, R, gs, cost, start, mu, nu = (eq[k] for k in ("A", "g", "E", "F", "C", "R", "gs", "cost", "start", "mu", "nu"))
    nxt, par, cst, cst0 = f32(B, 26), f32(B, 26), f32(B), f32(B)
    keep = [nxt, par, cst, cst0]                                   # (the closures below hold raw addresses)
    runs = {}
    state, trial = f64(h.shr_pose_lm_state_bytes(B)), f32(B, 26)
    assert h.shr_pose_lm_begin(p(start), B, 1e-3, p(state), p(trial), s0) == 0
    keep += [state, trial]
    runs["lm_step %d" % B] = lambda s, st=state, tr=trial: h.shr_pose_lm_step(
        p(st), p(A), p(g), p(cost), p(tr), None, p(mu), 1, B, p(nxt), p(par), p(cst), p(cst0), s)
    for T in (8, 32):
        G = B // T
        shape = "%dx%d" % (G, T)
        for label, name, Fp in (("seq_step", "seq", ()), ("seq2_step", "seq2", (p(F),)), ("seq2_no_F", "seq2", (None,))):
            state = f64(getattr(h, "shr_pose_lm_%s_state_bytes" % name)(B))
            ws, trial = f64(getattr(h, "shr_pose_lm_%s_workspace_bytes" % name)(B)), f32(B, 26)
            assert getattr(h, "shr_pose_lm_%s_begin" % name)(p(start), B, T, 1e-3, p(state), p(trial), s0) == 0
            keep += [state, ws, trial]
            step = getattr(h, "shr_pose_lm_%s_step" % name)
            runs["%s %s" % (label, shape)] = lambda s, step=step, st=state, tr=trial, w=ws, T=T, Fp=Fp: step(
                p(st), p(A), p(g), p(E), *Fp, p(cost), p(tr), None, p(mu), 1, B, T, p(nxt), p(par), p(cst), p(cst0), p(w), s)
        state, ws = f64(h.shr_pose_lm_shared_state_bytes(B, G, K)), f64(h.shr_pose_lm_shared_workspace_bytes(B, G, K))
        trial, trial_shape, nxt_shape, shp = f32(B, 26), f32(G, K), f32(G, K), f32(G, K)
        assert h.shr_pose_lm_shared_begin(p(start), p(eq["shape0"]), B, T, K, 1e-3, p(state), p(trial), p(trial_shape), s0) == 0
        keep += [state, ws, trial, trial_shape, nxt_shape, shp]
        runs["shared_step %s" % shape] = lambda s, st=state, tr=trial, ts=trial_shape, w=ws, T=T, ns=nxt_shape, sh=shp: \
            h.shr_pose_lm_shared_step(p(st), p(A), p(g), p(C), p(R), p(gs), p(cost), p(tr), p(ts), None, p(mu), None, p(nu), 1, B, T,
                                      K, p(nxt), p(ns), p(par), p(sh), p(cst), p(cst0), p(w), s)
    return runs, keep


def main(parent_lib=None):
    lib = _lib.lib()
    parent = load_parent(parent_lib) if parent_lib else None
    if parent is None:
        print("no --parent-lib: the steps are not held against the parent commit's library", flush=True)
    stream = torch.cuda.Stream()
    within = True
    with torch.cuda.stream(stream):
        eq = equations(torch.Generator().manual_seed(B + K))
        s0 = stream.cuda_stream
        this, keep = runs_of(lib, eq, s0)
        runs = {(k, "this"): fn for k, fn in this.items()}
        if parent is not None:
            theirs, kept = runs_of(parent, eq, s0)
            keep += kept
            runs = {(k, who): fn for k in this for who, fn in (("this", this[k]), ("parent", theirs[k]))}
        for key, fn in runs.items():                               # every shape from both libraries before anything is timed
            for _ in range(3):
                assert fn(s0) == 0, key
        stream.synchronize()
        if parent is not None:                                     # the same step of the same state: the same bits of trial_out
            for k in this:
                steps = []
                for fn, nxt in ((this[k], keep[0]), (theirs[k], kept[0])):
                    assert fn(s0) == 0, k
                    stream.synchronize()
                    steps.append(nxt.clone().view(torch.int32))
                assert torch.equal(*steps), k
        us = {k: [] for k in runs}
        for rnd in range(ROUNDS):
            for key, fn in (list(runs.items()) if rnd % 2 == 0 else list(runs.items())[::-1]):      # (odd rounds in reverse order)
                us[key].append(bench.mean_launch_us(fn, stream, 20, 3, 5, warm_ms=20.0))
            print("  round %d: %s" % (rnd, " | ".join("%s/%s %.2f" % (k[0], k[1], v[-1]) for k, v in us.items())), flush=True)
        spread = {k: float(max(v) - min(v)) for k, v in us.items()}
        us = {k: float(np.median(v)) for k, v in us.items()}
        print("| entry and shape | this build, us | spread | parent, us | spread | difference | |\n|---|---|---|---|---|---|---|")
        for k in this:
            if parent is None:
                print("| %s | %.2f | %.2f | | | | |" % (k, us[k, "this"], spread[k, "this"]), flush=True)
                continue
            diff, bar = us[k, "this"] - us[k, "parent"], max(spread[k, "this"], spread[k, "parent"])
            within = within and diff <= bar
            print("| %s | %.2f | %.2f | %.2f | %.2f | %+.2f | %s the spread |"
                  % (k, us[k, "this"], spread[k, "this"], us[k, "parent"], spread[k, "parent"], diff,
                     "within" if diff <= bar else "SLOWER than"), flush=True)
    return within


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None, help="libspherehand_hip.so built from the parent commit")
    sys.exit(0 if main(ap.parse_args().parent_lib) else 1)
