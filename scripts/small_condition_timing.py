#!/usr/bin/env python
"""Time DirectSolver.condition_batch (csrc/small.hip: one workgroup per member, the test points as further columns of
the member's matrix) against the route a batch of small dense GPs had before it: a loop of
GaussianProcess(k_b, X, diag=d_b).condition(y, Xt, diag=tau), reading .gp.covariance and, for draws, .gp.sample, one
solver per member (two with draws), each closed behind it.

    python scripts/small_condition_timing.py [--shapes 32x16,96x96,128x64,64x128] [--dims 1,3] [--draws 0,1,16]
                                             [--batch 1024] [--reps 9] [--loop-reps 3] [--packed-only]

Per cell (N, M, D, S), in one process, the routes alternating: two warm-ups each, then wall times around calls that end
in a device synchronise (all routes are blocking), fresh hyper-parameters and noise per member and per call, the
lowering and packing of the kernels and every host transfer included.
    batch_ms / batch_nocov_ms    the public call with and without the covariances returned (S = 0 without them is the
                                 value and the mean alone), median of `reps`
    packed_ms / packed_nocov_ms  tgp_small_condition alone on arrays packed beforehand: transfers, launch, join
    loop_ms                      the loop, every GP created inside it and its solvers closed, median of `loop-reps`
One JSON line per cell, with the largest difference between the two routes' means and covariances relative to
max(1, |want|).  --packed-only times the C call alone (to compare builds of the library through TGP_HIP_LIBRARY, or
under a profiler).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tinygp_amd import GaussianProcess, _ffi, kernels  # noqa: E402
from tinygp_amd.noise import Diagonal  # noqa: E402
from tinygp_amd.solvers import DirectSolver, small  # noqa: E402

TAU = 0.1


def member_kernel(d, s):
    if d == 1:
        return (1.3 * s) * kernels.ExpSquared(1.5 * s)
    return (0.9 * s) * kernels.Matern32(1.5 * s, distance=kernels.L2Distance())


def wall_ms(fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    return 1e3 * (time.perf_counter() - t0), out


def med(v):
    return round(float(np.median(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x16,96x96,128x64,64x128")
    ap.add_argument("--dims", default="1,3")
    ap.add_argument("--draws", default="0,1,16")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--packed-only", action="store_true")
    args = ap.parse_args()
    B = args.batch
    ctx = _ffi.default_ctx()
    for n, m in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        for d in [int(v) for v in args.dims.split(",")]:
            for S in [int(v) for v in args.draws.split(",")]:
                rng = np.random.default_rng([n, d, m])
                X = np.sort(rng.uniform(0.0, 4.0, n)) if d == 1 else rng.uniform(0.0, 3.0, (n, d))
                Xt = rng.uniform(0.0, 4.0, m) if d == 1 else rng.uniform(0.0, 3.0, (m, d))
                y = rng.standard_normal(n)
                base = rng.uniform(0.05, 0.15, n)
                xi = rng.standard_normal((S, m)) if S else None
                solver = DirectSolver(member_kernel(d, 1.0), X, Diagonal(base))

                def inputs(call):
                    scales = 1.0 + 0.5 * np.random.default_rng([call, n, d]).uniform(size=B)
                    return [member_kernel(d, s) for s in scales], base[None, :] * scales[:, None]

                def batch(call, cov):
                    ks, noise = inputs(call)
                    return solver.condition_batch(ks, y, Xt, noise, test_diag=TAU, xi=xi, return_cov=cov)

                def loop(call):
                    ks, noise = inputs(call)
                    mu, cov = np.empty((B, m)), np.empty((B, m, m))
                    for b in range(B):
                        gp = GaussianProcess(ks[b], X, diag=noise[b])
                        cond = gp.condition(y, Xt, diag=TAU).gp
                        mu[b], cov[b] = cond.loc, cond.covariance
                        if S:
                            cond.sample(b, shape=(S,))
                            cond.solver.close()
                        gp.solver.close()
                    return mu, cov

                def pack(call):
                    ks, noise = inputs(call)
                    lowered = [small.lower_member(k, X) for k in ks]
                    tests = [small.lower_test(k, None, X, Xt, low)[0] for k, low in zip(ks, lowered)]
                    return small.pack_condition([(low[0], low[1], noise[b], y) for b, low in enumerate(lowered)], tests,
                                                [np.full(m, TAU)] * B, None, [xi] * B)

                t = dict(batch=[], nocov=[], packed=[], packed_nocov=[], loop=[])
                worst = 0.0
                if not args.packed_only:
                    for call in (0, 1):
                        batch(call, True), batch(call, False), loop(call)
                else:
                    for call in (0, 1):
                        small.run_packed_condition(ctx, pack(call), True)
                for i in range(max(args.reps, 0 if args.packed_only else args.loop_reps)):
                    call = i + 2
                    if i < args.reps:
                        pc = pack(call)
                        t["packed"].append(wall_ms(small.run_packed_condition, ctx, pc, True)[0])
                        t["packed_nocov"].append(wall_ms(small.run_packed_condition, ctx, pc, False)[0])
                        if not args.packed_only:
                            ms, got = wall_ms(batch, call, True)
                            t["batch"].append(ms)
                            t["nocov"].append(wall_ms(batch, call, False)[0])
                    if not args.packed_only and i < args.loop_reps:
                        ms, want = wall_ms(loop, call)
                        t["loop"].append(ms)
                        if i < args.reps:
                            for g, w in ((got[1], want[0]), (got[2], want[1])):
                                worst = max(worst, float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w)))))
                solver.close()
                row = {"n": n, "m": m, "d": d, "draws": S, "batch": B, "packed_ms": med(t["packed"]),
                       "packed_nocov_ms": med(t["packed_nocov"])}
                if not args.packed_only:
                    row.update({"batch_ms": med(t["batch"]), "batch_min_ms": round(min(t["batch"]), 3),
                                "batch_max_ms": round(max(t["batch"]), 3), "batch_nocov_ms": med(t["nocov"]),
                                "loop_ms": med(t["loop"]), "loop_min_ms": round(min(t["loop"]), 3),
                                "speedup": round(float(np.median(t["loop"]) / np.median(t["batch"])), 1),
                                "speedup_nocov": round(float(np.median(t["loop"]) / np.median(t["nocov"])), 1),
                                "max_rel_diff": worst})
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
