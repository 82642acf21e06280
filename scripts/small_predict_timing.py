#!/usr/bin/env python
"""Time DirectSolver.predict_batch (csrc/small.hip: one workgroup per member and per chunk of test points) against the
route a batch of small dense GPs had before it: a loop of GaussianProcess(k_b, X, diag=d_b).predict(y, Xt,
return_var=True), one solver per member, each closed behind it.

    python scripts/small_predict_timing.py [--sizes 32,128,192] [--dims 1,3] [--tests 16,n,1024] [--batch 1024]
                                           [--reps 9] [--loop-reps 3] [--packed-only]

Per cell (N, D, M), in one process, the two routes alternating: two warm-ups each, then wall times around calls that
end in a device synchronise (both routes are blocking), fresh hyper-parameters and noise per member and per call, the
lowering and packing of the kernels and every host transfer included.  `n` in --tests stands for M = N.
    batch_ms    the public call, median of `reps`, with its smallest and largest sample
    packed_ms   tgp_small_predict alone on arrays packed beforehand: transfers, launch, join
    loop_ms     the loop, every GP created inside it and its solver closed, median of `loop-reps`
One JSON line per cell, with the largest difference between the two routes' means and variances relative to
max(1, |want|).  --packed-only times the C call alone (to compare builds of the library through TGP_HIP_LIBRARY, or
under a profiler).  For the kernel's own time run under
`rocprofv3 --kernel-trace --stats -- python scripts/small_predict_timing.py --packed-only --reps 3`.
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


def member_kernel(d, s):
    if d == 1:
        return (1.3 * s) * kernels.ExpSquared(1.5 * s)
    return (0.9 * s) * kernels.Matern32(1.5 * s, distance=kernels.L2Distance())


def wall_ms(fn, arg):
    t0 = time.perf_counter()
    out = fn(arg)
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"32,128,{small.MAX_N}")
    ap.add_argument("--dims", default="1,3")
    ap.add_argument("--tests", default="16,n,1024")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--packed-only", action="store_true")
    args = ap.parse_args()
    B = args.batch
    ctx = _ffi.default_ctx()
    for n in [int(v) for v in args.sizes.split(",")]:
        for d in [int(v) for v in args.dims.split(",")]:
            for m in [n if v == "n" else int(v) for v in args.tests.split(",")]:
                rng = np.random.default_rng([n, d, m])
                X = np.sort(rng.uniform(0.0, 4.0, n)) if d == 1 else rng.uniform(0.0, 3.0, (n, d))
                Xt = rng.uniform(0.0, 4.0, m) if d == 1 else rng.uniform(0.0, 3.0, (m, d))
                y = rng.standard_normal(n)
                base = rng.uniform(0.05, 0.15, n)
                solver = DirectSolver(member_kernel(d, 1.0), X, Diagonal(base))

                def inputs(call):
                    scales = 1.0 + 0.5 * np.random.default_rng([call, n, d]).uniform(size=B)
                    return [member_kernel(d, s) for s in scales], base[None, :] * scales[:, None]

                def batch(call):
                    ks, noise = inputs(call)
                    return solver.predict_batch(ks, y, Xt, noise)

                def loop(call):
                    ks, noise = inputs(call)
                    mu, var = np.empty((B, m)), np.empty((B, m))
                    for b in range(B):
                        gp = GaussianProcess(ks[b], X, diag=noise[b])
                        mu[b], var[b] = gp.predict(y, Xt, return_var=True)
                        gp.solver.close()
                    return mu, var

                def pack(call):
                    ks, noise = inputs(call)
                    lowered = [small.lower_member(k, X) for k in ks]
                    tests = [small.lower_test(k, None, X, Xt, low)[0] for k, low in zip(ks, lowered)]
                    return small.pack_predict([(low[0], low[1], noise[b], y) for b, low in enumerate(lowered)], tests)

                def packed_call(pp):
                    return small.run_packed_predict(ctx, pp)

                batch_ms, loop_ms, packed_ms, worst = [], [], [], 0.0
                if args.packed_only:
                    for call in range(args.reps + 2):
                        ms = wall_ms(packed_call, pack(call))[0]
                        if call >= 2:
                            packed_ms.append(ms)
                    solver.close()
                    print(json.dumps({"n": n, "d": d, "m": m, "batch": B,
                                      "packed_ms": round(float(np.median(packed_ms)), 3),
                                      "packed_min_ms": round(min(packed_ms), 3),
                                      "packed_max_ms": round(max(packed_ms), 3)}), flush=True)
                    continue
                for call in (0, 1):
                    batch(call)
                    loop(call)
                jitter = small.jitter(np.float64)
                for i in range(max(args.reps, args.loop_reps)):
                    call = i + 2
                    if i < args.reps:
                        ms, got = wall_ms(batch, call)
                        batch_ms.append(ms)
                        packed_ms.append(wall_ms(packed_call, pack(call))[0])
                    if i < args.loop_reps:
                        ms, want = wall_ms(loop, call)
                        loop_ms.append(ms)
                        if i < args.reps:
                            for g, w in ((got[1], want[0]), (got[2] + jitter, want[1])):
                                worst = max(worst, float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w)))))
                solver.close()
                print(json.dumps({
                    "n": n, "d": d, "m": m, "batch": B, "batch_ms": round(float(np.median(batch_ms)), 3),
                    "batch_min_ms": round(min(batch_ms), 3), "batch_max_ms": round(max(batch_ms), 3),
                    "packed_ms": round(float(np.median(packed_ms)), 3), "loop_ms": round(float(np.median(loop_ms)), 3),
                    "loop_min_ms": round(min(loop_ms), 3),
                    "speedup": round(float(np.median(loop_ms) / np.median(batch_ms)), 1), "max_rel_diff": worst}), flush=True)


if __name__ == "__main__":
    main()
