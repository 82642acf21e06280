#!/usr/bin/env python
"""Time DirectSolver.log_probability_batch (csrc/small.hip: one workgroup per member) against the route a batch of
small dense GPs had before it: a loop of GaussianProcess(k_b, X, diag=d_b).log_probability(y), one solver per member.

    python scripts/small_batch_timing.py [--sizes 32,128,192] [--dims 1,3] [--batch 1024] [--reps 9] [--loop-reps 3]

Per cell (N, D), in one process, the two routes alternating: two warm-ups each, then wall times around calls that end
in a device synchronise (both routes are blocking), fresh hyper-parameters and noise per member and per call, the
lowering and packing of the kernels and every host transfer included.
    batch_ms    the public call, median of `reps`
    packed_ms   tgp_small_logprob alone on arrays packed beforehand: transfers, launch, join
    loop_ms     the loop, every GP created inside it and its solver closed, median of `loop-reps`
One JSON line per cell, with the smallest loop sample, the spread of the batch samples and the largest difference
between the two routes' values relative to max(1, |value|).  For the kernel's own time run one cell under
`rocprofv3 --kernel-trace --stats -- python scripts/small_batch_timing.py --sizes 128 --dims 3 --loop-reps 1`.
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-reps", type=int, default=3)
    args = ap.parse_args()
    B = args.batch
    ctx = _ffi.default_ctx()
    for n in [int(v) for v in args.sizes.split(",")]:
        for d in [int(v) for v in args.dims.split(",")]:
            rng = np.random.default_rng([n, d])
            X = np.sort(rng.uniform(0.0, 4.0, n)) if d == 1 else rng.uniform(0.0, 3.0, (n, d))
            y = rng.standard_normal(n)
            base = rng.uniform(0.05, 0.15, n)
            solver = DirectSolver(member_kernel(d, 1.0), X, Diagonal(base))

            def inputs(call):
                scales = 1.0 + 0.5 * np.random.default_rng([call, n, d]).uniform(size=B)
                return [member_kernel(d, s) for s in scales], base[None, :] * scales[:, None]

            def batch(call):
                ks, noise = inputs(call)
                return solver.log_probability_batch(ks, y, noise)

            def loop(call):
                ks, noise = inputs(call)
                out = np.empty(B)
                for b in range(B):
                    gp = GaussianProcess(ks[b], X, diag=noise[b])
                    out[b] = gp.log_probability(y)
                    gp.solver.close()
                return out

            def packed_call(packed):
                return small.run_packed(ctx, packed)[0]

            for call in (0, 1):
                batch(call)
                loop(call)
            batch_ms, loop_ms, packed_ms, worst = [], [], [], 0.0
            for i in range(max(args.reps, args.loop_reps)):
                call = i + 2
                if i < args.reps:
                    ms, got = wall_ms(batch, call)
                    batch_ms.append(ms)
                    ks, noise = inputs(call)
                    lowered = [small.lower_member(k, X) for k in ks]
                    packed = small.pack_members([(low[0], low[1], noise[b], y) for b, low in enumerate(lowered)])
                    packed_ms.append(wall_ms(packed_call, packed)[0])
                if i < args.loop_reps:
                    ms, want = wall_ms(loop, call)
                    loop_ms.append(ms)
                    if i < args.reps:
                        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
            solver.close()
            print(json.dumps({
                "n": n, "d": d, "batch": B, "batch_ms": round(float(np.median(batch_ms)), 3),
                "batch_min_ms": round(min(batch_ms), 3), "batch_max_ms": round(max(batch_ms), 3),
                "packed_ms": round(float(np.median(packed_ms)), 3), "loop_ms": round(float(np.median(loop_ms)), 3),
                "loop_min_ms": round(min(loop_ms), 3), "speedup": round(float(np.median(loop_ms) / np.median(batch_ms)), 1),
                "max_rel_diff": worst}), flush=True)


if __name__ == "__main__":
    main()
