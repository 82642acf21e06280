#!/usr/bin/env python
"""Time DirectSolver.log_probability_and_grad_batch (csrc/small.hip: one workgroup per member, value and gradient)
against the route a batch of small dense gradients had before it: a loop of
GaussianProcess(k_b, X, diag=d_b).log_probability_and_grad(y), one solver per member.

    python scripts/small_grad_timing.py [--sizes 32,128,192] [--dims 1,3] [--batch 1024] [--reps 9] [--loop-reps 3]

The method of scripts/small_batch_timing.py.  Per cell (N, D), in one process, the two routes alternating: two warm-ups
each, then wall times around calls that end in a device synchronise (both routes are blocking), fresh hyper-parameters
and noise per member and per call, the lowering and packing of the kernels and every host transfer included.
    batch_ms    the public call, median of `reps`
    grad_ms     tgp_small_logprob_grad alone on arrays packed beforehand: transfers, launch, join
    value_ms    tgp_small_logprob alone on the same arrays; grad_ms / value_ms is the device's price of the gradient
    loop_ms     the loop, every GP created inside it and its solver closed, median of `loop-reps`
One JSON line per cell, with the smallest loop sample, the spread of the batch samples, whether the batch keeps the
shape (its median at least 1.2 x better than the loop's: the repeats of one call spread by about that much on a host
that shares its CPUs) and the largest difference between the two routes' values and kernel gradients, relative to
max(1, |value|) resp. to the largest component.
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

KEEP = 1.2


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
                return solver.log_probability_and_grad_batch(ks, y, noise)

            def loop(call):
                ks, noise = inputs(call)
                out, grads = np.empty(B), []
                for b in range(B):
                    gp = GaussianProcess(ks[b], X, diag=noise[b])
                    out[b], g = gp.log_probability_and_grad(y)
                    grads.append(np.asarray(g["kernel"], dtype=np.float64))
                    gp.solver.close()
                return out, grads

            def grad_call(packed):
                return small.run_packed_grad(ctx, packed)[0]

            def value_call(packed):
                return small.run_packed(ctx, packed)[0]

            for call in (0, 1):
                batch(call)
                loop(call)
            batch_ms, loop_ms, grad_ms, value_ms, worst, worst_grad = [], [], [], [], 0.0, 0.0
            for i in range(max(args.reps, args.loop_reps)):
                call = i + 2
                if i < args.reps:
                    ms, (got, got_grads) = wall_ms(batch, call)
                    batch_ms.append(ms)
                    ks, noise = inputs(call)
                    lowered = [small.lower_member(k, X) for k in ks]
                    packed = small.pack_members([(low[0], low[1], noise[b], y) for b, low in enumerate(lowered)])
                    grad_ms.append(wall_ms(grad_call, packed)[0])
                    value_ms.append(wall_ms(value_call, packed)[0])
                if i < args.loop_reps:
                    ms, (want, want_grads) = wall_ms(loop, call)
                    loop_ms.append(ms)
                    if i < args.reps:
                        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
                        worst_grad = max(worst_grad, max(float(np.max(np.abs(a - w)) / np.max(np.abs(w)))
                                                         for a, w in zip(got_grads["kernel"], want_grads)))
            solver.close()
            speedup = float(np.median(loop_ms) / np.median(batch_ms))
            print(json.dumps({
                "n": n, "d": d, "batch": B, "batch_ms": round(float(np.median(batch_ms)), 3),
                "batch_min_ms": round(min(batch_ms), 3), "batch_max_ms": round(max(batch_ms), 3),
                "grad_ms": round(float(np.median(grad_ms)), 3), "value_ms": round(float(np.median(value_ms)), 3),
                "grad_over_value": round(float(np.median(grad_ms) / np.median(value_ms)), 2),
                "loop_ms": round(float(np.median(loop_ms)), 3), "loop_min_ms": round(min(loop_ms), 3),
                "speedup": round(speedup, 1), "keeps_the_shape": bool(speedup >= KEEP), "max_rel_diff": worst,
                "max_grad_diff": worst_grad}), flush=True)


if __name__ == "__main__":
    main()
