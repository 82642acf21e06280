#!/usr/bin/env python
"""Time QuasisepSolver.log_probability_batch against a loop of B log_probability calls on one solver.

    python scripts/quasisep_batch_timing.py [--sizes 10,14,16,20] [--batches 1,8,64,256] [--reps 9]

The method of scripts/quasisep_timing.py: fresh hyper-parameters per call (every member's differ too), host transfers
and the lowering of the kernels included, two warm-ups, then the median of `reps` wall times.  Both sides run in the one
process on the same solver, y and noise (shared by the members).  One JSON line per cell: batch and loop time in ms and
their ratio.  For the per-kernel split of one cell run it under
`rocprofv3 --kernel-trace --stats -- python scripts/quasisep_batch_timing.py --sizes 14 --batches 64 --models matern32_J2`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tinygp_amd.kernels import quasisep as q  # noqa: E402
from tinygp_amd.noise import Diagonal  # noqa: E402
from tinygp_amd.solvers import QuasisepSolver  # noqa: E402

MODELS = {
    "matern32_J2": lambda s: q.Matern32(scale=2.0 * s),
    "m32xcos+sho_J6": lambda s: q.Matern32(scale=1.5 * s) * q.Cosine(scale=3.0) + q.SHO(omega=2.0 / s, quality=3.0),
    "celerite4_J8": lambda s: (q.Celerite(1.0, 0.2, 0.5 / s, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5 / s)
                               + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2 * s, 4.0)),
}


def median_ms(fn, reps):
    fn(0)
    fn(1)
    samples = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(i + 2)
        samples.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(samples)), float(max(samples) - min(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="10,14,16,20")
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--models", default=",".join(MODELS))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    for p in [int(v) for v in args.sizes.split(",")]:
        n = 1 << p
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        y = rng.standard_normal(n)
        noise = np.full(n, 0.1)
        for name in args.models.split(","):
            make = MODELS[name]
            s = QuasisepSolver(make(1.0), t, Diagonal(noise), assume_sorted=True)
            for nb in [int(v) for v in args.batches.split(",")]:
                def scale(i, b):
                    return 1.0 + 1e-3 * i + 1e-5 * b  # fresh per call, distinct per member

                def batch(i):
                    return s.log_probability_batch([make(scale(i, b)) for b in range(nb)], y)

                def loop(i):
                    out = np.empty(nb)
                    for b in range(nb):
                        s._ssm = make(scale(i, b))._lower_ssm()
                        out[b] = s.log_probability(y)
                    return out

                same = bool(np.all(batch(0) == loop(0)))
                b_ms, b_spread = median_ms(batch, args.reps)
                l_ms, l_spread = median_ms(loop, args.reps)
                print(json.dumps({"n": n, "kernel": name, "J": s._ssm.J, "B": nb, "batch_ms": round(b_ms, 4),
                                  "batch_spread_ms": round(b_spread, 4), "loop_ms": round(l_ms, 4),
                                  "loop_spread_ms": round(l_spread, 4), "ratio": round(l_ms / b_ms, 3),
                                  "bit_identical": same}), flush=True)
            s.close()


if __name__ == "__main__":
    main()
