#!/usr/bin/env python
"""Time QuasisepSolver.value_and_grad_batch against a loop of B value_and_grad calls on one solver.

    python scripts/quasisep_grad_batch_timing.py [--sizes 10,14,16,20] [--batches 1,8,64] [--reps 9] [--cell-seconds S]

The method of scripts/quasisep_batch_timing.py: fresh hyper-parameters per call (every member's differ too), host
transfers, the lowering of the kernels and of their tangents included, two warm-ups, then the median of `reps` wall
times with their spread (max - min) and the smallest sample.  Both sides run in the one process on the same solver, y
and noise (shared by the members); all kernel parameters plus the noise and mean vectors are differentiated.  One JSON
line per cell.  `--cell-seconds` bounds one side of a cell: where the first warm-up says that `reps` samples would take
longer, fewer are taken (at least 3) and the line says how many.  For the per-kernel split of one cell run it under
`rocprofv3 --kernel-trace --stats -- python scripts/quasisep_grad_batch_timing.py --sizes 14 --batches 64 --models
matern32_J2`.
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


def sample_ms(fn, reps, cell_seconds):
    """(median, spread, smallest, samples taken) after two warm-ups."""
    t0 = time.perf_counter()
    fn(0)
    first = time.perf_counter() - t0
    fn(1)
    if cell_seconds and first * (reps + 2) > cell_seconds:
        reps = max(3, min(reps, int(cell_seconds / first) - 2))
    samples = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(i + 2)
        samples.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(samples)), float(max(samples) - min(samples)), float(min(samples)), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="10,14,16,20")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--cell-seconds", type=float, default=0.0)
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
            npar = len(s.kernel.parameters())
            for nb in [int(v) for v in args.batches.split(",")]:
                def scale(i, b):
                    return 1.0 + 1e-3 * i + 1e-5 * b  # fresh per call, distinct per member

                def batch(i):
                    return s.value_and_grad_batch([make(scale(i, b)) for b in range(nb)], y)

                def loop(i):
                    out = []
                    for b in range(nb):
                        s.kernel = make(scale(i, b))
                        s._ssm = s.kernel._lower_ssm()
                        out.append(s.value_and_grad(y))
                    return out

                got, want = batch(0), loop(0)
                same = all(got[0][b] == v and np.array_equal(got[1]["kernel"][b], g["kernel"])
                           and np.array_equal(got[1]["noise_diag"][b], g["noise_diag"])
                           and np.array_equal(got[1]["mean"][b], g["mean"]) for b, (v, g) in enumerate(want))
                b_ms, b_spread, b_min, b_reps = sample_ms(batch, args.reps, args.cell_seconds)
                l_ms, l_spread, l_min, l_reps = sample_ms(loop, args.reps, args.cell_seconds)
                print(json.dumps({"n": n, "kernel": name, "J": s._ssm.J, "P": npar, "B": nb,
                                  "batch_ms": round(b_ms, 4), "batch_spread_ms": round(b_spread, 4),
                                  "batch_reps": b_reps, "loop_ms": round(l_ms, 4),
                                  "loop_spread_ms": round(l_spread, 4), "loop_min_ms": round(l_min, 4),
                                  "loop_reps": l_reps, "ratio": round(l_ms / b_ms, 3),
                                  "batch_below_loop_min": bool(b_ms < l_min), "bit_identical": same}), flush=True)
            s.close()


if __name__ == "__main__":
    main()
