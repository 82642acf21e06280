#!/usr/bin/env python
"""Time QuasisepSeriesSet.value_and_grad against the route a set of series had before it: a loop of
QuasisepSolver.value_and_grad over solvers created beforehand, one per series.

    python scripts/quasisep_series_grad_timing.py [--sizes 10,14,16] [--batches 1,8,64] [--reps 9]

The method of scripts/quasisep_series_timing.py: fresh hyper-parameters per call (every member's differ too), host
transfers and the lowering of the kernels and of their tangents included, two warm-ups, then the median of `reps` wall
times with their spread.  The B lengths of a cell are drawn once (seed 0) within +-30 % of N = 2^size; every series has
coordinates, noise and data of its own.  Per cell, in one process:
    set_ms     one value_and_grad call on a resident QuasisepSeriesSet (vectors wanted)
    warm_ms    the loop over solvers created beforehand: B launch chains and their stream synchronisations
One JSON line per cell, with the smallest loop sample (the bar: set_ms below warm_min_ms) and whether the set's values,
kernel gradients, noise gradients and alphas are the loop's bit for bit.  For the per-kernel split of one cell run it
under `rocprofv3 --kernel-trace --stats -- python scripts/quasisep_series_grad_timing.py --sizes 14 --batches 64 --models
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
from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver  # noqa: E402

MODELS = {
    "matern32_J2": lambda s: q.Matern32(scale=2.0 * s),
    "m32xcos+sho_J6": lambda s: q.Matern32(scale=1.5 * s) * q.Cosine(scale=3.0) + q.SHO(omega=2.0 / s, quality=3.0),
    "celerite4_J8": lambda s: (q.Celerite(1.0, 0.2, 0.5 / s, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5 / s)
                               + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2 * s, 4.0)),
}


def samples_ms(fn, reps):
    fn(0)
    fn(1)
    samples = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(i + 2)
        samples.append(1e3 * (time.perf_counter() - t0))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="10,14,16")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--models", default=",".join(MODELS))
    args = ap.parse_args()
    for p in [int(v) for v in args.sizes.split(",")]:
        for nb in [int(v) for v in args.batches.split(",")]:
            rng = np.random.default_rng(0)
            lengths = rng.integers(int(0.7 * (1 << p)), int(1.3 * (1 << p)) + 1, nb)
            ts = [np.sort(rng.uniform(0, 0.05 * n, n)) for n in lengths]
            ys = [rng.standard_normal(n) for n in lengths]
            noises = [rng.uniform(0.05, 0.2, n) for n in lengths]
            for name in args.models.split(","):
                make = MODELS[name]

                def scale(i, b):
                    return 1.0 + 1e-3 * i + 1e-5 * b  # fresh per call, distinct per member

                series = QuasisepSeriesSet(ts, assume_sorted=True)
                warm = [QuasisepSolver(make(1.0), t, Diagonal(d), assume_sorted=True) for t, d in zip(ts, noises)]

                def as_set(i):
                    return series.value_and_grad([make(scale(i, b)) for b in range(nb)], ys, noises)

                def warm_loop(i):
                    out = []
                    for b, s in enumerate(warm):
                        # a new model on a live handle, as scripts/quasisep_grad_batch_timing.py does it: value_and_grad
                        # reads the model from `_ssm` and the tangents from `kernel`; `same` below would catch a solver
                        # that began to cache anything else
                        s.kernel = make(scale(i, b))
                        s._ssm = s.kernel._lower_ssm()
                        out.append(s.value_and_grad(ys[b]))
                    return out

                got, want = as_set(0), warm_loop(0)
                same = all(got[0][b] == v and np.array_equal(got[1]["kernel"][b], g["kernel"])
                           and np.array_equal(got[1]["noise_diag"][b], g["noise_diag"])
                           and np.array_equal(got[1]["mean"][b], g["mean"]) for b, (v, g) in enumerate(want))
                cell = {"n": 1 << p, "points": int(lengths.sum()), "kernel": name, "J": warm[0]._ssm.J,
                        "P": len(warm[0].kernel.parameters()), "B": nb}
                for key, fn in (("set", as_set), ("warm", warm_loop)):
                    s = samples_ms(fn, args.reps)
                    cell[key + "_ms"] = round(float(np.median(s)), 4)
                    cell[key + "_spread_ms"] = round(max(s) - min(s), 4)
                    cell[key + "_min_ms"] = round(min(s), 4)
                cell["warm_over_set"] = round(cell["warm_ms"] / cell["set_ms"], 3)
                cell["set_below_warm_min"] = bool(cell["set_ms"] < cell["warm_min_ms"])
                cell["bit_identical"] = bool(same)
                print(json.dumps(cell), flush=True)
                series.close()
                for s in warm:
                    s.close()


if __name__ == "__main__":
    main()
