#!/usr/bin/env python
"""Time QuasisepSeriesSet.predict against the route a set of series had before it: a loop that builds one QuasisepSolver
per series, calls predict_mean_var and closes it.

    python scripts/quasisep_series_predict_timing.py [--rows 64:16384:4096:matern32_J2,...] [--reps 9]

The method of scripts/quasisep_series_grad_timing.py: fresh hyper-parameters per call (every member's differ too), host
transfers and the lowering of the kernels included, two warm-ups, then the median of `reps` wall times with their
spread.  A row is B:N:M:model -- B series whose lengths are drawn once (seed 0) within +-30 % of N, every series with
coordinates, noise, data and M unsorted test points of its own (drawn from a little before its first datum to a little
after its last).  Per row, in one process:
    set_ms     one predict call on a resident QuasisepSeriesSet (value, means and variances)
    loop_ms    the loop over the series: a fresh QuasisepSolver, predict_mean_var (which factors), close -- a handle, an
               upload, a launch chain and stream synchronisations per series; the value is not computed there
One JSON line per row, with the smallest loop sample (the bar: set_ms below loop_min_ms) and whether the set's means and
variances are the loop's bit for bit.  For the per-kernel split of one row run it under `rocprofv3 --kernel-trace
--stats -- python scripts/quasisep_series_predict_timing.py --rows 64:16384:4096:matern32_J2`.
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
ROWS = "64:16384:4096:matern32_J2,64:16384:4096:celerite4_J8,1024:1000:256:matern32_J2"


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
    ap.add_argument("--rows", default=ROWS)
    args = ap.parse_args()
    for row in args.rows.split(","):
        nb, n, m, name = row.split(":")
        nb, n, m, make = int(nb), int(n), int(m), MODELS[name]
        rng = np.random.default_rng(0)
        lengths = rng.integers(int(0.7 * n), int(1.3 * n) + 1, nb)
        ts = [np.sort(rng.uniform(0, 0.05 * k, k)) for k in lengths]
        ys = [rng.standard_normal(k) for k in lengths]
        noises = [rng.uniform(0.05, 0.2, k) for k in lengths]
        xts = [rng.uniform(t[0] - 0.5, t[-1] + 0.5, m) for t in ts]

        def scale(i, b):
            return 1.0 + 1e-3 * i + 1e-5 * b  # fresh per call, distinct per member

        series = QuasisepSeriesSet(ts, assume_sorted=True)

        def as_set(i):
            return series.predict([make(scale(i, b)) for b in range(nb)], ys, noises, xts)

        def loop(i):
            out = []
            for b in range(nb):
                s = QuasisepSolver(make(scale(i, b)), ts[b], Diagonal(noises[b]), assume_sorted=True)
                try:
                    out.append(s.predict_mean_var(ys[b], xts[b]))
                finally:
                    s.close()
            return out

        got, want = as_set(0), loop(0)
        same = all(np.array_equal(got[1][b], mu) and np.array_equal(got[2][b], var) for b, (mu, var) in enumerate(want))
        cell = {"B": nb, "n": n, "points": int(lengths.sum()), "m": m, "kernel": name,
                "J": make(1.0)._lower_ssm().J}
        for key, fn in (("set", as_set), ("loop", loop)):
            s = samples_ms(fn, args.reps)
            cell[key + "_ms"] = round(float(np.median(s)), 4)
            cell[key + "_spread_ms"] = round(max(s) - min(s), 4)
            cell[key + "_min_ms"] = round(min(s), 4)
        cell["loop_over_set"] = round(cell["loop_ms"] / cell["set_ms"], 3)
        cell["set_below_loop_min"] = bool(cell["set_ms"] < cell["loop_min_ms"])
        cell["bit_identical"] = bool(same)
        print(json.dumps(cell), flush=True)
        series.close()


if __name__ == "__main__":
    main()
