#!/usr/bin/env python
"""Time QuasisepSeriesSet.sample_conditional against the route a set of series had before it: a loop that builds one
QuasisepSolver per series, calls log_probability and sample_conditional and closes it.

    python scripts/quasisep_series_sample_timing.py [--rows 64:16384:4096:matern32_J2,...] [--cols 1,16] [--reps 9]

The method of scripts/quasisep_series_predict_timing.py and scripts/quasisep_sample_timing.py: fresh hyper-parameters per
call (every member's differ too), host transfers of the normals, the residuals, the test points and the samples and the
lowering of the kernels included, drawing the normals excluded (they are drawn once per row and column count), two
warm-ups, then the median of `reps` wall times with their spread.  A row is B:N:M:model -- B series whose lengths are
drawn once (seed 0) within +-30 % of N, every series with coordinates, noise, data and M unsorted test points of its own.
Per row and per R of --cols, in one process:
    set_ms     one sample_conditional call on a resident QuasisepSeriesSet (values, draws at the test points and at the data)
    loop_ms    the loop over the series: a fresh QuasisepSolver, log_probability, sample_conditional (return_data), close --
               a handle, an upload, a launch chain and stream synchronisations per series
    pack_ms    the part of set_ms that the host spends concatenating the members' normals into the call's two arrays
One JSON line per cell, with the smallest loop sample, the chains and column passes the set call took and whether the
set's values and draws are the loop's bit for bit.  For the per-kernel split of one cell run it under `rocprofv3
--kernel-trace --stats -- python scripts/quasisep_series_sample_timing.py --rows 64:16384:4096:matern32_J2 --cols 16`.
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
from tinygp_amd.solvers.quasisep import pack_series_normals  # noqa: E402

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
    ap.add_argument("--cols", default="1,16")
    args = ap.parse_args()
    for row in args.rows.split(","):
        nb, n, m, name = row.split(":")
        nb, n, m, make = int(nb), int(n), int(m), MODELS[name]
        J = make(1.0)._lower_ssm().J
        rng = np.random.default_rng(0)
        lengths = rng.integers(int(0.7 * n), int(1.3 * n) + 1, nb)
        ts = [np.sort(rng.uniform(0, 0.05 * k, k)) for k in lengths]
        ys = [rng.standard_normal(k) for k in lengths]
        noises = [rng.uniform(0.05, 0.2, k) for k in lengths]
        xts = [rng.uniform(t[0] - 0.5, t[-1] + 0.5, m) for t in ts]

        def scale(i, b):
            return 1.0 + 1e-3 * i + 1e-5 * b  # fresh per call, distinct per member

        series = QuasisepSeriesSet(ts, assume_sorted=True)
        for R in [int(v) for v in args.cols.split(",")]:
            xis = [rng.standard_normal((k + m, J, R)) for k in lengths]
            epss = [rng.standard_normal((k, R)) for k in lengths]

            def as_set(i):
                return series.sample_conditional([make(scale(i, b)) for b in range(nb)], ys, noises, xts, xi=xis,
                                                 eps=epss, return_data=True)

            def loop(i):
                out = []
                for b in range(nb):
                    s = QuasisepSolver(make(scale(i, b)), ts[b], Diagonal(noises[b]), assume_sorted=True)
                    try:
                        v = s.log_probability(ys[b])
                        out.append((v,) + s.sample_conditional(ys[b], xts[b], xi=xis[b], eps=epss[b], return_data=True))
                    finally:
                        s.close()
                return out

            got, want = as_set(0), loop(0)
            same = all(got[0][b] == v and np.array_equal(got[2][b], data) and np.array_equal(got[1][b], test)
                       for b, (v, data, test) in enumerate(want))
            cell = {"B": nb, "n": n, "points": int(lengths.sum()), "m": m, "kernel": name, "J": J, "R": R,
                    "chains": series.sample_chains, "passes": series.sample_passes,
                    "normals_MB": round(8e-6 * sum(a.size for a in xis + epss), 1)}
            del got, want
            def pack(i):  # the host's share of the set call that the loop does not pay: one concatenated copy
                return pack_series_normals(lengths, [m] * nb, J, xis, epss)

            for key, fn in (("set", as_set), ("loop", loop), ("pack", pack)):
                s = samples_ms(fn, args.reps)
                cell[key + "_ms"] = round(float(np.median(s)), 4)
                cell[key + "_spread_ms"] = round(max(s) - min(s), 4)
                cell[key + "_min_ms"] = round(min(s), 4)
            cell["loop_over_set"] = round(cell["loop_ms"] / cell["set_ms"], 3)
            cell["set_below_loop_min"] = bool(cell["set_ms"] < cell["loop_min_ms"])
            cell["bit_identical"] = bool(same)
            print(json.dumps(cell), flush=True)
            del xis, epss
        series.close()


if __name__ == "__main__":
    main()
