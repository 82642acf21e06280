#!/usr/bin/env python
"""Time QuasisepSolver.predict_terms: the terms of a sum at M test points on a factored solver.

    python scripts/quasisep_terms_timing.py [--reps 9] [--sizes 14,20] [--m 4096] [--sections regress,sharing,data]

Method of scripts/quasisep_predict_timing.py: wall time per call with a fresh residual each call (host synchronised;
the transfers of the residual, the test points and the results are included), fp64, two warm-up calls discarded,
median of the rest; beside each median the spread (max - min) of the samples.

regress   `predict_mean_var` (mean and variance) for the three kernels of that script.  It uses nothing this feature
          added, so the same section run from a checkout of the parent commit gives the figures to compare with.
sharing   the four-term Celerite sum: one `predict_terms` call for its K = 4 terms against four single-term calls
          (each with its own pair of scans), and against `predict_mean_var`.
data      `predict_terms(X_test=None)` against `predict_terms(X_test=t.copy())` at the largest size (M = N).
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
    "matern32_J2": lambda: q.Matern32(scale=2.0),
    "m32xcos+sho_J6": lambda: q.Matern32(scale=1.5) * q.Cosine(scale=3.0) + q.SHO(omega=2.0, quality=3.0),
    "celerite4_J8": lambda: (q.Celerite(1.0, 0.2, 0.5, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5)
                             + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2, 4.0)),
}


def sample_ms(fn, reps, warmup=2):
    """(median, spread) in ms of `reps` calls after `warmup` discarded ones."""
    for i in range(warmup):
        fn(i)
    times = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warmup + i)
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times)), 1e3 * float(max(times) - min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="14,20")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--sections", default="regress,sharing,data")
    args = ap.parse_args()
    sections = args.sections.split(",")
    sizes = [int(v) for v in args.sizes.split(",")]
    rng = np.random.default_rng(0)
    for p in sizes:
        n = 1 << p
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        ys = rng.standard_normal((args.reps + 2, n))
        xt = rng.uniform(t[0] - 1.0, t[-1] + 1.0, args.m)  # unsorted
        noise = np.full(n, 0.1)
        if "regress" in sections:
            for name, make in MODELS.items():
                s = QuasisepSolver(make(), t, Diagonal(noise), assume_sorted=True)
                s.refactor()
                ms, spread = sample_ms(lambda i: s.predict_mean_var(ys[i], xt), args.reps)
                print(json.dumps({"section": "regress", "n": n, "m": args.m, "kernel": name,
                                  "predict_mean_var_ms": ms, "spread_ms": spread}), flush=True)
                s.close()
        if "sharing" in sections:
            k = MODELS["celerite4_J8"]()
            terms = k._addends()
            s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
            s.refactor()
            for var in (True, False):
                one, one_sp = sample_ms(lambda i: s.predict_terms(ys[i], xt, return_var=var), args.reps)
                four, four_sp = sample_ms(
                    lambda i: [s.predict_terms(ys[i], xt, [term], return_var=var) for term in terms], args.reps)
                own, own_sp = sample_ms(lambda i: s.predict_mean_var(ys[i], xt, return_var=var), args.reps)
                print(json.dumps({"section": "sharing", "n": n, "m": args.m, "return_var": var, "terms": len(terms),
                                  "one_call_ms": one, "one_call_spread_ms": one_sp, "four_calls_ms": four,
                                  "four_calls_spread_ms": four_sp, "four_over_one": four / one,
                                  "predict_mean_var_ms": own, "predict_mean_var_spread_ms": own_sp}), flush=True)
            s.close()
    if "data" in sections:
        n = 1 << max(sizes)
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        ys = rng.standard_normal((args.reps + 2, n))
        k = MODELS["celerite4_J8"]()
        s = QuasisepSolver(k, t, Diagonal(np.full(n, 0.1)), assume_sorted=True)
        s.refactor()
        for sel, label in ((None, "4 terms"), ([k], "whole kernel")):
            none_ms, none_sp = sample_ms(lambda i: s.predict_terms(ys[i], None, sel), args.reps)
            copy_ms, copy_sp = sample_ms(lambda i: s.predict_terms(ys[i], t.copy(), sel), args.reps)
            a, b = s.predict_terms(ys[0], None, sel), s.predict_terms(ys[0], t.copy(), sel)
            print(json.dumps({"section": "data", "n": n, "m": n, "selectors": label, "x_test_none_ms": none_ms,
                              "x_test_none_spread_ms": none_sp, "x_test_copy_ms": copy_ms,
                              "x_test_copy_spread_ms": copy_sp,
                              "bit_identical": bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))}),
                  flush=True)
        s.close()


if __name__ == "__main__":
    main()
