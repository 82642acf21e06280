#!/usr/bin/env python
"""Time QuasisepSolver.sample_conditional: R posterior draws at M unsorted test points on a factored solver.

    python scripts/quasisep_sample_timing.py [--reps 9] [--sizes 14,16,20] [--m 4096] [--dense-reps 1]

Kernels: Matern32 (J = 2), Matern32 x Cosine + SHO (J = 6), a four-term Celerite sum (J = 8), as in
scripts/quasisep_predict_timing.py.  Wall time per call at R = 1 and R = 16 with a fresh residual each call (host
synchronised: the call returns host arrays; the transfers of the normals, the residual, the test points and the samples
are included, drawing the normals is not), two warm-up calls discarded, median of the rest.  Beside each: the same
run's `log_probability` (factor + forward solve, fresh hyper-parameters) and `predict_mean_var` (mean and variance) on
the same solver, and the sample time as a multiple of the prediction.  Last, at N = 2^14, the route a draw took before:
`gp.condition(y, X_test).gp.sample(key)` (k(X, X_test) on the host, M device solves, the M x M covariance and its dense
factorisation), for the same M.  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -- python scripts/quasisep_sample_timing.py --sizes 20 --dense-reps 0`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tinygp_amd import GaussianProcess  # noqa: E402
from tinygp_amd.kernels import quasisep as q  # noqa: E402
from tinygp_amd.noise import Diagonal  # noqa: E402
from tinygp_amd.solvers import QuasisepSolver  # noqa: E402

MODELS = {
    "matern32_J2": lambda s: q.Matern32(scale=2.0 * s),
    "m32xcos+sho_J6": lambda s: q.Matern32(scale=1.5 * s) * q.Cosine(scale=3.0) + q.SHO(omega=2.0 / s, quality=3.0),
    "celerite4_J8": lambda s: (q.Celerite(1.0, 0.2, 0.5 / s, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5 / s)
                               + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2 * s, 4.0)),
}
COLUMNS = (1, 16)


def median_ms(fn, reps, warmup=2):
    for i in range(warmup):
        fn(i)
    times = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warmup + i)
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="14,16,20")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--dense-reps", type=int, default=1, help="0 skips the dense route at N = 2^14")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    for p in [int(v) for v in args.sizes.split(",")]:
        n = 1 << p
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        ys = rng.standard_normal((args.reps + 2, n))
        xt = rng.uniform(t[0] - 1.0, t[-1] + 1.0, args.m)  # unsorted
        noise = np.full(n, 0.1)
        for name, make in MODELS.items():
            s = QuasisepSolver(make(1.0), t, Diagonal(noise), assume_sorted=True)
            J = s.state_dimension

            def logp(i):
                s._ssm = make(1.0 + 1e-3 * i)._lower_ssm()  # fresh hyper-parameters
                return s.log_probability(ys[0])

            logp_ms = median_ms(logp, args.reps)
            s.refactor(make(1.0))
            pred_ms = median_ms(lambda i: s.predict_mean_var(ys[i], xt), args.reps)
            row = {"n": n, "m": args.m, "kernel": name, "J": J, "log_probability_ms": logp_ms, "predict_ms": pred_ms}
            for R in COLUMNS:
                xi, eps = rng.standard_normal((n + args.m, J, R)), rng.standard_normal((n, R))
                ms = median_ms(lambda i: s.sample_conditional(ys[i], xt, xi=xi, eps=eps), args.reps)
                row.update({f"sample_R{R}_ms": ms, f"sample_R{R}_over_predict": ms / pred_ms,
                            f"passes_R{R}": s.sample_passes})
                del xi, eps
            print(json.dumps(row), flush=True)
            s.close()

    if args.dense_reps > 0:
        n = 1 << 14
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        ys = rng.standard_normal((args.reps + 2, n))
        xt = rng.uniform(t[0] - 1.0, t[-1] + 1.0, args.m)
        for name, make in MODELS.items():
            gp = GaussianProcess(make(1.0), t, diag=0.1, assume_sorted=True)
            dense_ms = median_ms(lambda i: gp.condition(ys[i], xt).gp.sample(i), args.dense_reps, warmup=0)
            ms = median_ms(lambda i: gp.sample_conditional(ys[i], xt, key=i), args.reps)
            print(json.dumps({"n": n, "m": args.m, "kernel": name, "condition_sample_ms": dense_ms,
                              "sample_conditional_ms": ms, "dense_over_sample": dense_ms / ms}), flush=True)
            gp.solver.close()


if __name__ == "__main__":
    main()
