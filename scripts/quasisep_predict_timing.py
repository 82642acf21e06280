#!/usr/bin/env python
"""Time QuasisepSolver.predict_mean_var: conditional mean and variance at M test points on a factored solver.

    python scripts/quasisep_predict_timing.py [--reps 9] [--sizes 14,16,20,22] [--m 4096] [--dense-reps 3]

Kernels: Matern32 (J = 2), Matern32 x Cosine + SHO (J = 6), a four-term Celerite sum (J = 8), as in
scripts/quasisep_timing.py.  Wall time per call with a fresh residual each call (host synchronised: the call returns
host arrays; the transfers of the residual, the test points and the results are included), two warm-up calls
discarded, median of the rest.  Beside each: this tree's `log_probability` on the same solver (factor + forward solve,
fresh hyper-parameters) and the ratio of the two.  Last, at N = 2^14, the dense route prediction took before
(`alpha` + host `kernel.matmul` for the mean, `_cond` for the variance: Ks on the host, M device solves), from the
same residual to the same two arrays.  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -- python scripts/quasisep_predict_timing.py --sizes 20 --dense-reps 0`.
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
    ap.add_argument("--sizes", default="14,16,20,22")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--dense-reps", type=int, default=3, help="0 skips the dense route at N = 2^14")
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

            def logp(i):
                s._ssm = make(1.0 + 1e-3 * i)._lower_ssm()  # fresh hyper-parameters
                return s.log_probability(ys[0])

            logp_ms = median_ms(logp, args.reps)
            s.refactor(make(1.0))
            pred_ms = median_ms(lambda i: s.predict_mean_var(ys[i], xt), args.reps)
            mean_ms = median_ms(lambda i: s.predict_mean_var(ys[i], xt, return_var=False), args.reps)
            print(json.dumps({"n": n, "m": args.m, "kernel": name, "J": s._ssm.J, "predict_ms": pred_ms,
                              "mean_only_ms": mean_ms, "log_probability_ms": logp_ms,
                              "predict_over_logp": pred_ms / logp_ms}), flush=True)
            s.close()

    if args.dense_reps > 0:
        n = 1 << 14
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        ys = rng.standard_normal((args.reps + 2, n))
        xt = rng.uniform(t[0] - 1.0, t[-1] + 1.0, args.m)
        for name, make in MODELS.items():
            k = make(1.0)
            s = QuasisepSolver(k, t, Diagonal(np.full(n, 0.1)), assume_sorted=True)

            def dense(i):
                alpha, _ = s.alpha(ys[i])
                return k.matmul(xt, t, alpha), s._cond(k, xt, True)

            def device(i):
                return s.predict_mean_var(ys[i], xt)

            dm, dv = dense(0)
            pm, pv = device(0)
            dense_ms = median_ms(dense, args.dense_reps, warmup=0)
            pred_ms = median_ms(device, args.reps)
            print(json.dumps({"n": n, "m": args.m, "kernel": name, "dense_route_ms": dense_ms, "predict_ms": pred_ms,
                              "dense_over_predict": dense_ms / pred_ms,
                              "max_abs_diff_mean": float(np.abs(dm - pm).max()),
                              "max_abs_diff_var": float(np.abs(dv - pv).max())}), flush=True)
            s.close()


if __name__ == "__main__":
    main()
