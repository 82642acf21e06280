#!/usr/bin/env python
"""Time QuasisepSolver.value_and_grad: the log-probability and its gradient with respect to every kernel parameter,
the noise and the mean.

    python scripts/quasisep_grad_timing.py [--reps 9] [--sizes 14,16,20,22]

Kernels: Matern32 (J = 2, 2 parameters), Matern32 x Cosine + SHO (J = 6, 7 parameters), a four-term Celerite sum
(J = 8, 16 parameters), as in scripts/quasisep_timing.py.  Wall time per call with fresh hyper-parameters each call
(host synchronised: the call returns host arrays; the transfers of the residual, the noise and both result vectors are
included), two warm-up calls discarded, median of the rest.  Beside each: this tree's `log_probability` on the same
solver in the same run, and the ratio of the two; `budget` is 1 + 2 P, the arithmetic of the gradient in
likelihood-equivalents.  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -- python scripts/quasisep_grad_timing.py --sizes 20 --reps 1`.
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
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    for p in [int(v) for v in args.sizes.split(",")]:
        n = 1 << p
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        y = rng.standard_normal(n)
        noise = np.full(n, 0.1)
        for name, make in MODELS.items():
            s = QuasisepSolver(make(1.0), t, Diagonal(noise), assume_sorted=True)

            def fresh(i):
                k = make(1.0 + 1e-3 * i)  # fresh hyper-parameters
                s._ssm, s.kernel = k._lower_ssm(), k

            def logp(i):
                fresh(i)
                return s.log_probability(y)

            def grad(i):
                fresh(i)
                return s.value_and_grad(y)

            logp_ms = median_ms(logp, args.reps)
            grad_ms = median_ms(grad, args.reps)
            npar = len(s.kernel.parameters())
            print(json.dumps({"n": n, "kernel": name, "J": s._ssm.J, "parameters": npar, "value_and_grad_ms": grad_ms,
                              "log_probability_ms": logp_ms, "grad_over_logp": grad_ms / logp_ms,
                              "budget": 1 + 2 * npar}), flush=True)
            s.close()


if __name__ == "__main__":
    main()
