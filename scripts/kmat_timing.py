#!/usr/bin/env python
"""Wall-clock of the kmat.hip kernels outside the assembly: `log_probability_and_grad` at N = 8192 for
`amp * ExpSquared` (the two-sum gradient evaluator) and for `amp * ExpSquared + amp * Matern32` (the general one), and
`Kernel.matmul` at 16 384 x 16 384 with 8 vectors for both.  Median of 5 after one warm-up; one JSON line per row.

    python scripts/kmat_timing.py [N_grad] [N_matmul]
"""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def median_ms(fn, reps=5):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    from tinygp_amd import GaussianProcess, kernels, synthetic

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    progs = {
        "amp_expsq": 1.5**2 * kernels.ExpSquared(2.5),
        "expsq_plus_m32": 1.5**2 * kernels.ExpSquared(2.5) + 0.3 * kernels.Matern32(1.2),
    }
    X, y = synthetic.make_inputs(n, 1)
    Xm, _ = synthetic.make_inputs(m, 1)
    V = np.random.default_rng(0).standard_normal((m, 8))
    for name, k in progs.items():
        gp = GaussianProcess(k, X, diag=0.01)
        med, lo, hi = median_ms(lambda: gp.log_probability_and_grad(y))
        print(json.dumps({"row": "log_probability_and_grad", "program": name, "n": n, "median_ms": med, "min_ms": lo,
                          "max_ms": hi}), flush=True)
        del gp
        med, lo, hi = median_ms(lambda: k.matmul(Xm, Xm, V))
        print(json.dumps({"row": "matmul_8_vectors", "program": name, "n": m, "median_ms": med, "min_ms": lo,
                          "max_ms": hi}), flush=True)


if __name__ == "__main__":
    main()
