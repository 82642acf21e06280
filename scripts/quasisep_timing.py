#!/usr/bin/env python
"""Time QuasisepSolver.log_probability (factor + forward solve + sums, fp64, fresh hyper-parameters per call).

    python scripts/quasisep_timing.py [--reps 10] [--sizes 14,16,20,22]

Kernels: Matern32 (J = 2), Matern32 x Cosine + SHO (J = 6), a four-term Celerite sum (J = 8).  Wall time per call
after warm-up (host synchronised: each call returns its value), the bytes the device must move per call (t, y and
the noise read, c and w written, each read again by the solve) over that time as a share of HBM bandwidth, and
beside them the dense DirectSolver at N = 16 384 on the equal stationary Matern32 and the sequential NumPy oracle.
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python scripts/quasisep_timing.py`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from tinygp_amd import GaussianProcess, kernels  # noqa: E402
from tinygp_amd.kernels import quasisep as q  # noqa: E402
from tinygp_amd.noise import Diagonal  # noqa: E402
from tinygp_amd.solvers import DirectSolver, QuasisepSolver  # noqa: E402

HBM_BYTES_PER_S = 8.0e12

MODELS = {
    "matern32_J2": lambda s: q.Matern32(scale=2.0 * s),
    "m32xcos+sho_J6": lambda s: q.Matern32(scale=1.5 * s) * q.Cosine(scale=3.0) + q.SHO(omega=2.0 / s, quality=3.0),
    "celerite4_J8": lambda s: (q.Celerite(1.0, 0.2, 0.5 / s, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5 / s)
                               + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2 * s, 4.0)),
}


def time_calls(fn, reps):
    fn(0)
    fn(1)
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i + 2)
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="14,16,20,22")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []
    for p in [int(v) for v in args.sizes.split(",")]:
        n = 1 << p
        t = np.sort(rng.uniform(0, 0.05 * n, n))
        y = rng.standard_normal(n)
        noise = np.full(n, 0.1)
        for name, make in MODELS.items():
            s = QuasisepSolver(make(1.0), t, Diagonal(noise), assume_sorted=True)
            J = s._ssm.J

            def call(i):
                s._ssm = make(1.0 + 1e-3 * i)._lower_ssm()  # fresh hyper-parameters
                return s.log_probability(y)

            sec = time_calls(call, args.reps)
            moved = n * 8 * (3 + 2 * (1 + J) + 2)  # t, y, noise; c, w written and re-read; z written, t re-read
            rows.append({"n": n, "kernel": name, "J": J, "ms": 1e3 * sec,
                         "hbm_share": moved / sec / HBM_BYTES_PER_S})
            print(json.dumps(rows[-1]), flush=True)
    n = 16384
    t = np.sort(rng.uniform(0, 0.05 * n, n))
    y = rng.standard_normal(n)

    def dense(i):
        k = kernels.Matern32(2.0 + 1e-3 * i)
        return GaussianProcess(k, t, diag=0.1, solver=DirectSolver).log_probability(y)

    print(json.dumps({"n": n, "kernel": "dense DirectSolver Matern32", "ms": 1e3 * time_calls(dense, 3)}), flush=True)
    import _quasisep_np as o

    m = 1 << 14
    t0 = time.perf_counter()
    o.log_probability(MODELS["matern32_J2"](1.0), t[:m], np.full(m, 0.1), y[:m])
    print(json.dumps({"n": m, "kernel": "NumPy sequential oracle matern32_J2",
                      "ms": 1e3 * (time.perf_counter() - t0)}), flush=True)


if __name__ == "__main__":
    main()
