#!/usr/bin/env python
"""Timings of the existing quasiseparable calls on one tree, for comparing two builds in one GPU visit.

    python scripts/quasisep_regress_timing.py ROOT

ROOT: the checkout whose package and library are timed (this one, or another commit exported and built elsewhere);
run the trees alternately.  Per N in {2^14, 2^20} and model (J = 2, 6, 8) one JSON line with [median, spread max - min]
in ms of nine samples after two warm-ups, fresh hyper-parameters per call, for `value_and_grad`, `log_probability`,
`QuasisepSeriesSet.log_probability` (B = 8 series within +-30 % of N) and `value_and_grad_batch` (B = 8)."""
import json
import os
import sys
import time

import numpy as np

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
from tinygp_amd.kernels import quasisep as q  # noqa: E402
from tinygp_amd.noise import Diagonal  # noqa: E402
from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver  # noqa: E402
import tinygp_amd  # noqa: E402

assert tinygp_amd.__file__.startswith(root), tinygp_amd.__file__
MODELS = {
    2: lambda s: q.Matern32(scale=2.0 * s),
    6: lambda s: q.Matern32(scale=1.5 * s) * q.Cosine(scale=3.0) + q.SHO(omega=2.0 / s, quality=3.0),
    8: lambda s: (q.Celerite(1.0, 0.2, 0.5 / s, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5 / s)
                  + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2 * s, 4.0)),
}


def samples(fn, reps=9):
    fn(0), fn(1)
    out = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(i + 2)
        out.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(out)), 4), round(max(out) - min(out), 4)


B = 8
for p in (14, 20):
    n = 1 << p
    rng = np.random.default_rng(0)
    t = np.sort(rng.uniform(0, 0.05 * n, n))
    y, noise = rng.standard_normal(n), rng.uniform(0.05, 0.2, n)
    lengths = rng.integers(int(0.7 * n), int(1.3 * n) + 1, B)
    ts = [np.sort(rng.uniform(0, 0.05 * m, m)) for m in lengths]
    ys, nzs = [rng.standard_normal(m) for m in lengths], [rng.uniform(0.05, 0.2, m) for m in lengths]
    for J, make in MODELS.items():
        s = QuasisepSolver(make(1.0), t, Diagonal(noise), assume_sorted=True)
        series = QuasisepSeriesSet(ts, assume_sorted=True)

        def renew(i, b=0):
            s.kernel = make(1.0 + 1e-3 * i + 1e-5 * b)
            s._ssm = s.kernel._lower_ssm()

        def vg(i):
            renew(i)
            return s.value_and_grad(y)

        def lp(i):
            renew(i)
            return s.log_probability(y)

        def sset(i):
            return series.log_probability([make(1.0 + 1e-3 * i + 1e-5 * b) for b in range(B)], ys, nzs)

        def vgb(i):
            return s.value_and_grad_batch([make(1.0 + 1e-3 * i + 1e-5 * b) for b in range(B)], y)

        row = {"n": n, "J": J}
        for key, fn in (("value_and_grad", vg), ("log_probability", lp), ("series_log_probability", sset),
                        ("value_and_grad_batch", vgb)):
            row[key] = samples(fn)
        print(json.dumps(row), flush=True)
        s.close()
        series.close()
