#!/usr/bin/env python
"""Every output of the quasiseparable device path on a fixed, seeded case list, for bit-for-bit comparison of two builds.

    python scripts/quasisep_bits.py dump FILE.npz
    python scripts/quasisep_bits.py compare A.npz B.npz

`dump` runs the cases on the device with whatever `libtgp_hip.so` the package loads (`TGP_HIP_LIBRARY` names another
build) and stores every array.  `compare` requires `np.array_equal` on every array (NaNs equal where both have one)
and exits non-zero on the first difference, naming the array.  Run both dumps on the same machine.

Cases: `matern32` (J = 2), `m32cos_plus_sho` (J = 6) and `celerite4` (J = 8) of tests/_quasisep_cases.py at
N = 1, 17, 1025, 4097 (one and two scan levels, a ragged last chunk), and `matern32` at N = 2^20 + 1 (three levels).
Per case: the factor, `log_probability`, both triangular solves and `dot_triangular` for 1, 9 and 17 columns,
`predict_mean_var` at 33 unsorted test points (before, after and on the data), `predict_terms` of the kernel's addends
there and at the data (`X_test=None`), `value_and_grad`, and a three-member `log_probability_batch` with a noise vector
per member.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

KERNELS = ("matern32", "m32cos_plus_sho", "celerite4")
SIZES = (1, 17, 1025, 4097)
LARGE = ("matern32", (1 << 20) + 1)
WIDTHS = (1, 9, 17)


def case_data(n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 0.2 * n + 1.0, n))
    if n > 8:
        t[7] = t[6]  # a repeated coordinate: dt = 0
    noise = rng.uniform(0.05, 0.2, n)
    resid = rng.standard_normal(n)
    rhs = rng.standard_normal((n, max(WIDTHS)))
    xt = rng.uniform(t[0], t[-1] + 1e-3, 33)
    xt[0], xt[1] = t[0] - 0.7, t[0] - 0.1          # before the first datum
    xt[2], xt[3] = t[-1] + 0.3, t[-1] + 2.5        # after the last
    xt[4], xt[5], xt[6] = t[0], t[-1], t[n // 2]   # exact ties with data
    xt[7] = t[min(7, n - 1)]                       # the repeated coordinate
    noises = rng.uniform(0.05, 0.2, (3, n))
    return t, noise, resid, rhs, rng.permutation(xt), noises


def run_case(name, n, seed, out):
    from _quasisep_cases import CASES

    from tinygp_amd.kernels import quasisep as q
    from tinygp_amd.noise import Diagonal
    from tinygp_amd.solvers import QuasisepSolver

    t, noise, resid, rhs, xt, noises = case_data(n, seed)
    kernel = CASES[name](q)
    tag = f"{name}/N{n}/"

    def put(key, value):
        out[tag + key] = np.asarray(value)

    s = QuasisepSolver(kernel, t, Diagonal(noise), assume_sorted=True)
    put("info", s.refactor())
    c, w = s.factor_data()
    put("c", c)
    put("w", w)
    for R in WIDTHS:
        y = rhs[:, 0] if R == 1 else rhs[:, :R]
        put(f"solve_R{R}", s.solve_triangular(y))
        put(f"solve_T_R{R}", s.solve_triangular(y, transpose=True))
        put(f"dot_R{R}", s.dot_triangular(y))
    mean, var = s.predict_mean_var(resid, xt)
    put("predict_mean", mean)
    put("predict_var", var)
    means, vars_ = s.predict_terms(resid, xt)
    put("terms_mean", means)
    put("terms_var", vars_)
    means, vars_ = s.predict_terms(resid, None)
    put("terms_data_mean", means)
    put("terms_data_var", vars_)
    s.close()

    s = QuasisepSolver(kernel, t, Diagonal(noise), assume_sorted=True)
    put("log_probability", s.log_probability(resid))
    value, grads = s.value_and_grad(resid)
    put("grad_value", value)
    put("grad_kernel", grads["kernel"])
    put("grad_noise", grads["noise_diag"])
    put("grad_mean", grads["mean"])
    members = [scale * CASES[name](q) for scale in (0.7, 1.0, 1.3)]
    values, info = s.log_probability_batch(members, resid, noises, return_info=True)
    put("batch_values", values)
    put("batch_info", info)
    s.close()


def dump(path):
    out = {}
    cases = [(k, n) for k in KERNELS for n in SIZES] + [LARGE]
    for seed, (name, n) in enumerate(cases):
        run_case(name, n, 100 + seed, out)
        print(f"{name} N={n}: done", flush=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    if sorted(a.files) != sorted(b.files):
        print(f"different sets of arrays: {sorted(set(a.files) ^ set(b.files))}")
        return 1
    for key in sorted(a.files):
        x, y = a[key], b[key]
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            where = ""
            if x.shape == y.shape and x.size:
                bad = np.flatnonzero(~((x == y) | ((x != x) & (y != y))).ravel())
                where = f": {bad.size} of {x.size} entries, first at flat index {bad[0]}"
            print(f"DIFFERENT {key}{where}")
            return 1
    print(f"{len(a.files)} arrays bit-identical")
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        return compare(sys.argv[2], sys.argv[3])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
