"""QuasisepSolver over a wide dynamic range of inputs, against the extended-precision sequential oracle.

The series hold a run of 40 tied points (longer than a chunk: every transition of that chunk is I), spacings of 1e-9,
gaps over which every transition underflows to exactly 0 (and shorter ones that take the over-damped SHO's cosh
argument past 710 while the transition is still non-zero), and noise over seven decades (10^-6 .. 10; at least
10^-3 on tied and near-tied points), relative to k(0).

Bar.  The reference is ``_quasisep_np`` / ``_quasisep_predict_np`` in ``o.EXT`` (80-bit ``np.longdouble``, or mpmath
where that is only a double).  For each quantity ``e64`` is the error of the float64 sequential oracle against it and
the device must be within ``max(project bar, 8 * e64)``; the project bar is 1e-8 relative for the likelihood and
rtol = atol = 5e-7 for solves and posteriors (error measure ``max |x - ref| / (1 + |ref|)``).  The 8 allows for the
reassociation of up to three scan levels on top of a chunk replay: a judgment, not a derivation.  The inputs are tamed
(the noise floor is raised on tied and near-tied points) until ``e64`` is at most 1e-9 for the likelihood and 5e-8 for
the rest, which the test asserts, so a reference that drifts cannot hide a failure."""
import numpy as np
import pytest

from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSolver

import _quasisep_np as o
import _quasisep_predict_np as po
from _quasisep_cases import CASES

pytestmark = pytest.mark.gpu

# name -> (kernel, slowest decay rate of its transition: exp(-rate dt) bounds every entry's envelope)
RANGE_CASES = {
    "matern32": (lambda: CASES["matern32"](q), np.sqrt(3) / 0.8),
    "matern52": (lambda: CASES["matern52"](q), np.sqrt(5) / 1.1),
    "m32cos_plus_sho": (lambda: CASES["m32cos_plus_sho"](q), 1.0 / 3.0),
    "celerite4": (lambda: CASES["celerite4"](q), 0.2),
    "m52_times_sho": (lambda: CASES["m52_times_sho"](q), 0.25),
    "sigma_1e3": (lambda: q.Matern32(scale=0.8, sigma=1e3) + q.SHO(omega=2.0, quality=3.0, sigma=1e3), 1.0 / 3.0),
    "sigma_1e-3": (lambda: 1e-6 * CASES["m32cos_plus_sho"](q), 1.0 / 3.0),
    "sho_q1e3": (lambda: q.SHO(omega=2.0, quality=1e3), 1e-3),
    "sho_q0.3": (lambda: CASES["sho_over"](q), 2 * 1.5 * 0.3 / (1 + 0.8)),
    "sho_q0.05": (lambda: q.SHO(omega=1.5, quality=0.05, sigma=1.3), 2 * 1.5 * 0.05 / (1 + np.sqrt(0.99))),
}
AMPLITUDE2 = {"sigma_1e3": 1e6, "sigma_1e-3": 1e-6}  # k(0) scale: the noise is drawn relative to it
SIZES = [1500, 70000]
TIES = slice(96, 136)  # steps with dt = 0: chunks [96, 112), [112, 128) of 16 and [96, 128) of 32 hold nothing else


def make_problem(name, n):
    """(kernel, t, noise, r, y, xt) and the indices of the steps whose transition must be exactly zero."""
    kernel, rate = RANGE_CASES[name]
    k = kernel()
    rng = np.random.default_rng(n + sum(map(ord, name)))
    dt = rng.exponential(0.3, n)
    dt[rng.uniform(size=n) < 0.15] = 1e-9
    dt[300:330] = 1e-9
    dt[rng.uniform(size=n) < 0.05] = 0.0
    dt[TIES] = 0.0
    zero_gaps = np.array([400, n // 2, n - 7])
    long_gaps = np.array([200, 700, n - 100])
    dt[zero_gaps] = 800.0 / rate   # exp(-800) = 0 in float64
    dt[long_gaps] = 200.0 / rate   # exp(-200): far down, not zero
    dt[0] = 0.0
    t = np.cumsum(dt)
    close = np.diff(t, prepend=-np.inf) < 1e-6
    close |= np.roll(close, -1)
    noise = 10.0 ** rng.uniform(-6, 1, n)
    noise[close] = np.maximum(noise[close], 10.0 ** rng.uniform(-3, 1, n)[close])  # the floor on (near-)tied points
    noise *= AMPLITUDE2.get(name, 1.0)
    r = rng.standard_normal(n) * np.sqrt(AMPLITUDE2.get(name, 1.0))
    y = rng.standard_normal((n, 2))
    xt = np.concatenate([
        rng.uniform(t[0], t[-1], 100), t[rng.integers(0, n, 60)], t[rng.integers(0, n, 30)] + 1e-9,
        t[[100, 120, 135, 136, 310]], t[zero_gaps] - 0.5 * 800.0 / rate, t[long_gaps] - 0.5 * 200.0 / rate,
        t[zero_gaps - 1] + 1.0, t[zero_gaps] - 1.0, [t[0] - 1.0, t[-1] + 1.0, t[0] - 1e4 / rate, t[-1] + 1e4 / rate]])
    return k, t, noise, r, y, xt, zero_gaps


def oracle_quantities(k, t, noise, r, y, xt, dtype):
    F = o.factor(k, t, noise, dtype)
    mean, var = po.predict(k, t, noise, r, xt, F=F, dtype=dtype)
    return dict(logp=o.log_probability(k, t, noise, r, dtype, F=F), solve=o.solve_lower(F, y),
                solve_T=o.solve_upper(F, y), mean=mean, var=var)


def error(x, ref, relative=False):
    d = np.abs(np.asarray(x, dtype=ref.dtype if isinstance(ref, np.ndarray) else None) - ref)
    return float(np.max(d / (np.abs(ref) if relative else 1 + np.abs(ref))))


BARS = dict(logp=(1e-8, 1e-9), solve=(5e-7, 5e-8), solve_T=(5e-7, 5e-8), mean=(5e-7, 5e-8), var=(5e-7, 5e-8))


def reference_errors(name, n):
    """The problem, the extended reference and e64 per quantity (CPU only)."""
    k, t, noise, r, y, xt, zero_gaps = make_problem(name, n)
    A = o.transitions(k, t)
    assert np.all(A[zero_gaps] == 0.0) and np.all(A[TIES] == np.eye(A.shape[-1]))
    assert np.all(np.isfinite(A))
    ref = oracle_quantities(k, t, noise, r, y, xt, o.EXT)
    f64 = oracle_quantities(k, t, noise, r, y, xt, np.float64)
    e64 = {key: error(f64[key], ref[key], relative=key == "logp") for key in BARS}
    return (k, t, noise, r, y, xt), ref, e64


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(RANGE_CASES))
def test_dynamic_range(name, n):
    (k, t, noise, r, y, xt), ref, e64 = reference_errors(name, n)
    s = QuasisepSolver(k, t, Diagonal(noise))
    mean, var = s.predict_mean_var(r, xt)
    dev = dict(logp=s.log_probability(r), solve=s.solve_triangular(y), solve_T=s.solve_triangular(y, transpose=True),
               mean=mean, var=var)
    assert s.info == 0
    s.close()
    failed = []
    for key, (bar, cond) in BARS.items():
        ed = error(dev[key], ref[key], relative=key == "logp")
        print(f"range {name} n={n} {key}: e64 = {e64[key]:.2e}, device = {ed:.2e}, ratio = "
              f"{ed / max(e64[key], 1e-300):.2f}, allowed = {max(bar, 8 * e64[key]):.1e}")
        assert e64[key] <= cond, f"{key}: the float64 oracle itself is {e64[key]:.2e} from the reference (> {cond:.0e})"
        if not ed <= max(bar, 8 * e64[key]):
            failed.append((key, ed, e64[key]))
    assert not failed
