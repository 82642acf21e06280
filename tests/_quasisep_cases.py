"""Quasiseparable kernel cases shared by the golden generator and the tests.  ``build(q)`` takes the module that
holds the classes (this package's ``kernels.quasisep`` or the reference's), so both sides build the same kernel."""
import numpy as np

CASES = {
    "exp": lambda q: q.Exp(scale=1.3, sigma=0.7),
    "matern32": lambda q: q.Matern32(scale=0.8, sigma=1.2),
    "matern52": lambda q: q.Matern52(scale=1.1, sigma=0.9),
    "cosine": lambda q: q.Cosine(scale=2.0, sigma=1.1),
    "celerite": lambda q: q.Celerite(a=1.0, b=0.2, c=0.5, d=1.5),
    "sho_under": lambda q: q.SHO(omega=2.0, quality=3.0),
    "sho_crit": lambda q: q.SHO(omega=1.5, quality=0.5, sigma=0.8),
    "sho_over": lambda q: q.SHO(omega=1.5, quality=0.3, sigma=1.3),
    "sum_sho_m32": lambda q: q.SHO(omega=2.0, quality=3.0) + q.Matern32(scale=5.0),
    "prod_m32_cos": lambda q: q.Matern32(scale=1.5) * q.Cosine(scale=3.0),
    "scale_m52": lambda q: 0.5 * q.Matern52(scale=2.0),
    "m32cos_plus_sho": lambda q: q.Matern32(scale=1.5) * q.Cosine(scale=3.0) + q.SHO(omega=2.0, quality=3.0),
    "m52_times_sho": lambda q: q.Matern52(scale=2.0) * q.SHO(omega=1.0, quality=2.0),
    "celerite4": lambda q: (q.Celerite(1.0, 0.2, 0.5, 1.5) + q.Celerite(0.5, 0.04, 0.3, 2.5)
                            + q.Celerite(0.8, 0.05, 1.0, 0.7) + q.Celerite(0.3, 0.01, 0.2, 4.0)),
    "scaled_sum": lambda q: 1.7 * (q.Exp(scale=0.5) + q.Matern32(scale=2.0, sigma=0.5)),
}


def data(n=64, seed=11):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 12.0, n))
    t[7] = t[6]  # a repeated coordinate: dt = 0
    noise = rng.uniform(0.05, 0.2, n)
    r = rng.standard_normal(n)
    return t, noise, r
