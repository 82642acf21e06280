"""The sequential oracle of the quasiseparable conditional mean and variance against dense LAPACK, and the C ABI's
declaration of the device entry point.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q

import _quasisep_predict_np as po
from _quasisep_cases import CASES

ROOT = Path(__file__).resolve().parents[1]


def _problem(n=300, m=200, seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 30.0, n))
    t[10] = t[9]  # tied inputs
    t[151] = t[150]
    noise = rng.uniform(0.01, 0.3, n)
    r = rng.standard_normal(n)
    xt = np.concatenate([rng.uniform(-3.0, 33.0, m),       # unsorted, some outside the data
                         t[:5], t[-3:], t[[9, 10, 150]],     # on data points, tied ones included
                         [t[0] - 1e-9, t[-1] + 7.0, -50.0]])
    return t, noise, r, xt[rng.permutation(len(xt))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_dense(name):
    """Bar 1e-10: plain fp64 recurrences over a few hundred well-conditioned steps sit at 1e-13 or below."""
    k = CASES[name](q)
    t, noise, r, xt = _problem(seed=len(name))
    mean, var = po.predict(k, t, noise, r, xt)
    dmean, dvar = po.dense(k, t, noise, r, xt)
    print(name, "mean", np.abs(mean - dmean).max(), "var", np.abs(var - dvar).max(), "min var", dvar.min())
    np.testing.assert_allclose(mean, dmean, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(var, dvar, rtol=1e-10, atol=1e-10)


def test_intervals_side_right():
    t = np.array([0.0, 1.0, 1.0, 2.0])
    np.testing.assert_array_equal(po.intervals(t, [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]), [-1, 0, 0, 2, 2, 3, 3])


def test_single_point_and_no_test_points():
    k = CASES["sho_under"](q)
    t, noise, r = np.array([1.5]), np.array([0.2]), np.array([0.7])
    xt = np.array([0.0, 1.5, 4.0])
    mean, var = po.predict(k, t, noise, r, xt)
    dmean, dvar = po.dense(k, t, noise, r, xt)
    np.testing.assert_allclose(mean, dmean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(var, dvar, rtol=1e-12, atol=1e-12)
    mean, var = po.predict(k, t, noise, r, np.zeros(0))
    assert mean.shape == var.shape == (0,)


def test_predict_entry_point_is_declared_and_bound():
    header = (ROOT / "include" / "tgp_hip.h").read_text()
    assert re.search(r"\bint\s+tgp_qsep_predict\s*\(", header)
    assert "tgp_qsep_predict" in _ffi.SIGNATURES
    assert len(_ffi.SIGNATURES["tgp_qsep_predict"]) == 7
