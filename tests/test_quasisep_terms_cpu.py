"""Terms of a quasiseparable sum without a device: the sequential oracle with the test-side vector g against dense
LAPACK, and ``Quasisep._term_vector``'s masks."""
import numpy as np
import pytest

from tinygp_amd.kernels import quasisep as q

import _quasisep_terms_np as tn
from _quasisep_cases import CASES

N = 300


def _problem(seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 0.05 * N + 1, N))
    t[7] = t[6]
    t[16] = t[15]
    xt = np.concatenate([rng.uniform(t[0] - 1, t[-1] + 1, 100), t[[0, 6, 7, 15, 16, N - 1]],
                         [t[0] - 2.0, t[-1] + 2.0]])
    return t, rng.uniform(0.05, 0.2, N), rng.standard_normal(N), xt[rng.permutation(len(xt))]


def _nested():
    k1, k2, k3 = q.Matern32(scale=1.5), q.SHO(omega=2.0, quality=3.0), 0.8 * q.Celerite(1.0, 0.2, 0.5, 1.5)
    return (k1 + k2) + k3, (k1, k2, k3)


def _celerite4():
    k = CASES["celerite4"](q)
    return k, tuple(k._addends())


@pytest.mark.parametrize("make", [_nested, _celerite4], ids=["m32_sho_celerite", "celerite4"])
def test_oracle_vs_dense(make):
    model, terms = make()
    t, noise, r, xt = _problem(3)
    selectors = list(terms) + [terms[0] + terms[-1], model]  # every term, one union, the whole kernel
    g = np.stack([model._term_vector(k) for k in selectors])
    means, vars_ = tn.predict_g(model, t, noise, r, xt, g)
    for j, k in enumerate(selectors):
        wmean, wvar = tn.dense_term(model, k, t, noise, r, xt)
        print(f"selector {j}: max |mean - dense| = {np.abs(means[j] - wmean).max():.3e}, "
              f"max |var - dense| = {np.abs(vars_[j] - wvar).max():.3e}")
        np.testing.assert_allclose(means[j], wmean, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(vars_[j], wvar, rtol=1e-10, atol=1e-10)
    one = tn.predict_g(model, t, noise, r, xt, g[1])  # a single vector gives the same row
    assert np.array_equal(one[0], means[1]) and np.array_equal(one[1], vars_[1])


def test_term_vector_masks_of_a_nested_sum():
    model, (k1, k2, k3) = _nested()
    h = model._ssm().h
    assert len(h) == 6
    mask = lambda *idx: np.where(np.isin(np.arange(6), idx), h, 0.0)  # noqa: E731
    assert np.array_equal(model._term_vector(k1), mask(0, 1))
    assert np.array_equal(model._term_vector(k2), mask(2, 3))
    assert np.array_equal(model._term_vector(k3), mask(4, 5))
    assert np.array_equal(model._term_vector(model.kernel1), mask(0, 1, 2, 3))  # the inner Sum node itself
    assert np.array_equal(model._term_vector(model), h)
    assert model._addends() == [k1, k2, k3]
    assert np.all(model._term_vector(k3)[4:] != 0)  # the Scale's factor sits in P, not in h


def test_term_vector_union_of_a_fresh_sum():
    model, (k1, k2, k3) = _nested()
    h = model._ssm().h
    want = h.copy()
    want[2:4] = 0.0
    assert np.array_equal(model._term_vector(k1 + k3), want)
    assert np.array_equal(model._term_vector(k3 + k1), want)
    assert np.array_equal(model._term_vector((k3 + k2) + k1), h)
    assert model._term_vector(k1 + q.Matern32(scale=1.5)) is None  # one addend is not in the model


def test_term_vector_of_non_terms_is_none():
    m32, cos, sho = q.Matern32(scale=1.5), q.Cosine(scale=3.0), q.SHO(omega=2.0, quality=3.0)
    scaled = 0.8 * sho
    model = m32 * cos + scaled
    assert model._term_vector(m32) is None and model._term_vector(cos) is None  # factors of a Product
    assert model._term_vector(sho) is None  # inside a Scale
    assert model._term_vector(q.Matern32(scale=1.5) * q.Cosine(scale=3.0)) is None  # equal-valued copy
    assert model._term_vector(0.8 * sho) is None
    assert model._term_vector(model.kernel1) is not None and model._term_vector(scaled) is not None
    # a kernel that is no sum has itself as its only term
    assert np.array_equal(m32._term_vector(m32), m32._ssm().h) and m32._addends() == [m32]
