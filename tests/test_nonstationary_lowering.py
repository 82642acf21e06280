"""Lowering of DotProduct / Polynomial (reference kernels/base.py:212-256) to the DOT leaf and the
unary POW of the kernel program (include/tgp_hip.h), and the host logic around it.  No device:
these run everywhere."""
import re
from pathlib import Path

import numpy as np
import pytest

import _nonstationary_np as nsn
from tinygp_amd import _device, transforms
from tinygp_amd.kernels import base
from tinygp_amd import kernels

ROOT = Path(__file__).resolve().parent.parent


def test_op_codes_match_the_header():
    h = (ROOT / "include" / "tgp_hip.h").read_text()
    assert int(re.search(r"TGP_K_DOT = (\d+)", h).group(1)) == base.K_DOT == 8
    assert int(re.search(r"TGP_K_POW = (\d+)", h).group(1)) == base.K_POW == 18


def test_leaf_programs_and_parameters():
    assert kernels.DotProduct().program() == [(base.K_DOT, 0, 1.0, 0.0)]
    assert kernels.DotProduct().parameters() == []
    p = kernels.Polynomial(order=3, scale=2.0, sigma=0.7)
    assert p.program() == [(base.K_DOT, 0, 2.0, 0.7), (base.K_POW, 0, 3.0, 0.0)]
    assert p.parameters() == [(p, "scale"), (p, "sigma"), (p, "order")]
    assert kernels.Polynomial(order=2).program() == [(base.K_DOT, 0, 1.0, 0.0), (base.K_POW, 0, 2.0, 0.0)]


@pytest.mark.parametrize("name", ["order", "scale", "sigma"])
def test_non_scalar_polynomial_parameters_raise(name):
    args = dict(order=2.0, scale=1.5, sigma=0.3)
    args[name] = np.array([1.0, 2.0])
    with pytest.raises(ValueError):
        kernels.Polynomial(**args).program()


def test_trees_lower_with_parameters_in_program_order():
    X = np.random.default_rng(0).normal(size=(7, 3))
    a, b, e = kernels.Constant(1.5**2), kernels.Constant(0.3), kernels.ExpSquared(2.5)
    d = kernels.DotProduct()
    k = a * e + b * d
    prog, P = k._lower(X)
    assert [o[0] for o in prog] == [base.K_CONST, base.K_EXPSQ, base.K_MUL, base.K_CONST, base.K_DOT, base.K_MUL,
                                    base.K_ADD]
    assert P is X
    assert k.parameters() == [(a, "value"), (e, "scale"), (b, "value")]

    p, m = kernels.Polynomial(order=2, scale=1.3, sigma=0.4), kernels.Matern32(1.2)
    k = p * m
    prog, _ = k._lower(X)
    assert prog == [(base.K_DOT, 0, 1.3, 0.4), (base.K_POW, 0, 2.0, 0.0), (base.K_M32, 0, 1.2, 0.0),
                    (base.K_MUL, 0, 0.0, 0.0)]
    assert k.parameters() == [(p, "scale"), (p, "sigma"), (p, "order"), (m, "scale")]

    s = np.array([0.5, 2.0, 1.5])
    p = kernels.Polynomial(order=3, scale=1.1, sigma=0.2)
    k = transforms.Linear(s, p)
    prog, P = k._lower(X)
    assert prog == [(base.K_DOT, 0, 1.1, 0.2), (base.K_POW, 0, 3.0, 0.0)]
    np.testing.assert_array_equal(P, X * s)
    assert k.parameters() == [(p, "scale"), (p, "sigma"), (p, "order")]
    assert transforms.covering_transform(k) is k
    # a bare dot product beside the transform sees the raw coordinates: no transform gradient
    assert transforms.covering_transform(k + kernels.DotProduct()) is None


def test_stack_depth_counts_pow_as_unary():
    """POW leaves the depth unchanged: eight right-nested polynomials need a stack of 8 (the device's
    limit), nine need 9 and go to the host route."""
    def nest(m):
        k = kernels.Polynomial(order=2, sigma=0.1)
        for _ in range(m - 1):
            k = kernels.Polynomial(order=2, sigma=0.1) + k
        return k

    X = np.ones((3, 2))
    prog, _ = nest(8)._lower(X)
    assert base._stack_peak(prog) == 8 and len(prog) == 23
    assert nest(8).program() == prog
    with pytest.raises(_device.DeviceLimit):
        nest(9).program()
    with pytest.raises(_device.DeviceLimit):
        nest(9)._lower(X)
    # a POW over constants is a constant operand (no coordinates): Constant ** order has no program of
    # its own, but the test in _lower_binary treats [CONST, POW] like [CONST]
    assert base._stack_peak([(base.K_CONST, 0, 2.0, 0.0), (base.K_POW, 0, 3.0, 0.0)]) == 1


def _cases():
    rng = np.random.default_rng(3)
    X1, X2 = rng.normal(size=(11, 4)), rng.normal(size=(9, 4))
    return X1, X2, {
        "dot": (kernels.DotProduct(), X1 @ X2.T),
        "poly3": (kernels.Polynomial(order=3, scale=2.0, sigma=0.0), ((X1 / 2.0) @ (X2 / 2.0).T) ** 3),
        "poly2.5": (kernels.Polynomial(order=2.5, scale=2.0, sigma=3.0),
                    ((X1 / 2.0) @ (X2 / 2.0).T + 9.0) ** 2.5),
        "expsq+dot": (1.5**2 * kernels.ExpSquared(2.5) + 0.3 * kernels.DotProduct(),
                      1.5**2 * np.exp(-0.5 * np.sum((X1[:, None] - X2[None]) ** 2, -1) / 2.5**2) + 0.3 * X1 @ X2.T),
        "poly*m32": (kernels.Polynomial(order=2, scale=1.3, sigma=0.4) * kernels.Matern32(1.2),
                     ((X1 / 1.3) @ (X2 / 1.3).T + 0.16) ** 2
                     * (1 + np.sqrt(3) * np.sum(np.abs(X1[:, None] - X2[None]), -1) / 1.2)
                     * np.exp(-np.sqrt(3) * np.sum(np.abs(X1[:, None] - X2[None]), -1) / 1.2)),
    }


@pytest.mark.parametrize("name", ["dot", "poly3", "poly2.5", "expsq+dot", "poly*m32"])
def test_numpy_program_evaluator_matches_the_reference_formulas(name):
    X1, X2, cases = _cases()
    k, want = cases[name]
    prog, _ = k._lower(X1)
    got = nsn.eval_prog(prog, X1, X2)
    order = max([o[2] for o in prog if o[0] == base.K_POW], default=1.0)
    bar = nsn.dot_bar(prog, X1, X2) ** order
    assert np.all(np.abs(got - want) <= 1e-14 * order * np.maximum(bar, np.abs(want)))
    # the bare leaves called directly keep the host formulas (no device involved)
    if name in ("dot", "poly3", "poly2.5"):
        np.testing.assert_allclose(k(X1, X2), want, rtol=1e-14)


def test_polynomial_keeps_the_sign_of_a_negative_base_for_integer_orders():
    X1 = np.array([[1.0, -2.0]])
    X2 = np.array([[3.0, 1.0]])
    prog = kernels.Polynomial(order=3).program()
    assert nsn.eval_prog(prog, X1, X2)[0, 0] == (1.0 * 3.0 - 2.0) ** 3 == 1.0
    X2 = np.array([[-3.0, 1.0]])
    assert nsn.eval_prog(prog, X1, X2)[0, 0] == -125.0


def test_beyond_the_device_limits_stays_on_the_host():
    """D = 20 and pytree inputs: DeviceLimit from _lower, the host route for the values."""
    rng = np.random.default_rng(5)
    X1, X2 = rng.normal(size=(6, 20)), rng.normal(size=(5, 20))
    k = 0.5 * kernels.ExpSquared(9.0) + kernels.Polynomial(order=2, scale=3.0, sigma=1.0)
    for kk in (kernels.DotProduct(), kernels.Polynomial(order=2), k):
        with pytest.raises(_device.DeviceLimit):
            kk._lower(X1)
    want = (0.5 * np.exp(-0.5 * np.sum((X1[:, None] - X2[None]) ** 2, -1) / 81.0)
            + ((X1 / 3.0) @ (X2 / 3.0).T + 1.0) ** 2)
    np.testing.assert_allclose(k(X1, X2), want, rtol=1e-13)
    np.testing.assert_allclose(base.host_diag(k, X1), np.diag(0.5 + ((X1 / 3.0) @ (X1 / 3.0).T + 1.0) ** 2),
                               rtol=1e-13)
    tree = (np.linspace(0.0, 1.0, 5), np.arange(5.0))
    with pytest.raises(_device.DeviceLimit):
        kernels.DotProduct()._lower(tree)
