"""Value AND gradient of batches of small dense GPs in one launch, one workgroup per member (``csrc/small.hip``,
``tgp_small_logprob_grad``) through ``DirectSolver.log_probability_and_grad_batch`` and
``log_probability_and_grad_datasets``.

Inputs and references: ``_dense_small_grad.py`` (float64 LAPACK with analytic dK/dtheta, its own conditions asserted)
and, for every leaf and operator, the single path ``GaussianProcess.log_probability_and_grad``, which existing tests
hold to analytic references.  Bars: the project's fp64 bars (ll 1e-8, kernel 2e-6, noise 1e-6, mean 1e-7; each rtol
plus the same fraction of the largest component as atol); value bits, independence and the routes to the single path
are held with tolerance zero."""
import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, kernels, transforms
from tinygp_amd.kernels import quasisep
from tinygp_amd.noise import Dense, Diagonal
from tinygp_amd.solvers import DirectSolver, small

import _dense_grad_np as dg
import _dense_small as ds
import _dense_small_grad as sg

pytestmark = pytest.mark.gpu

CAP = ds.CAP


def _inputs(name, n):
    X, diag, y = dg.inputs(n, sg.dim(name))
    return X, diag, y


def _batch(name, n, members, *, noise=None, resid=None, **kwargs):
    """The solver's batch of the given members (indices b) of program ``name`` at ``_dense_grad_np.inputs(n, d)``."""
    X, diag, y = _inputs(name, n)
    solver = DirectSolver(sg.member_kernel(name, kernels, 0), X, Diagonal(diag))
    try:
        ks = [sg.member_kernel(name, kernels, b) for b in members]
        nz = np.stack([sg.member_noise(name, n, b) for b in members]) if noise is None else noise
        return solver.log_probability_and_grad_batch(ks, y if resid is None else resid, nz, **kwargs)
    finally:
        solver.close()


def _datasets(name, ns, members, **kwargs):
    ks = [sg.member_kernel(name, kernels, b) for b in members]
    return tinygp_amd.log_probability_and_grad_datasets(
        ks, [_inputs(name, n)[0] for n in ns], [_inputs(name, n)[2] for n in ns],
        diags=[sg.member_noise(name, n, b) for n, b in zip(ns, members)], **kwargs)


def _member(values, grads, m):
    """Member m of a result as one tuple of arrays: value, kernel, transform, noise, mean."""
    noise, mean = grads["noise_diag"], grads["mean"]
    return (np.asarray(values[m]), np.asarray(grads["kernel"][m]),
            None if grads["transform"][m] is None else np.asarray(grads["transform"][m]),
            None if noise is None else np.asarray(noise[m]), None if mean is None else np.asarray(mean[m]))


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert (x is None) == (y is None), what
        if x is not None:
            assert np.array_equal(x, y, equal_nan=True), (what, x, y)


def _check(ref, member, what, worst):
    value, kgrad, tgrad, noise, mean = member
    e = sg.errors(ref, value, sg.full_gradient(kgrad, tgrad), noise, mean)
    for key, v in e.items():
        worst[key] = max(worst.get(key, 0.0), v)
    sg.check(ref, value, sg.full_gradient(kgrad, tgrad), noise, mean)
    assert kgrad.dtype == np.float64 and kgrad.shape == (dg.N_KERNEL[ref.name],), what


# ---- 1. parity with the analytic reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.NAMES)
@pytest.mark.parametrize("n", ds.EDGE_NS)
def test_parity_with_the_analytic_reference_at_the_edges(n, name):
    worst = {}
    for B in sg.BS:
        values, grads, info = _batch(name, n, range(B), return_info=True)
        assert values.shape == (B,) and values.dtype == np.float64 and not info.any()
        assert grads["noise_diag"].shape == grads["mean"].shape == (B, n)
        sets = _datasets(name, [n] * B, range(B))
        for b in range(B):
            _check(sg.reference(name, n, b), _member(values, grads, b), f"{name} n={n} B={B} member {b}", worst)
            _same_bits(_member(values, grads, b), _member(*sets, b), f"{name} n={n} B={B} data set {b}")
            assert (grads["transform"][b] is not None) == (name == "linear")
    print(f"{name} n={n}: worst error in bars " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 2. every leaf and operator against the single path ---------------------------------------------------------------------
@pytest.mark.parametrize("D", ds.LEAF_DS)
def test_every_leaf_and_operator_against_the_single_path(D):
    members = ds.leaf_members(kernels, transforms)
    X, n, y = ds.leaf_points(D), ds.LEAF_N, ds.resid(ds.LEAF_N)
    noise = np.stack([ds.leaf_noise() * (1.0 + 0.1 * b) for b in range(len(members))])
    ks = [k for _, k, _ in members]
    solver = DirectSolver(ks[1], X, Diagonal(ds.leaf_noise()))
    try:
        assert small.batch_route(n, True, [small.lower_member(k, X) for k in ks])  # one launch
        values, grads, info = solver.log_probability_and_grad_batch(ks, y, noise, return_info=True)
        plain = solver.log_probability_batch(ks, y, noise)
    finally:
        solver.close()
    assert not info.any() and np.array_equal(values, plain)
    b = sg.BARS
    worst = {}
    for m, (name, k, _) in enumerate(members):
        gp = GaussianProcess(k, X, diag=noise[m])
        want, g = gp.log_probability_and_grad(y)
        gp.solver.close()
        assert len(grads["kernel"][m]) == len(k.parameters()), name
        got_t, want_t = grads["transform"][m], g["transform"]
        assert (got_t is None) == (want_t is None), name
        pairs = [("ll", [values[m]], [want]), ("kernel", grads["kernel"][m], g["kernel"]),
                 ("noise", grads["noise_diag"][m], g["noise_diag"]), ("mean", grads["mean"][m], g["mean"])]
        if want_t is not None:
            pairs.append(("kernel", np.ravel(got_t), np.ravel(want_t)))
        for key, got, ref in pairs:
            if len(ref) == 0:  # (DotProduct: no parameters)
                continue
            worst[key] = max(worst.get(key, 0.0), dg.in_bars(got, ref, b[key], 0.0 if key == "ll" else b[key]))
            np.testing.assert_allclose(got, ref, rtol=b[key], atol=0.0 if key == "ll" else b[key] * np.abs(ref).max(),
                                       err_msg=f"D={D} {name} {key}")
    print(f"D={D}: worst error in bars " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 3. value bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.NAMES)
def test_values_have_the_bits_of_the_value_batch(name):
    for n in (1, 17, 65, CAP):
        X, diag, y = _inputs(name, n)
        ks = [sg.member_kernel(name, kernels, b) for b in range(3)]
        nz = np.stack([sg.member_noise(name, n, b) for b in range(3)])
        solver = DirectSolver(ks[0], X, Diagonal(diag))
        try:
            values, _ = solver.log_probability_and_grad_batch(ks, y, nz)
            plain = solver.log_probability_batch(ks, y, nz)
        finally:
            solver.close()
        assert np.array_equal(values, plain), (name, n, values, plain)


# ---- 4. independence, tolerance zero on every output ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.NAMES)
def test_a_members_bits_do_not_depend_on_the_batch(name):
    n, me = 8, 2
    alone = _member(*_batch(name, n, [me]), 0)
    sg.check(sg.reference(name, n, me), alone[0], sg.full_gradient(alone[1], alone[2]), alone[3], alone[4])
    _same_bits(alone, _member(*_batch(name, n, [me]), 0), "across two calls")
    for members in ([me, 0, 1], [0, me, 1], [0, 1, me]):  # first, middle and last of B = 3
        _same_bits(alone, _member(*_batch(name, n, members), members.index(me)), members)
    # inside B = 300 of mixed structures: every program at n = 8, each with coordinates of its own
    B = 300
    names = [sg.NAMES[m % len(sg.NAMES)] for m in range(B)]
    bs = [m % 7 for m in range(B)]
    at = [m for m in range(B) if names[m] == name][5]
    bs[at] = me
    ks = [sg.member_kernel(nm, kernels, b) for nm, b in zip(names, bs)]
    Xs = [np.asarray(_inputs(nm, n)[0], dtype=np.float64).reshape(n, -1) for nm in names]
    Xs = [np.hstack([X, np.zeros((n, 3 - X.shape[1]))]) for X in Xs]  # one D for the set: the 1-D programs get zeros
    mixed = tinygp_amd.log_probability_and_grad_datasets(
        ks, Xs, [_inputs(nm, n)[2] for nm in names], diags=[sg.member_noise(nm, n, b) for nm, b in zip(names, bs)])
    lone = tinygp_amd.log_probability_and_grad_datasets([ks[at]], [Xs[at]], [_inputs(name, n)[2]],
                                                        diags=[sg.member_noise(name, n, me)])
    _same_bits(_member(*lone, 0), _member(*mixed, at), "inside B = 300")
    assert np.all(np.isfinite(mixed[0]))
    if sg.dim(name) == 3:
        _same_bits(alone, _member(*lone, 0), "the same member through the two entry points")
    # beside a neighbour at the cap: the launch's LDS is sized by the larger member
    got = _datasets(name, [CAP, n, CAP], [0, me, 1])
    _same_bits(alone, _member(*got, 1), "beside a neighbour at the cap")
    big = _member(*got, 0)
    sg.check(sg.reference(name, CAP, 0), big[0], sg.full_gradient(big[1], big[2]), big[3], big[4])


# ---- 5. ragged sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.NAMES)
def test_ragged_sets_of_data_sets(name):
    ns = ds.RAGGED
    values, grads, info = _datasets(name, ns, range(len(ns)), return_info=True)
    assert values.shape == (len(ns),) and values.dtype == np.float64 and not info.any()
    worst = {}
    for b, n in enumerate(ns):
        got = _member(values, grads, b)
        assert got[3].shape == got[4].shape == (n,)
        _check(sg.reference(name, n, b), got, f"{name} data set {b} (n={n})", worst)
        _same_bits(got, _member(*_batch(name, n, [b]), 0), f"{name} data set {b} through the shared-X call")
    print(f"{name} ragged: worst error in bars " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 6. failure -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("fast", "linear"))
@pytest.mark.parametrize("n,p", ds.FAIL_CASES)
def test_failed_pivot_is_reported_and_stays_in_its_member(n, p, name):
    members = [0, 1, 2]
    good = np.stack([sg.member_noise(name, n, b) for b in members])
    clean = _batch(name, n, members, return_info=True)
    assert not clean[2].any()

    def all_nan(m):
        value, kgrad, tgrad, noise, mean = m
        return (np.all(np.isnan(kgrad)) and np.all(np.isnan(noise)) and np.all(np.isnan(mean))
                and (tgrad is None or np.all(np.isnan(tgrad))))

    for bad_value in (-2.0, np.nan):
        noise = np.array(good)
        noise[1, p] = bad_value  # the leading minor is positive definite, K_pp + noise_p < 0: pivot p + 1 fails
        values, grads, info = _batch(name, n, members, noise=noise, return_info=True)
        assert info.tolist() == [0, p + 1, 0], (bad_value, info)
        assert values[1] == -np.inf and all_nan(_member(values, grads, 1))
        assert (grads["transform"][1] is not None) == (name == "linear")
        for b in (0, 2):
            _same_bits(_member(*clean[:2], b), _member(values, grads, b), f"neighbour {b}")
    resid = np.tile(np.asarray(_inputs(name, n)[2]), (3, 1))
    resid[1, n // 2] = np.nan
    values, grads, info = _batch(name, n, members, resid=resid, return_info=True)
    assert info.tolist() == [0, 0, 0] and values[1] == -np.inf and all_nan(_member(values, grads, 1))
    for b in (0, 2):
        _same_bits(_member(*clean[:2], b), _member(values, grads, b), f"neighbour {b} of a NaN residual")


# ---- 7. routing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("fast", "linear"))
def test_above_the_cap_is_the_single_path(name):
    n = CAP + 1
    X, _, y = _inputs(name, n)
    values, grads, info = _batch(name, n, [0, 1], return_info=True)
    assert not info.any() and grads["noise_diag"].shape == (2, n)
    for b in range(2):
        gp = GaussianProcess(sg.member_kernel(name, kernels, b), X, diag=sg.member_noise(name, n, b))
        want, g = gp.log_probability_and_grad(y)
        gp.solver.close()
        single = (np.asarray(want), np.asarray(g["kernel"], dtype=np.float64),
                  None if g["transform"] is None else np.asarray(g["transform"]), g["noise_diag"], g["mean"])
        _same_bits(single, _member(values, grads, b), f"{name} member {b}")  # the same path: the same bits
        got = _member(values, grads, b)
        sg.check(sg.reference(name, n, b), got[0], sg.full_gradient(got[1], got[2]), got[3], got[4])
    # one such member among small ones: the order of the results is the caller's
    sets = _datasets(name, [17, n, 64], [2, 1, 0])
    _same_bits(_member(values, grads, 1), _member(*sets, 1), "a large data set among small ones")
    for m, (size, b) in enumerate(((17, 2), (n, 1), (64, 0))):
        got = _member(*sets, m)
        sg.check(sg.reference(name, size, b), got[0], sg.full_gradient(got[1], got[2]), got[3], got[4])


def test_members_the_device_cannot_lower_take_the_single_path():
    name, n = "m32c", 40
    X, diag, y = _inputs(name, n)
    custom = kernels.Custom(lambda a, b: 0.9 * np.exp(-0.5 * np.sum(np.square(a - b)) / 2.5**2))
    ks = [sg.member_kernel(name, kernels, 0), sg.member_kernel(name, kernels, 1)]
    solver = DirectSolver(ks[0], X, Diagonal(diag))
    try:
        with pytest.raises(NotImplementedError, match="on-device kernel program"):  # the single call's own answer
            solver.log_probability_and_grad_batch([ks[0], custom, ks[1]], y)
    finally:
        solver.close()
    sets = tinygp_amd.log_probability_and_grad_datasets(ks, [X, X], [y, y], diags=[diag, diag])
    # a noise model that is not Diagonal: every member on the single path, with that model
    N = np.diag(diag) + 0.01
    dense = GaussianProcess(ks[0], X, noise=Dense(N))
    values, grads = dense.solver.log_probability_and_grad_batch(ks, y)
    for b, k in enumerate(ks):
        gp = GaussianProcess(k, X, noise=Dense(N))
        want, g = gp.log_probability_and_grad(y)
        gp.solver.close()
        assert values[b] == want and np.array_equal(grads["kernel"][b], np.asarray(g["kernel"], dtype=np.float64))
        assert np.array_equal(grads["noise_diag"][b], g["noise_diag"]) and np.array_equal(grads["mean"][b], g["mean"])
        assert values[b] != sets[0][b]  # (another noise model: another number)
    dense.solver.close()


def test_quasisep_kernels_raise_the_pinned_error():
    t = np.sort(np.random.default_rng(3).uniform(0.0, 10.0, 30))
    ks = [quasisep.Matern32(1.0 + 0.1 * b) for b in range(2)]
    dense = GaussianProcess(ks[0], t, diag=0.1, solver=DirectSolver)
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.solver.log_probability_and_grad_batch(ks, np.zeros(30))
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.solver.log_probability_and_grad_batch([kernels.Matern32(1.0), ks[1]], np.zeros(30))
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        tinygp_amd.log_probability_and_grad_datasets(ks[0], [t], [np.zeros(30)], diags=[0.1])
    with pytest.raises(NotImplementedError, match="QuasisepSolver.*log_probability_and_grad_datasets"):
        dense.log_probability_and_grad_batch(np.zeros(30), [kernels.Matern32(1.0)])
    dense.solver.close()


# ---- 8. output details ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ess", "linear"))
def test_output_details(name):
    n, B = 65, 3
    full = _batch(name, n, range(B), return_info=True)
    bare = _batch(name, n, range(B), vectors=False, return_info=True)
    assert bare[1]["noise_diag"] is None and bare[1]["mean"] is None
    assert np.array_equal(full[0], bare[0]) and np.array_equal(full[2], bare[2]) and full[2].dtype == np.int32
    for b in range(B):
        _same_bits(_member(*full[:2], b)[:3], _member(*bare[:2], b)[:3], f"vectors=False member {b}")
    sets = _datasets(name, [n] * B, range(B), vectors=False)
    assert sets[1]["noise_diag"] is None and sets[1]["mean"] is None and np.array_equal(sets[0], full[0])
    # B = 0
    X, diag, y = _inputs(name, n)
    solver = DirectSolver(sg.member_kernel(name, kernels, 0), X, Diagonal(diag))
    try:
        values, grads, info = solver.log_probability_and_grad_batch([], y, return_info=True)
        assert values.shape == (0,) and values.dtype == np.float64 and info.shape == (0,) and info.dtype == np.int32
        assert grads["kernel"] == [] and grads["transform"] == []
        assert grads["noise_diag"].shape == grads["mean"].shape == (0, n) and grads["mean"].dtype == np.float64
        values, grads = solver.log_probability_and_grad_batch([], y, vectors=False)
        assert values.shape == (0,) and grads["noise_diag"] is None and grads["mean"] is None
        with pytest.raises(ValueError, match="resid must have shape"):
            solver.log_probability_and_grad_batch([solver.kernel] * 3, np.zeros((2, n)))
    finally:
        solver.close()


@pytest.mark.parametrize("name", ("fast", "linear"))
def test_fp32_inputs_are_computed_in_fp64_and_returned_as_fp32(name):
    n, B = 65, 3
    X32, diag32, y32 = dg.inputs(n, sg.dim(name), "float32")
    ks = [sg.member_kernel(name, kernels, b) for b in range(B)]
    solver = DirectSolver(ks[0], X32, Diagonal(diag32))
    assert solver.dtype == np.float32
    try:
        values, grads = solver.log_probability_and_grad_batch(ks, y32)
        empty, _ = solver.log_probability_and_grad_batch([], y32)
    finally:
        solver.close()
    assert values.dtype == np.float32 and empty.dtype == np.float32
    assert grads["noise_diag"].dtype == grads["mean"].dtype == np.float32
    assert all(k.dtype == np.float64 for k in grads["kernel"])
    # the same numbers as the float64 call on the rounded inputs, rounded once
    solver = DirectSolver(ks[0], X32.astype(np.float64), Diagonal(diag32.astype(np.float64)))
    try:
        v64, g64 = solver.log_probability_and_grad_batch(ks, y32.astype(np.float64))
    finally:
        solver.close()
    assert np.array_equal(values, v64.astype(np.float32))
    assert np.array_equal(grads["noise_diag"], g64["noise_diag"].astype(np.float32))
    assert np.array_equal(grads["mean"], g64["mean"].astype(np.float32))
    for b in range(B):
        assert np.array_equal(grads["kernel"][b], g64["kernel"][b])
    sets = tinygp_amd.log_probability_and_grad_datasets(ks, [X32] * B, [y32] * B, diags=[diag32] * B)
    assert sets[0].dtype == np.float64 and sets[1]["mean"][0].dtype == np.float32
    assert np.array_equal(sets[0], v64) and np.array_equal(sets[1]["mean"][1], grads["mean"][1])
