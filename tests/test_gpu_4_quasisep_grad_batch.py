"""Value and gradient of batches of quasiseparable models over one series (``tgp_qsep_grad_batch``): every member
against the sequential oracle at the gradient's bars and, to the bit, against the device's own single
``value_and_grad`` on a fresh solver, whatever the batch size, the member's position, the shared or per-member form of
the inputs and the split into member chains and direction passes.

Inputs: ``_quasisep_edges.series`` and ``KERNELS``; member b has every parameter x (1 + 0.04 b) and the noise x
(1 + 0.1 b).  Bars (``test_gpu_4_quasisep_grad.py``): value 1e-8 relative; kernel 2e-6, noise 1e-6 and mean 1e-7 of
the largest reference entry.  References are computed once per (kernel, N, member) and never written to."""
import ctypes as C

import numpy as np
import pytest

from tinygp_amd import GaussianProcess, _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

import _quasisep_grad_np as og
from _quasisep_cases import CASES
from _quasisep_edges import KERNELS, grad_figures, series, shape
from _quasisep_grad_batch import grad_split, member_noise
from _quasisep_grad_batch import member as _case_member

pytestmark = pytest.mark.gpu

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _member(name, b):
    return _case_member(CASES, q, name, b)


def _single(k, t, noise, r):
    """The device's single call on a fresh solver: ``(value, kernel (P,), noise_diag (N,), mean (N,), info)``."""
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    try:
        v, g = s.value_and_grad(r)
        return v, np.asarray(g["kernel"], dtype=np.float64), g["noise_diag"], g["mean"], s.info
    finally:
        s.close()


def _row(result, b):
    """Member b of a ``value_and_grad_batch`` result, in the form of ``_single`` (without info)."""
    v, g = result[0], result[1]
    pick = lambda a: None if a is None else a[b]  # noqa: E731
    return v[b], g["kernel"][b], pick(g["noise_diag"]), pick(g["mean"])


def _same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


def _rows_same(x, y):
    return len(x) >= 4 and len(y) >= 4 and all(_same(a, b) for a, b in zip(x[:4], y[:4]))


def _batch_inputs(name, noise, nb, every=None):
    """Members b mod ``every`` (all distinct when None): ``(kernels, noises (B, N))``."""
    idx = [b if every is None else b % every for b in range(nb)]
    return [_member(name, i) for i in idx], np.stack([member_noise(noise, i) for i in idx])


def _raw(s, kernels, resid, noise, vectors=True):
    """The low-level call: ``(out, dout, gnoise, alpha, info, nchains, npasses)``; resid and noise (N,) or (B, N)."""
    leaves, smap, h, P = q.pack_batch(kernels)
    dleaves, dh, dP, _ = q.pack_batch_tangents(kernels)
    nb, ndir = len(kernels), dh.shape[1]
    resid, noise = np.ascontiguousarray(resid, dtype=np.float64), np.ascontiguousarray(noise, dtype=np.float64)
    info, out, dout = np.zeros(nb, dtype=np.int32), np.empty(nb), np.empty((nb, ndir))
    gnoise, alpha = (np.empty((nb, s.n)), np.empty((nb, s.n))) if vectors else (None, None)
    nchains, npasses = C.c_int32(-1), C.c_int32(-1)
    _ffi.check(_ffi.lib().tgp_qsep_grad_batch(
        s._handle, nb, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
        _ffi.ptr(noise), s.n if noise.ndim == 2 else 0, _ffi.ptr(resid), s.n if resid.ndim == 2 else 0, ndir,
        _ffi.ptr(dleaves), _ffi.ptr(dh), _ffi.ptr(dP), _ffi.ptr(info), _ffi.ptr(out), _ffi.ptr(dout), _ffi.ptr(gnoise),
        _ffi.ptr(alpha), C.byref(nchains), C.byref(npasses)), "tgp_qsep_grad_batch")
    return out, dout, gnoise, alpha, info, nchains.value, npasses.value


@pytest.fixture
def solver():
    """``solver(kernel, t, noise)``: a ``QuasisepSolver`` that is closed when the test ends, passed or failed."""
    made = []

    def make(kernel, t, noise):
        made.append(QuasisepSolver(kernel, t, Diagonal(noise), assume_sorted=True))
        return made[-1]
    yield make
    for s in made:
        s.close()


# -- 1. parity and bits at the scan's edges ----------------------------------------------------------------------------
def _reference(name, n, b):
    """``(oracle, single call)`` of member b of case ``name`` at n points; computed once, shared by every batch size."""
    def make():
        t, noise, r = series(n)
        k, nz = _member(name, b), member_noise(noise, b)
        return tuple(og.value_and_grad(k, t, nz, r)), _single(k, t, nz, r)
    return _once((name, n, b), make)


@pytest.mark.parametrize("n", [15, 16, 17, 1024, 1025, 4097])
@pytest.mark.parametrize("name", KERNELS)
def test_parity_and_bits(solver, name, n):
    """One short chunk, one full chunk, a second chunk of one step, 64 chunks, a second scan group of one chunk of one
    step and five groups; P = 2 (one pass), 7 (a ragged pass) and 16 (two full passes); B = 1, 2, 3."""
    assert shape(n)[0] == {15: 1, 16: 1, 17: 2, 1024: 64, 1025: 65, 4097: 257}[n]
    t, noise, r = series(n)
    s = solver(_member(name, 0), t, noise)
    for nb in (1, 2, 3):
        ks, nz = _batch_inputs(name, noise, nb)
        got = s.value_and_grad_batch(ks, r, nz, return_info=True)
        values, g, info = got
        npar = len(ks[0].parameters())
        assert values.shape == (nb,) and values.dtype == np.float64 and not info.any()
        assert g["kernel"].shape == (nb, npar) and g["noise_diag"].shape == g["mean"].shape == (nb, n)
        assert g["transform"] is None
        for b in range(nb):
            oracle, single = _reference(name, n, b)
            row = _row(got, b)
            v, ke, ne, me = grad_figures((row[0], {"kernel": row[1], "noise_diag": row[2], "mean": row[3]}), oracle)
            print(f"{name} n={n} B={nb} member {b}: value rel {v:.2e}; kernel {ke:.2e}, noise {ne:.2e}, mean {me:.2e} "
                  f"of max")
            assert single[4] == 0
            assert v <= 1e-8 and ke <= 2e-6 and ne <= 1e-6 and me <= 1e-7
            assert _rows_same(row, single), (nb, b)


# -- 2. position and size independence ---------------------------------------------------------------------------------
def test_position_and_batch_size_do_not_matter(solver):
    n, name = 257, "m32cos_plus_sho"
    t, noise, r = series(n, seed=21)
    probe, probe_noise = _member(name, 7), member_noise(noise, 7)
    want = _single(probe, t, probe_noise, r)
    assert want[4] == 0 and np.isfinite(want[0])
    s = solver(_member(name, 0), t, noise)
    for nb in (2, 5, 65):
        for pos in sorted({0, nb // 2, nb - 1}):
            ks, nz = _batch_inputs(name, noise, nb, every=11)
            ks[pos], nz[pos] = probe, probe_noise
            got = s.value_and_grad_batch(ks, r, nz)
            assert _rows_same(_row(got, pos), want), (nb, pos)


# -- 3. the boundary between two member chains -------------------------------------------------------------------------
def test_sixty_five_members_run_as_two_chains(solver):
    n, name, nb = 40, "matern32", 65
    t, noise, r = series(n, seed=22)
    ks, nz = _batch_inputs(name, noise, nb, every=13)
    s = solver(ks[0], t, noise)
    out, dout, gnoise, alpha, info, nchains, npasses = _raw(s, ks, r, nz)
    want = grad_split(n, 2, 2, nb, True, False, True)
    assert nchains == want.chains == 2 and npasses == want.passes == 2 and not info.any()
    for b in (62, 63, 64):
        assert _rows_same((out[b], dout[b], gnoise[b], alpha[b]), _single(ks[b], t, nz[b], r)), b
    for a in (out, dout, gnoise, alpha):
        assert np.all(np.isfinite(a))


# -- 4. the memory cap drives the split --------------------------------------------------------------------------------
def test_memory_cap_cuts_the_direction_passes(solver):
    """N = 2^20, J = 8, P = 16, three members with their own noise and residual: the 1 GiB cap leaves fewer than 8
    directions per pass.  Members 0 and 2 are held to their single calls bitwise; there is no oracle at this size (the
    sequential one takes minutes per member here, which a test of a few seconds cannot afford), member 1 is checked
    for finiteness only."""
    n, name, nb = 1 << 20, "celerite4", 3
    t, noise, r = series(n, seed=23)
    ks, nz = _batch_inputs(name, noise, nb)
    rs = np.stack([r * (1.0 + 0.01 * b) for b in range(nb)])
    s = solver(ks[0], t, noise)
    out, dout, gnoise, alpha, info, nchains, npasses = _raw(s, ks, rs, nz)
    want = grad_split(n, 8, 16, nb, True, True, True)
    print(f"N = 2^20, J = 8, P = 16, B = 3: {nchains} chains, {npasses} passes; the rule: {want}")
    assert (nchains, npasses) == (want.chains, want.passes) and not info.any()
    assert npasses > -(-16 // 8) * nchains
    for a in (out, dout, gnoise, alpha):
        assert np.all(np.isfinite(a))
    for b in (0, 2):
        assert _rows_same((out[b], dout[b], gnoise[b], alpha[b]), _single(ks[b], t, nz[b], rs[b])), b


def test_one_member_beyond_the_cap_is_refused():
    """The check precedes every allocation: at n = 12 000 000, J = 8 one member needs more than 11 n doubles next to the
    2 n of the shared noise and residual, more than 2^27 doubles together, with the vectors or without."""
    n = 12_000_000
    assert grad_split(n, 8, 16, 1, False, False, True).members == 0
    assert grad_split(n, 8, 16, 1, False, False, False).members == 0
    t = np.arange(n, dtype=np.float64)
    s = QuasisepSolver(_member("celerite4", 0), t, Diagonal(np.ones(n)), assume_sorted=True)
    try:
        for vectors in (True, False):
            with pytest.raises(ValueError, match="exceeds its cap"):
                s.value_and_grad_batch([_member("celerite4", 1)], np.zeros(n), vectors=vectors)
    finally:
        s.close()


# -- 5. shared against per-member arrays -------------------------------------------------------------------------------
def test_shared_and_copied_inputs_give_the_same_bits(solver):
    n, name, nb = 1025, "m32cos_plus_sho", 4
    t, noise, r = series(n, seed=24)
    ks = [_member(name, b) for b in range(nb)]
    s = solver(ks[0], t, noise)
    shared = s.value_and_grad_batch(ks, r, noise)

    def same(res):
        return all(_rows_same(_row(res, b), _row(shared, b)) for b in range(nb))

    assert same(s.value_and_grad_batch(ks, r))  # the solver's own noise
    assert same(s.value_and_grad_batch(ks, np.tile(r, (nb, 1)), np.tile(noise, (nb, 1))))
    assert same(s.value_and_grad_batch(ks, np.tile(r, (nb, 1)), noise))
    assert same(s.value_and_grad_batch(ks, r, np.tile(noise, (nb, 1))))
    rs = np.stack([r + 0.1 * b * np.cos(t) for b in range(nb)])
    got = s.value_and_grad_batch(ks, rs, noise)
    for b in range(nb):
        assert _rows_same(_row(got, b), _single(ks[b], t, noise, rs[b])), b
    assert shared[0][0] == got[0][0] and np.all(shared[0][1:] != got[0][1:])
    bare = s.value_and_grad_batch(ks, rs, noise, vectors=False)
    assert bare[1]["noise_diag"] is None and bare[1]["mean"] is None and bare[1]["transform"] is None
    assert _same(bare[0], got[0]) and _same(bare[1]["kernel"], got[1]["kernel"])


# -- 6. one failing member ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 2, 4])
def test_one_failing_member_touches_no_other(solver, pos):
    """noise[k] = -10 with k(0) = 1.44 < 10: since h^T P^- h <= k(0), pivot k is negative whatever precedes it.  The
    step is the first, one inside a later chunk or the last, by the member's position."""
    n, name, nb = 1025, "matern32", 5
    k_bad = {0: 0, 2: 500, 4: 1024}[pos]
    t, noise, r = series(n, seed=26)
    ks, nz = _batch_inputs(name, noise, nb)
    ssm = ks[pos]._lower_ssm()
    assert float(ssm.h @ ssm.Pinf @ ssm.h) < 10.0
    s = solver(ks[0], t, noise)
    keep = [b for b in range(nb) if b != pos]
    clean = s.value_and_grad_batch([ks[b] for b in keep], r, nz[keep], return_info=True)
    assert not clean[2].any() and np.all(np.isfinite(clean[0]))
    bad = nz.copy()
    bad[pos, k_bad] = -10.0
    got = s.value_and_grad_batch(ks, r, bad, return_info=True)
    assert list(got[2]) == [k_bad + 1 if b == pos else 0 for b in range(nb)]
    v, gk, gn, gm = _row(got, pos)
    assert v == -np.inf and np.all(np.isnan(gk)) and np.all(np.isnan(gn)) and np.all(np.isnan(gm))
    for i, b in enumerate(keep):
        assert _rows_same(_row(got, b), _row(clean, i)), b
    out, dout, gnoise, alpha, info, _, _ = _raw(s, ks, r, bad)
    assert info[pos] == k_bad + 1 and np.isnan(out[pos])
    assert np.all(np.isnan(dout[pos])) and np.all(np.isnan(gnoise[pos])) and np.all(np.isnan(alpha[pos]))
    for i, b in enumerate(keep):
        assert _rows_same((out[b], dout[b], gnoise[b], alpha[b]), _row(clean, i)), b


# -- 7. the handle's resident state is left alone ----------------------------------------------------------------------
def test_handle_is_untouched(solver):
    n = 1025
    t, noise, r = series(n, seed=27)
    own = _member("m32cos_plus_sho", 0)
    xt = np.linspace(t[0] - 1.0, t[-1] + 1.0, 50)
    s = solver(own, t, noise)

    def snapshot():
        lp = s.log_probability(r)
        v, g = s.value_and_grad(r)
        mean, var = s.predict_mean_var(r, xt)
        return lp, v, np.asarray(g["kernel"]), g["noise_diag"], g["mean"], mean, var, s.info

    before = snapshot()
    ssm = s._ssm
    others, nz = _batch_inputs("celerite4", noise, 3)
    nz[1, 500] = -100.0
    got = s.value_and_grad_batch(others, 2.0 * r, nz, return_info=True)
    assert list(got[2]) == [0, 501, 0] and got[0][1] == -np.inf and np.isfinite(got[0][0]) and np.isfinite(got[0][2])
    assert s.kernel is own and s._ssm is ssm and s._info == 0 and s._factored
    # the resident factor and alpha, before anything refactors
    mean, var = s.predict_mean_var(r, xt)
    assert _same(mean, before[5]) and _same(var, before[6])
    after = snapshot()
    assert all(_same(a, b) for a, b in zip(before, after))

    lazy = solver(own, t, noise)
    assert not lazy._factored
    got2 = lazy.value_and_grad_batch(others, 2.0 * r, nz, return_info=True)
    assert all(_rows_same(_row(got2, b), _row(got, b)) for b in range(3)) and not lazy._factored
    out = C.c_double()
    assert _ffi.lib().tgp_qsep_normalization(lazy._handle, C.byref(out)) != 0  # the handle itself: not factored
    assert _same(lazy.log_probability(r), before[0])


# -- 8. damping regimes mixed in one batch -----------------------------------------------------------------------------
def test_mixed_damping_regimes(solver):
    n = 1025
    t, noise, r = series(n, seed=25)
    ks = [CASES[name](q) for name in ("sho_under", "sho_over", "sho_crit")]
    assert len({int(k._lower_ssm().leaves[0, 0]) for k in ks}) == 3
    iq = [attr for _, attr in ks[0].parameters()].index("quality")
    s = solver(ks[0], t, noise)
    for order in ([0, 1, 2], [2, 0, 1]):
        got = s.value_and_grad_batch([ks[i] for i in order], r, return_info=True)
        assert not got[2].any()
        nan = np.isnan(got[1]["kernel"])
        want = np.zeros_like(nan)
        want[order.index(2), iq] = True
        assert np.array_equal(nan, want)
        for b, i in enumerate(order):
            single = _single(ks[i], t, noise, r)
            assert _rows_same(_row(got, b), single), (order, b)
            wll, wg, wgn, walpha = _once(("sho", i), lambda: tuple(og.value_and_grad(ks[i], t, noise, r)))
            keep = ~nan[b]
            assert got[0][b] == pytest.approx(wll, rel=1e-8)
            assert np.abs(got[1]["kernel"][b][keep] - wg[keep]).max() <= 2e-6 * np.abs(wg[keep]).max()


# -- 9. the GP level ---------------------------------------------------------------------------------------------------
def _gp_rows_same(got, b, want):
    v, g = want
    return _rows_same(_row(got, b), (v, np.asarray(g["kernel"], dtype=np.float64), g["noise_diag"], g["mean"]))


def test_gp_batch_equals_separate_gps():
    n, name, nb = 1000, "m32cos_plus_sho", 4
    t, _, y = series(n, seed=28)
    ks = [_member(name, b) for b in range(nb)]
    diags = np.array([0.1, 0.15, 0.2, 0.05])
    means = np.array([0.0, 0.3, -0.2, 1.5])
    gp = GaussianProcess(ks[0], t, diag=0.1)
    got = gp.log_probability_and_grad_batch(y, ks, diags=diags, means=means)
    assert got[0].shape == (nb,) and got[0].dtype == np.float64 and got[1]["kernel"].shape == (nb, 7)
    for b in range(nb):
        want = GaussianProcess(ks[b], t, diag=diags[b], mean=means[b]).log_probability_and_grad(y)
        assert _gp_rows_same(got, b, want), b
    # (B, N) forms of the same inputs, and the GP's own mean and noise
    full = gp.log_probability_and_grad_batch(y, ks, diags=np.repeat(diags[:, None], n, 1),
                                             means=np.repeat(means[:, None], n, 1))
    assert all(_rows_same(_row(full, b), _row(got, b)) for b in range(nb))
    assert _gp_rows_same(gp.log_probability_and_grad_batch(y, ks), 0, gp.log_probability_and_grad(y))


def test_gp_batch_dtypes_empty_and_other_solvers():
    n, name = 300, "matern32"
    t, _, y = series(n, seed=29)
    ks = [_member(name, b) for b in range(3)]
    t32, y32 = t.astype(np.float32), y.astype(np.float32)
    d32 = np.array([0.1, 0.2, 0.3], dtype=np.float32)
    gp32 = GaussianProcess(ks[0], t32, diag=np.float32(0.1))
    got = gp32.log_probability_and_grad_batch(y32, ks, diags=d32)
    assert got[0].dtype == np.float32 and got[0].shape == (3,)
    assert got[1]["noise_diag"].dtype == got[1]["mean"].dtype == np.float32 and got[1]["kernel"].dtype == np.float64
    for b, d in enumerate(d32):
        assert _gp_rows_same(got, b, GaussianProcess(ks[b], t32, diag=d).log_probability_and_grad(y32)), b
    gp = GaussianProcess(ks[0], t, diag=0.1)
    values, grads = gp.log_probability_and_grad_batch(y, [])
    assert values.shape == (0,) and values.dtype == np.float64
    assert grads["kernel"].shape == (0, 2) and grads["noise_diag"].shape == grads["mean"].shape == (0, n)
    values, grads, info = gp.solver.value_and_grad_batch([], y, vectors=False, return_info=True)
    assert values.shape == (0,) and info.shape == (0,) and grads["noise_diag"] is None and grads["mean"] is None
    dense = GaussianProcess(ks[0], t, diag=0.1, solver=DirectSolver)
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.log_probability_and_grad_batch(y, ks)
    with pytest.raises(ValueError, match="kernel 1"):
        gp.log_probability_and_grad_batch(y, [ks[0], q.Matern52(1.0)])
    with pytest.raises(ValueError, match="kernel 1 .*parameters"):
        gp.log_probability_and_grad_batch(y, [ks[0], 2.0 * q.Matern32(1.0)])
    with pytest.raises(ValueError, match="resid must have shape"):
        gp.solver.value_and_grad_batch(ks, np.zeros((2, n)))


# -- 10. determinism ---------------------------------------------------------------------------------------------------
def test_same_batch_twice_is_bit_identical(solver):
    n, name, nb = 4097, "celerite4", 7
    t, noise, r = series(n, seed=30)
    ks, nz = _batch_inputs(name, noise, nb)
    s = solver(ks[0], t, noise)
    a, b = s.value_and_grad_batch(ks, r, nz), s.value_and_grad_batch(ks, r, nz)
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]["kernel"]))
    assert all(_rows_same(_row(a, i), _row(b, i)) for i in range(nb))
