"""Batches of quasiseparable models over one series (``tgp_qsep_logprob_batch``): every member against the sequential
oracle and, to the bit, against the device's own single call, whatever the batch size and the member's position."""
import ctypes as C
import functools

import numpy as np
import pytest

from tinygp_amd import GaussianProcess, _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

import _quasisep_np as o
from _quasisep_cases import CASES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _series(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    out = t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)
    for a in out:
        a.setflags(write=False)
    return out


def _member(name, b):
    """Case ``name`` with every parameter scaled by 1 + 0.04 b: member b of a batch (b = 0: the case itself)."""
    k = CASES[name](q)
    for obj, attr in k.parameters():
        setattr(obj, attr, getattr(obj, attr) * (1.0 + 0.04 * b))
    return k


def _member_noise(noise, b):
    return noise * (1.0 + 0.1 * b)


def _single(k, t, noise, r):
    """The device's single call on a fresh solver."""
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    try:
        return s.log_probability(r)
    finally:
        s.close()


def _raw(s, kernels, resid, noise):
    """The low-level call: ``(out, info, nchains)``; resid and noise (N,) or (B, N)."""
    leaves, smap, h, P = q.pack_batch(kernels)
    nb = len(kernels)
    resid, noise = np.ascontiguousarray(resid, dtype=np.float64), np.ascontiguousarray(noise, dtype=np.float64)
    info, out, nchains = np.zeros(nb, dtype=np.int32), np.empty(nb), C.c_int32(-1)
    _ffi.check(_ffi.lib().tgp_qsep_logprob_batch(
        s._handle, nb, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
        _ffi.ptr(noise), s.n if noise.ndim == 2 else 0, _ffi.ptr(resid), s.n if resid.ndim == 2 else 0,
        _ffi.ptr(info), _ffi.ptr(out), C.byref(nchains)), "tgp_qsep_logprob_batch")
    return out, info, nchains.value


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a == b))


# -- 1. parity and bit-identity over the scan's shapes ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name, n, b):
    """(oracle, single call) of member b of case ``name`` at n points; computed once, shared by every batch size."""
    t, noise, r = _series(n, seed=n)
    k, nz = _member(name, b), _member_noise(noise, b)
    return float(o.log_probability(k, t, nz, r)), float(_single(k, t, nz, r))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1024, 1025, 4097])
@pytest.mark.parametrize("name", ["exp", "matern32", "m32cos_plus_sho", "celerite4"])
def test_parity_and_bits(name, n):
    t, noise, r = _series(n, seed=n)
    s = QuasisepSolver(_member(name, 0), t, Diagonal(noise))
    for nb in (1, 2, 3):
        ks = [_member(name, b) for b in range(nb)]
        nz = np.stack([_member_noise(noise, b) for b in range(nb)])
        got, info = s.log_probability_batch(ks, r, nz, return_info=True)
        assert got.shape == (nb,) and got.dtype == np.float64 and not info.any()
        for b in range(nb):
            oracle, single = _reference(name, n, b)
            print(f"{name} n={n} B={nb} member {b}: batch {got[b]!r} single {single!r} oracle {oracle!r}")
            assert got[b] == pytest.approx(oracle, rel=1e-8)
            assert got[b] == single


# -- 2. position and size independence ---------------------------------------------------------------------------------------
def test_position_and_batch_size_do_not_matter():
    n, name = 257, "m32cos_plus_sho"
    t, noise, r = _series(n, seed=21)
    probe, probe_noise = _member(name, 7), _member_noise(noise, 7)
    want = _single(probe, t, probe_noise, r)
    s = QuasisepSolver(_member(name, 0), t, Diagonal(noise))
    for nb in (2, 5, 65):
        for pos in sorted({0, nb // 2, nb - 1}):
            ks = [_member(name, b % 11) for b in range(nb)]
            nz = np.stack([_member_noise(noise, b % 11) for b in range(nb)])
            ks[pos], nz[pos] = probe, probe_noise
            got = s.log_probability_batch(ks, r, nz)
            assert got[pos] == want, (nb, pos, got[pos], want)


# -- 3. the boundary between two launch chains ------------------------------------------------------------------------------
def test_sixty_five_members_run_as_two_chains():
    n, name, nb = 40, "matern32", 65
    t, noise, r = _series(n, seed=22)
    ks = [_member(name, b % 13) for b in range(nb)]
    nz = np.stack([_member_noise(noise, b % 13) for b in range(nb)])
    s = QuasisepSolver(ks[0], t, Diagonal(noise))
    out, info, nchains = _raw(s, ks, r, nz)
    assert nchains == 2 and not info.any()
    for b in (62, 63, 64):
        assert out[b] == _single(ks[b], t, nz[b], r), b
    assert np.all(np.isfinite(out))


# -- 4. the memory cap ------------------------------------------------------------------------------------------------------------
def _members_that_fit(n, J, own_noise, own_resid):
    """DESIGN section 11, "Batches of models": how many members one launch chain holds under the 1 GiB cap."""
    lc = 16
    while lc < 256 and lc * 4096 < n:
        lc *= 2
    nc = -(-n // lc)
    levels = [nc]
    while levels[-1] > 64:
        levels.append(-(-levels[-1] // 64))
    work = 4 * 64 * sum(levels)
    fixed = 64 * 141 + (0 if own_noise else n) + (0 if own_resid else n)
    per_member = n * (2 + J) + work + 3 * nc + 3 + (n if own_noise else 0) + (n if own_resid else 0)
    return min(64, ((1 << 30) // 8 - fixed) // per_member)


def test_memory_cap_splits_the_batch():
    """N = 2^20, J = 8, one more member than fits 1 GiB.  The first member, the last of chain one and the first of chain
    two are held to their single calls bitwise; the others are checked for finiteness only: the sequential oracle
    takes about a minute per member at this N, which a test of a few seconds cannot afford."""
    n, name = 1 << 20, "celerite4"
    fits = _members_that_fit(n, 8, True, True)
    nb = fits + 1
    assert 8 <= nb <= 16
    t, noise, r = _series(n, seed=23)
    ks = [_member(name, b) for b in range(nb)]
    nz = np.stack([_member_noise(noise, b) for b in range(nb)])
    rs = np.stack([r * (1.0 + 0.01 * b) for b in range(nb)])
    s = QuasisepSolver(ks[0], t, Diagonal(noise), assume_sorted=True)
    out, info, nchains = _raw(s, ks, rs, nz)
    assert nchains == 2 and not info.any()
    assert np.all(np.isfinite(out))
    for b in (0, fits - 1, fits):
        assert out[b] == _single(ks[b], t, nz[b], rs[b]), b


def test_one_member_beyond_the_cap_is_refused():
    """The check precedes every allocation: at n = 12 000 000, J = 8 one member needs about 11 n doubles next to the 2 n
    of the shared noise and residual, more than 2^27 doubles together."""
    n = 12_000_000
    assert _members_that_fit(n, 8, False, False) == 0
    t = np.arange(n, dtype=np.float64)
    s = QuasisepSolver(_member("celerite4", 0), t, Diagonal(np.ones(n)), assume_sorted=True)
    with pytest.raises(ValueError, match="exceeds its cap"):
        s.log_probability_batch([_member("celerite4", 1)], np.zeros(n))


# -- 5. shared against per-member arrays ---------------------------------------------------------------------------------------
def test_shared_and_copied_inputs_give_the_same_bits():
    n, name, nb = 1025, "m32cos_plus_sho", 4
    t, noise, r = _series(n, seed=24)
    ks = [_member(name, b) for b in range(nb)]
    s = QuasisepSolver(ks[0], t, Diagonal(noise))
    shared = s.log_probability_batch(ks, r, noise)
    assert _bits_equal(shared, s.log_probability_batch(ks, r))  # the solver's own noise
    assert _bits_equal(shared, s.log_probability_batch(ks, np.tile(r, (nb, 1)), np.tile(noise, (nb, 1))))
    assert _bits_equal(shared, s.log_probability_batch(ks, np.tile(r, (nb, 1)), noise))
    assert _bits_equal(shared, s.log_probability_batch(ks, r, np.tile(noise, (nb, 1))))
    rs = np.stack([r + 0.1 * b * np.cos(t) for b in range(nb)])
    got = s.log_probability_batch(ks, rs, noise)
    for b in range(nb):
        assert got[b] == _single(ks[b], t, noise, rs[b]), b
    assert shared[0] == got[0] and np.all(shared[1:] != got[1:])


# -- 6. damping regimes mixed in one batch ---------------------------------------------------------------------------------
def test_mixed_damping_regimes():
    n = 1025
    t, noise, r = _series(n, seed=25)
    ks = [CASES[name](q) for name in ("sho_under", "sho_crit", "sho_over")]
    assert len({int(k._lower_ssm().leaves[0, 0]) for k in ks}) == 3
    s = QuasisepSolver(ks[0], t, Diagonal(noise))
    for order in ([0, 1, 2], [2, 0, 1]):
        got, info = s.log_probability_batch([ks[i] for i in order], r, return_info=True)
        assert not info.any()
        for v, i in zip(got, order):
            assert v == pytest.approx(float(o.log_probability(ks[i], t, noise, r)), rel=1e-8)
            assert v == _single(ks[i], t, noise, r)


# -- 7. one failing member ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_bad", [0, 16, 1024])
def test_one_failing_member_touches_no_other(k_bad):
    """noise[k] = -(k(0) + 1): since h^T P^- h <= k(0), pivot k is negative whatever precedes it."""
    n, name, nb = 1025, "matern32", 5
    t, noise, r = _series(n, seed=26)
    ks = [_member(name, b) for b in range(nb)]
    nz = np.stack([_member_noise(noise, b) for b in range(nb)])
    s = QuasisepSolver(ks[0], t, Diagonal(noise))
    clean, clean_info = s.log_probability_batch(ks, r, nz, return_info=True)
    assert not clean_info.any() and np.all(np.isfinite(clean))
    ssm = ks[2]._lower_ssm()
    bad = nz.copy()
    bad[2, k_bad] = -(float(ssm.h @ ssm.Pinf @ ssm.h) + 1.0)
    got, info = s.log_probability_batch(ks, r, bad, return_info=True)
    assert list(info) == [0, 0, k_bad + 1, 0, 0]
    assert got[2] == -np.inf
    keep = [0, 1, 3, 4]
    assert _bits_equal(got[keep], clean[keep])
    raw, _, _ = _raw(s, ks, r, bad)
    assert np.isnan(raw[2]) and _bits_equal(raw[keep], clean[keep])


# -- 8. the handle's resident factor is left alone ---------------------------------------------------------------------------
def test_handle_is_untouched():
    n = 1025
    t, noise, r = _series(n, seed=27)
    own = _member("m32cos_plus_sho", 0)
    xt = np.linspace(t[0] - 1.0, t[-1] + 1.0, 50)
    s = QuasisepSolver(own, t, Diagonal(noise))
    s.refactor()

    def snapshot():
        mean, var = s.predict_mean_var(r, xt)
        return s.solve_triangular(r), float(s.normalization()), mean, var, s.info

    before = snapshot()
    ssm = s._ssm
    others = [_member("celerite4", b) for b in range(3)]
    nz = np.stack([_member_noise(noise, b) for b in range(3)])
    nz[1, 500] = -100.0
    got, info = s.log_probability_batch(others, 2.0 * r, nz, return_info=True)
    assert list(info) == [0, 501, 0] and got[1] == -np.inf and np.isfinite(got[0]) and np.isfinite(got[2])
    assert s.kernel is own and s._ssm is ssm and s._info == 0 and s._factored
    after = snapshot()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3]) and before[4] == after[4] == 0

    lazy = QuasisepSolver(own, t, Diagonal(noise))
    assert not lazy._factored
    got2 = lazy.log_probability_batch(others, 2.0 * r, nz)
    assert _bits_equal(got2, got) and not lazy._factored
    assert lazy.log_probability(r) == _single(own, t, noise, r)
    assert np.array_equal(lazy.solve_triangular(r), before[0])


# -- 9. the GP level ------------------------------------------------------------------------------------------------------------
def test_gp_batch_equals_separate_gps():
    n, name, nb = 1000, "m32cos_plus_sho", 4
    t, _, y = _series(n, seed=28)
    ks = [_member(name, b) for b in range(nb)]
    diags = np.array([0.1, 0.15, 0.2, 0.05])
    means = np.array([0.0, 0.3, -0.2, 1.5])
    gp = GaussianProcess(ks[0], t, diag=0.1)
    got = gp.log_probability_batch(y, ks, diags=diags, means=means)
    assert got.shape == (nb,) and got.dtype == np.float64
    for b in range(nb):
        want = GaussianProcess(ks[b], t, diag=diags[b], mean=means[b]).log_probability(y)
        assert got[b] == want, b
    # (B, N) forms of the same inputs, and the GP's own mean and noise
    full = gp.log_probability_batch(y, ks, diags=np.repeat(diags[:, None], n, 1), means=np.repeat(means[:, None], n, 1))
    assert _bits_equal(full, got)
    assert gp.log_probability_batch(y, ks)[0] == gp.log_probability(y)


def test_gp_batch_dtypes_empty_and_other_solvers():
    n, name = 300, "matern32"
    t, _, y = _series(n, seed=29)
    ks = [_member(name, b) for b in range(3)]
    t32, y32 = t.astype(np.float32), y.astype(np.float32)
    gp32 = GaussianProcess(ks[0], t32, diag=np.float32(0.1))
    got = gp32.log_probability_batch(y32, ks, diags=np.array([0.1, 0.2, 0.3], dtype=np.float32))
    assert got.dtype == np.float32 and got.shape == (3,)
    for b, d in enumerate(np.array([0.1, 0.2, 0.3], dtype=np.float32)):
        assert got[b] == GaussianProcess(ks[b], t32, diag=d).log_probability(y32)
    gp = GaussianProcess(ks[0], t, diag=0.1)
    empty = gp.log_probability_batch(y, [])
    assert empty.shape == (0,) and empty.dtype == np.float64
    out, info = gp.solver.log_probability_batch([], y, return_info=True)
    assert out.shape == (0,) and info.shape == (0,)
    dense = GaussianProcess(ks[0], t, diag=0.1, solver=DirectSolver)
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.log_probability_batch(y, ks)
    with pytest.raises(ValueError, match="kernel 1"):
        gp.log_probability_batch(y, [ks[0], q.Matern52(1.0)])
    with pytest.raises(ValueError, match="resid must have shape"):
        gp.solver.log_probability_batch(ks, np.zeros((2, n)))


# -- 10. determinism -----------------------------------------------------------------------------------------------------------
def test_same_batch_twice_is_bit_identical():
    n, name, nb = 4097, "celerite4", 7
    t, noise, r = _series(n, seed=30)
    ks = [_member(name, b) for b in range(nb)]
    nz = np.stack([_member_noise(noise, b) for b in range(nb)])
    s = QuasisepSolver(ks[0], t, Diagonal(noise))
    a, b = s.log_probability_batch(ks, r, nz), s.log_probability_batch(ks, r, nz)
    assert np.all(np.isfinite(a)) and _bits_equal(a, b)
