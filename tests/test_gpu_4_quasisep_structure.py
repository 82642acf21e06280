"""The affine recurrences of ``csrc/qsep.hip`` (L^-1 y, L^-T y, L z) at every chunk length, scan depth and width of
the right-hand side, against the float64 sequential oracle.

Shape of the scan (``tgp_qsep_create``, ``level_sizes``): chunks of lc = 16 steps up to N = 65 536, then 32, 64, 128
and 256 above 524 288; one scan level up to 64 chunks, two up to 4 096, three above; 8 right-hand sides per wavefront,
``ncg = ceil(R / 8)`` scans interleaved in the work buffer.  The bar is the project's solve bar, rtol = atol = 5e-7."""
import numpy as np
import pytest

from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSolver

import _quasisep_np as o
from _quasisep_cases import CASES
from _quasisep_edges import _levels

pytestmark = pytest.mark.gpu

BAR = dict(rtol=5e-7, atol=5e-7)
OPS = ["solve", "solve_T", "dot"]
THREE_LEVELS = (1 << 20) + 1  # 4 097 chunks of 256 -> 65 -> 2

SMALL_N = [1, 2, 15, 16, 17, 1023, 1024, 1025, 4097]
SMALL_R = [1, 7, 8, 9, 16, 17, 64, 65, (3, 3)]
# (N, lc, levels); the clustered series with ties at the lc = 64 size
LARGE = [(65536, 16, 2), (65537, 32, 2), (131073, 64, 2), (262145, 128, 2), (524289, 256, 2), (THREE_LEVELS, 256, 3)]
CLUSTERED_N = 131073
LARGE_KERNELS = ["matern32", "m32cos_plus_sho"]


def _series(n, seed=0, clustered=False):
    rng = np.random.default_rng(seed)
    if clustered:
        dt = np.where(rng.uniform(size=n) < 0.5, rng.exponential(0.001, n), rng.exponential(0.3, n))
        dt[rng.uniform(size=n) < 0.05] = 0.0
        t = np.cumsum(dt)
    else:
        t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)


def test_sizes_reach_the_shapes_they_name():
    assert [(n,) + _levels(n) for n, _, _ in LARGE] == LARGE
    assert [_levels(n) for n in SMALL_N] == [(16, 1)] * 7 + [(16, 2)] * 2  # 1024 points: 64 chunks, one level; 1025: 65
    assert _levels(1 << 22) == (256, 3)


@pytest.fixture(scope="module")
def problem():
    """(kernel name, N) -> series, device solver and the oracle's factor; built once per key, one key held at a time
    (the transitions of J = 6 at N = 2^20 + 1 are 300 MB)."""
    held = {}

    def get(name, n):
        if (name, n) not in held:
            for s in held.values():
                s["solver"].close()
            held.clear()
            k = CASES[name](q)
            t, noise, r = _series(n, seed=n, clustered=n == CLUSTERED_N)
            solver = QuasisepSolver(k, t, Diagonal(noise))
            assert solver.info == 0
            held[name, n] = dict(k=k, t=t, noise=noise, r=r, solver=solver, F=o.factor(k, t, noise))
        return held[name, n]

    yield get
    for s in held.values():
        s["solver"].close()


def _check(p, op, shape, tag):
    n = len(p["t"])
    seed = (n * 1000 + int(np.prod(shape))) * 3 + OPS.index(op)
    y = np.random.default_rng(seed).standard_normal((n,) + shape)  # distinct random columns
    s, F, y2 = p["solver"], p["F"], y.reshape(n, -1)  # the oracle takes (N, R): trailing axes are columns
    if op == "solve":
        got, want = s.solve_triangular(y), o.solve_lower(F, y2)
    elif op == "solve_T":
        got, want = s.solve_triangular(y, transpose=True), o.solve_upper(F, y2)
    else:
        got, want = s.dot_triangular(y), o.dot_lower(F, y2)
    want = want.reshape(y.shape)
    assert got.shape == want.shape == y.shape and got.dtype == np.float64
    err = np.abs(got - want).reshape(n, -1)
    worst = int(np.argmax(err.max(axis=0)))
    print(f"{tag} {op}: max |got - ref| = {err.max():.3e} (column {worst} of {err.shape[1]}), max |ref| = "
          f"{np.abs(want).max():.3e}")
    np.testing.assert_allclose(got, want, **BAR)  # every column, those of the ragged last column group included


def _shape(R):
    return R if isinstance(R, tuple) else (R,)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("R", SMALL_R, ids=lambda R: "x".join(map(str, _shape(R))))
@pytest.mark.parametrize("n", SMALL_N)
def test_small_sweep(problem, n, R, op):
    _check(problem("m32cos_plus_sho", n), op, _shape(R), f"m32cos_plus_sho n={n} R={R}")


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", [n for n, _, _ in LARGE])
@pytest.mark.parametrize("name", LARGE_KERNELS)
def test_large_sweep(problem, name, n, op):
    lc, levels = _levels(n)
    _check(problem(name, n), op, (9,), f"{name} n={n} lc={lc} levels={levels} R=9")


@pytest.mark.parametrize("name", LARGE_KERNELS[::-1])  # the large sweep leaves the last kernel's problem in place
def test_three_level_factor_over_all_steps(problem, name):
    """c_n, w_n and the likelihood at N = 2^20 + 1 against the oracle over every step, not a prefix."""
    p = problem(name, THREE_LEVELS)
    c, w = p["solver"].factor_data()
    _, _, oc, ow = p["F"]
    print(f"{name}: max rel |c - ref| = {np.max(np.abs(c - oc) / oc):.3e}, max |w - ref| = {np.abs(w - ow).max():.3e}")
    np.testing.assert_allclose(c, oc, rtol=1e-9)
    np.testing.assert_allclose(w, ow, rtol=1e-8, atol=1e-12)
    want = o.log_probability(p["k"], p["t"], p["noise"], p["r"], F=p["F"])
    got = p["solver"].log_probability(p["r"])
    print(f"{name}: log_probability {got!r} (oracle {want!r}, rel {abs(got - want) / abs(want):.3e})")
    assert got == pytest.approx(want, rel=1e-8)


def test_round_trip_4m_points_j8():
    """N = 2^22 (16 384 chunks of 256, three levels), J = 8, R = 9: L^-1 (L z) = z and L (L^-1 y) = y.  Device only
    (the sequential oracle costs minutes here); two errors that cancel would pass, the sweeps above are the check."""
    n = 1 << 22
    t, noise, _ = _series(n, seed=13)
    s = QuasisepSolver(CASES["celerite4"](q), t, Diagonal(noise), assume_sorted=True)
    assert s.info == 0
    z = np.random.default_rng(14).standard_normal((n, 9))
    back = s.solve_triangular(s.dot_triangular(z))
    print(f"solve(dot(z)): max |.. - z| = {np.abs(back - z).max():.3e}")
    np.testing.assert_allclose(back, z, **BAR)
    back = s.dot_triangular(s.solve_triangular(z))
    print(f"dot(solve(y)): max |.. - y| = {np.abs(back - z).max():.3e}")
    np.testing.assert_allclose(back, z, **BAR)
    s.close()


def test_no_columns(monkeypatch):
    """(N, 0) in, (N, 0) out, and the factored solver makes no library call for it."""
    t, noise, _ = _series(100, seed=1)
    s = QuasisepSolver(CASES["matern32"](q), t, Diagonal(noise))
    assert s.info == 0  # factors
    calls = []
    real = _ffi.check
    monkeypatch.setattr(_ffi, "check", lambda *a, **kw: (calls.append(a), real(*a, **kw))[1])
    for out in (s.solve_triangular(np.empty((100, 0))), s.solve_triangular(np.empty((100, 0)), transpose=True),
                s.dot_triangular(np.empty((100, 0))), s.solve_triangular(np.empty((100, 2, 0)))):
        assert out.shape[0] == 100 and out.size == 0 and out.dtype == np.float64
    assert s.dot_triangular(np.empty((100, 0))).shape == (100, 0)
    assert calls == []
    monkeypatch.undo()
    assert s.solve_triangular(np.ones((100, 1))).shape == (100, 1)
