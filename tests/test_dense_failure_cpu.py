"""What test_gpu_1_failure.py expects, proved on the host: for every (n, p) up to n = 1 100 that the GPU tests use,
the plain reference of tests/_dense_failure.py reports p + 1 for both families of planted matrices, LAPACK agrees for
the negative pivot, and the margins that make the value independent of rounding hold (every pivot before p >= the clean
diagonal, pivot p <= -7 for the noise plant and <= -1 for the overwritten diagonal).  A later change of the inputs that
would make the GPU tests vacuous fails here."""
import numpy as np
import pytest
from scipy.linalg import lapack

import _dense_failure as df


def _check_negative(K, p, c, top):
    info, d = df.first_bad_pivot(K)
    assert info == p + 1
    assert d[p] <= top and np.all(d[:p] >= c), (d[p], d[:p].min(initial=np.inf))
    assert lapack.dpotrf(K, lower=1)[1] == p + 1


@pytest.mark.parametrize("n,dtype,c", [(n, np.float64, 0.05) for n in df.RAW_SIZES] + [(640, np.float32, 0.5)])
def test_raw_factor_plants(n, dtype, c):
    K0 = df.spd(n, dtype, c).astype(np.float64)
    assert df.first_bad_pivot(K0)[0] == 0
    for p in df.raw_positions(n):
        seen = 0
        for form in df.RAW_FORMS:
            K = df.plant(K0, p, form)
            if K is None:
                continue
            seen += 1
            if form == "neg":
                _check_negative(K, p, c, -1.0)
            else:
                info, d = df.first_bad_pivot(K)
                assert info == p + 1 and np.isnan(d[p]) and np.all(d[:p] >= c), (p, form)
        # every form exists where its column does: the pair forms need a column in front of p in the step / tile
        assert seen == 3 + (p % df.STEP > 0) + (p % df.TILE >= df.STEP) + (p >= df.TILE), (p, seen)


NOISE_CASES = sorted({(n, p) for n in df.RAGGED_SIZES if n <= 1100 for p in df.ragged_positions(n)}
                     | {(df.CALLER_N, df.CALLER_P)} | {c for c in df.HANDLE_CASES if c[0] <= 1100})


@pytest.mark.parametrize("n,p", NOISE_CASES)
def test_noise_plant(n, p):
    _check_negative(df.noise_matrix(n, p), p, df.DIAG, -7.0)
    # ... and the NaN forms the caller-level tests reach through covariance= and through a NaN coordinate
    clean = df.noise_matrix(n, [])
    for K in (df.plant(clean, p, "nan_row"), _nan_coordinate(n, p)):
        info, d = df.first_bad_pivot(K)
        assert info == p + 1 and np.isnan(d[p]) and np.all(d[:p] >= df.DIAG)


def _nan_coordinate(n, p):
    from oracle import tinygp_np as o

    X = df.inputs(n)[0].copy()
    X[p] = np.nan
    K = df.kernel(o)(X, X) + df.DIAG * np.eye(n)
    assert np.all(np.isnan(K[p])) and np.all(np.isnan(K[:, p])) and np.isnan(K).sum() == 2 * n - 1
    return K


def test_fp32_margin():
    """fp32 (section 5 of the GPU file is past 1 100 rows; the same inputs at n = 1 100): on fp32-rounded inputs the
    clean pivots stay >= 0.5, far above fp32's rounding of a matrix with entries <= 2.75."""
    for p in (0, 127, 128, 1023, 1024, 1099):
        _check_negative(df.noise_matrix(1100, p, np.float32), p, df.DIAG, -7.0)


@pytest.mark.parametrize("p1,p2", [(130, 140), (130, 250), (130, 300), (0, 639), (511, 512)])
def test_the_first_of_two(p1, p2):
    K = df.noise_matrix(640, [p2, p1])
    info, d = df.first_bad_pivot(K)
    assert info == p1 + 1 and d[p1] <= -7.0 and np.all(d[:p1] >= df.DIAG)
    assert lapack.dpotrf(K, lower=1)[1] == p1 + 1


def test_positions_cover_every_edge_of_every_schedule():
    """SCHEDULE_POSITIONS holds both ends and the first and last column of every width the option sets name; the
    boundary cases put a position on each side of their panel width and of the 64-block limit, and on the last real
    row in front of the padding."""
    want = set(df.SCHEDULE_POSITIONS)
    assert {0, df.STEP - 1, df.STEP, df.TILE - 1, df.TILE, df.SCHEDULE_N - 1} <= want
    for opts in df.PANEL_CHAIN_VARIANTS:
        assert set(df.edges(df.SCHEDULE_N, opts)) <= want, opts
    assert len(df.BOUNDARY_CASES) == 9
    for n, opts in df.BOUNDARY_CASES:
        nb = opts.get("nb_first") or opts["nb_outer"]
        assert n % df.TILE != 0
        assert {nb - 1, nb, nb + 1, df.CHAIN_LIMIT - 1, df.CHAIN_LIMIT, n - 1} <= set(df.edges(n, opts, above=True)), (n, opts)
    for (n, _opts, p1, p2), where in zip(df.PAIRS.values(), ("step", "tile", "panel", None, None)):
        assert 0 <= p1 < p2 < n
        if where == "step":
            assert p1 // df.STEP == p2 // df.STEP
        elif where == "tile":
            assert p1 // df.STEP != p2 // df.STEP and p1 // df.TILE == p2 // df.TILE
        elif where == "panel":
            assert p1 // df.TILE != p2 // df.TILE and p1 // 1024 == p2 // 1024
    assert df.PAIRS["two_panels"][2] // 1024 != df.PAIRS["two_panels"][3] // 1024
    assert df.CALLER_P // df.TILE == 2
    for nb in df.DIST_NB:
        assert all(0 <= p < df.DIST_N for p in df.dist_positions(nb)) and df.DIST_N % nb


def test_the_plain_reference_is_a_cholesky():
    import scipy.linalg as sla

    K = df.spd(300)
    info, d = df.first_bad_pivot(K)
    assert info == 0
    np.testing.assert_allclose(np.sqrt(d), np.diag(sla.cholesky(K, lower=True)), rtol=1e-12)
