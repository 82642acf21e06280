"""tests/_gemm_exact.py on the CPU: the case lists of test_gpu_0_gemm_exact.py are exact by construction and not vacuous on
256 compute units, and the check rejects every kind of doctored result."""
import numpy as np
import pytest

import _gemm_exact as gx

CUS = 256


def _all_cases():
    return [gx.resolve(c, CUS) for c in gx.integer_cases()]


def test_every_case_keeps_its_sums_exact():
    """max |C0| + 225 k below 2^24 / 2^53 and the reference itself below it, for every case of the GPU file."""
    seen = set()
    for c in _all_cases():
        assert c.k % gx.BK == 0 and c.k > 0 and (c.dtype == "f64" or c.k <= 2048)
        assert gx.CMAX + c.k * gx.AMAX ** 2 < gx.LIMIT[c.dtype]
        key = (c.dtype, c.tm, c.tn, c.k, c.mode, c.padded)
        if key in seen or c.tm * c.tn > 32:  # (operands differ by seed only; the largest shapes by the bound above)
            continue
        seen.add(key)
        inp = gx.make_inputs(c)
        assert gx.magnitude_ok(c, inp), gx.case_id(c)
        A, B = inp.A[:inp.m].astype(np.int64), inp.B[:inp.n].astype(np.int64)
        assert np.abs(A).max() == gx.AMAX and np.abs(B).max() == gx.AMAX
        if c.tm * c.tn <= 6 and c.k <= 144:  # the BLAS route to the reference is NumPy's own int64 product
            np.testing.assert_array_equal(inp.prod, A @ B.T)
        assert inp.lda - inp.m == (128 if c.padded else 0) and inp.ldb - inp.n == (256 if c.padded else 0)
        assert inp.ldc - inp.m == (384 if c.padded else 0)
        for buf, rows in ((inp.A, inp.m), (inp.B, inp.n), (inp.C0, inp.m)):
            assert (gx._bits(np.ascontiguousarray(buf[rows:])) == gx.NAN_BITS[c.dtype]).all()
        if c.mode == 1:
            assert np.isnan(inp.C0).all()


def test_case_ids_are_unique():
    for group in (gx.group1, gx.group2, gx.group3, gx.group4, gx.group5, gx.group5_rejected, gx.group6, gx.group7):
        ids = [gx.case_id(c) for c in group()]
        assert len(ids) == len(set(ids)) and ids


def test_host_logic_restated():
    """split_factor and persistent_grid at the values gemm.hip's comments and the default context give."""
    assert [gx.split_factor(1, k, CUS) for k in gx.K_SPLIT] == [2, 2, 4, 4, 8]
    assert gx.split_factor(1, 272, CUS) == 1 and gx.split_factor(512, 1024, CUS) == 1  # odd k-tiles; no partly filled round
    assert gx.split_factor(105, 1024, CUS) == 4 and gx.split_factor(528, 256, CUS) == 2
    assert gx.persistent_grid(66, 0, CUS) == 66 and gx.persistent_grid(1000, 96, CUS) == 416
    assert gx.persistent_grid(21, 2 * CUS - 8, CUS) == 8 and gx.persistent_grid(3, 2 * CUS - 8, CUS) == 3
    assert gx.persistent_grid(100, 2 * CUS, CUS) == 8
    assert gx.tile_count(5, 2, 1) == 9 and gx.tile_count(2, 5, 1) == 3 and gx.tile_count(2, 3, 0) == 6


def test_case_lists_are_not_vacuous():
    g3 = [gx.resolve(c, CUS) for c in gx.group3()]
    S = [gx.split_factor(gx.nblk_of(c), c.k, CUS) for c in g3]
    assert {2, 4, 8} <= set(S)
    assert all(s > 1 for c, s in zip(g3, S) if c.k != 272) and all(s == 1 for c, s in zip(g3, S) if c.k == 272)
    big = [c for c in g3 if gx.nblk_of(c) > 2 * CUS]
    assert [(c.tm, gx.nblk_of(c)) for c in big] == [(32, 528)]
    assert {gx.nblk_of(c) for c in gx.group4()} == {1, 6, 10, 21}
    for c in gx.group4():
        nblk, grid = gx.nblk_of(c), gx.persistent_grid(gx.nblk_of(c), gx.options(c, CUS)["gemm_reserve"], CUS)
        assert grid == min(nblk, 8) and (grid < nblk or nblk <= 8)
    for c in gx.group5():
        cnt = gx.tile_count(c.tm, c.prefix // gx.BM, 1)
        assert 0 < cnt < gx.nblk_of(c) and c.k >= 128 and c.prefix < c.tm * gx.BM
    assert {gx.nblk_of(c) for c in gx.group2()} == {1, 3, 10, 66, 9}
    assert all(gx.tile_of(c) == gx.SM for c in gx.group6()) and all(gx.tile_of(c) == gx.BM for c in gx.group1())
    groups = [gx.group1(), gx.group3(), gx.group4(), gx.group5(), gx.group6()]
    for dt in ("f64", "f32"):  # the real-valued cases are cases of the groups they stand for
        picked = [c for c in gx.group7() if c.dtype == dt]
        for g in groups:
            if dt == "f32" and g is groups[1]:
                continue
            assert any(c in g for c in picked), dt


LOWER = gx.case("f64", 0, 3, 3, 144, 1, 0, True)
FULL32 = gx.case("f32", 0, 2, 3, 112, 0, 0, True)
SMALL = gx.case("f64", 1, 3, 3, 64, 1, 0, False)
SKIP = gx.case("f32", 5, 3, 3, 512, 1, 0, False)
WIDE = gx.case("f64", 0, 2, 5, 32, 1, 1, False)


@pytest.mark.parametrize("c", [LOWER, FULL32, SMALL, SKIP, WIDE], ids=gx.case_id)
def test_check_accepts_the_exact_result(c):
    inp = gx.make_inputs(c)
    gx.check_exact(c, inp, gx.exact_result(c, inp))
    if c.lower:  # what lies above the diagonal inside a diagonal tile may as well stay untouched
        got = gx.exact_result(c, inp)
        _, may, _ = gx.regions(c, inp)
        got[:inp.m][may] = inp.C0[:inp.m][may]
        gx.check_exact(c, inp, got)


def _tile(ti, tj, t=gx.BM):
    return slice(ti * t, (ti + 1) * t), slice(tj * t, (tj + 1) * t)


def _doctor(kind, c, inp):
    got = gx.exact_result(c, inp)
    A, B = inp.A[:inp.m].astype(np.float64), inp.B[:inp.n].astype(np.float64)
    if kind == "one entry off by one":
        got[2 * gx.BM + 77, gx.BM + 5] += 1
        return got, "(2, 1) with 1 of"
    if kind == "one k-tile missing from one tile":
        r, q = _tile(1, 1)
        got[:inp.m][r, q] += (A[r, 32:48] @ B[q, 32:48].T).astype(got.dtype)
        return got, "(1, 1) with"
    if kind == "one tile updated twice":
        r, q = _tile(2, 0)
        got[:inp.m][r, q] -= (A[r] @ B[q].T).astype(got.dtype)
        return got, "updated twice"
    if kind == "one tile not updated":
        r, q = _tile(1, 0)
        got[:inp.m][r, q] = inp.C0[:inp.m][r, q]
        return got, "not updated"
    if kind == "one padding row overwritten":
        got[inp.m + 200, gx.BM: 2 * gx.BM] = 0.0
        return got, f"padding entries of C overwritten, the first at row {inp.m + 200}, column {gx.BM}"
    if kind == "one padding entry with another NaN":
        got[inp.ldc - 1, inp.n - 1] = np.nan
        return got, "padding entries of C overwritten"
    if kind == "one far tile touched":
        r, q = _tile(0, 2)
        got[:inp.m][r, q] = inp.ref[r, q].astype(got.dtype)
        return got, "outside the update changed: first wrong 128x128 tile (ti, tj) = (0, 2)"
    if kind == "a NaN where an update was due":
        got[gx.BM, 3] = np.nan
        return got, "(1, 0) with 1 of 16384 entries wrong, 1 NaN"
    raise KeyError(kind)


KINDS = ["one entry off by one", "one k-tile missing from one tile", "one tile updated twice", "one tile not updated",
         "one padding row overwritten", "one padding entry with another NaN", "one far tile touched",
         "a NaN where an update was due"]


@pytest.mark.parametrize("kind", KINDS)
def test_check_rejects_a_doctored_result(kind):
    inp = gx.make_inputs(LOWER)
    got, says = _doctor(kind, LOWER, inp)
    with pytest.raises(AssertionError) as e:
        gx.check_exact(LOWER, inp, got)
    assert says in str(e.value) and gx.case_id(LOWER) in str(e.value), str(e.value)


def test_check_rejects_in_the_other_forms():
    # fp32: one unit in the last place the integers use
    inp = gx.make_inputs(FULL32)
    got = gx.exact_result(FULL32, inp)
    got[130, 300] -= 1
    with pytest.raises(AssertionError, match=r"\(1, 2\) with 1 of"):
        gx.check_exact(FULL32, inp, got)
    # 64 x 64 tiles: the 64-tile right of a diagonal one is outside the update although it shares its 128-tile
    inp = gx.make_inputs(SMALL)
    got = gx.exact_result(SMALL, inp)
    r, q = _tile(2, 3, gx.SM)
    got[r, q] = inp.ref[r, q]
    with pytest.raises(AssertionError, match=r"outside the update changed.*\(1, 1\)"):
        gx.check_exact(SMALL, inp, got)
    # skip00: the first diagonal block must come back as it went in
    inp = gx.make_inputs(SKIP)
    got = gx.exact_result(SKIP, inp)
    np.testing.assert_array_equal(got[:gx.BM, :gx.BM], inp.C0[:gx.BM, :gx.BM])
    got[5, 3] = inp.ref[5, 3]
    with pytest.raises(AssertionError, match=r"outside the update changed.*\(0, 0\) with 1 of"):
        gx.check_exact(SKIP, inp, got)
    # lower with n > m, mode 1: the columns past m keep their NaN
    inp = gx.make_inputs(WIDE)
    got = gx.exact_result(WIDE, inp)
    assert np.isnan(got[:, inp.m:]).all() and not np.isnan(np.tril(got[:, :inp.m])).any()
    got[0, inp.m + 1] = 0.0
    with pytest.raises(AssertionError, match=r"outside the update changed.*\(0, 2\)"):
        gx.check_exact(WIDE, inp, got)


def test_real_check_holds_the_bound_and_only_the_bound():
    for c in gx.group7()[:2] + [gx.case("f32", 1, 3, 3, 256, 1)]:
        inp = gx.make_real_inputs(c)
        assert inp.ref.dtype == (np.longdouble if c.dtype == "f64" else np.float64)
        must, may, _ = gx.regions(c, inp)
        got = inp.C0.copy(order="F")
        got[:inp.m][must | may] = inp.ref[must | may].astype(got.dtype)  # the correctly rounded result: half an ulp
        assert gx.check_real(c, inp, got) < 0.5
        i, j = inp.m - 1, 0
        got[i, j] += got.dtype.type(1.5 * inp.bound[i, j])
        with pytest.raises(AssertionError, match="differs from the reference"):
            gx.check_real(c, inp, got)
