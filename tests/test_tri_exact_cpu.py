"""tests/_tri_exact.py on the CPU: the right-hand sides are exact integer products at every size the GPU file uses, LAPACK
returns the integer solution with error 0 on family X (within BAR_D on family D) in both directions and from the right, the
models of the streaming forward solve and of the right-sided sweep visit every tile exactly once under every G and every
panel width, and one dropped or doubled tile product fails the checks with its block named."""
import numpy as np
import pytest
import scipy.linalg as sla

import _chol_exact as cx
import _tri_exact as tx

B = cx.TILE
FAMILIES = [("X", np.float64), ("D", np.float64), ("X", np.float32)]
IDS = ["X-f64", "D-f64", "X-f32"]
# the sizes of tests/test_gpu_1_tri_exact.py
N_SWEEP, N_ALPHA32, N_SOLVER = 4000, 1536, 2400
N_FEW = (128, 256, 384, 512, 640, 900)
RIGHT = [(1152, 128, 128), (1152, 384, 256), (1152, 128, 512), (2304, 128, 1024), (2176, 128, 1024)]  # (n, m, nb_outer)
NB_OUTER = (128, 256, 512, 1024)


def _solve(L0, y, trans=0):
    return sla.solve_triangular(np.asarray(L0), y, lower=True, trans=trans, check_finite=False)


def _held(got, want, family, check=tx.check_vec, **kw):
    """Family X: equal.  Family D: within BAR_D."""
    check(got, want, None if family == "X" else cx.BAR_D, **kw)


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=IDS)
def test_right_hand_sides_are_exact_at_every_size_of_the_gpu_file(family, dtype):
    """Every builder asserts, on the arrays it returns, that the product is the int64 product and that every partial sum of
    it stays below 2^53 / 2^24; here they run at every (n, dtype) of the GPU file, and LAPACK solves them back."""
    f64 = dtype == np.float64
    p, a = cx.PARAMS[cx._name(dtype)]
    L0 = cx.factor(N_SWEEP, family, dtype)
    w, r = cx.rhs(L0)
    _held(_solve(L0, r), w, family)
    wt, yt = tx.rhs_t(L0)
    assert yt.dtype == dtype and np.abs(wt).max() == 3 and not np.array_equal(wt, w)
    _held(_solve(L0, yt, trans=1), wt, family)
    nk = N_SWEEP if f64 else N_ALPHA32
    assert 3 * (p + a * nk) ** 2 < cx.LIMIT[cx._name(dtype)]  # (a priori; the builder asserts the tight bound)
    Lk = cx.factor(nk, family, dtype)
    v, u, rk = tx.rhs_k(Lk)
    assert rk.dtype == dtype
    _held(_solve(Lk, rk), u, family)
    _held(_solve(Lk, _solve(Lk, rk), trans=1), v, family)
    if not f64:
        with pytest.raises(AssertionError, match="partial sums up to"):  # (the bound has teeth: p^2 alone is 2^24 here)
            tx.rhs_k(64 * np.asarray(cx.factor(2 * B, "X", np.float32)))
    for n, m, _ in (RIGHT if f64 else RIGHT[1:2]):
        L0 = cx.factor(n, family, dtype)
        W, Bm = tx.rhs_right(L0, m)
        assert W.shape == Bm.shape == (m, n) and Bm.dtype == dtype
        _held(_solve(L0, Bm.T).T, W, family, tx.check_block, along=1)
    if family == "X" and f64:
        for n in N_FEW:
            L0 = cx.factor(n, "X")
            for w, y, trans in ((*cx.rhs(L0), 0), (*tx.rhs_t(L0), 1)):
                tx.check_vec(_solve(L0, y, trans), w)
            v, u, rk = tx.rhs_k(L0)
            tx.check_vec(_solve(L0, _solve(L0, rk), trans=1), v)
        L0 = cx.factor(N_SOLVER, "X")
        for r, transpose in ((2, False), (130, False), (2, True)):
            W, Y = tx.rhs_block(L0, r, transpose)
            assert W.shape == Y.shape == (N_SOLVER, r)
            tx.check_block(_solve(L0, Y, int(transpose)), W)


def test_the_reports_name_block_column_count_and_deviation():
    want = np.arange(700, dtype=np.float64)
    got = want.copy()
    tx.check_vec(got, want)
    got[5] = -0.0 * 1  # a signed zero is a zero
    want[5] = 0.0
    tx.check_vec(got, want)
    got[300] += 0.5
    got[383] += 0.25
    got[699] = np.nan
    with pytest.raises(AssertionError) as e:
        tx.check_vec(got, want)
    assert "first wrong 128-block 2 with 2 of 128 entries wrong, largest deviation 5.000e-01; 2 block(s) wrong" in str(e.value)
    with pytest.raises(AssertionError, match=r"128-block 5 with 1 of 60 entries wrong, no finite deviation, 1 not finite"):
        tx.check_vec(np.r_[want[:640], got[640:]], want)
    ok = want.copy()
    ok[130] += cx.BAR_D
    tx.check_vec(ok, want, cx.BAR_D)
    ok[130] += cx.BAR_D
    with pytest.raises(AssertionError, match="128-block 1 with 1 of 128"):
        tx.check_vec(ok, want, cx.BAR_D)
    Wn = np.zeros((300, 5))
    G = Wn.copy()
    tx.check_block(G, Wn)
    G[200, 3] = 1.0
    G[140, 4] = 2.0
    G[10, 1] = np.inf
    with pytest.raises(AssertionError) as e:
        tx.check_block(G[128:], Wn[128:])
    assert "first wrong (128-block, column) = (0, 3) with 1 of 128 entries wrong, largest deviation 1.000e+00 in it, 2 in" \
        in str(e.value)
    with pytest.raises(AssertionError, match=r"\(128-block, column\) = \(0, 1\) with 1 of 128 entries wrong, no finite dev"):
        tx.check_block(G, Wn)
    G[10, 1] = 0.0
    with pytest.raises(AssertionError, match=r"\(row, 128-column block\) = \(3, 1\) with 1 of 128 .* 1 block\(s\) wrong"):
        tx.check_block(np.ascontiguousarray(G.T), np.ascontiguousarray(Wn.T), along=1)


def test_groups_and_owners_follow_the_kernel():
    assert [tx.stream_groups(nb) for nb in (1, 40, 41, 256, 257)] == [3, 3, 4, 4, 6]
    assert [tx.stream_groups(31, g) for g in (-1, 0, 1, 2, 5, 8, 9, 100)] == [3, 3, 2, 2, 5, 8, 8, 8]
    assert [tx.stream_owner(9, c, 4) for c in (9, 8, 7, 6, 5, 4, 3)] == \
        ["primary W", "primary tf", "primary tf2", "helper 0", "helper 1", "helper 2", "helper 0"]
    assert tx.right_two(1152, 512) == (True, 512) and tx.right_two(1152, 512, lookahead=0) == (False, 512)
    assert tx.right_two(2048, 1024) == (False, 1024) and tx.right_two(2176, 1024) == (True, 1024)
    assert tx.right_two(1152, 200) == (True, 128) and tx.right_two(256, 64) == (False, 128)
    assert tx.right_ii_first(1152, 256) == (4, 0) and tx.right_ii_first(1152, 512) == (8, 0)
    assert tx.right_ii_first(1152, 256, panel=1) == (6, 2)


@pytest.mark.parametrize("G", range(2, 9))
def test_stream_model_visits_every_tile_once_and_is_exact(G):
    """N = 4 000 (32 blocks, the last ragged): at G = 8 every helper sees 1, 2, 3 and 4 tiles.  Family X comes back as w in
    fp64 and fp32, family D within BAR_D; the few-block sizes (helpers without a tile) as well."""
    nblk = -(-N_SWEEP // B)
    for family, dtype in FAMILIES:
        L0 = cx.factor(N_SWEEP, family, dtype)
        w, r = cx.rhs(L0)
        x, visits = tx.stream_model(L0, r, G)
        assert x.dtype == dtype and np.array_equal(visits, np.tril(np.ones((nblk, nblk), dtype=np.int64))), G
        _held(x, w, family, what=f"G={G} {family}")
        if family == "D":
            print(f"[stream_model G={G} family D] max |x - w| = {tx.worst(x, w):.3e}")
    if G == 8:  # every helper role holds 0, 1, 2, 3, 4 (and in the last rows 5) tiles somewhere down the matrix
        for h in range(7):
            counts = {sum(1 for c in range(b - 2) if tx.stream_owner(b, c, G) == f"helper {h}") for b in range(nblk)}
            assert counts >= {0, 1, 2, 3, 4}, (h, counts)
    if G in (2, 3, 8):
        for n in N_FEW:
            L0 = cx.factor(n, "X")
            w, r = cx.rhs(L0)
            x, visits = tx.stream_model(L0, r, G)
            nb = -(-n // B)
            assert np.array_equal(visits, np.tril(np.ones((nb, nb), dtype=np.int64)))
            tx.check_vec(x, w)


@pytest.mark.parametrize("n,m,nb_outer", [(1152, 128, nb) for nb in NB_OUTER] + [(1152, 384, 256)] + RIGHT[3:],
                         ids=lambda v: str(v))
def test_right_model_visits_every_tile_once_and_is_exact(n, m, nb_outer):
    nblk = n // B
    for family, dtype in FAMILIES:
        L0 = cx.factor(n, family, dtype)
        W, Bm = tx.rhs_right(L0, m)
        for two in (False, True):
            X, visits = tx.right_model(L0, Bm, nb_outer, two)
            assert np.array_equal(visits, np.tril(np.ones((nblk, nblk), dtype=np.int64))), (nb_outer, two)
            _held(X, W, family, tx.check_block, along=1, what=f"nb_outer={nb_outer} two={two} {family}")
            if family == "D":
                print(f"[right_model n={n} m={m} nb_outer={nb_outer} two={two} family D] max |X - W| = {tx.worst(X, W):.3e}")


def _stream_mutations(nblk, G):
    """The far corner, a tf2 tile, a tf tile, and the LAST tile of a helper with several (the one its tail step takes)."""
    b = nblk - 1
    last_of_helper = b - 3 - (G - 2)  # helper G - 2's last tile of the last row
    return [(b, 0), (nblk // 2, nblk // 2 - 2), (nblk // 2 + 1, nblk // 2), (b, last_of_helper)]


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=IDS)
def test_every_mutation_of_the_streaming_solve_is_caught(family, dtype):
    """One tile product dropped or doubled, for G = 3, 4 and 6 (an odd and two even tile counts per helper): the result
    fails the check at tolerance zero AND at BAR_D with block b named first, and an entry of x_b moves by at least 1 / p."""
    n = 1536
    L0 = cx.factor(n, family, dtype)
    w, r = cx.rhs(L0)
    p = cx.PARAMS[cx._name(dtype)][0]
    for G in (3, 4, 6):
        for tile in _stream_mutations(n // B, G):
            for kind in ("dropped", "doubled"):
                x, visits = tx.stream_model(L0, r, G, (kind, tile))
                assert visits.sum() == (n // B) * (n // B + 1) // 2
                where = rf"first wrong 128-block {tile[0]} with"
                with pytest.raises(AssertionError, match=where if family == "X" else None):  # (D: rounding comes first)
                    tx.check_vec(x, w)
                with pytest.raises(AssertionError, match=where):
                    tx.check_vec(x, w, cx.BAR_D)
                blk = slice(tile[0] * B, (tile[0] + 1) * B)
                assert np.abs(x[blk].astype(np.float64) - w[blk]).max() >= 1.0 / p, (G, tile, kind)
                assert 1.0 / p == 256 * cx.BAR_D or dtype == np.float32


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=IDS)
def test_every_mutation_of_the_right_sided_sweep_is_caught(family, dtype):
    """The far corner, an in-panel tile of the chain, the first column block of an (i) range and the first column block of an
    (ii) range -- in the two-stream split and in the single update -- dropped or doubled: column block j is named first."""
    n, m, nb_outer = 1152, 128, 256
    L0 = cx.factor(n, family, dtype)
    W, Bm = tx.rhs_right(L0, m)
    p = cx.PARAMS[cx._name(dtype)][0]
    tiles = [(n // B - 1, 0), (1, 0), (2, 0), tx.right_ii_first(n, nb_outer), tx.right_ii_first(n, nb_outer, panel=1)]
    for two in (True, False):
        for tile in tiles:
            for kind in ("dropped", "doubled"):
                X, _ = tx.right_model(L0, Bm, nb_outer, two, (kind, tile))
                where = rf"\(row, 128-column block\) = \(\d+, {tile[0]}\) with"
                with pytest.raises(AssertionError, match=where if family == "X" else None):  # (D: rounding comes first)
                    tx.check_block(X, W, along=1)
                with pytest.raises(AssertionError, match=where):
                    tx.check_block(X, W, cx.BAR_D, along=1)
                blk = slice(tile[0] * B, (tile[0] + 1) * B)
                assert np.abs(X[:, blk].astype(np.float64) - W[:, blk]).max() >= 1.0 / p, (two, tile, kind)


def test_a_decayed_factor_lets_the_same_mutation_through():
    """Why the integer inputs: on the factor of a sorted 1-D ExpSquared matrix (what the streaming-solve test at N = 16 384
    uses) the far-corner tile can be dropped or doubled under every G and the solve stays inside that test's 1e-9."""
    n = 1536
    t = np.linspace(0.0, 10.0, n)
    K = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.3 ** 2) + 0.05 * np.eye(n)
    L = sla.cholesky(K, lower=True)
    y = np.sin(3.0 * t)
    want = _solve(L, y)
    for G in (3, 6):
        for kind in ("dropped", "doubled"):
            x, _ = tx.stream_model(L, y, G, (kind, (n // B - 1, 0)))
            err = np.abs(x - want).max() / np.abs(want).max()
            print(f"[decayed factor G={G}] far corner {kind}: relative error {err:.3e}")
            assert err <= 1e-9
