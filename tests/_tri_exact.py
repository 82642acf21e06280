"""Right-hand sides for the triangular solves on tests/_chol_exact.py's integer factors, the checks that name the first
wrong 128-block, and NumPy models of the two device solves whose bookkeeping depends on an option, in NumPy alone.

With an integer L0 and an integer solution w in {-3..3}, y = L0 w (or L0^T w, W L0^T, L0 L0^T v) is an integer array, exact
in L0's dtype, and the solution of the triangular system is w itself: no reference computation is needed.  On family X
(diagonal blocks p I, p a power of two) a solver that substitutes block by block with the inverses 1 / p returns w entry for
entry, whatever the order of its sums: every partial sum of every product is an integer (or a multiple of 1 / p) below the
limit of the format.  On family D (dense diagonal blocks, fp64) the inverses of the diagonal blocks do not terminate and the
device is held to BAR_D.  Every off-diagonal tile of L0 weighs the same, so one lost or doubled tile product moves an entry
of the solution by at least 1 / p, 256 times BAR_D (tests/test_tri_exact_cpu.py asserts it).

  stream_model  trsv_fwd_stream_kernel (chol.hip): G workgroups per block row, G - 1 helpers with the kernel's own tile
                assignment and loop, the primary with W_b, tf_b = W_b L[b, b-1] and tf2_b = W_b L[b, b-2].
  right_model   trsm_right_lt (chol.hip): panels of nb_outer columns, a chain of 128-column solves and in-panel updates,
                then one update of everything to the right, or (i) the next panel's columns and (ii) the rest.

The models are for the CPU tests (every tile is visited exactly once under every G and every panel width; a mutation of one
tile is caught) and for failure messages (stream_owner: which role owned a tile).  They are NOT the reference: that is w.
"""
import zlib

import numpy as np

from _chol_exact import BAR_D, LIMIT, PARAMS, TILE, _name  # noqa: F401  (BAR_D: re-exported for the callers)


# ---- right-hand sides ----------------------------------------------------------------------------------------------------------

def _ints(shape, tag, dtype):
    rng = np.random.default_rng(zlib.crc32(f"tri-{tag}-{shape}".encode()))
    return rng.integers(-3, 4, size=shape).astype(dtype)


def _exact_product(A, x, got, what):
    """`got` (A @ x in floating point) is the int64 product, and every partial sum of it, in any order, stays below the
    limit of the format: max_i sum_j |a_ij| max_col |x_j| < 2^53 / 2^24 on the actual arrays."""
    limit = LIMIT[_name(got.dtype)]
    Ai, xi = np.asarray(A).astype(np.int64), np.asarray(x).astype(np.int64)
    assert np.array_equal(Ai, np.asarray(A)) and np.array_equal(xi, np.asarray(x)), f"{what}: operands are not integers"
    xmax = np.abs(xi) if xi.ndim == 1 else np.abs(xi).max(axis=1)
    bound = int((np.abs(Ai) @ xmax).max())
    assert bound < limit, f"{what}: partial sums up to {bound} >= {limit}"
    want = Ai @ xi
    assert np.abs(want).max() < limit and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want), \
        f"{what}: the product is not the int64 product"
    return bound


def rhs_t(L0, seed=0):
    """(w, L0^T w): the transposed solve returns w."""
    base = np.asarray(L0)
    w = _ints(base.shape[0], f"t-{seed}", base.dtype)
    y = base.T @ w
    _exact_product(base.T, w, y, "rhs_t")
    return w, y


def rhs_k(L0, seed=0):
    """(v, u = L0^T v, r = L0 u): alpha(r) = K^-1 r = v, and the whitened vector behind its log-likelihood is u.  The tight
    bound of this module: sum_j |l_ij| |u_j| < 2^24 in fp32 (a priori 3 (p + a n)^2: n below ~2 300)."""
    base = np.asarray(L0)
    v = _ints(base.shape[0], f"k-{seed}", base.dtype)
    u = base.T @ v
    _exact_product(base.T, v, u, "rhs_k: L0^T v")
    r = base @ u
    _exact_product(base, u, r, "rhs_k: L0 (L0^T v)")
    return v, u, r


def rhs_block(L0, r, transpose=False, seed=0):
    """(W, Y) with W an integer (n, r) matrix in {-3..3} and Y = L0 W or L0^T W."""
    base = np.asarray(L0)
    A = base.T if transpose else base
    W = _ints((base.shape[0], r), f"b-{int(transpose)}-{seed}", base.dtype)
    Y = A @ W
    _exact_product(A, W, Y, "rhs_block")
    return W, Y


def rhs_right(L0, m, seed=0):
    """(W, B = W L0^T) with W an integer (m, n) matrix: B L0^-T = W."""
    base = np.asarray(L0)
    W = _ints((m, base.shape[0]), f"r-{seed}", base.dtype)
    B = W @ base.T
    _exact_product(base, W.T, B.T, "rhs_right")
    return W, B


# ---- the checks ----------------------------------------------------------------------------------------------------------------

def _bad(got, want, bar):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    with np.errstate(invalid="ignore"):
        if bar is None:
            return ~(got == want)  # (as numbers: -0 is 0, NaN is wrong)
        return ~(np.abs(got.astype(np.float64) - want) <= bar)


def _figures(g, w, bad):
    with np.errstate(invalid="ignore"):
        dev = np.abs(g.astype(np.float64) - w)[bad]
    fin = dev[np.isfinite(dev)]
    worst = f"largest deviation {fin.max():.3e}" if fin.size else "no finite deviation"
    nan = int((~np.isfinite(g)).sum())
    return f"{int(bad.sum())} of {g.size} entries wrong, {worst}{f', {nan} not finite' if nan else ''}"


def check_vec(got, want, bar=None, what="the solution"):
    """got == want entry for entry (bar=None: as numbers) or |got - want| <= bar.  Raises AssertionError naming the first
    wrong 128-block, how many of its entries are wrong, the largest deviation and the number of non-finite entries."""
    bad = _bad(got, want, bar)
    if not bad.any():
        return
    blocks = np.add.reduceat(bad, np.arange(0, bad.size, TILE)) > 0
    b = int(np.argmax(blocks))
    sl = slice(b * TILE, (b + 1) * TILE)
    raise AssertionError(f"{what} differs: first wrong 128-block {b} with {_figures(got[sl], want[sl], bad[sl])}; "
                         f"{int(blocks.sum())} block(s) wrong in all")


def check_block(got, want, bar=None, along=0, what="the solution"):
    """The same for a matrix whose axis `along` runs over the triangular system: an (n, r) result (along=0) names the first
    wrong (128-block, column), an (m, n) result (along=1) the first wrong (row, 128-column block) -- the earliest block first,
    since substitution carries an error on to every later one."""
    assert got.ndim == 2 and along in (0, 1)
    bad = _bad(got, want, bar)
    if not bad.any():
        return
    g, w, bd = (got, want, bad) if along == 0 else (got.T, want.T, bad.T)
    blocks = np.add.reduceat(bd.any(axis=1), np.arange(0, bd.shape[0], TILE)) > 0
    b = int(np.argmax(blocks))
    sl = slice(b * TILE, (b + 1) * TILE)
    other = int(np.argmax(bd[sl].any(axis=0)))
    where = f"(128-block, column) = ({b}, {other})" if along == 0 else f"(row, 128-column block) = ({other}, {b})"
    raise AssertionError(f"{what} differs: first wrong {where} with {_figures(g[sl, other], w[sl, other], bd[sl, other])} "
                         f"in it, {int(bd[sl].sum())} in the block; {int(blocks.sum())} block(s) wrong in all")


def worst(got, want):
    """max |got - want| (NaN if any entry is)."""
    return float(np.max(np.abs(got.astype(np.float64) - want)))


# ---- the models ----------------------------------------------------------------------------------------------------------------

def _padded(L0):
    """L0 on whole 128-blocks, the padding an identity (as the device keeps a ragged factor)."""
    base = np.asarray(L0)
    n = base.shape[0]
    npad = -(-n // TILE) * TILE
    if npad == n:
        return base, n
    P = np.eye(npad, dtype=base.dtype)
    P[:n, :n] = base
    return P, n


def _inverse_lower(Lbb):
    """W = Lbb^-1 row by row, as winv_kernel substitutes: W[i] = (e_i - sum_{k < i} l_ik W[k]) / l_ii."""
    m = Lbb.shape[0]
    W = np.zeros_like(Lbb)
    for i in range(m):
        row = -(Lbb[i, :i] @ W[:i])
        row[i] += 1
        W[i] = row / Lbb[i, i]
    return W


def _spoil(mutate, tile, product):
    """The product of `tile` as the model applies it: dropped (zero), doubled, or as it is."""
    if mutate is None or tuple(mutate[1]) != tuple(tile):
        return product
    assert mutate[0] in ("dropped", "doubled"), mutate
    return 0 * product if mutate[0] == "dropped" else 2 * product


def stream_groups(nblk, trsv_groups=0):
    """G as trsv() chooses it: the option clamped to 2..8, 0 = by size (3 up to 40 blocks, 4 up to 256, 6 above)."""
    if trsv_groups <= 0:
        return 3 if nblk <= 40 else (4 if nblk <= 256 else 6)
    return min(max(trsv_groups, 2), 8)


def stream_owner(b, c, G):
    """Who applies tile (b, c) of the forward streaming solve: "primary W" / "primary tf" / "primary tf2" or "helper h"."""
    assert 0 <= c <= b and G >= 2
    if b - c <= 2:
        return ("primary W", "primary tf", "primary tf2")[b - c]
    return f"helper {(b - 3 - c) % (G - 1)}"


def stream_row(b, G):
    """Block row b under G, for a failure message: every role's tiles in the order it visits them."""
    roles = [f"helper {h}: tiles {[c for c in range(b - 2) if (b - 3 - c) % (G - 1) == h]}" for h in range(G - 1)
             if b - 3 - h >= 0]
    return "; ".join(roles + [f"primary: W_{b}" + (f", tf2 on x_{b - 2}" if b >= 2 else "") + (f", tf on x_{b - 1}" if b else "")])


def stream_model(L0, y, G, mutate=None):
    """Blocked forward substitution L0 x = y in the algebraic form of trsv_fwd_stream_kernel, in L0's dtype:
         x_b = W_b (y_b - sum_h part_h) - tf2_b x_{b-2} - tf_b x_{b-1},  part_h = sum of helper h's tiles L[b, c] x_c,
    helper h = 0..G-2 owning the tiles c = b-3-h, b-3-h-(G-1), ... visited in increasing c by the kernel's two-step loop.
    mutate = (kind, (b, c)), kind "dropped" or "doubled", spoils the ONE product that tile (b, c) enters.
    Returns (x, visits) with visits[b, c] the number of products that tile (b, c) entered."""
    assert 2 <= G <= 8
    L, n = _padded(L0)
    nblk = L.shape[0] // TILE
    dt = L.dtype
    yp = np.zeros(nblk * TILE, dtype=dt)
    yp[:n] = y
    x = np.full((nblk, TILE), np.nan, dtype=dt)
    visits = np.zeros((nblk, nblk), dtype=np.int64)
    nh = G - 1

    def t(b, c):
        return L[b * TILE:(b + 1) * TILE, c * TILE:(c + 1) * TILE]

    for b in range(nblk):
        part = []
        for role in range(nh):  # ---- the helpers, each with the kernel's own bookkeeping
            last = b - 3 - role
            if last < 0:
                part.append(None)
                continue
            first = last % nh
            cnt = (last - first) // nh + 1
            acc = np.zeros(TILE, dtype=dt)

            def step(c, more):
                nonlocal acc
                assert 0 <= c <= b - 3 and (not more or c + nh <= b - 3), (b, role, c)  # (the tile prefetched is this row's)
                visits[b, c] += 1
                acc = acc + _spoil(mutate, (b, c), t(b, c) @ x[c])

            c, left = first, cnt
            while left >= 2:
                step(c, True)
                step(c + nh, left > 2)
                left -= 2
                c += 2 * nh
            if left == 1:
                step(c, False)
            part.append(acc)
        # ---- the primary: waits for exactly the helpers that have a tile
        W = _inverse_lower(t(b, b))
        pv = np.zeros(TILE, dtype=dt)
        for h in range(nh):
            if b - 3 - h < 0:
                break
            assert part[h] is not None, (b, h)
            pv = pv + part[h]
        assert all(part[h] is None for h in range(nh) if b - 3 - h < 0)
        visits[b, b] += 1
        sp = _spoil(mutate, (b, b), W @ (yp[b * TILE:(b + 1) * TILE] - pv))
        if b >= 2:
            visits[b, b - 2] += 1
            sp = sp - _spoil(mutate, (b, b - 2), (W @ t(b, b - 2)) @ x[b - 2])
        if b >= 1:
            visits[b, b - 1] += 1
            sp = sp - _spoil(mutate, (b, b - 1), (W @ t(b, b - 1)) @ x[b - 1])
        x[b] = sp
    return x.reshape(-1)[:n], visits


def right_two(n, nb_outer, lookahead=1):
    """Whether trsm_right_lt takes its two-stream form, and the panel width it uses."""
    NB = max(nb_outer, TILE) // TILE * TILE
    return bool(lookahead != 0 and n > 2 * NB), NB


def right_model(L0, B, nb_outer, two, mutate=None):
    """B (m, n) -> B L0^-T as trsm_right_lt sweeps it, n a multiple of 128: per panel of nb_outer columns a chain of
    [128-column solve, update of the panel's later columns], then the update of everything to the right -- in one piece, or
    (two) as (i) the next panel's columns and (ii) the rest.  mutate = (kind, (j, k)) spoils the ONE contribution of tile
    L[j, k] to column block j.  Returns (X, visits) with visits[j, k] the number of updates that tile L[j, k] entered."""
    L = np.asarray(L0)
    n = L.shape[0]
    assert n % TILE == 0 and B.shape[1] == n
    nblk = n // TILE
    NB = max(nb_outer, TILE) // TILE * TILE
    X = np.array(B, dtype=L.dtype)
    visits = np.zeros((nblk, nblk), dtype=np.int64)

    def update(c0, c1, k0, k1):
        """X[:, c0:c1] -= X[:, k0:k1] L[c0:c1, k0:k1]^T"""
        assert 0 <= k0 < k1 <= c0 < c1 <= n
        visits[c0 // TILE:c1 // TILE, k0 // TILE:k1 // TILE] += 1
        X[:, c0:c1] -= X[:, k0:k1] @ L[c0:c1, k0:k1].T
        if mutate is not None:
            j, k = mutate[1]
            if c0 <= j * TILE < c1 and k0 <= k * TILE < k1:
                cj, ck = slice(j * TILE, (j + 1) * TILE), slice(k * TILE, (k + 1) * TILE)
                prod = X[:, ck] @ L[cj, ck].T
                X[:, cj] += prod - _spoil(mutate, (j, k), prod)

    for k0 in range(0, n, NB):
        kb = min(NB, n - k0)
        for j0 in range(k0, k0 + kb, TILE):  # the chain
            blk = slice(j0, j0 + TILE)
            visits[j0 // TILE, j0 // TILE] += 1
            X[:, blk] = X[:, blk] @ _inverse_lower(L[blk, blk]).T
            if k0 + kb > j0 + TILE:
                update(j0 + TILE, k0 + kb, j0, j0 + TILE)
        nxt = k0 + kb
        nr = n - nxt
        if nr <= 0:
            break
        kn = min(nr, NB)
        if not two:
            update(nxt, n, k0, nxt)
            continue
        update(nxt, nxt + kn, k0, nxt)      # (i)
        if nr > kn:
            update(nxt + kn, n, k0, nxt)    # (ii)
    return X, visits


def right_ii_first(n, nb_outer, panel=0):
    """Tile (j, k): the first column block of the (ii) range behind panel `panel`, and the first block of that panel."""
    NB = max(nb_outer, TILE) // TILE * TILE
    j = ((panel + 2) * NB) // TILE
    assert j * TILE < n, (n, nb_outer, panel)
    return j, panel * NB // TILE
