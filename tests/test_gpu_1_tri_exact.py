"""GPU: the triangular solves on a resident factor (chol.hip: trsv_fwd/bwd_stream_kernel, winv_kernel, the launch-per-block
kernels, trsm_right_lt in both of its forms), held to integer inputs on every route.

The factors are tests/_chol_exact.py's integer L0, the right-hand sides tests/_tri_exact.py's: y = L0 w, L0^T w, W L0^T or
L0 L0^T v with integer w, so the solution is known in advance and every tile of L0 weighs in it.  Family X (diagonal blocks
p I) must come back EXACTLY, in fp64 and fp32: W_b = I / p, tf_b = L[b, b-1] / p, every partial sum an integer or a multiple
of 1 / p below 2^53 / 2^24.  Family D (dense diagonal blocks) is held to BAR_D = 2^-20 against w, 256 times below the effect
of one lost tile product; each D case prints its largest deviation before it asserts.  tests/test_tri_exact_cpu.py proves
the inputs, and that a dropped or doubled tile fails these checks where a decayed kernel-matrix factor lets it through.

  1  the streaming solves under every trsv_groups (G - 1 helpers per block row: their tile lists, the two-step loop and its
     tails, the primary's wait list all change with G), and the launch-per-block kernels
  2  few blocks: helpers without a tile return, and the primary does not wait for them
  3  trsm_right_lt through the device pointer at every panel split, one stream and two
  4  the same through the solver with the defaults at N = 2 400 (more than two panels of 1 024: the two-stream form)
"""
import re

import numpy as np
import pytest

import _chol_exact as cx
import _lowlevel as ll
import _tri_exact as tx
from test_gpu_8_fused_schedules import RTOL_REF, _options
from tinygp_amd import kernels, noise
from tinygp_amd.solvers import DirectSolver

pytestmark = pytest.mark.gpu

N_SWEEP, N_ALPHA32, N_SOLVER = 4000, 1536, 2400  # 32 blocks, the last ragged; 12 blocks: rhs_k's fp32 bound; 19 blocks
FAMILIES = [("X", np.float64), ("D", np.float64), ("X", np.float32)]
IDS = ["X-f64", "D-f64", "X-f32"]
# the value comes back in the solver's dtype: the fp64 sum rounded ONCE to fp32 (2^-24) on top of the fp64 bar
RTOL_VALUE = {np.float64: RTOL_REF, np.float32: RTOL_REF + 2.0 ** -24}


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _bar(family):
    return None if family == "X" else cx.BAR_D


class _Case:
    """A solver on K = L0 L0^T through the covariance channel (the kernel only has to lower: it is not evaluated), factored,
    with its factor checked against L0 first: a wrong solve is then not the factor's."""

    def __init__(self, n, family, dtype):
        self.n, self.family, self.dtype = n, family, dtype
        self.L0 = cx.factor(n, family, dtype)
        self.s = DirectSolver(kernels.ExpSquared(1.0), np.arange(n, dtype=dtype), noise.Diagonal(np.zeros(n, dtype=dtype)),
                              covariance=cx.matrix(self.L0))
        assert self.s.dtype == dtype
        got = self.s.scale_tril
        assert self.s.info == 0
        if family == "X":
            cx.check_exact(got, self.L0)
        else:
            cx.check_close(got, self.L0, cx.BAR_D)
        self.w, self.r = cx.rhs(self.L0)
        self.wt, self.rt = tx.rhs_t(self.L0)
        self._k = None

    @property
    def k(self):
        if self._k is None:
            self._k = tx.rhs_k(self.L0)
        return self._k


@pytest.fixture(scope="module")
def cases():
    """One solver per (n, family, dtype) for the module, closed at its end."""
    made = {}

    def get(n, family, dtype):
        key = (n, family, np.dtype(dtype).name)
        if key not in made:
            made[key] = _Case(n, family, dtype)
        return made[key]

    yield get
    for c in made.values():
        c.s.close()


def _thrice(solve, what):
    """Three runs of a solve, the same bits each time; returns the first."""
    out = [solve() for _ in range(3)]
    for o in out[1:]:
        for a, b in zip(out[0] if isinstance(out[0], tuple) else (out[0],), o if isinstance(o, tuple) else (o,)):
            assert np.array_equal(_bits(np.atleast_1d(np.asarray(a))), _bits(np.atleast_1d(np.asarray(b)))), \
                f"{what}: not the same bits on a repeat"
    return out[0]


def _check_solution(x, w, case, what, G=None):
    """check_vec; a D case prints its figure first; a wrong forward block is reported with the roles of its row."""
    if case.family == "D":
        print(f"\n[{what}] max |x - w| = {tx.worst(x, w):.3e} (bar {cx.BAR_D:.3e})")
    try:
        tx.check_vec(x, w, _bar(case.family), what=what)
    except AssertionError as e:
        m = re.search(r"128-block (\d+)", str(e))
        if G is None or m is None:
            raise
        raise AssertionError(f"{e}\nblock row {m.group(1)} under G = {G}: {tx.stream_row(int(m.group(1)), G)}") from None


def _check_solves(c, ck, tag, G=None):
    """Both directions on `c`, alpha on `ck` (the same case unless fp32 needs the smaller N), and the separate value."""
    s = c.s
    x = _thrice(lambda: s.solve_triangular(c.r), f"{tag} L^-1")
    _check_solution(x, c.w, c, f"{tag} L^-1 (L0 w)", G)
    xt = _thrice(lambda: s.solve_triangular(c.rt, transpose=True), f"{tag} L^-T")
    _check_solution(xt, c.wt, c, f"{tag} L^-T (L0^T w)")
    v, u, rk = ck.k
    a, value = _thrice(lambda: ck.s.alpha(rk), f"{tag} alpha")
    assert a.dtype == c.dtype
    _check_solution(a, v, ck, f"{tag} alpha(L0 L0^T v) n={ck.n}", G)
    rtol = RTOL_VALUE[c.dtype]
    np.testing.assert_allclose(float(value), cx.loglik(ck.L0, u), rtol=rtol)
    # the already-factored handle: tgp_solver_logprob (the streaming solve on the resident factor + the reduction)
    np.testing.assert_allclose(float(s.log_probability(c.r)), cx.loglik(c.L0, c.w), rtol=rtol)


# ---- 1: every G, and the launch-per-block kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("family,dtype", FAMILIES, ids=IDS)
@pytest.mark.parametrize("groups", [0, 2, 3, 4, 5, 6, 7, 8], ids=lambda g: f"G{g}")
def test_streaming_solves_are_exact_under_every_group_count(cases, groups, family, dtype):
    """N = 4 000: 32 block rows, the last ragged; at G = 8 every helper role sees 1, 2, 3, 4 and 5 tiles down the matrix, at
    G = 2 one helper sees up to 29.  Forward, backward, alpha = K^-1 r (forward with G groups, then backward with 2 on the
    same work buffer) and the separate log-probability under each value of trsv_groups, three times with the same bits."""
    c = cases(N_SWEEP, family, dtype)
    ck = c if dtype == np.float64 else cases(N_ALPHA32, family, dtype)
    with _options(trsv_groups=groups):
        _check_solves(c, ck, f"{family} {np.dtype(dtype).name} trsv_groups={groups}",
                      G=tx.stream_groups(-(-c.n // cx.TILE), groups))


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=IDS)
def test_launch_per_block_solves_are_exact(cases, family, dtype):
    """stream_trsv = 0: one launch pair per block; on family D their 16 x 16 sub-steps see dense diagonal blocks."""
    c = cases(N_SWEEP, family, dtype)
    ck = c if dtype == np.float64 else cases(N_ALPHA32, family, dtype)
    with _options(stream_trsv=0):
        _check_solves(c, ck, f"{family} {np.dtype(dtype).name} stream_trsv=0")


# ---- 2: few blocks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [2, 3, 8], ids=lambda g: f"G{g}")
@pytest.mark.parametrize("n", [128, 256, 384, 512, 640, 900])
def test_few_blocks_where_helpers_have_no_tile(cases, n, groups):
    """1 to 8 block rows: in rows 0..2 no helper has a tile, in row b only the first b - 2 have one; they return at once and
    the primary waits for exactly the others."""
    c = cases(n, "X", np.float64)
    G = tx.stream_groups(-(-n // cx.TILE), groups)
    tag = f"n={n} trsv_groups={groups}"
    with _options(trsv_groups=groups):
        _check_solution(c.s.solve_triangular(c.r), c.w, c, f"{tag} L^-1", G)
        _check_solution(c.s.solve_triangular(c.rt, transpose=True), c.wt, c, f"{tag} L^-T")
        v, u, rk = c.k
        a, value = c.s.alpha(rk)
        _check_solution(a, v, c, f"{tag} alpha", G)
        np.testing.assert_allclose(float(value), cx.loglik(c.L0, u), rtol=RTOL_REF)


# ---- 3: trsm_right_lt through the device pointer ---------------------------------------------------------------------------------

def _right(n, m, family, dtype, **options):
    """B = W L0^T must come back as W; a two-stream case three times with the same bits."""
    L0 = cx.factor(n, family, dtype)
    W, Bm = tx.rhs_right(L0, m)
    ctx_nb = options.get("nb_outer", 1024)
    two, NB = tx.right_two(n, ctx_nb, options.get("lookahead", 1))
    what = f"trsm_right_lt {family} {np.dtype(dtype).name} n={n} m={m} {options or 'defaults'} ({'two streams' if two else 'one stream'})"
    L = np.asarray(L0)
    X = ll.trsm_right_lt(L, Bm, **options)
    for _ in range(2 if two else 0):
        again = ll.trsm_right_lt(L, Bm, **options)
        assert np.array_equal(_bits(np.ascontiguousarray(X)), _bits(np.ascontiguousarray(again))), f"{what}: not the same bits"
    if family == "D":
        print(f"\n[{what}] max |X - W| = {tx.worst(X, W):.3e} (bar {cx.BAR_D:.3e})")
    try:
        tx.check_block(np.ascontiguousarray(X), W, _bar(family), along=1, what=what)
    except AssertionError as e:
        j = int(re.search(r"block\) = \(\d+, (\d+)\)", str(e)).group(1))
        k0 = j * cx.TILE // NB * NB
        raise AssertionError(f"{e}\ncolumn block {j} lies in the panel of columns {k0}..{min(k0 + NB, n)}: updated by "
                             f"{'(i)' if two else 'the one update'} of the panel before it"
                             f"{', by (ii) of every earlier one' if two else ''}, then by its own chain") from None


@pytest.mark.parametrize("family", ["X", "D"])
@pytest.mark.parametrize("lookahead", [1, 0], ids=["two", "one"])
@pytest.mark.parametrize("nb_outer", [128, 256, 512])
@pytest.mark.parametrize("m", [128, 384])
def test_right_sided_solve_at_every_panel_split(m, nb_outer, lookahead, family):
    """n = 1 152: nine panels of 128; four of 256 and a narrow last one; 512 | 512 | 128, where the first (ii) has 128 columns
    and the second panel none.  lookahead = 1 takes the two-stream form (n > 2 nb_outer), lookahead = 0 the single stream."""
    assert tx.right_two(1152, nb_outer, lookahead)[0] == bool(lookahead)
    _right(1152, m, family, np.float64, nb_outer=nb_outer, lookahead=lookahead)


@pytest.mark.parametrize("family", ["X", "D"])
@pytest.mark.parametrize("n", [2304, 2176])
def test_right_sided_solve_with_the_default_panels(n, family):
    """The defaults (panels of 1 024, two streams above n = 2 048): 1 024 | 1 024 | 256, and | 128."""
    assert tx.right_two(n, 1024)[0]
    _right(n, 128, family, np.float64)


def test_right_sided_solve_in_fp32():
    _right(1152, 128, "X", np.float32, nb_outer=256)


# ---- 4: the same through the solver ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,transpose", [(2, False), (130, False), (2, True)], ids=["R2", "R130", "R2-T"])
def test_solver_multi_rhs_solves_past_two_panels(cases, r, transpose):
    """N = 2 400 (19 blocks, ragged, more than 2 x 1 024): solve_triangular(Y) pads R to 128 / 256 rows and takes the
    two-stream trsm_right_lt; transposed it runs one backward streaming solve per column.  Every result equals W."""
    c = cases(N_SOLVER, "X", np.float64)
    W, Y = tx.rhs_block(c.L0, r, transpose)
    X = _thrice(lambda: c.s.solve_triangular(Y, transpose=transpose), f"R={r} transpose={transpose}")
    assert X.shape == W.shape
    tx.check_block(X, W, what=f"solve_triangular n={N_SOLVER} R={r} transpose={transpose}")
