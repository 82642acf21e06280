"""Planted failures of the dense Cholesky: inputs, positions and the plain reference shared by test_dense_failure_cpu.py
(which proves the expected `info` on the host), test_gpu_1_failure.py and test_gpu_5_distributed.py.  No GPU here.

`info` is the 1-based index of the first pivot that is not > 0 (netlib's potrf).  Two families, for both of which the
expected value follows from the construction and not from a run:

* negative pivot: K = k(X, X) + diag(noise) with k positive semi-definite, noise = c > 0 everywhere but noise[p] = -10.
  Every pivot before p is a Schur complement of a matrix >= c I, hence >= c; pivot p is <= K[p, p] = k(0) - 10 < -7.
  So info = p + 1 whatever the rounding, in fp64 and in fp32.  (The raw-factor tests overwrite K[p, p] = -1 instead:
  pivot p <= -1.)
* NaN: `!(d > 0)`.  LAPACK builds differ on NaN (dpotrf may return info = 0), so the reference is `first_bad_pivot`
  below, never scipy.
"""
import functools

import numpy as np

import _cases
from _schedules import PANEL_CHAIN_VARIANTS
from oracle import tinygp_np as o
from test_gpu_8_fused_schedules import BOUNDARY, DIAG, KERNELS

TILE, STEP = 128, 16  # a potf2 tile and one of its 16-column elimination steps
CHAIN_LIMIT = 64 * TILE  # a panel of more block columns than this runs block by block (chol.hip)
BAD_NOISE = -10.0
AMP2, SCALE = KERNELS["k1"]
assert (AMP2, SCALE) == (1.5**2, 2.5)  # ... which is also the kernel of test_gpu_0_kernels.py::_spd

# 1. the raw factor
RAW_SIZES = (128, 256, 640)
RAW_FORMS = ("neg", "nan_diag", "nan_row", "nan_pair_step", "nan_pair_tile", "nan_pair_earlier")


def raw_positions(n):
    p = [0, 1, 15, 16, 17, 127]
    if n >= 256:
        p += [128, 129, 255]
    if n == 640:
        p += [511, 512, 639]
    return tuple(p)


# 2. every schedule: first and last column of every nb_first, sub_panel, chain_sub_panel, nb_outer and chain_full_rows
# value of tests/_schedules.py, plus both ends
SCHEDULE_N = 2560
SCHEDULE_POSITIONS = (0, 15, 16, 127, 128, 255, 256, 511, 512, 767, 768, 1023, 1024, 1025, 1535, 1536, 2047, 2048, 2431,
                      2432, 2559)
# 3. both sides of the chain limit
BOUNDARY_CASES = [(n, opts) for n, opts in BOUNDARY if n in (9100, 12200)]
# 4. ragged sizes and the padded tile
RAGGED_SIZES = (1, 100, 129, 1100, 2500)
# 5. fp32
FP32_N = 1536
FP32_POSITIONS = (0, 127, 128, 1023, 1024, 1535)
FP32_SCHEDULES = ({}, dict(chain_kernel=0, fused_step=1), dict(chain_full_rows=0))
# 6. the first of two: (n, extra options, p1, p2)
PAIR_SCHEDULES = ({}, dict(chain_kernel=0), dict(lookahead=0))
PAIRS = {
    "one_step": (2560, {}, 130, 140),
    "one_tile": (2560, {}, 130, 250),
    "two_tiles_of_a_panel": (2560, {}, 130, 300),
    "two_panels": (2560, {}, 1000, 1030),  # (nb_outer = 1024 by default)
    "two_chain_launches": (9100, dict(nb_first=8192), 8191, 8192),
}
# 7. what the caller sees: the third tile
CALLER_N, CALLER_P = 640, 300
# 8. the handle after a failure
HANDLE_CASES = ((1100, 700), (2560, 1500))
HANDLE_SCHEDULES = ({}, dict(chain_kernel=0), dict(chain_merged=0))
# the block-column driver
DIST_N = 1500
DIST_NB = (128, 512)


def ragged_positions(n):
    return tuple(sorted({0, n - 1} | ({TILE} if n > TILE else set())))


def dist_positions(nb):
    return (0, nb - 1, nb, nb + 1, 2 * nb, DIST_N - 1)


_WIDTHS = ("nb_first", "nb_outer", "sub_panel", "chain_sub_panel")


def edges(n, opts, above=False):
    """Columns of an n x n matrix at which the schedule `opts` changes hands: both ends, the last column below and the
    first at every panel or sub-panel width the options name (`above`: for a panel width also the column above), the
    chain limit, and the row at which at most chain_full_rows rows are left."""
    e = {0, n - 1}
    for key in _WIDTHS:
        w = opts.get(key, 0)
        if w > 0:
            e |= {w - 1, w} | ({w + 1} if above and key.startswith("nb_") else set())
    w = opts.get("chain_full_rows", 0)
    if w > 0:
        e |= {w - 1, w, n - w - 1, n - w}
    if n > CHAIN_LIMIT:
        e |= {CHAIN_LIMIT - 1, CHAIN_LIMIT}
    return tuple(sorted(p for p in e if 0 <= p < n))


def kernel(mod):
    return AMP2 * mod.ExpSquared(SCALE)


def inputs(n, dtype=np.float64):
    X, y = _cases.synthetic.make_inputs(n, 1)
    return X.astype(dtype), y.astype(dtype)


def bad_noise(n, ps, dtype=np.float64, c=DIAG):
    """Family 1: c everywhere, BAD_NOISE at every position of `ps` (an index or several)."""
    noise = np.full(n, c, dtype=dtype)
    noise[np.atleast_1d(ps).astype(np.intp)] = BAD_NOISE
    return noise


@functools.lru_cache(maxsize=4)
def _kxx(n, dtype):
    X = inputs(n, dtype)[0].astype(np.float64)
    K = kernel(o)(X, X)
    K.setflags(write=False)
    return K


def noise_matrix(n, ps, dtype=np.float64, c=DIAG):
    """k(X, X) + diag(bad_noise) in fp64 on the inputs as the device sees them in `dtype`."""
    K = _kxx(n, np.dtype(dtype)).copy()
    K[np.diag_indices(n)] += bad_noise(n, ps, dtype, c).astype(np.float64)
    return K


def spd(n, dtype=np.float64, diag=0.05):
    """The clean matrix of the raw-factor tests (test_gpu_0_kernels.py::_spd with its default seed)."""
    return (_kxx(n, np.dtype(np.float64)) + diag * np.eye(n)).astype(dtype)


def pair_column(p, form):
    """The column q < p of the NaN pair (p, q): in p's 16-column step, in an earlier step of p's tile, in the tile
    before p's.  None where p has no such column."""
    if form == "nan_pair_step":
        q = p - p % STEP
    elif form == "nan_pair_tile":
        q = p - p % TILE
        q = q if q < p - p % STEP else p
    else:
        q = p - p % TILE - 1
    return q if 0 <= q < p else None


def plant(K, p, form):
    """A copy of K with the failure `form` at pivot p, or None where the form does not exist at p."""
    K = K.copy()
    if form == "neg":
        K[p, p] = -1.0
    elif form == "nan_diag":
        K[p, p] = np.nan
    elif form == "nan_row":
        K[p, :] = np.nan
        K[:, p] = np.nan
    else:
        q = pair_column(p, form)
        if q is None:
            return None
        K[p, q] = K[q, p] = np.nan
    return K


def first_bad_pivot(K):
    """(info, pivots): a plain unblocked fp64 Cholesky, column by column, that stops at the first pivot which is not
    > 0.  info is its 1-based index (0: none), pivots the ones computed up to and including it."""
    A = np.asarray(K, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    d = np.empty(n)
    for j in range(n):
        d[j] = A[j, j] - L[j, :j] @ L[j, :j]
        if not d[j] > 0:
            return j + 1, d[:j + 1]
        L[j, j] = np.sqrt(d[j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0, d

