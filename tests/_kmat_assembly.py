"""The dense assembly (csrc/kmat.hip, launch_kmat_cols) in every form the solvers call: inputs, the image a correct call
leaves in a sentinel-filled buffer, and the check that names the first wrong tile -- in NumPy and the oracle alone.

  inputs    points(n, d, dtype): the first n of 640 sorted points on a segment, at integer positions (lattice(), kept under
            tests/golden) times a power of two.  Uniform random points cannot keep the entries of a row apart: a row has
            n^2 / 4 pairs of one entry left and one right of the diagonal, the matrix n^3 / 4, and each pair agrees to
            1e-6 with probability ~4e-7, so a few dozen do at n = 385.  The lattice is built so that no point sees the
            same distance to its left and to its right, and near the diagonal, where smooth kernels are flat, not even
            nearly: separation() -- no two entries of a row or column within 1e-6 relative -- then holds for every
            program here, a row being monotone on either side of the diagonal.  d > 1: the same segment along a direction
            with d distinct components.  Every coordinate is exact in float32.  This departs from uniform clouds on
            purpose: for d > 1 the points are collinear and no coordinate is negative; points in general position and of
            both signs are what tests/test_gpu_0_kernels.py and tests/test_gpu_2_kmat_edges.py evaluate.
            noise(n) = 0.5 + i / 1024: exact in both dtypes, neighbours 1e-3 apart.
            int_points / int_noise: coordinates iid in {-3 .. 3}, noise 1 + (i mod 7); DotProduct on them is exact.
  Form      one call of tgp_kmat: n1, n2, x_off (X1 = X2 = the points from x_off on), rows_out, cols_out, ld, lower,
            with_diag, out_off.  The three solver call forms are instances (square_padded, block_column, plain).
  expected  (image, mask): the ld x cols_out column-major buffer behind a correct call, NaN where the call must not write,
            and the class of every entry.
  check     raises AssertionError naming the first wrong 128 x 128 tile, the class of its first wrong entry and what is
            wrong with it.

No GPU and no library here: tests/test_kmat_assembly_cpu.py proves that the checks have teeth and that the inputs keep
errors apart from the bars, tests/test_gpu_2_kmat_assembly.py runs the device against them.
"""
import dataclasses
import functools
from pathlib import Path

import numpy as np

from oracle import tinygp_np as o

TILE = 128
LATTICE_FILE = Path(__file__).resolve().parent / "golden" / "kmat_assembly_lattice.npz"
SPAN = 3.1  # length of the segment at most: with scales near 1 the entries run from ~0.01 to 1
PHI = (1.0 + 5.0 ** 0.5) / 2.0
MAX_POINTS = 640
GAP = 307  # mean gap of the lattice in its units: 640 points span 3 at a unit of 2^-16
# A smooth leaf falls off from the diagonal like 1 - c d^2 with c >= 0.58 at the scales below (Matern52(1.2); ExpSquared(0.9)
# has 0.62): two entries of a row at distances d and e differ relatively by c |d^2 - e^2|.  Three times the 1e-6 that
# separation() must show, at the finest unit: |d^2 - e^2| >= 3e-6 / 0.58 * 2^32 lattice units squared.
SQ_GAP = 22300

VALUE, VALUE_NOISE, ONE, ZERO, UNTOUCHED = range(5)
CLASS_NAME = {VALUE: "kernel value", VALUE_NOISE: "kernel value plus noise", ONE: "padding one", ZERO: "padding zero",
              UNTOUCHED: "untouched"}


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def build_lattice(n_max=MAX_POINTS):
    """Increasing integers T_0 = 0 < T_1 < ...: the positions of the points in units of a power of two.  Gaps near
    GAP (1/2 + frac(m phi)); a candidate moves on by one unit until, for every earlier point i, its distance d to the
    right of i and every distance e to the left of i satisfy |d^2 - e^2| >= SQ_GAP (which implies d != e)."""
    T = np.zeros(n_max, dtype=np.int64)
    # [i, j < i]: the squared distances to the left of point i; elsewhere a value no d^2 comes near
    left2 = np.full((n_max, n_max), -(1 << 60), dtype=np.int64)
    for m in range(1, n_max):
        c = T[m - 1] + int(GAP * (0.5 + (m * PHI) % 1.0))
        while True:
            d = c - T[:m]
            if not (np.abs(left2[:m, :m] - (d * d)[:, None]) < SQ_GAP).any():
                break
            c += 1
        T[m] = c
        left2[m, :m] = (c - T[:m]) ** 2
    return T


@functools.lru_cache(maxsize=None)
def lattice():
    """build_lattice() as kept under tests/golden (three seconds to rebuild; tests/test_kmat_assembly_cpu.py holds the file
    to the construction)."""
    T = np.load(LATTICE_FILE)["T"].astype(np.int64)
    assert T.shape == (MAX_POINTS,)
    T.flags.writeable = False
    return T


# (d > 1) numerators over 64 of the direction's components: distinct, so that no two coordinates can be exchanged unnoticed
_DIRECTION = {2: (24, 40), 3: (12, 20, 32), 4: (8, 12, 18, 26), 5: (6, 9, 13, 16, 20), 16: tuple(range(1, 17))}


@functools.lru_cache(maxsize=None)
def points(n, d=1, dtype=np.float64):
    """(n,) for d = 1, else (n, d), read-only.  The first n positions of lattice() times the largest power of two that
    keeps the segment within SPAN, from 0.25 on; d > 1: half that segment along _DIRECTION[d] / 64 from (k + 1) / 32.
    Every coordinate has at most 24 significant bits: float32 and float64 hold the same points."""
    assert 1 <= n <= MAX_POINTS
    T = lattice()[:n]
    unit = 2.0 ** np.floor(np.log2(SPAN / max(int(T[-1]), 1)))
    t = T * unit
    if d == 1:
        X = 0.25 + t
    else:
        c = np.array(_DIRECTION[d], dtype=np.float64) / 64.0
        X = ((np.arange(d) + 1) / 32.0)[None, :] + (0.5 * t)[:, None] * c[None, :]
    out = np.ascontiguousarray(X, dtype=dtype)
    assert np.array_equal(out.astype(np.float64), X)
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def noise(n, dtype=np.float64):
    assert n <= 1024
    v = (0.5 + np.arange(n) / 1024.0).astype(dtype)
    v.flags.writeable = False
    return v


@functools.lru_cache(maxsize=None)
def int_points(n, d, dtype=np.float64):
    rng = np.random.default_rng(7000 + 100 * d + n)
    X = rng.integers(-3, 4, size=(n, d)).astype(dtype)
    X = X[:, 0].copy() if d == 1 else X
    X.flags.writeable = False
    return X


@functools.lru_cache(maxsize=None)
def int_noise(n, dtype=np.float64):
    v = (1 + np.arange(n) % 7).astype(dtype)
    v.flags.writeable = False
    return v


def int_matrix(X):
    """X X^T as int64 (the reference of the integer family) and the largest sum_k |x_ik x_jk| + noise any partial sum can reach."""
    P = np.asarray(X).reshape(np.shape(X)[0], -1).astype(np.int64)
    return P @ P.T, int((np.abs(P) @ np.abs(P).T).max()) + 7


# ---- programs: name -> build(module); the module is oracle_kernels below or tinygp_amd.kernels ----------------------------------

class _Polynomial(o.Kernel):
    """Reference kernels/base.py:254-256: ((x1 / scale) . (x2 / scale) + sigma^2) ** order"""

    def __init__(self, order, scale=1.0, sigma=0.0):
        self.order, self.scale, self.sigma = order, scale, sigma

    def evaluate(self, X1, X2):
        return (np.sum((X1 / self.scale) * (X2 / self.scale), axis=-1) + np.square(self.sigma)) ** self.order


class _OracleKernels:
    """oracle.tinygp_np with the reference's Polynomial restated (the oracle module has no dot-product kernels)."""
    Polynomial = _Polynomial

    def __getattr__(self, name):
        return getattr(o, name)


oracle_kernels = _OracleKernels()

_LEAVES = {"exp": ("Exp", 1.1), "expsq": ("ExpSquared", 0.9), "m32": ("Matern32", 0.8), "m52": ("Matern52", 1.2)}
_METRICS = {"l1": "L1Distance", "l2": "L2Distance"}


def _leaf(k, leaf, metric):
    cls, scale = _LEAVES[leaf]
    return getattr(k, cls)(scale, distance=getattr(k, _METRICS[metric])())


def _programs():
    out = {}
    for leaf in _LEAVES:
        for metric in _METRICS:
            out[f"{leaf}_{metric}"] = functools.partial(_leaf, leaf=leaf, metric=metric)
            out[f"amp*{leaf}_{metric}"] = lambda k, leaf=leaf, metric=metric: 1.7 * _leaf(k, leaf, metric)
            out[f"{leaf}_{metric}*amp"] = lambda k, leaf=leaf, metric=metric: _leaf(k, leaf, metric) * 0.6
    out["sum_fam1"] = lambda k: k.ExpSquared(0.9) + 0.3 * k.Matern32(0.8)
    # (the period, 7, is more than twice SPAN: sin^2 stays monotone over every distance of the inputs)
    out["sum_fam0"] = lambda k: 1.5 * k.Matern32(1.0) + 0.9 * k.ExpSineSquared(scale=7.0, gamma=1.3)
    out["poly"] = lambda k: k.Polynomial(order=2.0, scale=3.5, sigma=0.5)
    return out


PROGRAMS = _programs()
STRAIGHT_LINE = [name for name in PROGRAMS if name not in ("sum_fam1", "sum_fam0", "poly")]  # fast_prog accepts them at d <= 3
TRIGONOMETRIC = ("sum_fam0",)
FAST, GENERAL = "amp*m32_l1", "sum_fam1"  # the pair that meets every form: both measure L1 (sum_fam1 also L2)


@functools.lru_cache(maxsize=256)
def oracle_matrix(name, n, d=1, dtype=np.float64):
    """K(X, X) of PROGRAMS[name] by the oracle in float64 on points(n, d, dtype), read-only."""
    X = points(n, d, dtype).astype(np.float64)
    K = PROGRAMS[name](oracle_kernels)(X, X)
    K.flags.writeable = False
    return K


def separation(K):
    """The smallest relative distance between two entries in different positions of one row or one column, the diagonal
    aside (inf below three points)."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    if n < 3:
        return np.inf
    best = np.inf
    for A in (K, K.T):
        off = A[~np.eye(n, dtype=bool)].reshape(n, n - 1)
        s = np.sort(off, axis=1)
        best = min(best, float(np.min(np.diff(s, axis=1) / np.maximum(np.abs(s[:, 1:]), np.abs(s[:, :-1])))))
    return best


# ---- the form of a call and the image it leaves ----------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Form:
    n1: int
    n2: int
    x_off: int = 0          # X1 = X2 = the points from this index on; diag is offset by it too
    rows_out: int = -1      # default n1
    cols_out: int = -1      # default n2
    ld: int = -1            # default rows_out
    lower: bool = False
    with_diag: bool = False
    out_off: int = 0        # elements by which `out` is moved inside its allocation

    def __post_init__(self):
        if self.rows_out < 0:
            object.__setattr__(self, "rows_out", self.n1)
        if self.cols_out < 0:
            object.__setattr__(self, "cols_out", self.n2)
        if self.ld < 0:
            object.__setattr__(self, "ld", self.rows_out)
        assert self.rows_out >= self.n1 and self.cols_out >= self.n2 and self.ld >= self.rows_out

    def __str__(self):
        return (f"{self.n1}x{self.n2}_at{self.x_off}_out{self.rows_out}x{self.cols_out}_ld{self.ld}"
                f"{'_lower' if self.lower else ''}{'_diag' if self.with_diag else ''}{f'_off{self.out_off}' if self.out_off else ''}")


def round_up(n, m=TILE):
    return -(-n // m) * m


def plain(n):
    """_device.kmat's form (and, with_diag, tgp_solver_covariance's): square, nothing padded."""
    return Form(n, n)


def square_padded(n, size=None, ld_extra=0, lower=True, with_diag=True, out_off=0):
    """assemble_lower's form (capi.hip): rows_out = cols_out = size (default the next multiple of 128)."""
    size = round_up(n) if size is None else size
    return Form(n, n, 0, size, size, size + ld_extra, lower, with_diag, out_off)


def block_column(n, nb, j0):
    """assemble_columns' form (dist.hip) for the block column at j0: a tall rectangle inside a buffer of npad rows."""
    npad = round_up(n, nb)
    return Form(max(n - j0, 0), max(min(nb, n - j0), 0), min(j0, n), npad - j0, nb, npad, True, True, j0)


def expected(form, K, diag=None):
    """(image, mask), both (ld, cols_out), entry [i, j] = row i, column j of the column-major buffer: what a correct call
    leaves in a buffer pre-filled with a sentinel.  image is long double (it holds both dtypes' values and the diagonal's sum
    exactly) and NaN where mask is UNTOUCHED: rows rows_out .. ld - 1 and, with `lower`, every 128 x 128 tile strictly above
    the diagonal tile of its column (include/tgp_hip.h: "only 128-tiles on/below the diagonal are written"; the upper
    triangle inside a diagonal tile is).  K is the matrix over ALL points, diag the noise over all points."""
    f = form
    i = np.arange(f.rows_out)[:, None]
    j = np.arange(f.cols_out)[None, :]
    inside = (i < f.n1) & (j < f.n2)
    val = np.where(i == j, np.longdouble(1), np.longdouble(0)) + np.zeros((f.rows_out, f.cols_out), dtype=np.longdouble)
    cls = np.where(i == j, ONE, ZERO).astype(np.int8) + np.zeros((f.rows_out, f.cols_out), dtype=np.int8)
    val[:f.n1, :f.n2] = np.asarray(K)[f.x_off:f.x_off + f.n1, f.x_off:f.x_off + f.n2]
    cls[inside] = VALUE
    if f.with_diag:
        assert diag is not None
        k = np.arange(min(f.n1, f.n2))
        val[k, k] += np.asarray(diag)[f.x_off + k].astype(np.longdouble)
        cls[k, k] = VALUE_NOISE
    written = (i // TILE >= j // TILE) if f.lower else np.ones((f.rows_out, f.cols_out), dtype=bool)
    image = np.full((f.ld, f.cols_out), np.nan, dtype=np.longdouble)
    mask = np.full((f.ld, f.cols_out), UNTOUCHED, dtype=np.int8)
    image[:f.rows_out][written] = val[written]
    mask[:f.rows_out][written] = cls[written]
    return image, mask


# ---- the buffer and the check ------------------------------------------------------------------------------------------------

_SENTINEL_BITS = {"float64": np.uint64(0x7FF8DEADBEEF0BAD), "float32": np.uint32(0x7FC0BEEF)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def sentinel(dtype):
    """The NaN that fills the buffer in front of a call: no arithmetic produces its payload."""
    b = _SENTINEL_BITS[np.dtype(dtype).name]
    return np.array([b]).view(dtype)[0]


def is_sentinel(a):
    return _bits(a) == _SENTINEL_BITS[a.dtype.name]


def filled(form, dtype, tail=0):
    """The flat allocation in front of the call: out_off + ld * cols_out + tail sentinels."""
    return np.full(form.out_off + form.ld * form.cols_out + tail, sentinel(dtype), dtype=dtype)


def image_of(flat, form):
    """(ld, cols_out) view [i, j] of the flat column-major allocation, and the elements in front of and behind it."""
    size = form.ld * form.cols_out
    body = flat[form.out_off:form.out_off + size].reshape(form.cols_out, form.ld).T
    return body, np.concatenate([flat[:form.out_off], flat[form.out_off + size:]])


def deviation(got, want):
    """|got - want| in units of the last place of got's dtype at |want| (long double arithmetic)."""
    w = np.abs(want)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.where(np.isfinite(w), w, 0).astype(got.dtype)).astype(np.longdouble)
        return np.abs(got.astype(np.longdouble) - want) / ulp


def _bad_values(got, want, bar):
    kind = bar[0]
    with np.errstate(invalid="ignore"):
        if kind == "ulp":
            ok = deviation(got, want) <= bar[1]
        elif kind == "tol":  # (rtol, atol) like numpy.testing.assert_allclose
            ok = np.abs(got.astype(np.longdouble) - want) <= bar[2] + bar[1] * np.abs(want)
        elif kind == "abs":  # a scalar or an (ld, cols_out) array of absolute bars
            ok = np.abs(got.astype(np.longdouble) - want) <= bar[1]
        else:
            raise ValueError(bar)
    return ~ok  # (NaN compares false: not ok)


def check(got, want, mask, bars, label="", untouched=True):
    """got (ld, cols_out) in the device's dtype against expected()'s (want, mask).  bars: class -> ("ulp", k) |
    ("tol", rtol, atol) | ("abs", a) for VALUE and VALUE_NOISE; the padding is held exactly and UNTOUCHED to the sentinel's
    bits (untouched=False: not looked at -- a buffer that no sentinel filled).  Raises AssertionError with the first wrong 128 x 128 tile (column by column), the class of its first wrong entry
    and whether a sentinel was overwritten, a written entry was left as sentinel or a value is off, and by how many ulp."""
    assert got.shape == want.shape == mask.shape, (got.shape, want.shape, mask.shape)
    sent = is_sentinel(got)
    overwritten = (mask == UNTOUCHED) & ~sent & bool(untouched)
    left = (mask != UNTOUCHED) & sent
    off = np.zeros(got.shape, dtype=bool)
    for cls in (VALUE, VALUE_NOISE, ONE, ZERO):
        sel = (mask == cls) & ~sent
        if sel.any():
            bar = bars[cls] if cls in (VALUE, VALUE_NOISE) else ("abs", 0)
            if bar[0] == "abs" and np.ndim(bar[1]):
                bar = ("abs", np.asarray(bar[1])[sel])
            off[sel] = _bad_values(got[sel], want[sel], bar)
    bad = overwritten | left | off
    if not bad.any():
        return
    ld, w = got.shape
    tr, tc = -(-ld // TILE), -(-w // TILE)
    pad = np.zeros((tr * TILE, tc * TILE), dtype=bool)
    pad[:ld, :w] = bad
    tiles = pad.reshape(tr, TILE, tc, TILE).any(axis=(1, 3))
    tj, ti = np.argwhere(tiles.T)[0]
    sl = (slice(ti * TILE, (ti + 1) * TILE), slice(tj * TILE, (tj + 1) * TILE))
    c, r = np.argwhere(bad[sl].T)[0]
    r, c = int(r + ti * TILE), int(c + tj * TILE)
    if overwritten[r, c]:
        what = f"a sentinel was overwritten with {got[r, c]!r}"
    elif left[r, c]:
        what = f"a written entry was left as sentinel (expected {float(want[r, c])!r})"
    else:
        dev = float(deviation(got[r:r + 1, c:c + 1], want[r:r + 1, c:c + 1])[0, 0])
        what = f"the value is off by {dev:.3g} ulp (got {got[r, c]!r}, expected {float(want[r, c])!r})"
    counts = ", ".join(f"{int(x[sl].sum())} {n}" for x, n in ((overwritten, "overwritten"), (left, "left as sentinel"),
                                                               (off, "off")) if x[sl].any())
    raise AssertionError(f"{label}{': ' if label else ''}first wrong 128x128 tile (i, j) = ({ti}, {tj}), entry ({r}, {c}) of class "
                         f"'{CLASS_NAME[int(mask[r, c])]}': {what}; in this tile {counts}; {int(tiles.sum())} tile(s) wrong in all")


def render(want, mask, dtype):
    """The buffer a correct device leaves: expected()'s image rounded to `dtype`, the sentinel where nothing is written."""
    with np.errstate(invalid="ignore"):
        got = want.astype(dtype)
    got[mask == UNTOUCHED] = sentinel(dtype)
    return got


def worst(got, want, mask, cls=VALUE):
    """max |got - want| / |want| over the entries of one class (0 if there are none)."""
    sel = mask == cls
    if not sel.any():
        return 0.0
    return float(np.max(np.abs(got[sel].astype(np.longdouble) - want[sel]) / np.abs(want[sel])))


# ---- the cases of tests/test_gpu_2_kmat_assembly.py (tests/test_kmat_assembly_cpu.py asserts separation() on every one) ---------

SIZES = (1, 127, 128, 129, 255, 256, 257, 385)  # every program at d = 1
LARGE = 640                                      # once: 15 tiles in the triangular grid
DIMS = (1, 2, 3, 4, 5, 16)                       # the fast kernel's three forms, the general kernel's last static one, the dynamic loop
DIM_SIZES = (129, 257)
FORM_SIZES = (128, 129, 257, 385)
COLUMN_SIZES = (257, 385, 640)
COLUMN_WIDTHS = (128, 256)
SOLVER_SIZES = (257, 385, 640)
SOLVER_PROGRAMS = (FAST, "m52_l2*amp")           # the first and the second factorisation of one handle
COVARIANCE_SIZES = (127, 128, 129, 257)
KDIAG_SIZES = (255, 256, 257, 513)
KDIAG_PROGRAMS = ("sum_fam0", "sum_fam1")


def float_inputs():
    """(program, n, d) of every kernel matrix on points() that the GPU file evaluates."""
    out = {(name, n, 1) for name in PROGRAMS for n in SIZES}
    out |= {(name, n, d) for name in (FAST, GENERAL) for n in DIM_SIZES for d in DIMS}
    out |= {(name, n, 1) for name in (FAST, GENERAL) for n in FORM_SIZES + COLUMN_SIZES + COVARIANCE_SIZES + (LARGE,)}
    out |= {(name, n, 1) for name in SOLVER_PROGRAMS for n in SOLVER_SIZES}
    out |= {(name, n, 1) for name in KDIAG_PROGRAMS for n in KDIAG_SIZES}
    return sorted(out)


def int_inputs():
    """(n, d) of every integer point set the GPU file uses."""
    return sorted({(n, 1) for n in SIZES} | {(n, d) for n in DIM_SIZES for d in DIMS} | {(n, 1) for n in KDIAG_SIZES})


def forms(n):
    """Every form of one square call that the GPU file holds to the plain image, deduplicated."""
    out = [Form(n, n, with_diag=True), Form(n, n, lower=True), Form(n, n, lower=True, with_diag=True)]
    for size in (n, round_up(n), round_up(n) + TILE):       # the last: one tile that is identity alone
        for extra in (0, 1, 2):                             # an odd ld takes the general kernel alone
            out.append(square_padded(n, size, extra))
        if size % 2 == 0:
            out.append(square_padded(n, size, 0, out_off=1))  # an even ld, but `out` is not 16-byte aligned
    return list(dict.fromkeys(out))
