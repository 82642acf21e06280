"""GPU: the dense assembly (csrc/kmat.hip, launch_kmat_cols) held entry by entry in every form the solvers call.

tests/test_gpu_0_kernels.py and tests/test_gpu_2_kmat_edges.py reach the assembly through `_device.kmat`: rectangular, no
fused noise, no padding, ld = n1.  The solvers call it lower-only with fused noise and identity padding, cut into two column
tile ranges (assemble_lower, capi.hip), as a tall rectangle per block column with X, diag and out offset (assemble_columns,
dist.hip), and with an odd leading dimension (tgp_solver_covariance).  Here every such call goes into a buffer that
tgp_memcpy_h2d filled with a sentinel NaN, and tests/_kmat_assembly.py's check names the first wrong 128 x 128 tile: a wrong
value, a tile not written, a write where the contract has none.

  (a) the plain form against oracle/tinygp_np.py at the bars of tests/test_gpu_0_kernels.py: 4 ulp in fp64 (rtol 1e-13 /
      atol 1e-14 with a sine in the program; rtol 1e-12 at d = 16, where NumPy sums pairwise and the device in order:
      test_kernel_matrix_ragged_shapes), Polynomial included; fp32 against the float64 oracle on the same points at FP32_BAR,
      four times the largest distance measured on these inputs and below 1e-5.
  (b) every other form against (a)'s DEVICE image of the same points, program and dtype: tolerance zero off the diagonal (the
      flags change placement, not arithmetic), one ulp of plain_ii + noise_i summed in long double on it.
  (c) DotProduct() on integer points with integer noise against the int64 product, tolerance zero in both dtypes: the
      lowering is [DOT(1, 0)], r3 / (1 * 1) + 0 * 0 with r3 a sum of integer products below 2^24 -- every step exact.

The solver's own assembly cannot be read before the factorisation overwrites it: tril(L L^T) is held to the oracle's
K + diag(noise) tile by tile at 16 times LAPACK's own residual.  tests/test_kmat_assembly_cpu.py shows that each of these
checks catches a misplaced tile, row of noise or padding entry, and that the inputs keep such an error far from every bar.
"""
import contextlib
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import _kmat_assembly as ka
from _schedules import trace_options
from tinygp_amd import _device, _ffi, kernels
from tinygp_amd.distributed import HipBlockOps

pytestmark = pytest.mark.gpu

FP32_BAR = 4 * 4.97e-7  # four times the largest |device - oracle| / |oracle| of the plain fp32 form on these inputs
SAME = {ka.VALUE: ("abs", 0), ka.VALUE_NOISE: ("ulp", 1)}   # (b)
EXACT = {ka.VALUE: ("abs", 0), ka.VALUE_NOISE: ("abs", 0)}  # (c)
DTYPES = [np.float64, np.float32]
TAIL = 256  # sentinels behind the buffer


def _program(name):
    return ka.PROGRAMS[name](kernels).program()


INT_PROGRAM = kernels.DotProduct().program()


def _call(form, prog, X, diag=None):
    """One tgp_kmat call in `form` on the points X (all of them: the form's x_off selects) into a sentinel-filled buffer:
    the (ld, cols_out) image [row, column] and the allocation's elements in front of and behind it."""
    ctx, lib = _ffi.default_ctx(), _ffi.lib()
    P = _device.points(X)
    dt, d = P.dtype, P.shape[1]
    assert form.x_off + max(form.n1, form.n2) <= P.shape[0]
    flat = ka.filled(form, dt, tail=TAIL)
    kp, nops = _ffi.as_kprog(prog)
    dev = [ctx.upload(flat), ctx.upload(P)]  # (upload = tgp_memcpy_h2d)
    try:
        d_diag = None
        if form.with_diag:
            dev.append(ctx.upload(np.ascontiguousarray(diag, dtype=dt)))
            d_diag = C.c_void_p(dev[2] + form.x_off * dt.itemsize)
        x = C.c_void_p(dev[1] + form.x_off * d * dt.itemsize)
        _ffi.check(lib.tgp_kmat(ctx.handle, _ffi.dtype_code(dt), kp, nops, form.n1, form.n2, d, x, x, d_diag,
                                C.c_void_p(dev[0] + form.out_off * dt.itemsize), form.ld, form.rows_out, form.cols_out,
                                int(form.lower)), "tgp_kmat")
        got = ctx.download(dev[0], flat.shape, dt)
    finally:
        for p in dev:
            ctx.free(p)
    return ka.image_of(got, form)


def _hold(form, prog, X, diag, K, bars, label):
    """The call's image against expected(form, K, diag) at `bars`, nothing written outside it."""
    got, outside = _call(form, prog, X, diag)
    want, mask = ka.expected(form, K, diag)
    ka.check(got, want, mask, bars, label=f"{label} {form}")
    assert ka.is_sentinel(outside).all(), f"{label} {form}: {int((~ka.is_sentinel(outside)).sum())} entries written outside the buffer"
    return got, want, mask


@functools.lru_cache(maxsize=64)
def _plain(name, n, d, dtype):
    """(a)'s device image [i, j] of the plain form, read-only."""
    got, outside = _call(ka.plain(n), _program(name), ka.points(n, d, dtype))
    assert ka.is_sentinel(outside).all() and not ka.is_sentinel(got).any()
    got = np.array(got)
    got.flags.writeable = False
    return got


def _oracle_bar(name, n, d, dtype):
    """The bar of (a) for one program, dimension and dtype."""
    if dtype == np.float32:
        return ("tol", FP32_BAR, 0)
    if name in ka.TRIGONOMETRIC:
        return ("tol", 1e-13, 1e-14)
    return ("tol", 1e-12, 0) if d >= 8 else ("ulp", 4)


def _hold_plain_and_solver_form(name, n, d, dtype):
    """(a) at (name, n, d, dtype), then assemble_lower's form of the same call against it."""
    K = ka.oracle_matrix(name, n, d)
    X, prog = ka.points(n, d, dtype), _program(name)
    label = f"{name} d={d} {np.dtype(dtype).name}"
    got = _plain(name, n, d, dtype)
    want, mask = ka.expected(ka.plain(n), K)
    print(f"\n[plain {label} n={n}] worst |device - oracle| / |oracle| = {ka.worst(got, want, mask):.3e}"
          f" = {float(ka.deviation(got, want).max()):.2f} ulp")
    ka.check(got, want, mask, {ka.VALUE: _oracle_bar(name, n, d, dtype)}, label=f"{label} plain against the oracle")
    _hold(ka.square_padded(n), prog, X, ka.noise(n, dtype), got, SAME, label)


def test_fp32_bar_stays_below_1e_5():
    assert FP32_BAR < 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(ka.PROGRAMS))
def test_every_program_at_every_size(name, dtype):
    for n in ka.SIZES:
        _hold_plain_and_solver_form(name, n, 1, dtype)


@pytest.mark.parametrize("name", [ka.FAST, ka.GENERAL])
def test_fifteen_tiles_in_the_triangular_grid(name):
    _hold_plain_and_solver_form(name, ka.LARGE, 1, np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", ka.DIM_SIZES)
@pytest.mark.parametrize("d", ka.DIMS)
def test_every_dimension(d, n, dtype):
    """d = 1, 2, 3: the straight-line kernel's forms (FAST); 4: the general kernel's last static form; 5, 16: its loop."""
    for name in (ka.FAST, ka.GENERAL):
        _hold_plain_and_solver_form(name, n, d, dtype)


FORMS = [(n, form) for n in ka.FORM_SIZES for form in ka.forms(n)]


@pytest.mark.parametrize("n,form", FORMS, ids=[str(form) for _, form in FORMS])
def test_every_form_leaves_the_plain_image(n, form):
    """with_diag alone, lower with and without noise, rows_out = cols_out in {n, the next multiple of 128, 128 more}, ld in
    {rows_out, + 1, + 2} (the odd one refuses the straight-line kernel) and out_off = 1 with an even ld (so does that): the
    bits of the plain form where the form writes, the sentinel everywhere else."""
    for name in (ka.FAST, ka.GENERAL):
        for dtype in DTYPES:
            _hold(form, _program(name), ka.points(n, 1, dtype), ka.noise(n, dtype), _plain(name, n, 1, dtype), SAME,
                  f"{name} {np.dtype(dtype).name}")


@pytest.mark.parametrize("n", ka.COLUMN_SIZES)
@pytest.mark.parametrize("nb", ka.COLUMN_WIDTHS)
def test_block_column_rectangle(nb, n):
    """assemble_columns' call (dist.hip) for every block column j0: n1 = n - j0, n2 = min(nb, n - j0), X, diag and out moved
    by j0 inside a buffer of npad rows."""
    for name in (ka.FAST, ka.GENERAL):
        for dtype in DTYPES:
            for j0 in range(0, n, nb):
                _hold(ka.block_column(n, nb, j0), _program(name), ka.points(n, 1, dtype), ka.noise(n, dtype),
                      _plain(name, n, 1, dtype), SAME, f"{name} {np.dtype(dtype).name} nb={nb} j0={j0}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_integer_family_is_exact(dtype):
    """(c): plain, assemble_lower's form with a tile of identity, and the block columns, against the int64 product."""
    lim = 2 ** 24 if dtype == np.float32 else 2 ** 53
    for n, d in ka.int_inputs():
        if n > max(ka.SIZES):  # (tgp_kdiag's size alone)
            continue
        X, diag = ka.int_points(n, d, dtype), ka.int_noise(n, dtype)
        K, bound = ka.int_matrix(X)
        assert bound < lim
        for form in (ka.plain(n), ka.square_padded(n, ka.round_up(n) + ka.TILE, 1), ka.square_padded(n, ka.round_up(n)),
                     ka.block_column(n, 128, n // 256 * 128)):
            _hold(form, INT_PROGRAM, X, diag, K, EXACT, f"DotProduct d={d} {np.dtype(dtype).name}")


# ---- the block-column driver itself ----------------------------------------------------------------------------------------

DRIVER = [(w, r, nb, n, name, np.float64) for w, r in ((1, 0), (3, 0), (3, 1), (3, 2)) for nb in ka.COLUMN_WIDTHS
          for n in (257, 640) for name in (ka.FAST, ka.GENERAL)] + [(3, 1, 128, 640, ka.FAST, np.float32)]


@pytest.mark.parametrize("world,rank,nb,n,name,dtype", DRIVER,
                         ids=[f"{r}of{w}-nb{nb}-n{n}-{name}-{np.dtype(t).name}" for w, r, nb, n, name, t in DRIVER])
def test_block_column_driver(world, rank, nb, n, name, dtype):
    """HipBlockOps.setup / assemble / first_panel / column for one rank, no process group: tgp_dist_assemble writes the first
    owned block column, tgp_dist_first_panel the others (it only assembles and records an event: no tgp_dist_begin is
    needed in front of it).  Each owned column: the lower tiles of the plain image plus noise, identity down to npad.  The
    driver's matrix is not sentinel-filled and `column` starts at j0, so the tiles above a column's diagonal tile are not
    part of this image; the matrix first holds the OTHER program's columns, which a tile left out would show."""
    other = ka.GENERAL if name == ka.FAST else ka.FAST
    P = _device.points(ka.points(n, 1, dtype))
    ops = HipBlockOps(0)
    try:
        ops.setup(P, ka.noise(n, dtype), nb, world, rank)
        npad = ka.round_up(n, nb)
        assert ops.npad == npad and ops.nloc == len(range(rank, npad // nb, world))
        for prog in (_program(other), _program(name)):
            ops.assemble(prog)
            ops.first_panel()
        for l in range(ops.nloc):
            j0 = (l * world + rank) * nb
            got = ops.column(l, npad - j0)
            f = ka.block_column(n, nb, j0)
            want, mask = ka.expected(dataclasses.replace(f, ld=f.rows_out, out_off=0), _plain(name, n, 1, dtype), ka.noise(n, dtype))
            ka.check(np.ascontiguousarray(got), want, mask, SAME, label=f"{name} local column {l} (j0 = {j0})", untouched=False)
    finally:
        ops.close()
        ops.ctx.close()


# ---- the solver handle -------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _options(**opts):
    ctx = _ffi.default_ctx()
    old = {}
    try:
        for key, value in opts.items():
            old[key] = ctx.set_option(key, value)
        yield
    finally:
        for key, value in old.items():
            ctx.set_option(key, value)


class _Solver:
    """A tgp_solver handle through the C ABI alone."""

    def __init__(self, X, diag):
        self.P = _device.points(X)
        self.dt, (self.n, self.d) = self.P.dtype, self.P.shape
        self.h = C.c_void_p()
        _ffi.check(_ffi.lib().tgp_solver_create(_ffi.default_ctx().handle, _ffi.dtype_code(self.dt), self.n, self.d,
                                                _ffi.ptr(self.P), _ffi.ptr(np.ascontiguousarray(diag, dtype=self.dt)),
                                                C.byref(self.h)), "tgp_solver_create")

    def factor(self, prog):
        kp, nops = _ffi.as_kprog(prog)
        info = C.c_int32(-1)
        _ffi.check(_ffi.lib().tgp_solver_factor(self.h, kp, nops, None, C.byref(info)), "tgp_solver_factor")
        assert info.value == 0
        L = np.empty((self.n, self.n), dtype=self.dt)
        _ffi.check(_ffi.lib().tgp_solver_get_factor(self.h, _ffi.ptr(L)), "tgp_solver_get_factor")
        return L

    def set_noise(self, diag):
        _ffi.check(_ffi.lib().tgp_solver_set_noise(self.h, _ffi.ptr(np.ascontiguousarray(diag, dtype=self.dt))),
                   "tgp_solver_set_noise")

    def covariance(self):
        out = np.empty((self.n, self.n), dtype=self.dt)
        _ffi.check(_ffi.lib().tgp_solver_covariance(self.h, _ffi.ptr(out)), "tgp_solver_covariance")
        return out

    def variance(self):
        out = np.empty(self.n, dtype=self.dt)
        _ffi.check(_ffi.lib().tgp_solver_variance(self.h, _ffi.ptr(out)), "tgp_solver_variance")
        return out

    def close(self):
        if self.h:
            _ffi.lib().tgp_solver_destroy(self.h)
            self.h = None


def _full(name, n, diag):
    """The oracle's K + diag(noise), float64."""
    K = np.array(ka.oracle_matrix(name, n))
    K[np.diag_indices(n)] += diag
    return K


def _residual(L, K):
    """max |tril(L L^T - K)| / max |K|"""
    L = np.tril(L)
    return float(np.abs(np.tril(L @ L.T - K)).max() / np.abs(K).max())


@functools.lru_cache(maxsize=None)
def _allowed():
    """16 times the largest residual max |L L^T - K| / max |K| of LAPACK's own factor over the cases below: the device's
    blocked order and its multiplications by inverses of the diagonal blocks add to LAPACK's rounding, not a tile's worth."""
    worst = 0.0
    for n in ka.SOLVER_SIZES:
        for name in ka.SOLVER_PROGRAMS:
            for diag in (ka.noise(n), ka.noise(n)[::-1]):
                K = _full(name, n, diag)
                worst = max(worst, _residual(sla.cholesky(K, lower=True), K))
    print(f"\n[two-range assembly] LAPACK's largest residual {worst:.3e}, allowed {16 * worst:.3e}")
    return 16 * worst


def _hold_product(L, name, n, diag, label):
    """tril(L L^T) against the oracle's K + diag(noise), tile by tile, at _allowed() of max |K|."""
    K = _full(name, n, diag)
    allowed = _allowed()
    assert allowed < 1e-9
    L = np.tril(L.astype(np.float64))
    got = np.tril(L @ L.T)
    print(f"\n[two-range assembly {label}] device residual {_residual(L, K):.3e}")
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    mask = np.where(i >= j, ka.VALUE, ka.UNTOUCHED).astype(np.int8)
    ka.check(got, K.astype(np.longdouble), mask, {ka.VALUE: ("abs", allowed * np.abs(K).max())}, label=label, untouched=False)


def _two_range(defer):
    """Options under which assemble_lower cuts the assembly in two: the first panel is nb_outer = 128 columns wide
    (first_panel_cols: nb_first = 0, and without the chain kernel no launch takes the whole matrix), lookahead = 1 keeps the
    assembly stream in use.  The cut depends on these options alone, so the dry run below, which takes them on a context
    of its own with the library's defaults for the rest, speaks for the default context that factors."""
    return dict(nb_outer=128, nb_first=0, lookahead=1, chain_kernel=0, asm_defer=defer)


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("n", ka.SOLVER_SIZES)
def test_two_range_assembly_of_the_solver(n, defer):
    """tgp_solver_factor twice on one handle, with two programs: the product of each factor is the oracle's matrix of THAT
    program -- a tile left from the first, or not assembled before the trailing update read it, is off by ~0.1.  That the
    two-range route is taken rests on tgp_trace_factor's two assembly records (tgp_solver_timings' ms[0] is positive on
    either route and shows nothing)."""
    opts = _two_range(defer)
    records = trace_options(ka.round_up(n), opts, 0)
    assert [r[0] for r in records].count(7) == 2, "the options do not cut the assembly in two"
    assert [r[0] for r in trace_options(ka.round_up(n), {}, 0)].count(7) == 1
    with _options(**opts):
        s = _Solver(ka.points(n), ka.noise(n))
        try:
            for name in ka.SOLVER_PROGRAMS:
                L = s.factor(_program(name))
                _hold_product(L, name, n, ka.noise(n), f"{name} n={n} asm_defer={defer}")
        finally:
            s.close()


def test_new_noise_reaches_the_next_factorisation():
    n, name = 257, ka.FAST
    with _options(**_two_range(0)):
        s = _Solver(ka.points(n), ka.noise(n))
        try:
            _hold_product(s.factor(_program(name)), name, n, ka.noise(n), "first noise")
            s.set_noise(ka.noise(n)[::-1])
            _hold_product(s.factor(_program(name)), name, n, ka.noise(n)[::-1], "second noise")
        finally:
            s.close()


@pytest.mark.parametrize("n", ka.COVARIANCE_SIZES)
def test_covariance_and_variance_of_the_solver(n):
    """tgp_solver_covariance: no padding flag, fused noise, ld = n (odd at 127 and 129: the general kernel alone; even at 128:
    the straight-line one) -- the plain image plus noise at the bars of (b).  The host array is row-major: the transpose of
    the device's column-major buffer.  tgp_solver_variance: its diagonal."""
    for name in (ka.FAST, ka.GENERAL):
        for dtype in DTYPES:
            diag = ka.noise(n, dtype)
            s = _Solver(ka.points(n, 1, dtype), diag)
            try:
                s.factor(_program(name))
                cov, var = s.covariance(), s.variance()
            finally:
                s.close()
            want, mask = ka.expected(ka.Form(n, n, with_diag=True), _plain(name, n, 1, dtype), diag)
            label = f"{name} {np.dtype(dtype).name} n={n}"
            ka.check(np.ascontiguousarray(cov.T), want, mask, SAME, label=f"{label} covariance")
            k = np.arange(n)
            ka.check(var[:, None], want[k, k][:, None], mask[k, k][:, None], SAME, label=f"{label} variance")


@pytest.mark.parametrize("n", ka.KDIAG_SIZES)
def test_kdiag_is_the_diagonal_of_the_plain_image(n):
    for name in ka.KDIAG_PROGRAMS:
        for dtype in DTYPES:
            got = _device.kdiag(_program(name), ka.points(n, 1, dtype))
            want = np.diag(_plain(name, n, 1, dtype)).astype(np.longdouble)
            ka.check(got[:, None], want[:, None], np.full((n, 1), ka.VALUE, dtype=np.int8), SAME,
                     label=f"{name} {np.dtype(dtype).name} kdiag")
    for dtype in DTYPES:
        X = ka.int_points(n, 1, dtype)
        got = _device.kdiag(INT_PROGRAM, X)
        want = np.diag(ka.int_matrix(X)[0]).astype(np.longdouble)
        ka.check(got[:, None], want[:, None], np.full((n, 1), ka.VALUE, dtype=np.int8), EXACT, label="DotProduct kdiag")
