"""Exact references for the MFMA product kernels (gemm.hip): cases, inputs and the check, in NumPy alone.

A, B and C0 hold small integers, so every partial sum of C0 -+ A B^T is an integer below 2^24 (fp32) or 2^53 (fp64): whatever
the order of summation, fused or not, split along k or not, the kernel must return the int64 product bit for bit.  A dropped,
doubled or mis-sliced k-tile, a tile mapped twice or not at all, a stage read before it landed, a wrong sign and a store outside
the tile all change bits.  (The one thing an int64 reference does not say is the sign of a zero: updated entries are compared as
numbers, everything that must come back untouched as bit patterns.)

No GPU and no library here: tests/test_gemm_exact_cpu.py checks the case lists and the check itself on the CPU,
tests/test_gpu_0_gemm_exact.py runs them on the device.
"""
import zlib
from collections import namedtuple

import numpy as np

BM = 128  # tile of gemm_nt_kernel
SM = 64   # tile of gemm_nt_small_kernel
BK = 16
AMAX, CMAX = 15, 1000
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
LIMIT = {"f64": 2 ** 53, "f32": 2 ** 24}
DTYPES = {"f64": np.float64, "f32": np.float32}
# the padding's quiet NaN, with a payload that no arithmetic produces
NAN_BITS = {"f64": np.uint64(0x7FF8_0000_DEAD_BEEF), "f32": np.uint32(0x7FC0_BEEF)}

# tm = None: the smallest tm whose lower triangle has more tiles than the chip has workgroup slots (resolve())
# reserve: gemm_reserve = 2 cus - 8 (a grid of 8 workgroups);  prefix: gemm_prefix_cols
Case = namedtuple("Case", "dtype role tm tn k lower mode padded band split reserve prefix")


def case(dtype, role, tm, tn, k, lower, mode=0, padded=False, band=8, split=0, reserve=False, prefix=0):
    return Case(dtype, role, tm, tn, k, int(lower), mode, padded, band, split, reserve, prefix)


def case_id(c):
    tm, tn = ("N", "N") if c.tm is None else (c.tm, c.tn)
    s = f"{c.dtype}-role{c.role}-{tm}x{tn}{'L' if c.lower else 'F'}-k{c.k}-mode{c.mode}-band{c.band}"
    for flag, text in ((c.padded, "-ld"), (c.split, "-split"), (c.reserve, "-reserve"), (c.prefix, f"-prefix{c.prefix}")):
        if flag:
            s += text
    return s


# ---- the launcher's host logic, restated -----------------------------------------------------------------------------------

def tile_count(tm, tn, lower):
    if not lower:
        return tm * tn
    c = min(tn, tm)
    return c * tm - c * (c - 1) // 2


def split_factor(nblk, k, cus):
    """launch_gemm_nt's split-tail rule: workgroups per tile of the last, partly filled round."""
    slots = 2 * cus
    R = nblk % slots
    nkt = k // BK
    S = 1
    while R > 0 and 2 * S * R <= slots and 2 * S <= 8 and nkt % (2 * S) == 0 and nkt // (2 * S) >= 8:
        S *= 2
    return S


def persistent_grid(nblk, reserve, cus):
    if reserve <= 0:
        return nblk
    slots = (2 * cus - reserve) // 8 * 8
    slots = max(slots, 8)
    return min(nblk, slots)


def resolve(c, cus):
    """The case with its chip-dependent shape filled in."""
    if c.tm is not None:
        return c
    tm = 1
    while tile_count(tm, tm, 1) <= 2 * cus:
        tm += 1
    return c._replace(tm=tm, tn=tm)


def options(c, cus):
    """Context options that hold for the call."""
    o = dict(gemm_role=c.role, tile_band=c.band, split_tail=c.split, gemm_reserve=0, gemm_prefix_cols=0)
    if c.reserve:
        o["gemm_reserve"] = 2 * cus - 8
    if c.prefix:
        o["gemm_prefix_cols"] = c.prefix
    return o


def tile_of(c):
    """Tile size the launcher picks for the case: the 64 x 64 kernel for roles 1 / 3 up to k = 256 and for roles 4 / 5."""
    return SM if (c.role in (1, 3) and c.k <= 256) or c.role in (4, 5) else BM


def skip00(c):
    return c.role in (3, 5)


def nblk_of(c):
    return tile_count(c.tm, c.tn, c.lower)


# ---- the case lists ----------------------------------------------------------------------------------------------------------

SHAPES_1 = [(1, 1, 0, False), (2, 3, 0, True), (3, 3, 1, True), (5, 2, 1, False), (2, 5, 1, False)]  # (tm, tn, lower, padded)
K_EDGES = {"f64": (16, 32, 112, 128, 144, 272), "f32": (16, 32, 48, 64, 80, 112)}


def group1():
    out = []
    for dt in ("f64", "f32"):
        for k in K_EDGES[dt]:
            for mode in (0, 1):
                for tm, tn, lower, padded in SHAPES_1:
                    out.append(case(dt, 0, tm, tn, k, lower, mode, padded))
        out.append(case(dt, 1, 3, 3, 272, 1, 0, True))  # the same kernel as ROLE 1
    return out


def group2():
    out = []
    for dt in ("f64", "f32"):
        for tm, tn, lower in ((1, 1, 1), (2, 2, 1), (4, 4, 1), (11, 11, 1), (3, 3, 0)):
            for band in (0, 3, 8):
                for k in (16, 144):
                    out.append(case(dt, 0, tm, tn, k, lower, 0, False, band))
    return out


K_SPLIT = (256, 384, 512, 768, 1024)


def group3():
    out = []
    for tm in (1, 2):
        for k in K_SPLIT + (272,):
            out.append(case("f64", 0, tm, tm, k, 1, split=1))
    out.append(case("f64", 0, 14, 14, 1024, 1, split=1))    # R = 105 tiles: 2 S R <= slots stops at S = 4 on 256 CUs
    out.append(case("f64", 0, None, None, 256, 1, split=1))  # more tiles than slots: a full round, then a split tail
    return out


def group4():
    out = []
    for dt in ("f64", "f32"):
        for tm in (1, 3, 4, 6):
            for k in (16, 128, 144):
                for mode in (0, 1):
                    for band in (0, 8):
                        out.append(case(dt, 0, tm, tm, k, 1, mode, False, band, reserve=True))
    return out


def group5():
    out = []
    for dt in ("f64", "f32"):
        for cols in (128, 256):
            for tm in (2, 3, 9):
                if cols >= tm * BM:
                    continue
                for k in (128, 144):
                    for reserve in (False, True):
                        for band in (0, 8):
                            out.append(case(dt, 0, tm, tm, k, 1, 0, False, band, reserve=reserve, prefix=cols))
    return out


def group5_rejected():
    return [case(dt, 0, 3, 3, 112, 1, prefix=128) for dt in ("f64", "f32")]


SHAPES_6 = [(2, 3, 0), (3, 3, 1), (5, 2, 1), (2, 5, 1)]


def group6():
    out = []
    for dt in ("f64", "f32"):
        for role, k in ((1, 16), (1, 32), (1, 48), (1, 64), (1, 256), (4, 512)):
            for tm, tn, lower in SHAPES_6:
                for mode in (0, 1):
                    for band in (0, 8):
                        out.append(case(dt, role, tm, tn, k, lower, mode, False, band))
        for role, k in ((5, 512), (3, 128)):  # without the first 128 x 128 diagonal block
            for tm, tn in ((3, 3), (5, 2)):
                for band in (0, 8):
                    out.append(case(dt, role, tm, tn, k, 1, 0, False, band))
    return out


def group7():
    """One shape per form, real-valued operands."""
    out = []
    for dt in ("f64", "f32"):
        out.append(case(dt, 0, 2, 3, 272 if dt == "f64" else 112, 0, 0, True))         # group 1
        if dt == "f64":
            out.append(case(dt, 0, 2, 2, 512, 1, split=1))                               # group 3
        out.append(case(dt, 0, 4, 4, 144, 1, reserve=True))                              # group 4
        out.append(case(dt, 0, 3, 3, 144, 1, reserve=True, prefix=128))                  # group 5
        out.append(case(dt, 1, 3, 3, 256, 1))                                            # group 6
        out.append(case(dt, 4, 2, 3, 512, 0, 1))
    return out


def integer_cases():
    return group1() + group2() + group3() + group4() + group5() + group5_rejected() + group6()


# ---- inputs ------------------------------------------------------------------------------------------------------------------

Inputs = namedtuple("Inputs", "A B C0 ref m n k lda ldb ldc prod bound")  # prod: integer cases, bound: real-valued ones


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _padded(body, ld, nan):
    """(rows, cols) values -> column-major (ld, cols) buffer whose rows past `rows` hold the NaN payload."""
    buf = np.empty((ld, body.shape[1]), dtype=body.dtype, order="F")
    _bits(buf)[...] = nan
    buf[:body.shape[0]] = body
    return buf


def _dims(c):
    m, n = c.tm * BM, c.tn * BM
    if c.padded:
        return m, n, m + 128, n + 256, m + 384
    return m, n, m, n, m


def _finish(c, A, B, C0, ref, prod, bound):
    dt, nan = DTYPES[c.dtype], NAN_BITS[c.dtype]
    m, n, lda, ldb, ldc = _dims(c)
    C0 = C0.astype(dt)
    if c.mode == 1:  # C = A B^T must not read C
        C0 = np.empty_like(C0)
        _bits(C0)[...] = nan
    return Inputs(_padded(A.astype(dt), lda, nan), _padded(B.astype(dt), ldb, nan), _padded(C0, ldc, nan), ref, m, n, c.k,
                  lda, ldb, ldc, prod, bound)


def make_inputs(c):
    """Integer operands, seeded by the case; ref = C0 -+ A B^T as int64.

    The product goes through the float64 BLAS and is then cast: it is the int64 product exactly, for the reason the kernels must
    be (every partial sum is an integer below 2^53; magnitude_ok() asserts the bound) -- test_gemm_exact_cpu.py holds it to
    NumPy's own int64 matmul on the small cases.  int64 matmul itself has no BLAS and takes seconds on the largest case."""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    m, n = c.tm * BM, c.tn * BM
    A = rng.integers(-AMAX, AMAX + 1, size=(m, c.k))
    B = rng.integers(-AMAX, AMAX + 1, size=(n, c.k))
    C0 = rng.integers(-CMAX, CMAX + 1, size=(n, m)).T  # (column-major like the device buffers: the check runs along memory)
    prod = (B.astype(np.float64) @ A.astype(np.float64).T).astype(np.int64).T
    ref = prod if c.mode == 1 else C0 - prod
    return _finish(c, A, B, C0, ref, prod, None)


def magnitude_ok(c, inp):
    """The condition that makes every summation order exact, on the reference alone."""
    c0 = 0 if c.mode == 1 else int(np.max(np.abs(inp.C0[:inp.m].astype(np.int64))))
    return c0 + c.k * AMAX * AMAX < LIMIT[c.dtype] and int(np.max(np.abs(inp.ref))) < LIMIT[c.dtype]


def make_real_inputs(c):
    """A, B, C0 ~ N(0, 1) in the case's dtype; ref in float64 (fp32 cases) or long double (fp64), and the elementwise bound
    (k + 2) u (|A| |B|^T + |C0|): the standard bound of an inner product in any order, with or without FMA."""
    rng = np.random.default_rng(zlib.crc32(("real-" + case_id(c)).encode()))
    dt = DTYPES[c.dtype]
    hi = np.float64 if c.dtype == "f32" else np.longdouble
    m, n = c.tm * BM, c.tn * BM
    A = rng.normal(size=(m, c.k)).astype(dt)
    B = rng.normal(size=(n, c.k)).astype(dt)
    C0 = rng.normal(size=(n, m)).astype(dt).T
    prod = (B.astype(hi) @ A.astype(hi).T).T
    ref = prod if c.mode == 1 else C0.astype(hi) - prod
    bound = (np.abs(B).astype(np.float64) @ np.abs(A).astype(np.float64).T).T
    if c.mode == 0:
        bound = bound + np.abs(C0).astype(np.float64)
    bound *= (c.k + 2) * U[c.dtype]
    return _finish(c, A, B, C0, ref, None, bound)


# ---- the check ---------------------------------------------------------------------------------------------------------------

def regions(c, inp):
    """(must, may, keep) masks over the m x n matrix: entries that must equal the reference, entries that are either updated or
    untouched (above the diagonal inside a diagonal tile), entries that must come back as C0."""
    i = np.arange(inp.m)[None, :]  # built as (n, m) and transposed: column-major, like the buffers
    j = np.arange(inp.n)[:, None]
    must, may, keep = _regions_t(c, inp, i, j)
    return must.T, may.T, keep.T


def _regions_t(c, inp, i, j):
    if c.lower:
        t = tile_of(c)
        must = i >= j                # (columns past m hold no such entry: with n > m they are untouched)
        keep = (i // t) < (j // t)
        may = ~must & ~keep
    else:
        must = np.ones((inp.n, inp.m), dtype=bool)
        keep = np.zeros_like(must)
        may = keep.copy()
    if skip00(c):
        block = (i < BM) & (j < BM)
        must = must & ~block
        may = may & ~block
        keep = keep | block
    return must, may, keep


def exact_result(c, inp):
    """The buffer a correct kernel returns (whole diagonal tiles updated, as the kernels do)."""
    must, may, _ = regions(c, inp)
    out = inp.C0.copy(order="F")
    body = out[:inp.m]
    upd = must | may
    body[upd] = inp.ref[upd].astype(out.dtype)
    return out


def _report(c, inp, got, bad, why):
    """Name the first wrong 128 x 128 tile (column by column) and what its residual looks like."""
    tj, ti = np.argwhere(bad.reshape(inp.m // BM, BM, inp.n // BM, BM).any(axis=(1, 3)).T)[0]
    sl = (slice(ti * BM, (ti + 1) * BM), slice(tj * BM, (tj + 1) * BM))
    nbad = int(bad[sl].sum())
    tiles = int(bad.reshape(inp.m // BM, BM, inp.n // BM, BM).any(axis=(1, 3)).sum())
    g = got[:inp.m][sl].astype(np.float64)
    res = g - inp.ref[sl].astype(np.float64)
    hint = ""
    if inp.prod is not None:
        p = inp.prod[sl].astype(np.float64)
        if np.isnan(g).any():
            hint = f", {int(np.isnan(g).sum())} NaN"
        elif np.array_equal(res, p) and c.mode == 0:
            hint = ", the tile came back as C0 (not updated)"
        elif np.array_equal(res, -p):
            hint = ", residual = -(A B^T) of the tile (updated twice)" if c.mode == 0 else ", the tile came back as zero"
        else:
            fin = res[np.isfinite(res)]
            hint = f", residual in [{fin.min():.0f}, {fin.max():.0f}]" if fin.size else ""
    return (f"{case_id(c)}: {why}: first wrong 128x128 tile (ti, tj) = ({ti}, {tj}) with {nbad} of {BM * BM} entries wrong"
            f"{hint}; {tiles} tile(s) wrong in all")


def _check(c, inp, got, close):
    assert got.shape == (inp.ldc, inp.n) and got.dtype == inp.C0.dtype, (got.shape, got.dtype)
    body, c0 = got[:inp.m], inp.C0[:inp.m]
    must, may, keep = regions(c, inp)
    same = _bits(body) == _bits(c0)
    bad_keep = keep & ~same
    assert not bad_keep.any(), _report(c, inp, got, bad_keep, "an entry outside the update changed")
    bad = (must & ~close) | (may & ~(close | same))
    assert not bad.any(), _report(c, inp, got, bad, "the update differs from the reference")
    if inp.ldc > inp.m:
        pad = _bits(got[inp.m:]) != NAN_BITS[c.dtype]
        assert not pad.any(), (f"{case_id(c)}: {int(pad.sum())} padding entries of C overwritten, the first at row "
                               f"{inp.m + int(np.argwhere(pad)[0][0])}, column {int(np.argwhere(pad)[0][1])}")


def check_exact(c, inp, got):
    """got: the whole (ldc, n) buffer after the call.  Raises AssertionError with the first wrong tile."""
    with np.errstate(invalid="ignore"):
        close = got[:inp.m] == inp.ref.astype(got.dtype)  # (exact: |ref| < 2^24 / 2^53; NaN equals nothing)
    _check(c, inp, got, close)


def check_real(c, inp, got):
    """Real-valued operands: |got - ref| <= (k + 2) u (|A| |B|^T + |C0|) elementwise."""
    with np.errstate(invalid="ignore"):
        err = np.abs(got[:inp.m].astype(inp.ref.dtype) - inp.ref).astype(np.float64)
        close = err <= inp.bound
    _check(c, inp, got, close)
    must, _, _ = regions(c, inp)
    return float(np.max(err[must] / inp.bound[must]))  # worst entry, in units of its bound
