"""NumPy front-ends to the device-pointer C ABI, for the GPU parity tests only."""
import ctypes as C

import numpy as np

from tinygp_amd import _ffi


def _f(a, dt):
    return np.asfortranarray(a, dtype=dt)


def potrf(A, nb_outer=None, lookahead=None, **options):
    """In-place lower Cholesky of a symmetric (n,n) host matrix, n % 128 == 0. Returns (L, info).
    Further context options (fused_step, gate_split, chain_reserve, ...) by keyword."""
    ctx = _ffi.default_ctx()
    dt = A.dtype
    n = A.shape[0]
    old = {}
    if nb_outer is not None:
        old["nb_outer"] = ctx.set_option("nb_outer", nb_outer)
    if lookahead is not None:
        old["lookahead"] = ctx.set_option("lookahead", lookahead)
    for k, v in options.items():
        old[k] = ctx.set_option(k, v)
    dA = ctx.upload(_f(A, dt).ravel(order="K"))
    info = C.c_int32()
    try:
        _ffi.check(_ffi.lib().tgp_potrf(ctx.handle, _ffi.dtype_code(dt), n, C.c_void_p(dA), n,
                                        C.byref(info)), "tgp_potrf")
        out = ctx.download(dA, (n, n), dt).T  # column-major buffer read row-major = transpose
    finally:
        ctx.free(dA)
        for k, v in old.items():
            ctx.set_option(k, v)
    return np.tril(out), info.value


def trsv(L, y, transpose=False):
    ctx = _ffi.default_ctx()
    dt = L.dtype
    n = L.shape[0]
    dL = ctx.upload(_f(L, dt).ravel(order="K"))
    dy = ctx.upload(np.ascontiguousarray(y, dtype=dt))
    try:
        _ffi.check(_ffi.lib().tgp_trsv(ctx.handle, _ffi.dtype_code(dt), n, C.c_void_p(dL), n,
                                       int(transpose), C.c_void_p(dy)), "tgp_trsv")
        return ctx.download(dy, (n,), dt)
    finally:
        ctx.free(dL), ctx.free(dy)


def trsm_right_lt(L, B, **options):
    """B (m, n) -> B L^-T.  Context options (nb_outer, lookahead, ...) by keyword: set for the call, restored behind it."""
    ctx = _ffi.default_ctx()
    dt = L.dtype
    n = L.shape[0]
    m = B.shape[0]
    old = {}
    for k, v in options.items():
        old[k] = ctx.set_option(k, v)
    dL = ctx.upload(_f(L, dt).ravel(order="K"))
    dB = ctx.upload(_f(B, dt).ravel(order="K"))
    try:
        _ffi.check(_ffi.lib().tgp_trsm_right_lt(ctx.handle, _ffi.dtype_code(dt), m, n,
                                                C.c_void_p(dL), n, C.c_void_p(dB), m),
                   "tgp_trsm_right_lt")
        return ctx.download(dB, (n, m), dt).T
    finally:
        ctx.free(dL), ctx.free(dB)
        for k, v in old.items():
            ctx.set_option(k, v)


def gemm_nt(A, B, Cm, alpha, beta, lower=False):
    """C <- beta C + alpha A B^T; returns the full C (entries outside `lower` tiles untouched)."""
    ctx = _ffi.default_ctx()
    dt = A.dtype
    m, k = A.shape
    n = B.shape[0]
    dA = ctx.upload(_f(A, dt).ravel(order="K"))
    dB = ctx.upload(_f(B, dt).ravel(order="K"))
    dC = ctx.upload(_f(Cm, dt).ravel(order="K"))
    try:
        _ffi.check(_ffi.lib().tgp_gemm_nt(ctx.handle, _ffi.dtype_code(dt), m, n, k, float(alpha),
                                          C.c_void_p(dA), m, C.c_void_p(dB), n, float(beta),
                                          C.c_void_p(dC), m, int(lower)), "tgp_gemm_nt")
        return ctx.download(dC, (n, m), dt).T
    finally:
        ctx.free(dA), ctx.free(dB), ctx.free(dC)


def gemm_nt_ld(A, B, C0, m, n, k, mode, lower, options=None, repeat=1, read=()):
    """tgp_gemm_nt on column-major buffers with their own leading dimensions: A (lda, k), B (ldb, k), C0 (ldc, n), of which the
    call uses the first m / n / m rows.  mode 0: C -= A B^T, 1: C = A B^T.  `options` hold for the call and are restored.
    The call is made `repeat` times, each on a fresh upload of C0; returns one (C, values, error) per call: the WHOLE (ldc, n)
    buffer, padding rows included, the context options named in `read` behind the call, and the ValueError of a rejected
    argument (None otherwise)."""
    ctx = _ffi.default_ctx()
    dt = C0.dtype
    lda, ldb, ldc = A.shape[0], B.shape[0], C0.shape[0]
    assert A.shape[1] == k and B.shape[1] == k and C0.shape[1] == n and lda >= m and ldb >= n and ldc >= m
    alpha, beta = ((-1.0, 1.0), (1.0, 0.0))[mode]
    flat = _f(C0, dt).ravel(order="K")
    old, dev, out = {}, [], []
    try:
        for key, v in (options or {}).items():
            old[key] = ctx.set_option(key, v)
        dev.append(ctx.upload(_f(A, dt).ravel(order="K")))
        dev.append(ctx.upload(_f(B, dt).ravel(order="K")))
        dev.append(ctx.upload(flat))
        dA, dB, dC = dev
        for rep in range(repeat):
            if rep:
                _ffi.check(_ffi.lib().tgp_memcpy_h2d(ctx.handle, C.c_void_p(dC), flat.ctypes.data_as(C.c_void_p), flat.nbytes),
                           "tgp_memcpy_h2d")
            err = None
            try:
                _ffi.check(_ffi.lib().tgp_gemm_nt(ctx.handle, _ffi.dtype_code(dt), m, n, k, alpha, C.c_void_p(dA), lda,
                                                  C.c_void_p(dB), ldb, beta, C.c_void_p(dC), ldc, int(lower)), "tgp_gemm_nt")
            except ValueError as e:
                err = e
            got = ctx.download(dC, (n, ldc), dt).T
            out.append((got, {key: ctx.get_option(key) for key in read}, err))
    finally:
        for p in dev:
            ctx.free(p)
        for key, v in old.items():
            ctx.set_option(key, v)
    return out


def ubench(dtype):
    ctx = _ffi.default_ctx()
    out = C.c_double()
    _ffi.check(_ffi.lib().tgp_ubench_mfma(ctx.handle, _ffi.dtype_code(dtype), C.byref(out)),
               "tgp_ubench_mfma")
    return out.value
