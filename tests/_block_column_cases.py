"""The resident solves of the block-column driver (``tinygp_amd/distributed.py``, ``csrc/dist.hip``) at every block
edge: the cases, the drive that runs them against ONE factorisation, and the checks -- shared by
``test_block_column_resident_cpu.py`` (NumPy stand-in under gloo), ``test_gpu_5_resident_edges.py`` (world size 1, RCCL
self-collectives) and ``test_gpu_6_resident_edges_one_gpu.py`` (two and three ranks on one GPU, gloo).

Inputs and references are those of ``_dense_np.py`` (the box that does not grow with N: every 128 x 128 tile of the
factor and of the cross covariance carries weight, asserted there on the float64 reference alone) and, for the gradient,
of ``_dense_grad_np.py`` (analytic dK/dtheta, LAPACK's K^-1, every tile of K^-1 weighted).  Nothing here is measured on
the code under test: the bars are the project's,

* solves, ``alpha``, colsum(A o A) and A^T A: ``_dense_np.solve_bar`` on the quantity's own scale (fp64: rtol 1e-10 and
  1e-10 max|want|; fp32: 2e-3 max|want|);
* ``L Z``: long double product of the driver's OWN factor (gathered from the owners' block columns) with
  ``_dense_np.dot_bar``, the componentwise gamma_N bound;
* conditional covariance and variance through ``_dense_np.conditional`` and the posterior mean: ``posterior_bar``;
* log-likelihoods: the ``ll`` bar of ``_dense_grad_np.BARS``; the gradient: ``_dense_grad_np.check``;
* form against form -- left-looking against right-looking forward solve, chunked against unchunked test points -- under
  the solve bar on the reference's scale; every rank against rank 0 to the bit.

Pairs that are bit-identical on the device are asserted EQUAL there (``on_device=True``), not merely close:

* colsum(A o A) in chunks of 128 test points against one pass, under both forms of the forward solve, at world sizes 1
  and 2: a right-hand side's column never meets another's in the solves, and how many columns ride along changes no
  order of summation (the split-k tail of the left-looking product combines its slices in slice order);
* A^T A in chunks against one pass likewise, in block columns of up to 256.

Observed on an MI355X and NOT asserted equal, only held to the bar: A^T A in block columns of 512 (the k = 512 product of a
128-wide and of a 384-wide operand differ in their last bits, 1e-15 of the largest entry); anything at world
size 3 (gloo sums three addends in an order that depends on the message's length; two addends commute); the
left-looking against the right-looking forward solve from three blocks on (different orders of the same sums).  On the
stand-in nothing is asserted equal: the host BLAS picks its blocking by the operand's width.
"""
import functools
import math

import numpy as np
import scipy.linalg as sla

import _dense_grad_np as dg
import _dense_np as dn
from oracle import tinygp_np as o

F64, F32 = "float64", "float32"
D = 1  # input dimension of every case (the 1-D kernel of _dense_np: 1.3 ExpSquared(1.5))
WORLDS = (1, 2, 3)
# (N, nb): one ragged block | exactly one | a last block of ONE row | three blocks twice | nine, five and three blocks
SHAPES = ((100, 128), (128, 128), (129, 128), (257, 128), (300, 128), (1100, 128), (1100, 256), (1100, 512))
CASES = tuple((n, nb, F64) for n, nb in SHAPES) + ((300, 128, F32),)
R_WIDTHS = (1, 2, 127, 128, 129, 257)  # right-hand sides of solve_triangular (padded to 128, 256, 384 columns)
VAR_MS = (1, 128, 129, 257)            # test points of condition_colsumsq
GRAM_MS = (1, 128, 129, 300)           # test points of condition_gram
MEAN_M = 129
CHUNK = 128                            # RHS_CHUNK / GRAM_CHUNK of the chunked runs
FORMS = ("right", "left")
# (program of _dense_grad_np, N, nb, GRAD_CHUNK): chunks of 128 in blocks of 256 start mid-block (first = 0, 0, 1, 1, ..);
# chunks of 512 in blocks of 128 start at blocks 0, 4 and 8 (the last: the ragged block alone)
GRAD_CASES = (("ess", 300, 256, 128), ("ess", 1100, 256, 128), ("ess", 1100, 128, 512))
# ranks WITHOUT a block column: N = 100 and 128 at world 2 and 3 (one block), N = 129 at world 3 (two blocks), the
# gradient's N = 300 in blocks of 256 at world 3


def identical_on_device(what, nb, world):
    """Whether chunked test points and one pass give the same bits on the device (see the docstring)."""
    return world <= 2 and (what == "var" or nb <= 256)


def case_id(c):
    return "-".join(map(str, c))


def nblocks(n, nb):
    return -(-n // nb)


def resid(n, dtype=F64):
    """The right-hand side the factorisation carries along."""
    X = np.asarray(dn.train(n, D, dtype)[0], dtype=np.float64)
    return (np.sin(2.0 * X) + 0.3 * X).astype(dtype)


def other_resid(n, dtype=F64):
    """A right-hand side other than the factored one (alpha, resident_log_probability, condition_mean)."""
    return np.ascontiguousarray(dn.rhs(n, dtype)[:, 5])


def third_resid(n, dtype=F64):
    """One more (resident_log_probability: its own forward solve, not the one alpha() left behind)."""
    return np.ascontiguousarray(dn.rhs(n, dtype)[:, 6])


# ---- the drive: every resident quantity against ONE factorisation ------------------------------------------------
def drive(make, n, nb, dtype):
    """``make(kernel, X, diag, nb) -> BlockCyclicCholesky``; returns {name: array} (replicated results, this rank's
    block columns of the factor as ``col/<j>``, and ``panels`` = panel chunks factored [by the first pass, in all])."""
    from tinygp_amd import kernels

    X, diag = dn.train(n, D, dtype)
    s = make(dn.kernel(kernels, D), X, diag, nb)
    calls = {"panel": 0}
    real = s.ops.panel_chunk

    def counting(k, c, nch):
        calls["panel"] += 1
        real(k, c, nch)

    s.ops.panel_chunk = counting
    out = {}
    try:
        out["ll"] = np.float64(s.log_probability(resid(n, dtype)))
        out["info"] = np.int64(s.info)
        factored = calls["panel"]
        Y = dn.rhs(n, dtype)
        vec = np.ascontiguousarray(Y[:, 0])
        out["fwd/vec"] = s.solve_triangular(vec)
        out["bwd/vec"] = s.solve_triangular(vec, transpose=True)
        for r in R_WIDTHS:
            Yr = np.ascontiguousarray(Y[:, :r])
            out[f"bwd/{r}"] = s.solve_triangular(Yr, transpose=True)
            for form in FORMS:
                s.FORWARD = form
                out[f"fwd/{form}/{r}"] = s.solve_triangular(Yr)
        s.FORWARD = "auto"
        out["dot/vec"] = s.dot_triangular(vec)
        out["dot/3"] = s.dot_triangular(np.ascontiguousarray(Y[:, :3]))
        default = (s.RHS_CHUNK, s.GRAM_CHUNK)
        for form in FORMS:
            s.FORWARD = form
            for tag, chunk in (("one", default), ("chunked", (CHUNK, CHUNK))):
                s.RHS_CHUNK, s.GRAM_CHUNK = chunk
                for m in VAR_MS:
                    out[f"var/{form}/{tag}/{m}"] = s.condition_colsumsq(dn.query_points(m, D, dtype)[0])
                for m in GRAM_MS:
                    out[f"gram/{form}/{tag}/{m}"] = s.condition_gram(dn.query_points(m, D, dtype)[0])
        s.FORWARD = "auto"  # (right-looking alone, left-looking with peers)
        for tag, chunk in (("one", default), ("chunked", (CHUNK, CHUNK))):
            s.RHS_CHUNK, s.GRAM_CHUNK = chunk
            for m in GRAM_MS:
                out[f"gram_other/{tag}/{m}"] = s.condition_gram(dn.query_points(m, D, dtype)[0],
                                                                kernel=dn.other_kernel(kernels, D))
        s.RHS_CHUNK, s.GRAM_CHUNK = default
        r2 = other_resid(n, dtype)
        out["rll"] = np.float64(s.resident_log_probability(third_resid(n, dtype)))
        out["alpha"] = np.array(s.ops.rhs_to_host(s.alpha(r2))[:n])
        out["mean"] = s.condition_mean(r2, dn.query_points(MEAN_M, D, dtype)[0])
        for l, j in enumerate(s.owned):
            out[f"col/{j}"] = np.array(s.ops.column(l, s.rows(j)))
        out["panels"] = np.array([factored, calls["panel"]])
    finally:
        s.close(close_ops=True)
    return out


def drive_grad(make, name, n, nb, chunk):
    from tinygp_amd import kernels

    X, diag, y = dg.inputs(n, dg.PROGRAMS[name][0])
    kern = dg.kernel(name, kernels)
    s = make(kern, X, diag, nb)
    try:
        s.GRAD_CHUNK = chunk
        ll, g = s.log_probability_and_grad(y)
        flat = np.array(g["kernel"])  # 2 per op of the postfix program; a leaf's parameters are its p0, p1
        slots: list = []
        kern._slots(slots)
        assert len(flat) == 2 * len(slots)
        got = np.array([flat[2 * i + q] for i, pair in enumerate(slots) for q in (0, 1) if pair[q] is not None])
        return {"ll": np.float64(ll), "info": np.int64(s.info), "kernel": got, "noise": np.array(g["noise_diag"]),
                "mean": np.array(g["mean"])}
    finally:
        s.close(close_ops=True)


def run_all(make):
    """Every case through ``make`` on this rank: {case: results}."""
    out = {c: drive(make, *c) for c in CASES}
    out.update({c: drive_grad(make, *c) for c in GRAD_CASES})
    return out


# ---- references (float64, cached, read-only) --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_refs(n, dtype):
    ref = dn.reference(n, D, dtype)
    Y = dn.rhs(n, dtype)[:, :max(R_WIDTHS)]
    return dn._frozen(dn.solve_reference(ref.L, Y, False)), dn._frozen(dn.solve_reference(ref.L, Y, True))


@functools.lru_cache(maxsize=None)
def cross_refs(n, dtype, m, other):
    """``(colsum(A o A), A^T A, Kss)`` with ``A = L^-1 K(X, X*)``; the cross covariance's condition asserted."""
    ref = dn.reference(n, D, dtype)
    kern = (dn.other_kernel if other else dn.kernel)(o, D)
    Xt = dn.query_points(m, D, dtype)[0].astype(np.float64)
    Ks = kern(ref.X, Xt)
    dn.check_cross(Ks)
    A = sla.solve_triangular(ref.L, Ks, lower=True, check_finite=False)
    return dn._frozen(np.sum(A * A, axis=0)), dn._frozen(A.T @ A), dn._frozen(kern(Xt, Xt))


@functools.lru_cache(maxsize=None)
def vector_refs(n, dtype):
    """``(ll of resid, ll of third_resid, alpha of other_resid, posterior mean of other_resid at MEAN_M points)``."""
    ref = dn.reference(n, D, dtype)
    half_logdet = float(np.sum(np.log(np.diag(ref.L))))

    def ll(r):
        z = sla.solve_triangular(ref.L, r.astype(np.float64), lower=True, check_finite=False)
        return -0.5 * float(z @ z) - half_logdet - 0.5 * n * math.log(2.0 * math.pi)

    r2 = other_resid(n, dtype)
    alpha = sla.cho_solve((ref.L, True), r2.astype(np.float64), check_finite=False)
    Xt = dn.query_points(MEAN_M, D, dtype)[0].astype(np.float64)
    mean = dn.kernel(o, D)(Xt, ref.X) @ alpha
    return ll(resid(n, dtype)), ll(third_resid(n, dtype)), dn._frozen(alpha), dn._frozen(mean)


# ---- checks -----------------------------------------------------------------------------------------------------------
def _ratio(got, want, rtol, atol):
    """``max |got - want| / (atol + rtol |want|)``: the error in units of assert_allclose's bar (NaN counts as inf)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    if got.shape != want.shape:
        return math.inf
    with np.errstate(all="ignore"):
        r = np.abs(got - want) / (atol + rtol * np.abs(want))
    return math.inf if not np.all(np.isfinite(r)) else float(np.max(r, initial=0.0))


class Ledger:
    """Worst ratio to the bar per kind of quantity; the names of everything past its bar."""

    def __init__(self):
        self.worst, self.failed, self.same = {}, [], {}

    def add(self, kind, name, ratio):
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)
        if not ratio <= 1.0:
            self.failed.append(f"{name}: {ratio:.3g} of the bar")

    def note_same(self, pair, a, b):
        """Remember whether every instance of ``pair`` was bit-identical (printed; asserted only where listed)."""
        self.same[pair] = self.same.get(pair, True) and bool(np.array_equal(a, b))

    def equal(self, name, a, b):
        if not (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)):
            self.failed.append(f"{name}: not bit-identical")

    def line(self, what):
        return (f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())) + " of the bar; identical: "
                + ", ".join(f"{k} {v}" for k, v in sorted(self.same.items())))


def gather_factor(per_rank, n, nb, world):
    """The driver's own factor (n, n) from every owner's block columns; every block column exactly once."""
    nblk = nblocks(n, nb)
    npad = nblk * nb
    L = np.zeros((npad, npad), dtype=np.float64)
    for rank, res in enumerate(per_rank):
        owned = sorted(int(k.split("/")[1]) for k in res if k.startswith("col/"))
        assert owned == list(range(rank, nblk, world)), (rank, owned)
        for j in owned:
            col = res[f"col/{j}"]
            assert col.shape == (npad - j * nb, nb), (j, col.shape)
            L[j * nb:, j * nb:(j + 1) * nb] = col
    return np.tril(L)[:n, :n]


def check(case, world, per_rank, on_device):
    """One sweep case: every rank's results against the references, the forms against each other, every rank against
    rank 0 to the bit.  Returns the :class:`Ledger` (asserted empty of failures here)."""
    n, nb, dtype = case
    assert len(per_rank) == world
    led = Ledger()
    ref = dn.reference(n, D, dtype)
    tol = dn.posterior_bar(dtype)
    llbar = dg.BARS[dtype]["ll"]
    fwd, bwd = solve_refs(n, dtype)
    want_ll, want_rll, want_alpha, want_mean = vector_refs(n, dtype)
    Ldev = gather_factor(per_rank, n, nb, world)
    Y = dn.rhs(n, dtype)
    dot_want, dot_mag = dn.dot_reference(Ldev, Y[:, :3])
    dot_lim = dn.dot_bar(n, dtype, dot_mag)
    nblk = nblocks(n, nb)

    def solve_like(kind, name, got, want, rank):
        assert got.dtype == np.dtype(dtype), (name, got.dtype)
        led.add(kind, f"{name} rank {rank}", _ratio(got, want, *dn.solve_bar(dtype, want)))

    for rank, res in enumerate(per_rank):
        assert int(res["info"]) == 0
        owns = len(range(rank, nblk, world))
        assert res["panels"][0] == res["panels"][1], "a panel was factored again"
        assert (res["panels"][0] > 0) == (owns > 0), (rank, res["panels"], owns)
        led.add("ll", f"ll rank {rank}", _ratio(res["ll"], want_ll, llbar, 0.0))
        led.add("ll", f"resident ll rank {rank}", _ratio(res["rll"], want_rll, llbar, 0.0))
        solve_like("solve", "fwd/vec", res["fwd/vec"], fwd[:, 0], rank)
        solve_like("solve", "bwd/vec", res["bwd/vec"], bwd[:, 0], rank)
        for r in R_WIDTHS:
            solve_like("solve", f"bwd/{r}", res[f"bwd/{r}"], bwd[:, :r], rank)
            for form in FORMS:
                solve_like("solve", f"fwd/{form}/{r}", res[f"fwd/{form}/{r}"], fwd[:, :r], rank)
            # left-looking against right-looking, on the reference's scale
            led.note_same("fwd left=right", res[f"fwd/left/{r}"], res[f"fwd/right/{r}"])
            led.add("left-right", f"fwd left against right {r} rank {rank}",
                    _ratio(res[f"fwd/left/{r}"], res[f"fwd/right/{r}"], 0.0, dn.solve_bar(dtype, fwd[:, :r])[1]))
        solve_like("solve", "alpha", res["alpha"], want_alpha, rank)
        led.add("posterior", f"mean rank {rank}", _ratio(res["mean"], want_mean, tol["rtol"], tol["atol"]))
        for key, want, lim in (("dot/vec", dot_want[:, 0], dot_lim[:, 0]), ("dot/3", dot_want, dot_lim)):
            got = res[key]
            assert got.shape == want.shape and got.dtype == np.dtype(dtype)
            with np.errstate(all="ignore"):
                rr = np.abs(got.astype(np.longdouble) - want) / lim
            led.add("dot", f"{key} rank {rank}", float(np.max(rr)) if np.all(np.isfinite(rr)) else math.inf)
        for m in VAR_MS:
            want_var, _, Kss = cross_refs(n, dtype, m, False)
            cvar = dn.conditional(D, n, m, True, False, False, dtype)[1]
            for form in FORMS:
                for tag in ("one", "chunked"):
                    key = f"var/{form}/{tag}/{m}"
                    solve_like("colsumsq", key, res[key], want_var, rank)
                    led.add("posterior", f"variance {key} rank {rank}",
                            _ratio(np.diag(Kss) - res[key].astype(np.float64), cvar, tol["rtol"], tol["atol"]))
        for m in GRAM_MS:
            _, want_gram, Kss = cross_refs(n, dtype, m, False)
            nz = dn.query_points(m, D, dtype)[1].astype(np.float64)
            ccov = dn.conditional(D, n, m, True, True, False, dtype)[0]
            for form in FORMS:
                for tag in ("one", "chunked"):
                    key = f"gram/{form}/{tag}/{m}"
                    solve_like("gram", key, res[key], want_gram, rank)
                    np.testing.assert_array_equal(res[key], res[key].T, err_msg=key)
                    led.add("posterior", f"covariance {key} rank {rank}",
                            _ratio(Kss + np.diag(nz) - res[key].astype(np.float64), ccov, tol["rtol"], tol["atol"]))
            _, want_other, Kss_o = cross_refs(n, dtype, m, True)
            ccov_o = dn.conditional(D, n, m, True, True, True, dtype)[0]
            for tag in ("one", "chunked"):
                key = f"gram_other/{tag}/{m}"
                solve_like("gram", key, res[key], want_other, rank)
                led.add("posterior", f"covariance {key} rank {rank}",
                        _ratio(Kss_o + np.diag(nz) - res[key].astype(np.float64), ccov_o, tol["rtol"], tol["atol"]))
        # the forms against each other, on the reference's scale
        for what, ms in (("var", VAR_MS), ("gram", GRAM_MS)):
            for m in ms:
                want = cross_refs(n, dtype, m, False)[0 if what == "var" else 1]
                atol = dn.solve_bar(dtype, want)[1]
                for tag in ("one", "chunked"):
                    led.add("left-right", f"{what} left against right {tag}/{m} rank {rank}",
                            _ratio(res[f"{what}/left/{tag}/{m}"], res[f"{what}/right/{tag}/{m}"], 0.0, atol))
                for form in FORMS:
                    a, b = res[f"{what}/{form}/chunked/{m}"], res[f"{what}/{form}/one/{m}"]
                    if m > CHUNK:
                        led.note_same(f"{what} {form} chunked=one", a, b)
                    if on_device and identical_on_device(what, nb, world):
                        led.equal(f"{what} chunked against one pass {form}/{m} rank {rank}", a, b)
                    led.add("chunked-one", f"{what} chunked against one pass {form}/{m} rank {rank}", _ratio(a, b, 0.0, atol))
        for m in GRAM_MS:
            atol = dn.solve_bar(dtype, cross_refs(n, dtype, m, True)[1])[1]
            led.add("chunked-one", f"gram_other chunked against one pass {m} rank {rank}",
                    _ratio(res[f"gram_other/chunked/{m}"], res[f"gram_other/one/{m}"], 0.0, atol))
        # replicated results: every rank has rank 0's bits
        if rank:
            for key, val in per_rank[0].items():
                if not key.startswith("col/") and key != "panels":
                    led.equal(f"{key} rank {rank} against rank 0", np.asarray(res[key]), np.asarray(val))
    assert not led.failed, f"{case_id(case)} world {world}: " + "; ".join(led.failed)
    return led


def check_grad(case, world, per_rank):
    name, n, nb, chunk = case
    ref = dg.reference(name, n)
    led = Ledger()
    for rank, res in enumerate(per_rank):
        assert int(res["info"]) == 0 and np.isfinite(res["ll"])
        assert len(res["kernel"]) == dg.N_KERNEL[name]
        for k, v in dg.errors(ref, res["ll"], res["kernel"], res["noise"], res["mean"]).items():
            led.add(f"grad {k}", f"{k} rank {rank}", v)
        dg.check(ref, res["ll"], res["kernel"], res["noise"], res["mean"])
        if rank:
            for key, val in per_rank[0].items():
                led.equal(f"{key} rank {rank} against rank 0", np.asarray(res[key]), np.asarray(val))
    assert not led.failed, f"{case_id(case)} world {world}: " + "; ".join(led.failed)
    return led
