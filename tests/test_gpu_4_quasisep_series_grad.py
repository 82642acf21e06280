"""Value and gradient for sets of series (``QuasisepSeriesSet.value_and_grad`` / ``tgp_qsep_series_grad``): every member
to the bit against the device's single ``value_and_grad`` on a fresh ``QuasisepSolver`` -- value, every kernel-gradient
entry, noise gradient and alpha -- whatever the set's size, the member's position, the other members' lengths, the split
into launch chains and direction passes and the vectors asked for; once per case against the sequential oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver
from tinygp_amd.solvers.quasisep import pack_series, pack_series_tangents

import _quasisep_grad_np as og
import _quasisep_series as qs
import _quasisep_series_grad as qg
from _quasisep_cases import CASES
from _quasisep_grad_batch import member, member_noise

pytestmark = pytest.mark.gpu


def _member(name, b):
    return member(CASES, q, name, b)


def _single_call(k, t, noise, r):
    """The device's single call on a fresh solver: ``(value, kernel (P,), noise gradient (N,), alpha (N,))``."""
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    try:
        v, g = s.value_and_grad(r)
    finally:
        s.close()
    return float(v), np.array(g["kernel"], dtype=np.float64), np.asarray(g["noise_diag"]), np.asarray(g["mean"])


@functools.lru_cache(maxsize=None)
def _single(name, n, b):
    """Member b of case ``name`` on the series of length n, alone; computed once for every set that holds it."""
    t, noise, r = qs.series(n)
    out = _single_call(_member(name, b), t, member_noise(noise, b), r)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _inputs(name, lengths, bs):
    """Member i: the series of length lengths[i] under kernel and noise number bs[i]."""
    data = [qs.series(n) for n in lengths]
    return ([_member(name, b) for b in bs], [d[0] for d in data],
            [member_noise(d[1], b) for d, b in zip(data, bs)], [d[2] for d in data])


def _same(values, grads, i, want, tag=""):
    """Member i of a set's result has the bits of a single call's."""
    v, gk, gn, al = want
    assert values[i] == v, (tag, i, values[i], v)
    assert np.array_equal(grads["kernel"][i], gk, equal_nan=True), (tag, i, grads["kernel"][i], gk)
    if grads["noise_diag"] is not None:
        assert grads["noise_diag"][i].shape == gn.shape and np.array_equal(grads["noise_diag"][i], gn), (tag, i)
        assert grads["mean"][i].shape == al.shape and np.array_equal(grads["mean"][i], al), (tag, i)


def _evaluate(name, lengths, bs, **kw):
    ks, ts, nz, rs = _inputs(name, lengths, bs)
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    try:
        values, grads, info = s.value_and_grad(ks, rs, nz, return_info=True, **kw)
    finally:
        s.close()
    assert values.shape == (len(lengths),) and values.dtype == np.float64 and not info.any()
    assert grads["kernel"].dtype == np.float64 and grads["kernel"].shape[0] == len(lengths) and grads["transform"] is None
    return values, grads


def _raw(s, kernels, ys, diags, *, ndir=None, gnoise=True, alpha=True):
    """The low-level call: ``(out, info, dout, gnoise, alpha, nchains, npasses)``."""
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, kernels, ys, diags)
    dleaves, dh, dP, _ = pack_series_tangents(s.lengths, kernels)
    nb, total = len(s), int(s.lengths.sum())
    ndir = dh.shape[1] if ndir is None else ndir
    info, out, dout = np.zeros(nb, dtype=np.int32), np.empty(nb), np.zeros((nb, ndir))
    gn, al = np.empty(total) if gnoise else None, np.empty(total) if alpha else None
    nchains, npasses = C.c_int32(-1), C.c_int32(-1)
    _ffi.check(_ffi.lib().tgp_qsep_series_grad(
        s._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
        _ffi.ptr(noise), _ffi.ptr(resid), ndir, _ffi.ptr(dleaves), _ffi.ptr(dh), _ffi.ptr(dP), _ffi.ptr(info),
        _ffi.ptr(out), _ffi.ptr(dout), _ffi.ptr(gn), _ffi.ptr(al), C.byref(nchains), C.byref(npasses)),
        "tgp_qsep_series_grad")
    return out, info, dout, gn, al, nchains.value, npasses.value


def _dims(name):
    k = CASES[name](q)
    return k._lower_ssm().J, len(k.parameters())


def _mirror(name, lengths, vectors=True):
    """``(nchains, npasses)`` of the host's restatement of the rule."""
    chains = qg.series_grad_split(lengths, *_dims(name), vectors)
    return len(chains), sum(c[2] for c in chains)


# -- 1. every scan edge in one set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", qs.EDGE_CASES)
def test_every_scan_edge_in_one_set(name, reverse):
    """One- and two-level scans, 64 and 65 chunks and last chunks of one step side by side, J = 1, 2, 6 and 8; celerite4's
    16 directions run as two passes of 8.  A length keeps its kernel and noise when the order is reversed.  The forward
    order is also held to the sequential oracle at the project's bars (value 1e-8; kernel 2e-6, noise 1e-6, mean 1e-7
    of the largest reference entry)."""
    order = list(range(len(qs.EDGE_LENGTHS)))[::-1 if reverse else 1]
    lengths = [qs.EDGE_LENGTHS[b] for b in order]
    values, grads = _evaluate(name, lengths, order)
    assert grads["kernel"].shape == (len(lengths), _dims(name)[1])
    for i, (n, b) in enumerate(zip(lengths, order)):
        _same(values, grads, i, _single(name, n, b), f"{name} n={n}")
    if reverse:
        return
    for i, (n, b) in enumerate(zip(lengths, order)):
        t, noise, r = qs.series(n)
        wll, wg, wgn, walpha = og.value_and_grad(_member(name, b), t, member_noise(noise, b), r)
        ks, ns, ms = np.abs(wg).max(), np.abs(wgn).max(), np.abs(walpha).max()
        gk, gn, al = grads["kernel"][i], grads["noise_diag"][i], grads["mean"][i]
        print(f"{name} n={n}: value rel {abs(values[i] - wll) / abs(wll):.2e}; kernel {np.abs(gk - wg).max() / ks:.2e}; "
              f"noise {np.abs(gn - wgn).max() / ns:.2e}; mean {np.abs(al - walpha).max() / ms:.2e} of max")
        assert values[i] == pytest.approx(wll, rel=1e-8)
        np.testing.assert_allclose(gk, wg, rtol=2e-6, atol=2e-6 * ks)
        np.testing.assert_allclose(gn, wgn, rtol=1e-6, atol=1e-6 * ns)
        np.testing.assert_allclose(al, walpha, rtol=1e-7, atol=1e-7 * ms)


# -- 2. mixed chunk lengths and scan depths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qs.MIXED_CASES)
def test_mixed_chunk_lengths_and_depths(name):
    """Chunks of 32, 16, 128 and 16 steps, scans of two, one, two and one level; celerite4: one chain of two 8-direction
    passes."""
    lengths = qs.MIXED_LENGTHS
    assert [qs.extent(n).lc for n in lengths] == [32, 16, 128, 16]
    assert [len(qs.extent(n).levels) for n in lengths] == [2, 1, 2, 1]
    if name == "celerite4":
        assert qg.series_grad_split(lengths, 8, 16, True) == [(4, 8, 2)]
    ks, ts, nz, rs = _inputs(name, lengths, range(4))
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    values, grads = s.value_and_grad(ks, rs, nz)
    raw = _raw(s, ks, rs, nz)
    s.close()
    assert (raw[5], raw[6]) == _mirror(name, lengths) and not raw[1].any()
    assert np.array_equal(raw[0], values) and np.array_equal(raw[2], grads["kernel"])
    assert np.array_equal(raw[3], np.concatenate(grads["noise_diag"])) and np.array_equal(raw[4], np.concatenate(grads["mean"]))
    for b, n in enumerate(lengths):
        _same(values, grads, b, _single(name, n, b), f"{name} n={n}")


# -- 3. one, two and three levels in one chain -----------------------------------------------------------------------------------
def test_one_two_and_three_scan_levels_in_one_chain():
    name, lengths = "matern32", qs.DEEP_LENGTHS
    assert [len(qs.extent(n).levels) for n in lengths] == [3, 1, 2, 1]
    assert qg.series_grad_split(lengths, 2, 2, True) == [(4, 2, 1)]
    values, grads = _evaluate(name, lengths, range(4), vectors=True)
    for b, n in enumerate(lengths):
        _same(values, grads, b, _single(name, n, b), f"n={n}")


# -- 4. position and company do not matter ------------------------------------------------------------------------------------
def test_position_and_company_do_not_matter():
    name, n = qs.PROBE_CASE, qs.PROBE_LENGTH
    want = _single(name, n, 7)
    for nb in (2, 5):
        for pos in range(nb):
            lengths = [qs.COMPANY_LENGTHS[b % 4] for b in range(nb)]
            bs = [b % 11 for b in range(nb)]
            lengths[pos], bs[pos] = n, 7
            values, grads = _evaluate(name, lengths, bs)
            _same(values, grads, pos, want, f"set of {nb}, position {pos}")


# -- 5. splits ------------------------------------------------------------------------------------------------------------------------
def test_sixty_five_series_run_as_two_chains():
    name, n, nb = "matern32", 40, 65
    bs = [b % 13 for b in range(nb)]
    ks, ts, nz, rs = _inputs(name, [n] * nb, bs)
    assert qg.series_grad_split([n] * nb, 2, 2, True) == [(64, 2, 1), (1, 2, 1)]
    s = QuasisepSeriesSet(ts)
    out, info, dout, gn, al, nchains, npasses = _raw(s, ks, rs, nz)
    s.close()
    assert (nchains, npasses) == (2, 2) == _mirror(name, [n] * nb) and not info.any() and np.all(np.isfinite(out))
    grads = {"kernel": dout, "noise_diag": gn.reshape(nb, n), "mean": al.reshape(nb, n)}
    for b in (62, 63, 64):
        _same(out, grads, b, _single(name, n, bs[b]))


def test_the_cap_cuts_the_chain_and_the_passes():
    """Ten series of 2^20 points, J = 2, P = 2, vectors: 10.5 M doubles per member and 3.95 M per direction, so nine
    members leave room for one direction per pass (two passes) and the tenth runs alone with both (one pass)."""
    name, n, nb = "matern32", 1 << 20, 10
    assert qg.series_grad_split([n] * nb, 2, 2, True) == [(9, 1, 2), (1, 2, 1)]
    ks, ts, nz, rs = _inputs(name, [n] * nb, range(nb))
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    out, info, dout, gn, al, nchains, npasses = _raw(s, ks, rs, nz)
    s.close()
    assert (nchains, npasses) == (2, 3) == _mirror(name, [n] * nb) and not info.any() and np.all(np.isfinite(out))
    grads = {"kernel": dout, "noise_diag": gn.reshape(nb, n), "mean": al.reshape(nb, n)}
    for b in (0, nb - 1):
        _same(out, grads, b, _single(name, n, b))


# -- 6. vectors ------------------------------------------------------------------------------------------------------------------------
def test_without_the_vectors_the_rest_keeps_its_bits():
    name, lengths = "m32cos_plus_sho", [1025, 17, 300, 4097]
    ks, ts, nz, rs = _inputs(name, lengths, range(4))
    s = QuasisepSeriesSet(ts)
    values, grads = s.value_and_grad(ks, rs, nz, vectors=False)
    assert grads["noise_diag"] is None and grads["mean"] is None
    for b, n in enumerate(lengths):
        _same(values, grads, b, _single(name, n, b))
    full = _raw(s, ks, rs, nz)
    only_gnoise = _raw(s, ks, rs, nz, alpha=False)
    only_alpha = _raw(s, ks, rs, nz, gnoise=False)
    value_only = _raw(s, ks, rs, nz, ndir=0, gnoise=False, alpha=False)
    plain = s.log_probability(ks, rs, nz)
    s.close()
    assert np.array_equal(full[0], values) and np.array_equal(full[2], grads["kernel"])
    for got in (only_gnoise, only_alpha):
        assert np.array_equal(got[0], values) and np.array_equal(got[2], grads["kernel"]) and not got[1].any()
    assert only_gnoise[4] is None and np.array_equal(only_gnoise[3], full[3])
    assert only_alpha[3] is None and np.array_equal(only_alpha[4], full[4])
    assert np.array_equal(value_only[0], plain) and np.array_equal(plain, values) and value_only[6] == 0


# -- 7. failure stays in its member ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_failure_stays_in_its_member(pos):
    """noise = -10 at local step 5 of one series: h^T P^- h <= k(0) = 1.44 (1 + 0.04 b)^2, so that pivot is negative."""
    name, lengths = "matern32", [300, 1025, 64]
    lengths = lengths[-pos:] + lengths[:-pos]  # the series of 1025 points fails: in the middle, last, first
    bad = lengths.index(1025)
    ks, ts, nz, rs = _inputs(name, lengths, range(3))
    nz[bad] = nz[bad].copy()
    nz[bad][5] = -10.0
    s = QuasisepSeriesSet(ts)
    values, grads, info = s.value_and_grad(ks, rs, nz, return_info=True)
    raw = _raw(s, ks, rs, nz)
    s.close()
    assert list(info) == list(raw[1]) == [6 if b == bad else 0 for b in range(3)]
    assert values[bad] == -np.inf and np.isnan(raw[0][bad]) and np.all(np.isnan(raw[2][bad]))
    assert np.all(np.isnan(grads["kernel"][bad])) and grads["noise_diag"][bad].shape == (1025,)
    assert np.all(np.isnan(grads["noise_diag"][bad])) and np.all(np.isnan(grads["mean"][bad]))
    lo = int(np.sum(lengths[:bad]))
    assert np.all(np.isnan(raw[3][lo:lo + 1025])) and np.all(np.isnan(raw[4][lo:lo + 1025]))
    for b in range(3):
        if b != bad:
            _same(values, grads, b, _single(name, lengths[b], b))


# -- 8. kernels ------------------------------------------------------------------------------------------------------------------
def test_one_shared_kernel_equals_equal_copies():
    name, lengths = "m32cos_plus_sho", [17, 1025, 300]
    _, ts, nz, rs = _inputs(name, lengths, range(3))
    s = QuasisepSeriesSet(ts)
    shared = s.value_and_grad(_member(name, 2), rs, nz)
    copies = s.value_and_grad([_member(name, 2) for _ in lengths], rs, nz)
    s.close()
    assert np.all(np.isfinite(shared[0])) and np.array_equal(shared[0], copies[0])
    assert np.array_equal(shared[1]["kernel"], copies[1]["kernel"])
    for key in ("noise_diag", "mean"):
        assert all(np.array_equal(a, b) for a, b in zip(shared[1][key], copies[1][key]))
    t, _, r = qs.series(1025)
    _same(*shared, 1, _single_call(_member(name, 2), t, nz[1], r))


def test_damping_regimes_share_one_set():
    ks = [q.SHO(omega=1.5, quality=quality) for quality in (3.0, 0.5, 0.3)]
    assert len({int(k._lower_ssm().leaves[0, 0]) for k in ks}) == 3
    iq = [attr for _, attr in ks[0].parameters()].index("quality")
    lengths = [1025, 40, 300]
    data = [qs.series(n) for n in lengths]
    s = QuasisepSeriesSet([d[0] for d in data])
    values, grads, info = s.value_and_grad(ks, [d[2] for d in data], [d[1] for d in data], return_info=True)
    s.close()
    assert not info.any() and np.all(np.isfinite(values))
    want = np.zeros_like(grads["kernel"], dtype=bool)
    want[1, iq] = True  # the critically damped member's quality, and nothing else
    assert np.array_equal(np.isnan(grads["kernel"]), want)
    assert all(np.all(np.isfinite(a)) for key in ("noise_diag", "mean") for a in grads[key])
    for b, (k, (t, noise, r)) in enumerate(zip(ks, data)):
        _same(values, grads, b, _single_call(k, t, noise, r))


# -- 9. the handle ---------------------------------------------------------------------------------------------------------------
def test_the_handle_serves_call_after_call():
    """log_probability, the gradient with J = 2, with J = 8, without the vectors, log_probability again: the resident
    table is cut again before each, and every call has the bits of a fresh set's and of the single calls."""
    lengths = [1025, 17, 300]
    _, ts, nz, rs = _inputs("matern32", lengths, range(3))
    first = [_member("matern32", b) for b in range(3)]        # J = 2
    second = [_member("celerite4", b) for b in range(3)]      # J = 8

    def fresh(method, ks, **kw):
        s = QuasisepSeriesSet(ts)
        try:
            return getattr(s, method)(ks, rs, nz, **kw)
        finally:
            s.close()

    s = QuasisepSeriesSet(ts)
    a = s.log_probability(first, rs, nz)
    b = s.value_and_grad(first, rs, nz)
    c = s.value_and_grad(second, rs, nz)
    d = s.value_and_grad(first, rs, nz, vectors=False)
    e = s.log_probability(first, rs, nz)
    s.close()
    assert np.array_equal(a, fresh("log_probability", first)) and np.array_equal(e, a)
    for got, (name, ks, kw) in ((b, ("matern32", first, {})), (c, ("celerite4", second, {})),
                                (d, ("matern32", first, {"vectors": False}))):
        want = fresh("value_and_grad", ks, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1]["kernel"], want[1]["kernel"])
        for key in ("noise_diag", "mean"):
            if kw:
                assert got[1][key] is None and want[1][key] is None
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got[1][key], want[1][key]))
        for i, n in enumerate(lengths):
            _same(*got, i, _single(name, n, i), name)
    assert np.array_equal(a, b[0])
    with pytest.raises(ValueError, match="closed"):
        s.value_and_grad(first, rs, nz)


# -- 10. the public function -------------------------------------------------------------------------------------------------------
def test_public_function_equals_separate_gps():
    name, lengths = "m32cos_plus_sho", [1000, 33, 257, 1]
    ks, ts, _, ys = _inputs(name, lengths, range(4))
    diags = [0.1, 0.15, qs.series(257)[1], 0.05]
    for means in ([0.0, 0.3, -0.2, 1.5], [0.1 * np.cos(t) for t in ts], None):
        values, grads = tinygp_amd.log_probability_and_grad_series(ks, ts, ys, diags=diags, means=means)
        assert values.shape == (4,) and values.dtype == np.float64 and grads["kernel"].shape == (4, 7)
        for b in range(4):
            mean = {} if means is None else {"mean": means[b]} if np.ndim(means[b]) == 0 else {"mean_value": means[b]}
            v, g = GaussianProcess(ks[b], ts[b], diag=diags[b], **mean).log_probability_and_grad(ys[b])
            _same(values, grads, b, (float(v), np.array(g["kernel"]), np.asarray(g["noise_diag"]), np.asarray(g["mean"])))
    values, grads = tinygp_amd.log_probability_and_grad_series(ks, ts, ys, diags=diags, vectors=False)
    assert grads["noise_diag"] is None and grads["mean"] is None and np.all(np.isfinite(grads["kernel"]))


# -- 11. argument errors of the C entry point ---------------------------------------------------------------------------------
def test_grad_refuses_null_arrays_and_negative_directions():
    name, lengths = "matern32", [17, 40]
    ks, ts, nz, rs = _inputs(name, lengths, range(2))
    s = QuasisepSeriesSet(ts)
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, ks, rs, nz)
    dleaves, dh, dP, _ = pack_series_tangents(s.lengths, ks)
    info, out, dout = np.zeros(2, dtype=np.int32), np.empty(2), np.empty((2, 2))
    full = [leaves, smap, h, P, noise, resid, dleaves, dh, dP, info, out, dout]

    def call(a, ndir):
        _ffi.check(_ffi.lib().tgp_qsep_series_grad(
            s._handle, _ffi.ptr(a[0]), leaves.shape[1], _ffi.ptr(a[1]), h.shape[1], _ffi.ptr(a[2]), _ffi.ptr(a[3]),
            _ffi.ptr(a[4]), _ffi.ptr(a[5]), ndir, _ffi.ptr(a[6]), _ffi.ptr(a[7]), _ffi.ptr(a[8]), _ffi.ptr(a[9]),
            _ffi.ptr(a[10]), _ffi.ptr(a[11]), None, None, None, None))

    for missing in range(len(full)):
        with pytest.raises(ValueError, match="null"):
            call([None if i == missing else x for i, x in enumerate(full)], 2)
    with pytest.raises(ValueError, match="negative number of directions"):
        call(full, -1)
    # without directions their arrays may be missing
    call([None if 6 <= i <= 8 or i == 11 else x for i, x in enumerate(full)], 0)
    values, grads = s.value_and_grad(ks, rs, nz)  # the refusals left the set usable
    s.close()
    assert np.array_equal(out, values)
    for b, n in enumerate(lengths):
        _same(values, grads, b, _single(name, n, b))


def test_a_series_beyond_the_cap_is_refused():
    """6 000 000 points with J = 8 and P = 16 need more than 23 n = 1.38 * 10^8 doubles with one direction, the cap is
    2^27 = 1.34 * 10^8; the check precedes every allocation of the chain's buffer and every launch, and a short
    neighbour does not help.  (5 000 000 points fit: the mirror's worked example.)"""
    n = 6_000_000
    assert qg.series_grad_split([40, n], 8, 16, True) is None and qg.series_grad_split([40, 5_000_000], 8, 16, True)
    t = np.zeros(n)
    s = QuasisepSeriesSet([t[:40], t], assume_sorted=True)
    with pytest.raises(ValueError, match=r"series 1 \(n = 6000000\) .*exceeds its cap"):
        s.value_and_grad(_member("celerite4", 0), [t[:40], t], [1.0, 1.0])
    s.close()


# -- 12. the set and the batch run one sequence ------------------------------------------------------------------------------
def test_a_set_on_equal_time_stamps_has_the_bits_of_the_batch():
    """Three series on the same 1040 time stamps (chunks of 16 steps, 65 chunks, a two-level scan) as a set, where an
    extent table says where each member lies, and as a batch over one handle, where strides do: the same host arrays
    give the same bits.  Members have their own model, noise and residual; P = 3."""
    name, n, nb = "sho_over", 1040, 3
    assert qs.extent(n) == (16, 65, (65, 2))
    t, noise, _ = qs.series(n)
    ks = [_member(name, b) for b in range(nb)]
    nz = [member_noise(noise, b) for b in range(nb)]
    rs = [qs.series(n, seed=b + 1)[2] for b in range(nb)]
    lengths = np.full(nb, n, dtype=np.int64)
    leaves, smap, h, P, noise_c, resid_c = pack_series(lengths, ks, rs, nz)
    dleaves, dh, dP, _ = pack_series_tangents(lengths, ks)
    nl, J, ndir = leaves.shape[1], h.shape[1], dh.shape[1]
    assert ndir == 3 and noise_c.shape == resid_c.shape == (nb * n,)
    lib = _ffi.lib()

    def outputs(p, vectors):
        return (np.empty(nb), np.zeros(nb, dtype=np.int32), np.zeros((nb, p)),
                np.empty(nb * n) if vectors else None, np.empty(nb * n) if vectors else None)

    def as_set(s, p, vectors):
        out, info, dout, gn, al = outputs(p, vectors)
        _ffi.check(lib.tgp_qsep_series_grad(
            s._handle, _ffi.ptr(leaves), nl, _ffi.ptr(smap), J, _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise_c),
            _ffi.ptr(resid_c), p, _ffi.ptr(dleaves), _ffi.ptr(dh), _ffi.ptr(dP), _ffi.ptr(info), _ffi.ptr(out),
            _ffi.ptr(dout), _ffi.ptr(gn), _ffi.ptr(al), None, None), "tgp_qsep_series_grad")
        return out, info, dout, gn, al

    def as_batch(b, p, vectors):
        out, info, dout, gn, al = outputs(p, vectors)
        _ffi.check(lib.tgp_qsep_grad_batch(
            b._handle, nb, _ffi.ptr(leaves), nl, _ffi.ptr(smap), J, _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise_c), n,
            _ffi.ptr(resid_c), n, p, _ffi.ptr(dleaves), _ffi.ptr(dh), _ffi.ptr(dP), _ffi.ptr(info), _ffi.ptr(out),
            _ffi.ptr(dout), _ffi.ptr(gn), _ffi.ptr(al), None, None), "tgp_qsep_grad_batch")
        return out, info, dout, gn, al

    s = QuasisepSeriesSet([t] * nb, assume_sorted=True)
    b = QuasisepSolver(ks[0], t, Diagonal(nz[0]), assume_sorted=True)
    try:
        set_full, batch_full = as_set(s, ndir, True), as_batch(b, ndir, True)
        set_value, batch_value = as_set(s, 0, False), as_batch(b, 0, False)
        set_plain, batch_plain = outputs(0, False)[:2], outputs(0, False)[:2]
        _ffi.check(lib.tgp_qsep_series_logprob(
            s._handle, _ffi.ptr(leaves), nl, _ffi.ptr(smap), J, _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise_c),
            _ffi.ptr(resid_c), _ffi.ptr(set_plain[1]), _ffi.ptr(set_plain[0]), None), "tgp_qsep_series_logprob")
        _ffi.check(lib.tgp_qsep_logprob_batch(
            b._handle, nb, _ffi.ptr(leaves), nl, _ffi.ptr(smap), J, _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise_c), n,
            _ffi.ptr(resid_c), n, _ffi.ptr(batch_plain[1]), _ffi.ptr(batch_plain[0]), None), "tgp_qsep_logprob_batch")
    finally:
        s.close()
        b.close()
    assert not set_full[1].any() and all(np.all(np.isfinite(a)) for a in set_full)
    assert len(set(set_full[0])) == nb  # the members differ
    for what, got, want in zip(("out", "info", "dout", "gnoise", "alpha"), set_full, batch_full):
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), what
    assert set_value[3] is None and set_value[4] is None and batch_value[3] is None and batch_value[4] is None
    for got in (set_value, batch_value, set_plain, batch_plain):
        assert np.array_equal(got[0], set_full[0]) and np.array_equal(got[1], set_full[1])
