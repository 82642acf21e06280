"""Prediction for sets of series (``tgp_qsep_series_predict``): the split rule of ``csrc/qsep.hip`` restated on the host,
the host's value-sort-then-locate order, and the test points of the tests (test infrastructure; shared by
``test_quasisep_series_predict_cpu.py`` and ``test_gpu_4_quasisep_series_predict.py``).

DESIGN section 11, "Batches of series: prediction": a call runs as launch chains filled in the order given, a function
of (N_0 .. N_{B-1}, M_0 .. M_{B-1}, J, mean wanted or not, variance wanted or not) alone.  If ``series_predict_need`` or
``series_predict_split`` in ``csrc/qsep.hip`` change, this has to follow by hand (the handle reports the number of
chains of a call, not the rule)."""
import functools

import numpy as np

from _quasisep_series import CAP_DOUBLES, MAX_LEVELS, MAX_MEMBERS, MODEL_DOUBLES, extent, series

PT = 10  # doubles a test point keeps between the forward and the backward pass: q^T F, q^T D q, e (8)
BUDGET = CAP_DOUBLES - MAX_MEMBERS * MODEL_DOUBLES


def need(n, m, J, want_mean=True, want_var=True):
    """Doubles of a chain's buffer that a series of n points with m test points takes: the value's noise, residual, c,
    z (n each), w (n J), per-chunk sums and bad-pivot slots (3 per chunk) and results (3); the scan work space at the
    prediction scan's 384 per element of MAX_LEVELS levels; its entry in the table of test points (3); with the mean
    alpha (n); per test point xt, sidx, order (1 each), pt (PT) and the mean and the variance if wanted (1 each)."""
    e = extent(n)
    s4 = sum(e.levels) + MAX_LEVELS - len(e.levels)
    return (n * (4 + J) + 384 * s4 + 3 * e.nchunks + 6 + (n if want_mean else 0)
            + m * (3 + PT + bool(want_mean) + bool(want_var)))


def series_predict_split(lengths, counts, J, want_mean=True, want_var=True):
    """The members of every chain: filled in the order given, a chain ends at MAX_MEMBERS members or before the member
    whose need would take it past the cap.  ``None``: a series does not fit alone (the call is refused).  A member at its
    own data counts its N_b test points."""
    needs = [need(n, m, J, want_mean, want_var) for n, m in zip(lengths, counts)]
    if any(x > BUDGET for x in needs):
        return None
    chains, used = [], 0
    for x in needs:
        if not chains or chains[-1] == MAX_MEMBERS or used + x > BUDGET:
            chains.append(0)
            used = 0
        chains[-1] += 1
        used += x
    return chains


def sort_then_locate(t, x):
    """What the chain does with one member's test points: ``(order, sidx)``.  The host sorts them by value (stable, NaN
    first: the key of a NaN is -inf), the device then finds, for sorted position j, the interval of x[order[j]] -- the
    number of t_n <= x less one, by the bisection of ``interval_of`` restated here."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    key = np.where(np.isnan(x), -np.inf, x)
    order = np.argsort(key, kind="stable")
    sidx = np.empty(len(x), dtype=np.int64)
    for j, p in enumerate(order):
        lo, hi = 0, len(t)
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if t[mid] <= x[p]:
                lo = mid + 1
            else:
                hi = mid
        sidx[j] = lo - 1
    return order, sidx


@functools.lru_cache(maxsize=None)
def test_points(n, m, seed=0):
    """m unsorted test points for ``series(n)``: drawn from a little before the first datum to a little after the last,
    so that every placement occurs by itself at m = 300; the first few are planted -- before the first point, after the
    last, exactly on data points (twice the same one: a duplicate), and either side of the last chunk boundary."""
    t = series(n)[0]
    rng = np.random.default_rng(1000 * n + m + seed)
    span = t[-1] - t[0] + 1.0
    x = rng.uniform(t[0] - 0.05 * span, t[-1] + 0.05 * span, m)
    e = extent(n)
    edge = min((e.nchunks - 1) * e.lc, n - 1)  # the first step of the last chunk
    planted = [t[0] - 0.7, t[-1] + 0.3, t[n // 2], t[n // 2], t[0], t[-1], t[edge], np.nextafter(t[edge], -np.inf),
               0.5 * (t[edge] + t[max(edge - 1, 0)])]
    k = min(m, len(planted))
    x[:k] = planted[:k]
    x = rng.permutation(x)
    x.setflags(write=False)
    return x


test_points.__test__ = False  # a helper, not a test
