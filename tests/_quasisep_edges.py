"""Series, sizes and test points that put the quasiseparable scans on their edges (test infrastructure; shared by
``test_gpu_4_quasisep_edges.py``, ``test_quasisep_edges_cpu.py`` and ``test_gpu_4_quasisep_predict.py``).

Below 65 536 points a chunk holds 16 steps and a scan group 64 chunks.  ``EDGE_N`` walks the ends of both: one short and
one full chunk, a second chunk of one step, 64 chunks (the last one-level size) with a last chunk of 1, 15 and 16 steps,
65 chunks (a second group of one chunk) with that chunk of one step and full, and 5 groups whose last holds one chunk
of one step.  ``SHAPES`` states that as numbers and a test holds the list to it.  ``_levels`` restates the choice of
``tgp_qsep_create`` and ``level_sizes`` (the handle does not report its own): if ``qsep.hip`` changes that choice, the
table has to follow by hand."""
import numpy as np

LC = 16      # chunk length below 65 536 points
GROUP = 64   # chunks per scan group

EDGE_N = [15, 16, 17, 1009, 1023, 1024, 1025, 1040, 4097]
# N -> (chunks, levels, steps in the last chunk, groups at level 0, chunks in the last group)
SHAPES = {
    15: (1, 1, 15, 1, 1),
    16: (1, 1, 16, 1, 1),
    17: (2, 1, 1, 1, 2),
    1009: (64, 1, 1, 1, 64),
    1023: (64, 1, 15, 1, 64),
    1024: (64, 1, 16, 1, 64),
    1025: (65, 2, 1, 2, 1),
    1040: (65, 2, 16, 2, 1),
    4097: (257, 2, 1, 5, 1),
}
KERNELS = ["matern32", "m32cos_plus_sho", "celerite4"]  # J = 2, 6, 8 with 2, 7, 16 parameters


def _levels(n):
    """(chunk length, scan depth) of a series of n points, as ``tgp_qsep_create`` and ``level_sizes`` choose them."""
    lc = 16
    while lc < 256 and lc * 4096 < n:
        lc *= 2
    count, levels = -(-n // lc), 1
    while count > GROUP:
        count, levels = -(-count // GROUP), levels + 1
    return lc, levels


def shape(n):
    """The row of ``SHAPES`` for n, from the chunk arithmetic."""
    lc, levels = _levels(n)
    chunks = -(-n // lc)
    groups = -(-chunks // GROUP)
    return chunks, levels, n - (chunks - 1) * lc, groups, chunks - (groups - 1) * GROUP


def series(n, seed=None):
    """``(t, noise, r)``: t sorted uniform on [0, 0.05 n + 1] with one tie inside a chunk and one across the first
    chunk boundary."""
    rng = np.random.default_rng(n if seed is None else seed)
    t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    if n > 8:
        t[7] = t[6]
    if n > LC:
        t[LC] = t[LC - 1]
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)


def tied_points(t):
    n = len(t)
    return t[([6, 7] if n > 8 else []) + ([LC - 1, LC] if n > LC else [])]


def _test_points(t, m, seed, lc=LC):
    """Unsorted; outside the range on both sides, on data points (tied ones too), in the first and the last chunk
    and exactly on the data points either side of chunk boundaries."""
    rng = np.random.default_rng(seed)
    n = len(t)
    edges = np.unique(np.clip(np.concatenate([np.arange(lc - 1, n, lc), np.arange(lc, n, lc), [0, n - 1]]), 0, n - 1))
    edges = edges[rng.permutation(len(edges))[:60]]
    special = np.concatenate([
        t[edges], t[[0, n - 1]], t[:3], t[-3:],
        rng.uniform(t[0], t[min(lc, n) - 1], 8),            # inside the first chunk
        rng.uniform(t[max(0, n - lc // 2)], t[-1], 8),      # inside the last chunk
        t[0] - rng.uniform(0, 3, 6), t[-1] + rng.uniform(0, 3, 6), [t[0] - 40.0, t[-1] + 40.0],
    ])
    xt = np.concatenate([rng.uniform(t[0] - 1, t[-1] + 1, max(0, m - len(special))), special])
    return xt[rng.permutation(len(xt))]


def edge_test_points(t):
    """The test points of the edge sweep: ``_test_points(t, 200, seed=n)``, the tied data points and, up to N = 1040
    (where the dense reference is cheap), every data point."""
    n = len(t)
    parts = [_test_points(t, 200, seed=n), tied_points(t)]
    if n <= 1040:
        parts.append(t)
    return np.concatenate(parts)


def direction_matrix(ndir, npar, seed=5):
    """(ndir, npar) with entries in [-1, 1]; the first min(ndir, 3) rows are the unit vectors e_0, e_1, e_2."""
    C = np.random.default_rng(seed).uniform(-1.0, 1.0, (ndir, npar))
    for i in range(min(ndir, 3, npar)):
        C[i] = 0.0
        C[i, i] = 1.0
    return C


def combine_tangents(C, tangents):
    """``C @ tangents`` for ``dleaves``, ``dh`` and ``dPinf`` alike.  Zero coefficients are skipped, so a unit row is
    that tangent's own arrays, bit for bit."""
    out = []
    for field in ("dleaves", "dh", "dPinf"):
        arrs = [np.asarray(getattr(tg, field), dtype=np.float64) for tg in tangents]
        rows = []
        for row in C:
            acc = np.zeros_like(arrs[0])
            for cj, a in zip(row, arrs):
                if cj != 0.0:
                    acc = acc + cj * a
            rows.append(acc)
        out.append(np.stack(rows))
    return tuple(out)


def eight_exp_terms(q):
    """J = 8 as a sum of eight ``Exp`` terms of distinct scales and sigmas (the model of
    ``test_gpu_4_quasisep_terms.test_batching_does_not_matter``): ``(kernel, terms)``."""
    terms = [q.Exp(scale=0.3 * 1.7 ** j, sigma=0.5 + 0.1 * j) for j in range(8)]
    k = terms[0]
    for term in terms[1:]:
        k = k + term
    return k, terms


def grad_figures(got, want):
    """``(value rel, kernel, noise, mean)``: the last three as the largest difference over the largest reference
    entry."""
    ll, g = got
    wll, wg, wgn, walpha = want
    return (abs(ll - wll) / abs(wll), np.abs(np.asarray(g["kernel"]) - wg).max() / np.abs(wg).max(),
            np.abs(g["noise_diag"] - wgn).max() / np.abs(wgn).max(), np.abs(g["mean"] - walpha).max() / np.abs(walpha).max())
