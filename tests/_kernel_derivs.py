"""Programs, pairs and the reference of the two-point probe of every kernel derivative (``test_gpu_2_kernel_derivs.py``;
its conditions are asserted without a GPU by ``test_kernel_derivs_cpu.py``).

A member is a GP on n = 2 points.  Its gradient is

    g_p = 1/2 G_00 dK_00 + G_10 dK_10 + 1/2 G_11 dK_11,      G = alpha alpha^T - K^-1,

so the device's derivative at ONE pair of points is visible on its own, and the whole reference is a 2 x 2 closed form.
It is computed in ``np.longdouble`` and rounded to float64 at the end: K from the oracle's leaves
(``oracle.tinygp_np``; the dot-product leaf from ``oracle.kernel_derivs_np.dot_value``), det, K^-1 and alpha written
out for 2 x 2, dK from the closed forms of ``oracle/kernel_derivs_np.py`` composed by the sum, product and power rules
below.  Nothing is differenced.

Programs are trees of the node classes below; a tree builds the product's kernel (``Program.build``) and evaluates its
own value and derivatives from the same theta.  Noise and residual of a member scale with the largest diagonal entry of
its noise-free K (noise 0.12 and 0.08 of it), so that cond(K) <= (2 + 0.08) / 0.08 = 26 for every program, the
polynomial ones at D = 16 included.

``WRONG`` switches single closed forms to deliberately wrong variants; the CPU file uses it to show that the chosen
pairs tell the formulas apart.  Everything returned from a cache is read-only.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import kernel_derivs_np as kd
from oracle import tinygp_np as o

import _dense_grad_np as dg

LD = np.longdouble
BARS = dg.BARS
COND_MAX = 1e4
WEIGHT_MIN = 100.0
DS = (1, 2, 3, 16)  # 16: TGP_MAX_DIM
_frozen = dg._frozen

# the deliberately wrong closed forms of the discrimination table (test_kernel_derivs_cpu.py); empty: the right ones
VARIANTS = ("w_swap", "l1_for_l2", "m52_no_1pa", "ess_gamma_sign", "rq_alpha_no_log", "dot_scale_factor2",
            "product_one_term")
WRONG = set()


# ---- closed forms, with the wrong variants beside them ---------------------------------------------------------------
def _dleaf(leaf, X, param):
    if "l1_for_l2" in WRONG and isinstance(leaf.distance, o.L2Distance):
        extra = {k: getattr(leaf, k) for k in ("gamma", "alpha") if hasattr(leaf, k)}
        leaf = type(leaf)(leaf.scale, distance=o.L1Distance(), **extra)
    l = float(leaf.scale)
    if "m52_no_1pa" in WRONG and isinstance(leaf, o.Matern52):
        a = np.sqrt(5) * kd._r(leaf, X, X) / l
        return (a * a / 3) * np.exp(-a) / l
    if "ess_gamma_sign" in WRONG and isinstance(leaf, o.ExpSineSquared) and param == "gamma":
        return -kd.dleaf(leaf, X, X, param)
    if "rq_alpha_no_log" in WRONG and isinstance(leaf, o.RationalQuadratic) and param == "alpha":
        q = 0.5 * kd._r(leaf, X, X, squared=True) / (float(leaf.alpha) * l**2)
        return (1 + q) ** -float(leaf.alpha) * (q / (1 + q) - (1 + q))
    return kd.dleaf(leaf, X, X, param)


def _dleaf_dlog(leaf, X):
    if "w_swap" in WRONG:  # the weight of the OTHER metric: |d_q| / sum |d| under L2, d_q^2 / sum d^2 under L1
        d = X[:, None, :] - X[None, :, :]
        l1 = isinstance(leaf.distance, o.L1Distance)
        num = d * d if l1 else np.abs(d)
        den = np.sum(num, axis=-1)
        w = np.where((den > 0)[..., None], num / np.where(den > 0, den, np.ones_like(den))[..., None], np.zeros_like(d))
        return (kd.dleaf_dr(leaf, X, X) * kd._r(leaf, X, X))[None] * np.moveaxis(w, -1, 0)
    return kd.dleaf_dlogscale(leaf, X, X)


def _ddot(X, scale, sigma, param):
    if "dot_scale_factor2" in WRONG and param == "scale":
        return kd.ddot(X, X, scale, sigma, param) / 2
    return kd.ddot(X, X, scale, sigma, param)


# ---- the nodes of a program: value (2, 2), derivs [(2, 2)] in the order of kernel.parameters(), dlog (D, 2, 2) -------------
class Leaf:
    """A stationary leaf: ``kind`` of oracle.tinygp_np / tinygp_amd.kernels under metric "L1" or "L2"."""

    dot = False

    def __init__(self, kind, scale, metric, **extra):
        self.kind, self.scale, self.metric, self.extra = kind, scale, metric, extra
        self.names = ["scale"] + list(extra)

    def _make(self, mod):
        return getattr(mod, self.kind)(self.scale, distance=getattr(mod, self.metric + "Distance")(), **self.extra)

    def build(self, mod):
        return self._make(mod)

    def slots(self):
        return [(self.__dict__, "scale")] + [(self.extra, k) for k in self.extra]

    def value(self, X):
        return self._make(o)(X, X)

    def derivs(self, X):
        return [_dleaf(self._make(o), X, p) for p in self.names]

    def dlog(self, X):
        return _dleaf_dlog(self._make(o), X)


class Const:
    dot = False

    def __init__(self, value):
        self.c = value

    def build(self, mod):
        return mod.Constant(self.c)

    def slots(self):
        return [(self.__dict__, "c")]

    def value(self, X):
        return np.full((len(X), len(X)), self.c, dtype=X.dtype)

    def derivs(self, X):
        return [np.ones((len(X), len(X)), dtype=X.dtype)]

    def dlog(self, X):
        return np.zeros((X.shape[1], len(X), len(X)), dtype=X.dtype)


class Dot:
    """``DotProduct``: x1 . x2, no parameter."""

    dot = True

    def build(self, mod):
        return mod.DotProduct()

    def slots(self):
        return []

    def value(self, X):
        return kd.dot_value(X, X)

    def derivs(self, X):
        return []

    def dlog(self, X):
        return kd.ddot_dlogscale(X, X, 1.0)


class Poly:
    """``Polynomial``: u^P with u = x1 . x2 / l^2 + sigma^2; parameters scale, sigma, order; the power rule."""

    dot = True

    def __init__(self, order, scale, sigma):
        self.order, self.scale, self.sigma = order, scale, sigma

    def build(self, mod):
        return mod.Polynomial(self.order, scale=self.scale, sigma=self.sigma)

    def slots(self):
        return [(self.__dict__, k) for k in ("scale", "sigma", "order")]

    def _u(self, X):
        u = kd.dot_value(X, X, self.scale, self.sigma)
        assert np.all(u > 0), "sigma must keep the base positive"
        return u

    def value(self, X):
        return self._u(X) ** self.order

    def derivs(self, X):
        u = self._u(X)
        chain = self.order * u ** (self.order - 1)
        return [chain * _ddot(X, self.scale, self.sigma, "scale"), chain * _ddot(X, self.scale, self.sigma, "sigma"),
                u**self.order * np.log(u)]

    def dlog(self, X):
        u = self._u(X)
        return (self.order * u ** (self.order - 1))[None] * kd.ddot_dlogscale(X, X, self.scale)


class _Binary:
    def __init__(self, a, b):
        self.a, self.b = a, b
        self.dot = a.dot or b.dot

    def slots(self):
        """``(dict, key)`` of every parameter, in the order of ``derivs`` (the CPU file differences through them)."""
        return self.a.slots() + self.b.slots()


class Add(_Binary):
    def build(self, mod):
        return mod.Sum(self.a.build(mod), self.b.build(mod))

    def value(self, X):
        return self.a.value(X) + self.b.value(X)

    def derivs(self, X):
        return self.a.derivs(X) + self.b.derivs(X)

    def dlog(self, X):
        return self.a.dlog(X) + self.b.dlog(X)


class Mul(_Binary):
    def build(self, mod):
        return mod.Product(self.a.build(mod), self.b.build(mod))

    def value(self, X):
        return self.a.value(X) * self.b.value(X)

    def derivs(self, X):
        va, vb = self.a.value(X), self.b.value(X)
        second = [np.zeros_like(va) for _ in self.b.derivs(X)] if "product_one_term" in WRONG else \
            [va * d for d in self.b.derivs(X)]
        return [d * vb for d in self.a.derivs(X)] + second

    def dlog(self, X):
        va, vb = self.a.value(X), self.b.value(X)
        first = self.a.dlog(X) * vb[None]
        return first if "product_one_term" in WRONG else first + va[None] * self.b.dlog(X)


class Program:
    """A tree, optionally under ONE ``transforms.Linear(vector)`` ("linear") or ``transforms.Cholesky(vector)``
    ("cholesky"); ``vector(D)`` gives the per-dimension parameter.  x' = s x under Linear, x / f under Cholesky, so
    d / d s_q = (d / d log s_q) / s_q  and  d / d f_q = -(d / d log s_q) / f_q  (log s_q = -log f_q)."""

    def __init__(self, tree, transform=None):
        self.tree, self.transform = tree, transform
        self.dot = tree.dot
        self.vectors = {}

    def vector(self, D):
        if D not in self.vectors:
            self.vectors[D] = np.round(np.random.default_rng([5, D]).uniform(0.6, 1.6, D), 3)
        return self.vectors[D]

    def build(self, kernels, transforms, D):
        k = self.tree.build(kernels)
        if self.transform == "linear":
            return transforms.Linear(np.array(self.vector(D)), k)
        if self.transform == "cholesky":
            return transforms.Cholesky(np.array(self.vector(D)), k)
        return k

    def _mapped(self, X):
        if self.transform is None:
            return X
        v = self.vector(X.shape[1]).astype(X.dtype)
        return X * v if self.transform == "linear" else X / v

    def value(self, X):
        return self.tree.value(self._mapped(X))

    def derivs(self, X):
        """``(dK per kernel parameter, dK per entry of the transform's vector)``."""
        Xm = self._mapped(X)
        own = self.tree.derivs(Xm)
        if self.transform is None:
            return own, []
        v = self.vector(X.shape[1]).astype(X.dtype)
        sign = 1 if self.transform == "linear" else -1
        return own, [sign * dl / v[q] for q, dl in enumerate(self.tree.dlog(Xm))]


# ---- the programs ------------------------------------------------------------------------------------------------------
def _leaf(kind, metric, scale=None):
    scales = dict(Exp=1.3, ExpSquared=1.1, Matern32=1.6, Matern52=0.9, Cosine=2.7, ExpSineSquared=1.9,
                  RationalQuadratic=1.2)
    extra = dict(ExpSineSquared=dict(gamma=0.7), RationalQuadratic=dict(alpha=1.4)).get(kind, {})
    return Leaf(kind, scales[kind] if scale is None else scale, metric, **extra)


KINDS = ("Exp", "ExpSquared", "Matern32", "Matern52", "Cosine", "ExpSineSquared", "RationalQuadratic")
FAST_KINDS = KINDS[:4]  # FastEval's four leaves


def _programs():
    groups = {}
    # every stationary leaf, both metrics, as leaf / amp * leaf / leaf * amp: FastEval's eight specialisations in three
    # forms each, and the one-leaf and two-leaf shortcuts of the general evaluator
    g = groups["leaf"] = {}
    for kind in KINDS:
        for metric in ("L1", "L2"):
            g[f"{kind}_{metric}"] = Program(_leaf(kind, metric))
            g[f"amp*{kind}_{metric}"] = Program(Mul(Const(1.7), _leaf(kind, metric)))
            g[f"{kind}_{metric}*amp"] = Program(Mul(_leaf(kind, metric), Const(0.6)))
    g = groups["product"] = {}
    g["ExpSquared_L1*Cosine_L2"] = Program(Mul(_leaf("ExpSquared", "L1"), _leaf("Cosine", "L2")))
    g["ESS_L2*RQ_L1"] = Program(Mul(_leaf("ExpSineSquared", "L2"), _leaf("RationalQuadratic", "L1")))
    g["sum_of_products"] = Program(Add(Mul(Mul(Const(1.3), _leaf("Matern32", "L2")), _leaf("ExpSineSquared", "L1")),
                                       Mul(_leaf("RationalQuadratic", "L2"), Mul(Const(0.8), _leaf("Exp", "L1")))))
    g = groups["deep"] = {}
    # right-nested: the postfix program is its eight leaves, then seven operators -- stack depth 8, the first leaf's
    # derivative seeded at the bottom of the stack and the last one's at the top
    g["deep8"] = Program(Add(_leaf("Exp", "L1"), Mul(_leaf("ExpSquared", "L2"), Add(
        _leaf("Matern32", "L2"), Mul(_leaf("Matern52", "L1"), Add(_leaf("Cosine", "L2"), Mul(
            _leaf("ExpSineSquared", "L1"), Add(_leaf("RationalQuadratic", "L2"), Const(0.9)))))))))
    # 32 operations, the longest program: seven amp * leaf terms (21), a polynomial (2) and a constant, summed (9)
    terms = [Mul(Const(0.5 + 0.1 * i), _leaf(kind, "L2" if i % 2 else "L1")) for i, kind in enumerate(KINDS)]
    tree = terms[0]
    for t in terms[1:]:
        tree = Add(tree, t)
    g["long32"] = Program(Add(Add(tree, Poly(2.0, 2.2, 1.7)), Const(0.4)))
    g = groups["dot"] = {}
    g["DotProduct"] = Program(Dot())
    g["Polynomial"] = Program(Poly(2.5, 2.0, 1.7))
    g["Polynomial*Matern32_L2"] = Program(Mul(Poly(2.5, 2.0, 1.7), _leaf("Matern32", "L2")))
    g = groups["linear"] = {}
    for kind in KINDS:
        for metric in ("L1", "L2"):
            g[f"Linear({kind}_{metric})"] = Program(_leaf(kind, metric), "linear")
    g["Linear(Matern52_L1*ExpSquared_L2)"] = Program(Mul(_leaf("Matern52", "L1"), _leaf("ExpSquared", "L2")), "linear")
    g["Linear(DotProduct)"] = Program(Dot(), "linear")
    g["Linear(Polynomial)"] = Program(Poly(2.5, 2.0, 1.7), "linear")
    g = groups["cholesky"] = {}
    g["Cholesky(Exp_L2)"] = Program(_leaf("Exp", "L2"), "cholesky")
    g["Cholesky(Matern32_L1)"] = Program(_leaf("Matern32", "L1"), "cholesky")
    g["Cholesky(amp*RationalQuadratic_L2)"] = Program(Mul(Const(1.7), _leaf("RationalQuadratic", "L2")), "cholesky")
    return groups


GROUPS = _programs()
PROGRAMS = {name: p for g in GROUPS.values() for name, p in g.items()}
assert sum(len(g) for g in GROUPS.values()) == len(PROGRAMS)

# the single dense path in float32: the eight FastEval forms, one general family-0 program, one family-2 program.  (At
# float32's bar, 2e-3 of |g_p| + max |g|, 100 bars are 0.2 of the largest component and more: only programs of few
# parameters of similar weight can meet the off-diagonal condition, and these do; the longer ones meet it in float64.)
FP32_PROGRAMS = tuple(f"amp*{kind}_{metric}" for kind in FAST_KINDS for metric in ("L1", "L2")) + (
    "amp*Cosine_L2", "Polynomial*Matern32_L2")


# ---- the pairs ---------------------------------------------------------------------------------------------------------
PAIRS = ("generic", "wide", "one_coordinate", "identical", "close", "tiny", "far")
NONDEGENERATE = PAIRS[:3]
# the single dense path in float32 (a member there costs a handle and a launch chain; in float32 the separations of 1e-9
# and 1e-200 round away): the minimum of the three kinds.  In float64 it runs every pair, at ~1 ms a member.
FP32_PAIRS = ("generic", "one_coordinate", "identical")
FAR = 4000.0


def pairs_of(program):
    """The pairs a program is probed at.  ``far`` -- a separation at which exp(-a) underflows -- concerns the
    stationary leaves; a program with a dot-product leaf cannot meet cond(K) <= 1e4 there (its diagonal grows with
    |x|^2) and leaves it out."""
    return tuple(p for p in PAIRS if not (program.dot and p == "far"))


@functools.lru_cache(maxsize=None)
def pair_points(pair, D):
    """The two points (2, D) float64.  ``generic``: every coordinate differs, L1 distance ~ D^(1/4), L2 distance
    ~ D^(-1/4): of the order of the length scales (0.9 .. 2.7) at every D; ``wide``: three times that;
    ``one_coordinate``: 0.8 apart in coordinate D // 2 alone; ``identical``; ``close``: 1e-9 apart in every
    coordinate; ``tiny``: 0 and 1e-200 in coordinate D // 2 alone (r2 = 1e-400 underflows, r1 does not);
    ``far``: 4 000 apart in every coordinate."""
    rng = np.random.default_rng([7, D])
    x0 = rng.uniform(0.3, 1.2, D)
    sign = rng.choice([-1.0, 1.0], D)
    step = rng.uniform(0.5, 1.5, D) * sign / D**0.75
    j = D // 2
    x1 = x0.copy()
    if pair == "generic":
        x1 = x0 + step
    elif pair == "wide":
        x1 = x0 + 3.0 * step
    elif pair == "one_coordinate":
        x1[j] += 0.8
    elif pair == "close":
        x1 = x0 + 1e-9 * sign
    elif pair == "tiny":
        x0[j], x1[j] = 0.0, 1e-200
    elif pair == "far":
        x1 = x0 + FAR * sign
    else:
        assert pair == "identical", pair
    return _frozen(np.stack([x0, x1]))


NOISE_FRACTION = (0.12, 0.08)


def _resid_unit(pair, D):
    rng = np.random.default_rng([11, D, PAIRS.index(pair)])
    return rng.uniform(0.7, 1.5, 2) * np.array([1.0, -1.0 if rng.uniform() < 0.5 else 1.0])


# ---- the reference -----------------------------------------------------------------------------------------------------
def _compute(name, D, pair, dtype):
    prog = PROGRAMS[name]
    X = np.asarray(pair_points(pair, D), dtype=dtype)
    XL = X.astype(LD)
    K0 = prog.value(XL)
    kscale = float(max(K0[0, 0], K0[1, 1]))
    if not kscale > 1e-100:  # (DotProduct at the origin: K is the noise alone)
        kscale = 1.0
    noise = (np.array(NOISE_FRACTION) * kscale).astype(dtype)
    y = (_resid_unit(pair, D) * math.sqrt(kscale)).astype(dtype)
    a, b, c = K0[0, 0] + LD(noise[0]), K0[1, 0], K0[1, 1] + LD(noise[1])
    det = a * c - b * b
    Kinv = np.array([[c, -b], [-b, a]], dtype=LD) / det
    yl = y.astype(LD)
    alpha = Kinv @ yl
    ll = -(yl @ alpha) / 2 - np.log(det) / 2 - np.log(2 * LD(np.pi))
    G = np.outer(alpha, alpha) - Kinv
    dks, dts = prog.derivs(XL)
    dKs = list(dks) + list(dts)
    g = np.array([G[0, 0] * dK[0, 0] / 2 + G[1, 0] * dK[1, 0] + G[1, 1] * dK[1, 1] / 2 for dK in dKs], dtype=LD)
    off = np.array([abs(G[1, 0] * dK[1, 0]) for dK in dKs], dtype=LD)
    # eigenvalues of the symmetric 2 x 2
    mid, rad = (a + c) / 2, np.sqrt(((a - c) / 2) ** 2 + b * b)
    cond = float((mid + rad) / (mid - rad))
    frac = BARS[dtype]["kernel"]
    gmax = float(np.abs(g).max()) if len(g) else 0.0
    bars = frac * np.abs(g.astype(np.float64)) + frac * gmax
    with np.errstate(divide="ignore", invalid="ignore"):
        weight = np.where(bars > 0, off.astype(np.float64) / bars, 0.0)
    return SimpleNamespace(name=name, D=D, pair=pair, dtype=dtype, X=_frozen(X), noise_diag=_frozen(noise), y=_frozen(y),
                           ll=float(ll), g=_frozen(g.astype(np.float64)), n_kernel=len(dks),
                           noise=_frozen((np.diag(G) / 2).astype(np.float64)), alpha=_frozen(alpha.astype(np.float64)),
                           cond=cond, bars=_frozen(bars), weight=_frozen(weight))


@functools.lru_cache(maxsize=None)
def reference(name, D, pair, dtype="float64"):
    """The member of program ``name`` at ``pair_points(pair, D)`` rounded to ``dtype``: its inputs ``X`` (2, D),
    ``noise_diag`` and ``y`` in ``dtype``, and in float64 ``ll``, ``g`` (the kernel parameters in the order of
    ``kernel.parameters()``, ``n_kernel`` of them, then the transform's vector), ``noise`` = 1/2 diag G, ``alpha``;
    ``cond`` = cond(K), ``bars[p]`` the bar of g_p and ``weight[p]`` = |G_10 dK_p,10| in units of it."""
    assert not WRONG
    return _compute(name, D, pair, dtype)


def kernel(name, D, kernels, transforms):
    return PROGRAMS[name].build(kernels, transforms, D)


def full_gradient(kernel_grad, transform_grad):
    k = np.asarray(kernel_grad, dtype=np.float64).reshape(-1)
    return k if transform_grad is None else np.concatenate([k, np.ravel(np.asarray(transform_grad, dtype=np.float64))])


def errors(ref, ll, grad, noise_grad, mean_grad):
    """The worst error of each of the device's numbers in units of its bar (to print; ``check`` asserts)."""
    b = BARS[ref.dtype]
    e = dict(ll=abs(float(ll) - ref.ll) / (b["ll"] * abs(ref.ll)),
             noise=dg.in_bars(noise_grad, ref.noise, b["noise"], b["noise"]),
             mean=dg.in_bars(mean_grad, ref.alpha, b["mean"], b["mean"]))
    if len(ref.g):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.abs(np.asarray(grad, dtype=np.float64) - ref.g) / ref.bars
        e["kernel"] = float(np.max(np.where(np.asarray(grad) == ref.g, 0.0, r)))
    return e


def check(ref, ll, grad, noise_grad, mean_grad):
    """The device's numbers against ``ref`` at the project's bars; every number finite."""
    b = BARS[ref.dtype]
    what = f"{ref.name} D={ref.D} {ref.pair} {ref.dtype}"
    grad = np.asarray(grad, dtype=np.float64)
    assert grad.shape == ref.g.shape, what
    assert np.isfinite(ll) and np.all(np.isfinite(grad)) and np.all(np.isfinite(noise_grad)) \
        and np.all(np.isfinite(mean_grad)), what
    np.testing.assert_allclose(ll, ref.ll, rtol=b["ll"], err_msg=what)
    if len(ref.g):
        np.testing.assert_allclose(grad, ref.g, rtol=b["kernel"], atol=b["kernel"] * np.abs(ref.g).max(), err_msg=what)
    np.testing.assert_allclose(noise_grad, ref.noise, rtol=b["noise"], atol=b["noise"] * np.abs(ref.noise).max(),
                               err_msg=what)
    np.testing.assert_allclose(mean_grad, ref.alpha, rtol=b["mean"], atol=b["mean"] * np.abs(ref.alpha).max(),
                               err_msg=what)
