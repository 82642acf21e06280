"""The host side of the batched small dense gradient (``tgp_small_logprob_grad``, ``tinygp_amd/solvers/small.py``)
without a GPU: the reference's own conditions at every case ``test_gpu_1_small_grad.py`` uses, the agreement of header,
prototype and binding, the public names, the per-member output offsets and the mapping from the device's ``[2 i + q]``
layout to ``kernel.parameters()``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import _ffi, kernels, transforms
from tinygp_amd.solvers import DirectSolver, small

import _dense_grad_np as dg
import _dense_small as ds
import _dense_small_grad as sg

ROOT = Path(__file__).resolve().parent.parent


# ---- the reference's own conditions -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.NAMES)
def test_reference_conditions_at_every_case_the_gpu_file_uses(name):
    cond = gap = 0.0
    light = np.inf
    for n, b in sg.gpu_cases():
        ref = sg.reference(name, n, b)  # asserts cond, the LU route and, from n = 3, the two edge weights
        cond, gap = max(cond, ref.cond), max(gap, ref.route_gap)
        if n >= 3:
            light = min(light, ref.last_row, ref.first_col)
    print(f"{name}: worst cond {cond:.3g}, worst LU gap {gap:.3g}, lightest last row / first column {light:.4g} bars")
    assert cond <= sg.COND_MAX and gap <= sg.ROUTE_GAP_MAX and light >= sg.WEIGHT_MIN
    # member 0 is _dense_grad_np's own problem: the same numbers as its reference where that one has no tile condition
    mine, theirs = sg.reference(name, 128, 0), dg.reference(name, 128)
    assert mine.ll == theirs.ll and np.array_equal(mine.g, theirs.g) and np.array_equal(mine.alpha, theirs.alpha)
    assert len(mine.g) == dg.N_KERNEL[name] + (3 if name == "linear" else 0)


def test_the_length_scale_derivative_is_exactly_zero_at_one_point():
    for name in sg.NAMES:
        ref = sg.reference(name, 1, 0)
        assert ref.g[1 if name != "m32c" else 0] == 0.0, name


# ---- header, prototype, binding -----------------------------------------------------------------------------------------
def test_header_prototype_and_binding_agree():
    text = (ROOT / "include" / "tgp_hip.h").read_text()
    assert int(re.search(r"#define\s+TGP_ABI_VERSION\s+(\d+)", text).group(1)) == _ffi.ABI_VERSION == 6
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int\s+tgp_small_logprob_grad\s*\((.*?)\)\s*;", plain, flags=re.S)
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    ctype = {"tgp_ctx*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const tgp_kop*": C.c_void_p,
             "const int32_t*": _ffi._pi32, "const int64_t*": _ffi._pi64, "const double*": C.c_void_p,
             "int32_t*": _ffi._pi32, "double*": _ffi._pdbl}
    want = [ctype[a.rsplit(" ", 1)[0]] for a in args]
    names = [a.rsplit(" ", 1)[1] for a in args]
    value = re.search(r"int\s+tgp_small_logprob\s*\((.*?)\)\s*;", plain, flags=re.S)
    value_names = [" ".join(a.split()).rsplit(" ", 1)[1] for a in value.group(1).split(",")]
    # the arguments of tgp_small_logprob, and the gradient's own
    assert names == value_names[:12] + ["want_dims"] + value_names[12:] + ["grad_params_host", "grad_noise_host",
                                                                          "alpha_host", "grad_logscale_host"]
    assert _ffi.SIGNATURES["tgp_small_logprob_grad"] == want
    assert _ffi.SIGNATURES["tgp_small_logprob_grad"][:12] == _ffi.SIGNATURES["tgp_small_logprob"][:12]
    lib = _ffi.load_library()  # needs no GPU
    assert lib.tgp_small_logprob_grad.argtypes == want and lib.tgp_abi_version() == 6
    # without a context the call is refused before anything is touched
    none = [None] * 19
    none[1], none[6], none[8] = 1, 1, 0
    assert lib.tgp_small_logprob_grad(*none) == _ffi.E_ARG
    assert b"null context" in lib.tgp_last_error()


def test_public_entry_points_exist():
    assert tinygp_amd.log_probability_and_grad_datasets is small.log_probability_and_grad_datasets
    assert callable(DirectSolver.log_probability_and_grad_batch)
    # the pinned absences: the quasiseparable names stay the quasiseparable solver's
    assert not hasattr(DirectSolver, "value_and_grad_batch") and not hasattr(DirectSolver, "value_and_grad")
    doc = tinygp_amd.GaussianProcess.log_probability_and_grad_batch.__doc__
    assert "QuasisepSolver" in doc and "DirectSolver.log_probability_and_grad_batch" in doc
    assert "log_probability_and_grad_datasets" in doc
    assert "kernels[b].parameters()" in DirectSolver.log_probability_and_grad_batch.__doc__
    import inspect

    sig = inspect.signature(DirectSolver.log_probability_and_grad_batch)
    assert list(sig.parameters) == ["self", "kernels", "resid", "noise", "vectors", "return_info"]
    assert sig.parameters["vectors"].default is True and sig.parameters["return_info"].default is False
    sig = inspect.signature(tinygp_amd.log_probability_and_grad_datasets)
    assert list(sig.parameters) == ["kernels", "Xs", "ys", "diags", "means", "vectors", "return_info", "ctx"]


# ---- the per-member output offsets --------------------------------------------------------------------------------------
class _FakeLib:
    """Stands in for the library: records the call and fills every output with the index it was written at."""

    def __init__(self):
        self.calls = []

    def tgp_small_logprob_grad(self, ctx, nb, progs, prog_off, x_off, n, d, X, x_rows, vec_off, noise, resid, want_dims,
                               info, out, gparams, gnoise, alpha, glog):
        nops = prog_off[nb]
        total = sum(n[b] for b in range(nb))
        self.calls.append(dict(nb=nb, d=d, want_dims=None if not want_dims else [want_dims[b] for b in range(nb)],
                               vectors=bool(gnoise), glog=bool(glog)))
        for b in range(nb):
            out[b], info[b] = -10.0 - b, 0
        for t in range(2 * nops):
            gparams[t] = float(t)
        for t in range(total):
            if gnoise:
                gnoise[t], alpha[t] = 1000.0 + t, 2000.0 + t
        if glog:
            for t in range(nb * d):
                glog[t] = 3000.0 + t
        return 0


def test_outputs_are_read_at_the_members_offsets(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_ffi, "lib", lambda: fake)
    monkeypatch.setattr(_ffi, "default_ctx", lambda: type("Ctx", (), {"handle": None})())
    lin = transforms.Linear(np.array([1.0, 2.0, 0.5]), kernels.ExpSquared(1.2, distance=kernels.L2Distance()))
    ks = [kernels.Matern32(1.5, distance=kernels.L2Distance()),                          # 1 op
          1.5 * lin,                                                                      # 3 ops, a covering transform
          kernels.Exp(1.0) + kernels.ExpSineSquared(2.0, gamma=0.7) * kernels.Constant(0.3)]  # 5 ops
    ns = (5, 9, 2)
    Xs = [dg.inputs(n, 3)[0] for n in ns]
    ys = [np.asarray(dg.inputs(n, 3)[2]) for n in ns]
    values, grads, info = tinygp_amd.log_probability_and_grad_datasets(ks, Xs, ys, diags=[0.1, 0.2, 0.3],
                                                                       return_info=True)
    assert fake.calls == [dict(nb=3, d=3, want_dims=[0, 1, 0], vectors=True, glog=True)]
    assert values.tolist() == [-10.0, -11.0, -12.0] and info.tolist() == [0, 0, 0]
    # grad_params at 2 * prog_off[b]: prog_off = [0, 1, 4, 9]
    assert grads["kernel"][0].tolist() == [0.0]                    # op 0 p0
    assert grads["kernel"][1].tolist() == [2.0, 4.0]               # Constant at op 0 -> 2, ExpSquared scale at op 1 -> 4
    assert grads["kernel"][2].tolist() == [8.0, 10.0, 11.0, 12.0]  # Exp, ESS scale and gamma, Constant
    assert [len(k.parameters()) for k in ks] == [1, 2, 4]
    # the vectors at vec_off[b] = [0, 5, 14]
    assert grads["noise_diag"][1].tolist() == [1005.0 + t for t in range(9)]
    assert grads["mean"][2].tolist() == [2014.0, 2015.0] and grads["mean"][0].shape == (5,)
    # the scale gradients at b * d, through the transform's own rule d / d s_q = (d / d log s_q) / s_q
    assert grads["transform"][0] is None and grads["transform"][2] is None
    assert np.array_equal(grads["transform"][1], np.array([3003.0, 3004.0, 3005.0]) / np.array([1.0, 2.0, 0.5]))
    # vectors=False: no vector outputs are passed at all; nobody with a transform: no scale output
    fake.calls.clear()
    values, grads = tinygp_amd.log_probability_and_grad_datasets([ks[0], ks[2]], Xs[:2], ys[:2], diags=[0.1, 0.2],
                                                                 vectors=False)
    assert fake.calls == [dict(nb=2, d=3, want_dims=None, vectors=False, glog=False)]
    assert grads["noise_diag"] is None and grads["mean"] is None and grads["transform"] == [None, None]
    assert grads["kernel"][1].tolist() == [2.0, 4.0, 5.0, 6.0]


def test_the_raw_packing_of_mixed_structures_and_ragged_lengths():
    ks = [kernels.Matern32(1.5), 1.3 * kernels.ExpSquared(1.5), kernels.Exp(1.0) + kernels.Matern52(2.0) * kernels.Cosine(3.0)]
    ns = (4, 7, 3)
    members = [small.lower_member(k, dg.inputs(n, 1)[0]) + (np.full(n, 0.1), np.zeros(n)) for k, n in zip(ks, ns)]
    p = small.pack_members(members)
    assert p.prog_off.tolist() == [0, 1, 4, 9] and p.vec_off.tolist() == [0, 4, 11] and p.n.tolist() == [4, 7, 3]
    assert 2 * len(p.progs) == 18  # the length of grad_params


# ---- the [2 i + q] layout and kernel.parameters() ------------------------------------------------------------------------
def test_the_device_layout_maps_onto_the_parameters_of_a_nested_program():
    ess, rq = kernels.ExpSineSquared(1.7, gamma=0.6), kernels.RationalQuadratic(1.2, alpha=0.8)
    poly = kernels.Polynomial(2.0, scale=2.5, sigma=0.7)
    k = 0.5 * kernels.Exp(1.1) + ess * kernels.Cosine(5.0) + kernels.Constant(0.2) * (poly + rq) + kernels.DotProduct()
    prog = k.program()
    gparams = np.arange(2 * len(prog), dtype=np.float64)
    kgrad, tgrad = small.member_gradient(k, gparams)
    assert tgrad is None and kgrad.dtype == np.float64
    params = k.parameters()
    assert len(kgrad) == len(params) == 11
    slots = []
    k._slots(slots)
    assert len(slots) == len(prog)
    want = [2 * i + q for i, pair in enumerate(slots) for q in (0, 1) if pair[q] is not None]
    assert kgrad.tolist() == [float(t) for t in want]
    # every named parameter is the op's p0 / p1 (Polynomial's order is the POW op's p0)
    for (obj, attr), t in zip(params, want):
        assert float(getattr(obj, attr)) == float(prog[t // 2][2 + t % 2]), (attr, t)
    # operators and DotProduct own no parameter: their slots are skipped whatever the device wrote there
    skipped = sorted(set(range(2 * len(prog))) - set(want))
    assert all(slots[t // 2][t % 2] is None for t in skipped) and len(skipped) == 2 * len(prog) - 11
    with pytest.raises(ValueError, match="program ops"):
        small.member_gradient(k, gparams[:-2])
    # a covering transform: scalar and per-dimension scales, and the failed member's NaN in the same shapes
    lin = 1.5 * transforms.Linear(np.array([1.0, 2.0, 0.5]), kernels.ExpSquared(1.2, distance=kernels.L2Distance()))
    kgrad, tgrad = small.member_gradient(lin, np.arange(6.0), np.array([3.0, 4.0, 5.0]))
    assert kgrad.tolist() == [0.0, 2.0] and np.array_equal(tgrad, np.array([3.0, 2.0, 10.0]))
    assert small.member_gradient(lin, np.arange(6.0))[1] is None
    kg, tg = small.failed_gradient(kgrad, tgrad)
    assert kg.shape == (2,) and tg.shape == (3,) and np.all(np.isnan(kg)) and np.all(np.isnan(tg))
    scalar = transforms.Linear(0.8, kernels.Matern32(1.3))
    assert small.member_gradient(scalar, np.arange(2.0), np.array([3.0, 4.0]))[1] == pytest.approx(7.0 / 0.8)
    # a transform beside a leaf on the raw coordinates does not cover the kernel: no flag, no gradient
    assert small.dims_flags([scalar + kernels.Matern32(1.0), kernels.Matern32(1.0)]) is None
    assert small.dims_flags([scalar + kernels.Matern32(1.0), scalar, lin]).tolist() == [0, 1, 1]
