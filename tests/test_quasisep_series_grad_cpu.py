"""Value and gradient for sets of series, host side: the mirrored split rule with its worked examples, the tangents'
packing and the entry point's declaration."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.solvers.quasisep import pack_series_tangents

import _quasisep_series as qs
import _quasisep_series_grad as qg
from _quasisep_cases import CASES

ROOT = Path(__file__).resolve().parent.parent
M = 1 << 20


# -- the mirrored rule -----------------------------------------------------------------------------------------------------------
def test_parts_of_a_short_and_a_long_series():
    # 40 points, J = 2, P = 2, vectors: 3 chunks, S4 = 3 + 3
    member, per_dir = qg.parts(40, 2, 2, True)
    assert member == 40 * 6 + 128 * 3 + 384 * 6 + 9 + 3 + 4 + 80 and per_dir == 40 * 3 + 192 * 6 + 6
    # 2^20 points, J = 2, P = 2, vectors: 4096 chunks, S4 = 4096 + 64 + 2
    assert qg.parts(M, 2, 2, True) == (8 * M + 128 * 4096 + 384 * 4162 + 12288 + 7, 3 * M + 192 * 4162 + 8192)
    assert qg.parts(M, 2, 2, True) == (10_523_399, 3_953_024)
    assert qg.FIXED == 64 * 141 + 64 * 8 * 104 and qg.BUDGET == (1 << 27) - qg.FIXED


def test_split_worked_examples():
    # the member limit cuts
    assert qg.series_grad_split([40] * 65, 2, 2, True) == [(64, 2, 1), (1, 2, 1)]
    # the cap cuts: nine members with one direction each take 130.3 M doubles, the rest holds no second direction
    assert qg.series_grad_split([M] * 10, 2, 2, True) == [(9, 1, 2), (1, 2, 1)]
    assert qg.series_grad_split([M] * 10, 8, 16, True) == [(4, 1, 16), (4, 1, 16), (2, 4, 4)]
    # the sets of the GPU tests
    assert qg.series_grad_split([M + 1, 40, 65_537, 1], 2, 2, True) == [(4, 2, 1)]
    assert qg.series_grad_split([65_537, 40, 262_145, 1], 8, 16, True) == [(4, 8, 2)]
    # one series alone, J = 8, P = 16: 23 n and the rest
    assert qg.series_grad_split([5_000_000], 8, 16, True) == [(1, 1, 16)]
    assert qg.series_grad_split([6_000_000], 8, 16, True) is None
    assert qg.series_grad_split([40, 6_000_000], 8, 16, True) is None  # a short neighbour does not help


@pytest.mark.parametrize("lengths, J", [([40] * 65, 2), ([40] * 128, 2), ([40] * 129, 8), ([M] * 10, 8), ([M] * 10, 2),
                                        ([M] * 9 + [40, M, 40], 8), ([40, M] * 9 + [M], 8), ([40, 12_000_000], 8),
                                        ([40, 12_000_000], 1)])
def test_the_value_alone_is_the_value_s_split_with_kept_prefixes(lengths, J):
    """P = 0 without vectors: a member takes what the value's chain takes plus its kept prefixes (2 x 64 per chunk), and
    the fixed part holds a pass's directions as well.  Neither changes the value's own examples."""
    for n in set(lengths):
        assert qg.parts(n, J, 0, False)[0] == qs.need(n, J) + 128 * qs.extent(n).nchunks
    assert qg.BUDGET == qs.CAP_DOUBLES - qs.MAX_MEMBERS * qs.MODEL_DOUBLES - 64 * 8 * 104
    got, want = qg.series_grad_split(lengths, J, 0, False), qs.series_split(lengths, J)
    if want is None:
        assert got is None
    else:
        assert [c[0] for c in got] == want and all(c[1:] == (0, 0) for c in got)


def test_adding_a_series_never_merges_chains():
    rng = np.random.default_rng(0)
    for trial in range(40):
        J, P = int(rng.choice([1, 2, 8])), int(rng.choice([0, 2, 16]))
        lengths = [int(n) for n in rng.choice([1, 40, 1025, 65_537, M, 3 * M], size=int(rng.integers(1, 40)))]
        before = qg.series_grad_split(lengths, J, P, True)
        after = qg.series_grad_split(lengths + [int(rng.choice([1, M, 3 * M]))], J, P, True)
        assert before is not None and after is not None
        assert len(after) >= len(before)
        assert after[:len(before) - 1] == before[:-1]  # every closed chain stays as it was
        assert after[len(before) - 1][0] >= before[-1][0] and sum(c[0] for c in after) == len(lengths) + 1


def test_sixty_four_members_is_a_hard_limit():
    assert [c[0] for c in qg.series_grad_split([1] * 200, 1, 2, False)] == [64, 64, 64, 8]
    assert [c[0] for c in qg.series_grad_split([1] * 64, 8, 16, True)] == [64]
    assert all(c[0] <= 64 for c in qg.series_grad_split([1, 40, 1025] * 50, 2, 2, True))


# -- the tangents -------------------------------------------------------------------------------------------------------------------
def _by_hand(kernels):
    tangents = [k._ssm_tangents() for k in kernels]
    return (np.stack([[t.dleaves for t in ts] for ts in tangents]), np.stack([[t.dh for t in ts] for ts in tangents]),
            np.stack([[t.dPinf for t in ts] for ts in tangents]))


def test_a_shared_kernel_is_lowered_once_and_repeated():
    k = CASES["m32cos_plus_sho"](q)
    dleaves, dh, dP, undefined = pack_series_tangents([3, 2, 7], k)
    ssm, npar = k._lower_ssm(), len(k.parameters())
    assert dleaves.shape == (3, npar, len(ssm.leaves), 4) and dh.shape == (3, npar, ssm.J)
    assert dP.shape == (3, npar, ssm.J, ssm.J) and undefined.shape == (3, npar) and undefined.dtype == bool
    assert all(a.flags.c_contiguous for a in (dleaves, dh, dP, undefined)) and not undefined.any()
    copies = pack_series_tangents([3, 2, 7], [CASES["m32cos_plus_sho"](q) for _ in range(3)])
    for a, b in zip((dleaves, dh, dP, undefined), copies):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    for a, b in zip((dleaves, dh, dP), _by_hand([k] * 3)):
        assert np.array_equal(a, b)


def test_b_kernels_are_stacked():
    ks = [q.Matern32(scale=1.0 + 0.1 * b, sigma=0.5 + b) for b in range(4)]
    got = pack_series_tangents([5, 1, 9, 2], ks)
    assert got[0].shape[:2] == (4, 2) and got[1].shape == (4, 2, 2) and got[2].shape == (4, 2, 2, 2)
    for a, b in zip(got[:3], _by_hand(ks)):
        assert np.array_equal(a, b) and a.dtype == np.float64
    assert not np.array_equal(got[2][0], got[2][3])


def test_a_critically_damped_member_is_flagged_and_zeroed():
    ks = [q.SHO(omega=1.5, quality=quality) for quality in (3.0, 0.5, 0.3)]
    iq = [attr for _, attr in ks[0].parameters()].index("quality")
    dleaves, dh, dP, undefined = pack_series_tangents([4, 4, 4], ks)
    want = np.zeros_like(undefined)
    want[1, iq] = True
    assert np.array_equal(undefined, want)
    assert not dleaves[1, iq].any() and not dh[1, iq].any() and not dP[1, iq].any()
    assert all(np.all(np.isfinite(a)) for a in (dleaves, dh, dP))
    shared = pack_series_tangents([4, 4], ks[1])
    assert np.array_equal(shared[3], want[[1, 1]])


def test_wrong_counts_name_the_member():
    k = q.Matern32(1.0)
    with pytest.raises(ValueError, match=r"kernels must be one kernel or one per series \(2\); got 3"):
        pack_series_tangents([3, 2], [k, k, k])
    with pytest.raises(ValueError, match=r"kernel 2 of the batch has 4 parameters, kernel 0 has 2"):
        pack_series_tangents([3, 2, 4], [k, q.Matern32(2.0), q.Matern32(1.0) + q.Matern32(3.0)])
    with pytest.raises(TypeError, match="kernel 1 of the batch"):
        pack_series_tangents([3, 2], [k, "matern"])


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tgp_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+tgp_qsep_series_grad\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/tgp_hip.h does not declare tgp_qsep_series_grad"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _ffi.SIGNATURES["tgp_qsep_series_grad"]
    assert len(params) == len(sig) == 20
    scalars = {i for i, p in enumerate(params) if "*" not in p}
    assert scalars == {2, 4, 9} and all(params[i].startswith("int32_t ") and sig[i] is C.c_int32 for i in scalars)
    assert hasattr(_ffi.load_library(), "tgp_qsep_series_grad")


def test_the_public_names():
    import tinygp_amd
    from tinygp_amd.solvers import QuasisepSeriesSet

    assert callable(tinygp_amd.log_probability_and_grad_series) and hasattr(QuasisepSeriesSet, "value_and_grad")
