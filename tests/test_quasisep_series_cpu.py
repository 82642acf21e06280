"""Sets of series on coordinates of their own, host side: validation, the mirrored extent and split rules, the entry
points' declarations, and the pivots of the GPU tests' inputs under the sequential oracle."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _device, _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.solvers.quasisep import check_series, pack_series

import _quasisep_np as o
import _quasisep_series as qs
from _quasisep_cases import CASES
from _quasisep_grad_batch import member, member_noise

ROOT = Path(__file__).resolve().parent.parent


# -- validation ------------------------------------------------------------------------------------------------------------------
def test_an_unsorted_or_empty_member_is_named():
    good = np.arange(5.0)
    with pytest.raises(ValueError, match=r"series 2: .*sorted"):
        check_series([good, good[:3], np.array([0.0, 2.0, 1.0])])
    assert len(check_series([good, np.array([0.0, 2.0, 1.0])], assume_sorted=True)) == 2
    with pytest.raises(ValueError, match=r"series 1 is empty"):
        check_series([good, np.empty(0)])
    with pytest.raises(ValueError, match=r"series 1: .*\(N,\) or \(N, 1\)"):
        check_series([good, np.zeros((4, 2))])
    with pytest.raises(ValueError, match="at least one series"):
        check_series([])
    ts = check_series([good[:, None], good.astype(np.float32)])
    assert all(t.shape == (5,) and t.dtype == np.float64 and t.flags.c_contiguous for t in ts)


def test_wrong_counts_and_lengths_name_the_member():
    k, lengths = q.Matern32(1.0), [3, 2]
    ys, diags = [np.zeros(3), np.ones(2)], [0.1, np.full(2, 0.2)]
    leaves, smap, h, P, noise, resid = pack_series(lengths, k, ys, diags, means=[1.0, np.ones(2)])
    assert leaves.shape == (2, 1, 5) and h.shape == (2, 2) and P.shape == (2, 2, 2) and smap.dtype == np.int32
    assert np.array_equal(noise, [0.1, 0.1, 0.1, 0.2, 0.2]) and np.array_equal(resid, [-1, -1, -1, 0, 0])
    with pytest.raises(ValueError, match=r"kernels must be one kernel or one per series \(2\); got 3"):
        pack_series(lengths, [k, k, k], ys, diags)
    with pytest.raises(ValueError, match=r"ys must hold one entry per series \(2\); got 1"):
        pack_series(lengths, k, ys[:1], diags)
    with pytest.raises(ValueError, match=r"diags must hold one entry per series \(2\); got 3"):
        pack_series(lengths, k, ys, diags + [0.3])
    with pytest.raises(ValueError, match=r"ys\[1\] must have shape \(2,\) for series 1; got \(3,\)"):
        pack_series(lengths, k, [ys[0], np.zeros(3)], diags)
    with pytest.raises(ValueError, match=r"ys\[0\] must have shape \(3,\) for series 0; got \(\)"):
        pack_series(lengths, k, [0.0, ys[1]], diags)
    with pytest.raises(ValueError, match=r"diags\[0\] must have shape \(3,\) or be a scalar for series 0"):
        pack_series(lengths, k, ys, [np.ones(4), 0.1])
    with pytest.raises(ValueError, match=r"means\[1\] .*series 1"):
        pack_series(lengths, k, ys, diags, means=[0.0, np.ones(5)])


def test_structure_mismatch_and_nine_states():
    ys, diags = [np.zeros(3), np.ones(2)], [0.1, 0.2]
    with pytest.raises(ValueError, match=r"kernel 1 .*J = 3.*J = 2"):
        pack_series([3, 2], [q.Matern32(1.0), q.Matern52(1.0)], ys, diags)
    nine = q.Matern52(1.0) + q.Matern52(2.0) + q.Matern52(3.0)
    with pytest.raises(_device.DeviceLimit, match="J = 9"):
        pack_series([3, 2], nine, ys, diags)


def test_a_shared_kernel_is_its_copies():
    k = CASES["m32cos_plus_sho"](q)
    ys, diags = [np.zeros(3), np.ones(2), np.ones(7)], [0.1, 0.2, 0.3]
    a = pack_series([3, 2, 7], k, ys, diags)
    b = pack_series([3, 2, 7], [CASES["m32cos_plus_sho"](q) for _ in range(3)], ys, diags)
    assert all(np.array_equal(x, y) and x.dtype == y.dtype and x.flags.c_contiguous for x, y in zip(a, b))


# -- the mirrored rules ------------------------------------------------------------------------------------------------------------
def test_extents_at_the_rule_s_edges():
    assert qs.extent(1) == qs.Extent(16, 1, (1,))
    assert qs.extent(1024) == qs.Extent(16, 64, (64,))
    assert qs.extent(1025) == qs.Extent(16, 65, (65, 2))
    assert qs.extent(65_536) == qs.Extent(16, 4096, (4096, 64))
    assert qs.extent(65_537) == qs.Extent(32, 2049, (2049, 33))
    assert qs.extent(262_145) == qs.Extent(128, 2049, (2049, 33))
    assert qs.extent(1 << 20) == qs.Extent(256, 4096, (4096, 64))
    assert qs.extent((1 << 20) + 1) == qs.Extent(256, 4097, (4097, 65, 2))


def test_split_worked_examples():
    # a series of 40 points, J = 2: 40 x 6 + 256 x (3 + 3) + 3 x 3 + 3 doubles
    assert qs.need(40, 2) == 240 + 1536 + 9 + 3
    # 2^20 points, J = 8: 12 n + 256 x (4096 + 64 + 2) + 3 x 4096 + 3
    assert qs.need(1 << 20, 8) == 12 * (1 << 20) + 256 * 4162 + 12288 + 3 == 13_660_675
    # the member limit cuts: 65 short series
    assert qs.series_split([40] * 65, 2) == [64, 1]
    assert qs.series_split([40] * 128, 2) == [64, 64] and qs.series_split([40] * 129, 8) == [64, 64, 1]
    # the cap cuts: nine series of 2^20 points with J = 8 take 122.9 M of the 2^27 - 64 x 141 doubles, ten do not fit
    assert 9 * qs.need(1 << 20, 8) <= qs.CAP_DOUBLES - 64 * 141 < 10 * qs.need(1 << 20, 8)
    assert qs.series_split([1 << 20] * 10, 8) == [9, 1]
    assert qs.series_split([1 << 20] * 10, 2) == [10]                      # J = 2: 7.4 M doubles each
    # greedy in the order given: the tenth long series ends the chain, the short one before it still joined it
    assert qs.series_split([1 << 20] * 9 + [40, 1 << 20, 40], 8) == [10, 2]
    assert qs.series_split([40, 1 << 20] * 9 + [1 << 20], 8) == [18, 1]
    # a series that does not fit alone is refused: 12 M points, J = 8 need more than 12 n = 144 M doubles
    assert qs.need(12_000_000, 8) > qs.CAP_DOUBLES and qs.series_split([40, 12_000_000], 8) is None
    assert qs.series_split([40, 12_000_000], 1) == [2]                       # 5 n + work fits


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_three_entry_points():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tgp_hip.h").read_text(), flags=re.S)
    lib = _ffi.load_library()
    for name, nargs, scalars in (("tgp_qsep_series_create", 5, {1: C.c_int32}), ("tgp_qsep_series_destroy", 1, {}),
                                 ("tgp_qsep_series_logprob", 12, {2: C.c_int32, 4: C.c_int32})):
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"include/tgp_hip.h does not declare {name}"
        params = [p.strip() for p in m.group(1).split(",")]
        sig = _ffi.SIGNATURES[name]
        assert len(params) == len(sig) == nargs
        found = {i: (C.c_int32 if p.startswith("int32_t ") else C.c_int64) for i, p in enumerate(params) if "*" not in p}
        assert found == scalars
        for i, ct in scalars.items():
            assert sig[i] is ct, (name, i, params[i])
        assert hasattr(lib, name)


# -- the oracle on the GPU tests' inputs -----------------------------------------------------------------------------------------------
def _pivots(name, n, b, plant=None):
    t, noise, _ = qs.series(n)
    noise = member_noise(noise, b)
    if plant is not None:
        noise[plant] = -10.0
    with np.errstate(invalid="ignore"):  # the planted pivot's square root
        return o.factor(member(CASES, q, name, b), t, noise)[2]


@pytest.mark.parametrize("name", qs.EDGE_CASES)
def test_oracle_pivots_are_positive_on_the_edge_set(name):
    for b, n in enumerate(qs.EDGE_LENGTHS):
        assert np.all(_pivots(name, n, b) > 0), (name, n)


def test_oracle_pivots_of_the_other_sets():
    assert np.all(_pivots(qs.PROBE_CASE, qs.PROBE_LENGTH, 7) > 0)
    for b in range(11):
        n = qs.COMPANY_LENGTHS[b % 4]
        assert np.all(_pivots(qs.PROBE_CASE, n, b) > 0), (n, b)
    for name in qs.MIXED_CASES:
        assert np.all(_pivots(name, 40, 1) > 0)
    for b in range(13):
        assert np.all(_pivots("matern32", 40, b) > 0), b
    # the planted failure: local step 5 is the first non-positive pivot, whatever the member's kernel
    for b in range(3):
        for n in (300, 64):
            assert np.all(_pivots("matern32", n, b) > 0)
        c = _pivots("matern32", 1025, b, plant=5)
        assert np.all(c[:5] > 0) and c[5] < 0
