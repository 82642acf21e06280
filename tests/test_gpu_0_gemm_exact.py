"""Every form of the MFMA product kernels (gemm.hip) against the exact integer product, tolerance zero.

gemm_nt_kernel (128 x 128 tiles: the fp64 pipeline with its staged C read, the three-stage fp32 pipeline, the short-k path, the
split-k tail, the persistent loop, the counted write-through prefix, the XCD remap, both tile orders) and gemm_nt_small_kernel
(64 x 64 tiles, skip00) are launched through tgp_gemm_nt with the context's test switches; tests/_gemm_exact.py holds the cases,
the operands (small integers: every summation order gives the same bits) and the check, which names the first wrong tile.  The
last group repeats one shape per form with real-valued operands under the derived inner-product bound.
"""
import numpy as np
import pytest

import _gemm_exact as gx
import _lowlevel as ll

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [gx.case_id(c) for c in cases]


@pytest.fixture(scope="module")
def cus():
    from tinygp_amd import _ffi

    return int(_ffi.default_ctx().device_info()["cus"])


def _run(c, cus, repeat=1, read=(), real=False):
    c = gx.resolve(c, cus)
    inp = gx.make_real_inputs(c) if real else gx.make_inputs(c)
    if not real:
        assert gx.magnitude_ok(c, inp)
    runs = ll.gemm_nt_ld(inp.A, inp.B, inp.C0, inp.m, inp.n, inp.k, c.mode, c.lower, gx.options(c, cus), repeat, read)
    return c, inp, runs


def _exact(c, cus, repeat=1, read=()):
    c, inp, runs = _run(c, cus, repeat, read)
    for got, _, err in runs:
        assert err is None, err
        gx.check_exact(c, inp, got)
    return c, inp, runs


@pytest.mark.parametrize("c", gx.group1(), ids=_ids(gx.group1()))
def test_k_tile_edges_128(c, cus):
    """1, 2, 7 k-tiles (not pipelined), the 8 staged ones, one and more behind them; fewer, as many and more than the fp32
    stages; full, lower, clipped and padded shapes; both modes."""
    _exact(c, cus)


@pytest.mark.parametrize("c", gx.group2(), ids=_ids(gx.group2()))
def test_ids_to_tiles(c, cus):
    """The XCD remap and the tile order on the device: every tile once, whatever the count modulo 8 and the band."""
    _exact(c, cus)


@pytest.mark.parametrize("c", gx.group3(), ids=_ids(gx.group3()))
def test_split_tail(c, cus):
    """ROLE 2: the last round's tiles over S k-slices each; twice in a row (counters reset themselves, the workspace carries
    nothing over), the cases in sequence with different S."""
    c = gx.resolve(c, cus)
    nblk = gx.nblk_of(c)
    S = gx.split_factor(nblk, c.k, cus)
    if c.k == 272:
        assert S == 1  # an odd count of k-tiles cannot be split: the plain launch, still exact
    else:
        assert S > 1, (nblk, c.k, cus)
    if cus == 256:
        if c.tm <= 2 and c.k in gx.K_SPLIT:
            assert S == dict(zip(gx.K_SPLIT, (2, 2, 4, 4, 8)))[c.k]
        if c.tm == 14:
            assert S == 4
        if nblk > 2 * cus:
            assert (c.tm, nblk, S) == (32, 528, 2)
    _exact(c, cus, repeat=2)


@pytest.mark.parametrize("c", gx.group4(), ids=_ids(gx.group4()))
def test_persistent_loop(c, cus):
    """A grid of 8 workgroups walks up to three tiles each."""
    nblk = gx.nblk_of(c)
    assert gx.persistent_grid(nblk, gx.options(c, cus)["gemm_reserve"], cus) == min(nblk, 8)
    _exact(c, cus)


@pytest.mark.parametrize("c", gx.group5(), ids=_ids(gx.group5()))
def test_prefix(c, cus):
    """The write-through prefix: exact, and counted once per prefix tile in each of two calls."""
    _, _, runs = _exact(c, cus, repeat=2, read=("gemm_prefix_count",))
    want = gx.tile_count(c.tm, c.prefix // gx.BM, 1)
    assert [r[1]["gemm_prefix_count"] for r in runs] == [want, want]


@pytest.mark.parametrize("c", gx.group5_rejected(), ids=_ids(gx.group5_rejected()))
def test_prefix_rejected_below_128_k_columns(c, cus):
    c, inp, runs = _run(c, cus)
    got, _, err = runs[0]
    assert isinstance(err, ValueError) and "prefix" in str(err)
    np.testing.assert_array_equal(got.view(np.uint64 if c.dtype == "f64" else np.uint32),
                                  inp.C0.view(np.uint64 if c.dtype == "f64" else np.uint32))


@pytest.mark.parametrize("c", gx.group6(), ids=_ids(gx.group6()))
def test_small_kernel_64(c, cus):
    """gemm_nt_small_kernel: fewer, as many and more k-tiles than its stages; roles 3 / 5 leave C[0:128, 0:128] alone."""
    assert gx.tile_of(c) == gx.SM
    _exact(c, cus)


@pytest.mark.parametrize("c", gx.group7(), ids=_ids(gx.group7()))
def test_real_operands(c, cus):
    """Small integers would not show an operand that lost low-order bits on its way: N(0, 1) operands, elementwise within
    (k + 2) u (|A| |B|^T + |C0|)."""
    c, inp, runs = _run(c, cus, real=True)
    got, _, err = runs[0]
    assert err is None, err
    worst = gx.check_real(c, inp, got)
    print(f"{gx.case_id(c)}: worst entry at {worst:.3f} of its bound")
