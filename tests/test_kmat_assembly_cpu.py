"""CPU: tests/_kmat_assembly.py's check has teeth, and its inputs keep an error apart from every bar.

Each way an assembly goes wrong -- a tile with its neighbour's values, a lower tile not written, an upper tile written, the
noise a row off, twice, or missing in the ragged tile, a hole or a stray one in the identity padding, a write beyond rows_out,
the image of another n -- is applied to the image a correct call leaves, and check() must name the tile, the class of the
entry and the kind of damage.  Then, for every input of tests/test_gpu_2_kmat_assembly.py: no two entries of a row or column
of the oracle's matrix agree to 1e-6 (the bars are 4 ulp, 1e-13 and, in fp32, below 1e-5 against the oracle and zero
against the plain form), and the integer family stays exact in fp32."""
import numpy as np
import pytest

import _kmat_assembly as ka

BARS = {ka.VALUE: ("ulp", 4), ka.VALUE_NOISE: ("ulp", 1)}  # the widest fp64 bars of the GPU file but the trigonometric one


def _correct(n, lower, dtype=np.float64, extra=0):
    """(form, want, mask, got) of assemble_lower's form with one tile of padding rows and ld = rows_out + 2."""
    size = ka.round_up(n + 1) + extra
    form = ka.square_padded(n, size, 2, lower=lower)
    K = ka.oracle_matrix(ka.FAST, n)
    want, mask = ka.expected(form, K, ka.noise(n))
    return form, want, mask, ka.render(want, mask, dtype)


def _tile(ti, tj):
    return slice(ti * ka.TILE, (ti + 1) * ka.TILE), slice(tj * ka.TILE, (tj + 1) * ka.TILE)


def _neighbour_tile(n, lower, got, want):
    got[_tile(1, 0)] = want[_tile(1, 1)].astype(got.dtype)
    return (1, 0), "kernel value", "the value is off"


def _lower_tile_left(n, lower, got, want):
    got[_tile(2, 1)] = ka.sentinel(got.dtype)
    return (2, 1), "kernel value", "left as sentinel"


def _upper_tile_written(n, lower, got, want):
    got[_tile(0, 1)] = got[_tile(1, 0)].T
    return (0, 1), "untouched", "sentinel was overwritten"


def _noise_one_row_down(n, lower, got, want):
    k = np.arange(n - 1)
    got[k, k] -= ka.noise(n)[k]
    got[k + 1, k] += ka.noise(n)[k]
    return (0, 0), "kernel value plus noise", "the value is off"


def _noise_twice(n, lower, got, want):
    k = np.arange(n)
    got[k, k] += ka.noise(n)
    return (0, 0), "kernel value plus noise", "the value is off"


def _noise_missing_in_the_ragged_tile(n, lower, got, want):
    k = np.arange(n // ka.TILE * ka.TILE, n)
    got[k, k] -= ka.noise(n)[k]
    return (n // ka.TILE, n // ka.TILE), "kernel value plus noise", "the value is off"


def _padding_one_missing(n, lower, got, want):
    got[n, n] = 0
    return (n // ka.TILE, n // ka.TILE), "padding one", "the value is off"


def _padding_stray_one(n, lower, got, want):
    got[n + 1, n] = 1
    return ((n + 1) // ka.TILE, n // ka.TILE), "padding zero", "the value is off"


def _row_beyond_rows_out(n, lower, got, want):
    rows_out = got.shape[0] - 2
    got[rows_out, 5] = 0
    return (rows_out // ka.TILE, 0), "untouched", "sentinel was overwritten"


MUTATIONS = [_neighbour_tile, _lower_tile_left, _upper_tile_written, _noise_one_row_down, _noise_twice,
             _noise_missing_in_the_ragged_tile, _padding_one_missing, _padding_stray_one, _row_beyond_rows_out]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [False, True], ids=["full", "lower"])
@pytest.mark.parametrize("n", [257, 385])
def test_the_correct_image_passes(n, lower, dtype):
    form, want, mask, got = _correct(n, lower, dtype)
    ka.check(got, want, mask, BARS)
    assert (mask == ka.UNTOUCHED).sum() == 2 * form.cols_out + (sum(range(form.cols_out // ka.TILE)) * ka.TILE ** 2 if lower else 0)
    flat = ka.filled(form, dtype, tail=7)
    body, outside = ka.image_of(flat, form)
    assert body.shape == got.shape and ka.is_sentinel(body).all() and ka.is_sentinel(outside).all() and outside.size == 7


# (a full call writes the upper tiles: that mutation exists for `lower` alone)
MUTATION_CASES = [(n, lower, m) for n in (257, 385) for lower in (False, True) for m in MUTATIONS
                  if lower or m is not _upper_tile_written]


@pytest.mark.parametrize("n,lower,mutate", MUTATION_CASES,
                         ids=[f"{n}-{'lower' if lo else 'full'}-{m.__name__.strip('_')}" for n, lo, m in MUTATION_CASES])
def test_every_mutation_is_caught_and_named(n, lower, mutate):
    form, want, mask, got = _correct(n, lower)
    (ti, tj), cls, what = mutate(n, lower, got, want)
    with pytest.raises(AssertionError) as err:
        ka.check(got, want, mask, BARS, label=str(form))
    msg = str(err.value)
    assert f"first wrong 128x128 tile (i, j) = ({ti}, {tj})," in msg, msg
    assert f"of class '{cls}'" in msg and what in msg, msg
    if what == "the value is off":
        assert "ulp" in msg


@pytest.mark.parametrize("lower", [False, True], ids=["full", "lower"])
@pytest.mark.parametrize("step", [-1, 1])
@pytest.mark.parametrize("n", [257, 385])
def test_the_image_of_another_n_is_caught(n, step, lower):
    """The same buffer shape, the image of n + step in it: the first wrong entry is row min(n, n + step) of column 0 -- a
    kernel value where padding belongs, or padding where a kernel value does."""
    extra = ka.round_up(n + 2) - ka.round_up(n + 1)  # (both n share the padded size)
    form, want, mask, _ = _correct(n, lower, extra=extra)
    other = ka.square_padded(n + step, form.rows_out, 2, lower=lower)
    assert (other.rows_out, other.ld) == (form.rows_out, form.ld)
    got = ka.render(*ka.expected(other, ka.oracle_matrix(ka.FAST, n + step), ka.noise(n + step)), np.float64)
    row = min(n, n + step)
    with pytest.raises(AssertionError) as err:
        ka.check(got, want, mask, BARS)
    msg = str(err.value)
    assert f"first wrong 128x128 tile (i, j) = ({row // ka.TILE}, 0), entry ({row}, 0)" in msg, msg
    assert ("of class 'padding zero'" if step > 0 else "of class 'kernel value'") in msg, msg


def test_one_ulp_on_the_diagonal_and_none_off_it():
    """The bars of the forms against the plain image: zero off the diagonal, one ulp of the long-double sum on it."""
    form, want, mask, got = _correct(257, True)
    bars = {ka.VALUE: ("abs", 0), ka.VALUE_NOISE: ("ulp", 1)}
    ka.check(got, want, mask, bars)
    got[200, 200] = np.nextafter(np.nextafter(got[200, 200], np.inf), np.inf)  # (1.5 ulp or more from the long-double sum)
    with pytest.raises(AssertionError, match=r"tile \(i, j\) = \(1, 1\).*kernel value plus noise"):
        ka.check(got, want, mask, bars)
    form, want, mask, got = _correct(257, True)
    got[250, 5] = np.nextafter(got[250, 5], 0)
    with pytest.raises(AssertionError, match=r"tile \(i, j\) = \(1, 0\), entry \(250, 5\) of class 'kernel value'.*off by 1 ulp"):
        ka.check(got, want, mask, bars)
    ka.check(got, want, mask, BARS)


def test_block_column_form_is_the_rectangle_of_dist_hip():
    f = ka.block_column(385, 256, 256)
    assert (f.n1, f.n2, f.x_off, f.rows_out, f.cols_out, f.ld, f.out_off) == (129, 129, 256, 256, 256, 512, 256)
    want, mask = ka.expected(f, ka.oracle_matrix(ka.FAST, 385), ka.noise(385))
    assert want[0, 0] == np.longdouble(ka.oracle_matrix(ka.FAST, 385)[256, 256]) + np.longdouble(ka.noise(385)[256])
    assert mask[128, 128] == ka.VALUE_NOISE and mask[129, 129] == ka.ONE and mask[129, 128] == ka.ZERO
    assert (mask[:128, 128:] == ka.UNTOUCHED).all() and (mask[256:] == ka.UNTOUCHED).all()
    assert mask[200, 5] == ka.ZERO and mask[128, 0] == ka.VALUE and mask[129, 0] == ka.ZERO


def test_the_kept_lattice_is_the_construction():
    T = ka.build_lattice()
    assert np.array_equal(T, ka.lattice())
    assert (np.diff(T) >= ka.GAP // 2).all() and T[-1] * 2.0 ** -16 <= ka.SPAN
    for n, d in [(ka.LARGE, 1), (257, 16), (129, 5), (1, 1), (1, 3)]:
        assert np.array_equal(ka.points(n, d, np.float32).astype(np.float64), ka.points(n, d))
        assert np.array_equal(ka.noise(n, np.float32).astype(np.float64), ka.noise(n))
    assert (np.diff(ka.noise(1024)) == 2.0 ** -10).all()


@pytest.mark.parametrize("name,n,d", ka.float_inputs(), ids=lambda v: str(v))
def test_no_two_entries_of_a_row_or_column_agree(name, n, d):
    K = ka.oracle_matrix(name, n, d)
    assert K.shape == (n, n) and np.isfinite(K).all() and (K > 1e-3).all() and (K < 20).all()
    assert ka.separation(K) > 1e-6, (name, n, d, ka.separation(K))


@pytest.mark.parametrize("n,d", ka.int_inputs(), ids=lambda v: str(v))
def test_the_integer_family_is_exact_in_both_dtypes(n, d):
    X = ka.int_points(n, d)
    assert np.abs(X).max() <= 3 and np.array_equal(ka.int_points(n, d, np.float32).astype(np.float64), X)
    K, bound = ka.int_matrix(X)
    assert bound < 2 ** 24 and np.abs(K).max() + 7 <= bound
    assert ka.int_noise(n).min() == 1 and ka.int_noise(n).max() <= 7
