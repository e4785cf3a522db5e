"""csrc/np_sums.h and csrc/cube_means.h -- the order of additions that k_grid_reduce, k_cube_spatial, k_cube_temporal
and k_calib_cost share -- run on the host (tests/np_sums_main.cpp, a program of its own built with the host compiler
and -ffp-contract=off) and compared with numpy itself, bit for bit, where numpy changes strategy: below and from 8
terms, at blocks of 128, at halves aligned to 8, at the 8192 elements of its iterator buffer, and at the geometries of
spatial_mean where its iterator merges the two block axes.  No GPU, no tolerance.

np_sum is what equals np.sum at every length.  0.0 + np_pairwise_sum (one pairwise run) equals it up to 8192 terms
only: numpy's reduction hands its pairwise routine at most 8192 elements at a time, so at 8193, 16385 and 100003 terms
np.sum is compared with np_sum, and the single run is not expected to agree there."""
import numpy as np
import pytest

import np_sums_cases as K


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return K.build(tmp_path_factory.mktemp("np_sums"))


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_inputs_tell_numpys_order_from_wrong_ones():
    """A length whose values give the same bits in any order proves nothing: from 16 terms on, np.sum differs from the
    plain left-to-right sum or from the pairwise sum whose halves are not aligned to 8."""
    blind = [n for n in K.SUM_LENGTHS if n >= 16 and not K.tells_orders_apart(K.sum_case(n))]
    assert not blind, blind
    # and the two wrong orders are wrong: each differs from np.sum somewhere
    assert any(K.left_to_right(K.sum_case(n)) != float(np.sum(K.sum_case(n))) for n in (16, 17, 127, 128, 129))
    assert any(float(0.0 + K.unaligned_pairwise(K.sum_case(n))) != float(np.sum(K.sum_case(n))) for n in (129, 130, 135, 137, 143))


def test_contiguous_sums_equal_numpy(exe, tmp_path):
    values = [K.sum_case(n) for n in K.SUM_LENGTHS]
    got, _ = K.run(exe, tmp_path, [("sum", x) for x in values])
    wrong = []
    for n, x, (buffered, one_run) in zip(K.SUM_LENGTHS, values, got):
        want = np.sum(x)
        if bits(buffered) != bits(want) or (n <= 8192 and bits(one_run) != bits(want)):
            wrong.append(n)
        if n <= 8192:
            assert bits(one_run) == bits(np.float64(0.0 + K.one_run_pairwise(x))), n      # the restatement is the routine
    assert not wrong, wrong
    assert all(bits(one_run) != bits(np.sum(x)) for n, x, (_, one_run) in zip(K.SUM_LENGTHS, values, got) if n > 8192)


def test_negative_zero_and_nan_sums(exe, tmp_path):
    cases = [np.full(n, -0.0) for n in (0, 1, 7, 8, 129)] + [np.array([1.0] * 9 + [np.nan]), np.array([np.inf] * 8 + [-np.inf])]
    got, _ = K.run(exe, tmp_path, [("sum", a) for a in cases])
    for a, (buffered, one_run) in zip(cases, got):
        with np.errstate(invalid="ignore"):
            want = np.sum(a)
        if np.isnan(want):
            assert np.isnan(buffered) and np.isnan(one_run)
        else:
            assert bits(buffered) == bits(want) and bits(one_run) == bits(want), a


@pytest.mark.parametrize("nan_share", [0.0, 0.1])
def test_block_means_equal_numpy(exe, tmp_path, nan_share):
    fields = {}
    for rows, cols, c in K.GEOMETRIES:
        if (rows, cols) not in fields:
            fields[(rows, cols)] = K.field(rows, cols, nan_share, 3)
    cases = [("mean", fields[(rows, cols)], c) for rows, cols, c in K.GEOMETRIES]
    got, _ = K.run(exe, tmp_path, cases)
    wrong, nans = [], 0
    for (rows, cols, c), g in zip(K.GEOMETRIES, got):
        want = K.spatial_mean_numpy(fields[(rows, cols)], c)
        assert g.shape == want.shape
        nan = np.isnan(want)
        nans += int(nan.sum())
        if not (np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(want)[~nan])):
            wrong.append((rows, cols, c))
    assert not wrong, wrong
    assert (nans > 0) == (nan_share > 0)


def test_spatial_mean_of_the_package_is_the_reference_used_here():
    from iceberg_tracking_code_amd import postprocess
    a = K.field(23, 5, 0.1, 3)
    for c in (2, 8, 91):
        w, g = K.spatial_mean_numpy(a, c), postprocess.spatial_mean_host(a, c)
        assert np.array_equal(np.isnan(w), np.isnan(g)) and np.array_equal(bits(w)[~np.isnan(w)], bits(g)[~np.isnan(g)])
