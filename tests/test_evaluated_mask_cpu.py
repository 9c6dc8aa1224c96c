"""tolerances.evaluated_mask against the loop of process.cpp:46-52, written out: at odd n the reference's j = (i + n / 2) % n is not
undone by i = (j + n / 2) % n, which the mask used until this module (one bin off at both band edges); at even n nothing changed."""
import numpy as np
import pytest

from tests import tolerances as tol


def _brute(n, use_bandwidth, dc_ignore_bins):
    """process.cpp:46-52 in Python integers (the reference's uint32 arithmetic does not wrap for use_bandwidth <= 1)"""
    half = n // 2
    use_window = int(use_bandwidth * n / 2.0)
    m = np.zeros(n, bool)
    for i in range(n):
        j = (i + half) % n
        if j < dc_ignore_bins or (n - j) < dc_ignore_bins:
            continue
        if i < half - use_window or i > half + use_window:
            continue
        m[j] = True
    return m


def _old(n, use_bandwidth=0.75, dc_ignore_bins=4):
    """the mask as it was: built from j with i = (j + n / 2) % n"""
    half = n // 2
    use_window = int(use_bandwidth * n / 2.0)
    j = np.arange(n)
    i = (j + half) % n
    return ~((j < dc_ignore_bins) | ((n - j) < dc_ignore_bins) | (i < (half - use_window)) | (i > (half + use_window)))


@pytest.mark.parametrize("n", [17, 1023, 4097, 65535])
@pytest.mark.parametrize("bw,dc", [(0.75, 4), (0.75, 0), (1.0, 1), (0.5, 7)])
def test_odd_sizes_follow_the_reference_loop(n, bw, dc):
    m = tol.evaluated_mask(n, bw, dc)
    assert m.dtype == bool and m.shape == (n,)
    assert np.array_equal(m, _brute(n, bw, dc))


def test_the_old_mask_was_one_bin_off_at_odd_sizes():
    for n in (17, 1023, 4097, 65535):
        diff = np.flatnonzero(_old(n) != _brute(n, 0.75, 4))
        assert len(diff) == 2, (n, diff)    # one bin gained at one band edge, one lost at the other: same population


@pytest.mark.parametrize("n", [16, 64, 1000, 1004, 4096, 6000, 65536])
@pytest.mark.parametrize("bw,dc", [(0.75, 4), (0.75, 0), (1.0, 1), (0.5, 7)])
def test_even_sizes_are_unchanged(n, bw, dc):
    m = tol.evaluated_mask(n, bw, dc)
    assert np.array_equal(m, _old(n, bw, dc))
    assert np.array_equal(m, _brute(n, bw, dc))
