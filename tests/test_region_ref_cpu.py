"""CPU: tests/region_ref.py, the numpy restatement the GPU tests of the region statistics compare against, pinned from three sides: a
per-label double loop over the pixels, scipy.ndimage, and cases written out by hand (a tie, an empty row, the quantile rule)."""
import numpy as np
import pytest
from scipy import ndimage

import region_ref as ref


def case(seed, H=23, W=17, top=6, dtype=np.uint8, lo=0, hi=256):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, top + 1, (H, W)).astype(np.int32)
    labels[labels == 2] = 0                                             # label 2 is an empty row
    values = rng.randint(lo, hi, (H, W)).astype(dtype)
    within = rng.rand(H, W) < 0.6
    return labels, values, within, top


def loop_statistics(labels, values, max_label, within):
    """The definition, pixel by pixel in raster order, in Python integers."""
    R = max_label + 1
    count, total, sq = [0] * R, [0] * R, [0] * R
    mn, mx, amin, amax = [0] * R, [0] * R, [-1] * R, [-1] * R
    H, W = labels.shape
    for y in range(H):
        for x in range(W):
            L, v = int(labels[y, x]), int(values[y, x])
            if L < 0 or L > max_label or (within is not None and not within[y, x]):
                continue
            if count[L] == 0 or v < mn[L]:
                mn[L], amin[L] = v, y * W + x
            if count[L] == 0 or v > mx[L]:
                mx[L], amax[L] = v, y * W + x
            count[L] += 1
            total[L] += v
            sq[L] += v * v
    return dict(count=count, sum=total, sumsq=sq, min=mn, max=mx, argmin=amin, argmax=amax)


@pytest.mark.parametrize('dtype,lo,hi', [(np.uint8, 0, 256), (np.uint8, 0, 3), (np.int8, -128, 128), (np.int16, -32768, 32768),
                                         (np.int32, -2 ** 31, 2 ** 31)])
@pytest.mark.parametrize('use_within', [False, True])
def test_statistics_against_the_double_loop(dtype, lo, hi, use_within):
    labels, values, within, top = case(3, dtype=dtype, lo=lo, hi=hi)
    labels[0, 0], labels[5, 5] = -1, top + 3                            # outside [0, max_label]: counted nowhere
    w = within if use_within else None
    got, want = ref.statistics(labels, values, top, w), loop_statistics(labels, values, top, w)
    for name in want:
        if name == 'sumsq' and dtype == np.int32:
            continue
        assert got[name].tolist() == want[name], name
    assert got['count'][2] == 0 and got['argmin'][2] == -1 and got['argmax'][2] == -1 and got['min'][2] == 0 == got['max'][2]
    assert got['sum'].dtype == np.int64 and got['sumsq'].dtype == np.int64 and got['count'].dtype == np.int32
    assert ref.refused(labels, top) == 2


def test_statistics_against_scipy():
    labels, values, within, top = case(5, dtype=np.int16, lo=-300, hi=300)
    index = [L for L in range(top + 1) if (labels == L).any()]
    got = ref.statistics(labels, values, top)
    v64 = values.astype(np.int64)
    assert got['count'][index].tolist() == ndimage.sum(np.ones_like(v64), labels, index).astype(np.int64).tolist()
    assert got['sum'][index].tolist() == ndimage.sum(v64, labels, index).astype(np.int64).tolist()
    assert got['sumsq'][index].tolist() == ndimage.sum(v64 * v64, labels, index).astype(np.int64).tolist()
    assert got['min'][index].tolist() == ndimage.minimum(v64, labels, index).astype(np.int64).tolist()
    assert got['max'][index].tolist() == ndimage.maximum(v64, labels, index).astype(np.int64).tolist()
    W = labels.shape[1]
    assert got['argmin'][index].tolist() == [y * W + x for y, x in ndimage.minimum_position(v64, labels, index)]
    assert got['argmax'][index].tolist() == [y * W + x for y, x in ndimage.maximum_position(v64, labels, index)]


def test_positions_with_many_ties_against_scipy():
    """scipy does not say which of several equal extrema it reports (it sorts); the restatement reports the first in raster order.
    So: scipy's position holds the same value, and none of the region's pixels before ours does."""
    labels, values, within, top = case(9, dtype=np.uint8, lo=0, hi=3)   # three values: every extremum is attained many times
    index = [L for L in range(top + 1) if (labels == L).any()]
    got = ref.statistics(labels, values, top)
    W = labels.shape[1]
    flat_l, flat_v = labels.reshape(-1), values.reshape(-1)
    for name, where in (('min', ndimage.minimum_position(values, labels, index)), ('max', ndimage.maximum_position(values, labels, index))):
        for L, (y, x) in zip(index, where):
            ours = got['arg' + name][L]
            assert values[y, x] == got[name][L] == flat_v[ours] and flat_l[ours] == L and ours <= y * W + x
            assert not ((flat_l[:ours] == L) & (flat_v[:ours] == got[name][L])).any()


@pytest.mark.parametrize('use_within', [False, True])
def test_histogram_against_scipy_and_the_loop(use_within):
    labels, values, within, top = case(7)
    w = within if use_within else None
    got = ref.histogram(labels, values, top, w)
    assert got.shape == (top + 1, 256) and got.dtype == np.int32
    lab = labels if w is None else np.where(w, labels, -1)
    for L in range(top + 1):
        if (lab == L).any():
            assert got[L].tolist() == ndimage.histogram(values, 0, 256, 256, lab, L).tolist()
        else:
            assert not got[L].any()
    want = np.zeros((top + 1, 256), np.int64)
    for y in range(labels.shape[0]):
        for x in range(labels.shape[1]):
            if w is None or w[y, x]:
                want[labels[y, x], values[y, x]] += 1
    assert (got == want).all()
    assert (got.sum(1) == ref.statistics(labels, values, top, w)['count']).all()


def test_quantiles_from_pixels_and_from_histograms_agree():
    labels, values, within, top = case(11)
    qs = [0, 1, 1000, 3333, 4999, 5000, 9999, 10000]
    a = ref.quantiles(labels, values, qs, top, within)
    b = ref.quantiles_of_histogram(ref.histogram(labels, values, top, within), qs)
    assert a.dtype == np.uint8 and (a == b).all()
    st = ref.statistics(labels, values, top, within)
    assert (a[:, 0] == st['min']).all() and (a[:, -1] == st['max']).all()
    assert (a[2] == 0).all()                                            # the empty row


def test_cases_written_out_by_hand():
    labels = np.array([[1, 1, 0, 3],
                       [1, 3, 3, 0],
                       [5, 5, 5, 5]], np.int32)
    values = np.array([[7, 2, 9, 4],
                       [2, 4, 1, 9],
                       [6, 6, 6, 6]], np.int16)
    st = ref.statistics(labels, values, 5)
    assert st['count'].tolist() == [2, 3, 0, 3, 0, 4]
    assert st['sum'].tolist() == [18, 11, 0, 9, 0, 24]
    assert st['sumsq'].tolist() == [162, 57, 0, 33, 0, 144]
    assert st['min'].tolist() == [9, 2, 0, 1, 0, 6] and st['max'].tolist() == [9, 7, 0, 4, 0, 6]
    assert st['argmin'].tolist() == [2, 1, -1, 6, -1, 8]                # label 1: the 2 at index 1, not the one at 4; label 5: constant
    assert st['argmax'].tolist() == [2, 0, -1, 3, -1, 8]                # label 3: the 4 at index 3, not the one at 5; label 0: 9 at 2, not 7
    within = np.array([[0, 1, 1, 1], [1, 1, 1, 0], [0, 0, 2, 0]])
    st = ref.statistics(labels, values, 5, within)
    assert st['count'].tolist() == [1, 2, 0, 3, 0, 1] and st['argmax'].tolist() == [2, 1, -1, 3, -1, 10]
    assert st['sum'].tolist() == [9, 4, 0, 9, 0, 6]
    st = ref.statistics(labels, values, 2)                              # labels 3 and 5 are above max_label
    assert st['count'].tolist() == [2, 3, 0] and ref.refused(labels, 2) == 7
    # the quantile rule (kernels.KernelSpec.rank_filter, item 5): [10, 20] gives 20 at 5000 and 10 at 4999
    assert ref.quantile_of_sorted([10, 20], 5000) == 20 and ref.quantile_of_sorted([10, 20], 4999) == 10
    assert ref.quantile_of_sorted([], 5000) == 0 and ref.quantile_of_sorted([3], 0) == 3 == ref.quantile_of_sorted([3], 10000)
    v = list(range(25))
    assert ref.quantile_of_sorted(v, 2000) == 5 and ref.quantile_of_sorted(v, 1999) == 4 and ref.quantile_of_sorted(v, 10000) == 24
    q = ref.quantiles(labels, values.astype(np.uint8), [0, 5000, 10000], 5)
    assert q.tolist() == [[9, 9, 9], [2, 2, 7], [0, 0, 0], [1, 4, 4], [0, 0, 0], [6, 6, 6]]
    hist = np.zeros((3, 256), np.int64)
    hist[0, 0], hist[0, 255] = 2 ** 31 - 2, 1                           # n = 2^31 - 1: the product n q10k needs more than 32 bits
    hist[1, 255] = 2 ** 31 - 1
    assert ref.quantiles_of_histogram(hist, [0, 9999, 10000]).tolist() == [[0, 0, 255], [255, 255, 255], [0, 0, 0]]


def test_mean_std_two_pass():
    labels, values, within, top = case(13)
    mean, std = ref.mean_std(values, labels, top)
    idx = [L for L in range(top + 1) if (labels == L).any()]
    with np.errstate(invalid='ignore'):                                 # scipy divides by the count of the empty label 2 on its way
        assert np.allclose(mean[idx], ndimage.mean(values.astype(np.float64), labels, idx), rtol=0, atol=1e-10)
        assert np.allclose(std[idx], ndimage.standard_deviation(values.astype(np.float64), labels, idx), rtol=0, atol=1e-10)
    assert mean[2] == 0 and std[2] == 0
    const = np.full_like(values, 77)
    mean, std = ref.mean_std(const, labels, top)
    assert (std == 0).all() and set(mean.tolist()) == {0.0, 77.0}
