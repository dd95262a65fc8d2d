"""GPU: the region statistics (csrc/region.hip; cgc_net_amd.nuclei.region_statistics, region_histogram, region_quantiles,
region_mean_std, ring_labels, stain_features) against tests/region_ref.py, bit for bit, at the smallest shapes at which each mechanism
can fail: tile seams, more labels in a tile than its table holds, colliding labels, one label over many tiles at the ends of every
value type, equal extrema in different tiles and inside one wave's row -- and against the code of the stage that exists."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import region_ref as ref
import stain_ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

FIELDS = ('count', 'sum', 'sumsq', 'min', 'max', 'argmin', 'argmax')
QS = (0, 1000, 5000, 9000, 10000)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def geometry():
    k = kernels.get()
    return k.region_tile, k.region_slots


def check(labels, values, max_label=None, within=None, modes=('moments', 'hist')):
    """Every table of both modes against the restatement; labels, values, within: numpy arrays.  Returns the RegionStats."""
    top = int(labels.max()) if max_label is None and labels.size else (max_label or 0)
    L, V, Wn = gpu(labels), gpu(values), None if within is None else gpu(within)
    st = None
    if 'moments' in modes:
        st = nuclei.region_statistics(L, V, max_label=max_label, within=Wn)
        want = ref.statistics(labels, values, top, within)
        assert (st.sumsq is None) == (values.dtype == np.int32)
        for name in FIELDS:
            got = getattr(st, name)
            if got is None:
                continue
            assert got.dtype == (torch.int64 if name in ('sum', 'sumsq') else torch.int32) and tuple(got.shape) == (top + 1,), name
            assert np.array_equal(got.cpu().numpy(), want[name]), name
    if 'hist' in modes and values.dtype in (np.uint8, np.bool_):
        hist = nuclei.region_histogram(L, V, max_label=max_label, within=Wn)
        assert hist.dtype == torch.int32 and tuple(hist.shape) == (top + 1, 256)
        want = ref.histogram(labels, values, top, within)
        assert np.array_equal(hist.cpu().numpy(), want)
        q = nuclei.region_quantiles(L, V, [Q / 10000 for Q in QS], max_label=max_label, within=Wn)
        assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy(), ref.quantiles_of_histogram(want, QS))
    return st


def random_case(H, W, top, seed, dtype=np.uint8, lo=0, hi=256):
    rng = np.random.RandomState(seed)
    return rng.randint(0, top + 1, (H, W)).astype(np.int32), rng.randint(lo, hi, (H, W)).astype(dtype)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('shape', [(0, 5), (5, 0), (1, 1), (1, 7), (7, 1)])
def test_degenerate_shapes(shape):
    labels, values = random_case(shape[0], shape[1], 3, 1)
    check(labels, values, max_label=3)
    check(labels, values)                                               # the range read from the labels; an empty image has row 0 only
    check(labels, values.astype(np.int32), max_label=3)
    within = np.zeros(shape, bool)
    check(labels, values, max_label=3, within=within)


def test_max_label_zero_and_far_above_the_largest():
    t, S = geometry()
    labels, values = random_case(t + 3, 9, 0, 2)
    st = check(labels, values, max_label=0)
    assert st.count.tolist() == [labels.size]
    labels, values = random_case(t + 3, 9, 4, 3)
    st = check(labels, values, max_label=5000)                          # rows 5 .. 5000 are empty
    assert int(st.count[5:].sum()) == 0 and (st.argmin[5:] == -1).all() and (st.argmax[5:] == -1).all()
    assert int(st.min[5:].abs().sum() + st.max[5:].abs().sum() + st.sum[5:].abs().sum() + st.sumsq[5:].abs().sum()) == 0


def test_tile_seams():
    t, S = geometry()
    labels, values = random_case(t + 3, 2 * t + 5, 5, 4)
    check(labels, values)
    labels = np.zeros((2 * t + 1, 2 * t + 1), np.int32)
    labels[t:2 * t, t:2 * t] = 3                                        # one full tile exactly
    labels[-1, :] = 7                                                   # only on the image's last row ...
    labels[:, -1] = 7                                                   # ... and last column
    values = np.random.RandomState(5).randint(0, 256, labels.shape).astype(np.uint8)
    st = check(labels, values)
    assert int(st.count[3]) == t * t and int(st.count[7]) == 4 * t + 1


# ------------------------------------------------------------------ more labels than the table holds
@pytest.mark.parametrize('dtype', [np.uint8, np.int32])
def test_every_pixel_its_own_label(dtype):
    t, S = geometry()
    n = t + 6
    labels = np.random.RandomState(6).permutation(n * n).astype(np.int32).reshape(n, n)
    values = np.random.RandomState(7).randint(0, 256, (n, n)).astype(dtype)
    st = check(labels, values)
    assert (st.count == 1).all() and np.array_equal(st.argmin.cpu().numpy()[labels.reshape(-1)], np.arange(n * n))


def test_the_direct_route_with_within_on_partial_tiles():
    t, S = geometry()
    n = t + 6                                                           # four tiles, three of them partial; 64 labels of each fold
    labels = np.random.RandomState(6).permutation(n * n).astype(np.int32).reshape(n, n)
    values = np.random.RandomState(7).randint(0, 256, (n, n)).astype(np.uint8)
    within = (np.indices((n, n)).sum(0) % 2).astype(np.int16)           # a checkerboard
    st = check(labels, values, within=within)
    assert np.array_equal(st.count.cpu().numpy()[labels.reshape(-1)], within.reshape(-1))


@pytest.mark.parametrize('extra', [0, 1])
def test_exactly_as_many_labels_as_slots_and_one_more(extra):
    t, S = geometry()
    rng = np.random.RandomState(8 + extra)
    labels = rng.randint(0, S + extra, (t, t)).astype(np.int32)
    labels.reshape(-1)[:S + extra] = np.arange(S + extra)               # every label is there
    values = rng.randint(0, 256, (t, t)).astype(np.uint8)
    st = check(labels, values)
    assert (st.count > 0).all() and st.count.numel() == S + extra
    check(labels, values.astype(np.int16) * 100 - 12000)


@pytest.mark.parametrize('stride', ['S', '2S', 'sparse'])
def test_colliding_and_sparse_labels(stride):
    t, S = geometry()
    rng = np.random.RandomState(10)
    if stride == 'sparse':
        ids = np.unique(np.concatenate([rng.randint(0, 2 ** 17, 90), [2 ** 17]])).astype(np.int32)
    else:
        ids = (np.arange(40) * (S if stride == 'S' else 2 * S) + 5).astype(np.int32)      # congruent modulo S (2 S)
    labels = ids[rng.randint(0, len(ids), (t + 9, t + 2))]
    labels[::7] = ids[1]                                                # and long runs of one of them
    labels[1, 0] = ids[-1]                                              # the largest id is there
    values = rng.randint(0, 256, labels.shape).astype(np.uint8)
    within = rng.rand(*labels.shape) < 0.5
    if stride != 'sparse':
        check(labels, values)
        check(labels, values, within=within)
        return
    # a table of 2^17 + 1 rows: the moments whole; of the histograms the rows of the ids, and that no other row holds anything
    check(labels, values, modes=('moments',))
    check(labels, values, within=within, modes=('moments',))
    hist = nuclei.region_histogram(gpu(labels), gpu(values), within=gpu(within))
    assert tuple(hist.shape) == (2 ** 17 + 1, 256) and int(hist.sum()) == int(within.sum())
    compact = np.searchsorted(ids, labels).astype(np.int32)
    assert np.array_equal(hist[gpu(ids).long()].cpu().numpy(), ref.histogram(compact, values, len(ids) - 1, within))


# ------------------------------------------------------------------ one label over 3 x 3 tiles, at the ends of the value types
@pytest.mark.parametrize('dtype,value', [(np.uint8, 255), (np.int32, INT32_MAX), (np.int32, INT32_MIN), (np.int16, -32768), (np.int8, -128),
                                         (np.uint8, 77)])
def test_one_label_one_value_over_nine_tiles(dtype, value):
    t, S = geometry()
    n = 2 * t + 2
    labels = np.full((n, n), 2, np.int32)
    values = np.full((n, n), value, dtype)
    st = check(labels, values)
    assert st.count.tolist() == [0, 0, n * n] and st.sum.tolist() == [0, 0, n * n * value]
    if dtype != np.int32:
        assert st.sumsq.tolist() == [0, 0, n * n * value * value]
    assert st.min.tolist() == [0, 0, value] == st.max.tolist()
    assert st.argmin.tolist() == [-1, -1, 0] == st.argmax.tolist()      # a constant plane: the region's first pixel
    if dtype == np.uint8:
        hist = nuclei.region_histogram(gpu(labels), gpu(values))
        assert int(hist[2, value]) == n * n and int(hist.sum()) == n * n  # 16-bit partial counts of a tile did not wrap


def test_a_constant_plane_gives_the_first_pixel_of_every_region():
    t, S = geometry()
    labels, _ = random_case(t + 5, t + 7, 4, 11)
    labels[0, :3] = 4
    st = check(labels, np.full(labels.shape, -9, np.int16))
    first = [int(np.flatnonzero(labels.reshape(-1) == L)[0]) for L in range(5)]
    assert st.argmin.tolist() == first == st.argmax.tolist()


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize('dtype', [np.uint8, np.int16, np.int32])
def test_ties_across_tiles_and_inside_a_row(dtype):
    t, S = geometry()
    H, W = 2 * t + 3, 2 * t + 3
    labels = np.ones((H, W), np.int32)
    labels[:, W // 2:] = 2
    info = np.iinfo(dtype)
    values = np.random.RandomState(12).randint(10, 100, (H, W)).astype(dtype)
    # label 1: the extrema twice in one row of one tile (one wave sees both), and again in the tile below
    for y, x in ((5, 40), (5, 9), (t + 4, 3)):
        values[y, x] = info.max
    for y, x in ((7, 50), (7, 20), (t + 9, 1)):
        values[y, x] = info.min
    # label 2: in two different tiles of the same tile row, and in a later tile row at a smaller column
    for y, x in ((t + 2, 2 * t + 1), (t + 2, t + 5), (2 * t + 1, W // 2)):
        values[y, x] = info.max
    for y, x in ((3, 2 * t + 2), (3, t + 20), (t + 30, W // 2)):
        values[y, x] = info.min
    st = check(labels, values)
    assert st.argmax.tolist() == [-1, 5 * W + 9, (t + 2) * W + t + 5] and st.argmin.tolist() == [-1, 7 * W + 20, 3 * W + t + 20]
    assert st.max.tolist() == [0, info.max, info.max] and st.min.tolist() == [0, info.min, info.min]


# ------------------------------------------------------------------ dtypes, strides, within
@pytest.mark.parametrize('vdtype,lo,hi', [(np.bool_, 0, 2), (np.uint8, 0, 256), (np.int8, -128, 128), (np.int16, -32768, 32768),
                                          (np.int32, INT32_MIN, INT32_MAX + 1)])
def test_every_value_dtype(vdtype, lo, hi):
    t, S = geometry()
    labels, values = random_case(t + 11, t + 20, 9, 13, np.int64, lo, hi)
    values = values.astype(vdtype)
    L, V = gpu(labels), gpu(values)
    st = nuclei.region_statistics(L, V)
    want = ref.statistics(labels, values.astype(np.int64), 9)
    for name in FIELDS:
        if getattr(st, name) is not None:
            assert np.array_equal(getattr(st, name).cpu().numpy(), want[name]), name
    assert (st.sumsq is None) == (vdtype == np.int32)
    if vdtype in (np.bool_, np.uint8):
        assert np.array_equal(nuclei.region_histogram(L, V).cpu().numpy(), ref.histogram(labels, values.astype(np.uint8), 9))


@pytest.mark.parametrize('ldtype', [torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64])
def test_every_label_dtype(ldtype):
    t, S = geometry()
    labels, values = random_case(t + 2, t + 2, 100, 14)
    st = nuclei.region_statistics(gpu(labels).to(ldtype), gpu(values), max_label=100)
    want = ref.statistics(labels, values, 100)
    for name in FIELDS:
        assert np.array_equal(getattr(st, name).cpu().numpy(), want[name]), name
    q = nuclei.region_quantiles(gpu(labels).to(ldtype), gpu(values), 0.5)
    assert tuple(q.shape) == (101,) and np.array_equal(q.cpu().numpy(), ref.quantiles(labels, values, [5000], 100)[:, 0])


def test_labels_that_do_not_fit_int32_are_refused_not_wrapped():
    labels = torch.ones(4, 5, dtype=torch.int64, device=DEV)
    labels[1, 1] = 2 ** 32 + 1                                          # would be label 1 after a narrowing cast
    with pytest.raises(ValueError, match='outside'):
        nuclei.region_statistics(labels, torch.ones(4, 5, dtype=torch.uint8, device=DEV), max_label=3)


@pytest.mark.parametrize('view', ['steps', 'transpose'])
def test_non_contiguous_views_of_all_three_inputs(view):
    t, S = geometry()
    rng = np.random.RandomState(15)
    H, W = (2 * (t + 5), 3 * (t + 9) + 1) if view == 'steps' else (t + 9, t + 5)
    big = [rng.randint(0, 7, (H, W)).astype(np.int32), rng.randint(0, 256, (H, W)).astype(np.uint8), (rng.rand(H, W) < 0.6).astype(np.int64)]
    cut = (lambda a: a[::2, 1::3]) if view == 'steps' else (lambda a: a.T)
    L, V, Wn = (cut(gpu(a)) for a in big)
    assert not L.is_contiguous() and not V.is_contiguous() and not Wn.is_contiguous()
    labels, values, within = (np.ascontiguousarray(cut(a)) for a in big)
    st = nuclei.region_statistics(L, V, within=Wn, max_label=6)
    want = ref.statistics(labels, values, 6, within)
    for name in FIELDS:
        assert np.array_equal(getattr(st, name).cpu().numpy(), want[name]), name
    assert np.array_equal(nuclei.region_histogram(L, V, within=Wn, max_label=6).cpu().numpy(), ref.histogram(labels, values, 6, within))
    assert np.array_equal(nuclei.region_quantiles(L, V, (0.1, 0.9), within=Wn, max_label=6).cpu().numpy(),
                          ref.quantiles(labels, values, [1000, 9000], 6, within))


def test_within_as_bool_as_strided_int64_and_selecting_nothing():
    t, S = geometry()
    labels, values = random_case(t + 7, t + 1, 6, 16)
    rng = np.random.RandomState(17)
    within = rng.rand(*labels.shape) < 0.4
    check(labels, values, within=within)
    check(labels, values.astype(np.int16) - 77, within=within)
    wide = np.zeros((labels.shape[0], 2 * labels.shape[1]), np.int64)
    wide[:, ::2] = np.where(within, rng.randint(1, 2 ** 40, labels.shape) * rng.choice([-1, 1], labels.shape), 0)
    Wn = gpu(wide)[:, ::2]
    assert not Wn.is_contiguous()
    st = nuclei.region_statistics(gpu(labels), gpu(values), within=Wn)
    want = ref.statistics(labels, values, 6, within)
    for name in FIELDS:
        assert np.array_equal(getattr(st, name).cpu().numpy(), want[name]), name
    st = check(labels, values, within=np.zeros(labels.shape, bool))
    assert int(st.count.sum()) == 0 and (st.argmin == -1).all()


# ------------------------------------------------------------------ refusals that need the device
def test_labels_outside_the_range_raise():
    t, S = geometry()
    labels, values = random_case(t + 3, t + 3, 5, 18)
    L, V = gpu(labels), gpu(values)
    for fn in (nuclei.region_statistics, nuclei.region_histogram, lambda *a, **k: nuclei.region_quantiles(a[0], a[1], 0.5, **k)):
        with pytest.raises(ValueError, match='outside'):
            fn(L, V, max_label=4)                                       # label 5 is above max_label
        bad = L.clone()
        bad[t + 1, t + 2] = -3
        with pytest.raises(ValueError, match='outside'):
            fn(bad, V, max_label=5)
        with pytest.raises(ValueError, match='negative'):
            fn(bad, V)
        # ... whatever `within` says at that pixel
        with pytest.raises(ValueError, match='outside'):
            fn(bad, V, max_label=5, within=torch.zeros_like(L))
    # the library counts them: meta is the number of refused pixels, and the rest is still exact
    tables, meta = kernels.get().region_statistics(L, V, 4)
    assert int(meta) == int((labels == 5).sum()) == ref.refused(labels, 4)
    assert np.array_equal(tables[0].cpu().numpy(), ref.statistics(labels, values, 4)['count'])


# ------------------------------------------------------------------ QUANTILES on histograms made by hand
def test_quantiles_of_hand_made_histograms():
    k = kernels.get()
    hist = np.zeros((9, 256), np.int64)
    hist[1, 200] = 1                                                    # n = 1
    hist[2, 0] = 12345                                                  # all mass in bin 0
    hist[3, 255] = 999                                                  # ... in bin 255
    hist[4, 255] = INT32_MAX                                            # n q10k passes 2^32
    hist[5, 0], hist[5, 255] = INT32_MAX - 1, 1
    hist[6, 3], hist[6, 4], hist[6, 250] = 2 ** 30, 2 ** 30 - 7, 6
    hist[7] = np.random.RandomState(19).randint(0, 2 ** 22, 256)
    hist[8, 10], hist[8, 20] = 1, 1                                     # [10, 20]: 20 at 5000, 10 at 4999
    qs = [0, 1, 4999, 5000, 9999, 10000]
    got = k.region_quantiles(gpu(hist.astype(np.int32)), qs)
    want = ref.quantiles_of_histogram(hist, qs)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert want[0].tolist() == [0] * 6 and want[4].tolist() == [255] * 6 and want[5].tolist() == [0, 0, 0, 0, 0, 255]
    assert want[8].tolist() == [10, 10, 10, 20, 20, 20]
    for n in range(1, 9):                                               # every number of quantiles; rows beyond a block of four
        sub = qs[:n] if n <= 6 else qs + [2500, 7500][:n - 6]
        assert np.array_equal(k.region_quantiles(gpu(hist.astype(np.int32)), sub).cpu().numpy(), ref.quantiles_of_histogram(hist, sub))
    assert tuple(k.region_quantiles(torch.zeros(0, 256, dtype=torch.int32, device=DEV), [5000]).shape) == (0, 1)


# ------------------------------------------------------------------ against the code of the stage that exists
@functools.lru_cache(maxsize=None)
def tissue():
    labels, gray = nuclei.synthetic_tissue(300, 400, 120)
    return labels, gray


def test_tissue_against_the_restatement_and_the_extreme_quantiles():
    labels, gray = tissue()
    st = check(labels, gray)
    q = nuclei.region_quantiles(gpu(labels), gpu(gray), [0, 1])
    assert torch.equal(q[:, 0].to(torch.int32), st.min) and torch.equal(q[:, 1].to(torch.int32), st.max)
    st2 = nuclei.region_statistics(gpu(labels), gpu(gray))              # two calls: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(st, st2))
    h1, h2 = nuclei.region_histogram(gpu(labels), gpu(gray)), nuclei.region_histogram(gpu(labels), gpu(gray))
    assert torch.equal(h1, h2)


def test_count_is_the_sizes_of_label_instances():
    labels, gray = tissue()
    L, n, sizes = nuclei.label_instances(gpu(labels), return_sizes=True)
    st = nuclei.region_statistics(L, gpu(gray), max_label=n)
    assert torch.equal(st.count[1:], sizes) and int(st.count[0]) == int((labels == 0).sum())


def test_histogram_rows_are_the_masked_histograms():
    labels, gray = tissue()
    L, G = gpu(labels), gpu(gray)
    hist = nuclei.region_histogram(L, G)
    present = np.unique(labels)
    for lab in (0, int(present[1]), int(present[-1])):
        assert torch.equal(hist[lab].to(torch.int64), nuclei.histogram(G, within=L == lab))
    assert torch.equal(hist.sum(0).to(torch.int64), nuclei.histogram(G))


def test_the_median_of_one_label_is_the_median_of_a_window_that_covers_the_image():
    rng = np.random.RandomState(20)
    gray = rng.randint(0, 256, (40, 50)).astype(np.uint8)
    G = gpu(gray)
    q = nuclei.region_quantiles(torch.zeros(40, 50, dtype=torch.int32, device=DEV), G, 0.5)
    assert tuple(q.shape) == (1,) and int(q[0]) == int(nuclei.median(G, 63, 'square')[20, 25]) == int(np.sort(gray.reshape(-1))[1000])


def test_the_inscribed_radius_of_a_disc():
    yy, xx = np.mgrid[0:90, 0:100]
    labels = (((yy - 40) ** 2 + (xx - 70) ** 2 <= 15 ** 2) * 3).astype(np.int32)
    L = gpu(labels)
    dist2 = nuclei.distance_transform(L != 0)                           # the sites are the zero pixels: the background
    st = nuclei.region_statistics(L, dist2)
    inside = np.where(labels == 3, dist2.cpu().numpy(), -1).reshape(-1)
    assert int(st.max[3]) == inside.max() >= 15 ** 2 and int(st.argmax[3]) == int(np.flatnonzero(inside == inside.max())[0])
    assert int(st.argmax[3]) == 40 * 100 + 70 and int(st.max[0]) == 0    # the centre of the disc; the background is its own site


# ------------------------------------------------------------------ float columns
TOL = 255 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def stained():
    labels, tile, _ = stain_ref.tile_case()
    noise = np.random.RandomState(21).randint(-25, 26, tile.shape)
    tile = np.clip(tile.astype(np.int64) + noise, 1, 255).astype(np.uint8)
    return labels.copy(), tile                                          # the shared case is read-only; torch wants writable memory


def test_mean_std_within_the_rounding_of_float32():
    """Bound 255 * 2^-23.  The outputs are float32 roundings of numbers in [0, 255]: at most half an ulp of 255, 255 * 2^-24.  The
    float64 formula adds sqrt-amplified cancellation: var carries at most ~4 ulp64 of sumsq / n <= 65025, i.e. 3e-11, and a non-zero
    variance of integers is at least 1 / n^2 >= 1e-10 for n < 1e5, so std moves by at most 3e-11 / (2 * 1e-5) < 1e-5 < 255 * 2^-24."""
    labels, gray = tissue()
    for values in (gray, (gray.astype(np.int16) - 128) * 200, gray.astype(np.int8)):
        st = nuclei.region_statistics(gpu(labels), gpu(values))
        mean, std = nuclei.region_mean_std(st)
        assert mean.dtype == std.dtype == torch.float32
        wm, ws = ref.mean_std(values, labels, int(labels.max()))
        scale = max(1.0, float(np.abs(values.astype(np.float64)).max()) / 255)      # the bound is stated for a uint8 plane
        assert np.abs(mean.cpu().numpy().astype(np.float64) - wm).max() <= TOL * scale
        assert np.abs(std.cpu().numpy().astype(np.float64) - ws).max() <= TOL * scale
    st = nuclei.region_statistics(gpu(labels), gpu(np.full(labels.shape, 201, np.uint8)))
    mean, std = nuclei.region_mean_std(st)
    assert (std == 0).all() and set(mean.tolist()) <= {0.0, 201.0}      # a constant region: std exactly 0


@pytest.mark.parametrize('ring', [0, 6])
def test_stain_features_against_two_pass_numpy(ring):
    """Mean and std columns within 255 * 2^-23 of a float64 two-pass computation over the integer planes of separate_stains (derivation:
    test_mean_std_within_the_rounding_of_float32); median and range columns exact."""
    labels, tile = stained()
    L, T = gpu(labels), gpu(tile)
    top = int(labels.max())
    kept = torch.from_numpy(np.unique(labels[labels > 0]).astype(np.int32)).to(DEV)
    feats = nuclei.stain_features(L, T, kept, ring=ring, max_label=top)
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (kept.numel(), 16 if ring else 8)
    assert torch.equal(feats, nuclei.stain_features(L, T, kept, ring=ring))      # the range read from the labels; bit-identical
    planes = nuclei.separate_stains(T, planes=(0, 1)).cpu().numpy()
    regions = [labels]
    if ring:
        R = nuclei.ring_labels(L, ring)
        rings = R.cpu().numpy()
        assert not ((rings != 0) & (labels != 0)).any()                 # no ring pixel lies inside a nucleus
        assert set(np.unique(rings).tolist()) <= set(np.unique(labels).tolist())      # every ring label is one of the mask's
        assert (rings != 0).any() and R.dtype == L.dtype
        grown = nuclei.expand_labels(L, ring).cpu().numpy()
        assert np.array_equal(rings, np.where(labels != 0, 0, grown))
        regions.append(rings)
    got = feats.cpu().numpy().astype(np.float64)
    rows = kept.cpu().numpy()
    col = 0
    for reg in regions:
        for plane in planes:
            mean, std = ref.mean_std(plane, reg, top)
            q = ref.quantiles(reg, plane, [1000, 5000, 9000], top).astype(np.float64)
            assert np.abs(got[:, col] - mean[rows]).max() <= TOL and np.abs(got[:, col + 1] - std[rows]).max() <= TOL
            assert np.array_equal(got[:, col + 2], q[rows, 1]) and np.array_equal(got[:, col + 3], q[rows, 2] - q[rows, 0])
            col += 4
    assert got[:, :8].std(axis=0).min() > 0                             # the columns say something
    # row k describes kept_labels[k]: a permuted, shorter selection gives the same rows
    pick = torch.flip(kept, [0])[::3]
    assert torch.equal(nuclei.stain_features(L, T, pick.to(torch.int64), ring=ring, max_label=top), torch.flip(feats, [0])[::3])


def test_stain_features_refuses_kept_labels_out_of_range():
    labels, tile = stained()
    L, T = gpu(labels), gpu(tile)
    top = int(labels.max())
    for bad in ([1, top + 1], [-1, 2], [2 ** 31 - 1]):
        with pytest.raises(ValueError, match='kept_labels'):
            nuclei.stain_features(L, T, torch.tensor(bad, dtype=torch.int32, device=DEV), max_label=top)
    with pytest.raises(ValueError, match='outside'):
        nuclei.stain_features(L, T, torch.tensor([1], dtype=torch.int32, device=DEV), max_label=top - 1)
    assert tuple(nuclei.stain_features(L, T, torch.zeros(0, dtype=torch.int32, device=DEV), max_label=top).shape) == (0, 8)


def test_tile_to_node_table():
    """The lines of the module docstring, end to end."""
    labels, tile = stained()
    T = gpu(tile)
    L, n = nuclei.label_instances(gpu(labels) > 0)
    gray = nuclei.bgr_to_gray(T)
    features, cen, kept = nuclei.nucleus_features(L, gray, max_label=n)
    x = torch.cat([features, nuclei.stain_features(L, T, kept, ring=6, max_label=n)], 1)
    assert tuple(x.shape) == (kept.numel(), 32) and bool(torch.isfinite(x).all())
    item = nuclei.graph_item(x, cen, 1)
    assert tuple(item.x.shape) == (kept.numel(), 34)
