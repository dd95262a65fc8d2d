"""Rank filters on the GPU (csrc/rank.hip through cgc_net_amd.nuclei.rank_filter / median / quantile_range / local_entropy) against
tests/rank_ref.py (a numpy restatement, pinned by tests/test_rank_ref_cpu.py), and against the GPU's own flat morphology, window
sums and nucleus features.  Every comparison but the last is exact.

A workgroup owns a tile of ``rank_tile_rows`` (8) rows by ``rank_tile_cols(r)`` (256 - 2 * (r rounded up to 4), 128..256) columns;
inside it a wave slides a histogram along a row and stores its results 64 pixels at a time.  The shapes put footprints across every
tile edge, make r larger than both sides and the halo larger than the image, and make rows end inside a group of 64; the radii
0, 1, 2, 3, 7, 31, 63 use one pass (2 r + 1 <= 64 footprint rows) and two passes of the slide."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import rank_ref as ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

TOP = kernels.RANK_MAX_RADIUS
ETOP = kernels.ENTROPY_MAX_RADIUS
SHAPES = [(1, 1), (1, 300), (300, 1), (5, 9), (64, 64), (65, 63), (67, 131)]
RADII = [0, 1, 2, 3, 7, 31, TOP]
ENTROPY_RADII = [0, 1, 3, 7, ETOP]
KINDS = ['square', 'disk', 'diamond']
QS = [0, 1, 1999, 2000, 2500, 5000, 7500, 9999, 10000]
RANGE = (2500, 7500)
ids = dict(ids=lambda s: '%dx%d' % s)


def frac(q10k):
    return Fraction(q10k, 10000)


def tile_shape(r):
    """Two tiles and a bit in each direction at radius r, neither side a multiple of the tile or of 4."""
    k = kernels.get()
    H, W = 2 * k.rank_tile_rows + 3, 2 * k.rank_tile_cols(r) + 5
    assert H % k.rank_tile_rows and W % k.rank_tile_cols(r) and H % 4 and W % 4
    return H, W


@functools.lru_cache(maxsize=None)
def content(shape, kind):
    """A shared, write-protected image."""
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    if kind == 'random':
        a = np.random.RandomState(shape[0] * 7 + shape[1]).randint(0, 256, shape).astype(np.uint8)
    elif kind == 'few':                                                 # four levels: ties everywhere
        a = (np.random.RandomState(shape[0] * 5 + shape[1]).randint(0, 4, shape) * 85).astype(np.uint8)
    elif kind == 'checker':
        a = (((yy + xx) & 1) * 255).astype(np.uint8)
    elif kind == 'ramp':
        a = ((xx + 0 * yy) & 255).astype(np.uint8)
    else:
        a = np.full(shape, 255 if kind == 'full' else 0, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def selection(shape):
    w = np.random.RandomState(shape[0] * 3 + shape[1] + 1).rand(*shape) < 0.6
    w.setflags(write=False)
    return w


def results(image, kind, r, within=None, qs=QS):
    """Everything the reference says about one image, footprint and selection: {q10k: uint8, 'range': uint8, 'h16': int32 or None}."""
    cum = ref.cumulative(image, kind, r, within)
    out = {q: ref.quantile_of(cum, q).astype(np.uint8) for q in set(qs) | set(RANGE)}
    out['range'] = out[RANGE[1]] - out[RANGE[0]]
    out['h16'] = ref.h16_of(cum) if r <= ETOP else None
    return out


@functools.lru_cache(maxsize=None)
def want(shape, kind_of_content, kind, r, selected):
    """The reference results of a shared image, computed once."""
    return results(content(shape, kind_of_content), kind, r, selection(shape) if selected else None)


def formed(out, like, dtype=torch.uint8):
    assert out.dtype == dtype and tuple(out.shape) == tuple(like.shape) and out.is_contiguous() and out.device == like.device
    return out.cpu().numpy()


def compare(exp, it, kind, r, wt=None, qs=QS, note=''):
    """Every quantile of qs, the range and, where the radius allows, the entropy of the tensor `it` against the reference's `exp`."""
    for q in qs:
        got = formed(nuclei.rank_filter(it, r, frac(q), kind, wt), it)
        assert np.array_equal(got, exp[q]), (note, kind, r, q, np.argwhere(got != exp[q])[:5])
    got = formed(nuclei.quantile_range(it, r, frac(RANGE[0]), frac(RANGE[1]), kind, wt), it)
    assert np.array_equal(got, exp['range']), (note, kind, r, 'range', np.argwhere(got != exp['range'])[:5])
    if r <= ETOP:
        got = formed(nuclei.local_entropy(it, r, kind, wt, raw=True), it, torch.int32)
        assert np.array_equal(got, exp['h16']), (note, kind, r, 'entropy', np.argwhere(got != exp['h16'])[:5])
        as_float = formed(nuclei.local_entropy(it, r, kind, wt), it, torch.float32)
        assert np.array_equal(as_float, exp['h16'].astype(np.float32) / np.float32(65536))


def check(image, kind, r, image_t=None, within=None, within_t=None, qs=(0, 5000, 10000)):
    it = gpu(np.array(image)) if image_t is None else image_t
    wt = within_t if within_t is not None else None if within is None else gpu(np.array(within))
    compare(results(image, kind, r, within, qs), it, kind, r, wt, qs)


# ------------------------------------------------------------------ every shape, radius, footprint
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_every_radius(shape, kind):
    it = gpu(np.array(content(shape, 'random')))
    wt = gpu(np.array(selection(shape)))
    for r in sorted(set(RADII + ENTROPY_RADII)):
        if r >= 31 and shape == (67, 131):                              # large radii stay off the largest shape
            continue
        compare(want(shape, 'random', kind, r, False), it, kind, r, note=shape)
        compare(want(shape, 'random', kind, r, True), it, kind, r, wt, note=(shape, 'within'))


@pytest.mark.parametrize('fill', ['zeros', 'full'])
def test_constant_images_fill_one_bin(fill):
    shape = (129, 131)                                                  # one whole square of r = 63: a bin of 16129
    it = gpu(np.array(content(shape, fill)))
    value = 255 if fill == 'full' else 0
    assert min(shape) >= 2 * TOP + 1 and (2 * TOP + 1) ** 2 == 16129
    for kind, r in (('square', TOP), ('disk', TOP), ('square', 1), ('diamond', 3), ('square', ETOP)):
        compare(want(shape, fill, kind, r, False), it, kind, r, qs=(0, 5000, 10000), note=fill)
        assert (formed(nuclei.median(it, r, kind), it) == value).all()
        assert not formed(nuclei.quantile_range(it, r, 0, 1, kind), it).any()
    assert not formed(nuclei.local_entropy(it, ETOP, 'square', raw=True), it, torch.int32).any()


@pytest.mark.parametrize('fill', ['checker', 'ramp', 'few'])
def test_checkerboards_ramps_and_ties(fill):
    # on a 0 / 255 checkerboard the rank falls on the boundary between the two values: > against >=
    for shape, r in ((tile_shape(1), 1), (tile_shape(2), 2), (tile_shape(3), 3), (tile_shape(7), 7), ((65, 63), 31)):
        it = gpu(np.array(content(shape, fill)))
        wt = gpu(np.array(selection(shape)))
        for kind in KINDS:
            compare(want(shape, fill, kind, r, False), it, kind, r, note=(fill, shape))
        compare(want(shape, fill, 'disk', r, True), it, 'disk', r, wt, note=(fill, shape, 'within'))
    if fill == 'checker':
        it = gpu(np.array(content((9, 9), fill)))
        got = formed(nuclei.median(it, 1, 'square'), it)
        assert got[4, 4] == 0 and got[4, 5] == 255                      # 5 of 9 are 0 around an even pixel, 5 of 9 are 255 around an odd one
        got = formed(nuclei.median(it, 1, 'disk'), it)
        assert got[4, 4] == 255 and got[4, 5] == 0                      # the centre against its four neighbours


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('r', [1, 7, ETOP, 31, TOP])
def test_footprints_across_every_tile_edge(kind, r):
    shape = tile_shape(r)
    rows, cols = kernels.get().rank_tile_rows, kernels.get().rank_tile_cols(r)
    compare(want(shape, 'random', kind, r, False), gpu(np.array(content(shape, 'random'))), kind, r)
    compare(want(shape, 'random', kind, r, True), gpu(np.array(content(shape, 'random'))), kind, r, gpu(np.array(selection(shape))))
    # single extreme pixels at each corner of the image and on both sides of a tile corner
    spots = [(0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1), (rows - 1, cols - 1), (rows, cols),
             (rows - 1, cols), (rows, cols - 1), (2 * rows, 2 * cols)]
    a = np.zeros(shape, np.uint8)
    for y, x in spots:
        a[y, x] = 255
    check(a, kind, r, qs=(0, 5000, 9999, 10000))
    check(255 - a, kind, r, qs=(0, 1, 5000, 10000))
    for y, x in ((rows - 1, cols - 1), (rows, cols)):
        one = np.full(shape, 7, np.uint8)
        one[y, x] = 200
        check(one, kind, r, qs=(10000,))


def test_a_single_pixel_becomes_the_footprint():
    for kind in KINDS:
        for r in (0, 1, 2, 3, 7, 31, TOP):
            a = np.zeros((2 * r + 3, 2 * r + 5), np.uint8)
            a[r + 1, r + 2] = 77
            exp = np.zeros_like(a)
            exp[1:2 * r + 2, 2:2 * r + 3] = 77 * ref.footprint(kind, r)
            it = gpu(a)
            assert np.array_equal(formed(nuclei.rank_filter(it, r, 1, kind), it), exp), (kind, r)
            if r > 0:                                                   # r = 0: one pixel, range 0
                assert np.array_equal(formed(nuclei.quantile_range(it, r, 0, 1, kind), it), exp), (kind, r)
                assert not formed(nuclei.median(it, r, kind), it).any()     # one pixel never decides the median


def test_the_literal_cases_of_the_contract():
    two = gpu(np.array([[10, 20]], np.uint8))
    for kind in KINDS:
        assert nuclei.rank_filter(two, 1, 0.5, kind).tolist() == [[20, 20]]
        assert nuclei.rank_filter(two, 1, 0.4999, kind).tolist() == [[10, 10]]
        assert nuclei.median(two, 1, kind).tolist() == [[20, 20]]
    image = np.random.RandomState(5).permutation(25).reshape(5, 5).astype(np.uint8)     # the interior of a square of r = 2: n = 25
    it = gpu(image)
    for q, value in ((0.2, 5), (0.1999, 4), (0, 0), (1, 24), (0.9999, 24), (0.0001, 0), (0.5, 12)):
        assert int(nuclei.rank_filter(it, 2, q, 'square')[2, 2]) == value, q
    # entropy: constant 0; two values half and half exactly one bit; a (1, 3) split; sixteen different values four bits
    assert nuclei.local_entropy(gpu(np.full((9, 9), 77, np.uint8)), 3).tolist() == [[0.0] * 9] * 9
    assert nuclei.local_entropy(gpu(np.array([[5, 9, 5, 9]], np.uint8)), 3, 'square', raw=True).tolist() == [[65536] * 4]
    split = (8 * 65536 - ref.TERMS[3]) // 4
    assert nuclei.local_entropy(gpu(np.array([[1, 2, 2, 2]], np.uint8)), 3, 'square', raw=True).tolist() == [[split] * 4]
    assert nuclei.local_entropy(gpu(np.arange(16, dtype=np.uint8).reshape(1, 16)), 15, 'square').tolist() == [[4.0] * 16]


def test_a_square_larger_than_the_image_gives_the_global_quantile():
    for shape in ((1, 1), (5, 9), (40, 61)):
        a = content(shape, 'random')
        it = gpu(np.array(a))
        v = np.sort(a.ravel())
        for q in QS:
            got = formed(nuclei.rank_filter(it, TOP, frac(q), 'square'), it)
            assert (got == v[min(v.size - 1, v.size * q // 10000)]).all(), (shape, q)


# ------------------------------------------------------------------ within
def test_within_of_every_type_and_a_within_that_selects_nothing():
    shape = (67, 131)
    a, w = content(shape, 'random'), selection(shape)
    it = gpu(np.array(a))
    cases = (('disk', 3), ('square', 1), ('diamond', 31))
    exp = {c: results(a, c[0], c[1], w, (0, 5000, 10000)) for c in cases}
    for dtype, value in ((torch.bool, True), (torch.uint8, 200), (torch.int16, -3), (torch.int32, 2 ** 24), (torch.int64, 2 ** 40)):
        wt = gpu(np.array(w)).to(dtype) * value                         # non-zero only in a high byte: the whole element is read
        for kind, r in cases:
            compare(exp[kind, r], it, kind, r, wt, qs=(0, 5000, 10000), note=dtype)
        none = torch.zeros(shape, dtype=dtype, device=DEV)
        for q in (0, 0.5, 1):
            assert not formed(nuclei.rank_filter(it, 3, q, within=none), it).any()
        assert not formed(nuclei.quantile_range(it, 3, 0, 1, within=none), it).any()
        assert not formed(nuclei.local_entropy(it, 3, within=none, raw=True), it, torch.int32).any()
        assert not bool(nuclei.median(it > 100, 3, within=none).any())
    # the centre has no special role: a pixel outside `within` is still defined, from its counted neighbours
    w1 = np.ones(shape, bool)
    w1[30, 60] = False
    got = formed(nuclei.median(it, 1, 'square', gpu(w1)), it)
    assert got[30, 60] == np.sort(np.delete(a[29:32, 59:62].ravel(), 4))[4]
    # non-contiguous and unaligned `within`
    big = torch.zeros(shape[0], 2 * shape[1] + 1, dtype=torch.uint8, device=DEV)
    wt = big[:, 1::2]
    wt.copy_(gpu(np.array(w)))
    assert not wt.is_contiguous()
    check(a, 'disk', 7, image_t=it, within=w, within_t=wt)
    flat = torch.zeros(shape[0] * shape[1] + 1, dtype=torch.uint8, device=DEV)
    wt = flat[1:].view(shape)
    wt.copy_(gpu(np.array(w)))
    assert wt.is_contiguous() and wt.data_ptr() % 4 == 1
    check(a, 'disk', 7, image_t=it, within=w, within_t=wt)


# ------------------------------------------------------------------ strides, alignment, dtypes, empty shapes
def test_views_offsets_and_bool_images():
    base = np.random.RandomState(5).randint(0, 256, (60, 212)).astype(np.uint8)
    bt = gpu(base)
    views = [(bt.t(), base.T), (bt[::2, 1::3], base[::2, 1::3]), (bt[3:, 5:], base[3:, 5:])]
    flat = gpu(np.concatenate([np.zeros(1, np.uint8), base.ravel()]))   # a contiguous view whose base is not dword-aligned
    off = flat[1:].view(60, 212)
    assert off.is_contiguous() and off.data_ptr() % 4 == 1
    views.append((off, base))
    for vt, v in views:
        for kind, r in (('disk', 3), ('square', 7), ('diamond', 1)):
            check(v, kind, r, image_t=vt, qs=(500, 5000, 9500))
    wt = gpu(np.array(selection((60, 212))))
    check(base, 'disk', 3, image_t=off, within=selection((60, 212)), within_t=wt)
    m = base > 130
    mt = gpu(m)
    for kind in KINDS:
        for r in (0, 1, 5):
            got = nuclei.median(mt, r, kind)
            assert np.array_equal(formed(got, mt, torch.bool), ref.median(m, r, kind)), (kind, r)
            assert torch.equal(got, nuclei.median(mt.to(torch.uint8), r, kind) != 0)
            got = nuclei.rank_filter(mt, r, 0.25, kind)
            assert np.array_equal(formed(got, mt, torch.bool), ref.rank_filter(m, r, 2500, kind)), (kind, r)
            assert np.array_equal(formed(nuclei.quantile_range(mt, r, 0.25, 0.75, kind), mt), ref.quantile_range(m, r, 2500, 7500, kind))
            assert np.array_equal(formed(nuclei.local_entropy(mt, r, kind, raw=True), mt, torch.int32), ref.local_entropy_raw(m, r, kind))


def test_the_median_of_a_mask_is_the_majority_of_window_sums():
    base = np.random.RandomState(11).rand(3 * 8 + 5, 261) < 0.5
    mt = gpu(base)
    wt = gpu(np.array(selection(base.shape)))
    ties = False
    for r in (1, 2, 3, 7, 31, TOP):                                     # even counts at the border: ties give True
        for within in (None, wt):
            count, total, _ = nuclei.window_sums(mt.to(torch.uint8), r, within)
            majority = (2 * total >= count) & (count > 0)
            assert torch.equal(nuclei.median(mt, r, 'square', within), majority), r
            ties = ties or bool(((2 * total == count) & (count > 0)).any())
    assert ties


def test_empty_images():
    for shape in ((0, 5), (5, 0), (0, 0)):
        for dtype in (torch.uint8, torch.bool):
            empty = torch.zeros(shape, dtype=dtype, device=DEV)
            for within in (None, torch.zeros(shape, dtype=torch.bool, device=DEV)):
                for out, want_dtype in ((nuclei.rank_filter(empty, 3, 0.3, within=within), dtype),
                                        (nuclei.median(empty, 3, within=within), dtype),
                                        (nuclei.quantile_range(empty, 3, 0.1, 0.9, within=within), torch.uint8),
                                        (nuclei.local_entropy(empty, 3, within=within), torch.float32),
                                        (nuclei.local_entropy(empty, 3, within=within, raw=True), torch.int32)):
                    assert tuple(out.shape) == shape and out.device == empty.device and out.dtype == want_dtype


# ------------------------------------------------------------------ the GPU against itself
def test_extreme_quantiles_are_erode_dilate_and_the_gradient():
    shape = tile_shape(7)
    it = gpu(np.array(content(shape, 'random')))
    wt = gpu(np.array(selection(shape)) & (np.random.RandomState(3).rand(*shape) < 0.05))     # sparse: some windows count nothing
    empty = False
    for kind in KINDS:
        for r in (0, 1, 7, 31, TOP):
            for within in (None, wt):
                some = nuclei.dilate(wt if within is not None else torch.ones_like(it), r, kind) != 0
                lo, hi = nuclei.rank_filter(it, r, 0, kind, within), nuclei.rank_filter(it, r, 1, kind, within)
                assert torch.equal(lo[some], nuclei.erode(it, r, kind, within)[some])
                assert torch.equal(hi[some], nuclei.dilate(it, r, kind, within)[some])
                assert not bool(lo[~some].any()) and not bool(hi[~some].any())
                assert torch.equal(nuclei.quantile_range(it, r, 0, 1, kind, within), nuclei.morph_gradient(it, r, kind, within))
                empty = empty or bool((~some).any())
    assert empty


def test_monotone_in_q_and_deterministic():
    shape = tile_shape(3)
    it = gpu(np.array(content(shape, 'few')))
    wt = gpu(np.array(selection(shape)))
    for kind, r in (('disk', 3), ('square', 7), ('diamond', 31), ('disk', TOP)):
        for within in (None, wt):
            outs = [nuclei.rank_filter(it, r, frac(q), kind, within) for q in QS]
            assert all(bool((a <= b).all()) for a, b in zip(outs, outs[1:])), (kind, r)
            assert all(torch.equal(o, nuclei.rank_filter(it, r, frac(q), kind, within)) for o, q in zip(outs, QS))
            g = nuclei.quantile_range(it, r, 0.25, 0.75, kind, within)
            assert torch.equal(g.to(torch.int32), outs[QS.index(7500)].to(torch.int32) - outs[QS.index(2500)].to(torch.int32))
            assert torch.equal(g, nuclei.quantile_range(it, r, 0.25, 0.75, kind, within))
            if r <= ETOP:
                e = nuclei.local_entropy(it, r, kind, within, raw=True)
                assert torch.equal(e, nuclei.local_entropy(it, r, kind, within, raw=True))
                assert int(e.min()) >= 0 and int(e.max()) <= 2 * 65536          # four levels: at most two bits


def test_local_entropy_is_the_entropy_of_the_nucleus_features():
    """Three well-separated blobs, so that a crop's mask is the nucleus itself: the mean of local_entropy(gray, 3) over a blob is the
    mean_ent column.  atol: the derived 2^-15 of the fixed point plus the 1e-5 relative bar, times log2 29 < 4.86, that the existing
    tests hold that column to."""
    H, W = 90, 120
    yy, xx = np.mgrid[:H, :W]
    labels = np.zeros((H, W), np.int32)
    for lab, (cy, cx, ry, rx) in enumerate(((20, 25, 9, 14), (60, 60, 15, 8), (30, 95, 12, 12)), 1):
        labels[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = lab
    gray = np.random.RandomState(2).randint(0, 256, (H, W))
    gray[:, 60:] //= 32                                                 # few levels on the right: low entropy there
    gray = gray.astype(np.uint8)
    lt, gt = gpu(labels), gpu(gray)
    feats, _, kept = nuclei.nucleus_features(lt, gt)
    assert kept.tolist() == [1, 2, 3]
    ent = nuclei.local_entropy(gt, 3)
    col = nuclei.FEATURE_NAMES.index('mean_ent')
    for k in range(3):
        mean = float(ent[lt == k + 1].double().mean())
        assert abs(mean - float(feats[k, col])) <= 1e-4, (k, mean, float(feats[k, col]))
    assert float(feats[:, col].max()) - float(feats[:, col].min()) > 0.5       # the blobs do differ
