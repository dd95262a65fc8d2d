"""Flat grey-scale morphology on the GPU (csrc/morph.hip through cgc_net_amd.nuclei.erode / dilate / opening / closing / white_tophat
/ black_tophat / morph_gradient / open_by_reconstruction / close_by_reconstruction) against tests/morph_ref.py (a numpy restatement,
pinned by tests/test_morph_ref_cpu.py), and against the GPU's own distance transform and reconstruction.  Every comparison is exact.

A workgroup owns a tile of ``morph_tile_rows`` (32) rows by ``morph_tile_cols(r)`` (256 - 2 * (r rounded up to 4), 128..256) columns.
The shapes put footprints across every tile edge, make r larger than both sides and the halo larger than the image; the radii
0, 1, 2, 3, 7, 31, 63 use every level of the run-maximum table (run lengths 1, 3, 5, 7, 15, 63, 127 are levels 0, 1, 2, 2, 3, 5, 6,
and the shorter rows of a disk or diamond the levels below)."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import morph_ref as ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

TOP = kernels.MORPH_MAX_RADIUS
SHAPES = [(1, 1), (1, 300), (300, 1), (5, 9), (64, 64), (65, 63), (67, 131), (200, 333)]
RADII = [0, 1, 2, 3, 7, 31, TOP]
KINDS = ['square', 'disk', 'diamond']
CONTENTS = ['random', 'zeros', 'full', 'checker']
ids = dict(ids=lambda s: '%dx%d' % s)


def tile_shape(r):
    """Two tiles and a bit in each direction at radius r, neither side a multiple of the tile or of 4."""
    k = kernels.get()
    H, W = 2 * k.morph_tile_rows + 5, 2 * k.morph_tile_cols(r) + 3
    assert H % k.morph_tile_rows and W % k.morph_tile_cols(r) and H % 4 and W % 4
    return H, W


@functools.lru_cache(maxsize=None)
def content(shape, kind):
    """A shared, write-protected image."""
    if kind == 'random':
        a = np.random.RandomState(shape[0] * 7 + shape[1]).randint(0, 256, shape).astype(np.uint8)
    elif kind == 'checker':
        yy, xx = np.mgrid[:shape[0], :shape[1]]
        a = (((yy + xx) & 1) * 255).astype(np.uint8)
    else:
        a = np.full(shape, 255 if kind == 'full' else 0, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def selection(shape):
    w = np.random.RandomState(shape[0] * 3 + shape[1] + 1).rand(*shape) < 0.6
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def want(shape, kind_of_content, kind, r, op, selected):
    """The reference result, computed once and shared."""
    a = ref.flat_morphology(content(shape, kind_of_content), kind, r, op, selection(shape) if selected else None)
    a.setflags(write=False)
    return a


def formed(out, like, dtype=torch.uint8):
    assert out.dtype == dtype and tuple(out.shape) == tuple(like.shape) and out.is_contiguous() and out.device == like.device
    return out.cpu().numpy()


OPS = {'erode': nuclei.erode, 'dilate': nuclei.dilate, 'gradient': nuclei.morph_gradient}


def check(image, kind, r, image_t=None, within=None, within_t=None, ops=('erode', 'dilate', 'gradient')):
    it = gpu(np.array(image)) if image_t is None else image_t
    wt = within_t if within_t is not None else None if within is None else gpu(np.array(within))
    for op in ops:
        got = formed(OPS[op](it, r, kind, wt), it)
        exp = ref.flat_morphology(image, kind, r, op, within)
        assert np.array_equal(got, exp), (op, kind, r, np.argwhere(got != exp)[:5])


# ------------------------------------------------------------------ every shape, radius, footprint, content
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_every_radius(shape, kind):
    it = gpu(np.array(content(shape, 'random')))
    wt = gpu(np.array(selection(shape)))
    for r in RADII:
        for op, fn in OPS.items():
            got = formed(fn(it, r, kind), it)
            exp = want(shape, 'random', kind, r, op, False)
            assert np.array_equal(got, exp), (op, r, np.argwhere(got != exp)[:5])
            got = formed(fn(it, r, kind, wt), it)
            exp = want(shape, 'random', kind, r, op, True)
            assert np.array_equal(got, exp), (op, r, 'within', np.argwhere(got != exp)[:5])


@pytest.mark.parametrize('fill', CONTENTS[1:])
@pytest.mark.parametrize('shape', [(5, 9), (65, 63), (67, 131)], **ids)
def test_constant_and_checkerboard_images(shape, fill):
    it = gpu(np.array(content(shape, fill)))
    for kind in KINDS:
        for r in (0, 1, 3, TOP):
            for op, fn in OPS.items():
                got = formed(fn(it, r, kind), it)
                exp = want(shape, fill, kind, r, op, False)
                assert np.array_equal(got, exp), (op, kind, r)
    if fill != 'checker':                                               # closed form: a constant image stays, its gradient is 0
        assert (formed(nuclei.erode(it, 5), it) == content(shape, fill)).all() and not formed(nuclei.morph_gradient(it, 5), it).any()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('r', [1, 7, 31, TOP])
def test_footprints_across_every_tile_edge(kind, r):
    shape = tile_shape(r)
    rows, cols = kernels.get().morph_tile_rows, kernels.get().morph_tile_cols(r)
    check(content(shape, 'random'), kind, r)
    check(content(shape, 'random'), kind, r, within=selection(shape))
    # a single extreme pixel at each corner of the image and on both sides of a tile corner
    spots = [(0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1), (rows - 1, cols - 1), (rows, cols),
             (rows - 1, cols), (rows, cols - 1), (2 * rows, 2 * cols)]
    for y, x in spots:
        a = np.zeros(shape, np.uint8)
        a[y, x] = 255
        check(a, kind, r, ops=('dilate',))
        check(255 - a, kind, r, ops=('erode',))
    a = np.zeros(shape, np.uint8)
    for y, x in spots:
        a[y, x] = 255
    check(a, kind, r)


def test_a_single_pixel_becomes_the_footprint():
    for kind in KINDS:
        for r in (0, 1, 2, 3, 7, 31, TOP):
            a = np.zeros((2 * r + 3, 2 * r + 5), np.uint8)
            a[r + 1, r + 2] = 77
            exp = np.zeros_like(a)
            exp[1:2 * r + 2, 2:2 * r + 3] = 77 * ref.footprint(kind, r)
            it = gpu(a)
            assert np.array_equal(formed(nuclei.dilate(it, r, kind), it), exp), (kind, r)
            assert np.array_equal(formed(nuclei.erode(255 - it, r, kind), it), 255 - exp), (kind, r)


def test_a_square_larger_than_the_image_gives_the_global_extremum():
    for shape in ((1, 1), (5, 9), (40, 61)):
        a = content(shape, 'random')
        it = gpu(np.array(a))
        assert (formed(nuclei.erode(it, TOP, 'square'), it) == a.min()).all()
        assert (formed(nuclei.dilate(it, TOP, 'square'), it) == a.max()).all()
        assert (formed(nuclei.morph_gradient(it, TOP, 'square'), it) == int(a.max()) - int(a.min())).all()


# ------------------------------------------------------------------ within
def test_within_of_every_type_and_a_within_that_selects_nothing():
    shape = (67, 131)
    a, w = content(shape, 'random'), selection(shape)
    it = gpu(np.array(a))
    for dtype, value in ((torch.bool, True), (torch.uint8, 200), (torch.int16, -3), (torch.int32, 2 ** 24), (torch.int64, 2 ** 40)):
        wt = gpu(np.array(w)).to(dtype) * value                         # non-zero only in a high byte: the whole element is read
        for kind, r in (('disk', 3), ('square', 1), ('diamond', 31)):
            check(a, kind, r, image_t=it, within=w, within_t=wt)
        none = torch.zeros(shape, dtype=dtype, device=DEV)
        assert (formed(nuclei.erode(it, 3, within=none), it) == 255).all()
        assert (formed(nuclei.dilate(it, 3, within=none), it) == 0).all()
        assert (formed(nuclei.morph_gradient(it, 3, within=none), it) == 0).all()
    # the centre has no special role: a pixel outside `within` is still defined, from its counted neighbours
    w1 = np.ones(shape, bool)
    w1[30, 60] = False
    got = formed(nuclei.dilate(it, 1, 'square', gpu(w1)), it)
    assert got[30, 60] == np.delete(a[29:32, 59:62].ravel(), 4).max()
    # non-contiguous and unaligned `within`
    big = torch.zeros(shape[0], 2 * shape[1] + 1, dtype=torch.uint8, device=DEV)
    wt = big[:, 1::2]
    wt.copy_(gpu(np.array(w)))
    assert not wt.is_contiguous()
    check(a, 'disk', 7, image_t=it, within=w, within_t=wt)


# ------------------------------------------------------------------ compositions and epilogues
@pytest.mark.parametrize('kind', KINDS)
def test_opening_closing_and_the_top_hats(kind):
    for shape, r in (((5, 9), 1), ((65, 63), 2), ((67, 131), 3), ((200, 333), 7), (tile_shape(31), 31)):
        a, w = content(shape, 'random'), selection(shape)
        it, wt = gpu(np.array(a)), gpu(np.array(w))
        for name in ('opening', 'closing', 'white_tophat', 'black_tophat'):
            fn, rf = getattr(nuclei, name), getattr(ref, name)
            assert np.array_equal(formed(fn(it, r, kind), it), rf(a, r, kind)), (name, shape, r)
            assert np.array_equal(formed(fn(it, r, kind, wt), it), rf(a, r, kind, w)), (name, shape, r, 'within')
        x, o, c = (t.to(torch.int32) for t in (it, nuclei.opening(it, r, kind), nuclei.closing(it, r, kind)))
        assert bool((o <= x).all()) and bool((x <= c).all())
        assert torch.equal(nuclei.opening(o.to(torch.uint8), r, kind).to(torch.int32), o)           # idempotent
        assert torch.equal(nuclei.closing(c.to(torch.uint8), r, kind).to(torch.int32), c)
        assert torch.equal(nuclei.white_tophat(it, r, kind).to(torch.int32), x - o)                 # never negative before the clamp
        assert torch.equal(nuclei.black_tophat(it, r, kind).to(torch.int32), c - x)


def test_both_epilogues_clamp_at_zero():
    shape = (67, 131)
    a = content(shape, 'random')
    other = np.random.RandomState(8).randint(0, 256, shape).astype(np.uint8)
    it, ot = gpu(np.array(a)), gpu(other)
    k = kernels.get()
    for kind in KINDS:
        for op in ('erode', 'dilate', 'gradient'):
            for ep in ('other_minus', 'minus_other'):
                got = formed(k.flat_morphology(it, kind, 3, op, None, ot, ep), it)
                exp = ref.flat_morphology(a, kind, 3, op, None, other, ep)
                assert np.array_equal(got, exp) and (exp == 0).any() and (exp > 0).any(), (kind, op, ep)
                got = formed(k.flat_morphology(it, kind, 3, op, None, ot.t().contiguous().t(), ep), it)      # a strided `other`
                assert np.array_equal(got, exp)


# ------------------------------------------------------------------ strides, alignment, dtypes, empty shapes
def test_views_offsets_and_bool_images():
    base = np.random.RandomState(5).randint(0, 256, (140, 420)).astype(np.uint8)
    bt = gpu(base)
    views = [(bt.t(), base.T), (bt[::2, 1::3], base[::2, 1::3]), (bt[3:, 5:], base[3:, 5:])]
    flat = gpu(np.concatenate([np.zeros(1, np.uint8), base.ravel()]))   # a contiguous view whose base is not dword-aligned
    off = flat[1:].view(140, 420)
    assert off.is_contiguous() and off.data_ptr() % 4 == 1
    views.append((off, base))
    for vt, v in views:
        for kind, r in (('disk', 3), ('square', 7), ('diamond', 1)):
            check(v, kind, r, image_t=vt)
        assert np.array_equal(formed(nuclei.white_tophat(vt, 3), vt), ref.white_tophat(v, 3))
    wt = gpu(np.array(selection((140, 420))))
    check(base, 'disk', 3, image_t=off, within=selection((140, 420)), within_t=wt)
    for kind in KINDS:
        for r in (0, 1, 5):
            m = base > 60
            mt = gpu(m)
            for name in ('erode', 'dilate', 'opening', 'closing'):
                got = getattr(nuclei, name)(mt, r, kind)
                as_u8 = getattr(nuclei, name)(mt.to(torch.uint8), r, kind)
                assert np.array_equal(formed(got, mt, torch.bool), getattr(ref, name)(m, r, kind)), (name, kind, r)
                assert torch.equal(got, as_u8 != 0)
            for name in ('white_tophat', 'black_tophat', 'morph_gradient'):
                got = formed(getattr(nuclei, name)(mt, r, kind), mt, torch.uint8)
                assert np.array_equal(got, getattr(ref, name)(m, r, kind)), (name, kind, r)
    none = torch.zeros(140, 420, dtype=torch.bool, device=DEV)
    assert bool(nuclei.erode(gpu(base > 60), 2, within=none).all())     # the neutral value of a bool erosion is True


def test_empty_images():
    for shape in ((0, 5), (5, 0), (0, 0)):
        for dtype in (torch.uint8, torch.bool):
            empty = torch.zeros(shape, dtype=dtype, device=DEV)
            for name in ('erode', 'dilate', 'opening', 'closing', 'white_tophat', 'black_tophat', 'morph_gradient'):
                for within in (None, torch.zeros(shape, dtype=torch.bool, device=DEV)):
                    out = getattr(nuclei, name)(empty, 3, within=within)
                    assert tuple(out.shape) == shape and out.device == empty.device
                    assert out.dtype == (dtype if name in ('erode', 'dilate', 'opening', 'closing') else torch.uint8)


# ------------------------------------------------------------------ the GPU against itself
def test_duality_gradient_and_determinism():
    shape = tile_shape(7)
    it = gpu(np.array(content(shape, 'random')))
    wt = gpu(np.array(selection(shape)))
    for kind in KINDS:
        for r in (1, 7, 31, TOP):
            for within in (None, wt):
                e, d, g = nuclei.erode(it, r, kind, within), nuclei.dilate(it, r, kind, within), nuclei.morph_gradient(it, r, kind, within)
                assert torch.equal(d, 255 - nuclei.erode(255 - it, r, kind, within))
                assert torch.equal(g.to(torch.int32), (d.to(torch.int32) - e.to(torch.int32)).clamp(min=0))
                assert torch.equal(e, nuclei.erode(it, r, kind, within)) and torch.equal(g, nuclei.morph_gradient(it, r, kind, within))


def test_binary_erosion_by_a_disk_is_the_distance_transform():
    labels, _ = nuclei.synthetic_tissue(200, 260, 30)
    m = gpu(labels > 0)
    # distance to the nearest background pixel; the image border is not background for either
    dist2 = nuclei.distance_transform(m)
    for r in (1, 2, 3, 7, 12):
        assert torch.equal(nuclei.erode(m, r, 'disk'), dist2 > r * r), r


def test_squares_and_diamonds_compose():
    shape = (67, 131)
    it = gpu(np.array(content(shape, 'random')))
    for kind in ('square', 'diamond'):
        e = d = it
        for r in range(1, 8):
            e, d = nuclei.erode(e, 1, kind), nuclei.dilate(d, 1, kind)
            assert torch.equal(e, nuclei.erode(it, r, kind)) and torch.equal(d, nuclei.dilate(it, r, kind)), (kind, r)


def test_by_reconstruction():
    labels, gray = nuclei.synthetic_tissue(150, 190, 25)
    for x in (gpu(gray), gpu(labels > 0)):
        for kind, r, conn in (('disk', 3, 1), ('square', 2, 2), ('diamond', 5, 1)):
            o, obr = nuclei.opening(x, r, kind), nuclei.open_by_reconstruction(x, r, kind, conn)
            c, cbr = nuclei.closing(x, r, kind), nuclei.close_by_reconstruction(x, r, kind, conn)
            assert obr.dtype == x.dtype == cbr.dtype and obr.shape == x.shape
            i = [t.to(torch.int32) for t in (o, obr, x, cbr, c)]
            assert all(bool((a <= b).all()) for a, b in zip(i, i[1:])), (kind, r)
            assert torch.equal(obr, nuclei.reconstruct(nuclei.erode(x, r, kind), x, 'dilation', conn))
            assert torch.equal(cbr, nuclei.reconstruct(nuclei.dilate(x, r, kind), x, 'erosion', conn))


def test_the_docstring_example_end_to_end():
    labels, gray = nuclei.synthetic_tissue(300, 300, 60)
    # nuclei dark on a bright, unevenly lit background -> a bright-on-dark plane with a ramp under it
    ramp = np.linspace(0, 60, 300).astype(np.int32)[None, :]
    plane = gpu(np.clip((255 - gray.astype(np.int32)) // 2 + ramp, 0, 255).astype(np.uint8))
    flat = nuclei.white_tophat(plane, 15)
    fg = flat > nuclei.otsu_threshold(flat)
    markers, n = nuclei.label_instances(nuclei.erode(fg, 2))
    L = nuclei.watershed(nuclei.morph_gradient(plane, 1), markers, within=fg)
    assert n > 0 and L.dtype == markers.dtype and L.shape == plane.shape
    assert bool(fg.any()) and not bool(fg.all())
    assert not bool((L[~fg] != 0).any())                                # labels only inside the foreground
    assert bool((L[markers != 0] == markers[markers != 0]).all())       # markers keep their labels
    assert set(L.unique().tolist()) <= set(range(n + 1))
    assert np.array_equal(flat.cpu().numpy(), ref.white_tophat(plane.cpu().numpy(), 15))
