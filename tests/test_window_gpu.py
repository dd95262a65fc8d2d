"""Window sums and local thresholds on the GPU (csrc/window.hip through cgc_net_amd.nuclei.window_sums / local_threshold /
local_stain_foreground) against tests/window_ref.py (a numpy restatement, pinned by tests/test_window_ref_cpu.py).  Every comparison
is exact.

A workgroup owns a tile of ``window_tile_rows`` (16) rows by ``window_strip_cols(r)`` (1024 - 2 * (r rounded up to 4), 768..1024)
columns and scans 1024 per-column sums in uint32; the scan of Q wraps once a strip holds more than 2^32 / 255^3 = 259 full columns of
255s.  The shapes put windows across every tile edge, make r larger than both sides, and fill whole strips with 255s."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import stain_ref
import window_ref as ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 300), (300, 1), (5, 9), (64, 64), (65, 63), (67, 131), (200, 333), (1100, 1030)]
RADII = [0, 1, 2, 7, 31, 64, 127]
CONTENTS = ['random', 'zeros', 'full', 'checker']
K64S = [-128, -13, 0, 13, 128]
OFFSETS = [-255, -3, 0, 3, 255]
FLOORS = [None, 0, 100, 255]
ids = dict(ids=lambda s: '%dx%d' % s)


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


def sums(image, r, within=None):
    """The GPU's (n, S, Q) as numpy arrays, their form checked."""
    it = image if torch.is_tensor(image) else gpu(np.array(image))
    wt = within if within is None or torch.is_tensor(within) else gpu(within)
    n, S, Q = nuclei.window_sums(it, r, wt)
    for o, dtype in ((n, torch.int32), (S, torch.int32), (Q, torch.int64)):
        assert o.dtype == dtype and tuple(o.shape) == tuple(it.shape) and o.is_contiguous() and o.device == it.device
    return n.cpu().numpy(), S.cpu().numpy(), Q.cpu().numpy()


def check_sums(image, r, within=None, image_t=None, within_t=None):
    got = sums(image if image_t is None else image_t, r, within if within_t is None else within_t)
    for name, g, w in zip('nSQ', got, ref.window_sums(image, r, within)):
        assert np.array_equal(g, w), (name, r, np.argwhere(g != w)[:5])
    return got


def torch_rule(v, n, S, Q, k64, c, floor):
    """The rule of the contract in torch int64, on the device."""
    v, n, S = v.to(torch.int64), n.to(torch.int64), S.to(torch.int64)
    L = 64 * (n * v - S - c * n)
    D = n * Q - S * S
    L2, k2D = L * L, (k64 * k64) * D
    if k64 >= 0:
        fg = (L > 0) & (L2 > k2D)
    else:
        fg = (L > 0) | ((L == 0) & (D > 0)) | ((L < 0) & (L2 < k2D))
    return fg & (v > (-1 if floor is None else floor)) & (n >= 1)


def threshold(image_t, r, k64, c, floor, within_t=None):
    fg = nuclei.local_threshold(image_t, r, k64 / 64, c, floor, within_t)          # k64 / 64 is exact in binary floating point
    assert fg.dtype == torch.bool and tuple(fg.shape) == tuple(image_t.shape) and fg.is_contiguous() and fg.device == image_t.device
    return fg


# ------------------------------------------------------------------ window_sums
@pytest.mark.parametrize('kind', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_window_sums_every_radius(shape, kind):
    image = content(shape, kind)
    it = gpu(np.array(image))
    for r in RADII:
        check_sums(image, r, image_t=it)


def test_empty_images():
    for shape in ((0, 5), (5, 0), (0, 0)):
        empty = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        for o in nuclei.window_sums(empty, 3) + nuclei.window_sums(empty, 3, torch.zeros(shape, dtype=torch.bool, device=DEV)):
            assert tuple(o.shape) == shape
        fg = nuclei.local_threshold(empty, 3, k=0.2, offset=1, floor=4)
        assert tuple(fg.shape) == shape and fg.dtype == torch.bool


def test_q_above_2_31_and_scans_that_wrap():
    n, S, Q = check_sums(content((300, 300), 'full'), 127)
    assert Q[150, 150] == 4228250625 > 2 ** 31 and n[150, 150] == 65025 and S[150, 150] == 255 * 65025
    # three strips of 768 columns, each scanning 1024 columns of 255 x 255s: 1024 * 255^3 = 3.95 x 2^32
    n, S, Q = check_sums(content((260, 2100), 'full'), 127)
    assert Q[130, 1000] == 4228250625 and int(Q.max()) == 4228250625
    check_sums(content((260, 2100), 'checker'), 127)


def test_windows_across_every_tile_edge():
    k = kernels.get()
    rows = k.window_tile_rows
    assert rows == 16
    for r in (0, 5, 126, 127):
        cols = k.window_strip_cols(r)
        assert cols == 1024 - 2 * ((r + 3) // 4 * 4)
        for shape in ((2 * rows + 1, cols + 1), (rows, cols), (rows + 1, 2 * cols), (rows - 1, 2 * cols + 3)):
            image = np.random.RandomState(r + shape[0]).randint(0, 256, shape).astype(np.uint8)
            within = np.random.RandomState(r + shape[1]).rand(*shape) < 0.5
            check_sums(image, r)
            check_sums(image, r, within)


@pytest.mark.parametrize('dtype', [torch.bool, torch.uint8, torch.int32, torch.int64], ids=str)
def test_within_dtypes_and_selections(dtype):
    shape = (67, 131)
    image = content(shape, 'random')
    it = gpu(np.array(image))
    rng = np.random.RandomState(5)
    nothing, one, half = np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    one[40, 77] = True
    half[:, :66] = True
    for within in (rng.rand(*shape) < 0.6, nothing, one, half):
        if dtype == torch.bool:
            wt = gpu(within)
        else:                                                           # non-zero values of every size, a high bit among them
            top = {torch.uint8: 255, torch.int32: -2 ** 31, torch.int64: 2 ** 40}[dtype]
            wt = torch.where(gpu(within), torch.tensor(top, dtype=dtype, device=DEV), torch.tensor(0, dtype=dtype, device=DEV))
        for r in (0, 2, 31, 127):
            got = check_sums(image, r, within, image_t=it, within_t=wt)
        if not within.any():
            assert not any(g.any() for g in got)
    n, S, Q = check_sums(image, 127, one, image_t=it)
    assert (n == 1).all() and (S == image[40, 77]).all()                # r exceeds both sides: every window is the image


def test_strided_images_and_within():
    base = np.random.RandomState(9).randint(0, 256, (140, 150)).astype(np.uint8)
    mask = np.random.RandomState(10).rand(140, 150) < 0.5
    bt, mt = gpu(base), gpu(mask)
    for r in (1, 7, 64):
        for view, view_t, w, w_t in ((base.T, bt.t(), mask.T, mt.t()), (base[:, ::3], bt[:, ::3], mask[:, ::3], mt[:, ::3]),
                                     (base[5:70:2, 3:], bt[5:70:2, 3:], mask[5:70:2, 3:], mt[5:70:2, 3:])):
            assert not view_t.is_contiguous()
            check_sums(view, r, image_t=view_t)
            check_sums(view, r, w, image_t=view_t, within_t=w_t)
            want = ref.local_threshold(view, r, 13, -3, 100, w)
            assert np.array_equal(threshold(view_t, r, 13, -3, 100, w_t).cpu().numpy(), want)


def test_contiguous_images_on_an_unaligned_base():
    """W % 4 == 0 but the first pixel is not on a dword boundary: rows cannot be read as dwords."""
    H, W = 37, 64
    flat = np.random.RandomState(12).randint(0, 256, H * W + 3).astype(np.uint8)
    sel = np.random.RandomState(13).rand(H * W + 3) < 0.5
    ft, st = gpu(flat), gpu(sel)
    for off in (1, 2, 3):
        image, within = flat[off:off + H * W].reshape(H, W), sel[off:off + H * W].reshape(H, W)
        it, wt = ft[off:off + H * W].view(H, W), st[off:off + H * W].view(H, W)
        assert it.is_contiguous() and it.data_ptr() % 4 == off
        for r in (0, 3, 40):
            check_sums(image, r, image_t=it)
            check_sums(image, r, within, image_t=it, within_t=wt)
            check_sums(image, r, within, image_t=it, within_t=gpu(within))      # an aligned mask beside an unaligned image
            assert np.array_equal(threshold(it, r, -13, 3, 0, wt).cpu().numpy(), ref.local_threshold(image, r, -13, 3, 0, within))


# ------------------------------------------------------------------ local_threshold
@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_local_threshold_equals_the_rule_on_the_sums(shape):
    image = content(shape, 'random')
    it = gpu(np.array(image))
    within = np.random.RandomState(shape[1]).rand(*shape) < 0.7
    wt = gpu(within)
    big = shape[0] * shape[1] > 10 ** 5
    for r in RADII:
        for w_np, w_t in ((None, None), (within, wt)):
            n, S, Q = nuclei.window_sums(it, r, w_t)
            combos = [(k64, c, floor) for k64 in K64S for c in OFFSETS for floor in FLOORS]
            if big:                                                     # every value of every parameter, not every combination
                combos = [(K64S[i % 5], OFFSETS[(i // 5 + i) % 5], FLOORS[i % 4]) for i in range(20)]
            for k64, c, floor in combos:
                assert torch.equal(threshold(it, r, k64, c, floor, w_t), torch_rule(it, n, S, Q, k64, c, floor)), (r, k64, c, floor)
            for k64, c, floor in ((13, 3, None), (-13, -3, 100), (0, 0, 0)):
                want = ref.local_threshold(image, r, k64, c, -1 if floor is None else floor, w_np)
                assert np.array_equal(threshold(it, r, k64, c, floor, w_t).cpu().numpy(), want), (r, k64, c, floor)


@pytest.mark.parametrize('kind', ['zeros', 'full', 'checker'])
def test_local_threshold_flat_and_checkerboard(kind):
    for shape in ((5, 9), (67, 131), (200, 333)):
        image = content(shape, kind)
        it = gpu(np.array(image))
        for r in (0, 2, 31, 127):
            for k64 in K64S:
                for c in (-255, -1, 0, 1, 255):
                    want = ref.local_threshold(image, r, k64, c, -1)
                    assert np.array_equal(threshold(it, r, k64, c, None).cpu().numpy(), want), (shape, r, k64, c)


def test_constant_image_has_no_spread():
    it = torch.full((70, 1100), 93, dtype=torch.uint8, device=DEV)
    for r in (0, 3, 127):
        for k64 in K64S:
            assert not bool(threshold(it, r, k64, 0, None).any())       # D = 0: v = m is not above m
            assert bool(threshold(it, r, k64, -1, None).all())
            assert not bool(threshold(it, r, k64, -1, 93).any()) and bool(threshold(it, r, k64, -1, 92).all())
        nothing = torch.zeros(70, 1100, dtype=torch.uint8, device=DEV)
        assert not bool(threshold(it, r, -128, -255, None, nothing).any())      # n = 0: background


def test_exact_tie_is_background():
    it = torch.tensor([[0, 0, 0, 0, 200]], dtype=torch.uint8, device=DEV)
    assert threshold(it, 4, 128, 0, None).tolist() == [[False] * 5]
    assert threshold(it, 4, 127, 0, None).tolist() == [[False] * 4 + [True]]
    assert nuclei.local_threshold(it, 4, k=2, offset=0).tolist() == [[False] * 5]
    assert nuclei.local_threshold(it.t(), 4, k=127 / 64).tolist() == [[False]] * 4 + [[True]]


def test_two_calls_are_bit_identical():
    image = gpu(np.array(content((1100, 1030), 'random')))
    within = gpu(np.random.RandomState(3).rand(1100, 1030) < 0.5)
    for w in (None, within):
        a, b = nuclei.window_sums(image, 31, w), nuclei.window_sums(image, 31, w)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(nuclei.local_threshold(image, 31, 0.2, 3, 10, w), nuclei.local_threshold(image, 31, 0.2, 3, 10, w))


# ------------------------------------------------------------------ local_stain_foreground
@functools.lru_cache(maxsize=None)
def tile_256():
    labels, _ = nuclei.synthetic_tissue(256, 256, 40, seed=3)
    within = np.zeros(labels.shape, bool)
    within[10:230, 5:240] = True
    return labels, stain_ref.render_tile(labels), within


def test_local_stain_foreground_is_the_composition_of_the_public_pieces():
    labels, tile, within = tile_256()
    tt, wt = gpu(np.array(tile)), gpu(within)
    for w in (None, wt):
        fg, floor, plane = nuclei.local_stain_foreground(tt, 25, within=w, k=0.2, offset=4)
        want_plane = nuclei.smooth(nuclei.separate_stains(tt, None, 'bgr', (0,))[0], 2)
        assert floor is None and plane.dtype == torch.uint8 and torch.equal(plane, want_plane)
        assert torch.equal(plane, nuclei.stain_foreground(tt, within=w)[2])
        assert fg.dtype == torch.bool and torch.equal(fg, nuclei.local_threshold(plane, 25, 0.2, 4, None, w))
        assert np.array_equal(fg.cpu().numpy(), ref.local_threshold(plane.cpu().numpy(), 25, 13, 4, -1, None if w is None else within))
        fg9, floor9, _ = nuclei.local_stain_foreground(tt, 25, within=w, k=0.2, offset=4, floor=9)
        assert floor9 == 9 and torch.equal(fg9, fg & (plane > 9))
        fg_o, t, plane_o = nuclei.local_stain_foreground(tt, 25, within=w, k=0.2, offset=4, floor='otsu')
        assert isinstance(t, int) and t == nuclei.otsu_threshold(plane, w) and torch.equal(plane_o, plane)
        assert torch.equal(fg_o, fg & (plane > t))
    rgb = tt.flip(2)
    assert torch.equal(nuclei.local_stain_foreground(rgb, 25, order='rgb', k=0.2, offset=4)[0],
                       nuclei.local_stain_foreground(tt, 25, k=0.2, offset=4)[0])
    fg0, _, plane0 = nuclei.local_stain_foreground(tt, 7, stain=1, radius=0)
    assert torch.equal(plane0, nuclei.separate_stains(tt, None, 'bgr', (1,))[0]) and torch.equal(fg0, nuclei.local_threshold(plane0, 7))


# ------------------------------------------------------------------ the example that motivates the rule
def test_ramp_example_on_the_device():
    plane, disc = ref.ramp_discs()
    pt = gpu(plane)
    local = nuclei.local_threshold(pt, 20, k=0.0, offset=15).cpu().numpy()
    assert np.array_equal(local, disc > 0)                              # every pixel of every disc, no background pixel
    t = nuclei.otsu_threshold(pt)
    glob = (pt > t).cpu().numpy()
    assert t == 85
    lost = [d for d in range(1, 65) if not glob[disc == d].any()]
    assert len(lost) >= 1 and int((glob & (disc == 0)).sum()) > 0      # the global threshold loses whole discs and keeps background
