"""GPU: the stain front end (csrc/stain.hip, csrc/smooth.hip; cgc_net_amd.nuclei.separate_stains, histogram, otsu_threshold, smooth,
stain_foreground) against tests/stain_ref.py.  Integer arithmetic with a stated contract on both sides: every comparison is exact."""
import functools
import itertools

import numpy as np
import pytest
import torch
from scipy import ndimage

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import stain_ref as ref
from image_cases import DEV, DTYPES, gpu

pytestmark = pytest.mark.gpu

TILE_SHAPES = [(0, 0), (0, 7), (1, 1), (1, 3), (1, 5), (7, 1), (5, 13), (63, 65), (257, 129)]      # pixel counts 0, 1, 3, 5, 7: dword tails
SHAPES = [(1, 1), (1, 9), (9, 1), (63, 63), (64, 64), (65, 65), (63, 65), (130, 70)]
PLANES = [p for k in (1, 2, 3) for p in itertools.combinations((0, 1, 2), k)]
OTHER_STAINS = ((0.9, 0.3, 0.3), (0.2, 0.9, 0.4), (0.3, 0.3, 0.9))


def fresh(a):
    """A shared, write-protected reference array as a tensor on the device (through a writable copy)."""
    return gpu(np.array(a))


def random_tile(shape, seed):
    """uint8 [H, W, 3] with the extremes 0, 1, 254, 255 over-represented in every channel."""
    rng = np.random.RandomState(seed)
    pix = rng.randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)
    extreme = rng.rand(*pix.shape) < 0.2
    pix[extreme] = rng.choice(np.array([0, 1, 254, 255], np.uint8), size=int(extreme.sum()))
    return pix


# ------------------------------------------------------------------ separate_stains
@pytest.mark.parametrize('order', ['bgr', 'rgb'])
@pytest.mark.parametrize('shape', TILE_SHAPES)
def test_separate_stains_every_plane_subset(shape, order):
    pix = random_tile(shape, 7 + shape[0])
    image = gpu(pix)
    full = ref.separate(pix, ref.stain_matrix(), nuclei.STAIN_ORDERS[order])
    for planes in PLANES:
        out = nuclei.separate_stains(image, order=order, planes=planes)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (len(planes),) + tuple(shape) and out.is_contiguous()
        assert np.array_equal(out.cpu().numpy(), full[list(planes)]), planes


@pytest.mark.parametrize('shape', [(1, 7), (63, 65)])
def test_separate_stains_custom_matrix(shape):
    pix = random_tile(shape, 3)
    out = nuclei.separate_stains(gpu(pix), stains=OTHER_STAINS, order='rgb')
    assert np.array_equal(out.cpu().numpy(), ref.separate(pix, ref.stain_matrix(OTHER_STAINS), 1))
    skewed = ((0.6, 0.7, 0.3), (0.55, 0.75, 0.3), (0.3, 0.6, 0.75))             # nearly parallel stains: large entries of both signs
    out = nuclei.separate_stains(gpu(pix), stains=skewed)
    assert np.array_equal(out.cpu().numpy(), ref.separate(pix, nuclei.stain_matrix(skewed).astype(np.int64), 0))


def test_separate_stains_extreme_pixels():
    pix = np.array([[a, b, c] for a in (0, 1, 255) for b in (0, 1, 255) for c in (0, 1, 255)], np.uint8).reshape(3, 9, 3)
    for order in ('bgr', 'rgb'):
        out = nuclei.separate_stains(gpu(pix), order=order)
        assert np.array_equal(out.cpu().numpy(), ref.separate(pix, ref.stain_matrix(), nuclei.STAIN_ORDERS[order]))
    white = nuclei.separate_stains(gpu(np.full((2, 3, 3), 255, np.uint8)))
    assert int(white.max()) == 0


def test_separate_stains_strided_views():
    pix = random_tile((40, 58), 11)
    image = gpu(pix)
    M = ref.stain_matrix()
    flipped = image.flip(2)                                                     # BGR seen as RGB
    assert np.array_equal(nuclei.separate_stains(flipped, order='rgb').cpu().numpy(), ref.separate(pix, M, 0))
    colmajor = image[:, :, [2, 1, 0]].transpose(0, 1).contiguous().transpose(0, 1)      # channel-flipped, column-major pixels
    assert not colmajor.is_contiguous()
    assert np.array_equal(nuclei.separate_stains(colmajor).cpu().numpy(), ref.separate(pix[:, :, ::-1], M, 0))
    planar = image.permute(2, 0, 1).contiguous().permute(1, 2, 0)              # channel planes, as a decoder may deliver them
    assert not planar.is_contiguous()
    assert np.array_equal(nuclei.separate_stains(planar).cpu().numpy(), ref.separate(pix, M, 0))
    sub = image[::2, ::2]
    assert not sub.is_contiguous()
    assert np.array_equal(nuclei.separate_stains(sub).cpu().numpy(), ref.separate(pix[::2, ::2], M, 0))
    odd = image[1:, 3:]                                                         # a base that is no multiple of four bytes
    assert np.array_equal(nuclei.separate_stains(odd).cpu().numpy(), ref.separate(pix[1:, 3:], M, 0))


def test_stain_separate_refuses_overflowing_tables_on_the_device_path():
    image = gpu(random_tile((4, 4), 0))
    lut, m = list(nuclei.OD_LUT), nuclei.stain_matrix().tolist()
    with pytest.raises(ValueError):
        kernels.get().stain_separate(image, 0, lut, [[2 ** 20, 0, 0], [0, 1, 0], [0, 0, 1]], 7)
    with pytest.raises(ValueError):
        kernels.get().stain_separate(image, 0, lut, m, 0)


# ------------------------------------------------------------------ histogram
def check_histogram(img, within=None):
    out = nuclei.histogram(gpu(img), None if within is None else (within if torch.is_tensor(within) else gpu(within)))
    assert out.dtype == torch.int64 and tuple(out.shape) == (256,) and out.is_cuda
    want = ref.histogram(img, None if within is None else (within.cpu().numpy() if torch.is_tensor(within) else within))
    assert np.array_equal(out.cpu().numpy(), want)
    return want


@pytest.mark.parametrize('shape', TILE_SHAPES)
def test_histogram_sizes(shape):
    rng = np.random.RandomState(5 + shape[1])
    img = rng.randint(0, 256, shape).astype(np.uint8)
    assert check_histogram(img).sum() == img.size
    within = rng.rand(*shape) < 0.4
    assert check_histogram(img, within).sum() == within.sum()


def test_histogram_flat_checkerboard_and_random():
    H, W = 150, 131                                                             # two workgroups, the second one partly filled
    for v in (0, 77, 255):
        want = check_histogram(np.full((H, W), v, np.uint8))
        assert want[v] == H * W and want.sum() == H * W
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.where((yy + xx) % 2 == 0, 3, 250).astype(np.uint8)
    want = check_histogram(board)
    assert want[3] == (H * W + 1) // 2 and want[250] == H * W // 2
    runs = np.repeat(np.random.RandomState(3).randint(0, 256, (H, (W + 4) // 5)), 5, axis=1)[:, :W].astype(np.uint8)
    check_histogram(runs)                                                       # runs of five equal values, cut by the lanes' 16
    rnd = np.random.RandomState(4).randint(0, 256, (H, W)).astype(np.uint8)
    check_histogram(rnd)
    check_histogram(rnd, (yy // 3 + xx // 7) % 2 == 0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_histogram_within_dtypes(dtype):
    rng = np.random.RandomState(9)
    img = rng.randint(0, 256, (63, 65)).astype(np.uint8)
    sel = rng.rand(63, 65) < 0.5
    values = torch.from_numpy(rng.randint(1, 100, (63, 65))).to(DEV)
    within = (gpu(sel) if dtype == torch.bool else
              torch.where(gpu(sel), -values if dtype.is_signed else values, torch.zeros_like(values)).to(dtype))
    assert np.array_equal((within != 0).cpu().numpy(), sel)
    assert check_histogram(img, within).sum() == sel.sum()
    assert check_histogram(img, torch.zeros(63, 65, dtype=dtype, device=DEV)).sum() == 0
    if dtype == torch.int64:
        high = torch.where(gpu(sel), torch.full_like(values, 2 ** 40), torch.zeros_like(values))      # only the upper half is set
        check_histogram(img, high)


def test_histogram_around_the_workgroup_chunk():
    chunk = kernels.get().histogram_chunk
    assert chunk >= 256
    rng = np.random.RandomState(12)
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + 17):
        img = rng.randint(0, 256, (1, n)).astype(np.uint8)
        assert check_histogram(img).sum() == n
        assert check_histogram(np.full((1, n), 200, np.uint8))[200] == n
        within = rng.rand(1, n) < 0.5
        assert check_histogram(img, within).sum() == within.sum()


def test_histogram_strided_views():
    img = np.random.RandomState(13).randint(0, 256, (70, 90)).astype(np.uint8)
    g = gpu(img)
    assert np.array_equal(nuclei.histogram(g[::2, 1::3]).cpu().numpy(), ref.histogram(img[::2, 1::3]))
    assert np.array_equal(nuclei.histogram(g.t()).cpu().numpy(), ref.histogram(img))
    assert np.array_equal(nuclei.histogram(g[1:, 1:]).cpu().numpy(), ref.histogram(img[1:, 1:]))
    flat = g.reshape(-1)[3:3 + 69 * 90].reshape(69, 90)                          # a base that is no multiple of 16 bytes
    assert np.array_equal(nuclei.histogram(flat).cpu().numpy(), ref.histogram(img.reshape(-1)[3:3 + 69 * 90]))


# ------------------------------------------------------------------ smooth
@pytest.mark.parametrize('radius', range(6))
@pytest.mark.parametrize('shape', SHAPES)
def test_smooth(shape, radius):
    H, W = shape
    rng = np.random.RandomState(100 * radius + H + W)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    out = nuclei.smooth(gpu(img), radius)
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()
    assert np.array_equal(out.cpu().numpy(), ref.binomial_smooth(img, radius))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):                # an impulse in every corner: the replicated border
        imp = np.zeros(shape, np.uint8)
        imp[y, x] = 255
        assert np.array_equal(nuclei.smooth(gpu(imp), radius).cpu().numpy(), ref.binomial_smooth(imp, radius)), (y, x)
    flat = np.full(shape, 255, np.uint8)
    assert np.array_equal(nuclei.smooth(gpu(flat), radius).cpu().numpy(), flat)


def test_smooth_strided_odd_and_empty():
    img = np.random.RandomState(21).randint(0, 256, (80, 140)).astype(np.uint8)
    g = gpu(img)
    assert np.array_equal(nuclei.smooth(g[::2, ::3], 3).cpu().numpy(), ref.binomial_smooth(img[::2, ::3], 3))
    assert np.array_equal(nuclei.smooth(g.t(), 2).cpu().numpy(), ref.binomial_smooth(img.T, 2))
    assert np.array_equal(nuclei.smooth(g[:, :132], 5).cpu().numpy(), ref.binomial_smooth(img[:, :132], 5))      # W % 4 == 0, strided
    for shape in ((0, 5), (4, 0), (0, 0)):
        assert tuple(nuclei.smooth(torch.zeros(shape, dtype=torch.uint8, device=DEV), 2).shape) == shape
    again = nuclei.smooth(nuclei.smooth(g, 5), 5)                                # larger blurs are repeated calls
    assert np.array_equal(again.cpu().numpy(), ref.binomial_smooth(ref.binomial_smooth(img, 5), 5))


# ------------------------------------------------------------------ otsu_threshold, stain_foreground
@functools.lru_cache(maxsize=None)
def reference_pipeline(radius, with_within):
    labels, tile, within = ref.tile_case()
    return ref.stain_foreground(tile, radius=radius, within=within if with_within else None)


@pytest.mark.parametrize('with_within', [False, True])
@pytest.mark.parametrize('radius', [0, 2])
def test_stain_foreground_on_the_rendered_tile(radius, with_within):
    labels, tile, within = ref.tile_case()
    want_fg, want_t, want_plane = reference_pipeline(radius, with_within)
    fg, t, plane = nuclei.stain_foreground(fresh(tile), radius=radius, within=fresh(within) if with_within else None)
    assert isinstance(t, int) and t == want_t
    assert plane.dtype == torch.uint8 and np.array_equal(plane.cpu().numpy(), want_plane)
    assert fg.dtype == torch.bool and np.array_equal(fg.cpu().numpy(), want_fg)
    assert nuclei.otsu_threshold(plane, fresh(within) if with_within else None) == want_t
    if radius == 0:
        assert np.array_equal(fg.cpu().numpy(), labels > 0)                     # noise free: exactly the painted nuclei
    rgb = fresh(tile).flip(2)
    fg_rgb, t_rgb, _ = nuclei.stain_foreground(rgb, radius=radius, order='rgb', within=fresh(within) if with_within else None)
    assert t_rgb == want_t and torch.equal(fg_rgb, fg)


def test_otsu_threshold_matches_the_reference_on_noise():
    rng = np.random.RandomState(17)
    img = np.clip(np.where(rng.rand(120, 90) < 0.3, rng.normal(170, 20, (120, 90)), rng.normal(60, 25, (120, 90))), 0, 255).astype(np.uint8)
    within = rng.rand(120, 90) < 0.6
    assert nuclei.otsu_threshold(gpu(img)) == ref.otsu(ref.histogram(img))
    assert nuclei.otsu_threshold(gpu(img), gpu(within)) == ref.otsu(ref.histogram(img, within))


def test_degenerate_images():
    empty = torch.zeros(0, 9, dtype=torch.uint8, device=DEV)
    assert nuclei.otsu_threshold(empty) == 0 and int(nuclei.histogram(empty).sum()) == 0
    fg, t, plane = nuclei.stain_foreground(torch.zeros(0, 9, 3, dtype=torch.uint8, device=DEV))
    assert t == 0 and tuple(fg.shape) == (0, 9) and tuple(plane.shape) == (0, 9)
    for v in (0, 9, 255):
        assert nuclei.otsu_threshold(torch.full((33, 17), v, dtype=torch.uint8, device=DEV)) == v
    one = np.empty((20, 31, 3), np.uint8)
    one[...] = (180, 90, 200)                                                   # one colour: one level, nothing above it
    fg, t, plane = nuclei.stain_foreground(gpu(one), radius=3)
    want_fg, want_t, want_plane = ref.stain_foreground(one, radius=3)
    assert t == want_t == int(plane.max()) and not bool(fg.any()) and np.array_equal(plane.cpu().numpy(), want_plane)
    img = gpu(np.random.RandomState(2).randint(0, 256, (30, 30)).astype(np.uint8))
    assert nuclei.otsu_threshold(img, torch.zeros(30, 30, dtype=torch.bool, device=DEV)) == 0      # an empty selection


# ------------------------------------------------------------------ the whole chain
def test_tile_to_features():
    """Disjoint painted discs, each of more than min_size pixels: the chain tile -> foreground -> instances -> features runs on
    the device and finds one nucleus per disc."""
    H, W, min_size = 192, 160, 10
    yy, xx = np.mgrid[0:H, 0:W]
    labels = np.zeros((H, W), np.int32)
    centres = [(20, 20, 9), (20, 70, 6), (60, 40, 12), (60, 120, 8), (110, 30, 10), (120, 100, 14), (170, 60, 7), (165, 140, 9), (3, 150, 5)]
    for k, (cy, cx, r) in enumerate(centres):
        labels[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    labels[100, 150] = 99                                                        # a speck that min_size removes
    _, count = ndimage.label(labels > 0)
    sizes = ndimage.sum(labels > 0, ndimage.label(labels > 0)[0], range(1, count + 1))
    survivors = int((sizes >= min_size).sum())
    assert count == len(centres) + 1 and survivors == len(centres)
    tile = gpu(ref.render_tile(labels))
    fg, t, _ = nuclei.stain_foreground(tile, radius=0)
    assert np.array_equal(fg.cpu().numpy(), labels > 0)
    L, n = nuclei.split_touching(nuclei.fill_holes(fg), None, markers='h_maxima', growth='flood', h=2.0, min_size=min_size)
    assert n == survivors
    feats, cen, kept = nuclei.nucleus_features(L, nuclei.bgr_to_gray(tile), min_size=min_size, max_label=n)
    assert tuple(feats.shape) == (n, nuclei.NUM_FEATURES) and tuple(cen.shape) == (n, 2) and kept.tolist() == list(range(1, n + 1))
    assert bool(torch.isfinite(feats).all())
