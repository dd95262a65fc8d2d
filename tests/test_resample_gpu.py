"""GPU: resampling (csrc/resample.hip; cgc_net_amd.nuclei.resize, resize_labels, rescale) against tests/resample_ref.py.  The rule
is exact equality, at the smallest shapes that reach every path of the kernel: one pixel, rows shorter than a lane's group, more
than one workgroup per axis (a workgroup owns 8 rows x 252 columns of bytes), every position of the dword stores against the
row's address (output widths 255, 256, 257, 259 and a base one byte off), boxes with fractional borders, the sides next to the int32
limit.  The references are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import resample_ref as ref
from image_cases import DEV, gpu, tissue

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.bool_): torch.bool, np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16,
         np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


@functools.lru_cache(maxsize=None)
def image(H, W, kind='random'):
    if kind == 'random':
        return np.random.RandomState(H * 1000 + W).randint(0, 256, (H, W)).astype(np.uint8)
    if kind == 'white':
        return np.full((H, W), 255, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy + xx) & 1) * 255).astype(np.uint8)                      # checkerboard


@functools.lru_cache(maxsize=None)
def want_u8(H, W, size, mode, kind='random'):
    return ref.resize(image(H, W, kind), size, mode)


def same(got, want):
    assert got.dtype == TORCH[want.dtype] and tuple(got.shape) == want.shape and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want)


LINEAR = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((1, 9), (3, 4)), ((37, 53), (74, 106)), ((37, 53), (61, 40)), ((37, 53), (36, 53)),
          ((37, 53), (18, 26)), ((37, 53), (37, 53)), ((5, 7), (64, 3)), ((9, 130), (9, 255)), ((9, 130), (9, 256)), ((9, 130), (9, 257)),
          ((9, 130), (9, 259)), ((9, 130), (17, 600))]
AREA = [((1, 1), (1, 1)), ((37, 53), (18, 26)), ((37, 53), (36, 53)), ((37, 53), (37, 53)), ((40, 64), (13, 9)), ((40, 64), (5, 8)),
        ((33, 33), (32, 1)), ((9, 600), (9, 255)), ((9, 600), (9, 257)), ((20, 520), (10, 260))]


@pytest.mark.parametrize('shape,size', LINEAR)
@pytest.mark.parametrize('kind', ['random', 'white', 'checker'])
def test_linear(shape, size, kind):
    same(nuclei.resize(gpu(image(*shape, kind)), size), want_u8(*shape, size, 'linear', kind))


@pytest.mark.parametrize('shape,size', AREA)
@pytest.mark.parametrize('kind', ['random', 'white', 'checker'])
def test_area(shape, size, kind):
    same(nuclei.resize(gpu(image(*shape, kind)), size, 'area'), want_u8(*shape, size, 'area', kind))


def test_the_32_bit_edge():
    row = gpu(image(1, 32767))
    same(nuclei.resize(row, (1, 32766)), want_u8(1, 32767, (1, 32766), 'linear'))
    same(nuclei.resize(row, (1, 16383), 'area'), want_u8(1, 32767, (1, 16383), 'area'))
    same(nuclei.resize_labels(row, (1, 32766)), ref.nearest(image(1, 32767), (1, 32766)))
    col = gpu(image(1, 32767).T)                                         # the same along the other axis
    same(nuclei.resize(col, (32766, 1)), np.ascontiguousarray(want_u8(1, 32767, (1, 32766), 'linear').T))


@pytest.mark.parametrize('mode,size', [('linear', (61, 131)), ('linear', (20, 27)), ('area', (18, 26)), ('area', (37, 53))])
def test_strides_and_alignment(mode, size):
    img = image(37, 53)
    want = want_u8(37, 53, size, mode)
    same(nuclei.resize(gpu(np.ascontiguousarray(img.T)).t(), size, mode), want)                  # a transposed view
    wide = torch.zeros(74, 106, dtype=torch.uint8, device=DEV)
    wide[::2, ::2] = gpu(img)
    same(nuclei.resize(wide[::2, ::2], size, mode), want)                                        # a [::2, ::2] slice
    buf = torch.zeros(37 * 53 + 8, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):                                                                        # a base off alignment
        buf[off:off + 37 * 53] = gpu(img).reshape(-1)
        view = buf[off:off + 37 * 53].view(37, 53)
        assert view.data_ptr() % 4 == off
        same(nuclei.resize(view, size, mode), want)


@pytest.mark.parametrize('mode,size', [('linear', (74, 106)), ('linear', (9, 259)), ('linear', (36, 53)), ('area', (18, 26)),
                                       ('area', (13, 9)), ('area', (37, 53))])
def test_colour(mode, size):
    planes = [image(37, 53), image(37, 53, 'checker'), image(53, 37).T.copy()]
    tile = gpu(np.stack(planes, 2))
    want = np.stack([ref.resize(p, size, mode) for p in planes], 2)
    same(nuclei.resize(tile, size, mode), want)
    same(nuclei.resize(tile.flip(2), size, mode), np.ascontiguousarray(want[:, :, ::-1]))
    same(nuclei.resize(tile[:, :, 1], size, mode), want[:, :, 1])                                # one channel: a strided plane
    same(nuclei.rescale(tile, 1, mode), np.stack(planes, 2))


def test_rescale_is_resize():
    img = gpu(image(37, 53))
    from fractions import Fraction
    same(nuclei.rescale(img, Fraction(1, 2), 'area'), want_u8(37, 53, (19, 27), 'area'))          # 18.5 and 26.5 round half up
    same(nuclei.rescale(img, (2, Fraction(3, 4))), want_u8(37, 53, (74, 40), 'linear'))


@functools.lru_cache(maxsize=None)
def small_tissue():
    return nuclei.synthetic_tissue(96, 96, 12)[0]


def as_dtype(lab, dtype):
    return lab != 0 if dtype == np.bool_ else lab.astype(dtype)


@functools.lru_cache(maxsize=None)
def want_labels(dtype, size, mode):
    return ref.resize_labels(as_dtype(small_tissue(), dtype), size, mode)


CASES = [('nearest', (192, 192)), ('nearest', (288, 288)), ('nearest', (37, 130)), ('nearest', (96, 96)), ('majority', (48, 48)),
         ('majority', (32, 32)), ('majority', (12, 12)), ('majority', (37, 50)), ('majority', (96, 96))]


@pytest.mark.parametrize('mode,size', CASES)
@pytest.mark.parametrize('dtype', [np.bool_, np.uint8, np.int16, np.int32, np.int64])
def test_labels(dtype, mode, size):
    lab = as_dtype(small_tissue(), dtype)
    got = nuclei.resize_labels(gpu(lab), size, mode)
    same(got, want_labels(dtype, size, mode))
    assert set(np.unique(got.cpu().numpy()).tolist()) <= set(np.unique(lab).tolist())
    if mode == 'nearest' and size[0] % 96 == 0 and size[0] == size[1]:
        k = size[0] // 96
        same(got, np.repeat(np.repeat(lab, k, 0), k, 1))


def test_labels_ties_and_signs():
    def one(a, dtype):
        a = np.array(a, dtype)
        got = nuclei.resize_labels(gpu(a), (1, 1), 'majority')
        same(got, ref.majority(a, (1, 1)))
        return got.item()

    assert one([[0, 5], [5, 0]], np.uint8) == 0 and one([[7, 5], [5, 7]], np.int32) == 5
    assert one([[9, 3, 9], [3, 1, 3], [9, 3, 9]], np.int32) == 3 and one([[3, 9, 3], [9, 1, 9], [3, 9, 3]], np.int64) == 3
    assert one([[-2, 4], [4, -2]], np.int16) == -2 and one([[4, -32768], [-32768, 4]], np.int16) == -32768
    assert one([[-1, 4], [4, -1]], np.int64) == -1 and one([[-7, -9], [-9, -7]], np.int32) == -9
    assert one([[200, 4], [4, 200]], np.uint8) == 4                      # uint8 compares unsigned
    assert one([[True, False]], np.bool_) is False
    neg = (small_tissue().astype(np.int16) - 5)                          # negative values throughout
    same(nuclei.resize_labels(gpu(neg), (37, 50), 'majority'), ref.majority(neg, (37, 50)))
    same(nuclei.resize_labels(gpu(neg), (130, 37)), ref.nearest(neg, (130, 37)))
    shared = np.array([[6, 2, 2]], np.int32)                             # 3 -> 2: the middle pixel is shared between the boxes
    same(nuclei.resize_labels(gpu(shared), (1, 2), 'majority'), np.array([[6, 2]], np.int32))


def test_labels_strides():
    lab = small_tissue().astype(np.int32)
    same(nuclei.resize_labels(gpu(np.ascontiguousarray(lab.T)).t(), (37, 50), 'majority'), want_labels(np.int32, (37, 50), 'majority'))
    wide = torch.zeros(192, 192, dtype=torch.int32, device=DEV)
    wide[::2, ::2] = gpu(lab)
    same(nuclei.resize_labels(wide[::2, ::2], (37, 130)), want_labels(np.int32, (37, 130), 'nearest'))
    buf = torch.zeros(96 * 96 + 4, dtype=torch.uint8, device=DEV)
    buf[1:1 + 96 * 96] = gpu(lab.astype(np.uint8)).reshape(-1)
    same(nuclei.resize_labels(buf[1:1 + 96 * 96].view(96, 96), (37, 130)), want_labels(np.uint8, (37, 130), 'nearest'))


def test_linear_against_torch_interpolate():
    """Independent of the restatement: float64 bilinear interpolation with half-pixel centres on the device.  The kernel rounds the
    exact value once (1/2 level); float64 interpolation of bytes is exact to about 1e-12 level."""
    img = gpu(image(37, 53))
    got = nuclei.resize(img, (74, 106)).to(torch.float64)
    want = F.interpolate(img.to(torch.float64)[None, None], size=(74, 106), mode='bilinear', align_corners=False)[0, 0]
    diff = (got - want).abs().max().item()
    print('linear against F.interpolate: largest difference %.12f' % diff)
    assert diff <= 0.5 + 1e-6


def test_determinism():
    img, tile = gpu(image(37, 53)), gpu(np.stack([image(37, 53)] * 3, 2))
    lab = gpu(small_tissue().astype(np.int32))
    for call in (lambda: nuclei.resize(img, (61, 131)), lambda: nuclei.resize(tile, (18, 26), 'area'),
                 lambda: nuclei.resize_labels(lab, (37, 50), 'majority'), lambda: nuclei.resize_labels(lab, (130, 200))):
        assert torch.equal(call(), call())


def test_plumbing_into_nucleus_features():
    labels, gray, _ = tissue()
    L, g = gpu(labels), gpu(gray)
    n = int(labels.max())
    gray2, L2 = nuclei.resize(g, (600, 600)), nuclei.resize_labels(L, (600, 600))
    assert gray2.shape == L2.shape == (600, 600)
    f1, c1, kept1 = nuclei.nucleus_features(L, g, max_label=n)
    # min_size is a number of pixels like every other length of the stage: at twice the pixel count per axis the default 10 becomes 40,
    # and then exactly the same nuclei are kept (an area a passes 10 iff 4 a passes 40)
    f2, c2, kept2 = nuclei.nucleus_features(L2, gray2, max_label=n, min_size=40)
    assert f2.shape == f1.shape and c2.shape == c1.shape and torch.equal(kept2, kept1)
    # with the default min_size the call runs too; the nuclei of 3 to 9 pixels now pass it (58 rows against 55 on this tissue)
    f3, c3, kept3 = nuclei.nucleus_features(L2, gray2, max_label=n)
    assert set(kept1.tolist()) <= set(kept3.tolist()) and f3.shape == (kept3.numel(), 16)
    with pytest.raises(ValueError):
        nuclei.nucleus_features(L, gray2)
    same(nuclei.resize(gray2, (300, 300), 'area'), ref.area(ref.linear(gray, (600, 600)), (300, 300)))
