"""GPU: stain normalisation (csrc/stain.hip k_od_scan<SCAN_CONC>, k_od_recolor; kernels.HipKernels.concentration_histogram /
od_recolor; nuclei.stain_maxima, recolor, normalize_stains) against tests/normalize_ref.py.  Integer arithmetic with a stated contract
on both sides: every comparison is exact and covers every pixel."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import macenko_ref
import normalize_ref as ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

LUT = nuclei.OD_LUT
EXP = nuclei.EXP_LUT
B = ref.BINS
IDENTITY = [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]
REACH_CONC = (2 ** 31 - 2 ** 15 - 1) // 5674                                     # the largest sum_c |m[c][s]| that is admitted
REACH_RECOLOR = (2 ** 31 - 2 ** 11 - 1) // 5674
# 0, 1, 3, 4, 5 pixels: the 1-3 pixel tail of a 4-pixel lane; 16383, 16384, 16385: the edge of a workgroup's chunk; 181 x 181: two
# chunks and a tail
SHAPES = [(0, 0), (1, 1), (1, 3), (1, 4), (1, 5), (127, 129), (128, 128), (1, 16385), (181, 181)]
OD_MINS = [0, 154, 5674]
MATRICES = {                                                                     # m[c][s] / a[c][d]
    'stains': ref.stain_matrix().tolist(),                                       # rint(4096 inv(S)) of the default stains
    'normalise': ref.recolor_matrix(ref.DEFAULT_STAINS, (Fraction(300, 128), Fraction(250, 128))).tolist(),
    'identity': IDENTITY,
    'steep': [[40000, -30000, 9000], [-35000, 45000, -8000], [7000, -9000, 50000]],      # bins 0 and 511, k 0 and 6385, on many pixels
    'edge': [[REACH_CONC, 0, -1], [0, -REACH_CONC, 1], [0, 0, REACH_CONC - 2]],          # at the edge of the (tighter) overflow refusal
}


def random_tile(shape, seed):
    """uint8 [H, W, 3], uniform random bytes with the extremes 0, 1, 254, 255 over-represented."""
    rng = np.random.RandomState(seed)
    pix = rng.randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)
    extreme = rng.rand(*pix.shape) < 0.1
    pix[extreme] = rng.choice(np.array([0, 1, 254, 255], np.uint8), size=int(extreme.sum()))
    return pix


@functools.lru_cache(maxsize=None)
def random_case(shape):
    pix = random_tile(shape, 23 + shape[0] + shape[1])
    pix.setflags(write=False)
    return pix


def table():
    return kernels.get()


def counts_of(image, order, od_min, m, within=None):
    out = table().concentration_histogram(image, order, LUT, od_min, m, within)
    assert out.dtype == torch.int32 and tuple(out.shape) == (2 * B,) and out.device == image.device
    return out.tolist()


def recolored(image, order, a):
    out = table().od_recolor(image, order, LUT, a, EXP)
    assert out.dtype == torch.uint8 and out.shape == image.shape and out.device == image.device and out.is_contiguous()
    return out.cpu().numpy()


def check_both(pix, order, od_min=154, within=None, image=None, within_gpu=None, names=('stains', 'normalise')):
    """Both kernels on one input against the restatement, every bin and every pixel; returns the number of selected pixels."""
    image = gpu(np.array(pix)) if image is None else image
    if within is not None and within_gpu is None:
        within_gpu = gpu(np.array(within))
    n = None
    for name in names:
        want = ref.concentration_histogram(pix, order, ref.od_lut(), od_min, MATRICES[name], within)
        n = int(want[:B].sum())
        assert n == int(want[B:].sum())
        assert counts_of(image, order, od_min, MATRICES[name], within_gpu) == want.tolist(), name
        if within is None and od_min == 154:                                     # od_recolor takes neither
            assert np.array_equal(recolored(image, order, MATRICES[name]), ref.od_recolor(pix, order, ref.od_lut(), MATRICES[name], ref.exp_lut())), name
    return n


# ------------------------------------------------------------------ shapes, orders, thresholds, matrices
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('shape', SHAPES)
def test_random_tiles_every_matrix(shape, order):
    pix = random_case(shape)
    assert table().scan_chunk == 16384 and shape[0] * shape[1] in (0, 1, 3, 4, 5, 16383, 16384, 16385, 32761)
    n = check_both(pix, order, names=tuple(MATRICES))
    assert n > 1000 or shape[0] * shape[1] <= 5
    for od_min in OD_MINS:
        check_both(pix, order, od_min, names=('stains',))
    if shape == (181, 181):                                                      # the extreme bins and levels are reached, not only allowed
        hist = ref.concentration_histogram(pix, order, ref.od_lut(), 154, MATRICES['steep'])
        assert hist[0] > 100 and hist[B - 1] > 100 and hist[B] > 100 and hist[2 * B - 1] > 100
        out = ref.od_recolor(pix, order, ref.od_lut(), MATRICES['steep'], ref.exp_lut())
        assert (out == 0).sum() > 100 and (out == 255).sum() > 100
        O = ref.od_of(pix, order, ref.od_lut()) @ np.array(MATRICES['edge'], np.int64)
        assert O.max() > 2 ** 31 - 2 ** 16 and O.min() < -2 ** 31 + 2 ** 16      # sums next to the ends of int32


def test_empty_images():
    for shape in ((0, 0), (0, 7), (5, 0)):
        image = torch.zeros(shape + (3,), dtype=torch.uint8, device=DEV)
        assert counts_of(image, 0, 0, MATRICES['stains']) == [0] * (2 * B)
        assert counts_of(image, 1, 0, MATRICES['stains'], torch.zeros(shape, dtype=torch.bool, device=DEV)) == [0] * (2 * B)
        assert recolored(image, 0, IDENTITY).shape == shape + (3,)
        assert tuple(nuclei.recolor(image, IDENTITY).shape) == shape + (3,)


@pytest.mark.parametrize('value', [0, 1, 37, 255])
def test_flat_tiles(value):
    """Every lane on one bin of each stain."""
    pix = np.full((181, 181, 3), value, np.uint8)
    image = gpu(pix)
    n = check_both(pix, 0, 0, image=image)
    assert n == 32761
    hist = counts_of(image, 0, 0, MATRICES['stains'])
    assert max(hist[:B]) == 32761 == max(hist[B:])
    assert np.array_equal(recolored(image, 1, IDENTITY), np.maximum(pix, 1))
    check_both(pix, 1, 154, image=image)


def test_extreme_bins_and_levels():
    """Pixels and matrices that reach bins 0 and 511 and k of 0 and 6385, through negative and huge sums."""
    pix = np.array([[[0, 0, 0], [255, 255, 255], [1, 255, 255], [255, 0, 255], [255, 255, 0], [128, 128, 128], [0, 255, 0]]], np.uint8)
    image = gpu(pix)
    for sign in (1, -1):                                                         # column sums at the edge of the refusal
        p, q = REACH_CONC - REACH_CONC // 2, REACH_CONC // 2
        full = [[sign * p, -sign * p, 0], [-sign * q, sign * q, 0], [0, 0, 0]]
        want = ref.concentration_histogram(pix, 1, ref.od_lut(), 0, full)
        assert want[0] > 0 and want[B - 1] > 0 and want[B] > 0 and want[2 * B - 1] > 0
        assert counts_of(image, 1, 0, full) == want.tolist()
        p, q = REACH_RECOLOR - REACH_RECOLOR // 2, REACH_RECOLOR // 2
        full = [[sign * p, -sign * p, 7], [-sign * q, sign * q, 0], [0, 0, 0]]
        want = ref.od_recolor(pix, 1, ref.od_lut(), full, ref.exp_lut())
        assert (want[..., :2] == 0).any(axis=(0, 1)).all() and (want[..., :2] == 255).any(axis=(0, 1)).all()
        assert np.array_equal(recolored(image, 1, full), want)
        assert np.array_equal(recolored(gpu(np.ascontiguousarray(pix[..., ::-1])), 0, full), want[..., ::-1])
    # the last level before 0 and the first after 255: k = 6384 -> 1, k = 6385 -> 0, k = 1 -> 254 or 255, k = -1 -> 255
    one = np.array([[[1, 1, 1]]], np.uint8)                                      # OD 5674 in every channel
    for num, level in ((6384, 1), (6385, 0), (6386, 0), (0, 255), (-1, 255), (5674, 1)):
        a = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
        a[0][0] = int(np.ceil(num * 4096 / 5674)) if num > 0 else num
        k = (5674 * a[0][0] + 2048) >> 12
        got = recolored(gpu(one), 1, a)
        assert got[0, 0, 0] == ref.exp_lut()[min(max(k, 0), 6385)] and got[0, 0, 1] == 255 and (k != num or got[0, 0, 0] == level)


def test_recolor_with_the_identity():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for pix in (grey, random_case((127, 129))):
        for order in (0, 1):
            assert np.array_equal(recolored(gpu(np.array(pix)), order, IDENTITY), np.maximum(pix, 1))
        assert np.array_equal(nuclei.recolor(gpu(np.array(pix)), np.array(IDENTITY)).cpu().numpy(), np.maximum(pix, 1))


# ------------------------------------------------------------------ strides and bases
def test_strided_tiles_and_unaligned_bases():
    pix = random_case((128, 128))
    image = gpu(np.array(pix))
    sub = image[::2, 1::3]
    assert not sub.is_contiguous()
    check_both(pix[::2, 1::3], 0, image=sub)
    planar = image.permute(2, 0, 1).contiguous().permute(1, 2, 0)               # channel planes
    assert not planar.is_contiguous()
    check_both(pix, 1, image=planar)
    start = image[:, 1:]                                                         # a tile sliced to start one pixel in
    assert start.data_ptr() % 4 == 3 and not start.is_contiguous()
    check_both(pix[:, 1:], 0, image=start)
    for offset in (1, 2, 3):                                                     # a contiguous tile whose base is no multiple of 4 bytes
        H, W = 37, 23
        raw = torch.zeros(offset + H * W * 3 + 8, dtype=torch.uint8, device=DEV)
        view = raw[offset:offset + H * W * 3].view(H, W, 3)
        part = pix[:H, :W]
        view.copy_(gpu(np.array(part)))
        assert view.is_contiguous() and view.data_ptr() % 4 == offset
        check_both(part, 0, image=view)
        check_both(part, 1, image=view, names=('steep',))
        assert int(raw[:offset].sum()) == 0 and int(raw[offset + H * W * 3:].sum()) == 0


def test_an_output_base_off_the_dword_through_the_c_abi():
    """The kernel table always hands the library an aligned output; only the C ABI reaches the byte stores of an output whose base
    is no multiple of 4 bytes.  Every pixel, and the bytes around the output stay untouched."""
    import ctypes
    tab = table()
    lut = (ctypes.c_int * 256)(*LUT)
    exp = (ctypes.c_int * len(EXP))(*EXP)
    ws = torch.empty(int(tab.lib.cgc_od_recolor_ws_bytes()), dtype=torch.uint8, device=DEV)
    for shape, a in (((37, 23), MATRICES['normalise']), ((1, 5), MATRICES['steep']), ((128, 128), MATRICES['stains'])):
        pix = random_case((128, 128))[:shape[0], :shape[1]]
        image = gpu(np.array(pix))
        n = shape[0] * shape[1]
        want = ref.od_recolor(pix, 0, ref.od_lut(), a, ref.exp_lut())
        flat = (ctypes.c_int * 9)(*[v for row in a for v in row])
        for offset in (1, 2, 3):
            raw = torch.full((offset + 3 * n + 8,), 77, dtype=torch.uint8, device=DEV)
            assert raw.data_ptr() % 4 == 0
            rc = tab.lib.cgc_od_recolor(image.data_ptr(), ctypes.c_int64(n), 0, lut, flat, exp, len(EXP), ws.data_ptr(),
                                        raw.data_ptr() + offset, tab._stream())
            assert rc == 0
            got = raw.cpu().numpy()
            assert np.array_equal(got[offset:offset + 3 * n].reshape(want.shape), want), (shape, offset)
            assert (got[:offset] == 77).all() and (got[offset + 3 * n:] == 77).all()


# ------------------------------------------------------------------ within
@pytest.mark.parametrize('dtype', [torch.bool, torch.uint8, torch.int32, torch.int64])
def test_within_dtypes(dtype):
    pix = random_case((127, 129))
    image = gpu(np.array(pix))
    rng = np.random.RandomState(9)
    mask = rng.rand(127, 129) < 0.6
    values = np.where(mask, rng.randint(1, 100, mask.shape), 0)
    if dtype in (torch.int32, torch.int64):
        values = np.where(mask & (rng.rand(*mask.shape) < 0.5), {torch.int32: 2 ** 16, torch.int64: 2 ** 40}[dtype], values)
    w = torch.from_numpy(values.astype(np.int64)).to(DEV).to(dtype)
    assert check_both(pix, 0, 154, within=mask, image=image, within_gpu=w) > 0
    nothing = torch.zeros(127, 129, dtype=dtype, device=DEV)                     # a within that selects nothing
    assert check_both(pix, 1, 0, within=np.zeros(mask.shape, bool), image=image, within_gpu=nothing) == 0
    wide = torch.from_numpy(np.repeat(values, 2, axis=1).astype(np.int64)).to(DEV).to(dtype)      # a strided within
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    check_both(pix, 0, 0, within=mask, image=image, within_gpu=strided, names=('steep',))
    odd = random_case((1, 5))                                                    # the tail of a lane, and a within base off the dword
    m = np.array([[True, False, True, True, True]])
    buf = torch.zeros(1 + 5, dtype=dtype, device=DEV)
    wv = buf[1:].view(1, 5)
    wv.copy_(torch.from_numpy(m).to(DEV).to(dtype))
    assert check_both(odd, 0, 0, within=m, within_gpu=wv) == 4


# ------------------------------------------------------------------ the refusals on the device path
def test_the_tables_are_checked_on_the_device_path_too():
    image = gpu(np.array(random_case((1, 5))))
    with pytest.raises(ValueError):
        table().concentration_histogram(image, 0, LUT, 154, [[REACH_CONC + 1, 0, 0], [0, 1, 0], [0, 0, 1]])
    with pytest.raises(ValueError):
        table().concentration_histogram(image, 0, LUT, 5675, MATRICES['stains'])
    with pytest.raises(ValueError):
        table().od_recolor(image, 0, LUT, [[REACH_RECOLOR + 1, 0, 0], [0, 1, 0], [0, 0, 1]], EXP)
    for bad in (EXP[:-1], EXP[::-1], (254,) + EXP[1:], EXP[:-1] + (1,)):
        with pytest.raises(ValueError):
            table().od_recolor(image, 0, LUT, IDENTITY, bad)
    with pytest.raises(ValueError):
        nuclei.recolor(image, [[REACH_RECOLOR + 1, 0, 0], [0, 1, 0], [0, 0, 1]])
    # a caller's own table of the accepted kind, as a list: a step at the middle level
    step = [255] * 3000 + [0] * 3386
    want = ref.od_recolor(random_case((127, 129)), 0, ref.od_lut(), MATRICES['normalise'], step)
    got = table().od_recolor(gpu(np.array(random_case((127, 129)))), 0, LUT, MATRICES['normalise'], step)
    assert np.array_equal(got.cpu().numpy(), want) and set(np.unique(want)) == {0, 255}
    assert np.array_equal(recolored(image, 0, IDENTITY), np.maximum(random_case((1, 5)), 1))       # and the package's table again


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize('pair', [0, 1])
@pytest.mark.parametrize('shape', macenko_ref.TILE_SHAPES)
def test_normalize_stains_on_rendered_tiles(shape, pair):
    tile, S_ref, want, info_ref = ref.normalized_case(shape, pair)
    image = gpu(np.array(tile))

    def same_info(info, other):
        assert set(info) == {'stains', 'maxima', 'bins', 'n', 'matrix'}
        assert isinstance(info['stains'], np.ndarray) and info['stains'].dtype == np.float64 and np.array_equal(info['stains'], other['stains'])
        assert info['maxima'] == other['maxima'] and all(isinstance(v, Fraction) for v in info['maxima'])
        assert info['bins'] == other['bins'] and info['n'] == other['n']
        assert info['matrix'].dtype == np.int32 and np.array_equal(info['matrix'], other['matrix'])

    # estimated stains
    out, info = nuclei.normalize_stains(image, return_info=True)
    assert out.dtype == torch.uint8 and out.shape == image.shape and out.is_contiguous() and out.device == image.device
    same_info(info, info_ref)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(nuclei.normalize_stains(image).cpu().numpy(), want)    # twice: the workspace is new every time
    assert np.array_equal(nuclei.normalize_stains(image.flip(2), order='rgb').cpu().numpy(), want[..., ::-1])
    # the steps one by one
    assert nuclei.stain_maxima(image, S_ref) == info_ref['maxima'] == ref.stain_maxima(tile, S_ref)[0]
    a = nuclei.recolor_matrix(S_ref, info_ref['maxima'])
    assert np.array_equal(a, info_ref['matrix'])
    assert np.array_equal(nuclei.recolor(image, a).cpu().numpy(), want)
    # given stains, other targets, every pixel selected
    for kw in (dict(stains=ref.DEFAULT_STAINS), dict(stains=S_ref, beta=0, alpha=0.5),
               dict(stains=S_ref, target_stains=ref.DEFAULT_STAINS, target_max=(1.5, 1.25))):
        want_kw, info_kw = ref.normalize(tile, **kw)
        out, info = nuclei.normalize_stains(image, return_info=True, **kw)
        same_info(info, info_kw)
        assert np.array_equal(out.cpu().numpy(), want_kw), kw
        assert np.array_equal(nuclei.normalize_stains(image, **kw).cpu().numpy(), want_kw)
        assert nuclei.stain_maxima(image, kw['stains'], alpha=kw.get('alpha', 1.0), beta=kw.get('beta', 0.15)) == info_kw['maxima']


def test_normalize_stains_with_within_and_its_refusals():
    tile = macenko_ref.rendered_tile((96, 80), 1)
    image = gpu(np.array(tile))
    within = np.zeros((96, 80), bool)
    within[5:90, 3:70] = True
    for kw in (dict(beta=0.15, alpha=1.0), dict(beta=0.3, alpha=5), dict(beta=0.1, alpha=0)):
        want, info_ref = ref.normalize(tile, within=within, **kw)
        out, info = nuclei.normalize_stains(image, within=gpu(within), return_info=True, **kw)
        assert info['bins'] == info_ref['bins'] and info['n'] == info_ref['n'] and np.array_equal(info['matrix'], info_ref['matrix']), kw
        assert np.array_equal(out.cpu().numpy(), want), kw
    with pytest.raises(ValueError, match='too few stained pixels'):
        nuclei.normalize_stains(image, within=gpu(np.zeros((96, 80), bool)))
    with pytest.raises(ValueError, match='no stained pixel'):
        nuclei.normalize_stains(image, stains=ref.DEFAULT_STAINS, within=gpu(np.zeros((96, 80), bool)))
    with pytest.raises(ValueError, match='no stained pixel'):
        nuclei.stain_maxima(gpu(np.full((9, 9, 3), 255, np.uint8)))
    with pytest.raises(ValueError, match='none of stain'):
        nuclei.stain_maxima(gpu(np.full((9, 9, 3), 255, np.uint8)), beta=0)
    with pytest.raises(ValueError, match='saturated'):                           # black in one channel: 5.54 units of a stain along it
        nuclei.stain_maxima(gpu(np.full((9, 9, 3), 1, np.uint8)), [[1, 0, 0], [0, 1, 0], [0, 0, 1]])


def test_normalized_tile_feeds_the_stage():
    """The two lines of the documents: the foreground map and the gray image are taken from the normalised tile."""
    tile, _, want, _ = ref.normalized_case((200, 160), 1)
    norm = nuclei.normalize_stains(gpu(np.array(tile)))
    T3 = ref.target_matrix()
    fg, t, plane = nuclei.stain_foreground(norm, stains=T3)
    import stain_ref
    want_fg, want_t, want_plane = stain_ref.stain_foreground(want, stains=T3)
    assert t == want_t and np.array_equal(plane.cpu().numpy(), want_plane) and np.array_equal(fg.cpu().numpy(), want_fg)
    assert 0.05 < float(fg.float().mean()) < 0.95
    gray = nuclei.bgr_to_gray(norm)
    assert gray.shape == norm.shape[:2] and gray.dtype == torch.uint8
