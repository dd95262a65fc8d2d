"""GPU: stain estimation (csrc/stain.hip k_od_scan; kernels.HipKernels.od_moments / angle_histogram; nuclei.estimate_stains) against
tests/macenko_ref.py.  Integer arithmetic with a stated contract on both sides: every comparison of the reductions is exact, and the
3 x 3 result is compared bit for bit wherever both sides hold the same eigenvectors."""
import functools
import math

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import macenko_ref as ref
import stain_ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

K = ref.K
LUT = nuclei.OD_LUT
DIRS = nuclei.ANGLE_DIRS
# 1-3 tail pixels of a 4-pixel lane; one 16384-pixel chunk and a little; two chunks
SHAPES = [(1, 1), (1, 3), (1, 7), (3, 5), (128, 129), (200, 160)]
OD_MINS = [0, 154, 5674]
BASES = {                                                                        # E[j][c]: both rows within the contract's bounds
    'principal': [[2294, 2949, 1664], [2400, -500, -2300]],                      # e_1 along a typical stain: pixels on both sides of 0
    'negated': [[-2294, -2949, -1664], [2400, -500, -2300]],                     # e_1 negated: every selected pixel is skipped
    'extreme': [[2365, 2365, 2365], [-2365, 2365, -2365]],                       # sum |E| = 7095
    'axis': [[4096, 0, 0], [0, 4096, 0]],
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
    pix = random_tile(shape, 11 + shape[0] + shape[1])
    pix.setflags(write=False)
    return pix


def table():
    return kernels.get()


def moments_of(image, order, od_min, within=None):
    out = table().od_moments(image, order, LUT, od_min, within)
    assert out.dtype == torch.int64 and tuple(out.shape) == (10,) and out.device == image.device
    return out.tolist()


def angles_of(image, order, od_min, basis, within=None, dirs=DIRS):
    out = table().angle_histogram(image, order, LUT, od_min, basis, dirs, within)
    assert out.dtype == torch.int32 and tuple(out.shape) == (K + 1,) and out.device == image.device
    return out.tolist()


def check_both(pix, order, od_min, within=None, image=None, within_gpu=None, bases=('principal',)):
    """Both kernels on one input against the restatement; returns the number of selected pixels."""
    image = gpu(np.array(pix)) if image is None else image
    if within is not None and within_gpu is None:
        within_gpu = gpu(np.array(within))
    lut = ref.od_lut()
    want = ref.od_moments(pix, order, lut, od_min, within)
    assert moments_of(image, order, od_min, within_gpu) == want
    for name in bases:
        hist = ref.angle_histogram(pix, order, lut, od_min, BASES[name], ref.angle_dirs(), within)
        assert int(hist.sum()) == want[0]                                        # every selected pixel is binned or skipped
        assert angles_of(image, order, od_min, BASES[name], within_gpu) == hist.tolist(), name
    return want[0]


# ------------------------------------------------------------------ shapes, orders, thresholds
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('shape', SHAPES)
def test_random_tiles_every_threshold(shape, order):
    pix = random_case(shape)
    assert table().scan_chunk == 16384
    for od_min in OD_MINS:
        check_both(pix, order, od_min, bases=tuple(BASES))
    small = np.array(pix)
    small[..., 1] = np.maximum(small[..., 1], 40)                                # no channel G below 40: od_min 2000 excludes every pixel
    assert check_both(small, order, 2000) == 0


def test_empty_images():
    for shape in ((0, 0), (0, 7), (5, 0)):
        image = torch.zeros(shape + (3,), dtype=torch.uint8, device=DEV)
        assert moments_of(image, 0, 0) == [0] * 10
        assert angles_of(image, 1, 0, BASES['axis']) == [0] * (K + 1)
        assert moments_of(image, 0, 0, torch.zeros(shape, dtype=torch.bool, device=DEV)) == [0] * 10


@pytest.mark.parametrize('value', [0, 1])
def test_flat_tiles_accumulator_width(value):
    """Every lane on one bin, and the largest sums of products: 32000 * 5674^2 = 2^39.9 per product sum, far beyond 32 bits."""
    pix = np.full((200, 160, 3), value, np.uint8)
    image = gpu(pix)
    n = check_both(pix, 0, 154, image=image, bases=('principal', 'extreme', 'negated'))
    assert n == 32000
    got = moments_of(image, 1, 0)
    assert got == [32000] + [32000 * 5674] * 3 + [32000 * 5674 ** 2] * 6 and got[4] > 2 ** 39
    hist = angles_of(image, 0, 0, BASES['extreme'])
    assert max(hist) == 32000 and sum(hist) == 32000 and hist[K] == 0            # one value of p, p_1 = 9828: one bin
    white = gpu(np.full((40, 50, 3), 255, np.uint8))
    assert moments_of(white, 0, 0) == [2000] + [0] * 9
    assert angles_of(white, 0, 0, BASES['principal'])[K] == 2000                 # p = (0, 0): p_1 <= 0, skipped
    assert moments_of(white, 0, 1) == [0] * 10


# ------------------------------------------------------------------ strides and bases
def test_strided_tiles_and_unaligned_bases():
    pix = random_case((128, 129))
    image = gpu(np.array(pix))
    sub = image[::2, 1::3]
    assert not sub.is_contiguous()
    check_both(pix[::2, 1::3], 0, 154, image=sub)
    planar = image.permute(2, 0, 1).contiguous().permute(1, 2, 0)               # channel planes
    assert not planar.is_contiguous()
    check_both(pix, 1, 154, image=planar)
    flipped = image.flip(2)                                                      # BGR seen as RGB
    assert moments_of(flipped, 1, 154) == ref.od_moments(pix, 0, ref.od_lut(), 154)
    for offset in (1, 2, 3):                                                     # a contiguous tile whose base is no multiple of 4 bytes
        H, W = 37, 23
        raw = torch.zeros(offset + H * W * 3 + 8, dtype=torch.uint8, device=DEV)
        view = raw[offset:offset + H * W * 3].view(H, W, 3)
        part = pix[:H, :W]
        view.copy_(gpu(np.array(part)))
        assert view.is_contiguous() and view.data_ptr() % 4 == offset
        check_both(part, 0, 154, image=view)
        check_both(part, 1, 0, image=view, bases=('axis',))


# ------------------------------------------------------------------ within
@pytest.mark.parametrize('dtype', [torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64])
def test_within_dtypes(dtype):
    pix = random_case((128, 129))
    image = gpu(np.array(pix))
    rng = np.random.RandomState(9)
    mask = rng.rand(128, 129) < 0.6
    values = np.where(mask, rng.randint(1, 100, mask.shape), 0)
    if dtype in (torch.int16, torch.int32, torch.int64):
        values = np.where(mask & (rng.rand(*mask.shape) < 0.5), {torch.int16: -2 ** 15, torch.int32: 2 ** 16, torch.int64: 2 ** 40}[dtype],
                          values)                                                # low bytes zero: only "is zero" of the whole value counts
    w = torch.from_numpy(values.astype(np.int64)).to(DEV).to(dtype)
    assert check_both(pix, 0, 154, within=mask, image=image, within_gpu=w) > 0
    nothing = torch.zeros(128, 129, dtype=dtype, device=DEV)
    assert check_both(pix, 1, 0, within=np.zeros(mask.shape, bool), image=image, within_gpu=nothing) == 0
    wide = torch.from_numpy(np.repeat(values, 2, axis=1).astype(np.int64)).to(DEV).to(dtype)      # a strided within
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    check_both(pix, 0, 0, within=mask, image=image, within_gpu=strided, bases=('axis',))
    odd = random_case((3, 5))                                                    # tails of a lane, and a within base off the dword
    m = rng.rand(3, 5) < 0.7
    buf = torch.zeros(1 + 15, dtype=dtype, device=DEV)
    wv = buf[1:].view(3, 5)
    wv.copy_(torch.from_numpy(m).to(DEV).to(dtype))
    check_both(odd, 0, 0, within=m, within_gpu=wv, bases=('axis',))


# ------------------------------------------------------------------ the angle histogram's special cases
def test_negated_basis_skips_every_selected_pixel():
    tile = ref.rendered_tile((96, 80), 0)
    hist = angles_of(gpu(np.array(tile)), 0, 154, BASES['negated'])
    n = ref.od_moments(tile, 0, ref.od_lut(), 154)[0]
    assert n > 1000 and hist[K] == n and sum(hist[:K]) == 0


def test_pixels_on_both_sides_of_zero():
    tile = ref.rendered_tile((96, 80), 0)
    hist = angles_of(gpu(np.array(tile)), 0, 154, BASES['principal'])
    assert hist == ref.angle_histogram(tile, 0, ref.od_lut(), 154, BASES['principal'], ref.angle_dirs()).tolist()
    assert sum(hist[:K // 2]) > 100 and sum(hist[K // 2:K]) > 100 and hist[K] == 0


def test_pixels_exactly_on_a_boundary():
    """p = (c_k, s_k) scaled down is collinear with direction k: the cross product is 0, '>=' holds, the bin is k.  With the RGB order
    and the basis (4096, 0, 0), (0, +-4096, 0), p = (lut[R], +-lut[G]) exactly; the table entries with a common divisor whose reduced
    multiples are values of the OD table in both components make such pixels, on either side of 0."""
    value_of = {od: v for v, od in enumerate(LUT)}
    for sign in (1, -1):
        made = []
        for k, (c, s) in enumerate(DIRS, start=1):
            g = math.gcd(c, abs(s))
            if g == 1 or s * sign < 0:
                continue
            for m in range(1, 5674 * g // max(c, abs(s)) + 1):
                if c // g * m in value_of and abs(s) // g * m in value_of:
                    made.append((k, value_of[c // g * m], value_of[abs(s) // g * m]))
                    break
        assert len(made) >= 5, made
        basis = [[4096, 0, 0], [0, 4096 * sign, 0]]
        pix = np.array([[r, g, 7] for _, r, g in made], np.uint8).reshape(1, len(made), 3)
        p = ref.project(ref.selected_od(pix, 1, ref.od_lut(), 0), basis)
        cross = p[:, 1] * np.array([DIRS[k - 1][0] for k, _, _ in made]) - p[:, 0] * np.array([DIRS[k - 1][1] for k, _, _ in made])
        assert (cross == 0).all() and ref.count_bins(p, ref.angle_dirs()).tolist() == [k for k, _, _ in made]
        want = np.bincount([k for k, _, _ in made], minlength=K + 1)
        assert angles_of(gpu(pix), 1, 0, basis) == want.tolist()
    level = np.array([[[50, 255, 9], [200, 255, 9]]], np.uint8)                  # G = 255: p_2 = 0, on direction 512 = (16384, 0)
    assert angles_of(gpu(level), 1, 0, BASES['axis'])[K // 2] == 2


def test_the_table_is_checked_on_the_device_path_too():
    image = gpu(np.array(random_case((3, 5))))
    d = [list(v) for v in DIRS]
    for bad in (d[:300] + [d[301], d[300]] + d[302:], d[::-1], [[0, -16384]] + d[1:]):
        with pytest.raises(ValueError):
            table().angle_histogram(image, 0, LUT, 0, BASES['axis'], bad)
    with pytest.raises(ValueError):
        table().angle_histogram(image, 0, LUT, 0, [[4097, 0, 0], [0, 1, 0]], DIRS)
    with pytest.raises(ValueError):
        table().od_moments(image, 0, LUT, 5675)
    # a caller's own table of the accepted kind: the same angles on a grid half as fine, so boundaries fall elsewhere
    half = [[int(np.rint(8192.0 * np.cos(t))), int(np.rint(8192.0 * np.sin(t)))] for t in ref.angle_thetas()]
    assert half != [[c // 2, s_ // 2] for c, s_ in d]
    kernels.HipKernels._check_angle_tables(BASES['axis'], half)
    pix = random_case((128, 129))
    want = ref.angle_histogram(pix, 0, ref.od_lut(), 154, BASES['principal'], np.array(half, np.int64))
    assert angles_of(gpu(np.array(pix)), 0, 154, BASES['principal'], dirs=half) == want.tolist()


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize('pair', [0, 1])
@pytest.mark.parametrize('shape', ref.TILE_SHAPES)
def test_estimate_stains_on_rendered_tiles(shape, pair):
    tile, S_ref, info_ref, z, _ = ref.rendered_case(shape, pair)
    image = gpu(np.array(tile))
    mom = moments_of(image, 0, 154)
    assert mom == z['moments']
    assert angles_of(image, 0, 154, z['basis'].tolist()) == z['counts']
    S, info = nuclei.estimate_stains(image, return_info=True)
    assert isinstance(S, np.ndarray) and S.dtype == np.float64 and S.shape == (3, 3)
    # the device moments through the restated host code: eigh is the same call on the same matrix, so the planes are the same bits
    S_fed, info_fed, z_fed = ref.estimate(tile, moments=mom)
    assert info == info_fed == info_ref and set(info) == {'n', 'skipped', 'od_min', 'bins', 'eigenvalues'}
    assert np.array_equal(S, S_fed) and np.array_equal(S, S_ref)
    # ... and given the package's own eigenvectors, whatever eigh is
    n, lam, e1, e2 = nuclei._plane_of_moments(mom)
    basis = [[int(v) for v in np.rint(4096.0 * e)] for e in (e1, e2)]
    S_same, info_same, _ = ref.estimate(tile, moments=mom, counts=angles_of(image, 0, 154, basis), plane=(lam, e1, e2))
    assert np.array_equal(S, S_same) and info == info_same
    assert np.array_equal(nuclei.estimate_stains(image), S)                      # two calls: identical bits
    assert np.array_equal(nuclei.estimate_stains(image.flip(2), order='rgb'), S)
    assert np.allclose((S * S).sum(axis=1), 1.0, atol=1e-12) and S[0, 0] > S[1, 0]


def test_estimate_stains_with_within_beta_alpha():
    tile = ref.rendered_tile((96, 80), 1)
    image = gpu(np.array(tile))
    within = np.zeros((96, 80), bool)
    within[5:90, 3:70] = True
    for kw in (dict(beta=0.15, alpha=1.0), dict(beta=0.3, alpha=5), dict(beta=0.1, alpha=0.5), dict(beta=0, alpha=0)):
        S_ref, info_ref, _ = ref.estimate(tile, 0, kw['beta'], kw['alpha'], within)
        S, info = nuclei.estimate_stains(image, within=gpu(within), return_info=True, **kw)
        assert info == info_ref and np.array_equal(S, S_ref), kw
    with pytest.raises(ValueError, match='too few stained pixels'):
        nuclei.estimate_stains(image, within=gpu(np.zeros((96, 80), bool)))
    with pytest.raises(ValueError, match='too few stained pixels'):
        nuclei.estimate_stains(gpu(np.full((9, 9, 3), 255, np.uint8)))
    with pytest.raises(ValueError, match='one stain only'):
        nuclei.estimate_stains(gpu(np.full((9, 9, 3), 100, np.uint8)))


def test_estimate_stains_feeds_stain_foreground():
    tile, S_ref, _, _, _ = ref.rendered_case((200, 160), 0)
    image = gpu(np.array(tile))
    S = nuclei.estimate_stains(image)
    fg, t, plane = nuclei.stain_foreground(image, stains=S)
    want_fg, want_t, want_plane = stain_ref.stain_foreground(tile, stains=S_ref)
    assert t == want_t and np.array_equal(plane.cpu().numpy(), want_plane) and np.array_equal(fg.cpu().numpy(), want_fg)
    assert 0.05 < float(fg.float().mean()) < 0.95
    with pytest.raises(ValueError):
        nuclei.stain_foreground(image, stains='hed')


def test_uniform_random_bytes_end_to_end():
    pix = random_case((200, 160))
    image = gpu(np.array(pix))
    S_ref, info_ref, _ = ref.estimate(pix)
    S, info = nuclei.estimate_stains(image, return_info=True)
    assert info == info_ref and np.array_equal(S, S_ref)
