"""Connected-component labelling on the GPU (csrc/label.hip through cgc_net_amd.nuclei.label_instances) against tests/label_ref.py
(scipy.ndimage.label; pinned to a flood fill by tests/test_label_ref_cpu.py).  Every comparison is exact.

The kernels work on 64 x 64 tiles and number the components in blocks of 2048 consecutive raster indices: the shapes below sit under
one tile, on one tile exactly, one pixel over it in either direction, on several ragged tiles, and one pixel over a numbering block."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import label_ref as ref
import nuclei_ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
C = {k: i for i, k in enumerate(nuclei.FEATURE_NAMES)}

SHAPES = [(1, 1), (1, 37), (41, 1), (7, 5), (31, 33), (64, 64), (65, 63), (64, 65), (65, 64), (7, 293), (67, 131), (129, 257), (300, 300)]
DENSITIES = [0.0, 0.2, 0.45, 0.59, 0.75, 1.0]


def _gpu(image, connectivity=1, min_size=0):
    t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image)).to(DEV)
    labels, n, sizes = nuclei.label_instances(t, connectivity, min_size, return_sizes=True)
    assert labels.dtype == torch.int32 and labels.device == t.device and tuple(labels.shape) == tuple(t.shape)
    assert type(n) is int and sizes.dtype == torch.int32 and tuple(sizes.shape) == (n,)
    return labels.cpu().numpy(), n, sizes.cpu().numpy()


def check(image, connectivity, min_size=0):
    lab, n, sizes = _gpu(image, connectivity, min_size)
    rlab, rn, rsizes = ref.label(np.asarray(image), connectivity, min_size)
    assert n == rn, (n, rn)
    assert np.array_equal(lab, rlab), np.argwhere(lab != rlab)[:5]
    assert np.array_equal(sizes, rsizes)
    assert np.array_equal(sizes, np.bincount(lab.ravel(), minlength=n + 1)[1:])
    plain, pn = nuclei.label_instances(torch.from_numpy(np.ascontiguousarray(image)).to(DEV), connectivity, min_size)
    assert pn == n and np.array_equal(plain.cpu().numpy(), lab)         # without the size table: another workspace layout
    return lab, n, sizes


# ------------------------------------------------------------------ random masks
@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_masks(shape, connectivity):
    for density in DENSITIES:
        for seed in (0, 1):
            img = np.random.RandomState(1000 * seed + int(100 * density)).rand(*shape) < density
            lab, n, _ = check(img, connectivity)
            want, wn = ndimage.label(img, structure=ref.STRUCTURES[connectivity])       # scipy itself, bit for bit
            assert n == wn and np.array_equal(lab, want)


# ------------------------------------------------------------------ structured masks
def serpentine(H, W):
    img = np.zeros((H, W), bool)
    img[0::2] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        img[y, W - 1 if k % 2 == 0 else 0] = True
    return img


def spiral(N):
    img = np.zeros((N, N), bool)
    y = x = 0
    dy, dx = 0, 1
    img[0, 0] = True
    while True:
        steps = 0
        while True:
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx           # stop one short of a painted cell, so that the arms stay one background pixel apart
            if not (0 <= ny < N and 0 <= nx < N) or img[ny, nx] or (0 <= ay < N and 0 <= ax < N and img[ay, ax]):
                break
            y, x = ny, nx
            img[y, x] = True
            steps += 1
        if steps < 2:
            return img
        dy, dx = dx, -dy


def comb(H, W):
    img = np.zeros((H, W), bool)
    img[H - 1] = True
    img[:, 0::2] = True
    return img


def prongs(H, W):
    img = np.zeros((H, W), bool)
    img[:, 3] = True
    img[:, W - 4] = True
    img[H - 1, 3:W - 3] = True
    return img


def rings(N):
    img = np.zeros((N, N), bool)
    for k in range(0, N // 2, 2):
        img[k, k:N - k] = img[N - 1 - k, k:N - k] = True
        img[k:N - k, k] = img[k:N - k, N - 1 - k] = True
    return img


@pytest.mark.parametrize('connectivity', [1, 2])
def test_serpentine_spiral_comb_are_one_component(connectivity):
    for img in (serpentine(299, 300), serpentine(300, 131), spiral(300), spiral(131), comb(300, 299), comb(67, 300)):
        lab, n, sizes = check(img, connectivity)
        assert n == 1 and sizes[0] == img.sum()


@pytest.mark.parametrize('connectivity', [1, 2])
def test_prongs_take_the_number_of_the_left_first_pixel(connectivity):
    img = prongs(300, 300)
    img[0, 150] = True                          # a second component whose first pixel lies between the prongs' first pixels
    lab, n, _ = check(img, connectivity)
    assert n == 2 and lab[0, 3] == 1 and lab[0, 296] == 1 and lab[0, 150] == 2


@pytest.mark.parametrize('connectivity', [1, 2])
def test_concentric_rings_are_numbered_by_their_top_left_corners(connectivity):
    img = rings(300)
    lab, n, _ = check(img, connectivity)
    assert n == 75 and all(lab[k, k] == k // 2 + 1 for k in range(0, 150, 2))


def test_checkerboard():
    img = (np.add.outer(np.arange(64), np.arange(64)) % 2 == 0)
    lab, n, sizes = check(img, 1)
    assert n == 2048 and np.array_equal(lab[img], np.arange(1, 2049)) and (sizes == 1).all()
    lab, n, sizes = check(img, 2)
    assert n == 1 and sizes[0] == 2048
    big = (np.add.outer(np.arange(130), np.arange(131)) % 2 == 1)          # across tile corners
    assert check(big, 2)[1] == 1 and check(big, 1)[1] == big.sum()


def test_diagonals():
    N = 300
    main, anti = np.eye(N, dtype=bool), np.eye(N, dtype=bool)[:, ::-1].copy()
    for img in (main, anti):
        assert check(img, 2)[1] == 1
        lab, n, _ = check(img, 1)
        assert n == N and np.array_equal(lab[img], np.arange(1, N + 1))
    both = main | anti
    assert check(both, 2)[1] == 1


# ------------------------------------------------------------------ integer images
@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('seed', [0, 1])
def test_tissue_is_split_into_connected_pieces(seed, connectivity):
    labels0, _ = nuclei.synthetic_tissue(512, 512, 120, seed)
    lab, n, _ = check(labels0, connectivity)
    assert n >= np.unique(labels0[labels0 > 0]).size
    assert np.array_equal(lab > 0, labels0 > 0)
    first = np.unique(lab, return_index=True)[1][1:]
    assert (np.diff(first) > 0).all()                                       # numbered by first raster index
    for k in (1, n // 2, n):
        assert np.unique(labels0[lab == k]).size == 1                      # never merges two values


@pytest.mark.parametrize('connectivity', [1, 2])
def test_hand_made_values(connectivity):
    img = np.zeros((20, 140), np.int32)
    img[2:6, 3:9] = 7
    img[10:15, 100:130] = 7                                                 # the same value, apart
    img[2:6, 9:12] = 4                                                      # shares an edge with the first rectangle
    lab, n, sizes = check(img, connectivity)
    assert n == 3 and lab[2, 3] == 1 and lab[2, 9] == 2 and lab[10, 100] == 3 and sizes.tolist() == [24, 12, 150]
    neg = np.zeros((8, 70), np.int32)
    neg[1, 1:5] = -1
    neg[1, 5:9] = 1                                                         # negative: foreground, apart from the positive run
    neg[2, 60:68] = -2
    neg[3, 60:68] = -2 ** 31
    lab, n, _ = check(neg, connectivity)
    assert n == 4 and lab[1, 1] == 1 and lab[1, 5] == 2 and lab[2, 60] == 3 and lab[3, 60] == 4
    wide = np.zeros((4, 6), np.int64)
    wide[1, 1:3] = 5
    wide[1, 3:5] = 5 + 2 ** 32                                              # equal in their low 32 bits only
    wide[3, 0] = 2 ** 40                                                    # zero in its low 32 bits
    lab, n, _ = check(wide, connectivity)
    assert n == 3 and lab[3, 0] == 3


# ------------------------------------------------------------------ min_size and sizes
@pytest.mark.parametrize('connectivity', [1, 2])
def test_min_size_and_sizes(connectivity):
    mask = np.random.RandomState(5).rand(257, 129) < 0.45
    tissue, _ = nuclei.synthetic_tissue(512, 512, 120, 0)
    for img in (mask, tissue):
        base = check(img, connectivity, 0)
        one = check(img, connectivity, 1)
        assert one[1] == base[1] and np.array_equal(one[0], base[0]) and np.array_equal(one[2], base[2])
        for min_size in (2, 10):
            lab, n, sizes = check(img, connectivity, min_size)
            assert n == int((base[2] >= min_size).sum()) and (sizes >= min_size).all()
            assert np.array_equal(sizes, base[2][base[2] >= min_size])


# ------------------------------------------------------------------ dtypes, strides, empties, refusals
def test_dtypes_and_strides():
    mask = np.random.RandomState(9).rand(131, 67) < 0.5
    want = _gpu(mask, 2)
    for dt in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        got = _gpu(torch.from_numpy(mask).to(DEV).to(dt), 2)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), dt
    t = torch.from_numpy(mask).to(DEV).to(torch.int16)
    view = t.t()
    assert not view.is_contiguous()
    a, b = _gpu(view, 1), _gpu(view.contiguous(), 1)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[0], ref.label(mask.T, 1)[0])
    step = torch.from_numpy(mask).to(DEV)[::2, 1::3]
    assert np.array_equal(_gpu(step, 2)[0], ref.label(mask[::2, 1::3], 2)[0])


def test_empty_inputs():
    for shape in ((0, 0), (0, 17), (9, 0)):
        labels, n, sizes = nuclei.label_instances(torch.zeros(shape, dtype=torch.uint8, device=DEV), return_sizes=True)
        assert tuple(labels.shape) == shape and labels.dtype == torch.int32 and n == 0 and sizes.numel() == 0
    labels, n = nuclei.label_instances(torch.zeros(70, 70, dtype=torch.bool, device=DEV), 2, 3)
    assert n == 0 and labels.dtype == torch.int32 and not labels.any().item()


def test_refusals():
    ok = torch.ones(4, 4, dtype=torch.uint8, device=DEV)
    for bad in (np.ones((4, 4), np.uint8), ok.cpu(), ok.float(), ok.double(), ok.half()):
        with pytest.raises(TypeError):
            nuclei.label_instances(bad)
    for bad in (ok[0], ok[None]):
        with pytest.raises(ValueError):
            nuclei.label_instances(bad)
    for c in (0, 3, 8):
        with pytest.raises(ValueError):
            nuclei.label_instances(ok, connectivity=c)
    with pytest.raises(ValueError):
        nuclei.label_instances(ok, min_size=-1)
    huge = torch.zeros(1, 1, dtype=torch.uint8, device=DEV).expand(2 ** 16, 2 ** 15)      # 2^31 pixels, one byte behind them
    with pytest.raises(ValueError):
        nuclei.label_instances(huge)


# ------------------------------------------------------------------ components that span the whole chip
@pytest.mark.parametrize('density,connectivity', [(0.59, 1), (0.41, 2)])
def test_percolating_clusters_across_all_tiles(density, connectivity):
    img = np.random.RandomState(17).rand(2048, 2048) < density
    t = torch.from_numpy(img).to(DEV)
    a, na = nuclei.label_instances(t, connectivity)
    b, nb = nuclei.label_instances(t, connectivity)
    want, wn = ndimage.label(img, structure=ref.STRUCTURES[connectivity])
    assert na == wn and nb == wn
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), want)
    assert np.bincount(want.ravel())[1:].max() > 2048 * 64                  # a cluster far larger than a row of tiles is in there


# ------------------------------------------------------------------ into the feature stage
def _ulp_close(a, b, n=1):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    tol = n * np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol


def test_pipeline_into_nucleus_features():
    labels0, gray = nuclei.synthetic_tissue(1024, 1024, 500)
    g = torch.from_numpy(gray).to(DEV)
    L, n = nuclei.label_instances(torch.from_numpy(labels0 > 0).to(DEV))
    want = ndimage.label(labels0 > 0)[0].astype(np.int32)
    assert np.array_equal(L.cpu().numpy(), want)
    f, c, k, info = (x.cpu().numpy() for x in nuclei.nucleus_features(L, g, return_info=True, max_label=n))
    rf, rc, rk, rinfo = nuclei_ref.nucleus_features(want, gray, min_size=10)
    # the per-column bars of tests/nuclei_cases.py::check_against_reference, restated
    assert f.shape == rf.shape and np.array_equal(k, rk)
    assert np.array_equal(info[:, :3], rinfo)
    assert _ulp_close(c, rc).all()
    for name in ('area', 'perimeter', 'solidity', 'mean_im_out', 'diff', 'var_im'):
        assert _ulp_close(f[:, C[name]], rf[:, C[name]]).all(), name
    for name in ('glcm_dissimilarity', 'glcm_homogeneity', 'glcm_energy', 'glcm_ASM'):
        np.testing.assert_allclose(f[:, C[name]], rf[:, C[name]], rtol=1e-6, atol=0, err_msg=name)
    np.testing.assert_allclose(f[:, C['skew_im']], rf[:, C['skew_im']], rtol=0, atol=1e-6)
    np.testing.assert_allclose(f[:, C['mean_ent']], rf[:, C['mean_ent']], rtol=1e-5, atol=0)
    for name in ('majoraxis_length', 'minoraxis_length', 'eccentricity'):
        np.testing.assert_allclose(f[:, C[name]], rf[:, C[name]], rtol=1e-4, atol=1e-6, err_msg=name)
    maj, mnr = rf[:, C['majoraxis_length']].astype(np.float64), rf[:, C['minoraxis_length']].astype(np.float64)
    sel = (maj - mnr) / np.maximum(maj, 1e-30) > 1e-3
    d = np.abs(f[sel, C['orientation']].astype(np.float64) - rf[sel, C['orientation']]) % 180
    assert (np.minimum(d, 180 - d) <= 1e-3).all()
    assert np.isfinite(f).all()
    # max_label only replaces the host read of the label range
    for x, y in zip(nuclei.nucleus_features(L, g, return_info=True, max_label=n), nuclei.nucleus_features(L, g, return_info=True)):
        assert torch.equal(x, y) and np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    for x, y in zip(nuclei.nucleus_features(L, g, max_label=n + 1000), nuclei.nucleus_features(L, g)):
        assert torch.equal(x, y)


def test_max_label_is_checked_against_the_pixels():
    L = torch.zeros(64, 64, dtype=torch.int32, device=DEV)
    g = torch.zeros(64, 64, dtype=torch.uint8, device=DEV)
    assert nuclei.nucleus_features(L, g, max_label=0)[0].shape == (0, 16)
    L[10:20, 10:20] = 3
    assert nuclei.nucleus_features(L, g, max_label=3)[2].tolist() == [3]
    for wrong in (0, 2):
        with pytest.raises(ValueError):
            nuclei.nucleus_features(L, g, max_label=wrong)
    with pytest.raises(ValueError):
        nuclei.nucleus_features(L, g, max_label=-1)
