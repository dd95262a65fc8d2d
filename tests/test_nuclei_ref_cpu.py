"""The CPU restatement of the nucleus-feature stage (tests/nuclei_ref.py) against closed forms, and the host-side helpers of
cgc_net_amd.nuclei.  No GPU needed."""
import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import nuclei_ref as ref

COL = {k: i for i, k in enumerate(nuclei.FEATURE_NAMES)}


def _image(H=64, W=64, fill=50):
    return np.zeros((H, W), np.int64), np.full((H, W), fill, np.uint8)


@pytest.mark.parametrize('w,h', [(7, 5), (12, 12), (3, 9)])
def test_rectangle_closed_forms(w, h):
    labels, gray = _image()
    labels[20:20 + h, 30:30 + w] = 7
    rng = np.random.RandomState(w * h)
    gray[:] = rng.randint(1, 255, size=gray.shape)
    f, c, kept, info = ref.nucleus_features(labels, gray)
    assert kept.tolist() == [7] and info[0].tolist() == [0, 0, 4]
    r = f[0]
    assert r[COL['area']] == (w - 1) * (h - 1)
    assert r[COL['perimeter']] == 2 * (w - 1 + h - 1)
    assert r[COL['solidity']] == 1
    assert r[COL['majoraxis_length']] == 1 and r[COL['minoraxis_length']] == 1 and r[COL['orientation']] == 0
    assert r[COL['eccentricity']] == 0
    assert np.allclose(c[0], [20 + (h - 1) / 2, 30 + (w - 1) / 2])


def test_constant_image():
    labels, gray = _image(fill=90)
    labels[10:20, 10:25] = 3
    f, _, _, _ = ref.nucleus_features(labels, gray)
    r = f[0]
    assert r[COL['mean_ent']] == 0 and r[COL['skew_im']] == 0 and r[COL['var_im']] == 0
    assert r[COL['glcm_homogeneity']] == 1 and r[COL['glcm_ASM']] == 1 and r[COL['glcm_energy']] == 1
    assert r[COL['glcm_dissimilarity']] == 0 and abs(r[COL['mean_im_out']] - 90) < 1e-4 and r[COL['diff']] < 1e-4


def test_two_level_stripes():
    labels, gray = _image()
    labels[10:14, 10:16] = 1                     # 4 rows x 6 columns
    gray[:, 10:16:2], gray[:, 11:16:2] = 10, 20  # per row: 10 20 10 20 10 20 -> pairs (10,20) x3, (20,10) x2
    f, _, _, _ = ref.nucleus_features(labels, gray)
    r = f[0]
    assert r[COL['glcm_dissimilarity']] == pytest.approx(10.0)
    assert r[COL['glcm_homogeneity']] == pytest.approx(1 / 101)
    assert r[COL['glcm_ASM']] == pytest.approx(0.6 ** 2 + 0.4 ** 2)
    assert r[COL['glcm_energy']] == pytest.approx(np.sqrt(0.52))
    assert r[COL['mean_im_out']] == pytest.approx(15.0) and r[COL['var_im']] == pytest.approx(25.0)


def test_small_label_removed_and_background_for_neighbour():
    labels, gray = _image()
    labels[10:20, 10:20] = 4                     # 100 px, crop rows 10..20, columns 10..20
    labels[12:15, 20:23] = 9                     # 9 px: removed; its column 20 lies in the crop of label 4
    gray[labels == 4], gray[labels == 9] = 100, 200
    f, _, kept, info = ref.nucleus_features(labels, gray)
    assert kept.tolist() == [4] and info[0].tolist() == [0, 0, 4]
    bg = (18 * 50 + 3 * 200) / (21 + 1e-8)
    assert f[0, COL['diff']] == pytest.approx(100 * 100 / (100 + 1e-8) - bg, rel=1e-6)
    f9, _, kept9, _ = ref.nucleus_features(labels, gray, min_size=9)
    assert kept9.tolist() == [4, 9]
    with pytest.raises(ValueError):
        ref.nucleus_features(np.full((4, 4), -1), np.zeros((4, 4), np.uint8))


def test_neighbour_fragment_is_the_contour():
    labels, gray = _image()
    labels[10:20, 10:19] = 1                     # columns 10..18
    labels[10:13, 19] = 1                        # column 19 only in rows 10..12: the crop ends at row 20, column 20
    labels[18:26, 20:30] = 2                     # a neighbour: (18..20, 20) lie in label 1's crop, not 8-adjacent to label 1
    _, _, kept, info = ref.nucleus_features(labels, gray)
    assert kept.tolist() == [1, 2]
    assert info[0].tolist() == [8, 10, 2]        # the 3-pixel vertical fragment of label 2: 2 vertices
    crop = labels[10:21, 10:21] > 0
    assert ref.choose_contour(crop) == (8, 10)


def test_ring_with_inner_nucleus():
    labels, gray = _image()
    labels[10:31, 10:31] = 5
    labels[15:26, 15:26] = 0                     # the hole
    labels[18:23, 18:23] = 6                     # a nucleus inside it
    _, _, kept, info = ref.nucleus_features(labels, gray)
    assert kept.tolist() == [5, 6]
    assert info[0].tolist() == [0, 0, 4]         # the ring's outer border, not the later-starting inner nucleus (not top-level)
    assert info[1].tolist() == [0, 0, 4]


@pytest.mark.parametrize('phi', [0, 30, 90, 135])
def test_digitised_ellipse_axes_and_orientation(phi):
    H = W = 120
    a, b = 30.0, 14.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    t = np.deg2rad(phi)
    dx, dy = xx - 60.3, yy - 59.6
    u, v = dx * np.cos(t) + dy * np.sin(t), -dx * np.sin(t) + dy * np.cos(t)
    labels = ((u / a) ** 2 + (v / b) ** 2 <= 1).astype(np.int64) * 3
    f, _, _, info = ref.nucleus_features(labels, np.full((H, W), 80, np.uint8))
    r = f[0]
    assert info[0, 2] > 4
    assert abs(r[COL['majoraxis_length']] / (2 * a) - 1) < 0.04
    assert abs(r[COL['minoraxis_length']] / (2 * b) - 1) < 0.06
    d = abs(float(r[COL['orientation']]) - (phi + 90) % 180) % 180
    assert min(d, 180 - d) < 2.0, (r[COL['orientation']], phi)


def test_bgr_to_gray_values():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [10, 20, 30]]], np.uint8)
    assert ref.bgr_to_gray(px).tolist() == [[29, 150, 76, 255, 0, (1868 * 10 + 9617 * 20 + 4899 * 30 + 8192) >> 14]]


def test_entropy_closed_form():
    gray = np.zeros((9, 9), np.uint8)
    gray[:, 5:] = 1                              # at the centre (4, 4): columns 1..4 hold 0, columns 5..7 hold 1 under the disk
    under = [gray[4 + dy, 4 + dx] for dy, dx in ref.DISK3]
    p = np.bincount(under) / 29.0
    assert ref.entropy_at(gray, np.array([4]), np.array([4]))[0] == pytest.approx(-(p * np.log2(p)).sum())
    corner = ref.entropy_at(gray, np.array([0]), np.array([0]))[0]
    assert corner == 0.0                         # 10 in-image pixels, all 0


def test_synthetic_tissue_has_every_case():
    labels, gray = nuclei.synthetic_tissue(512, 512, 120, seed=3)
    assert labels.dtype == np.int32 and gray.dtype == np.uint8 and labels.shape == gray.shape == (512, 512)
    ids = np.unique(labels[labels > 0])
    assert ids.size > 80 and ids.max() > ids.size                               # gaps in the label values
    counts = np.bincount(labels.ravel())
    assert ((counts[ids] < 10)).any()                                            # objects under 10 px
    for edge in (labels[0], labels[-1], labels[:, 0], labels[:, -1]):
        assert (edge > 0).any()                                                  # every image edge cuts a nucleus
    pieces = [ndi_count(labels == L) for L in ids]
    assert max(pieces) > 1                                                       # a label in several pieces
    assert (gray == 0).any() or gray.min() < 20


def ndi_count(m):
    from scipy import ndimage
    return ndimage.label(m, structure=np.ones((3, 3), int))[1]


def test_graph_item_and_reference_files(tmp_path):
    f = torch.arange(3 * 16, dtype=torch.float32).view(3, 16)
    c = torch.tensor([[1.5, 2.0], [3.0, 4.5], [5.0, 6.0]])
    d = nuclei.graph_item(f, c, 2)
    assert d.x.shape == (3, 18) and torch.equal(d.x[:, 16:], c) and torch.equal(d.pos, c) and d.y.tolist() == [2]
    pf, pc = nuclei.save_reference_files(str(tmp_path), 'colorectal', 'fold_1/1_normal', 'img_001.npy', f, c)
    assert pf.endswith('feature/colorectal/fold_1/1_normal/img_001.npy') and np.array_equal(np.load(pf), f.numpy())
    assert np.load(pc).dtype == np.float32 and np.array_equal(np.load(pc), c.numpy())


def test_inputs_are_checked_before_any_launch():
    with pytest.raises(ValueError):
        nuclei.nucleus_features(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(TypeError):
        nuclei.nucleus_features(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        nuclei.nucleus_features(torch.full((4, 4), -2, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.uint8))
