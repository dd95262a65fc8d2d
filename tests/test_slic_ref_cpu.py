"""CPU: tests/slic_ref.py, the sequential restatement of superpixels that the GPU tests compare against, pinned against hand-worked
cases and against the properties the contract promises (KernelSpec.slic_iterate, KernelSpec.slic_merge, nuclei.superpixels)."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import slic_ref as ref


def noisy(C, H, W, seed, smooth=0):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (C, H, W)).astype(np.float64)
    if smooth:
        a = ndimage.uniform_filter(a, (0, smooth, smooth), mode='nearest')
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def holed(H, W):
    """A mask with a hole and, cut off from the rest by a ring of zeros, an island."""
    w = np.ones((H, W), np.uint8)
    w[H // 2 - 3:H // 2 + 2, W // 2 - 4:W // 2 + 3] = 0
    w[1:8, 1:8] = 0
    w[3:5, 3:6] = 1
    return w


CASES = [  # planes, S, m, n_iter, min_size, within
    (noisy(1, 9, 9, 0), 8, 10, 3, None, None),
    (noisy(3, 24, 31, 1, 5), 5, 10, 4, None, None),
    (noisy(1, 37, 53, 2), 8, 1, 3, None, None),
    (noisy(2, 30, 26, 3, 3), 6, 40, 5, 7, holed(30, 26)),
    (noisy(1, 20, 33, 4, 3), 16, 10, 2, None, holed(20, 33)),
    (noisy(3, 16, 16, 5), 8, 10, 2, None, None),
]


# ------------------------------------------------------------------ hand-worked
def test_grid_and_start():
    assert ref.grid(8, 8, 4) == (2, 2) and ref.grid(6, 10, 4) == (2, 3) and ref.grid(9, 9, 8) == (1, 1) and ref.grid(5, 40, 8) == (1, 5)
    assert ref.grid(37, 53, 8) == (5, 7) and ref.grid(11, 12, 8) == (1, 2)         # 11 < 1.5 S <= 12
    plane = np.arange(60, dtype=np.uint8).reshape(1, 6, 10)
    assert ref.start_centres(plane, 4) == [[1, 1, 11], [1, 5, 15], [1, 8, 18], [4, 1, 41], [4, 5, 45], [4, 8, 48]]


def test_flat_8x8_ties_go_to_the_smaller_centre():
    """8 x 8 of one value, S = 4, m = 1: centres (2, 2) (2, 6) (6, 2) (6, 6); row 4 and column 4 are as far from 2 as from 6."""
    plane = np.full((1, 8, 8), 7, np.uint8)
    labels, centres, count = ref.iterate(plane, 4, 1, 1)
    rows = np.array([0, 0, 0, 0, 0, 1, 1, 1])
    assert (labels == (rows[:, None] * 2 + rows[None, :] + 1)).all()
    assert labels[4, 4] == 1 and labels[4, 5] == 2 and labels[5, 4] == 3
    assert count.tolist() == [25, 15, 15, 9]
    assert centres.tolist() == [[2, 2, 7], [2, 6, 7], [6, 2, 7], [6, 6, 7]]


def test_6x10_colour_only_an_empty_centre_keeps_its_value():
    """6 x 10, S = 4, m = 0: six centres.  All pixels are 0 but (4, 5), the start of centre 4, which is 200 and masked out: centre
    4 starts with colour 200 and no pixel takes it.  Every other pixel is at D = 0 from every other centre and takes the smallest k
    among its 9 cells: 0 for columns 0..6 (home columns 0 and 1), 1 for columns 7..9."""
    plane = np.zeros((1, 6, 10), np.uint8)
    plane[0, 4, 5] = 200
    within = np.ones((6, 10), np.uint8)
    within[4, 5] = 0
    labels, centres, count = ref.iterate(plane, 4, 0, 1, within)
    want = np.ones((6, 10), np.int32)
    want[:, 7:] = 2
    want[4, 5] = 0
    assert (labels == want).all()
    assert count.tolist() == [41, 18, 0, 0, 0, 0]
    # centre 0: sum y = 7 * 15 - 4 = 101, sum x = 6 * 21 - 5 = 121, n = 41: 243 // 82 = 2, 283 // 82 = 3
    # centre 1: sum y = 45, sum x = 144, n = 18: 108 // 36 = 3 (2.5 rounds up), 306 // 36 = 8
    assert centres.tolist() == [[2, 3, 0], [3, 8, 0], [1, 8, 0], [4, 1, 0], [4, 5, 200], [4, 8, 0]]


def test_the_merge_rule_by_hand():
    """A row of pieces 1 | 2 | 3 | 4: sizes 1, 1, 1, 5.  min_size 2: 3 joins 4 in round 1, 2 in round 2, 1 in round 3."""
    pieces = np.array([[1, 2, 3, 4, 4, 4, 4, 4]], np.int32)
    group, rounds = ref.merge(pieces, 4, 2)
    assert group[1:] == [4, 4, 4, 4] and rounds == 3
    # the largest count wins, then the smallest piece number
    pieces = np.array([[1, 1, 1, 2, 2, 2],
                       [1, 1, 3, 3, 2, 2],
                       [4, 4, 4, 4, 4, 4]], np.int32)
    assert ref.contacts(pieces) == {(1, 2): 1, (1, 3): 2, (1, 4): 2, (2, 3): 2, (2, 4): 2, (3, 4): 2}
    group, rounds = ref.merge(pieces, 4, 3)                     # 3 has 2 pixels: contacts 2 with 1, 2 and 4: the smallest number
    assert group[1:] == [1, 2, 1, 4] and rounds == 1
    group, rounds = ref.merge(pieces, 4, 6)                     # only 4 is settled: 1, 2, 3 all touch it
    assert group[1:] == [4, 4, 4, 4] and rounds == 1
    group, rounds = ref.merge(pieces, 4, 7)                     # nothing is settled, nothing ever is
    assert group[1:] == [0, 0, 0, 0] and rounds == 0


# ------------------------------------------------------------------ properties
@pytest.fixture(scope='module')
def results():
    return [ref.superpixels(p, S, m, it, ms, w, return_info=True) for p, S, m, it, ms, w in CASES]


def test_regions_are_connected_numbered_by_first_pixel_and_large_enough(results):
    for (planes, S, m, it, ms, within), (final, n, info) in zip(CASES, results):
        ms = ref.default_min_size(S) if ms is None else ms
        assert sorted(set(final.ravel().tolist()) - {0}) == list(range(1, n + 1))
        firsts = []
        for v in range(1, n + 1):
            where = final == v
            assert ndimage.label(where, ref.CROSS)[1] == 1, v
            firsts.append(int(np.flatnonzero(where.ravel())[0]))
            assert where.sum() >= ms or v in info['leftovers'], v
        assert firsts == sorted(firsts)
        assert ((final == 0) == ((within == 0) if within is not None else np.zeros_like(final, bool))).all()


def test_leftover_blobs_touch_no_other_region(results):
    seen = 0
    for (final, n, info) in results:
        for v in info['leftovers']:
            seen += 1
            grown = ndimage.binary_dilation(final == v, ref.CROSS)
            assert set(final[grown].tolist()) <= {0, v}
    assert seen >= 1                                            # the islands of `holed`: smaller than min_size


def test_pieces_are_scipy_components_in_raster_order():
    labels = np.array([[1, 1, 2, 2, 1],
                       [3, 1, 2, 1, 1],
                       [3, 3, 0, 2, 2]], np.int32)
    pieces, P = ref.pieces_of(labels)
    assert P == 5 and pieces.tolist() == [[1, 1, 2, 2, 3], [4, 1, 2, 3, 3], [4, 4, 0, 5, 5]]


def test_noise_gives_many_pieces_and_several_rounds():
    planes, S, m, it, ms, within = CASES[2]
    final, n, info = ref.superpixels(planes, S, m, it, return_info=True)
    assert info['P'] > 300 and info['rounds'] >= 3


def test_all_small_pieces_become_one_region_by_rule_e():
    planes = noisy(1, 16, 24, 7)
    final, n, info = ref.superpixels(planes, 8, 10, 1, min_size=10 ** 6, return_info=True)
    assert n == 1 and (final == 1).all() and info['rounds'] == 0 and info['leftovers'] == [1]


def test_two_tones_are_never_mixed():
    plane = np.full((1, 32, 48), 40, np.uint8)
    plane[:, :, 21:] = 200
    final, n = ref.superpixels(plane, 8, 10, 10)
    assert n > 1
    for v in range(1, n + 1):
        assert len(set(plane[0][final == v].tolist())) == 1, v


def test_graph_is_symmetric_and_equals_a_contact_scan(results):
    for final, n, info in results:
        for loop in (True, False):
            e, border = ref.graph(final, n, loop)
            got = {(int(a), int(b)): int(c) for a, b, c in zip(e[0], e[1], border)}
            assert len(got) == e.shape[1] and all((b, a) in got and got[(b, a)] == c for (a, b), c in got.items())
            assert (np.diff(e[0] * max(n, 1) + e[1]) > 0).all()
            want = {}
            H, W = final.shape
            for y in range(H):
                for x in range(W):
                    for yy, xx in ((y, x + 1), (y + 1, x), (y, x - 1), (y - 1, x)):
                        if 0 <= yy < H and 0 <= xx < W and final[y, x] and final[yy, xx] and final[y, x] != final[yy, xx]:
                            key = (final[y, x] - 1, final[yy, xx] - 1)
                            want[key] = want.get(key, 0) + 1
            if loop:
                want.update({(i, i): 0 for i in range(n)})
            assert got == want


# ------------------------------------------------------------------ the host side's numbering, on tables of the restatement
def test_superpixel_numbers_follow_rule_f(results):
    for final, n, info in results:
        pieces, P, group = info['pieces'], info['P'], info['group']
        blobs, nb = ndimage.label((pieces != 0) & (np.array(group)[pieces] == 0), ref.CROSS)
        piece_blob = np.zeros(P + 1, np.int64)
        piece_blob[pieces.ravel()] = blobs.ravel()
        table, count = nuclei._superpixel_numbers(torch.tensor(group, dtype=torch.int32), torch.from_numpy(piece_blob) if nb else None)
        assert int(count) == n and table.dtype == torch.int32 and int(table[0]) == 0
        assert (table.numpy()[pieces] == final).all()


def test_regions_at_rounds_to_the_pixel_under_the_point():
    labels = torch.arange(1, 13, dtype=torch.int32).reshape(3, 4)
    pts = torch.tensor([[0.0, 0.0], [0.49, 0.5], [-0.5, 0.0], [-0.51, 0.0], [2.49, 3.49], [2.5, 0.0], [1.0, 3.5], [1.5, 2.5],
                        [float('nan'), 0.0], [1e12, 1.0]], dtype=torch.float64)
    assert nuclei.regions_at(labels, pts).tolist() == [1, 2, 1, 0, 12, 0, 0, 12, 0, 0]
    assert nuclei.regions_at(labels, pts.to(torch.float32)[:3]).dtype == torch.int32
    assert nuclei.regions_at(labels, torch.zeros(0, 2)).shape == (0,)
    with pytest.raises(TypeError):
        nuclei.regions_at(labels, torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        nuclei.regions_at(labels, torch.zeros(2, 3))
