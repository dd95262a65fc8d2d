"""GPU: superpixels (csrc/slic.hip; cgc_net_amd.nuclei.superpixels, superpixel_graph, superpixel_features, regions_at;
kernels.HipKernels.slic_iterate) against tests/slic_ref.py.  The clustering's labels, centres and counts, the final labels and n must
equal the restatement EXACTLY -- integers, no tolerance -- at the smallest shapes at which each mechanism can fail: sides the step
does not divide, one cell, one row of cells, a side one pixel past the tile's seam (t = the tile side read from the library), steps
small enough that a tile meets more cells than its table in LDS holds (the exact fallback), colour alone and distance alone, ties
everywhere, a merge of several rounds, leftover blobs, strided inputs."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import slic_ref as ref
from image_cases import gpu

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def tile():
    k = kernels.get()
    assert k.slic_tile == k.region_tile
    return k.slic_tile


def noisy(C, H, W, seed, smooth=0):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (C, H, W)).astype(np.float64)
    if smooth:
        a = ndimage.uniform_filter(a, (0, smooth, smooth), mode='nearest')
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def holed(H, W):
    """A mask with a hole and, cut off from the rest by a ring of zeros, an island smaller than any min_size used here."""
    w = np.ones((H, W), np.uint8)
    w[H // 2 - 3:H // 2 + 2, W // 2 - 4:W // 2 + 3] = 0
    w[1:8, 1:8] = 0
    w[3:5, 3:6] = 1
    return w


def spot():
    plane = np.zeros((1, 6, 10), np.uint8)
    plane[0, 4, 5] = 200
    return plane


@functools.lru_cache(maxsize=None)
def case(name):
    """(planes, S, m, n_iter, min_size, within) by name; the restatement of each is computed once (``expected``)."""
    t = tile()
    return {
        'odd sides':      (noisy(1, 37, 53, 2), 8, 1, 3, None, None),                  # noise: hundreds of pieces, a merge of >= 3 rounds
        'long merge':     (noisy(1, 37, 53, 2), 8, 1, 3, 6, None),                     # the same pieces, 12 rounds, 23 regions: the key decides
        'one cell':       (noisy(1, 9, 9, 0), 8, 10, 3, None, None),
        'one row':        (noisy(2, 5, 40, 6, 3), 8, 10, 4, None, None),
        'seam':           (noisy(1, t + 1, t + 1, 8, 5), 8, 10, 2, None, None),        # four tiles, three of them one pixel wide or high
        'small step':     (noisy(1, t + 6, t + 1, 9, 3), 4, 10, 2, None, None),        # t / 4 + 4 cells per axis: past the table
        'four planes':    (noisy(4, 24, 31, 1, 5), 5, 10, 4, None, None),
        'colour only':    (noisy(1, 30, 41, 10, 3), 8, 0, 3, None, None),
        'distance only':  (noisy(3, 26, 30, 11), 6, 1024, 3, None, None),
        'flat':           (np.full((2, 23, 29), 99, np.uint8), 6, 10, 3, None, None),  # every decision is a tie
        'hole, island':   (noisy(2, 30, 26, 3, 3), 6, 40, 5, 7, holed(30, 26)),
        'all small':      (noisy(1, 16, 24, 7), 8, 10, 1, 10 ** 6, None),
        'empty centre':   (spot(), 4, 0, 2, None, spot()[0] == 0),                     # centre 4 starts on the masked spot: no pixel takes it
    }[name]


NAMES = ('odd sides', 'long merge', 'one cell', 'one row', 'seam', 'small step', 'four planes', 'colour only', 'distance only', 'flat', 'hole, island',
         'all small', 'empty centre')


@functools.lru_cache(maxsize=None)
def expected(name):
    planes, S, m, n_iter, min_size, within = case(name)
    clustered = ref.iterate(planes, S, m, n_iter, within)
    final, n, info = ref.connect(clustered[0], ref.default_min_size(S) if min_size is None else min_size, return_info=True)
    return clustered, final, n, info


def same(got, want, what):
    assert got.is_cuda and got.dtype == torch.int32, what
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.cpu().numpy()
    assert np.array_equal(g, want), (what, np.argwhere(g != want)[:4].tolist())


@pytest.mark.parametrize('name', NAMES)
def test_clustering_equals_the_restatement(name):
    planes, S, m, n_iter, min_size, within = case(name)
    (labels, centres, count), _, _, _ = expected(name)
    got = kernels.get().slic_iterate(gpu(planes), S, m, n_iter, None if within is None else gpu(within))
    same(got[0], labels, 'labels')
    same(got[1], centres, 'centres')
    same(got[2], count, 'count')
    assert int(got[2].sum()) == (planes[0].size if within is None else int((within != 0).sum()))


@pytest.mark.parametrize('name', NAMES)
def test_superpixels_equal_the_restatement(name):
    planes, S, m, n_iter, min_size, within = case(name)
    (labels, centres, count), final, n, info = expected(name)
    got, got_n, (got_centres, got_count) = nuclei.superpixels(gpu(planes), S, m, n_iter, min_size, None if within is None else gpu(within),
                                                              return_centres=True)
    assert got_n == n
    same(got, final, 'final labels')
    same(got_centres, centres, 'centres')
    same(got_count, count, 'count')
    assert ((got == 0).cpu().numpy() == ((within == 0) if within is not None else np.zeros(final.shape, bool))).all()


def test_what_the_cases_are_there_for():
    t = tile()
    assert expected('odd sides')[3]['rounds'] >= 3 and expected('odd sides')[3]['P'] > 300      # many pieces per cell, several rounds
    assert expected('long merge')[3]['rounds'] >= 10 and expected('long merge')[2] >= 20        # ... that end in many regions
    assert expected('hole, island')[3]['leftovers'] and expected('all small')[3]['leftovers'] == [1] and expected('all small')[2] == 1
    planes, S = case('small step')[:2]
    H, W = planes.shape[1:]
    ny, nx = ref.grid(H, W, S)
    assert min(t // (H // ny), t // (W // nx)) + 2 > kernels.get().slic_table        # home cells alone pass the table: the fallback runs
    assert len(set(expected('flat')[0][0].ravel().tolist())) > 1
    assert expected('empty centre')[0][2].tolist()[2:] == [0, 0, 0, 0] and expected('empty centre')[0][1][4].tolist() == [4, 5, 200]
    assert (expected('one cell')[0][0] == 1).all() and ref.grid(5, 40, 8) == (1, 5)
    assert expected('colour only')[3]['P'] > 3 * expected('colour only')[0][2].size      # colour alone: many pieces per cell


def test_merge_rounds_match_and_extra_rounds_change_nothing():
    _, final, n, info = expected('long merge')
    assert len(set(info['group'][1:])) >= 20                        # a wrong choice among the offers lands in another group
    pieces = gpu(info['pieces'])
    sizes = torch.bincount(pieces.reshape(-1).to(torch.int64), minlength=info['P'] + 1)[1:].to(torch.int32)
    pairs, count = nuclei.region_adjacency(pieces, 1)
    k = kernels.get()
    group, launched = k.slic_merge(sizes, pairs, count, 6)
    assert group.tolist() == info['group'] and launched >= info['rounds'] + 1
    shuffle = torch.randperm(pairs.shape[0], generator=torch.Generator().manual_seed(3)).to(pairs.device)
    again, _ = k.slic_merge(sizes, pairs[shuffle], count[shuffle], 6)
    assert torch.equal(again, group)                                                      # the order of the pairs does not matter


def test_strided_and_non_contiguous_inputs():
    planes, S, m, n_iter, min_size, within = case('hole, island')
    _, final, n, _ = expected('hole, island')
    C, H, W = planes.shape
    wide = torch.zeros(H, W, C + 1, dtype=torch.uint8, device='cuda')                    # channels last, one spare channel
    wide[:, :, :C] = gpu(planes).permute(1, 2, 0)
    p = wide.permute(2, 0, 1)[:C]
    w = torch.zeros(W, 2 * H, dtype=torch.int16, device='cuda')
    w[:, ::2] = gpu(within.astype(np.int16) * -300).t()
    w = w[:, ::2].t()
    assert not p.is_contiguous() and not w.is_contiguous()
    got, got_n = nuclei.superpixels(p, S, m, n_iter, min_size, w)
    assert got_n == n
    same(got, final, 'final labels')


def test_two_calls_are_bit_identical():
    for name in ('odd sides', 'small step'):
        planes, S, m, n_iter, min_size, within = case(name)
        p = gpu(planes)
        a = nuclei.superpixels(p, S, m, n_iter, return_centres=True)
        b = nuclei.superpixels(p, S, m, n_iter, return_centres=True)
        assert a[1] == b[1] and torch.equal(a[0], b[0]) and torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])


def test_graph_equals_the_restatement():
    for name in ('four planes', 'hole, island', 'all small'):
        _, final, n, _ = expected(name)
        for loop in (True, False):
            e, border = nuclei.superpixel_graph(gpu(final), n, loop=loop, return_attr=True)
            we, wb = ref.graph(final, n, loop)
            assert e.dtype == torch.int64 and border.dtype == torch.int32
            assert np.array_equal(e.cpu().numpy(), we) and np.array_equal(border.cpu().numpy(), wb)
            assert torch.equal(nuclei.superpixel_graph(gpu(final), n, loop=loop), e)
    with pytest.raises(ValueError, match='outside'):
        nuclei.superpixel_graph(gpu(expected('four planes')[1]), 3)


def test_features_within_the_rounding_of_float32():
    """Area is exact.  Mean and std: the bar of region_mean_std's own test, 255 * 2^-23 (tests/test_region_gpu.py derives it).  A
    centroid is the float32 rounding of a float64 quotient below the image's side: half an ulp of the side at most, side * 2^-24; the
    bound is side * 2^-23."""
    planes = case('four planes')[0]
    _, final, n, _ = expected('four planes')
    C, H, W = planes.shape
    feats, cen = nuclei.superpixel_features(gpu(final), gpu(planes), n)
    assert feats.dtype == cen.dtype == torch.float32 and tuple(feats.shape) == (n, 3 + 2 * C) and tuple(cen.shape) == (n, 2)
    feats, cen = feats.cpu().numpy().astype(np.float64), cen.cpu().numpy().astype(np.float64)
    want = np.zeros((n, 3 + 2 * C))
    for v in range(1, n + 1):
        ys, xs = np.nonzero(final == v)
        want[v - 1, :3] = len(ys), ys.mean(), xs.mean()
        for c in range(C):
            vals = planes[c][ys, xs].astype(np.float64)
            want[v - 1, 3 + 2 * c] = vals.mean()
            want[v - 1, 4 + 2 * c] = np.sqrt(((vals - vals.mean()) ** 2).mean())
    assert np.array_equal(feats[:, 0], want[:, 0])
    assert np.abs(feats[:, 1:3] - want[:, 1:3]).max() <= max(H, W) * 2.0 ** -23
    assert np.array_equal(cen, feats[:, 1:3])
    assert np.abs(feats[:, 3:] - want[:, 3:]).max() <= 255 * 2.0 ** -23
    assert len(nuclei.SUPERPIXEL_FEATURE_NAMES[:3 + 2 * C]) == feats.shape[1]


def test_regions_at_is_exact():
    _, final, n, _ = expected('hole, island')
    H, W = final.shape
    rng = np.random.RandomState(5)
    pts = np.concatenate([rng.uniform(-2, max(H, W) + 2, (200, 2)), [[-0.5, -0.5], [H - 0.5, 0], [H - 0.51, W - 0.51], [3.5, 4.5]]])
    at = np.floor(pts + 0.5).astype(np.int64)
    inside = (at[:, 0] >= 0) & (at[:, 0] < H) & (at[:, 1] >= 0) & (at[:, 1] < W)
    want = np.where(inside, final[np.clip(at[:, 0], 0, H - 1), np.clip(at[:, 1], 0, W - 1)], 0)
    got = nuclei.regions_at(gpu(final), gpu(pts))
    assert got.dtype == torch.int32 and got.tolist() == want.tolist()
    assert inside.sum() > 50 and (~inside).sum() > 5 and (want == 0).sum() > (~inside).sum()      # also points in the hole
