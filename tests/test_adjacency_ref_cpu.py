"""CPU: pins tests/adjacency_ref.py, the numpy restatement the GPU tests compare against, by three independent means: a brute-force
Python double loop on small random images, scipy's binary dilation per label on a tissue's Voronoi cells, and the closed forms for an
image of all-distinct labels."""
import numpy as np
import pytest
from scipy import ndimage

import adjacency_ref as ref
import edt_ref


def synthetic_tissue(*args):
    """nuclei.synthetic_tissue without importing the package's GPU parts at collection."""
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import nuclei
    return nuclei.synthetic_tissue(*args)


def brute(labels, connectivity, value=None):
    H, W = labels.shape
    table = {}
    for y in range(H):
        for x in range(W):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dy, dx) == (0, 0) or (connectivity == 1 and dy != 0 and dx != 0):
                        continue
                    yy, xx = y + dy, x + dx
                    if not (0 <= yy < H and 0 <= xx < W) or (yy, xx) < (y, x):      # each unordered pixel pair once
                        continue
                    a, b = int(labels[y, x]), int(labels[yy, xx])
                    if a == 0 or b == 0 or a == b:
                        continue
                    key = (min(a, b), max(a, b))
                    s = None if value is None else max(-2 ** 31, min(2 ** 31 - 1, int(value[y, x]) + int(value[yy, xx])))
                    c, m = table.get(key, (0, None))
                    table[key] = (c + 1, s if m is None else min(m, s))
    keys = sorted(table)
    return keys, [table[k][0] for k in keys], [table[k][1] for k in keys]


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('with_value', [False, True])
def test_brute_force_on_small_random_images(connectivity, with_value):
    rng = np.random.RandomState(7 + connectivity + 2 * with_value)
    for trial in range(60):
        H, W = rng.randint(1, 13), rng.randint(1, 13)
        pool = np.array([0, 0, 1, 2, 3, 7, -1, -5, -2 ** 31, 2 ** 31 - 1], dtype=np.int64)
        labels = pool[rng.randint(0, 2 + rng.randint(1, len(pool) - 1), size=(H, W))].astype(np.int32)
        value = None
        if with_value:
            value = rng.randint(-50, 50, size=(H, W)).astype(np.int32)
            if trial % 5 == 0:
                value[rng.rand(H, W) < 0.3] = 2 ** 31 - 1
                value[rng.rand(H, W) < 0.3] = -2 ** 31
        pairs, count, min_sum = ref.region_adjacency(labels, connectivity, value)
        keys, c, m = brute(labels, connectivity, value)
        assert pairs.dtype == np.int32 and count.dtype == np.int32 and pairs.shape == (len(keys), 2)
        assert [tuple(r) for r in pairs.tolist()] == keys
        assert count.tolist() == c
        if with_value:
            assert min_sum.dtype == np.int32 and min_sum.tolist() == m
        else:
            assert min_sum is None


def test_degenerate_shapes():
    for shape in ((0, 5), (5, 0), (1, 1), (1, 7), (7, 1)):
        for connectivity in (1, 2):
            pairs, count, min_sum = ref.region_adjacency(np.ones(shape, np.int32), connectivity, np.ones(shape, np.int32))
            assert pairs.shape == (0, 2) and count.shape == (0,) and min_sum.shape == (0,)
    two = np.ones((5, 6), np.int32)
    two[:, 3:] = 2
    pairs, count, _ = ref.region_adjacency(two, 1)
    assert pairs.tolist() == [[1, 2]] and count.tolist() == [5]
    pairs, count, _ = ref.region_adjacency(two, 2)
    assert count.tolist() == [5 + 2 * 4]


@pytest.mark.parametrize('n', [2, 5, 96])
def test_closed_forms_for_all_distinct_labels(n):
    labels = np.arange(1, n * n + 1, dtype=np.int32).reshape(n, n)
    for connectivity, want in ((1, 2 * n * (n - 1)), (2, 2 * n * (n - 1) + 2 * (n - 1) ** 2)):
        pairs, count, _ = ref.region_adjacency(labels, connectivity)
        assert len(pairs) == want and np.all(count == 1)
    if n == 96:
        assert 2 * n * (n - 1) == 18240 and 2 * n * (n - 1) + 2 * (n - 1) ** 2 == 36290


@pytest.fixture(scope='module')
def tissue_cells():
    labels, _ = synthetic_tissue(300, 300, 60)
    return labels, edt_ref.expand_labels(labels, 50)


def test_tissue_pair_set_against_binary_dilation(tissue_cells):
    _, cells = tissue_cells
    for connectivity, structure in ((1, ndimage.generate_binary_structure(2, 1)), (2, np.ones((3, 3), bool))):
        want = set()
        for a in np.unique(cells[cells != 0]).tolist():
            ring = ndimage.binary_dilation(cells == a, structure) & (cells != a) & (cells != 0)
            for b in np.unique(cells[ring]).tolist():
                want.add((min(a, b), max(a, b)))
        pairs, count, _ = ref.region_adjacency(cells, connectivity)
        assert set(map(tuple, pairs.tolist())) == want and len(pairs) == len(want)
        assert np.all(count >= 1)
        if connectivity == 1:
            assert len(want) == 146


def test_tissue_figures(tissue_cells):
    labels, cells = tissue_cells
    assert len(np.unique(labels[labels != 0])) == 59
    assert len(ref.region_adjacency(labels, 1)[0]) == 11 and len(ref.region_adjacency(labels, 2)[0]) == 13
    edge_index, border, gap = ref.voronoi_graph(labels, 50, loop=False)
    deg = ref.degrees(edge_index, 59)
    assert edge_index.shape[1] == 2 * 146 and deg.max() <= 12 and abs(deg.mean() - 4.9) < 0.06
    assert np.array_equal(edge_index[:, np.lexsort((edge_index[1], edge_index[0]))], edge_index)
    assert set(map(tuple, edge_index.T.tolist())) == set(map(tuple, edge_index[::-1].T.tolist()))
    assert np.all(border >= 1) and np.all(gap >= 1.0)                      # two cells' pixels are at least one step apart


def test_voronoi_graph_options(tissue_cells):
    labels, _ = tissue_cells
    full, _, gap = ref.voronoi_graph(labels, 50, loop=False)
    near, _, gap_near = ref.voronoi_graph(labels, 50, loop=False, max_gap=20)
    assert 0 < near.shape[1] < full.shape[1] and gap_near.max() <= 20 and np.sum(gap <= 20) == near.shape[1]
    assert ref.voronoi_graph(labels, 50, loop=False, max_gap=0)[0].shape == (2, 0)
    looped, border, gap = ref.voronoi_graph(labels, 50, loop=True)
    diag = looped[0] == looped[1]
    assert diag.sum() == 59 and np.all(border[diag] == 0) and np.all(gap[diag] == 0)
    sizes = np.bincount(labels.ravel())
    kept = np.nonzero(sizes >= 10)[0][1:].astype(np.int32)
    assert len(kept) < 59                                                  # the tissue's sub-10-pixel objects vanish as nodes
    small, _, _ = ref.voronoi_graph(labels, 50, kept_labels=kept)
    assert small.max() == len(kept) - 1
    _, cells, t = ref.voronoi_cells(labels, 50, kept)
    assert set(np.unique(cells).tolist()) <= set([0] + kept.tolist()) and t.min() >= 0 and np.all(t[cells == 0] == 0)
    assert ref.bound_eighths(0.124) == 0 and ref.bound_eighths(0.125) == 1 and ref.bound_eighths(20) == 160
    assert ref.eighths(np.array([0, 1, 2, 2 ** 31 - 2])).tolist() == [0, 8, 11, 370727]
