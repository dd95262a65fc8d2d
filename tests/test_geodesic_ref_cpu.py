"""CPU: tests/geodesic_ref.py, the oracle of the GPU geodesic distance transform, pinned to a brute force over all seed-pixel pairs
(scipy.sparse.csgraph.dijkstra on the explicit step graph for the costs, the smallest seed index among the ties), to
scipy.ndimage.distance_transform_cdt on an all-ones domain, and to the invariant "reached = the seeded components of the domain"."""
import numpy as np
import pytest
from scipy import ndimage, sparse
from scipy.sparse import csgraph

import geodesic_ref as ref
import label_ref

SHAPES = [(1, 1), (1, 9), (8, 1), (5, 7), (12, 12), (9, 12)]
METRICS = [(5, 7), (1, 0), (1, 1), (3, 4)]


def step_graph(dom, a, b, connectivity):
    """The explicit graph of the contract's steps, written out pair by pair (not through ref.neighbours)."""
    H, W = dom.shape
    rows, cols, costs = [], [], []
    for y in range(H):
        for x in range(W):
            if not dom[y, x]:
                continue
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if (dy == 0 and dx == 0) or not (0 <= ny < H and 0 <= nx < W) or not dom[ny, nx]:
                        continue
                    if dy != 0 and dx != 0:
                        if b == 0 or (connectivity == 1 and not (dom[ny, x] or dom[y, nx])):
                            continue
                        cost = b
                    else:
                        cost = a
                    rows.append(y * W + x)
                    cols.append(ny * W + nx)
                    costs.append(cost)
    return sparse.csr_matrix((np.array(costs, np.float64), (rows, cols)), shape=(H * W, H * W))


def brute(seeds, within, a, b, connectivity):
    H, W = seeds.shape
    dist = np.full(H * W, ref.GEO_INF, np.int64)
    near = np.full(H * W, -1, np.int64)
    sidx = np.nonzero(seeds.ravel())[0]
    if sidx.size:
        g = step_graph(ref.domain(seeds, within), a, b, connectivity)
        cost = csgraph.dijkstra(g, directed=True, indices=sidx)            # [seed, pixel], inf where unreachable
        for p in range(H * W):
            best = cost[:, p].min()
            if np.isfinite(best):
                dist[p] = int(best)
                near[p] = sidx[cost[:, p] == best].min()
    return dist.reshape(H, W).astype(np.int32), near.reshape(H, W).astype(np.int32)


def cases(shape):
    H, W = shape
    for i, (dd, sd) in enumerate([(0.6, 0.05), (0.8, 0.1), (1.0, 0.02), (0.5, 0.3), (0.7, 0.0), (0.7, 1.0)]):
        rng = np.random.RandomState(100 * H + W + i)
        yield rng.rand(H, W) < sd, rng.rand(H, W) < dd
    rng = np.random.RandomState(H + W)
    yield rng.rand(H, W) < 0.1, None


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_oracle_equals_brute_force(shape):
    for seeds, within in cases(shape):
        for a, b in METRICS:
            for connectivity in (1, 2):
                dist, near = ref.geodesic(seeds, within, (a, b), connectivity)
                bdist, bnear = brute(seeds, within, a, b, connectivity)
                assert dist.dtype == np.int32 and near.dtype == np.int32
                assert np.array_equal(dist, bdist), np.argwhere(dist != bdist)[:5]
                assert np.array_equal(near, bnear), np.argwhere(near != bnear)[:5]
                assert (dist[seeds] == 0).all() and np.array_equal(near[seeds], np.nonzero(seeds.ravel())[0])
                outside = ~ref.domain(seeds, within)
                assert (dist[outside] == ref.GEO_INF).all() and (near[outside] == -1).all()


@pytest.mark.parametrize('max_distance,bound', [(0, 0), (1, 5), (1.5, 7), (3, 15), (10, 50), (1.4, 7), (1.39, 6)])
def test_bound(max_distance, bound):
    assert ref.bound_of(max_distance, 5) == bound
    rng = np.random.RandomState(3)
    seeds, within = rng.rand(12, 12) < 0.03, rng.rand(12, 12) < 0.8
    full_d, full_n = ref.geodesic(seeds, within)
    d, n = ref.geodesic(seeds, within, max_distance=max_distance)
    keep = full_d <= bound
    assert np.array_equal(d, np.where(keep, full_d, ref.GEO_INF)) and np.array_equal(n, np.where(keep, full_n, -1))


def test_all_ones_domain_is_scipy_cdt():
    for shape in ((1, 1), (9, 14), (23, 17)):
        for density in (0.01, 0.1):
            seeds = np.random.RandomState(shape[0] + int(100 * density)).rand(*shape) < density
            seeds[shape[0] // 2, shape[1] // 3] = True
            for metric, name in (((1, 0), 'taxicab'), ((1, 1), 'chessboard')):
                want = ndimage.distance_transform_cdt(~seeds, metric=name)
                for within in (None, np.ones(shape, np.uint8)):
                    for connectivity in (1, 2):
                        assert np.array_equal(ref.geodesic(seeds, within, metric, connectivity)[0], want)
    assert np.array_equal(ref.geodesic(seeds, None, 'cityblock')[0], ref.geodesic(seeds, None, (1, 0))[0])
    assert np.array_equal(ref.geodesic(seeds, None, 'chamfer')[0], ref.geodesic(seeds, None, (5, 7))[0])


def squares_touching_at_a_corner():
    dom = np.zeros((9, 10), bool)
    dom[1:4, 1:4] = True
    dom[4:8, 4:9] = True            # (3, 3) and (4, 4) touch only at a corner
    seeds = np.zeros_like(dom)
    seeds[2, 2] = True
    return seeds, dom


def test_reached_set_is_the_seeded_components():
    seeds, dom = squares_touching_at_a_corner()
    assert label_ref.label(dom, 1)[1] == 2 and label_ref.label(dom, 2)[1] == 1
    for a, b in METRICS:
        for connectivity in (1, 2):
            dist, near = ref.geodesic(seeds, dom, (a, b), connectivity)
            reached = dist != ref.GEO_INF
            assert np.array_equal(reached, near >= 0)
            if b == 0 or connectivity == 1:
                assert np.array_equal(reached, ref.seeded_components(seeds, dom, 1))
                assert not reached[4:8, 4:9].any() and reached[1:4, 1:4].all()          # never through the corner contact
            else:
                assert np.array_equal(reached, ref.seeded_components(seeds, dom, 2)) and np.array_equal(reached, dom)
                assert dist[4, 4] == dist[3, 3] + b
    for i in range(6):
        rng = np.random.RandomState(40 + i)
        seeds, within = rng.rand(12, 11) < 0.03, rng.rand(12, 11) < 0.55
        for a, b in METRICS:
            for connectivity in (1, 2):
                reached = ref.geodesic(seeds, within, (a, b), connectivity)[0] != ref.GEO_INF
                assert np.array_equal(reached, ref.seeded_components(seeds, within, 1 if b == 0 else connectivity))


def test_expand_and_split_on_top():
    # a wall of within == 0 with one opening: the label behind it arrives through the opening, not across the wall
    lab = np.zeros((9, 11), np.int32)
    lab[:, 0], lab[:, 10] = 9, 4
    within = np.ones(lab.shape, bool)
    within[1:, 3] = False                               # the wall: column 3, open at row 0
    out = ref.expand_labels_geodesic(lab, None, within)
    assert (out[:, 1:3] == 9).all() and (out[1:, 3] == 0).all() and (out[8, 4:10] == 4).all() and out[0, 3] == 9
    assert np.array_equal(ref.expand_labels_geodesic(lab, 0, within), lab)
    near = ref.expand_labels_geodesic(lab, 2, within)
    assert (near[:, 1:3] == 9).all() and (near[:, 8:10] == 4).all() and (near[:, 3:8] == 0).all()
    # the thin ellipse of the issue: one instance with geodesic growth
    yy, xx = np.mgrid[0:40, 0:60]
    m = ((yy - 20) / 4.2) ** 2 + ((xx - 30) / 22.0) ** 2 <= 1.0
    lab, n = ref.split_touching_geodesic(m, 3)
    assert n == 1 and np.array_equal(lab != 0, m)
    import edt_ref
    assert edt_ref.split_touching(m, 3)[1] == 3
