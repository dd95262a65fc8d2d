"""CPU: pins tests/knn_ref.py, the brute-force restatement the GPU tests of the graph front end compare against, by three means:
the cKDTree reference (oracle/flat_ref.py) on tie-free inputs, closed forms on lattices and lines whose spacing is the radius, and
the check that no layout of tests/knn_cases.py leaves its verdict to the rounding of a float64 sum."""
import numpy as np
import pytest
import torch

import knn_cases as cases
import knn_ref as ref


def tree(pos, gptr, r, k, loop):
    from oracle.flat_ref import TorchKernels
    return TorchKernels().radius_knn(torch.from_numpy(pos), torch.from_numpy(gptr), len(gptr) - 1, r, k, loop).numpy()


@pytest.mark.parametrize('counts,side,k,loop', [([300], 700.0, 8, True), ([1800, 1500, 2100], 1800.0, 8, True),
                                                ([257, 1, 0, 64, 5], 300.0, 8, True), ([400, 380], 900.0, 8, False),
                                                ([500], 900.0, 16, True), ([200, 200], 4000.0, 4, True)])
def test_against_the_tree_on_the_random_parametrisations(counts, side, k, loop):
    """The six inputs of test_kernels_gpu.py::test_radius_knn_matches_the_host_tree, drawn the same way."""
    rng = np.random.RandomState(sum(counts) + k)
    pos = rng.uniform(0.0, side, size=(sum(counts), 2)).astype(np.float32)
    gptr = np.cumsum([0] + counts).astype(np.int32)
    assert ref.exact_or_separated(pos, gptr, 100.0)
    got = ref.radius_knn(pos, gptr, 100.0, k, loop)
    assert got.dtype == np.int64 and np.array_equal(got, tree(pos, gptr, 100.0, k, loop))


@pytest.mark.parametrize('m,step,r,k', [(12, 7.0, 24.0, 8),(9, 3.0, 10.0, 32)])
def test_against_the_tree_on_tie_free_lattices(m, step, r, k):
    """A lattice sheared and stretched by dyadic amounts until no node sees two others at one distance: the tree's order is then
    defined, and the points still sit on a regular grid."""
    q = cases.lattice(m, step).astype(np.float64)
    q = np.stack([q[:, 0] + 0.125 * q[:, 1] + q[:, 0] ** 2 / 64, 1.25 * q[:, 1] + q[:, 1] ** 2 / 128 + q[:, 0] / 32], 1)
    pos, gptr = cases.batch([q])
    d2 = ref._d2(pos.astype(np.float64))
    near = np.sort(np.where(d2 <= ref.cut2(r), d2, np.inf), 1)
    assert np.all((near[:, 1:] > near[:, :-1]) | np.isinf(near[:, 1:])), 'the layout has a tie'
    assert ref.exact_or_separated(pos, gptr, r)
    for loop in (True, False):
        got = ref.radius_knn(pos, gptr, r, k, loop)
        assert np.array_equal(got, tree(pos, gptr, r, k, loop))
    assert (d2 <= ref.cut2(r)).sum(1).max() > 9                    # dense enough for the cut at k = 8 to drop neighbours


@pytest.mark.parametrize('r', [1.0, 97.0, 172.75, 200.0])
@pytest.mark.parametrize('m', [2, 5, 8])
def test_closed_forms_at_spacing_equal_to_radius(m, r):
    pos, gptr = cases.batch([cases.lattice(m, r, 460.0)])
    e = ref.radius_knn(pos, gptr, r, 8, True)
    assert e.shape[1] == m * m + 4 * m * (m - 1)
    assert np.array_equal(e[0], np.sort(e[0])) and np.array_equal(e[:, e[0] == e[1]][0], np.arange(m * m))
    assert ref.radius_knn(pos, gptr, r, 8, False).shape[1] == 4 * m * (m - 1)
    for line in (cases.x_line, cases.y_line):
        pos, gptr = cases.batch([line(m, r, -405.125)])
        deg = ref.degrees(ref.radius_knn(pos, gptr, r, 8, True), m)
        assert deg.tolist() == ([2] + [3] * (m - 2) + [2] if m > 2 else [2, 2])
        e = ref.radius_knn(pos, gptr, r, 8, False)
        assert sorted(map(tuple, e.T.tolist())) == sorted([(i, i + 1) for i in range(m - 1)] + [(i + 1, i) for i in range(m - 1)])


def test_spacing_batch_closed_form():
    for r in (1.0, 97.0, 33.25):
        pos, gptr = cases.spacing_batch(r)
        assert len(pos) == 148 and len(gptr) == 13
        for loop in (True, False):
            assert np.array_equal(ref.degrees(ref.radius_knn(pos, gptr, r, 8, loop), 148), cases.spacing_closed_form(loop))


def test_order_among_ties_and_the_cut():
    """The documented order, spelled out on the 9 x 9 unit lattice: from the centre (node 40) with r = 2.5, the rings are 4 nodes at
    1, 4 at sqrt 2, 4 at 2 and 8 at sqrt 5; inside a ring the lower index comes first, and k cuts a ring after its lowest indices."""
    pos, gptr = cases.unit_lattice()
    row = lambda k, loop: ref.radius_knn(pos, gptr, 2.5, k, loop)[1][ref.radius_knn(pos, gptr, 2.5, k, loop)[0] == 40].tolist()
    full = [40, 31, 39, 41, 49, 30, 32, 48, 50, 22, 38, 42, 58, 21, 23, 29, 33, 47, 51, 57, 59]
    assert row(32, True) == full and row(32, False) == full[1:]
    for k in cases.TIE_KS:
        assert row(k, True) == full[:k + 1] and row(k, False) == full[1:k + 1]
    # three coincident copies of every site, 81 indices apart: the node itself, then its copies by index, then the first ring's
    # twelve nodes by index, which is copy by copy
    pos, gptr = cases.unit_lattice(3)
    e = ref.radius_knn(pos, gptr, 2.5, 6, True)
    assert e[1][e[0] == 40 + 81].tolist() == [121, 40, 202, 31, 39, 41, 49]
    e = ref.radius_knn(pos, gptr, 2.5, 6, False)
    assert e[1][e[0] == 40 + 81].tolist() == [40, 202, 31, 39, 41, 49]
    e = ref.radius_knn(pos, gptr, 2.5, 10, False)
    assert e[1][e[0] == 40 + 81].tolist() == [40, 202, 31, 39, 41, 49, 112, 120, 122, 130]


def test_zero_radius_and_small_graphs():
    pos, gptr = cases.zero_radius_batch()
    e = ref.radius_knn(pos, gptr, 0.0, 3, True)
    rows = [e[1][e[0] == i].tolist() for i in range(12)]
    assert rows[0] == [0, 2, 4, 6] and rows[8] == [8, 0, 2, 4] and rows[1] == [1, 5] and rows[3] == [3] and rows[9] == [9, 10]
    e = ref.radius_knn(pos, gptr, 0.0, 3, False)
    rows = [e[1][e[0] == i].tolist() for i in range(12)]
    assert rows[0] == [2, 4, 6] and rows[8] == [0, 2, 4] and rows[5] == [1] and rows[3] == [] and rows[11] == []
    assert ref.radius_knn(pos[:0], np.zeros(3, np.int32), 1.0, 8, True).shape == (2, 0)
    with pytest.raises(ValueError):
        ref.radius_knn(pos, gptr, 1.0, 33, True)


@pytest.mark.parametrize('name', sorted(cases.RADIUS_EDGE))
def test_radius_edge_cases_state_their_own_answer(name):
    pos, gptr, r, want = cases.radius_edge(name)
    e = ref.radius_knn(pos, gptr, r, 8, False)
    edges = sorted((int(gptr[g]) + i, int(gptr[g]) + j) for g, pairs in enumerate(want) for i, j in pairs)
    assert sorted(map(tuple, e.T.tolist())) == sorted(edges + [(j, i) for i, j in edges])


def test_every_layout_is_exact_or_well_separated():
    seen = 0
    for name, pos, gptr, r in cases.every_knn_layout():
        assert pos.dtype == np.float32 and gptr.dtype == np.int32 and gptr[-1] == len(pos), name
        assert ref.exact_or_separated(pos, gptr, r), name
        seen += 1
    assert seen > 200
    for r in cases.SPACING_RADII:                          # the dyadic layouts really are: nothing was rounded on the way to float32
        pos, _ = cases.spacing_batch(r)
        assert np.array_equal(pos * 8, np.round(pos * 8)) and np.abs(pos).max() < 2 ** 13 and float(np.float32(r)) == r


def test_the_separation_helper_rejects_what_it_should():
    gptr = np.array([0, 3], np.int32)
    third = np.float32(1) / np.float32(3)
    # two neighbours whose squared distances differ in the last bits only, neither exact
    a, b = np.float32(0.001), np.nextafter(np.float32(0.001), np.float32(1))
    pos = np.array([(0, 0), (third, a), (third, -b)], np.float32)
    d2 = ref._d2(pos.astype(np.float64))[0]
    assert 0 < abs(d2[1] - d2[2]) < ref.REL_GAP * d2[1] and not ref.exact_or_separated(pos, gptr, 1.0)
    # equal in this evaluation order but rounded: a contracted evaluation may split them
    pos = np.array([(0, 0), (third, a), (a, third)], np.float32)
    assert not ref.exact_or_separated(pos, gptr, 1.0)
    # exact ties pass; so does a distance that is exactly r although (r + 1e-8)^2 is relatively close to r^2
    pos = np.array([(0, 0), (180, 0), (0, 180)], np.float32)
    assert ref.exact_or_separated(pos, gptr, 180.0) and (ref.cut2(180.0) - 180.0 ** 2) < ref.REL_GAP * 180.0 ** 2
    # a rounded distance that close to the cut does not
    x = np.nextafter(np.float32(180), np.float32(0))
    y = np.float32(np.sqrt(180.0 ** 2 - float(x) ** 2))
    pos = np.array([(0, 0), (x, y), (500, 500)], np.float32)
    d2 = ref._d2(pos.astype(np.float64))[0, 1]
    assert abs(d2 - ref.cut2(180.0)) < ref.REL_GAP * 180.0 ** 2 and not ref.exact_or_separated(pos, gptr, 180.0)
