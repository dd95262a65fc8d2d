"""GPU: the graph front end -- csrc/knn.hip against tests/knn_ref.py's brute force, csrc/fps.hip against the host loop of
oracle/flat_ref.py -- on the inputs where uniformly random floats say nothing: neighbours at exactly the radius (lattice spacing = r
puts them on a grid-cell edge of the bucket search), every slot count of the insertion network, rings of equidistant points cut by k,
coincident points, the +1e-8 of the host tree's bound, and for the sampler equal distances in every register slot, lane and wave.

Every comparison is torch.equal: there are no tolerances.  Every kNN input is first shown, in the reference alone, to be exact or
well separated (knn_ref.exact_or_separated), so that neither the order of a float64 sum nor its contraction into an FMA has a say."""
import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
from oracle.flat_ref import TorchKernels

import knn_cases as cases
import knn_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REF = TorchKernels()


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def g(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(DEV)


def knn(pos, gptr, r, k, loop):
    return hip().radius_knn(g(pos), g(gptr), len(gptr) - 1, r, k, loop).cpu()


def diff(got, want, limit=12):
    """The edges on one side only, for the assertion message."""
    a, b = set(map(tuple, got.T.tolist())), set(map(tuple, want.T.tolist()))
    return 'missing %s, extra %s' % (sorted(b - a)[:limit], sorted(a - b)[:limit])


def check(pos, gptr, r, k, loop, separated=None):
    """The kernel's edge list is the reference's, edge for edge in the same order."""
    assert ref.exact_or_separated(pos, gptr, r) if separated is None else separated
    want = torch.from_numpy(ref.radius_knn(pos, gptr, r, k, loop))
    got = knn(pos, gptr, r, k, loop)
    assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[0] == 2
    assert torch.equal(got, want), 'r=%r k=%d loop=%s: %s' % (r, k, loop, diff(got, want))
    return got


# ------------------------------------------------------------------------------------------------ kNN: spacing equals radius
@pytest.mark.parametrize('loop', [True, False])
def test_knn_neighbours_at_exactly_the_radius(loop):
    """Lines and lattices whose spacing is the radius, for every integer radius to 200 and four quarter-values, at four origins:
    the reference, and the closed form (axis neighbours only; the diagonal is r sqrt 2)."""
    degree = torch.from_numpy(cases.spacing_closed_form(loop))
    wrong = []
    for r in cases.SPACING_RADII:
        pos, gptr = cases.spacing_batch(r)
        assert ref.exact_or_separated(pos, gptr, r)
        want = torch.from_numpy(ref.radius_knn(pos, gptr, r, 8, loop))
        got = knn(pos, gptr, r, 8, loop)
        assert torch.equal(torch.bincount(want[0], minlength=148), degree)
        if not torch.equal(got, want):
            wrong.append('r=%r: %s' % (r, diff(got, want, 4)))
    assert not wrong, '%d radii of %d: %s' % (len(wrong), len(cases.SPACING_RADII), '; '.join(wrong[:6]))


@pytest.mark.parametrize('loop', [True, False])
@pytest.mark.parametrize('r', cases.SIMULATED_MISSES)
def test_knn_line_whose_far_pair_a_float32_model_puts_two_cells_apart(r, loop):
    """0, r, 2r, 3r: with cell = r and float32 cell arithmetic, (2r) / r truncates to 1 and (3r) / r to 3 for these radii, so a 3x3
    scan would not see the neighbour at exactly r."""
    pos, gptr = cases.miss_line(r)
    got = check(pos, gptr, r, 8, loop)
    own = [0, 1, 2, 3] if loop else []
    assert sorted(map(tuple, got.T.tolist())) == sorted([(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)] + [(i, i) for i in own])


@pytest.mark.parametrize('r', cases.NON_DYADIC_RADII)
def test_knn_spacing_equal_to_a_non_dyadic_radius(r):
    """Coordinates rounded to float32 like any centroid: the neighbour 'at r' is a rounding error inside or outside; the reference
    alone decides which."""
    pos, gptr = cases.spacing_batch(r)
    for loop in (True, False):
        check(pos, gptr, r, 8, loop)


# ------------------------------------------------------------------------------------------------ kNN: every slot count
@pytest.mark.parametrize('loop', [True, False])
def test_knn_every_slot_count(loop):
    """k from 0 to 32 through the 9-, 17- and 33-slot kernels, with k below, at and above a slot count's edge, on a batch with graphs
    smaller than k + 1, a single node and an empty graph; dense enough that every slot fills."""
    pos, gptr = cases.slot_batch()
    separated = ref.exact_or_separated(pos, gptr, 100.0)
    for k in cases.SLOT_KS:
        got = check(pos, gptr, 100.0, k, loop, separated)
        deg = torch.bincount(got[0], minlength=len(pos))
        assert int(deg[:257].max()) == k + (1 if loop else 0) and int(deg[257]) == (1 if loop else 0)

@pytest.mark.parametrize('k', [33, -1])
def test_knn_refuses_a_k_outside_its_slots(k):
    pos, gptr = cases.slot_batch()
    with pytest.raises(RuntimeError):
        knn(pos, gptr, 100.0, k, True)
    torch.cuda.synchronize()


def test_knn_zero_radius_sees_coincident_nodes_only():
    pos, gptr = cases.zero_radius_batch()
    for k in (0, 3, 8):
        for loop in (True, False):
            check(pos, gptr, 0.0, k, loop)
    rows = lambda e: [e[1][e[0] == i].tolist() for i in range(12)]
    assert rows(knn(pos, gptr, 0.0, 3, True)) == [[0, 2, 4, 6], [1, 5], [2, 0, 4, 6], [3], [4, 0, 2, 6], [5, 1], [6, 0, 2, 4], [7],
                                                  [8, 0, 2, 4], [9, 10], [10, 9], [11]]
    assert rows(knn(pos, gptr, 0.0, 8, False)) == [[2, 4, 6, 8], [5], [0, 4, 6, 8], [], [0, 2, 6, 8], [1], [0, 2, 4, 8], [],
                                                   [0, 2, 4, 6], [10], [9], []]


# ------------------------------------------------------------------------------------------------ kNN: ties at the cut
@pytest.mark.parametrize('copies', [1, 3])
def test_knn_ties_at_the_cut_go_to_the_lower_index(copies):
    """9 x 9 unit lattice, r = 2.5: rings of 4, 4, 4 and 8 equidistant nodes; k cuts inside a ring and the lower indices win.  With
    three coincident copies per site: the node itself, then its copies by index, then the ring by index."""
    pos, gptr = cases.unit_lattice(copies)
    separated = ref.exact_or_separated(pos, gptr, 2.5)
    for k in cases.TIE_KS:
        for loop in (True, False):
            got = check(pos, gptr, 2.5, k, loop, separated)
            assert int(torch.bincount(got[0])[40]) == k + (1 if loop else 0)
    got = knn(pos, gptr, 2.5, 6, True)
    want = [40, 31, 39, 41, 49, 30, 32] if copies == 1 else [40, 121, 202, 31, 39, 41, 49]
    assert got[1][got[0] == 40].tolist() == want


@pytest.mark.parametrize('layout,r', [('unit', 2.5), ('unit3', 2.5), ('slots', 100.0)])
def test_knn_permuting_the_nodes_permutes_the_answer(layout, r):
    """Shuffled within each graph, the kernel gives the reference of the shuffled input (ties then fall to other nodes: the rule is
    by index, not by position)."""
    pos, gptr = {'unit': cases.unit_lattice, 'unit3': lambda: cases.unit_lattice(3), 'slots': cases.slot_batch}[layout]()
    pos, gptr = cases.permuted(pos, gptr, seed=len(pos))
    for k in (5, 10, 32):
        check(pos, gptr, r, k, True)
    check(pos, gptr, r, 6, False)


# ------------------------------------------------------------------------------------------------ kNN: the radius edge
@pytest.mark.parametrize('name', sorted(cases.RADIUS_EDGE))
def test_knn_radius_edge(name):
    pos, gptr, r, want = cases.radius_edge(name)
    got = check(pos, gptr, r, 8, False)
    edges = sorted((int(gptr[b]) + i, int(gptr[b]) + j) for b, pairs in enumerate(want) for i, j in pairs)
    assert sorted(map(tuple, got.T.tolist())) == sorted(edges + [(j, i) for i, j in edges])
    check(pos, gptr, r, 8, True)


# ------------------------------------------------------------------------------------------------ kNN: batch isolation
def test_knn_graphs_of_a_batch_do_not_see_each_other():
    one, _ = cases.batch([cases.lattice(5, 50.0, 460.0)])
    pos, gptr = cases.batch([one, one, cases.x_line(6, 97.0), one])
    got = check(pos, gptr, 100.0, 8, True)
    graph_of = torch.from_numpy(np.repeat(np.arange(4), np.diff(gptr)))
    assert torch.equal(graph_of[got[0]], graph_of[got[1]])                       # identical coordinates, no cross edges
    pos, gptr = cases.slot_batch()
    whole = knn(pos, gptr, 100.0, 8, True)
    parts = [knn(pos[lo:hi], np.array([0, hi - lo], np.int32), 100.0, 8, True) + int(lo)
             for lo, hi in zip(gptr[:-1], gptr[1:]) if hi > lo]
    assert torch.equal(whole, torch.cat(parts, 1))


# ------------------------------------------------------------------------------------------------ kNN: image-stage centroids
def test_knn_on_centroids_of_the_image_stage():
    from cgc_net_amd import nuclei
    labels, gray = nuclei.synthetic_tissue(300, 300, 60)
    L, n = nuclei.label_instances(g(labels))
    _, centroids, kept = nuclei.nucleus_features(L, g(gray), max_label=n)
    pos = centroids.cpu().numpy()
    assert pos.dtype == np.float32 and pos.shape == (len(kept), 2) and len(kept) > 50
    gptr = np.array([0, len(pos)], np.int32)
    check(pos, gptr, 100.0, 8, True)
    check(pos, gptr, 100.0, 8, False)


# ------------------------------------------------------------------------------------------------ FPS
def fps(pos, gptr, start, ks, table16, fill=-7):
    B = len(gptr) - 1
    optr = torch.tensor(np.cumsum([0] + list(ks)), dtype=torch.int32)
    start = torch.tensor(start, dtype=torch.int32)
    nmax = int(np.diff(gptr).max())
    want = torch.full((int(optr[-1]),), fill, dtype=torch.int32)
    got = torch.full((int(optr[-1]),), fill, dtype=torch.int32, device=DEV)
    REF.farthest_point_sample(torch.from_numpy(pos), torch.from_numpy(gptr), B, nmax, start, optr, want, table16)
    hip().farthest_point_sample(g(pos), g(gptr), B, nmax, g(start), g(optr), got, table16)
    got = got.cpu()
    assert torch.equal(got, want), 'first difference at pick %d' % int((got != want).nonzero()[0])
    return got


@pytest.mark.parametrize('table16', [False, True])
def test_fps_integer_lattice(table16):
    """40 x 40 from the corner, every node picked: after the opposite corner the two remaining corners tie, and from then on nearly
    every pick is a tie between register slots, lanes and waves."""
    pos, gptr = cases.fps_lattice()
    got = fps(pos, gptr, [0], [1600], table16)
    assert got[:3].tolist() == [0, 1599, 39]
    if not table16:
        assert sorted(got.tolist()) == list(range(1600))              # squared distances: zero only at a picked node


@pytest.mark.parametrize('table16', [False, True])
def test_fps_coincident_points(table16):
    """Once every remaining distance is zero, numpy's argmax returns local index 0 again and again."""
    pos, gptr = cases.fps_coincident()
    got = fps(pos, gptr, [3, 9], [17, 53], table16)
    second = (got[17:] - 17).tolist()
    assert second[0] == 9 and sorted(second[:4]) == [5, 9, 20, 52] and second[4:] == [0] * 49


@pytest.mark.parametrize('table16', [False, True])
def test_fps_graph_sizes_around_the_thread_and_node_limits(table16):
    """1, 1023, 1024, 1025, 2049 and 16384 nodes, an empty graph and one without picks between them, first picks below 0 and past
    the end (clamped), integer coordinates full of ties."""
    pos, gptr = cases.fps_sizes()
    got = fps(pos, gptr, cases.FPS_START, cases.FPS_KS, table16)
    first = got[np.cumsum([0] + cases.FPS_KS)[[0, 1, 3, 5, 6, 7]]].tolist()
    lo = gptr[:-1]
    assert first == [0, lo[1] + 1022, lo[3] + 5, lo[5], lo[6] + 2048, lo[7] + 16383]


def test_fps_refuses_a_graph_over_the_node_limit():
    pos, gptr = cases.batch([np.random.RandomState(1).randint(0, 64, size=(16385, 2))])
    out = torch.full((32,), -7, dtype=torch.int32, device=DEV)
    args = (g(pos), g(gptr), 1, 16385, g(torch.zeros(1, dtype=torch.int32)), g(torch.tensor([0, 32], dtype=torch.int32)), out)
    for table16 in (False, True):
        with pytest.raises(RuntimeError):
            hip().farthest_point_sample(*args, table16)
    torch.cuda.synchronize()
    assert bool((out == -7).all())
