"""Layouts for the graph front end (csrc/knn.hip, csrc/fps.hip) that tests/test_knn_ref_cpu.py and tests/test_graph_front_gpu.py
share.  A plain module: numpy only, no pytest hooks, no fixtures.  Every layout is (pos float32 [n, 2], gptr int32 [B + 1]).

Where uniformly random floats never produce two equal distances, these put the work on the rules themselves: neighbours at exactly
the radius (lattice spacing = r, so that a neighbour sits on a grid-cell edge of the bucket search), rings of equidistant points cut
by k, coincident points, and the +1e-8 of the host tree's bound.  Tie layouts use dyadic coordinates (multiples of 1/8 below 2^13 in
magnitude): every difference, square and sum is then exact in float64, which knn_ref.exact_or_separated verifies."""
import numpy as np

OFFSETS = (0.0, 460.0, 4736.0, -405.125)
SPACING_RADII = tuple(float(v) for v in range(1, 201)) + (146.5, 172.75, 33.25, 108.5)      # spacing == radius, all dyadic
SIMULATED_MISSES = (97.0, 47.0, 172.75)            # a float32 model of the cell arithmetic puts 2r and 3r two cells apart
NON_DYADIC_RADII = tuple(float(np.float32(v)) for v in (33.3, 108.28453, 0.1, 61.7))
SLOT_COUNTS = [257, 1, 0, 64, 5, 40]               # with side 300 and r = 100: ~90 in-radius neighbours per node of the big graph
SLOT_KS = (0, 1, 4, 7, 8, 9, 15, 16, 17, 31, 32)
TIE_KS = (2, 3, 5, 6, 10)


def batch(graphs):
    graphs = [np.asarray(q, np.float32).reshape(-1, 2) for q in graphs]
    gptr = np.cumsum([0] + [len(q) for q in graphs]).astype(np.int32)
    return np.concatenate(graphs).astype(np.float32), gptr


def _steps(m, step, off):
    """off + i * step for i < m, evaluated in float32 (exact for the dyadic radii and offsets; rounded like any float32 centroid
    for the others)."""
    return (np.float32(off) + np.arange(m, dtype=np.float32) * np.float32(step)).astype(np.float32)


def x_line(m, step, off=0.0):
    return np.stack([_steps(m, step, off), np.full(m, off, np.float32)], 1)


def y_line(m, step, off=0.0):
    return x_line(m, step, off)[:, ::-1].copy()


def lattice(m, step, off=0.0):
    """m x m sites, node y * m + x at (off + x step, off + y step)."""
    s = _steps(m, step, off)
    xx, yy = np.meshgrid(s, s)
    return np.stack([xx.ravel(), yy.ravel()], 1)


def spacing_batch(r):
    """An x-line of 6, a y-line of 6 and a 5 x 5 lattice at spacing r, at each of the four origin offsets: 12 graphs, 148 nodes."""
    return batch([f(m, r, off) for off in OFFSETS for f, m in ((x_line, 6), (y_line, 6), (lattice, 5))])


def spacing_closed_form(loop):
    """Degrees of spacing_batch(r) for a dyadic r and k >= 4: only axis neighbours are within r (the diagonal is r sqrt 2)."""
    line = np.array([1, 2, 2, 2, 2, 1])
    a = np.arange(5)
    inner = ((a > 0).astype(int) + (a < 4).astype(int))
    lat = (inner[None, :] + inner[:, None]).ravel()
    return np.concatenate([line, line, lat] * len(OFFSETS)) + (1 if loop else 0)


def miss_line(r):
    """The 4-point line 0, r, 2r, 3r."""
    return batch([x_line(4, r)])


def slot_batch():
    rng = np.random.RandomState(20)
    return batch([rng.uniform(0.0, 300.0, size=(c, 2)) for c in SLOT_COUNTS])


def unit_lattice(copies=1):
    """9 x 9 unit lattice; with ``copies`` > 1 the whole lattice repeated, so that coincident nodes are 81 indices apart."""
    return batch([np.tile(lattice(9, 1.0), (copies, 1))])


def permuted(pos, gptr, seed):
    """Nodes shuffled within each graph."""
    rng = np.random.RandomState(seed)
    perm = np.concatenate([gptr[g] + rng.permutation(int(gptr[g + 1] - gptr[g])) for g in range(len(gptr) - 1)])
    return pos[perm].copy(), gptr


def zero_radius_batch():
    """r = 0: only coincident nodes are neighbours.  A group of five, a pair, singles, in two graphs."""
    a = [(1, 1), (3, 3), (1, 1), (2, 5), (1, 1), (3, 3), (1, 1), (0, 0), (1, 1)]
    b = [(1, 1), (1, 1), (7.5, 2.25)]
    return batch([a, b])


_UP, _DOWN = np.nextafter(np.float32(100), np.float32(np.inf)), np.nextafter(np.float32(100), np.float32(0))
_R10 = 2.0 ** -10
# name -> (graphs, r, the edges without loops that must be there, as local (i, j) with i < j, per graph)
RADIUS_EDGE = {
    'pythagorean_60_80': ([[(0, 0), (60, 80)]], 100.0, [[(0, 1)]]),
    'one_ulp_outside': ([[(0, 0), (_UP, 0)], [(0, 0), (0, _UP)]], 100.0, [[], []]),
    'one_ulp_inside': ([[(0, 0), (_DOWN, 0)], [(0, 0), (0, _DOWN)]], 100.0, [[(0, 1)], [(0, 1)]]),
    'within_1e-8': ([[(-2.0 ** -28, 0), (0.5, 0)], [(0, -2.0 ** -28), (0, 0.5)]], 0.5, [[(0, 1)], [(0, 1)]]),
    'beyond_1e-8': ([[(-2.0 ** -26, 0), (0.5, 0)], [(0, -2.0 ** -26), (0, 0.5)]], 0.5, [[], []]),
    # the same pair with a third node that moves the grid's origin to -0.5
    'within_1e-8_shifted_origin': ([[(-0.5, 0), (-2.0 ** -28, 0), (0.5, 0)]], 0.5, [[(0, 1), (1, 2)]]),
    # separation r + 2^-27 <= r + 1e-8 with the nearer node just short of one radius from the grid's origin: in exact arithmetic
    # the two are in columns 0 and 2 of a grid whose cell is r, so the cell has to exceed r + 1e-8
    'within_1e-8_across_two_cells': ([[(0, 0), (_R10 - 2.0 ** -30, 0), (2 * _R10 + 2.0 ** -27 - 2.0 ** -30, 0)],
                                      [(0, 0), (0, _R10 - 2.0 ** -30), (0, 2 * _R10 + 2.0 ** -27 - 2.0 ** -30)]],
                                     _R10, [[(0, 1), (1, 2)], [(0, 1), (1, 2)]]),
}


def radius_edge(name):
    graphs, r, want = RADIUS_EDGE[name]
    pos, gptr = batch(graphs)
    assert np.array_equal(pos.astype(np.float64), np.concatenate([np.asarray(q, np.float64) for q in graphs]))   # all float32 values
    return pos, gptr, r, want


def every_knn_layout():
    """(name, pos, gptr, r) of every layout the GPU tests feed to radius_knn, for the separation check."""
    for r in SPACING_RADII + NON_DYADIC_RADII:
        yield ('spacing r=%r' % r,) + spacing_batch(r) + (r,)
    for r in SIMULATED_MISSES:
        yield ('miss line r=%r' % r,) + miss_line(r) + (r,)
    yield ('slots',) + slot_batch() + (100.0,)
    yield ('slots permuted',) + permuted(*slot_batch(), seed=1) + (100.0,)
    for copies in (1, 3):
        yield ('unit lattice x%d' % copies,) + unit_lattice(copies) + (2.5,)
        yield ('unit lattice x%d permuted' % copies,) + permuted(*unit_lattice(copies), seed=copies) + (2.5,)
    yield ('zero radius',) + zero_radius_batch() + (0.0,)
    for name in RADIUS_EDGE:
        yield ('edge ' + name,) + radius_edge(name)[:3]


# ---------------------------------------------------------------------------------------------------------------- FPS
FPS_SIZES = [1, 1023, 0, 1024, 700, 1025, 2049, 16384]          # an empty graph and (FPS_KS) a graph with no picks in the middle
FPS_KS = [1, 32, 0, 32, 0, 32, 32, 32]
FPS_START = [-5, 1023 + 7, 0, 5, 3, -5, 2049 + 7, 16383]


def fps_lattice():
    """40 x 40 integer lattice, node y * 40 + x: 1600 nodes, two register slots per thread."""
    return batch([lattice(40, 1.0)])


def fps_coincident():
    """A plain graph in front, then 50 coincident points with 3 distinct ones among them."""
    rng = np.random.RandomState(4)
    q = np.full((53, 2), 7.0)
    q[[5, 20, 52]] = [(0, 0), (30, 7), (7, 90)]
    return batch([rng.randint(0, 50, size=(17, 2)), q])


def fps_sizes():
    """Integer coordinates in 0..63: coincident nodes and equal distances everywhere, in every register slot, lane and wave."""
    rng = np.random.RandomState(8)
    return batch([rng.randint(0, 64, size=(c, 2)) for c in FPS_SIZES])
