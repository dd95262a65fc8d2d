"""The oracle of cgc_net_amd.nuclei.geodesic_distance_transform / expand_labels(geodesic=True) / split_touching(growth='geodesic'):
a heap Dijkstra over the lexicographic key (cost, seed index), numpy + Python only, written for the tests and sharing no code with the
kernel (tests/test_geodesic_ref_cpu.py pins it to a brute force over all seed-pixel pairs on an explicit step graph).

The step rules are those of kernels.KernelSpec.geodesic_transform: the domain is {within != 0} u {seeds != 0}; an axial step between
two domain pixels costs a, a diagonal one b (b = 0: none); with connectivity 1 the diagonal step (y, x) -> (y + dy, x + dx) also needs
(y + dy, x) or (y, x + dx) in the domain."""
import heapq

import numpy as np

import edt_ref
import label_ref

GEO_INF = 2 ** 31 - 1
STEPS = {'cityblock': (1, 0), 'chessboard': (1, 1), 'chamfer': (5, 7)}
AXIAL = ((-1, 0), (0, -1), (0, 1), (1, 0))
DIAGONAL = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def steps_of(metric):
    a, b = STEPS[metric] if isinstance(metric, str) else metric
    assert (1 <= a <= b <= 2 * a) or (a >= 1 and b == 0)
    return int(a), int(b)


def domain(seeds, within=None):
    seeds = np.asarray(seeds) != 0
    return seeds | (np.ones(seeds.shape, bool) if within is None else np.asarray(within) != 0)


def neighbours(dom, y, x, a, b, connectivity):
    """The (y', x', cost) of every allowed step out of the domain pixel (y, x)."""
    H, W = dom.shape
    for dy, dx in AXIAL:
        ny, nx = y + dy, x + dx
        if 0 <= ny < H and 0 <= nx < W and dom[ny, nx]:
            yield ny, nx, a
    if b:
        for dy, dx in DIAGONAL:
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and dom[ny, nx] and (connectivity == 2 or dom[ny, x] or dom[y, nx]):
                yield ny, nx, b


def bound_of(max_distance, a):
    """The largest integer k with k / a <= max_distance (None: no bound)."""
    if max_distance is None:
        return None
    k = int(np.floor(max_distance * a)) + 2
    while k > 0 and k / a > max_distance:
        k -= 1
    return k


def geodesic(seeds, within=None, metric='chamfer', connectivity=1, max_distance=None):
    """(dist int32 [H, W], nearest int32 [H, W]) of the contract of geodesic_distance_transform; costs in raw units."""
    a, b = steps_of(metric)
    assert connectivity in (1, 2)
    seeds = np.asarray(seeds) != 0
    H, W = seeds.shape
    dom = domain(seeds, within)
    best = {}
    heap = []
    for y, x in zip(*np.nonzero(seeds)):
        p = int(y) * W + int(x)
        best[p] = (0, p)
        heap.append((0, p, p))
    heapq.heapify(heap)
    while heap:
        cost, seed, p = heapq.heappop(heap)
        if best[p] != (cost, seed):
            continue
        for ny, nx, c in neighbours(dom, p // W, p % W, a, b, connectivity):
            q = ny * W + nx
            cand = (cost + c, seed)
            if q not in best or cand < best[q]:
                best[q] = cand
                heapq.heappush(heap, (cand[0], seed, q))
    dist = np.full(H * W, GEO_INF, np.int64)
    near = np.full(H * W, -1, np.int64)
    dmax = bound_of(max_distance, a)
    for p, (cost, seed) in best.items():
        if dmax is None or cost <= dmax:
            dist[p], near[p] = cost, seed
    return dist.reshape(H, W).astype(np.int32), near.reshape(H, W).astype(np.int32)


def expand_labels_geodesic(labels, distance, within=None, metric='chamfer', connectivity=1):
    labels = np.asarray(labels)
    _, near = geodesic(labels, within, metric, connectivity, distance)
    fill = (labels == 0) & (near >= 0)
    out = labels.copy()
    out[fill] = labels.ravel()[near[fill]]
    return out


def split_touching_geodesic(mask, core_radius, connectivity=1, min_size=0):
    fg = np.asarray(mask) != 0
    d2 = edt_ref.dist2_scipy(~fg)
    dist = np.where(d2 == edt_ref.EDT_INF, np.inf, np.sqrt(d2.astype(np.float64)))
    cores, k, _ = label_ref.label(dist > core_radius, connectivity)
    grown = expand_labels_geodesic(cores, None, within=fg, connectivity=connectivity)      # unbounded: every pixel joined to a core
    rest, _, _ = label_ref.label(fg & (grown == 0), connectivity)                          # = the components without a core
    combined = np.where(rest > 0, rest + k, grown)
    lab, n, _ = label_ref.label(combined, connectivity, min_size)
    return lab, n


def seeded_components(seeds, within=None, connectivity=1):
    """bool [H, W]: the pixels of the ``connectivity``-components of the domain that hold a seed."""
    seeds = np.asarray(seeds) != 0
    lab, _, _ = label_ref.label(domain(seeds, within), connectivity)
    hit = np.unique(lab[seeds])
    return np.isin(lab, hit[hit > 0])
