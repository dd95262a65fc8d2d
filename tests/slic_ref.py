"""A sequential numpy restatement of superpixels (KernelSpec.slic_iterate, KernelSpec.slic_merge, nuclei.superpixels and
nuclei.superpixel_graph), written from the contract: Python integers and loops over pixels and centres, no tiles, no tables, no
atomics.  scipy is used for connected components only."""
import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)


def grid(H, W, S):
    return max(1, (2 * H + S) // (2 * S)), max(1, (2 * W + S) // (2 * S))


def start_centres(planes, S):
    C, H, W = planes.shape
    ny, nx = grid(H, W, S)
    cen = []
    for i in range(ny):
        for j in range(nx):
            y, x = ((2 * i + 1) * H) // (2 * ny), ((2 * j + 1) * W) // (2 * nx)
            cen.append([y, x] + [int(planes[c, y, x]) for c in range(C)])
    return cen


def assign(planes, S, m, cen, within=None):
    """labels [H, W] of one assignment against the centres ``cen`` (a list of K rows of Python integers)."""
    C, H, W = planes.shape
    ny, nx = grid(H, W, S)
    labels = np.zeros((H, W), np.int32)
    for y in range(H):
        hi = y * ny // H
        for x in range(W):
            if within is not None and within[y, x] == 0:
                continue
            hj = x * nx // W
            best = None
            for i in range(max(0, hi - 1), min(ny, hi + 2)):
                for j in range(max(0, hj - 1), min(nx, hj + 2)):
                    k = i * nx + j
                    c = cen[k]
                    d = S * S * sum((int(planes[q, y, x]) - c[2 + q]) ** 2 for q in range(C)) + m * m * ((y - c[0]) ** 2 + (x - c[1]) ** 2)
                    if best is None or (d, k) < best:
                        best = (d, k)
            labels[y, x] = best[1] + 1
    return labels


def update(planes, labels, cen):
    """The centres after one update, and the counts."""
    C = planes.shape[0]
    out, count = [], []
    for k, c in enumerate(cen):
        ys, xs = np.nonzero(labels == k + 1)
        n = len(ys)
        count.append(n)
        if n == 0:
            out.append(list(c))
            continue
        sums = [int(ys.sum()), int(xs.sum())] + [int(planes[q][ys, xs].astype(np.int64).sum()) for q in range(C)]
        out.append([(2 * s + n) // (2 * n) for s in sums])
    return out, count


def iterate(planes, S, m, n_iter, within=None):
    """(labels int32 [H, W], centres int32 [K, 2 + C], count int32 [K])."""
    planes = np.asarray(planes)
    C, H, W = planes.shape
    if H * W == 0:
        return np.zeros((H, W), np.int32), np.zeros((0, 2 + C), np.int32), np.zeros(0, np.int32)
    cen = start_centres(planes, S)
    for _ in range(n_iter):
        labels = assign(planes, S, m, cen, within)
        cen, count = update(planes, labels, cen)
    return labels, np.array(cen, np.int32).reshape(len(cen), 2 + C), np.array(count, np.int32)


def pieces_of(labels):
    """Rule (a): every value split into its 4-connected pieces, numbered by the raster order of their first pixels."""
    H, W = labels.shape
    pieces = np.zeros((H, W), np.int32)
    firsts = []
    for v in np.unique(labels):
        if v == 0:
            continue
        lab, n = ndimage.label(labels == v, CROSS)
        for t in range(1, n + 1):
            firsts.append((int(np.flatnonzero(lab.ravel() == t)[0]), v, lab == t))
    firsts.sort(key=lambda f: f[0])
    for number, (_, _, where) in enumerate(firsts):
        pieces[where] = number + 1
    return pieces, len(firsts)


def contacts(labels):
    """{(a, b): count} with a < b over the 4-neighbour pixel pairs that carry two different non-zero values."""
    H, W = labels.shape
    out = {}
    for y in range(H):
        for x in range(W):
            a = int(labels[y, x])
            for yy, xx in ((y, x + 1), (y + 1, x)):
                if yy < H and xx < W:
                    b = int(labels[yy, xx])
                    if a != 0 and b != 0 and a != b:
                        key = (min(a, b), max(a, b))
                        out[key] = out.get(key, 0) + 1
    return out


def default_min_size(S):
    return max(1, S * S // 4)


def merge(pieces, P, min_size):
    """Rules (b) to (d): (group of every piece, index 0 unused, 0 = never settled; the rounds that settled something)."""
    sizes = np.bincount(pieces.ravel(), minlength=P + 1)
    group = [0] * (P + 1)
    for p in range(1, P + 1):
        if sizes[p] >= min_size:
            group[p] = p
    near = {}
    for (a, b), n in contacts(pieces).items():
        near.setdefault(a, []).append((b, n))
        near.setdefault(b, []).append((a, n))
    rounds = 0
    while True:
        before = list(group)
        joined = 0
        for p in range(1, P + 1):
            if before[p] != 0:
                continue
            offers = [(-n, q) for q, n in near.get(p, []) if before[q] != 0]
            if offers:
                group[p] = before[min(offers)[1]]
                joined += 1
        if joined == 0:
            return group, rounds
        rounds += 1


def connect(labels, min_size, return_info=False):
    """Rules (a) to (f) on the labels of ``iterate``: (final int32 [H, W], n) and, if asked, a dict with the pieces, the merge
    rounds and the numbers of the regions that are leftover blobs of rule (e)."""
    H, W = labels.shape
    pieces, P = pieces_of(labels)
    group, rounds = merge(pieces, P, min_size)
    settled = np.array(group)[pieces]                          # per pixel: its group, 0 where unsettled or outside
    regions = [settled == g for g in sorted(set(group[1:]) - {0})]
    blobs, nb = ndimage.label((pieces != 0) & (settled == 0), CROSS)
    leftover_from = len(regions)
    regions += [blobs == t for t in range(1, nb + 1)]
    order = sorted(range(len(regions)), key=lambda r: int(np.flatnonzero(regions[r].ravel())[0]))
    final = np.zeros((H, W), np.int32)
    leftovers = []
    for number, r in enumerate(order):
        final[regions[r]] = number + 1
        if r >= leftover_from:
            leftovers.append(number + 1)
    if return_info:
        return final, len(regions), dict(pieces=pieces, P=P, rounds=rounds, leftovers=leftovers, group=group)
    return final, len(regions)


def superpixels(planes, S, m=10, n_iter=10, min_size=None, within=None, return_info=False):
    labels, centres, count = iterate(planes, S, m, n_iter, within)
    if min_size is None:
        min_size = default_min_size(S)
    return connect(labels, min_size, return_info)


def graph(labels, n, loop=True):
    """(edge_index int64 [2, E], border int32 [E]): both directions of every contact, (i, i) with ``loop``, rows then columns ascending."""
    edges = {}
    for (a, b), c in contacts(labels).items():
        edges[(a - 1, b - 1)] = c
        edges[(b - 1, a - 1)] = c
    if loop:
        for i in range(n):
            edges[(i, i)] = 0
    keys = sorted(edges)
    return np.array(keys, np.int64).reshape(len(keys), 2).T, np.array([edges[k] for k in keys], np.int32)
