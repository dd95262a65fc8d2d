"""numpy restatement of the contract of region_adjacency (kernels.KernelSpec.region_adjacency, items 1 to 6) and of
nuclei.voronoi_graph, on tests/edt_ref.py's distance transform.  A plain module: tests/test_adjacency_ref_cpu.py pins it against a
brute-force double loop, scipy's binary dilation and closed forms; tests/test_adjacency_gpu.py compares the kernels against it."""
import math

import numpy as np

import edt_ref

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
OFFSETS = {1: ((0, 1), (1, 0)), 2: ((0, 1), (1, 0), (1, 1), (1, -1))}      # each unordered pixel pair once


def region_adjacency(labels, connectivity=1, value=None):
    """(pairs int32 [P, 2], count int32 [P], min_sum int32 [P] or None)."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and labels.size < 2 ** 29 and connectivity in (1, 2)
    L = labels.astype(np.int64)
    V = None if value is None else np.asarray(value).astype(np.int64)
    H, W = L.shape
    a_all, b_all, s_all = [], [], []
    for dy, dx in OFFSETS[connectivity]:
        if H - dy <= 0 or W - abs(dx) <= 0:
            continue
        ys, yq = slice(0, H - dy), slice(dy, H)
        xs, xq = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        p, q = L[ys, xs], L[yq, xq]
        m = (p != q) & (p != 0) & (q != 0)
        a_all.append(np.minimum(p, q)[m])
        b_all.append(np.maximum(p, q)[m])
        if V is not None:
            s_all.append(np.clip(V[ys, xs] + V[yq, xq], INT32_MIN, INT32_MAX)[m])
    a = np.concatenate(a_all) if a_all else np.zeros(0, np.int64)
    b = np.concatenate(b_all) if b_all else np.zeros(0, np.int64)
    if a.size == 0:
        empty = np.zeros(0, np.int32)
        return np.zeros((0, 2), np.int32), empty, (None if value is None else empty.copy())
    ab = np.stack([a, b], axis=1)
    pairs, inverse, count = np.unique(ab, axis=0, return_inverse=True, return_counts=True)      # rows in lexicographic (signed) order
    inverse = inverse.reshape(-1)
    min_sum = None
    if V is not None:
        min_sum = np.full(len(pairs), INT32_MAX, np.int64)
        np.minimum.at(min_sum, inverse, np.concatenate(s_all))
        min_sum = min_sum.astype(np.int32)
    return pairs.astype(np.int32), count.astype(np.int32), min_sum


def eighths(dist2):
    """The largest integer T with T^2 <= 64 dist2, in Python integers."""
    flat = [math.isqrt(64 * int(v)) for v in np.asarray(dist2).ravel()]
    return np.array(flat, dtype=np.int64).reshape(np.shape(dist2))


def bound_eighths(distance):
    """The largest integer k with k / 8 <= distance."""
    k = int(math.floor(float(distance) * 8))
    while (k + 1) / 8 <= distance:
        k += 1
    while k > 0 and k / 8 > distance:
        k -= 1
    return k


def voronoi_cells(labels, max_distance, kept_labels=None):
    """(kept_labels ascending, cells, T): steps 1 to 3 of voronoi_graph."""
    labels = np.asarray(labels).astype(np.int32)
    assert labels.size == 0 or labels.min() >= 0
    if kept_labels is None:
        kept_labels = np.unique(labels[labels != 0])
    kept_labels = np.asarray(kept_labels).astype(np.int32)
    assert np.all(kept_labels[1:] > kept_labels[:-1]) and np.all(kept_labels > 0)
    kept = np.where(np.isin(labels, kept_labels), labels, 0).astype(np.int32)
    d2, near = edt_ref.edt(kept, 'nonzero', max_distance)
    cells = edt_ref.expand_labels(kept, max_distance)
    t = np.where(near >= 0, eighths(np.where(near >= 0, d2, 0)), 0).astype(np.int32)
    return kept_labels, cells, t


def voronoi_graph(labels, max_distance, kept_labels=None, connectivity=1, loop=True, max_gap=None):
    """(edge_index int64 [2, E], border int32 [E], gap float32 [E]) of nuclei.voronoi_graph(..., return_attr=True)."""
    return graph_of_cells(*voronoi_cells(labels, max_distance, kept_labels), connectivity=connectivity, loop=loop, max_gap=max_gap)


def graph_of_cells(kept_labels, cells, t, connectivity=1, loop=True, max_gap=None):
    """Steps 4 to 6 of voronoi_graph on the output of voronoi_cells (which does not depend on the three options)."""
    n = len(kept_labels)
    edges = {}
    if n > 0 and cells.size > 0:
        pairs, count, min_sum = region_adjacency(cells, connectivity, value=t)
        gap8 = min_sum.astype(np.int64) + 8
        for (a, b), c, g in zip(pairs.tolist(), count.tolist(), gap8.tolist()):
            if max_gap is not None and g > bound_eighths(max_gap):
                continue
            i, j = int(np.searchsorted(kept_labels, a)), int(np.searchsorted(kept_labels, b))
            assert kept_labels[i] == a and kept_labels[j] == b
            edges[(i, j)] = edges[(j, i)] = (c, g)
    if loop:
        for i in range(n):
            edges[(i, i)] = (0, 0)
    order = sorted(edges)
    edge_index = np.array(order, dtype=np.int64).reshape(-1, 2).T
    border = np.array([edges[e][0] for e in order], dtype=np.int32)
    gap = (np.array([edges[e][1] for e in order], dtype=np.float64) / 8).astype(np.float32)
    return edge_index, border, gap


def degrees(edge_index, n):
    return np.bincount(edge_index[0], minlength=n).astype(np.int64)
