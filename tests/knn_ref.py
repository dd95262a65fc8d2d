"""numpy restatement of the contract of radius_knn (kernels.KernelSpec.radius_knn, csrc/knn.hip) by brute force, and the test that
tells whether an input's verdict can depend on how a float64 sum is rounded.  A plain module: tests/test_knn_ref_cpu.py pins it
against the cKDTree reference (oracle/flat_ref.py) and closed forms; tests/test_graph_front_gpu.py compares the kernels against it.

Unlike the tree, whose order among equal distances is unspecified, this states the kernel's documented order: by distance, the node
itself first, then by index -- so inputs full of ties (lattices, coincident points) have one right answer."""
import numpy as np

REL_GAP = 1e-9                           # two squared distances further apart than this, relatively, compare the same in any rounding


def cut2(r):
    """The squared search radius: the radius is a float32 call argument, the host tree's bound is r + 1e-8, in double.  The square
    is the IEEE product, which is correctly rounded (Python's ``** 2`` goes through pow() and can be one ulp off, 22.00000001 is
    such a value); an ulp of the cut decides nothing on an input that exact_or_separated accepts."""
    rr = float(np.float32(r)) + 1e-8
    return rr * rr


def _pos64(pos):
    p = np.asarray(pos)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 2
    return p.astype(np.float64)


def _d2(q):
    dx, dy = q[None, :, 0] - q[:, None, 0], q[None, :, 1] - q[:, None, 1]
    return dx * dx + dy * dy


def radius_knn(pos, gptr, r, k, loop):
    """pos float32 [n, 2], gptr [B + 1]: for every node the k + 1 nearest nodes of its graph within r + 1e-8, itself among them,
    ordered by (squared distance, the node itself first, local index); the node itself is then dropped unless ``loop``.
    Returns int64 [2, nnz] with global ids, rows ascending."""
    if not 0 <= k <= 32 or not r >= 0:
        raise ValueError('k in 0..32 and r >= 0')
    p, gp, c2 = _pos64(pos), np.asarray(gptr).astype(np.int64), cut2(r)
    rows, cols = [], []
    for g in range(len(gp) - 1):
        lo, m = int(gp[g]), int(gp[g + 1] - gp[g])
        if m <= 0:
            continue
        d2 = _d2(p[lo:lo + m])
        idx = np.broadcast_to(np.arange(m), (m, m))
        other = idx != np.arange(m)[:, None]
        order = np.lexsort((idx, other, d2), axis=1)                   # last key first: d2, then self, then index
        take = np.minimum((d2 <= c2).sum(1), k + 1)
        for i in range(m):
            row = order[i, :take[i]]
            if not loop:
                row = row[row != i]
            rows.append(np.full(len(row), lo + i, np.int64))
            cols.append(lo + row.astype(np.int64))
    if not rows:
        return np.zeros((2, 0), np.int64)
    return np.stack([np.concatenate(rows), np.concatenate(cols)])


def _two_sum_err(a, b):
    """The rounding error of a + b in float64 (Knuth): zero iff the sum is exact."""
    s = a + b
    bb = s - a
    return (a - (s - bb)) + (b - bb)


def _d2_exact(q):
    """(d2, exact): exact[i, j] holds where every operation of d2[i, j] is free of rounding -- the differences (two-sum error zero),
    the squares (a difference of at most 24 significant bits has an exact square in float64; a sufficient test) and their sum."""
    x, y = q[:, 0], q[:, 1]
    dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]
    exact = (_two_sum_err(x[None, :], -x[:, None]) == 0) & (_two_sum_err(y[None, :], -y[:, None]) == 0)
    with np.errstate(over='ignore'):
        exact &= (dx.astype(np.float32).astype(np.float64) == dx) & (dy.astype(np.float32).astype(np.float64) == dy)
    sx, sy = dx * dx, dy * dy
    exact &= _two_sum_err(sx, sy) == 0
    return sx + sy, exact


def exact_or_separated(pos, gptr, r):
    """True iff the graph of (pos, gptr, r) does not depend on how float64 rounds: for every node, the squared distances to the
    nodes of its graph up to twice the cut (r + 1e-8)^2, and the cut itself, sorted, are such that two consecutive values either
    differ by more than REL_GAP relative or are both exact (then every evaluation order, contracted into an FMA or not, yields
    the same two numbers, equal or not; the cut is one double, the same on both sides).  Stricter than asking it of the in-radius
    candidates only: a value just outside the cut is looked at too, and two values that are bit-equal here but not exact count as
    a failure."""
    p, gp, c2 = _pos64(pos), np.asarray(gptr).astype(np.int64), cut2(r)
    for g in range(len(gp) - 1):
        lo, m = int(gp[g]), int(gp[g + 1] - gp[g])
        if m <= 0:
            continue
        d2, exact = _d2_exact(p[lo:lo + m])
        v = np.concatenate([d2, np.full((m, 1), c2)], 1)
        e = np.concatenate([exact, np.ones((m, 1), bool)], 1)
        order = np.argsort(v, axis=1, kind='stable')
        v, e = np.take_along_axis(v, order, 1), np.take_along_axis(e, order, 1)
        ok = (v[:, 1:] - v[:, :-1] > REL_GAP * v[:, 1:]) | (e[:, 1:] & e[:, :-1]) | (v[:, 1:] > 2 * c2)
        if not ok.all():
            return False
    return True


def degrees(edge_index, n):
    return np.bincount(np.asarray(edge_index)[0], minlength=n).astype(np.int64)
