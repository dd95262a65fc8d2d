"""The contract of region outlines (cgc_net_amd.kernels.KernelSpec.region_outlines) restated with Python integers: one crack after
the other, a loop at a time.  Nothing here is shared with the kernels, which never walk a loop.

A pixel (y, x) is the square [x, x + 1] x [y, y + 1]; side 0 is its top, 1 right, 2 bottom, 3 left.  A crack runs with its pixel on the
right: top east, right south, bottom west, left north.  Points are (y, x) lattice corners."""
import numpy as np

DIRECTION = ((0, 1), (1, 0), (0, -1), (-1, 0))                           # (dy, dx) of a crack of side s
TAIL = ((0, 0), (0, 1), (1, 1), (1, 0))                                   # the tail of side s, from the pixel's top-left corner
TABLES = ('label_ptr', 'loop_ptr', 'loop_label', 'loop_start', 'loop_cracks', 'loop_area2', 'vertices')
DTYPES = dict(label_ptr=np.int64, loop_ptr=np.int64, loop_label=np.int32, loop_start=np.int32, loop_cracks=np.int32, loop_area2=np.int64,
              vertices=np.int32)


def values(labels, max_label, within=None):
    """The row every pixel is counted in, -1 for none: a list of lists of Python integers."""
    labels = np.asarray(labels)
    H, W = labels.shape
    on = np.ones((H, W), bool) if within is None else np.asarray(within) != 0
    return [[int(labels[y, x]) if on[y, x] and 0 <= int(labels[y, x]) <= max_label else -1 for x in range(W)] for y in range(H)]


def refused(labels, max_label):
    labels = np.asarray(labels).astype(np.int64)
    return int(((labels < 0) | (labels > max_label)).sum())


def successor(val, y, x, s, connectivity):
    """The crack after side s of pixel (y, x), from the 2 x 2 block at its head."""
    H, W = len(val), len(val[0])
    v = val[y][x]

    def inside(py, px):
        return 0 <= py < H and 0 <= px < W and val[py][px] == v

    ay, ax = y + DIRECTION[s][0], x + DIRECTION[s][1]                     # A: ahead on the region's side
    by, bx = ay + DIRECTION[(s + 3) % 4][0], ax + DIRECTION[(s + 3) % 4][1]      # B: ahead on the other side
    a, b = inside(ay, ax), inside(by, bx)
    right, straight, left = (y, x, (s + 1) % 4), (ay, ax, s), (by, bx, (s + 3) % 4)
    if connectivity == 1:
        return right if not a else (straight if not b else left)
    return left if b else (straight if a else right)


def area2(points):
    """The shoelace sum of x1 y2 - x2 y1 over a closed list of (y, x) points."""
    n = len(points)
    return sum(points[i][1] * points[(i + 1) % n][0] - points[(i + 1) % n][1] * points[i][0] for i in range(n))


def corners(points):
    """The closed list without every point whose incoming and outgoing step have the same direction."""
    n = len(points)

    def step(i):
        (y1, x1), (y2, x2) = points[i % n], points[(i + 1) % n]
        return (y2 - y1, x2 - x1)

    return [points[i] for i in range(n) if step(i - 1) != step(i)]


def loops(labels, max_label, connectivity=1, within=None, background=False):
    """[(label, start id, [the tails (y, x) in loop order])], ordered by (label, start id)."""
    val = values(labels, max_label, within)
    H = len(val)
    W = len(val[0]) if H else 0
    lowest = 0 if background else 1

    def is_crack(y, x, s):
        v = val[y][x]
        if v < lowest:
            return False
        ny, nx = y + DIRECTION[(s + 3) % 4][0], x + DIRECTION[(s + 3) % 4][1]      # the pixel across side s lies to the crack's left
        return not (0 <= ny < H and 0 <= nx < W and val[ny][nx] == v)

    seen = set()
    out = []
    for y in range(H):
        for x in range(W):
            for s in range(4):
                if not is_crack(y, x, s) or (y, x, s) in seen:
                    continue
                tails = []
                at = (y, x, s)
                while at not in seen:                                     # ascending ids: the first crack met is the loop's smallest
                    seen.add(at)
                    assert is_crack(*at)
                    tails.append((at[0] + TAIL[at[2]][0], at[1] + TAIL[at[2]][1]))
                    at = successor(val, at[0], at[1], at[2], connectivity)
                assert at == (y, x, s), 'the successors are a permutation: a loop closes at its start'
                out.append((val[y][x], 4 * (y * W + x) + s, tails))
    return sorted(out, key=lambda t: (t[0], t[1]))


def outlines(labels, max_label, connectivity=1, within=None, mode='corners', background=False):
    """The tables of region_outlines as numpy arrays."""
    found = loops(labels, max_label, connectivity, within, background)
    lists = [tails if mode == 'cracks' else corners(tails) for _, _, tails in found]
    t = dict(loop_label=[v for v, _, _ in found], loop_start=[i for _, i, _ in found], loop_cracks=[len(p) for _, _, p in found],
             loop_area2=[area2(p) for _, _, p in found])
    t['loop_ptr'] = [0] + list(np.cumsum([len(p) for p in lists], dtype=np.int64))
    t['label_ptr'] = [sum(1 for v, _, _ in found if v < L) for L in range(max_label + 2)]
    t['vertices'] = np.array([p for points in lists for p in points], np.int32).reshape(-1, 2)
    return {k: np.asarray(t[k], DTYPES[k]) for k in TABLES}


def per_label(t, max_label):
    """(outer loops, holes, cracks, the sum of area2) per label, int64 [R] each: what outline_tables returns."""
    R = max_label + 1
    outer, holes, cracks, area = (np.zeros(R, np.int64) for _ in range(4))
    for v, n, a in zip(t['loop_label'], t['loop_cracks'], t['loop_area2']):
        outer[v] += a > 0
        holes[v] += a < 0
        cracks[v] += n
        area[v] += a
    return outer, holes, cracks, area


def serpentine(H, W):
    """Rows 1, 3, 5, ... over columns 1 .. W - 2, joined alternately at the right and the left end: one region, one very long loop."""
    a = np.zeros((H, W), np.int32)
    rows = list(range(1, H - 1, 2))
    for y in rows:
        a[y, 1:W - 1] = 1
    for k, y in enumerate(rows[:-1]):
        a[y + 1, W - 2 if k % 2 == 0 else 1] = 1
    return a
