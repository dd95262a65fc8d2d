"""CPU: tests/outline_ref.py, the restatement of KernelSpec.region_outlines, pinned against things it shares no code with: the pixel
count, tests/shape_ref.py's perimeter_crack and Euler numbers (bit quads), scipy.ndimage.label's components, and vertex lists written
out by hand.  The last test restates the KERNELS' route in numpy -- successors as compact indices, pointer doubling for the start and
the position, the scatter, the corner filter through a prefix sum -- and requires the follower's output from it."""
import numpy as np
import pytest
from scipy import ndimage

import outline_ref as ref
import shape_ref

STRUCTURE = {1: ndimage.generate_binary_structure(2, 1), 2: ndimage.generate_binary_structure(2, 2)}


def holed_block():
    a = np.ones((5, 6), np.int32)
    a[2, 2:5] = 0
    return a


def island_in_hole():
    a = np.zeros((9, 9), np.int32)
    a[1:8, 1:8] = 1
    a[2:7, 2:7] = 0
    a[4, 4] = 1
    return a


def ring_around():
    a = np.zeros((7, 8), np.int32)
    a[1:6, 1:7] = 1
    a[2:5, 2:6] = 2
    return a


HAND = {'one_pixel': np.array([[0, 0, 0], [0, 1, 0]], np.int32), 'block': np.pad(np.ones((2, 3), np.int32), 1),
        'diagonal': np.array([[1, 0], [0, 1]], np.int32), 'holed': holed_block(), 'island': island_in_hole(), 'ring': ring_around(),
        'checkerboard': (np.indices((8, 8)).sum(0) % 2).astype(np.int32), 'serpentine': ref.serpentine(12, 9)}


def random_images(count, seed=0):
    rng = np.random.RandomState(seed)
    for _ in range(count):
        H, W = rng.randint(1, 14, size=2)
        yield rng.randint(0, 4, size=(H, W)).astype(np.int32)


def identities(labels, connectivity, background):
    top = 3
    t = {mode: ref.outlines(labels, top, connectivity, mode=mode, background=background) for mode in ('cracks', 'corners')}
    outer, holes, cracks, area = ref.per_label(t['cracks'], top)
    g = shape_ref.geometry(labels, top)
    s = shape_ref.shape(g)
    for v in range(0 if background else 1, top + 1):
        assert area[v] == 2 * int((labels == v).sum()), v
        assert cracks[v] == s['perimeter_crack'][v], v
        assert outer[v] - holes[v] == s['euler4' if connectivity == 1 else 'euler8'][v], v
        assert outer[v] == ndimage.label(labels == v, STRUCTURE[connectivity])[1], v
    if not background:
        assert outer[0] == holes[0] == cracks[0] == 0
    for mode in ('cracks', 'corners'):
        assert t[mode]['loop_label'].tolist() == sorted(t[mode]['loop_label'].tolist())
        assert np.array_equal(t[mode]['label_ptr'], np.searchsorted(t[mode]['loop_label'], np.arange(top + 2)))
    for name in ('loop_label', 'loop_start', 'loop_cracks', 'loop_area2', 'label_ptr'):
        assert np.array_equal(t['cracks'][name], t['corners'][name]), name
    c = t['corners']
    for j in range(len(c['loop_start'])):
        ring = [tuple(p) for p in c['vertices'][c['loop_ptr'][j]:c['loop_ptr'][j + 1]].tolist()]
        assert len(ring) >= 4 and len(ring) % 2 == 0
        assert ref.area2(ring) == c['loop_area2'][j]
    assert np.array_equal(t['cracks']['loop_ptr'][1:], np.cumsum(t['cracks']['loop_cracks']))


@pytest.mark.parametrize('connectivity', (1, 2))
@pytest.mark.parametrize('background', (False, True))
def test_identities_on_random_and_hand_images(connectivity, background):
    for labels in list(random_images(30)) + list(HAND.values()):
        identities(labels, connectivity, background)


def rings(t):
    return [[tuple(p) for p in t['vertices'][a:b].tolist()] for a, b in zip(t['loop_ptr'][:-1], t['loop_ptr'][1:])]


@pytest.mark.parametrize('connectivity', (1, 2))
def test_one_pixel_and_block(connectivity):
    a = np.zeros((3, 4), np.int32)
    a[1, 2] = 1
    for mode in ('cracks', 'corners'):
        t = ref.outlines(a, 1, connectivity, mode=mode)
        assert rings(t) == [[(1, 2), (1, 3), (2, 3), (2, 2)]]
        assert t['loop_start'].tolist() == [4 * (1 * 4 + 2)] and t['loop_cracks'].tolist() == [4] and t['loop_area2'].tolist() == [2]
        assert t['label_ptr'].tolist() == [0, 0, 1] and t['loop_ptr'].tolist() == [0, 4]
    b = np.ones((2, 3), np.int32)
    t = ref.outlines(b, 1, connectivity, mode='cracks')
    assert rings(t) == [[(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (2, 2), (2, 1), (2, 0), (1, 0)]]
    assert t['loop_area2'].tolist() == [12]
    assert rings(ref.outlines(b, 1, connectivity, mode='corners')) == [[(0, 0), (0, 3), (2, 3), (2, 0)]]


def test_diagonal_pair():
    a = HAND['diagonal']
    t = ref.outlines(a, 1, 1, mode='cracks')
    assert rings(t) == [[(0, 0), (0, 1), (1, 1), (1, 0)], [(1, 1), (1, 2), (2, 2), (2, 1)]]
    assert t['loop_start'].tolist() == [0, 12] and t['loop_area2'].tolist() == [2, 2]
    for mode in ('cracks', 'corners'):
        t = ref.outlines(a, 1, 2, mode=mode)
        assert rings(t) == [[(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1), (1, 0)]]      # through (1, 1) twice
        assert t['loop_cracks'].tolist() == [8] and t['loop_area2'].tolist() == [4]


@pytest.mark.parametrize('connectivity', (1, 2))
def test_holed_block(connectivity):
    a = HAND['holed']
    t = ref.outlines(a, 1, connectivity, mode='corners')
    assert t['loop_start'].tolist() == [0, 34] and 34 == 4 * (1 * 6 + 2) + 2       # the bottom side of pixel (1, 2)
    assert t['loop_cracks'].tolist() == [22, 8] and t['loop_area2'].tolist() == [60, -6]
    assert rings(t) == [[(0, 0), (0, 6), (5, 6), (5, 0)], [(2, 2), (3, 2), (3, 5), (2, 5)]]
    cracks = rings(ref.outlines(a, 1, connectivity, mode='cracks'))[1]
    assert cracks == [(2, 3), (2, 2), (3, 2), (3, 3), (3, 4), (3, 5), (2, 5), (2, 4)]      # the start crack's tail (2, 3) is no corner


def test_checkerboard_and_serpentine_counts():
    cb = HAND['checkerboard']
    t = ref.outlines(cb, 1, 1)
    assert t['loop_cracks'].tolist() == [4] * 32
    t = ref.outlines(cb, 1, 2)
    assert len(t['loop_cracks']) == 19 and t['loop_cracks'].tolist()[0] == 56 and sorted(t['loop_cracks'].tolist())[:18] == [4] * 18
    assert (t['loop_area2'] < 0).sum() == 18
    for (H, W), cracks, corners in (((64, 64), 3906, 124), ((128, 256), 32130, 252)):
        t = ref.outlines(ref.serpentine(H, W), 1, 1)
        assert t['loop_cracks'].tolist() == [cracks] and len(t['vertices']) == corners


def test_within_and_refused_values():
    a = np.array([[1, 1, 1, 5]], np.int32)
    w = np.array([[1, 0, 1, 1]], np.uint8)
    assert ref.refused(a, 1) == 1
    t = ref.outlines(a, 1, 1, within=w, mode='corners')
    assert rings(t) == [[(0, 0), (0, 1), (1, 1), (1, 0)], [(0, 2), (0, 3), (1, 3), (1, 2)]]
    assert ref.outlines(np.zeros((0, 4), np.int32), 2)['label_ptr'].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ the kernels' route, in numpy
def doubled(labels, top, connectivity, mode, background):
    """region_outlines as csrc/outline.hip computes it: no loop is followed."""
    val = np.array(ref.values(labels, top), np.int64).reshape(labels.shape)
    H, W = val.shape
    lowest = 0 if background else 1
    pad = np.full((H + 2, W + 2), -1, np.int64)
    pad[1:-1, 1:-1] = val
    across = [pad[:-2, 1:-1], pad[1:-1, 2:], pad[2:, 1:-1], pad[1:-1, :-2]]
    mask = sum(((val >= lowest) & (across[s] != val)).astype(np.int64) << s for s in range(4)).reshape(-1)
    count = np.array([bin(m).count('1') for m in mask], np.int64)
    off = np.cumsum(count)
    n = int(off[-1]) if off.size else 0
    crack, succ = np.zeros(n, np.int64), np.zeros(n, np.int64)

    def index_of(i, s):
        return off[i] - count[i] + bin(mask[i] & ((1 << s) - 1)).count('1')

    for i in np.nonzero(mask)[0]:
        y, x = divmod(int(i), W)
        for s in range(4):
            if mask[i] >> s & 1:
                py, px, ps = ref.successor(val.tolist(), y, x, s, connectivity)
                assert mask[py * W + px] >> ps & 1
                crack[index_of(i, s)] = 4 * i + s
                succ[index_of(i, s)] = index_of(py * W + px, ps)
    assert sorted(succ.tolist()) == list(range(n))                        # a permutation
    rounds = 0
    while (1 << rounds) < n:
        rounds += 1
    low, jump = np.arange(n), succ.copy()
    for _ in range(rounds):
        low, jump = np.minimum(low, low[jump]), jump[jump]
    start = low
    last = succ == start
    steps, jump = np.where(last, 0, 1), np.where(last, -1, succ)
    for _ in range(rounds):
        go = jump >= 0
        at = np.where(go, jump, 0)
        steps, jump = np.where(go, steps + steps[at], steps), np.where(go, jump[at], -1)
    assert (jump == -1).all()
    heads = np.nonzero(start == np.arange(n))[0]
    keys = sorted((int(val.reshape(-1)[crack[k] >> 2]), int(k)) for k in heads)
    loop_of = {k: p for p, (_, k) in enumerate(keys)}
    lengths = np.array([steps[k] + 1 for _, k in keys], np.int64)
    first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    slots, keep, area = np.zeros((n, 2), np.int64), np.zeros(n, np.int64), np.zeros(len(keys), np.int64)
    for k in range(n):
        p = loop_of[int(start[k])]
        pos = steps[start[k]] - steps[k]
        s, i = crack[k] & 3, crack[k] >> 2
        ty, tx = i // W + ref.TAIL[s][0], i % W + ref.TAIL[s][1]
        slots[first[p] + pos] = (ty, tx)
        keep[first[p] + (pos + 1) % lengths[p]] = (crack[succ[k]] & 3) != s
        area[p] += tx * ref.DIRECTION[s][0] - ref.DIRECTION[s][1] * ty
    place = np.concatenate([[0], np.cumsum(keep)])
    vertices = slots if mode == 'cracks' else slots[keep != 0]
    return dict(loop_label=[v for v, _ in keys], loop_start=[crack[k] for _, k in keys], loop_cracks=lengths, loop_area2=area,
                loop_ptr=first if mode == 'cracks' else place[first], vertices=vertices), rounds


@pytest.mark.parametrize('connectivity', (1, 2))
@pytest.mark.parametrize('mode', ('cracks', 'corners'))
def test_doubling_reproduces_the_follower(connectivity, mode):
    for labels in list(random_images(12, seed=1)) + list(HAND.values()):
        for background in (False, True):
            got, _ = doubled(labels, 3, connectivity, mode, background)
            want = ref.outlines(labels, 3, connectivity, mode=mode, background=background)
            for name, g in got.items():
                assert np.array_equal(np.asarray(g, np.int64).reshape(want[name].shape), want[name]), name
    assert doubled(ref.serpentine(64, 64), 1, 1, 'corners', False)[1] == 12
