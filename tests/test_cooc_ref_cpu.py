"""CPU: tests/cooc_ref.py, the numpy restatement the GPU tests of the region co-occurrence compare with, pinned against a pure-Python
loop over pixels and offsets, against cases written out by hand (one of them the example of skimage's graycomatrix documentation),
and against identities of the tables; its ``properties`` against a second float64 formulation with explicit loops over i and j, within
the bound tests/test_cooc_gpu.py uses -- the reference alone stays inside it."""
import math

import numpy as np
import pytest

import cooc_ref as ref

ALL_OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1), (-1, 0), (0, -1), (2, -3), (-4, 2))


def loop_tables(labels, values, offsets, levels, lut, symmetric, max_label, within):
    H, W = labels.shape
    out = np.zeros((max_label + 1, len(offsets), levels, levels), np.int64)
    for k, (dy, dx) in enumerate(offsets):
        for y in range(H):
            for x in range(W):
                for sym in range(2 if symmetric else 1):
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < H and 0 <= qx < W):
                        continue
                    R = int(labels[y, x])
                    if R != int(labels[qy, qx]) or not 0 <= R <= max_label:
                        continue
                    if within is not None and (within[y, x] == 0 or within[qy, qx] == 0):
                        continue
                    a, b = lut[int(values[y, x])], lut[int(values[qy, qx])]
                    if sym:
                        a, b = b, a
                    out[R, k, a, b] += 1
    return out


def loop_properties(table):
    """One table [levels, levels] of integers -> dict of floats, every sum written out."""
    lv = table.shape[0]
    n = float(sum(int(table[i, j]) for i in range(lv) for j in range(lv)))
    if n == 0:
        return dict.fromkeys(ref.PROPERTIES, 0.0)
    P = [[int(table[i, j]) / n for j in range(lv)] for i in range(lv)]
    out = dict(contrast=0.0, dissimilarity=0.0, homogeneity=0.0, ASM=0.0, entropy=0.0)
    mu_i = mu_j = 0.0
    for i in range(lv):
        for j in range(lv):
            p = P[i][j]
            out['contrast'] += p * (i - j) ** 2
            out['dissimilarity'] += p * abs(i - j)
            out['homogeneity'] += p / (1 + (i - j) ** 2)
            out['ASM'] += p * p
            if p > 0:
                out['entropy'] -= p * math.log2(p)
            mu_i += i * p
            mu_j += j * p
    out['energy'] = math.sqrt(out['ASM'])
    var_i = var_j = cov = 0.0
    for i in range(lv):
        for j in range(lv):
            var_i += P[i][j] * (i - mu_i) ** 2
            var_j += P[i][j] * (j - mu_j) ** 2
            cov += P[i][j] * (i - mu_i) * (j - mu_j)
    rows = sum(1 for i in range(lv) if any(table[i, j] for j in range(lv)))
    cols = sum(1 for j in range(lv) if any(table[i, j] for i in range(lv)))
    out['correlation'] = 1.0 if rows <= 1 or cols <= 1 else cov / (math.sqrt(var_i) * math.sqrt(var_j))
    out['sigma_product'] = math.sqrt(var_i) * math.sqrt(var_j)
    return out


def random_case(H, W, top, seed, frac=0.7):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, top + 1, (H, W)).astype(np.int32), rng.randint(0, 256, (H, W)).astype(np.uint8), rng.rand(H, W) < frac)


# ------------------------------------------------------------------ against loops
@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (7, 1), (2, 2), (5, 6), (9, 11), (0, 4), (4, 0)])
@pytest.mark.parametrize('symmetric', [False, True])
def test_tables_against_loops(shape, symmetric):
    labels, values, within = random_case(shape[0], shape[1], 2, 3 + shape[0])
    for levels in (2, 5, 16):
        lut = ref.level_lut(levels)
        for w in (None, within):
            for max_label in (2, 1, 4):                                 # 1: label 2 is refused and counted nowhere
                got = ref.tables(labels, values, ALL_OFFSETS, levels, lut, symmetric, max_label, w)
                assert got.dtype == np.int64 and got.shape == (max_label + 1, len(ALL_OFFSETS), levels, levels)
                assert np.array_equal(got, loop_tables(labels, values, ALL_OFFSETS, levels, lut, symmetric, max_label, w))
    assert ref.refused(labels, 1) == int((labels == 2).sum()) and ref.refused(labels, 2) == 0


def test_long_offsets_and_a_custom_lut_against_loops():
    labels, values, within = random_case(9, 11, 1, 11)
    lut = (np.random.RandomState(12).permutation(256) % 7).tolist()
    offsets = ((8, 10), (-8, -10), (9, 0), (0, 11), (16, 16), (3, -10))
    got = ref.tables(labels, values, offsets, 7, lut, True, 1, within)
    assert np.array_equal(got, loop_tables(labels, values, offsets, 7, lut, True, 1, within))
    assert got[:, 2:5].sum() == 0                                       # offsets that pass the image: no pair


# ------------------------------------------------------------------ by hand
def test_the_example_of_the_graycomatrix_documentation():
    image = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], np.uint8)
    lut = [min(v, 3) for v in range(256)]
    zero = np.zeros((4, 4), np.int32)
    got = ref.tables(zero, image, ((0, 1), (1, 0)), 4, lut, False, 0, None)
    assert got[0, 0].tolist() == [[2, 2, 1, 0], [0, 2, 0, 0], [0, 0, 3, 1], [0, 0, 0, 1]]
    assert got[0, 1].tolist() == [[3, 0, 2, 0], [0, 2, 2, 0], [0, 0, 1, 2], [0, 0, 0, 0]]
    sym = ref.tables(zero, image, ((0, 1),), 4, lut, True, 0, None)
    assert sym[0, 0].tolist() == [[4, 2, 1, 0], [2, 4, 0, 0], [1, 0, 6, 1], [0, 0, 1, 2]]


def test_two_labels_by_hand():
    labels = np.array([[1, 1, 2], [1, 2, 2]], np.int32)
    values = np.array([[0, 255, 255], [255, 0, 255]], np.uint8)          # levels [[0, 1, 1], [1, 0, 1]]
    offsets = ((0, 1), (1, 0), (1, -1))
    got = ref.tables(labels, values, offsets, 2, None, False, 2, None)
    want = np.zeros((3, 3, 2, 2), np.int64)
    want[1, 0, 0, 1] = 1      # (0,0) -> (0,1)
    want[2, 0, 0, 1] = 1      # (1,1) -> (1,2)
    want[1, 1, 0, 1] = 1      # (0,0) -> (1,0)
    want[2, 1, 1, 1] = 1      # (0,2) -> (1,2)
    want[1, 2, 1, 1] = 1      # (0,1) -> (1,0)
    want[2, 2, 1, 0] = 1      # (0,2) -> (1,1)
    assert np.array_equal(got, want)
    within = np.ones((2, 3), np.uint8)
    within[1, 2] = 0                                                    # a partner twice, never an anchor of a counted pair
    want[2, 0, 0, 1] = want[2, 1, 1, 1] = 0
    assert np.array_equal(ref.tables(labels, values, offsets, 2, None, False, 2, within), want)
    assert np.array_equal(ref.tables(labels, values, offsets, 2, None, True, 2, within), want + want.transpose(0, 1, 3, 2))
    # the background is a region like any other, and a label above max_label is counted nowhere
    got = ref.tables(labels - 1, values, offsets, 2, None, False, 0, None)
    assert got.shape[0] == 1 and np.array_equal(got[0], ref.tables(labels, values, offsets, 2, None, False, 2, None)[1])


# ------------------------------------------------------------------ identities
def test_identities():
    labels, values, within = random_case(9, 11, 3, 21)
    lut = ref.level_lut(6, 20, 200)
    plain = ref.tables(labels, values, ALL_OFFSETS, 6, lut, False, 3, within)
    sym = ref.tables(labels, values, ALL_OFFSETS, 6, lut, True, 3, within)
    assert np.array_equal(sym, plain + plain.transpose(0, 1, 3, 2))
    back = ref.tables(labels, values, [(-dy, -dx) for dy, dx in ALL_OFFSETS], 6, lut, False, 3, within)
    assert np.array_equal(back, plain.transpose(0, 1, 3, 2))
    for H, W in ((9, 11), (1, 5), (3, 3)):
        one = np.zeros((H, W), np.int32)
        values = np.random.RandomState(H).randint(0, 256, (H, W)).astype(np.uint8)
        t = ref.tables(one, values, ALL_OFFSETS, 4, None, False, 0, None)
        assert t.sum(axis=(0, 2, 3)).tolist() == [max(0, H - abs(dy)) * max(0, W - abs(dx)) for dy, dx in ALL_OFFSETS]


def test_level_lut():
    for levels in (2, 4, 8, 16):
        assert ref.level_lut(levels) == [v * levels >> 8 for v in range(256)]
    for levels in range(2, 17):
        for lo, hi in ((0, 255), (20, 159), (0, 1), (254, 255), (100, 101), (7, 250)):
            lut = ref.level_lut(levels, lo, hi)
            assert len(lut) == 256 and lut[0] == 0 and lut[255] == levels - 1 and min(lut) == 0 and max(lut) == levels - 1
            assert all(a <= b for a, b in zip(lut, lut[1:]))              # monotone
            assert all(lut[v] == 0 for v in range(lo + 1)) and all(lut[v] == levels - 1 for v in range(hi, 256))
    assert ref.level_lut(3, 10, 13) == [0] * 11 + [0, 1] + [2] * 243      # 11 -> floor(3 / 4), 12 -> floor(6 / 4)


# ------------------------------------------------------------------ properties
REL, ABS, CORR_ABS = 2.0 ** -23, 2.0 ** -40, 2.0 ** -22                  # the bounds of tests/test_cooc_gpu.py


def test_properties_against_loops_within_the_bound_of_the_gpu_test():
    labels, values, within = random_case(40, 50, 5, 31)
    for levels, symmetric in ((16, True), (7, False), (2, True)):
        t = ref.tables(labels, values, ref.DIRECTIONS, levels, None, symmetric, 5, within)
        got = ref.properties(t)
        assert got.dtype == np.float64 and got.shape == (6, 4, 7)
        smallest = np.inf
        for R in range(6):
            for k in range(4):
                want = loop_properties(t[R, k])
                smallest = min(smallest, want['sigma_product'])
                for c, name in enumerate(ref.PROPERTIES):
                    bound = CORR_ABS if name == 'correlation' else REL * abs(want[name]) + ABS
                    assert abs(got[R, k, c] - want[name]) <= bound, (name, R, k)
        # float64 error of the centred correlation: 256 terms of at most 15^2, over sigma_i sigma_j
        assert 256 * 15 ** 2 * 2.0 ** -52 / smallest < CORR_ABS


def test_properties_of_tables_by_hand():
    t = np.zeros((1, 5, 3, 3), np.int64)
    t[0, 0] = [[2, 0, 0], [0, 0, 0], [0, 0, 2]]                           # P = 1/2 at (0, 0) and (2, 2)
    t[0, 1] = [[0, 0, 4], [0, 0, 0], [4, 0, 0]]                           # P = 1/2 at (0, 2) and (2, 0)
    t[0, 2] = [[0, 0, 0], [0, 9, 0], [0, 0, 0]]                           # one level: correlation is 1 by rule
    t[0, 3] = [[0, 3, 5], [0, 0, 0], [0, 0, 0]]                           # one level in the anchors' marginal only
    got = ref.properties(t)
    names = ref.PROPERTIES
    assert dict(zip(names, got[0, 0])) == dict(contrast=0, dissimilarity=0, homogeneity=1, ASM=0.5, energy=math.sqrt(0.5), correlation=1,
                                               entropy=1)
    assert dict(zip(names, got[0, 1])) == dict(contrast=4, dissimilarity=2, homogeneity=0.2, ASM=0.5, energy=math.sqrt(0.5), correlation=-1,
                                               entropy=1)
    assert dict(zip(names, got[0, 2])) == dict(contrast=0, dissimilarity=0, homogeneity=1, ASM=1, energy=1, correlation=1, entropy=0)
    assert got[0, 3, 5] == 1.0 and got[0, 3, 0] == (3 * 1 + 5 * 4) / 8
    assert got[0, 4].tolist() == [0.0] * 7                              # n = 0
    assert ref.properties(t.transpose(0, 1, 3, 2))[0, 3, 5] == 1.0      # ... and in the partners' marginal only
