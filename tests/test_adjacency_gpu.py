"""Region adjacency and Voronoi graphs on the GPU (csrc/adjacency.hip through cgc_net_amd.nuclei.region_adjacency / voronoi_graph)
against tests/adjacency_ref.py (a numpy restatement, pinned by tests/test_adjacency_ref_cpu.py).  Every comparison is exact.

A workgroup folds one tile of side t = the library's exported tile side (plus a one-pixel halo) into a table in LDS that may hold 512
distinct pairs: the shapes put borders on the seams between tiles, on the image's last row and column, and more pairs into a tile
than the table folds."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei
from cgc_net_amd.data import Batch
from cgc_net_amd.graph import BatchGraph

import adjacency_ref as ref
from image_cases import DEV, gpu, tissue

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def tile_side():
    return kernels.get().adjacency_tile


def run(labels, connectivity=1, value=None):
    """The GPU's outputs as numpy arrays, their form checked."""
    lt = labels if torch.is_tensor(labels) else gpu(labels)
    vt = value if value is None or torch.is_tensor(value) else gpu(value)
    out = nuclei.region_adjacency(lt, connectivity, vt)
    assert len(out) == (2 if value is None else 3)
    pairs, count = out[:2]
    assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.device == lt.device and pairs.is_contiguous()
    for o in out[1:]:
        assert o.dtype == torch.int32 and tuple(o.shape) == (pairs.shape[0],) and o.device == lt.device
    return tuple(o.cpu().numpy() for o in out)


def check(labels, connectivity, value=None, want=None):
    """One call against the restatement (or against ``want``, computed once by the caller); returns the GPU's outputs."""
    got = run(labels, connectivity, value)
    wp, wc, wm = ref.region_adjacency(labels, connectivity, value) if want is None else want
    assert np.array_equal(got[0], wp), (got[0][:5], wp[:5], got[0].shape, wp.shape)
    assert np.array_equal(got[1], wc), np.argwhere(got[1] != wc)[:5]
    if value is not None:
        assert np.array_equal(got[2], wm), np.argwhere(got[2] != wm)[:5]
    return got


# ------------------------------------------------------------------ degenerate images
@pytest.mark.parametrize('shape', [(0, 5), (5, 0), (1, 1), (1, 7), (7, 1)], ids=lambda s: '%dx%d' % s)
def test_degenerate_shapes(shape):
    rng = np.random.RandomState(3)
    for connectivity in (1, 2):
        for labels in (np.ones(shape, np.int32), rng.randint(0, 3, size=shape).astype(np.int32)):
            check(labels, connectivity)
            check(labels, connectivity, value=rng.randint(-9, 9, size=shape).astype(np.int32))


def test_no_contact_and_two_halves():
    H, W = 37, 45
    for connectivity in (1, 2):
        for labels in (np.zeros((H, W), np.int32), np.full((H, W), 7, np.int32)):      # all zero, one label only
            pairs, count = check(labels, connectivity)
            assert pairs.shape == (0, 2) and count.shape == (0,)
        two = np.full((H, W), 3, np.int32)
        two[:, 20:] = 9
        pairs, count = check(two, connectivity)
        assert pairs.tolist() == [[3, 9]] and count.tolist() == [H if connectivity == 1 else H + 2 * (H - 1)]
        gap = two.copy()
        gap[:, 20] = 0                                                                  # background between them: no contact
        assert check(gap, connectivity)[0].shape == (0, 2)


# ------------------------------------------------------------------ seams between tiles
def seam_sides():
    t = tile_side()
    return [t - 1, t, t + 1, 2 * t + 1]


def test_borders_on_tile_seams():
    t = tile_side()
    for H in seam_sides():
        for W in seam_sides():
            cols = np.ones((H, W), np.int32)
            cols[:, t:] = 2                                                             # meet exactly on column t - 1 | t
            rows = np.ones((H, W), np.int32)
            rows[t:, :] = 2                                                             # ... on row t - 1 | t
            quad = 1 + (np.arange(H)[:, None] >= t) * 2 + (np.arange(W)[None, :] >= t)
            last = np.ones((H, W), np.int32)
            last[H - 1, :] = 5                                                          # the image's last row and column
            last[:, W - 1] = 6
            for connectivity in (1, 2):
                for labels in (cols, rows, quad.astype(np.int32), last):
                    check(labels, connectivity)
                pairs, count = run(cols, connectivity)
                assert (pairs.tolist() == [[1, 2]] and count.tolist() == [H if connectivity == 1 else 3 * H - 2]) if W > t else len(pairs) == 0


def test_single_pixels_across_tile_corners():
    t = tile_side()
    for H in seam_sides():
        for W in seam_sides():
            if H <= t or W <= t:
                continue
            corners = [(cy, cx) for cy in range(t, H, t) for cx in range(t, W, t)]
            for down_right in (True, False):
                labels = np.zeros((H, W), np.int32)
                for k, (cy, cx) in enumerate(corners):                                  # two single pixels that meet only across the corner
                    labels[cy - 1, cx - 1 if down_right else cx] = 10 + 2 * k
                    labels[cy, cx if down_right else cx - 1] = 11 + 2 * k
                assert check(labels, 1)[0].shape == (0, 2)
                pairs, count = check(labels, 2)
                assert pairs.tolist() == [[10 + 2 * k, 11 + 2 * k] for k in range(len(corners))] and np.all(count == 1)


# ------------------------------------------------------------------ table pressure
@pytest.mark.parametrize('shape', [(96, 96), (130, 70)], ids=lambda s: '%dx%d' % s)
def test_all_distinct_labels(shape):
    H, W = shape
    labels = np.random.RandomState(1).permutation(H * W).astype(np.int32).reshape(H, W) + 1      # every contact is its own pair
    value = np.random.RandomState(2).randint(-1000, 1000, size=shape).astype(np.int32)
    for connectivity in (1, 2):
        pairs, count, _ = check(labels, connectivity, value)
        want = H * (W - 1) + W * (H - 1) + (2 * (H - 1) * (W - 1) if connectivity == 2 else 0)
        assert len(pairs) == want and np.all(count == 1)
    if shape == (96, 96):
        assert len(run(labels, 1)[0]) == 18240 and len(run(labels, 2)[0]) == 36290


@functools.lru_cache(maxsize=None)
def noise(labels_n, side, seed):
    rng = np.random.RandomState(seed)
    labels = rng.randint(1, labels_n + 1, size=(side, side)).astype(np.int32)
    value = rng.randint(-2 ** 20, 2 ** 20, size=(side, side)).astype(np.int32)
    return labels, value, {c: ref.region_adjacency(labels, c, value) for c in (1, 2)}


def test_noise_over_three_labels():
    labels, value, want = noise(3, 200, 11)                                             # three pairs, every lane on the same keys
    for connectivity in (1, 2):
        pairs, count, _ = check(labels, connectivity, value, want[connectivity])
        assert pairs.tolist() == [[1, 2], [1, 3], [2, 3]]


def test_noise_over_a_thousand_labels():
    labels, value, want = noise(1000, 128, 12)                                          # thousands of pairs per tile: past what the table folds
    for connectivity in (1, 2):
        check(labels, connectivity, value, want[connectivity])


def test_one_frequent_pair_in_a_tile_past_the_table():
    """A tile with more distinct pairs than the table folds AND one pair with thousands of contacts: the per-contact records of that
    pair meet again in the merge."""
    t = tile_side()
    labels = np.where(np.random.RandomState(4).rand(2 * t, 2 * t) < 0.5, 1, 2).astype(np.int32)
    labels[:t:2, :t:2] = (3 + np.arange((t // 2) ** 2)).reshape(t // 2, t // 2)           # 1024 own labels in the first tile
    for connectivity in (1, 2):
        check(labels, connectivity, np.random.RandomState(5).randint(-50, 50, size=labels.shape).astype(np.int32))


# ------------------------------------------------------------------ values of labels, dtypes, strides
def test_extreme_labels_in_signed_order():
    rng = np.random.RandomState(8)
    pool = np.array([0, INT32_MIN, -1, 1, INT32_MAX, INT32_MIN + 1, INT32_MAX - 1], dtype=np.int64)
    labels = pool[rng.randint(0, len(pool), size=(70, 131))].astype(np.int32)
    for connectivity in (1, 2):
        pairs, _ = check(labels, connectivity)
        assert pairs[0].tolist() == [INT32_MIN, INT32_MIN + 1] and pairs[-1].tolist() == [INT32_MAX - 1, INT32_MAX]
        assert np.all(pairs[:, 0] < pairs[:, 1])
        keys = [tuple(r) for r in pairs.tolist()]
        assert keys == sorted(set(keys))


@pytest.mark.parametrize('dtype', [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32], ids=str)
def test_every_accepted_dtype(dtype):
    rng = np.random.RandomState(9)
    lo, hi = {torch.bool: (0, 2), torch.uint8: (0, 256), torch.int8: (-128, 128), torch.int16: (-300, 300), torch.int32: (-300, 300)}[dtype]
    labels = gpu(rng.randint(lo, hi, size=(67, 90))).to(dtype)
    value = gpu(rng.randint(lo, hi, size=(67, 90))).to(dtype)
    as32 = lambda t: t.to(torch.int32).cpu().numpy()                                    # noqa: E731
    want = ref.region_adjacency(as32(labels), 2, as32(value))
    got = run(labels, 2, value)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    if dtype == torch.bool:
        assert got[0].shape == (0, 2)                                                   # one region only


def test_views_equal_their_contiguous_copies():
    rng = np.random.RandomState(10)
    base = gpu(rng.randint(0, 6, size=(140, 150)).astype(np.int32))
    vals = gpu(rng.randint(-99, 99, size=(140, 150)).astype(np.int32))
    for view in (lambda t: t.t(), lambda t: t[3:133:2, 5:140:3], lambda t: t[:, 1:]):
        lv, vv = view(base), view(vals)
        assert not lv.is_contiguous()
        a = run(lv, 2, vv)
        b = run(lv.contiguous(), 2, vv.contiguous())
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        check(lv.cpu().numpy(), 2, vv.cpu().numpy())


# ------------------------------------------------------------------ value
def test_random_values_and_the_clamp():
    rng = np.random.RandomState(13)
    labels = rng.randint(0, 5, size=(75, 133)).astype(np.int32)
    value = rng.randint(INT32_MIN, INT32_MAX, size=labels.shape, dtype=np.int64).astype(np.int32)
    for connectivity in (1, 2):
        check(labels, connectivity, value)
    two = np.ones((5, 70), np.int32)
    two[:, 64:] = 2
    for fill, want in ((INT32_MAX, INT32_MAX), (INT32_MIN, INT32_MIN)):                 # both ends at the limit: the sum is clamped
        _, _, min_sum = check(two, 1, np.full(two.shape, fill, np.int32))
        assert min_sum.tolist() == [want]
    mixed = np.full(two.shape, INT32_MAX, np.int32)
    mixed[2, 63], mixed[2, 64] = INT32_MIN, INT32_MAX
    assert check(two, 1, mixed)[2].tolist() == [-1]
    assert len(nuclei.region_adjacency(gpu(two))) == 2                                  # min_sum absent without value


# ------------------------------------------------------------------ tissue
@functools.lru_cache(maxsize=None)
def tissue_cells(distance):
    """The GPU's own expand_labels output, fed to both sides: a difference is then the new kernel's, not the distance transform's."""
    labels = tissue()[0]
    cells = nuclei.expand_labels(gpu(labels), distance)
    dist2 = nuclei.distance_transform(gpu(labels), sites='nonzero', max_distance=distance)
    t = torch.where(dist2 == nuclei.EDT_INF, 0, nuclei._eighths(dist2))
    return cells.cpu().numpy(), t.cpu().numpy()


def test_tissue_raw_labels():
    labels = tissue()[0]
    assert len(check(labels, 1)[0]) == 11 and len(check(labels, 2)[0]) == 13


@pytest.mark.parametrize('distance', [10, 50])
def test_tissue_cells(distance):
    cells, t = tissue_cells(distance)
    for connectivity in (1, 2):
        pairs, _, _ = check(cells, connectivity, t)
        if distance == 50 and connectivity == 1:
            assert len(pairs) == 146


def test_outputs_are_bit_identical_from_call_to_call():
    labels, value, _ = noise(1000, 128, 12)
    cells, t = tissue_cells(50)
    for lab, val in ((labels, value), (cells, t)):
        lt, vt = gpu(lab), gpu(val)
        first = [o.clone() for o in nuclei.region_adjacency(lt, 2, vt)]
        second = nuclei.region_adjacency(lt, 2, vt)
        assert all(torch.equal(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------ voronoi_graph
@functools.lru_cache(maxsize=None)
def tissue_nodes():
    labels, gray, _ = tissue()
    feats, cen, kept = nuclei.nucleus_features(gpu(labels), gpu(gray), min_size=10)
    return feats, cen, kept


@functools.lru_cache(maxsize=None)
def wanted_cells(with_kept):
    """Steps 1 to 3 of the restatement, once for all options."""
    return ref.voronoi_cells(tissue()[0], 50, tissue_nodes()[2].cpu().numpy() if with_kept else None)


def check_graph(edge_index, n, loop):
    e = edge_index.cpu().numpy()
    assert edge_index.dtype == torch.int64 and e.shape[0] == 2
    assert e.size == 0 or (e.min() >= 0 and e.max() < n)                                # every end is a node
    assert np.array_equal(e[:, np.lexsort((e[1], e[0]))], e)                            # sorted: centres, then columns
    pairs = set(map(tuple, e.T.tolist()))
    assert len(pairs) == e.shape[1] and pairs == set((j, i) for i, j in pairs)          # each once, symmetric
    assert [(i, i) in pairs for i in range(n)] == [loop] * n                            # loops iff asked


@pytest.mark.parametrize('with_kept', [True, False], ids=['kept', 'all'])
def test_voronoi_graph_against_the_restatement(with_kept):
    labels = tissue()[0]
    kept = tissue_nodes()[2] if with_kept else None
    kept_np = None if kept is None else kept.cpu().numpy()
    n = len(kept_np) if with_kept else 59
    assert n == (len(kept_np) if with_kept else len(np.unique(labels[labels != 0]))) and (not with_kept or n < 59)
    for connectivity, loop, max_gap in ((1, True, None), (1, False, 20), (2, True, 20), (2, False, None), (1, True, 0), (2, False, 0)):
        want = ref.graph_of_cells(*wanted_cells(with_kept), connectivity=connectivity, loop=loop, max_gap=max_gap)
        got = nuclei.voronoi_graph(gpu(labels), 50, kept, connectivity, loop, max_gap, return_attr=True)
        check_graph(got[0], n, loop)
        assert got[1].dtype == torch.int32 and got[2].dtype == torch.float32
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w)
        plain = nuclei.voronoi_graph(gpu(labels), 50, kept, connectivity, loop, max_gap)
        assert torch.is_tensor(plain) and torch.equal(plain, got[0])
        if max_gap == 0:
            assert got[0].shape[1] == (n if loop else 0)
    if with_kept:                                                                       # the sub-10-pixel objects claim no cell
        cells = wanted_cells(True)[1]
        assert set(np.unique(cells).tolist()) <= set([0] + kept_np.tolist())


def test_into_the_models_structure():
    labels = tissue()[0]
    feats, cen, kept = tissue_nodes()
    n = kept.numel()
    items, degrees = [], []
    for connectivity, max_gap in ((1, None), (2, 20)):
        ei = nuclei.voronoi_graph(gpu(labels), 50, kept, connectivity, True, max_gap)
        items.append(nuclei.graph_item(feats, cen, 1, edge_index=ei))
        assert items[-1].edge_index.device.type == 'cpu' and items[-1].edge_index.dtype == torch.int64
        degrees.append(ref.degrees(ref.graph_of_cells(*wanted_cells(True), connectivity=connectivity, loop=True, max_gap=max_gap)[0], n))
    batch = Batch.from_data_list(items, device=DEV)
    assert batch.edge_index.device == DEV and batch.x.shape == (2 * n, 18)
    g = BatchGraph.from_batch(batch).validate()
    rowptr = g.rowptr.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.diff(rowptr), np.concatenate(degrees))
