"""Seeded watershed on the GPU (csrc/watershed.hip through cgc_net_amd.nuclei.watershed / split_touching(growth='flood') and the kernel
table's watershed_flood) against tests/watershed_ref.py (a heap Dijkstra over the flood key, parents by their definition, roots by
following pointers; pinned by tests/test_watershed_ref_cpu.py).  Every comparison is exact: level, source and labels.

The kernel relaxes 64 x 64 tiles with a one-pixel halo, 16 pixels per thread, in rounds that are launches, then resolves the parent
pointers by jumping: the shapes sit under, on and one over a tile and span 3 x 2 tiles, the plateau, the basins and the staircases
cross tile borders and the corner at (64, 64), and the serpentine valley needs more than one batch of rounds and of jumps."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import edt_ref
import geodesic_ref
import reconstruct_ref
import watershed_ref as ref
from image_cases import DEV, gpu, tissue
from test_geodesic_gpu import staircase

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (63, 63), (64, 64), (65, 65), (63, 65), (130, 70)]
HEIGHT_DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32]
MARKER_DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64]
LOW, HIGH = ref.INT32_MIN, ref.INT32_MAX


def flood(height, seeds, within=None, metric='chamfer', connectivity=1):
    """(level, source) of the kernel table, as numpy."""
    a, b = geodesic_ref.steps_of(metric)
    h = gpu(np.asarray(height).astype(np.int32))
    s = gpu(seeds)
    w = None if within is None else gpu(within)
    level, source = kernels.get().watershed_flood(h, s, w, a, b, connectivity)
    for o in (level, source):
        assert o.dtype == torch.int32 and o.device == h.device and tuple(o.shape) == tuple(h.shape) and o.is_contiguous()
    return level.cpu().numpy(), source.cpu().numpy()


def check(height, seeds, within=None, metric='chamfer', connectivity=1):
    wl, ws = ref.flood(height, seeds, within, metric, connectivity)
    level, source = flood(height, seeds, within, metric, connectivity)
    assert np.array_equal(level, wl), (metric, connectivity, np.argwhere(level != wl)[:5])
    assert np.array_equal(source, ws), (metric, connectivity, np.argwhere(source != ws)[:5])
    return wl, ws


def blobs(rng, shape, levels=4, cell=5, noise=0.15):
    """int64 heights in 0 .. levels - 1: plateaus of ``cell`` x ``cell`` pixels with single pixels flipped."""
    coarse = rng.randint(0, levels, size=(shape[0] // cell + 2, shape[1] // cell + 2))
    h = np.kron(coarse, np.ones((cell, cell), np.int64))[:shape[0], :shape[1]]
    return np.where(rng.rand(*shape) < noise, rng.randint(0, levels, size=shape), h).astype(np.int64)


def sparse_seeds(rng, shape, p):
    seeds = rng.rand(*shape) < p
    if not seeds.any():
        seeds[rng.randint(shape[0]), rng.randint(shape[1])] = True
    return seeds


# ------------------------------------------------------------------ tile geometry
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_heights(shape):
    rng = np.random.RandomState(19 * shape[0] + shape[1])
    k = 0
    for metric in ((5, 7), (1, 1)):
        for connectivity in (1, 2):
            height = blobs(rng, shape) if k % 2 == 0 else rng.randint(-3, 4, size=shape).astype(np.int64)
            within = None if k == 1 else rng.rand(*shape) < (0.7, 0.85, 1.0)[k % 3]
            check(height, sparse_seeds(rng, shape, (0.003, 0.02)[k % 2]), within, metric, connectivity)
            k += 1


@pytest.mark.parametrize('shape', [(1, 1), (9, 1), (65, 63), (130, 70)], ids=lambda s: '%dx%d' % s)
def test_no_seed_every_seed_and_seeds_outside_within(shape):
    rng = np.random.RandomState(5 * shape[0] + shape[1])
    height = blobs(rng, shape)
    within = rng.rand(*shape) < 0.8
    for connectivity in (1, 2):
        level, source = check(height, np.zeros(shape, bool), within, 'chamfer', connectivity)            # no seed: nothing is reached
        assert (source == -1).all() and np.array_equal(level, height)
        level, source = check(height, np.ones(shape, np.uint8), within, 'chamfer', connectivity)         # every pixel a seed
        assert np.array_equal(source.ravel(), np.arange(height.size)) and np.array_equal(level, height)
    seeds = sparse_seeds(rng, shape, 0.01) & ~within                                                     # seeds outside within only
    seeds[shape[0] // 2, shape[1] // 2] = True
    within[shape[0] // 2, shape[1] // 2] = False
    level, source = check(height, seeds, within, 'chamfer', 1)
    assert (source[seeds] >= 0).all() and np.array_equal(source >= 0, geodesic_ref.seeded_components(seeds, within, 1))


# ------------------------------------------------------------------ plateaus and basins across tile borders
def field(rng, shape=(130, 130)):
    return 4 + blobs(rng, shape, levels=3)                               # 4 .. 6


def test_plateau_across_the_tile_corner():
    rng = np.random.RandomState(3)
    height = field(rng)
    height[40:90, 38:92] = 5                                             # one plateau over all four tiles around (64, 64)
    seeds = np.zeros(height.shape, bool)
    seeds[3, 5] = seeds[120, 10] = seeds[70, 125] = seeds[45, 60] = True
    for connectivity in (1, 2):
        level, _ = check(height, seeds, None, 'chamfer', connectivity)
        assert (level[40:90, 38:92] == 5).all()                          # the water runs level over it: only the way travelled decides
    check(height, seeds, None, 'cityblock', 1)


def test_unmarked_basin_across_the_tile_corner():
    rng = np.random.RandomState(4)
    height = field(rng)
    height[55:75, 55:75] = 9                                             # the rim
    height[56:74, 56:74] = blobs(rng, (18, 18), levels=3)                # the floor, 0 .. 2, over the corner at (64, 64); no seed inside
    height[60, 74] = 7                                                   # the lowest pass
    height[74, 66] = 8                                                   # a higher one
    seeds = np.zeros(height.shape, bool)
    seeds[5, 5] = seeds[125, 120] = True
    for connectivity in (1, 2):
        level, source = check(height, seeds, None, 'chamfer', connectivity)
        assert (level[56:74, 56:74] == 7).all()                          # filled to its lowest pass
        assert len(np.unique(source[56:74, 56:74])) == 1                 # by the water that came over it


def test_basin_whose_pass_lies_in_another_tile():
    rng = np.random.RandomState(5)
    height = field(rng, (70, 200))
    height[8:34, 8:34] = 9
    height[9:33, 9:33] = 0                                               # the floor, in tile (0, 0)
    height[18:23, 33:150] = 9
    height[19:22, 33:149] = 1                                            # a canal through tile (0, 1) into tile (0, 2)
    height[20, 149] = 6                                                  # the lowest pass, at the canal's far end
    seeds = np.zeros(height.shape, bool)
    seeds[60, 190] = seeds[65, 3] = True
    for connectivity in (1, 2):
        level, source = check(height, seeds, None, 'chamfer', connectivity)
        assert (level[9:33, 9:33] == 6).all() and (source[9:33, 9:33] == 60 * 200 + 190).all()


@pytest.mark.parametrize('anti', [False, True], ids=['main', 'anti'])
def test_staircase_across_a_tile_corner(anti):
    dom, path = staircase(anti)
    rng = np.random.RandomState(6 + anti)
    height = rng.randint(0, 3, size=dom.shape).astype(np.int64)
    for end in (0, -1):
        seeds = np.zeros_like(dom)
        seeds[path[end]] = True
        _, source = check(height, seeds, dom, 'chamfer', 2)
        assert np.array_equal(source >= 0, dom)                          # conducted through the pure corner contact at (64, 64)
        _, source = check(height, seeds, dom, 'chamfer', 1)
        assert 0 < (source >= 0).sum() < dom.sum()                       # stops there
        check(height, seeds, dom, 'cityblock', 1)


@pytest.mark.parametrize('connectivity', [1, 2])
def test_porous_domain_with_corner_contacts(connectivity):
    rng = np.random.RandomState(8 + connectivity)
    shape = (70, 130)
    within = rng.rand(*shape) < 0.55                                     # near the percolation threshold: corner contacts everywhere
    seeds = sparse_seeds(rng, shape, 0.004)
    height = blobs(rng, shape)
    for metric in ('chamfer', 'cityblock', (3, 4)):
        _, source = check(height, seeds, within, metric, connectivity)
        comp = 1 if geodesic_ref.steps_of(metric)[1] == 0 else connectivity
        assert np.array_equal(source >= 0, geodesic_ref.seeded_components(seeds, within, comp))


# ------------------------------------------------------------------ many rounds, many jumps
def test_serpentine_valley_needs_many_rounds_and_jumps():
    valley = np.ones((130, 131), bool)
    for i, r in enumerate(range(1, 130, 2)):
        valley[r, :] = False
        valley[r, 130 if i % 2 == 0 else 0] = True
    height = np.where(valley, 0, 100).astype(np.int32)                   # walls of 100 between the turns
    seeds = np.zeros_like(valley)
    seeds[0, 0] = True
    wl, ws = ref.flood(height, seeds)
    assert (ws == 0).all() and np.array_equal(wl, height)                # one basin; the valley floor is never raised
    keys = ref.flood_keys(height, seeds)
    assert max(k[1] for k in keys.values()) > 5 * 2 ** 10                # the water runs level for more than 2^10 steps
    h, s = gpu(height), gpu(seeds)
    table = kernels.get()
    first = table.watershed_flood(h, s, None, 5, 7, 1)
    rounds, jumps = table.watershed_rounds, table.watershed_jumps
    second = table.watershed_flood(h, s, None, 5, 7, 1)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert np.array_equal(first[0].cpu().numpy(), wl) and np.array_equal(first[1].cpu().numpy(), ws)
    assert rounds > 8 and jumps >= 11
    table.watershed_flood(h, gpu(np.ones_like(seeds)), None, 5, 7, 1)   # every pixel a seed: one batch of each
    assert (table.watershed_rounds, table.watershed_jumps) == (kernels.GEO_FIRST_BATCH, kernels.WS_JUMP_BATCH)


# ------------------------------------------------------------------ values
@pytest.mark.parametrize('shape', [(9, 1), (65, 63), (130, 70)], ids=lambda s: '%dx%d' % s)
def test_the_whole_int32_range(shape):
    rng = np.random.RandomState(23 * shape[0] + shape[1])
    seeds = sparse_seeds(rng, shape, 0.01)
    height = rng.randint(LOW, HIGH + 1, size=shape, dtype=np.int64)
    height.ravel()[rng.randint(height.size)] = LOW
    height.ravel()[rng.randint(height.size)] = HIGH
    check(height, seeds, None, 'chamfer', 2)
    ends = np.where(rng.rand(*shape) < 0.5, LOW, HIGH).astype(np.int64)   # only the two ends: plateaus at INT32_MIN beside seeds
    check(ends, seeds, rng.rand(*shape) < 0.9, 'chamfer', 1)
    for value in (5, LOW, HIGH):
        level, source = check(np.full(shape, value, np.int64), seeds, None, 'chamfer', 1)               # a constant image
        assert (level == value).all() and (source >= 0).all()


@pytest.mark.parametrize('connectivity', [1, 2])
def test_level_is_the_reconstruction_by_erosion(connectivity):
    """GPU against GPU: with the whole image as the domain, level on reached non-seed pixels is the reconstruction by erosion of
    min(height, g) from g = INT32_MIN on seeds, INT32_MAX elsewhere."""
    rng = np.random.RandomState(40 + connectivity)
    shape = (130, 70)
    height = gpu(blobs(rng, shape, levels=6).astype(np.int32) * 1000 - 2500)
    seeds = gpu(sparse_seeds(rng, shape, 0.003))
    metric = 'chamfer' if connectivity == 2 else 'cityblock'
    labels, level = nuclei.watershed(height, seeds, metric=metric, connectivity=connectivity, return_level=True)
    g = torch.where(seeds, torch.full_like(height, LOW), torch.full_like(height, HIGH))
    want = nuclei.reconstruct(g, torch.minimum(height, g), 'erosion', connectivity)
    assert labels.dtype == torch.bool and labels.all() and level.dtype == torch.int32
    assert torch.equal(level[~seeds], want[~seeds]) and torch.equal(level[seeds], height[seeds])


# ------------------------------------------------------------------ input forms
@functools.lru_cache(maxsize=None)
def form_case():
    rng = np.random.RandomState(13)
    shape = (70, 133)
    height = blobs(rng, shape, levels=5) * 20 + rng.randint(0, 3, size=shape)      # 0 .. 82: fits every dtype but bool
    markers = np.where(rng.rand(*shape) < 0.004, rng.randint(1, 100, size=shape), 0)
    within = rng.rand(*shape) < 0.9
    return height, markers, within


@functools.lru_cache(maxsize=None)
def form_want(binary):
    height, markers, within = form_case()
    return ref.watershed((height > 40) if binary else height, markers, within, 'chamfer', 2)


@pytest.mark.parametrize('dtype', HEIGHT_DTYPES, ids=str)
def test_height_dtypes(dtype):
    height, markers, within = form_case()
    want, want_level = form_want(dtype == torch.bool)
    h = gpu(height > 40) if dtype == torch.bool else gpu(height).to(dtype)
    labels, level = nuclei.watershed(h, gpu(markers), gpu(within), connectivity=2, return_level=True)
    assert labels.dtype == torch.int64 and level.dtype == torch.int32 and labels.is_contiguous()
    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(level.cpu().numpy(), want_level)


@pytest.mark.parametrize('dtype', MARKER_DTYPES, ids=str)
def test_marker_dtypes(dtype):
    height, markers, within = form_case()
    want, _ = form_want(False)
    m = gpu(markers != 0) if dtype == torch.bool else gpu(markers).to(dtype)
    labels = nuclei.watershed(gpu(height).to(torch.int16), m, gpu(within).to(dtype), connectivity=2)
    assert labels.dtype == dtype and tuple(labels.shape) == markers.shape
    got = labels.cpu().numpy()
    assert np.array_equal(got, want != 0) if dtype == torch.bool else np.array_equal(got.astype(np.int64), want)
    assert torch.equal(labels[m != 0], m[m != 0])                        # marker pixels unchanged


def test_views():
    height, markers, within = form_case()
    want, want_level = ref.watershed(height.T, markers.T, within.T, 'chamfer', 2)
    ht, mt, wt = gpu(height.astype(np.int32)).t(), gpu(markers.astype(np.int16)).t(), gpu(within).t()
    assert not ht.is_contiguous()
    labels, level = nuclei.watershed(ht, mt, wt, connectivity=2, return_level=True)
    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(level.cpu().numpy(), want_level)
    want, want_level = form_want(False)
    wide_h = gpu(np.repeat(np.repeat(height.astype(np.int16), 2, axis=0), 3, axis=1))[::2, ::3]
    wide_m = gpu(np.repeat(np.repeat(markers.astype(np.uint8), 2, axis=0), 3, axis=1))[::2, ::3]
    wide_w = gpu(np.repeat(np.repeat(within, 2, axis=0), 3, axis=1))[::2, ::3]
    assert not wide_h.is_contiguous() and tuple(wide_h.shape) == height.shape
    labels, level = nuclei.watershed(wide_h, wide_m, wide_w, connectivity=2, return_level=True)
    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(level.cpu().numpy(), want_level)
    assert np.array_equal(wide_h.cpu().numpy(), height) and np.array_equal(wide_m.cpu().numpy(), markers)      # inputs left alone


def test_empty_images():
    for shape in ((0, 5), (4, 0), (0, 0)):
        h = torch.zeros(shape, dtype=torch.int16, device=DEV)
        m = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        labels, level = nuclei.watershed(h, m, return_level=True)
        assert tuple(labels.shape) == shape and labels.dtype == torch.uint8 and tuple(level.shape) == shape and level.dtype == torch.int32
        lab, n = nuclei.split_touching(m, 2, growth='flood')
        assert tuple(lab.shape) == shape and lab.dtype == torch.int32 and n == 0
        lab, n = nuclei.split_touching(m, None, growth='flood', markers='h_maxima', h=1)
        assert tuple(lab.shape) == shape and n == 0


def test_overflowing_sizes_are_refused_before_any_launch():
    h = torch.zeros(1, 1, dtype=torch.int32, device=DEV).expand(20000, 20000)      # 7 H W reaches 2^31; no memory behind it
    with pytest.raises(ValueError):
        nuclei.watershed(h, h)


# ------------------------------------------------------------------ split_touching(growth='flood')
def test_two_discs_are_cut_at_the_neck():
    mask, big = ref.disc_pair()
    t = gpu(mask)
    lab, n = nuclei.split_touching(t, None, growth='flood', markers='h_maxima', h=2)
    want, wn = ref.split_touching_flood(mask, None, markers='h_maxima', h=2)
    got = lab.cpu().numpy()
    assert n == wn == 2 and np.array_equal(got, want)
    cut, large, small = ref.cut_of(got)
    assert abs(cut - ref.NECK) <= 2 and abs(large - big) <= 0.01 * big
    glab, gn = nuclei.split_touching(t, None, growth='geodesic', markers='h_maxima', h=2)
    gcut, glarge, _ = ref.cut_of(glab.cpu().numpy())
    assert gn == 2 and gcut == 55 and big - glarge > 0.05 * big          # the geodesic midline: unchanged


@functools.lru_cache(maxsize=None)
def tissue_mask():
    return tissue()[0] > 0


@pytest.mark.parametrize('markers,connectivity,min_size', [('core', 1, 0), ('core', 2, 10), ('h_maxima', 1, 0), ('h_maxima', 2, 10)])
def test_split_flood_tissue(markers, connectivity, min_size):
    m = tissue_mask()
    kw = dict(markers='h_maxima', h=1.5) if markers == 'h_maxima' else {}
    radius = None if markers == 'h_maxima' else 3
    lab, n = nuclei.split_touching(gpu(m), radius, connectivity, min_size, growth='flood', **kw)
    want, wn = ref.split_touching_flood(m, radius, connectivity, min_size, **kw)
    assert lab.dtype == torch.int32 and n == wn and n > 20
    assert np.array_equal(lab.cpu().numpy(), want)
    if min_size == 0:
        assert np.array_equal(want > 0, m)                               # no foreground pixel is lost
    again, n2 = nuclei.split_touching(gpu(m), radius, connectivity, min_size, growth='flood', **kw)
    assert n2 == n and torch.equal(again, lab)


def test_other_growths_are_unchanged():
    m = tissue_mask()
    t = gpu(m)
    lab, n = nuclei.split_touching(t, 3, growth='geodesic')
    want, wn = geodesic_ref.split_touching_geodesic(m, 3)
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)
    for kw in ({}, {'growth': 'euclidean'}):
        lab, n = nuclei.split_touching(t, 3, **kw)
        want, wn = edt_ref.split_touching(m, 3)
        assert n == wn and np.array_equal(lab.cpu().numpy(), want)
    lab, n = nuclei.split_touching(t, None, growth='geodesic', markers='h_maxima', h=1.5)
    want, wn = reconstruct_ref.split_touching_h_maxima(m, 1.5)
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)


def test_two_calls_give_identical_tensors():
    height, markers, within = form_case()
    h, m, w = gpu(height.astype(np.int32)), gpu(markers), gpu(within)
    first = nuclei.watershed(h, m, w, return_level=True)
    second = nuclei.watershed(h, m, w, return_level=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    table = kernels.get()
    a = table.watershed_flood(h, m, w, 5, 7, 1)
    b = table.watershed_flood(h, m, w, 5, 7, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
