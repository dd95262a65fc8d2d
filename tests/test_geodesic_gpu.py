"""Geodesic distance transform on the GPU (csrc/geodesic.hip through cgc_net_amd.nuclei.geodesic_distance_transform /
expand_labels(geodesic=True) / split_touching(growth='geodesic')) against tests/geodesic_ref.py (a heap Dijkstra over (cost, seed
index); pinned to a brute force by tests/test_geodesic_ref_cpu.py).  Every comparison is exact, on dist and on nearest.

The kernel relaxes 64 x 64 tiles with a one-pixel halo, 16 pixels per thread, in rounds that are launches: the shapes sit under, on
and one over one and two tiles in both directions, the staircases cross a tile corner diagonally, and the serpentine needs more than a
hundred rounds."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import edt_ref
import geodesic_ref as ref
from image_cases import DEV, DTYPES, gpu, tissue, two_discs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (41, 1), (7, 5), (63, 9), (64, 64), (65, 63), (64, 65), (5, 129), (129, 5), (130, 131), (200, 70)]
METRICS = [(5, 7), (1, 0), (1, 1), (3, 4)]


def run(seeds, within=None, **kw):
    s = seeds if torch.is_tensor(seeds) else gpu(seeds)
    w = within if within is None or torch.is_tensor(within) else gpu(within)
    dist, near = nuclei.geodesic_distance_transform(s, w, return_nearest=True, **kw)
    for o in (dist, near):
        assert o.dtype == torch.int32 and o.device == s.device and tuple(o.shape) == tuple(s.shape) and o.is_contiguous()
    return dist.cpu().numpy(), near.cpu().numpy()


def check(seeds, within, metric, connectivity, want=None):
    wd, wn = ref.geodesic(seeds, within, metric, connectivity) if want is None else want
    dist, near = run(seeds, within, metric=metric, connectivity=connectivity)
    assert np.array_equal(dist, wd), (metric, connectivity, np.argwhere(dist != wd)[:5])
    assert np.array_equal(near, wn), (metric, connectivity, np.argwhere(near != wn)[:5])
    return wd, wn


# ------------------------------------------------------------------ tile geometry
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_domains(shape):
    H, W = shape
    rng = np.random.RandomState(17 * H + W)
    k = 0
    for metric in METRICS:
        for connectivity in (1, 2):
            within = rng.rand(H, W) < (0.6, 0.7, 0.85, 1.0)[k % 4]
            seeds = rng.rand(H, W) < (0.002, 0.01, 0.05)[k % 3]
            if not seeds.any():
                seeds[rng.randint(H), rng.randint(W)] = True
            check(seeds, within, metric, connectivity)
            k += 1
    within = rng.rand(H, W) < 0.8
    for metric, connectivity in (((5, 7), 1), ((1, 0), 2)):
        wd, wn = check(np.zeros(shape, bool), within, metric, connectivity)                  # no seed: nothing is reached
        assert (wd == nuclei.GEO_INF).all() and (wn == -1).all()
        wd, wn = check(np.ones(shape, np.uint8), within, metric, connectivity)               # every pixel a seed (and so in the domain)
        assert (wd == 0).all() and np.array_equal(wn.ravel(), np.arange(H * W))


# ------------------------------------------------------------------ across tile corners
def staircase(anti):
    """A one-pixel-wide staircase (steps right / left, then down) that crosses the corner where four tiles meet -- (63, 63) -> (64, 64),
    or (63, 64) -> (64, 63) with ``anti`` -- as a pure corner contact; returns (domain, its pixels in path order)."""
    dom = np.zeros((130, 130), bool)
    path = []
    for i in range(55, 64):
        path += [(i, i - 1), (i, i)]
    for i in range(64, 75):
        path += [(i, i), (i, i + 1)]
    if anti:
        path = [(y, 127 - x) for y, x in path]
    for y, x in path:
        dom[y, x] = True
    return dom, path


@pytest.mark.parametrize('anti', [False, True], ids=['main', 'anti'])
def test_staircase_across_a_tile_corner(anti):
    dom, path = staircase(anti)
    assert path[17] == ((63, 64) if anti else (63, 63)) and path[18] == ((64, 63) if anti else (64, 64))
    for end in (0, -1):
        seeds = np.zeros_like(dom)
        seeds[path[end]] = True
        order = path if end == 0 else path[::-1]
        cut = 18 if end == 0 else len(path) - 18
        for metric in ((5, 7), (1, 1)):
            dist, near = check(seeds, dom, metric, 2)
            assert np.array_equal(dist != nuclei.GEO_INF, dom)                               # reached to the end
            dist, near = check(seeds, dom, metric, 1)
            reached = np.zeros_like(dom)
            for y, x in order[:cut]:
                reached[y, x] = True
            assert np.array_equal(dist != nuclei.GEO_INF, reached)                           # stops at the pure corner contact
        dist, _ = check(seeds, dom, (1, 0), 2)
        assert (dist != nuclei.GEO_INF).sum() == cut


# ------------------------------------------------------------------ many rounds
def test_serpentine_needs_many_rounds():
    within = np.ones((200, 200), bool)
    for i, r in enumerate(range(3, 200, 4)):
        within[r, :] = False
        within[r, 199 if i % 2 == 0 else 0] = True
    seeds = np.zeros_like(within)
    seeds[0, 0] = True
    wd, wn = ref.geodesic(seeds, within)
    assert wd[within].max() == 50148 and (wd[within] != ref.GEO_INF).all()
    s, w = gpu(seeds), gpu(within)
    first = nuclei.geodesic_distance_transform(s, w, return_nearest=True)
    rounds = kernels.get().geodesic_rounds
    second = nuclei.geodesic_distance_transform(s, w, return_nearest=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert np.array_equal(first[0].cpu().numpy(), wd) and np.array_equal(first[1].cpu().numpy(), wn)
    assert (first[1].cpu().numpy()[within] == 0).all()
    assert rounds > 100                     # three tile edges per corridor, fifty corridors


# ------------------------------------------------------------------ bound
@functools.lru_cache(maxsize=None)
def bound_case():
    rng = np.random.RandomState(23)
    seeds, within = rng.rand(140, 150) < 0.004, rng.rand(140, 150) < 0.8
    return seeds, within, ref.geodesic(seeds, within)


@pytest.mark.parametrize('max_distance,dmax', [(0, 0), (1, 5), (1.5, 7), (3, 15), (10, 50)])
def test_max_distance(max_distance, dmax):
    seeds, within, (wd, wn) = bound_case()
    assert nuclei._geodesic_bound(max_distance, 5, 'max_distance') == dmax
    keep = wd <= dmax
    dist, near = run(seeds, within, max_distance=max_distance)
    assert kernels.get().geodesic_rounds == kernels.GEO_FIRST_BATCH                          # one host read
    assert np.array_equal(dist, np.where(keep, wd, nuclei.GEO_INF)) and np.array_equal(near, np.where(keep, wn, -1))
    od, on = ref.geodesic(seeds, within, max_distance=max_distance)                          # the oracle's own conversion agrees
    assert np.array_equal(dist, od) and np.array_equal(near, on)


# ------------------------------------------------------------------ invariant
@pytest.mark.parametrize('connectivity', [1, 2])
def test_reached_pixels_are_the_seeded_components(connectivity):
    rng = np.random.RandomState(5 + connectivity)
    seeds, within = rng.rand(150, 170) < 0.003, rng.rand(150, 170) < 0.6
    s, w = gpu(seeds), gpu(within)
    lab, _ = nuclei.label_instances(s | w, connectivity)
    hit = torch.unique(lab[s])
    for metric in ((5, 7), (1, 0)):
        dist = nuclei.geodesic_distance_transform(s, w, metric=metric, connectivity=connectivity)
        if metric[1] == 0 and connectivity == 2:                                             # no diagonal steps: connectivity-1 components
            lab1, _ = nuclei.label_instances(s | w, 1)
            want = torch.isin(lab1, torch.unique(lab1[s]))
        else:
            want = torch.isin(lab, hit)
        assert torch.equal(dist != nuclei.GEO_INF, want)
        assert 0 < int(want.sum()) < int((s | w).sum())                                      # some components hold no seed


# ------------------------------------------------------------------ input forms
@functools.lru_cache(maxsize=None)
def form_case():
    rng = np.random.RandomState(11)
    seeds = (rng.rand(70, 133) < 0.01) * rng.randint(-3, 4, size=(70, 133))
    within = (rng.rand(70, 133) < 0.75) * rng.randint(-3, 4, size=(70, 133))
    return seeds, within, ref.geodesic(seeds, within)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_dtypes(dtype):
    seeds, within, (wd, wn) = form_case()
    conv = lambda a, dt: gpu(a != 0).to(dt) if dt in (torch.bool, torch.uint8) else gpu(a).to(dt)
    for sdt, wdt in ((dtype, torch.bool), (torch.int32, dtype), (dtype, dtype)):
        dist, near = run(conv(seeds, sdt), conv(within, wdt))
        assert np.array_equal(dist, wd) and np.array_equal(near, wn)


def test_views_none_and_no_nearest():
    seeds, within, (wd, wn) = form_case()
    st, wt = gpu(seeds.astype(np.int32)).t(), gpu(within.astype(np.int16)).t()
    assert not st.is_contiguous()
    td, tn = ref.geodesic(seeds.T, within.T)
    dist, near = run(st, wt)
    assert np.array_equal(dist, td) and np.array_equal(near, tn)
    wide_s = gpu(np.repeat(seeds.astype(np.int16), 2, axis=1))[:, ::2]
    wide_w = gpu(np.repeat(within.astype(np.int64), 3, axis=0))[::3]
    dist, near = run(wide_s, wide_w)
    assert np.array_equal(dist, wd) and np.array_equal(near, wn)
    only = nuclei.geodesic_distance_transform(gpu(seeds), gpu(within))
    assert torch.is_tensor(only) and np.array_equal(only.cpu().numpy(), wd)
    for metric in ('chamfer', 'cityblock', 'chessboard'):
        fd, fn = ref.geodesic(seeds, None, metric)
        dist, near = run(seeds, None, metric=metric)                                         # within=None: every pixel
        assert np.array_equal(dist, fd) and np.array_equal(near, fn)
        dist, near = run(seeds, np.ones(seeds.shape, bool), metric=nuclei.GEODESIC_STEPS[metric])
        assert np.array_equal(dist, fd) and np.array_equal(near, fn)
    assert nuclei.GEODESIC_STEPS == {'cityblock': (1, 0), 'chessboard': (1, 1), 'chamfer': (5, 7)} and nuclei.GEO_INF == 2 ** 31 - 1


def test_empty_images():
    for shape in ((0, 5), (4, 0), (0, 0)):
        t = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        dist, near = nuclei.geodesic_distance_transform(t, t, return_nearest=True)
        assert tuple(dist.shape) == shape and tuple(near.shape) == shape and dist.dtype == near.dtype == torch.int32
        out = nuclei.expand_labels(t, None, geodesic=True)
        assert tuple(out.shape) == shape and out.dtype == torch.uint8
        lab, n = nuclei.split_touching(t, 2, growth='geodesic')
        assert tuple(lab.shape) == shape and lab.dtype == torch.int32 and n == 0


# ------------------------------------------------------------------ expand_labels(geodesic=True)
@pytest.mark.parametrize('distance', [1, 2.5, 6, None])
def test_expand_labels_geodesic_tissue(distance):
    labels, _, within = tissue()
    t = gpu(labels)
    out = nuclei.expand_labels(t, distance, within=gpu(within), geodesic=True)
    if distance is not None:
        assert kernels.get().geodesic_rounds == kernels.GEO_FIRST_BATCH                      # a few pixels: one host read
    assert out.dtype == t.dtype and out.device == t.device and tuple(out.shape) == labels.shape
    got = out.cpu().numpy()
    want = ref.expand_labels_geodesic(labels, distance, within)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(got[labels != 0], labels[labels != 0])                             # labelled pixels never change
    assert (got[(labels == 0) & ~within] == 0).all()
    assert np.array_equal(t.cpu().numpy(), labels)                                           # the input is left alone
    small = nuclei.expand_labels(gpu(labels.astype(np.int16)), distance, within=gpu(within), geodesic=True, connectivity=2)
    assert small.dtype == torch.int16
    assert np.array_equal(small.cpu().numpy(), ref.expand_labels_geodesic(labels, distance, within, connectivity=2))


def test_expand_labels_through_the_opening_of_a_wall():
    lab = np.zeros((70, 40), np.uint8)
    lab[:, :2], lab[:, 38:] = 9, 4
    within = np.ones(lab.shape, bool)
    within[:, 6] = False                     # a wall next to label 9 ...
    within[69, 6] = True                     # ... open at the bottom row only
    got = nuclei.expand_labels(gpu(lab), 40, within=gpu(within), geodesic=True).cpu().numpy()
    assert np.array_equal(got, ref.expand_labels_geodesic(lab, 40, within))
    assert (got[:, 2:6] == 9).all() and (got[:69, 6] == 0).all() and got[69, 6] == 9
    assert (got[0, 7:38] == 4).all()         # behind the wall, far from the opening: label 4, although label 9 is 5 pixels away
    assert (got[69, 7:20] == 9).all()        # behind the wall at the opening: label 9 arrives through it
    eu = nuclei.expand_labels(gpu(lab), 40, within=gpu(within)).cpu().numpy()
    assert np.array_equal(eu, edt_ref.expand_labels(lab, 40, within))
    assert (eu[0, 7:20] == 9).all() and not np.array_equal(eu, got)                          # Euclidean nearness crosses the wall


# ------------------------------------------------------------------ split_touching(growth='geodesic')
@pytest.mark.parametrize('core_radius,connectivity,min_size', [(2, 1, 0), (3, 1, 0), (4, 1, 10), (2.5, 2, 10)])
def test_split_geodesic_tissue(core_radius, connectivity, min_size):
    labels, _, _ = tissue()
    m = labels > 0
    lab, n = nuclei.split_touching(gpu(m), core_radius, connectivity, min_size, growth='geodesic')
    want, wn = ref.split_touching_geodesic(m, core_radius, connectivity, min_size)
    got = lab.cpu().numpy()
    assert type(n) is int and lab.dtype == torch.int32
    assert n == wn and np.array_equal(got, want), (n, wn, np.argwhere(got != want)[:5])
    if min_size == 0:
        assert np.array_equal(got != 0, m)                                                   # every mask pixel is labelled
    assert n <= nuclei.split_touching(gpu(m), core_radius, connectivity, min_size)[1]


def test_split_geodesic_shapes():
    yy, xx = np.mgrid[0:40, 0:60]
    ellipse = ((yy - 20) / 4.2) ** 2 + ((xx - 30) / 22.0) ** 2 <= 1.0
    lab, n = nuclei.split_touching(gpu(ellipse), 3, growth='geodesic')
    assert n == 1 and np.array_equal(lab.cpu().numpy() != 0, ellipse)
    assert nuclei.split_touching(gpu(ellipse), 3)[1] == 3                                    # the tips are out of the Euclidean reach
    m = two_discs()
    for radius, count in ((8, 2), (7, 1)):
        lab, n = nuclei.split_touching(gpu(m), radius, growth='geodesic')
        want, wn = ref.split_touching_geodesic(m, radius)
        assert n == wn == count and np.array_equal(lab.cpu().numpy(), want) and np.array_equal(want != 0, m)
    labels, gray, _ = tissue()
    for connectivity, min_size in ((1, 0), (2, 10)):
        image = gpu(labels)
        lab, n = nuclei.split_touching(image, 0, connectivity, min_size, growth='geodesic')
        want, wn = nuclei.label_instances(image != 0, connectivity, min_size)
        assert n == wn and torch.equal(lab, want)


def test_split_geodesic_feeds_nucleus_features():
    labels, gray, _ = tissue()
    lab, n = nuclei.split_touching(gpu(labels > 0), 3, min_size=10, growth='geodesic')
    feats, cen, kept = nuclei.nucleus_features(lab, gpu(gray), max_label=n)
    assert tuple(feats.shape) == (n, nuclei.NUM_FEATURES) and tuple(cen.shape) == (n, 2)
    assert np.array_equal(kept.cpu().numpy(), np.arange(1, n + 1))


# ------------------------------------------------------------------ defaults untouched
def test_defaults_are_untouched():
    labels, _, within = tissue()
    out = nuclei.expand_labels(gpu(labels), 2.5, within=gpu(within))
    assert np.array_equal(out.cpu().numpy(), edt_ref.expand_labels(labels, 2.5, within=within))
    m = labels > 0
    lab, n = nuclei.split_touching(gpu(m), 4)
    want, wn = edt_ref.split_touching(m, 4)
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)
    lab, n = nuclei.split_touching(gpu(m), 4, growth='euclidean')
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    ok = torch.zeros(8, 9, dtype=torch.uint8, device=DEV)
    geo = nuclei.geodesic_distance_transform
    for bad in ('euclid', (0, 0), (2, 1), (2, 5), (1, -1), (1.5, 2), (5,), 5, None):
        with pytest.raises(ValueError):
            geo(ok, metric=bad)
        with pytest.raises(ValueError):
            nuclei.expand_labels(ok, 1, geodesic=True, metric=bad)
    with pytest.raises(ValueError):
        nuclei.split_touching(ok, 1, growth='watershed')
    for fn in (lambda **kw: geo(ok, **kw), lambda **kw: nuclei.expand_labels(ok, 1, geodesic=True, **kw),
               lambda **kw: nuclei.split_touching(ok, 1, growth='geodesic', **kw)):
        with pytest.raises(ValueError):
            fn(connectivity=3)
    with pytest.raises(ValueError):
        nuclei.expand_labels(ok, None)
    with pytest.raises(ValueError):
        nuclei.expand_labels(ok, None, within=ok)
    for bad in (-1, -0.5, float('nan')):
        with pytest.raises(ValueError):
            geo(ok, max_distance=bad)
        with pytest.raises(ValueError):
            nuclei.expand_labels(ok, bad, geodesic=True)
    for fn in (lambda w: geo(ok, w), lambda w: nuclei.expand_labels(ok, 1, within=w, geodesic=True)):
        with pytest.raises(ValueError):
            fn(torch.zeros(9, 8, dtype=torch.bool, device=DEV))
        with pytest.raises(TypeError):
            fn(torch.zeros(8, 9, dtype=torch.bool))                                          # a host tensor
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError):
                fn(torch.zeros(8, 9, dtype=torch.bool, device='cuda:1'))                     # another device
        with pytest.raises(TypeError):
            fn(torch.zeros(8, 9, dtype=torch.float32, device=DEV))
        with pytest.raises(TypeError):
            fn(np.zeros((8, 9), np.uint8))
    for fn in (lambda t: geo(t), lambda t: nuclei.expand_labels(t, 1, geodesic=True)):
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 8, 9, dtype=torch.uint8, device=DEV))
        with pytest.raises(TypeError):
            fn(torch.zeros(8, 9, dtype=torch.float32, device=DEV))
        with pytest.raises(TypeError):
            fn(torch.zeros(8, 9, dtype=torch.uint8))
        with pytest.raises(TypeError):
            fn(np.zeros((8, 9), np.uint8))


def test_library_refuses_overflowing_sizes():
    lib = kernels.get().lib
    assert lib.cgc_geodesic_ws_bytes(300, 300) > 0 and lib.cgc_geodesic_ws_bytes(0, 7) == 0
    assert lib.cgc_geodesic_ws_bytes(65536, 32768) == 0 and lib.cgc_geodesic_ws_bytes(-1, 4) == 0        # H * W = 2^31
    einval = -1                                                                              # CGC_EINVAL before anything is touched
    assert lib.cgc_geodesic_begin(None, 1, None, 0, 20000, 20000, 5, 7, None, None) == einval            # 7 * 4e8 >= 2^31
    assert lib.cgc_geodesic_begin(None, 1, None, 0, 40000, 40000, 1, 0, None, None) == einval            # 1 * 1.6e9 < 2^31: NULL pointers
    assert lib.cgc_geodesic_begin(None, 1, None, 0, 50000, 50000, 1, 0, None, None) == einval            # 2.5e9 >= 2^31
    assert lib.cgc_geodesic_begin(None, 1, None, 0, 4, 4, 2, 5, None, None) == einval                    # b > 2a
    assert lib.cgc_geodesic_begin(None, 3, None, 0, 4, 4, 5, 7, None, None) == einval
    assert lib.cgc_geodesic_rounds(20000, 20000, 5, 7, 1, -1, None, 0, 4, None, None) == einval
    assert lib.cgc_geodesic_rounds(4, 4, 5, 7, 3, -1, None, 0, 4, None, None) == einval
    assert lib.cgc_geodesic_finish(65536, 32768, None, None, None, None) == einval
    with pytest.raises(ValueError):
        nuclei.geodesic_distance_transform(torch.zeros(1, 1, dtype=torch.bool, device=DEV).expand(20000, 20000))
