"""CPU: the host side of region adjacency and Voronoi graphs (csrc/adjacency.hip; cgc_net_amd.nuclei.region_adjacency, voronoi_graph,
graph_item, kernels.HipKernels.region_adjacency): what the public functions refuse before any launch, and what the library refuses
without launching.

As in tests/test_normalize_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


@pytest.fixture
def no_launch(monkeypatch):
    """Host tensors pass the image check; asking for the kernel table fails the test."""
    check = nuclei._check_image

    def lifted(fn, name, image, dtypes=None, on_gpu=True):
        return check(fn, name, image, on_gpu=False) if dtypes is None else check(fn, name, image, dtypes, on_gpu=False)

    def refuse():
        pytest.fail('a launch was reached')

    monkeypatch.setattr(nuclei, '_check_image', lifted)
    monkeypatch.setattr(kernels, 'get', refuse)


def image(*shape, dtype=torch.int32):
    return torch.ones(shape or (4, 5), dtype=dtype)


def public_calls():
    return (lambda labels, **kw: nuclei.region_adjacency(labels, **kw),
            lambda labels, **kw: nuclei.voronoi_graph(labels, 5.0, **kw))


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for fn in public_calls():
        for bad in (image(), np.ones((4, 5), np.int32), None, [[1, 2]]):
            with pytest.raises(TypeError):
                fn(bad)


def test_form_of_the_labels(no_launch):
    for fn in public_calls():
        with pytest.raises(TypeError, match=r'\.to\(torch\.int32\)'):
            fn(image(dtype=torch.int64))
        for dtype in (torch.float32, torch.float16, torch.float64):
            with pytest.raises(TypeError):
                fn(image(dtype=dtype))
        for shape in ((3, 4, 5), (5,), (1, 4, 5)):
            with pytest.raises(ValueError):
                fn(image(*shape))
        for bad in (0, 3, 4, 8, None, '1'):
            with pytest.raises(ValueError, match='connectivity'):
                fn(image(), connectivity=bad)


def test_form_of_value(no_launch):
    for other in (image(5, 4), image(4, 6), image(4, 5, 1)):
        with pytest.raises(ValueError):
            nuclei.region_adjacency(image(), value=other)
    with pytest.raises(ValueError, match='device'):
        nuclei.region_adjacency(image(), value=torch.zeros(4, 5, dtype=torch.int32, device='meta'))
    for dtype in (torch.int64, torch.float32):                                   # as ``within`` elsewhere: a TypeError
        with pytest.raises(TypeError):
            nuclei.region_adjacency(image(), value=image(dtype=dtype))


def test_empty_images_return_empty_tensors_without_a_launch(no_launch):
    for shape in ((0, 5), (5, 0), (0, 0)):
        out = nuclei.region_adjacency(image(*shape))
        assert len(out) == 2 and out[0].shape == (0, 2) and out[1].shape == (0,) and out[0].dtype == out[1].dtype == torch.int32
        out = nuclei.region_adjacency(image(*shape, dtype=torch.uint8), connectivity=2, value=image(*shape, dtype=torch.int16))
        assert len(out) == 3 and out[2].shape == (0,) and out[2].dtype == torch.int32
        assert nuclei.voronoi_graph(image(*shape), 5.0).shape == (2, 0)
        kept = torch.tensor([2, 5], dtype=torch.int32)
        ei, border, gap = nuclei.voronoi_graph(image(*shape), 5.0, kept_labels=kept, return_attr=True)
        assert ei.tolist() == [[0, 1], [0, 1]] and ei.dtype == torch.int64       # the loops of two nodes without a pixel
        assert border.tolist() == [0, 0] and border.dtype == torch.int32 and gap.tolist() == [0.0, 0.0] and gap.dtype == torch.float32
        assert nuclei.voronoi_graph(image(*shape), 5.0, kept_labels=kept, loop=False).shape == (2, 0)


def test_voronoi_graph_refusals(no_launch):
    labels = image()
    labels[1, 2] = -1
    with pytest.raises(ValueError, match='negative'):
        nuclei.voronoi_graph(labels, 5.0)
    for bad in (-1, -1e-9, float('nan'), None, 'a'):
        with pytest.raises((ValueError, TypeError)):
            nuclei.voronoi_graph(image(), bad)
    with pytest.raises(ValueError, match='max_distance'):
        nuclei.voronoi_graph(image(), -1.0)
    for bad in (-1, -0.5, float('nan')):
        with pytest.raises(ValueError, match='max_gap'):
            nuclei.voronoi_graph(image(), 5.0, max_gap=bad)
    for bad in ([3, 2], [1, 1], [0, 1], [-1, 2], [2, 5, 4]):
        with pytest.raises(ValueError, match='ascending'):
            nuclei.voronoi_graph(image(), 5.0, kept_labels=torch.tensor(bad, dtype=torch.int32))
    for bad in (torch.tensor([1, 2]), torch.tensor([[1, 2]], dtype=torch.int32), [1, 2], np.array([1, 2], np.int32),
                torch.zeros(2, dtype=torch.int32, device='meta')):
        with pytest.raises(ValueError, match='kept_labels'):
            nuclei.voronoi_graph(image(), 5.0, kept_labels=bad)


def test_graph_item_carries_edges_on_the_host():
    f, c = torch.zeros(3, 16), torch.zeros(3, 2)
    assert nuclei.graph_item(f, c, 1).edge_index is None
    item = nuclei.graph_item(f, c, 1, edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]], dtype=torch.int32))
    assert item.edge_index.dtype == torch.int64 and item.edge_index.device.type == 'cpu' and item.edge_index.tolist() == [[0, 1, 2], [1, 2, 0]]
    assert item.x.shape == (3, 18) and item.num_edges == 3
    for bad in (torch.zeros(3, 2), torch.zeros(4)):
        with pytest.raises(ValueError):
            nuclei.graph_item(f, c, 1, edge_index=bad)


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_a_bad_connectivity_before_any_tensor():
    for bad in (0, 3, -1, None):
        with pytest.raises(ValueError, match='connectivity'):
            kernels.HipKernels.region_adjacency(None, Untouchable(), bad)


def test_signatures_and_documents():
    p = inspect.signature(nuclei.region_adjacency).parameters
    assert list(p) == ['labels', 'connectivity', 'value'] and p['connectivity'].default == 1 and p['value'].default is None
    p = inspect.signature(nuclei.voronoi_graph).parameters
    assert list(p) == ['labels', 'max_distance', 'kept_labels', 'connectivity', 'loop', 'max_gap', 'return_attr']
    assert [p[k].default for k in list(p)[2:]] == [None, 1, True, None, False]
    p = inspect.signature(nuclei.graph_item).parameters
    assert list(p) == ['features', 'centroids', 'y', 'edge_index'] and p['edge_index'].default is None
    assert 'Host syncs: two' in nuclei.region_adjacency.__doc__ and 'Host syncs:' in nuclei.voronoi_graph.__doc__
    assert 'NOT the true gap' in nuclei.voronoi_graph.__doc__ and '3/8 px' in nuclei.voronoi_graph.__doc__
    p = inspect.signature(kernels.KernelSpec.region_adjacency).parameters
    assert list(p) == ['self', 'labels', 'connectivity', 'value'] and p['value'].default is None
    assert list(inspect.signature(kernels.HipKernels.region_adjacency).parameters) == list(p)
    doc = kernels.KernelSpec.region_adjacency.__doc__
    for k in range(1, 9):
        assert '\n        %d.  ' % k in doc, k
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_adjacency(None, 1)
    assert kernels.ADJ_MAX_PIXELS == 2 ** 29
    for name in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'region_adjacency' in text and 'voronoi_graph' in text, name
    assert '## Region adjacency and Voronoi graphs (csrc/adjacency.hip)' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'adjacency.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    out = (ctypes.c_int64 * 64)()                                                 # any non-NULL address: nothing is launched
    some = ctypes.addressof(out)

    # cgc_adjacency_count(labels, H, W, connectivity, ws, n_records_out, stream)
    # cgc_adjacency_records(labels, value, H, W, connectivity, ws, n_records, keys, counts, sums, stream)
    def count(H=4, W=5, connectivity=1, labels=some, ws=some, n_out=some):
        return lib.cgc_adjacency_count(labels, H, W, connectivity, ws, n_out, None)

    def records(H=4, W=5, connectivity=1, labels=some, value=None, ws=some, n=3, keys=some, counts=some, sums=None):
        return lib.cgc_adjacency_records(labels, value, H, W, connectivity, ws, n, keys, counts, sums, None)

    for fn in (count, records):
        for connectivity in (0, 3, -1, 4, 8):
            assert fn(connectivity=connectivity) == einval
        for H, W in ((-1, 5), (4, -1), (-4, -5), (2 ** 15, 2 ** 14), (2 ** 29, 1), (1, 2 ** 29), (2 ** 20, 2 ** 20), (46341, 46341)):
            assert fn(H=H, W=W) == einval
        assert fn(labels=None) == einval and fn(ws=None) == einval
    assert count(n_out=None) == einval and count(n_out=None, H=0) == einval
    assert records(keys=None) == einval and records(counts=None) == einval
    assert records(value=some) == einval and records(sums=some) == einval         # value and sums come together
    assert records(n=-1) == einval and records(n=4 * 4 * 5 + 1) == einval         # more records than contacts
    assert records(n=0) == 0 and records(n=0, labels=None, ws=None, keys=None, counts=None) == 0

    # cgc_adjacency_heads(sorted_keys, n_records, ws, n_pairs_out, stream)
    # cgc_adjacency_merge(sorted_keys, perm, counts, sums, n_records, ws, n_pairs, pairs, count, min_sum, stream)
    def heads(keys=some, n=3, ws=some, n_out=some):
        return lib.cgc_adjacency_heads(keys, n, ws, n_out, None)

    def merge(keys=some, perm=some, counts=some, sums=None, n=3, ws=some, n_pairs=2, pairs=some, count=some, min_sum=None):
        return lib.cgc_adjacency_merge(keys, perm, counts, sums, n, ws, n_pairs, pairs, count, min_sum, None)

    for fn in (heads, merge):
        for n in (-1, 2 ** 31, 2 ** 40):
            assert fn(n=n) == einval
        assert fn(keys=None) == einval and fn(ws=None) == einval
    assert heads(n_out=None) == einval and heads(n_out=None, n=0) == einval
    assert merge(n_pairs=-1) == einval and merge(n_pairs=4) == einval            # more pairs than records
    for name in ('perm', 'counts', 'pairs', 'count'):
        assert merge(**{name: None}) == einval
    assert merge(sums=some) == einval and merge(min_sum=some) == einval
    assert merge(n_pairs=0) == 0 and merge(n_pairs=0, n=0, keys=None, perm=None, counts=None, ws=None, pairs=None, count=None) == 0


def test_workspace_sizes_and_the_tile_side(lib):
    t = lib.cgc_adjacency_tile_side()
    assert t == 64
    assert lib.cgc_adjacency_ws_bytes(0, 0) == 256 and lib.cgc_adjacency_ws_bytes(0, 7) == 256      # no tile: the scan's total alone
    assert lib.cgc_adjacency_ws_bytes(1, 1) == 512 == lib.cgc_adjacency_ws_bytes(t, t)             # one tile: offsets, dense flag
    assert lib.cgc_adjacency_ws_bytes(t + 1, t) == 512 and lib.cgc_adjacency_ws_bytes(8 * t, 8 * t + 1) == 2 * 512
    assert lib.cgc_adjacency_ws_bytes(-1, 4) == 0 and lib.cgc_adjacency_ws_bytes(2 ** 15, 2 ** 14) == 0
    assert lib.cgc_adjacency_ws_bytes(2 ** 14, 2 ** 14) > 0                                         # 2^28 pixels: admitted
    assert lib.cgc_adjacency_merge_ws_bytes(0) == 0 and lib.cgc_adjacency_merge_ws_bytes(1) == 256
    assert lib.cgc_adjacency_merge_ws_bytes(2048 * 64) == 256 and lib.cgc_adjacency_merge_ws_bytes(2048 * 64 + 1) == 512
    assert lib.cgc_adjacency_merge_ws_bytes(-1) == 0 and lib.cgc_adjacency_merge_ws_bytes(2 ** 31) == 0
    for name in ('cgc_adjacency_ws_bytes', 'cgc_adjacency_merge_ws_bytes'):
        assert getattr(lib, name).restype is ctypes.c_int64


def test_abi_18_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 18
    assert re.search(r'^ \*  18: region adjacency', header, flags=re.M)
    for name in ('cgc_adjacency_tile_side', 'cgc_adjacency_count', 'cgc_adjacency_records', 'cgc_adjacency_heads', 'cgc_adjacency_merge'):
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    for name in ('cgc_adjacency_ws_bytes', 'cgc_adjacency_merge_ws_bytes'):
        assert name in _abi.PROTOTYPES and re.search(r'^int64_t %s\(' % name, header, flags=re.M), name
