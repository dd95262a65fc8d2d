"""CPU: the host side of the rank filters (csrc/rank.hip; cgc_net_amd.nuclei.rank_q10k, rank_filter, median, quantile_range,
local_entropy; kernels.HipKernels.rank_filter): what the public functions refuse before any launch, and what the library refuses
without launching.

As in tests/test_morph_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

import rank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rank_filter', 'median', 'quantile_range', 'local_entropy')
SYMBOLS = ('cgc_rank_max_radius', 'cgc_rank_entropy_max_radius', 'cgc_rank_tile_rows', 'cgc_rank_tile_cols', 'cgc_rank_entropy_term',
           'cgc_rank_filter')


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


def image(*shape, dtype=torch.uint8):
    return torch.ones(shape or (4, 5), dtype=dtype)


def calls():
    """Every public function as f(image, radius=..., footprint=..., within=...) with valid quantiles."""
    return [('rank_filter', lambda im, radius=2, **kw: nuclei.rank_filter(im, radius, 0.5, **kw)),
            ('median', lambda im, radius=2, **kw: nuclei.median(im, radius, **kw)),
            ('quantile_range', lambda im, radius=2, **kw: nuclei.quantile_range(im, radius, 0.25, 0.75, **kw)),
            ('local_entropy', lambda im, radius=2, **kw: nuclei.local_entropy(im, radius, **kw))]


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for name, fn in calls():
        for bad in (image(), image(dtype=torch.bool), np.ones((4, 5), np.uint8), None, [[1, 2]]):
            with pytest.raises(TypeError):
                fn(bad)


def test_form_of_the_image(no_launch):
    for name, fn in calls():
        for dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float16):     # int32 is out of scope
            with pytest.raises(TypeError):
                fn(image(dtype=dtype))
        for shape in ((3, 4, 5), (5,), (1, 4, 5)):
            with pytest.raises(ValueError):
                fn(image(*shape))
            with pytest.raises(ValueError):
                fn(image(*shape, dtype=torch.bool))


def test_form_of_within(no_launch):
    for name, fn in calls():
        for other in (image(5, 4), image(4, 6), image(4, 5, 1), image(20)):
            with pytest.raises(ValueError):
                fn(image(), within=other)
        with pytest.raises(ValueError, match='device'):
            fn(image(), within=torch.zeros(4, 5, dtype=torch.uint8, device='meta'))
        for bad in (image(dtype=torch.float32), np.ones((4, 5), bool), 1):
            with pytest.raises(TypeError):
                fn(image(), within=bad)


def test_radius_and_footprint(no_launch):
    assert kernels.RANK_MAX_RADIUS == nuclei.RANK_MAX_RADIUS == ref.MAX_RADIUS == 63
    assert kernels.ENTROPY_MAX_RADIUS == nuclei.ENTROPY_MAX_RADIUS == ref.ENTROPY_MAX_RADIUS == 15
    for name, fn in calls():
        top = 15 if name == 'local_entropy' else 63
        for bad in (-1, top + 1, 1000, 2.0, 2.5, None, '3', True, float('nan')):
            with pytest.raises(ValueError, match='radius'):
                fn(image(), radius=bad)
        for bad in ('circle', 'Disk', '', None, 1, ('disk',), b'disk', ref.footprint('disk', 1)):
            with pytest.raises(ValueError, match='footprint'):
                fn(image(), footprint=bad)
    with pytest.raises(ValueError, match='radius'):
        nuclei.local_entropy(image(), 16)


def test_quantiles(no_launch):
    for bad in (-0.001, 1.0001, 2, -1, float('nan'), float('inf'), True, False, None, '0.5', 1 + 0j, Fraction(10001, 10000), [0.5]):
        with pytest.raises(ValueError, match='q'):
            nuclei.rank_filter(image(), 2, bad)
        with pytest.raises(ValueError, match='q'):
            nuclei.quantile_range(image(), 2, bad, 1)
        with pytest.raises(ValueError, match='q'):
            nuclei.quantile_range(image(), 2, 0, bad)
        with pytest.raises(ValueError, match='q'):
            nuclei.rank_q10k(bad)
    for lo, hi in ((0.5, 0.25), (1, 0), (Fraction(1, 2), 0.4999), (0.00016, 0.00014)):
        with pytest.raises(ValueError, match='q_lo <= q_hi'):
            nuclei.quantile_range(image(), 2, lo, hi)


def test_rank_q10k():
    q = nuclei.rank_q10k
    assert q(0) == 0 and q(1) == 10000 and q(0.5) == 5000 and q(0.05) == 500 and q(0.95) == 9500 and q(0.25) == 2500
    assert q(0.0) == 0 and q(1.0) == 10000 and q(Fraction(1, 2)) == 5000
    assert q(Fraction(1, 3)) == 3333 and q(Fraction(2, 3)) == 6667
    # halves round up, decided exactly
    assert q(Fraction(1, 20000)) == 1 and q(Fraction(3, 20000)) == 2 and q(Fraction(19999, 20000)) == 10000
    assert q(Fraction(9999, 200000000)) == 0 and q(Fraction(10001, 200000000)) == 1
    assert q(0.00005) == math_floor_half(0.00005) and q(0.00015) == math_floor_half(0.00015)
    assert q(np.float32(0.5)) == 5000 and q(np.float64(0.25)) == 2500
    for k in range(0, 10001, 7):
        assert q(Fraction(k, 10000)) == k and q(k / 10000) == k
    assert all(isinstance(q(v), int) for v in (0, 1, 0.3, Fraction(1, 7)))


def math_floor_half(x):
    """floor(10000 x + 1/2) of the float's exact value."""
    return (Fraction(x) * 10000 + Fraction(1, 2)).__floor__()


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.rank_filter
    for bad in (-1, kernels.RANK_MAX_RADIUS + 1, None, 2.0, True):
        with pytest.raises(ValueError, match='radius'):
            call(None, Untouchable(), 'disk', bad, 'quantile', 0, 5000)
    for bad in (16, 63):
        with pytest.raises(ValueError, match='radius'):
            call(None, Untouchable(), 'disk', bad, 'entropy')
    for bad in ('circle', 0, 1, None, 3):
        with pytest.raises(ValueError, match='kind'):
            call(None, Untouchable(), bad, 2, 'quantile', 0, 5000)
    for bad in ('median', 0, None, 'QUANTILE'):
        with pytest.raises(ValueError, match='op'):
            call(None, Untouchable(), 'disk', 2, bad, 0, 5000)
    for bad in (-1, 10001, 0.5, None, True, '5000'):
        with pytest.raises(ValueError, match='q_hi'):
            call(None, Untouchable(), 'disk', 2, 'quantile', 0, bad)
        with pytest.raises(ValueError, match='q_lo'):
            call(None, Untouchable(), 'disk', 2, 'range', bad, 10000)
    with pytest.raises(ValueError, match='q_lo <= q_hi'):
        call(None, Untouchable(), 'disk', 2, 'range', 5001, 5000)


def test_signatures_and_documents():
    sig = {'rank_filter': (['image', 'radius', 'q', 'footprint', 'within'], ['disk', None]),
           'median': (['image', 'radius', 'footprint', 'within'], ['disk', None]),
           'quantile_range': (['image', 'radius', 'q_lo', 'q_hi', 'footprint', 'within'], ['disk', None]),
           'local_entropy': (['image', 'radius', 'footprint', 'within', 'raw'], [3, 'disk', None, False])}
    for name in NAMES:
        p = inspect.signature(getattr(nuclei, name)).parameters
        names, defaults = sig[name]
        assert list(p) == names, name
        assert [p[k].default for k in names[len(names) - len(defaults):]] == defaults, name
        assert 'Host syncs: none.' in getattr(nuclei, name).__doc__
    assert 'majority' in nuclei.median.__doc__ and 'tie gives True' in nuclei.median.__doc__
    params = ['self', 'image', 'kind', 'radius', 'op', 'q_lo', 'q_hi', 'within']
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.rank_filter).parameters) == params
    doc = kernels.KernelSpec.rank_filter.__doc__
    for k in range(1, 10):
        assert '\n        %d.  ' % k in doc, k
    for text in ('F16', 'CLIPPED', 'min(n - 1,', 'q10k', '[20, 20]', '[10, 10]', 'E >= 0', '(m + 1) / 2', '2^-15', 'H * W = 0',
                 'no host read', 'CGC_EINVAL', 'NO workspace', 'rank_tile_cols'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().rank_filter(None, 'disk', 1, 'quantile')
    assert kernels.RANK_OPS == {'quantile': 0, 'range': 1, 'entropy': 2}
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'local_entropy' in text and 'median' in text and 'quantile_range' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Rank filters (csrc/rank.hip)' in design and 'rank_bench.json' in design
    assert 'rank.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'rank_bench.json'))
    assert os.path.exists(os.path.join(ROOT, 'tools', 'rank_bench.py'))
    for text in ('median(separate_stains(', 'fill_holes(median(', 'local_entropy('):
        assert text in nuclei.__doc__, text


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    out = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(out)
    top = lib.cgc_rank_max_radius()

    # cgc_rank_filter(img, within, within_bytes, H, W, kind, radius, op, q_lo, q_hi, out, stream)
    def rank(img=some, within=None, wbytes=0, H=4, W=5, kind=1, radius=2, op=0, q_lo=0, q_hi=5000, out=some):
        return lib.cgc_rank_filter(img, within, wbytes, H, W, kind, radius, op, q_lo, q_hi, out, None)

    for H, W in ((-1, 5), (4, -1), (-4, -5), (2 ** 16, 2 ** 15), (2 ** 31 - 1, 2), (46341, 46341)):
        assert rank(H=H, W=W) == einval
    for op in (0, 1):
        for radius in (-1, top + 1, 255, 2 ** 20, -2 ** 31):
            assert rank(radius=radius, op=op) == einval
    for radius in (-1, 16, 17, 63, 64):
        assert rank(radius=radius, op=2) == einval
    for kind in (-1, 3, 100):
        assert rank(kind=kind) == einval
    for op in (-1, 3, 100):
        assert rank(op=op) == einval
    for op in (0, 1, 2):
        for q in (-1, 10001, 2 ** 20, -2 ** 31):
            assert rank(op=op, q_lo=0 if q > 0 else q, q_hi=q if q > 0 else 5000) == einval
            assert rank(op=op, q_lo=q, q_hi=q) == einval
        assert rank(op=op, q_lo=5001, q_hi=5000) == einval and rank(op=op, q_lo=10000, q_hi=0) == einval
    for wbytes in (0, 3, 5, 16, -1):
        assert rank(within=some, wbytes=wbytes) == einval
    assert rank(img=None) == einval and rank(out=None) == einval
    for H, W in ((0, 7), (7, 0), (0, 0)):                               # an empty image: nothing to do
        for op in (0, 1, 2):
            assert rank(H=H, W=W, op=op) == 0 and rank(H=H, W=W, op=op, img=None, out=None) == 0
        assert rank(H=H, W=W, radius=top + 1) == einval                 # ... but still a refusal
        assert rank(H=H, W=W, kind=3) == einval and rank(H=H, W=W, op=3) == einval and rank(H=H, W=W, q_hi=10001) == einval
        assert rank(H=H, W=W, op=2, radius=16) == einval and rank(H=H, W=W, q_lo=2, q_hi=1) == einval


def test_tile_geometry_and_constants(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'rank.hip')).read()
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()

    def constant(name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1))

    top = lib.cgc_rank_max_radius()
    assert top == constant('RANK_MAX_RADIUS') == kernels.RANK_MAX_RADIUS == ref.MAX_RADIUS == 63
    assert lib.cgc_rank_entropy_max_radius() == constant('RANK_ENTROPY_MAX_RADIUS') == kernels.ENTROPY_MAX_RADIUS == 15
    assert lib.cgc_rank_tile_rows() == constant('RANK_ROWS') >= 1
    span = constant('RANK_SPAN')
    for r in range(0, top + 1):
        assert lib.cgc_rank_tile_cols(r) == span - 2 * ((r + 3) // 4 * 4) >= 128
    assert lib.cgc_rank_tile_cols(-1) == 0 == lib.cgc_rank_tile_cols(top + 1)
    for name, code in (('QUANTILE', 0), ('RANGE', 1), ('ENTROPY', 2)):
        assert re.search(r'^#define CGC_RANK_%s %d$' % (name, code), header, flags=re.M), name
    assert kernels.RANK_OPS == {'quantile': 0, 'range': 1, 'entropy': 2}
    assert lib.cgc_rank_entropy_term(0) == 0 == lib.cgc_rank_entropy_term(1) and lib.cgc_rank_entropy_term(2) == 2 * 65536
    assert lib.cgc_rank_entropy_term(961) == ref.TERMS[961] and lib.cgc_rank_entropy_term(962) == -1 == lib.cgc_rank_entropy_term(-1)


def test_abi_22_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 22
    assert re.search(r'^ \*  22: rank filters', header, flags=re.M)
    assert '/* ---- F16 (' in header
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _abi.PROTOTYPES['cgc_rank_filter'] == [P, P, I, I, I, I, I, I, I, I, P, P]
    assert _abi.PROTOTYPES['cgc_rank_tile_cols'] == [I] and _abi.PROTOTYPES['cgc_rank_entropy_term'] == [I]
