"""The front end that window.hip, morph.hip and rank.hip share (csrc/image_window.hpp): the same pixels, presented so that the library
takes each of the loader's four forms <WITHIN, DWORDS>, must give the same window sums, gradient, median and entropy -- those of the
numpy references, bit for bit.  Each stage's own file has larger versions of these cases; this one is where a change to the shared
loader fails first.

The image is 37 x 44: W % 4 == 0, 37 rows cross a tile boundary of all three kernels (8, 16, 32 rows), and one tile spans the width,
so the halo lies outside the image on all four sides."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import morph_ref
import rank_ref
import window_ref
from image_cases import DEV, gpu

pytestmark = pytest.mark.gpu

H, W = 37, 44
NAMES = ('n', 'S', 'Q', 'gradient', 'median', 'h16')
DTYPES = (np.int32, np.int32, np.int64, np.uint8, np.uint8, np.int32)


@functools.lru_cache(maxsize=None)
def pixels():
    rng = np.random.RandomState(3744)
    a, w = rng.randint(0, 256, (H, W)).astype(np.uint8), rng.rand(H, W) < 0.6
    a.setflags(write=False)
    w.setflags(write=False)
    return a, w


@functools.lru_cache(maxsize=None)
def expected(cols, selected):
    """The references on the first ``cols`` columns, with or without the selection: computed once, write-protected."""
    a, w = (np.ascontiguousarray(p[:, :cols]) for p in pixels())
    w = w if selected else None
    cum = rank_ref.cumulative(a, 'disk', 3, w)
    exact = tuple(window_ref.window_sums(a, 2, w)) + (morph_ref.morph_gradient(a, 3, 'disk', w), rank_ref.quantile_of(cum, 5000),
                                                      rank_ref.h16_of(cum))
    out = tuple(e.astype(dtype) for e, dtype in zip(exact, DTYPES))     # the library's types hold every value
    for o, e in zip(out, exact):
        assert np.array_equal(o, e)
        o.setflags(write=False)
    return out


def run(image, within):
    n, S, Q = nuclei.window_sums(image, 2, within)
    out = (n, S, Q, nuclei.morph_gradient(image, 3, 'disk', within), nuclei.median(image, 3, 'disk', within),
           nuclei.local_entropy(image, 3, 'disk', within, raw=True))
    return tuple(o.cpu().numpy() for o in out)


def unaligned(a):
    """The array on the device, contiguous, its first element one byte past a dword boundary."""
    flat = torch.zeros(a.size + 4, dtype=torch.uint8, device=DEV)
    t = flat[1:1 + a.size].view(a.shape)
    t.copy_(gpu(np.array(a)))
    assert t.is_contiguous() and t.data_ptr() % 4 == 1
    return t


def same(got, want, note):
    for name, g, e in zip(NAMES, got, want):
        assert g.dtype == e.dtype and np.array_equal(g, e), (note, name, np.argwhere(g != e)[:5])


def test_the_four_loaders_agree_on_the_same_pixels():
    a, w = pixels()
    w8 = w.astype(np.uint8)
    aligned = gpu(np.array(a))
    assert aligned.data_ptr() % 4 == 0
    high = gpu(w8).to(torch.int32) * (1 << 24)                          # non-zero only in the high byte: the whole element is read
    with_within = {'<true, true> aligned, uint8 within': run(aligned, gpu(w8)),
                   '<true, false> unaligned base': run(unaligned(a), unaligned(w8)),
                   '<true, false> int32 within': run(aligned, high)}
    without = {'<false, true> aligned': run(aligned, None), '<false, false> unaligned base': run(unaligned(a), None)}
    for variants, selected in ((with_within, True), (without, False)):
        first = None
        for note, got in variants.items():
            same(got, expected(W, selected), note)
            first = got if first is None else first
            same(got, first, note + ' against the first variant')


def test_a_width_that_is_no_multiple_of_four():
    a, w = (np.ascontiguousarray(p[:, :W - 1]) for p in pixels())
    assert a.shape[1] % 4 != 0
    same(run(gpu(a), gpu(w.astype(np.uint8))), expected(W - 1, True), '<true, false> 37 x 43')
    same(run(gpu(a), None), expected(W - 1, False), '<false, false> 37 x 43')
