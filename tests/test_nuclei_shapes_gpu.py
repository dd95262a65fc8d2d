"""Nucleus features on the GPU (csrc/nuclei.hip) on the hand-made scenes of tests/nuclei_cases.py: degenerate contours, both sides of
the LDS limit, more large crops than workspace slots, long relaxations, the zero rules of the moments and the GLCM, the label pass and
the compaction at their wave and chunk edges, min_size at equality.  Same oracle (tests/nuclei_ref.py) and same bars as
tests/test_nuclei_gpu.py; tests/test_nuclei_ref_cpu.py shows that the scenes are what they claim and pins the oracle on them."""
import numpy as np
import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels

import nuclei_cases as cases
from nuclei_cases import _gpu, check_against_reference

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def _path(names, kept, info, shape):
    return int(info[int(np.nonzero(kept == cases.by_name(names)[shape])[0][0]), 3])


def test_shapes_match_the_restatement():
    labels, gray, min_size, names = cases.shapes()
    assert kernels.get().lib.cgc_nuclei_lds_max_pixels() == cases.LDS_PIXELS
    _, _, k, info = check_against_reference(labels, gray, min_size=min_size)
    assert k.tolist() == sorted(names) and (info[:, 2] > 0).all()
    assert [_path(names, k, info, s) for s in ('rect_lds_2048', 'rect_global_2080', 'rect_corner_2048')] == [0, 1, 0]
    assert int(info[:, 3].sum()) == 1                                       # nothing else is large


def test_shapes_min_size_0_is_min_size_1():
    labels, gray, _, _ = cases.shapes()
    assert _bits_equal(_gpu(labels, gray, min_size=0), _gpu(labels, gray, min_size=1))


def test_shapes_with_a_max_label_beyond_the_largest():
    labels, gray, min_size, _ = cases.shapes()
    assert _bits_equal(_gpu(labels, gray, min_size=min_size), _gpu(labels, gray, min_size=min_size, max_label=int(labels.max()) + 1000))


def test_many_big_reuses_its_workspace_slots():
    labels, gray, min_size, names = cases.many_big()
    first = check_against_reference(labels, gray, min_size=min_size)
    assert first[2].size == 40 > cases.BIG_SLOTS and (first[3][:, 3] == 1).all() and (first[3][:, 2] > 0).all()
    runs = [_gpu(labels, gray, min_size=min_size)]
    other = cases.shapes()
    _gpu(other[0], other[1], min_size=other[2])                             # leaves other data in the memory the next calls allocate
    runs += [_gpu(labels, gray, min_size=min_size), _gpu(labels, gray, min_size=min_size)]
    for again in runs:
        assert _bits_equal(first, again)


def test_spirals_match_the_restatement():
    labels, gray, min_size, names = cases.spirals()
    _, _, k, info = check_against_reference(labels, gray, min_size=min_size)
    assert k.tolist() == [1, 2] and (info[:, 2] > 0).all()
    assert (_path(names, k, info, 'spiral_global'), _path(names, k, info, 'spiral_lds')) == (1, 0)


def test_stripes_64_labels_per_wave():
    labels, gray, min_size, _ = cases.stripes()
    _, c, k, info = check_against_reference(labels, gray, min_size=min_size)
    assert k.tolist() == list(range(1, 68)) and (info[:, 2] > 0).all()
    assert np.array_equal(c, np.stack([np.full(67, 19.5), np.arange(67)], 1).astype(np.float32))   # exact in float32


@pytest.mark.parametrize('min_size', [10, 12])
def test_label_edges_kept_at_equality(min_size):
    labels, gray, _, _ = cases.label_edges()
    _, _, k, info = check_against_reference(labels, gray, min_size=min_size)    # the 9-pixel neighbours are background of the crops
    assert k.tolist() == list(cases.LABEL_EDGE_KEPT) and (info[:, 2] > 0).all() and (info[:, 3] == 0).all()


def test_label_edges_one_pixel_short():
    labels, gray, _, _ = cases.label_edges()
    f, c, k, info = check_against_reference(labels, gray, min_size=13)
    assert f.shape == (0, 16) and c.shape == (0, 2) and k.size == 0 and info.shape == (0, 4)
