"""Instance masks, then nucleus features and centroids from them, on the GPU: the steps that make the node tables of every graph
(dataflow/construct_feature_graph.py:50-123 + common/nuc_feature.py, then dataflow/prepare_cv_dataset.py:57-72).

``label_instances(image)`` is the step in front: it turns a thresholded foreground map into an instance mask (connected-component
labelling, scipy.ndimage.label's numbering) or splits every value of an integer mask into its connected pieces (csrc/label.hip; the
contract item by item: kernels.KernelSpec.label_components).  Its ``labels`` and ``n`` go straight into
``nucleus_features(labels, gray, max_label=n)``.  The reference starts from finished masks and has no such step.

``distance_transform``, ``expand_labels`` and ``split_touching`` sit between the two: an exact Euclidean distance transform with the
nearest site of every pixel (csrc/edt.hip; kernels.KernelSpec.distance_transform), skimage's expand_labels on top of it, and the
erode-label-grow split that keeps touching nuclei from merging into one node.  ``geodesic_distance_transform`` measures distance
along paths that stay inside a mask instead (csrc/geodesic.hip; kernels.KernelSpec.geodesic_transform): ``expand_labels(...,
geodesic=True)`` grows labels along such paths, so that no label reaches across a gap, and ``split_touching(..., growth='geodesic')``
gives every mask pixel that is connected to a core the geodesically nearest core.

``reconstruct`` is grayscale morphological reconstruction (csrc/reconstruct.hip; kernels.KernelSpec.morph_reconstruct), and
``h_maxima``, ``regional_maxima`` and ``fill_holes`` stand on it: ``fill_holes`` closes the holes of a binary or an instance mask
before the features are taken, and ``split_touching(..., markers='h_maxima', h=...)`` takes as cores the maxima of the distance map
whose dynamic is at least ``h``, which finds one core per nucleus whatever its size.

``watershed`` is the marker-controlled watershed (csrc/watershed.hip; kernels.KernelSpec.watershed_flood): water rises from the
markers over a height image and every pixel takes the marker whose water wets it first.  ``split_touching(..., growth='flood')``
floods the negated distance map from the cores, which puts the cut between two touching nuclei on the neck between them, however
unequal they are.

``stain_foreground`` is the step in front of all of them, for a user who holds only the H&E tile: colour deconvolution into a
haematoxylin plane (``separate_stains``; csrc/stain.hip, kernels.KernelSpec.stain_separate), a little binomial smoothing (``smooth``;
csrc/smooth.hip) and Otsu's threshold of the plane's histogram (``histogram``, ``otsu_threshold``) -- all in integer arithmetic with a
stated contract, so that the foreground map is a pure function of the tile.  Its output goes into ``fill_holes`` and
``split_touching``.  ``estimate_stains`` (Macenko et al. 2009) takes the stain vectors from the tile itself instead of the fixed
``DEFAULT_STAINS`` -- two integer reductions on the device (kernels.KernelSpec.od_moments, angle_histogram), a 3 x 3 eigenproblem and
two exact percentiles on the host: ``stain_foreground(tile, stains=estimate_stains(tile))``.
``normalize_stains`` is the other half of Macenko's method and makes tiles of different slides comparable: it deconvolves with the
tile's own vectors, scales each stain so that its robust maximum matches a reference (``stain_maxima``; one more integer reduction,
kernels.KernelSpec.concentration_histogram) and re-composes the tile with reference vectors (``recolor_matrix``, ``recolor``;
kernels.KernelSpec.od_recolor).  With normalisation in front, the stage reads
    norm = normalize_stains(tile)
    fg, t, plane = stain_foreground(norm, stains=TARGET_STAINS + residual)
    ...
    nucleus_features(L, bgr_to_gray(norm), max_label=n)
where ``TARGET_STAINS + residual`` stands for the 3 x 3 vectors made of the two target rows plus their cross product.

``local_threshold`` is the local counterpart of ``plane > otsu_threshold(plane)``: every pixel is compared with the mean, and
optionally the spread (Niblack), of the window around it, so that a tile whose staining or density varies keeps its pale side and
does not merge its crowded side (csrc/window.hip; kernels.KernelSpec.local_threshold -- exact integers, one byte read and one
written per pixel).  ``window_sums`` is the primitive under it, for rules of one's own: count, sum and sum of squares of every
window, over the pixels of ``within`` only if wanted.  ``local_stain_foreground`` is ``stain_foreground`` with the local rule.

``erode``, ``dilate`` and ``morph_gradient`` are the min / max filters over a flat square, disk or diamond (csrc/morph.hip;
kernels.KernelSpec.flat_morphology -- one launch each, exact, clipped to the image and optionally to ``within``), and ``opening``,
``closing``, ``white_tophat``, ``black_tophat``, ``open_by_reconstruction`` and ``close_by_reconstruction`` stand on them.  They sit
on the stain plane, between ``separate_stains`` / ``smooth`` and the threshold: an opening removes specks smaller than the footprint
where ``smooth`` would blur them, the white top-hat flattens an unevenly stained background before ``otsu_threshold``, and the
gradient of the plane is the other standard height for ``watershed`` -- it puts the cut on the stain edge, where the negated distance
map puts it on the geometric neck.  On a bool mask they are binary erosion and dilation with a square or diamond footprint (the EDT
gives the Euclidean disk).  End to end:
    plane = smooth(separate_stains(tile, planes=(0,))[0], 2)
    flat = white_tophat(plane, 15)                       # nuclei stand out, the background is gone
    fg = flat > otsu_threshold(flat)
    markers, n = label_instances(erode(fg, 2))           # cores: what survives a small erosion
    L = watershed(morph_gradient(plane, 1), markers, within=fg)

``rank_filter``, ``median``, ``quantile_range`` and ``local_entropy`` are the order statistics of the same windows (csrc/rank.hip;
kernels.KernelSpec.rank_filter -- one launch each, exact integers, footprints, clipping and ``within`` as erode).  ``median`` sits
between ``separate_stains`` and the threshold as the alternative to ``smooth``: it removes specks and keeps the stain edge that
``watershed(morph_gradient(plane, 1), ...)`` cuts on.  A low or high quantile is the robust erode or dilate -- one hot pixel does not
move it --, and ``quantile_range`` the robust gradient.  On a bool mask ``median`` is the majority filter, which smooths a ragged
foreground map in front of ``fill_holes`` / ``split_touching``; ``local_entropy`` (skimage.filters.rank.entropy) is a texture map to
threshold or to hand to ``watershed`` as a height:
    plane = median(separate_stains(tile, planes=(0,))[0], 2)
    fg = fill_holes(median(plane > otsu_threshold(plane), 1, 'square'))
    texture = local_entropy(bgr_to_gray(tile), 3)

``region_adjacency`` reads off a label image which regions touch and along how many pixels (csrc/adjacency.hip;
kernels.KernelSpec.region_adjacency), and ``voronoi_graph`` builds on it the other standard cell graph of the literature: the cells of
``expand_labels`` are the discrete Voronoi partition of the instance mask, and two nuclei are joined iff their cells share a border.
Its ``edge_index`` goes into ``graph_item(..., edge_index=...)`` in place of the radius graph on centroids.

``region_statistics``, ``region_histogram`` and ``region_quantiles`` join the planes of the image stage to the instance mask
(csrc/region.hip; kernels.KernelSpec.region_statistics, region_histogram, region_quantiles): per label value the count, sum, sum of
squares, minimum and maximum of a plane with the positions of both, its 256-bin histogram, and quantiles read off it -- one pass over
the pixels, exact integers, bit-identical from call to call, with ``within`` as everywhere else.  "The mean haematoxylin of nucleus
37" is ``region_mean_std(region_statistics(L, plane))[0][37]``, its median entropy ``region_quantiles(L, entropy_u8, 0.5)[37]``;
the ``max`` and ``argmax`` of ``region_statistics(L, distance_transform(L != 0))`` are the inscribed radius squared of every nucleus
and its centre.  ``ring_labels`` is the cytoplasm ring around every nucleus, and ``stain_features`` the node features the reference
stops short of: mean, spread, median and quantile range of haematoxylin and eosin per nucleus and, if wanted, per ring, row for row
beside the sixteen gray-level columns (the network's input width is a constructor argument):
    features, cen, kept = nucleus_features(L, gray, max_label=n)
    x = torch.cat([features, stain_features(L, tile, kept, ring=6, max_label=n)], 1)
    graph_item(x, cen, y)

``region_cooccurrence`` is the second-order statistic beside them (csrc/region.hip; kernels.KernelSpec.region_cooccurrence): per
label value and offset the grey-level co-occurrence table of any uint8 plane, over the pixel pairs that lie in the same region, at up
to 8 offsets of up to 16 pixels and 2 to 16 levels (``level_lut``) -- exact integers again, with ``within`` at both pixels of a pair.
``cooccurrence_properties`` reads the Haralick properties off the tables (contrast, dissimilarity, homogeneity, ASM, energy,
correlation, entropy), and ``texture_features`` is the chromatin texture of every nucleus: their mean and range over the four
directions ``COOC_DIRECTIONS`` on the haematoxylin plane, twelve columns beside the others.  The four GLCM columns among
``nucleus_features``' sixteen keep the reference's form (gray plane, one offset, 256 levels, a crop that includes the neighbours):
    x = torch.cat([features, stain_features(L, tile, kept, max_label=n), texture_features(L, tile, kept, hi=159, max_label=n)], 1)

``region_geometry`` is the shape beside them, from the label image alone (csrc/region.hip; kernels.KernelSpec.region_geometry): per
label value the pixel count, the coordinate sums up to second order, the extents in eight directions, the bit-quad counts and the
pixels on the image frame -- exact integers once more.  ``region_shape`` reads the usual properties off them (centroid, moments,
axes, eccentricity, orientation, bounding box, crack and bit-quad perimeter, circularity, Euler numbers, Feret widths, the area of the
enclosing 16-gon), ``shape_features`` is thirteen columns of them per nucleus, and ``clear_border`` drops the nuclei the tile cuts.
Nine of ``nucleus_features``' sixteen columns are shape too and keep the reference's form (a crop in which neighbours count as
foreground, one contour that may belong to a neighbour); these describe the pixels of their own label only, also where nuclei touch:
    x = torch.cat([features, stain_features(...), texture_features(...), shape_features(L, kept, max_label=n)], 1)

``region_hull`` is the one thing the geometry tables cannot give: the exact convex hull of the pixel squares of every label
(kernels.KernelSpec.region_hull) -- its vertices, twice its area, its diameter with the end points, its minimum width and its
perimeter, integers but for the last.  ``hull_shape`` reads true solidity and the true Feret diameters off it, and ``hull_features``
is seven columns of them per nucleus -- what a nucleus cut at a neck by ``split_touching`` or ``watershed`` needs:
    x = torch.cat([..., shape_features(L, kept, max_label=n), hull_features(L, kept, max_label=n)], 1)

``region_outlines`` gives the outline itself back: the ordered boundary of every label as closed polygons of lattice corners, outer
boundaries and holes (csrc/outline.hip; kernels.KernelSpec.region_outlines), in the convention of ``region_hull`` and
``perimeter_crack``.  ``outline_tables`` counts them per label, ``outline_polygons`` brings them to the host as rings with their holes,
at another resolution if asked, and ``evalio.outlines_to_geojson`` writes them as an annotation layer for a slide viewer:
    polygons = outline_polygons(region_outlines(L, max_label=n), kept, scale=(L.shape, slide_shape))

``superpixels`` is the one step that is not about nuclei: it cuts the tile into compact, colour-homogeneous, 4-connected tissue
regions -- stroma, epithelium, lumen -- by SLIC in exact integers (csrc/slic.hip; kernels.KernelSpec.slic_iterate, slic_merge), on
``separate_stains``' planes or the tile's own channels.  ``superpixel_graph`` (region contacts as edges), ``superpixel_features`` (area,
centroid, mean and spread of every plane) and ``regions_at`` (the region under every nucleus) make the tissue graph that hierarchical
cell-graph models place beside the cell graph:
    planes = separate_stains(tile)
    T, nt = superpixels(planes, 32)
    tissue = graph_item(*superpixel_features(T, planes, nt), y, edge_index=superpixel_graph(T, nt))
    node_of_nucleus = regions_at(T, cen) - 1

``resize``, ``rescale``, ``resize_labels``, ``rescale_labels`` and ``scale_points`` change the pixel size of a tile, a plane, a label
image and the coordinates that go with them (csrc/resample.hip; kernels.KernelSpec.resample_u8, resample_labels).  Every length of
the stage is a number of pixels -- radii, ``ring``, ``max_distance``, the area, axis and perimeter columns -- so tiles scanned at
another magnification are brought to one working resolution first, and a cheap coarse pass (an Otsu floor, a tissue mask,
``estimate_stains``) runs on an area-mean downscale:
    norm = normalize_stains(rescale(tile, Fraction(1, 2), 'area'))
Pixel centres sit at half-integers (cv2, PIL); 'linear' is exact rational bilinear interpolation with one rounding, 'area' the exact
box mean, 'nearest' and 'majority' keep label values -- integers with a stated contract like everything else here.  A mask from a
segmentation network that ran at another resolution than the tile meets the gray image either way round:
``nucleus_features(L, resize(gray, L.shape))`` is the reference's dataflow/construct_feature_graph.py:61, and
``resize_labels(L, gray.shape)`` keeps the tile's resolution instead.

``nucleus_features(labels, gray)`` returns the reference's ``feature`` / ``coordinate`` arrays of one image (csrc/nuclei.hip; the
arithmetic item by item: kernels.KernelSpec.nucleus_features), ``graph_item`` turns them into the ``Data`` that
``_read_one_raw_graph`` builds, and ``save_reference_files`` writes them where the reference's dataset preparation reads them.

Differences from the reference, all stated: an image without a surviving nucleus gives empty tensors (the reference's
``np.vstack`` raises); labels must be non-negative (``ValueError``, as skimage); gray and mask must have the same size
(``ValueError``; the reference resizes the gray image to the mask with cv2's bilinear interpolation, line 61 -- here that step is
spelled out, ``nucleus_features(L, resize(gray, L.shape))``, with exact weights where cv2 rounds them to 11 bits, and
``nucleus_features`` itself keeps its ``ValueError``).  OpenCV, scikit-image and xtract-features are restated from their
documented behaviour, not linked: see DESIGN.md, "Nucleus features".
"""
import collections
import math
import numbers
import operator
import os
from fractions import Fraction

import numpy as np
import torch

from . import kernels

NUM_FEATURES = 16
FEATURE_NAMES = ('mean_im_out', 'diff', 'var_im', 'skew_im', 'mean_ent', 'glcm_dissimilarity', 'glcm_homogeneity', 'glcm_energy',
                 'glcm_ASM', 'eccentricity', 'area', 'majoraxis_length', 'minoraxis_length', 'perimeter', 'solidity', 'orientation')
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
_INT32_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32)      # reconstruction: values must fit int32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
EDT_INF = kernels.EDT_INF          # dist2 of a pixel that has no site (within max_distance)
GEO_INF = kernels.GEO_INF          # geodesic dist of a pixel that no seed reaches (within max_distance)
GEODESIC_STEPS = {'cityblock': (1, 0), 'chessboard': (1, 1), 'chamfer': (5, 7)}      # (axial, diagonal) step costs; 0: no such step


def _check_image(fn, name, image, dtypes=(torch.bool,) + _INT_DTYPES, on_gpu=True):
    """The form of every image argument: a 2-D bool / integer tensor on the GPU of fewer than 2^31 pixels.  (nucleus_features takes
    no bool labels, and finds a tensor on the host at its launch: what it refuses before that, it refuses without a GPU.)"""
    if not torch.is_tensor(image) or (on_gpu and not image.is_cuda):
        raise TypeError('%s takes torch tensors on the GPU (%s)' % (fn, name))
    if image.dtype not in dtypes:
        raise TypeError('%s: %s must be %s integer image, got %s' % (fn, name, 'a bool or' if torch.bool in dtypes else 'an', image.dtype))
    if image.dim() != 2:
        raise ValueError('%s: %s must be 2-D (got %s)' % (fn, name, tuple(image.shape)))
    if image.shape[0] * image.shape[1] >= 2 ** 31:
        raise ValueError('%s: images of 2^31 pixels or more are not supported (%d x %d)' % ((fn,) + tuple(image.shape)))


def _check_within(fn, within, image):
    if within is None:
        return
    _check_image(fn, 'within', within)
    if tuple(within.shape) != tuple(image.shape) or within.device != image.device:
        raise ValueError('%s: within must have the shape and device of the image (got %s on %s and %s on %s)'
                         % (fn, tuple(within.shape), within.device, tuple(image.shape), image.device))


def _check_connectivity(connectivity):
    if connectivity not in (1, 2):
        raise ValueError('connectivity must be 1 (4 neighbours) or 2 (8 neighbours), got %r' % (connectivity,))


def _check_min_size(min_size):
    if min_size < 0:
        raise ValueError('min_size must not be negative (got %r)' % (min_size,))


def label_instances(image, connectivity=1, min_size=0, return_sizes=False):
    """image: 2-D bool / uint8 / int8 / int16 / int32 / int64 tensor on the GPU, any strides; 0 = background, every other value
    (negative ones too) foreground.  Returns (labels int32 [H, W], n) and, with ``return_sizes``, int32 [n] pixel counts (sizes[k - 1]
    belongs to label k).  Two pixels share a component iff a path of neighbours (``connectivity`` 1: 4 neighbours, 2: 8) that all
    carry the same value joins them, so a bool or 0/1 image is labelled as scipy.ndimage.label does -- components numbered 1..n by the
    raster order of their first pixels, bit for bit -- and an integer mask has each value split into its connected pieces.  With
    ``min_size`` > 0 components of fewer pixels become background and take no number (skimage's remove_small_objects, then labelling).

    Host syncs: one, the read of n."""
    _check_image('label_instances', 'image', image)
    _check_connectivity(connectivity)
    _check_min_size(min_size)
    H, W = image.shape
    if H * W == 0:
        labels, n = torch.zeros(H, W, dtype=torch.int32, device=image.device), 0
        sizes = torch.zeros(0, dtype=torch.int32, device=image.device)
    else:
        with torch.cuda.device(image.device):
            labels, n, sizes = kernels.get().label_components(image, int(connectivity), int(min_size), bool(return_sizes))
    return (labels, n, sizes) if return_sizes else (labels, n)


def _bound(distance, name, guess, value, cap):
    """The largest integer k with value(k) <= distance, for an increasing ``value``, capped at ``cap``.  guess(distance) is the
    inverse of ``value`` in floating point: int(guess) can be off by one in either direction, so its neighbours are checked."""
    d = float(distance)
    if not d >= 0:
        raise ValueError('%s must be a number >= 0 (got %r)' % (name, distance))
    if guess(d) >= cap + 1:
        return cap
    k = int(guess(d))
    while value(k + 1) <= d:
        k += 1
    while k > 0 and value(k) > d:
        k -= 1
    return k


def _d2max(distance, name):
    """The largest integer k with sqrt(k) <= distance (float64 sqrt, which is correctly rounded), capped at EDT_INF - 1, which no
    squared distance of a supported image exceeds."""
    return _bound(distance, name, lambda d: d * d, math.sqrt, EDT_INF - 1)


def distance_transform(image, sites='zero', max_distance=None, return_nearest=False):
    """image: 2-D bool / uint8 / int8 / int16 / int32 / int64 tensor on the GPU, any strides, each side <= 32767.  Returns dist2
    (int32 [H, W]): the exact squared Euclidean distance dy^2 + dx^2 from every pixel to the nearest site, 0 on sites -- and, with
    ``return_nearest``, nearest (int32 [H, W]): the raster index y' * W + x' of that site, of several equally near ones the one with
    the smallest raster index.  ``sites='zero'`` (default): the sites are the zero pixels, i.e. scipy.ndimage.distance_transform_edt
    (image) squared; ``sites='nonzero'``: the non-zero pixels.  Distances are measured to sites inside the image only (scipy's
    convention): a nucleus cut by the border is not near background there.  An image without a site gives dist2 = EDT_INF (2^31 - 1)
    and nearest = -1.  ``max_distance`` (float >= 0): pixels farther than that from every site report EDT_INF and -1, all others are
    exact, and the search stops there -- without it the cost per pixel grows with the distance to its nearest site (O(W) per pixel on
    rows whose columns hold no site).  ``dist2.double().sqrt()`` is the distance.

    Host syncs: none."""
    _check_image('distance_transform', 'image', image)
    if sites not in ('zero', 'nonzero'):
        raise ValueError("sites must be 'zero' or 'nonzero', got %r" % (sites,))
    d2max = -1 if max_distance is None else _d2max(max_distance, 'max_distance')
    with torch.cuda.device(image.device):      # the kernel table refuses sides over EDT_MAX_SIDE
        dist2, nearest = kernels.get().distance_transform(image, sites == 'nonzero', d2max, bool(return_nearest))
    return (dist2, nearest) if return_nearest else dist2


def _geodesic_steps(metric):
    """(a, b) of a name of GEODESIC_STEPS or of an (a, b) pair of integers with 1 <= a <= b <= 2a or b == 0."""
    if isinstance(metric, str):
        if metric not in GEODESIC_STEPS:
            raise ValueError('metric must be one of %s or an (a, b) pair, got %r' % (sorted(GEODESIC_STEPS), metric))
        return GEODESIC_STEPS[metric]
    try:
        a, b = metric
        ok = int(a) == a and int(b) == b and int(a) >= 1 and (int(b) == 0 or int(a) <= int(b) <= 2 * int(a))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('metric must be one of %s or a pair of integer step costs (a, b) with 1 <= a <= b <= 2a or b == 0, got %r'
                         % (sorted(GEODESIC_STEPS), metric))
    return int(a), int(b)


def _geodesic_bound(distance, a, name):
    """The largest integer k with k / a <= distance (a distance in pixels -> a bound in raw cost units), capped at GEO_INF - 1, which no
    path cost of a supported image exceeds."""
    return _bound(distance, name, lambda d: d * a, lambda k: k / a, GEO_INF - 1)


def _geodesic(seeds, within, metric, connectivity, distance, name, want_nearest):
    a, b = _geodesic_steps(metric)
    dmax = -1 if distance is None else _geodesic_bound(distance, a, name)
    with torch.cuda.device(seeds.device):      # the kernel table refuses a bad connectivity and path costs that overflow int32
        return kernels.get().geodesic_transform(seeds, within, a, b, connectivity, dmax, bool(want_nearest))


def geodesic_distance_transform(seeds, within=None, metric='chamfer', connectivity=1, max_distance=None, return_nearest=False):
    """seeds, within: 2-D bool / uint8 / int8 / int16 / int32 / int64 tensors on the same GPU, of the same shape, any strides.  Returns
    dist (int32 [H, W]): the smallest cost of a path from any seed (a non-zero pixel of ``seeds``) to the pixel that stays inside the
    domain {within != 0} u {seeds != 0} (``within=None``: the whole image), 0 on seeds -- and, with ``return_nearest``, nearest (int32
    [H, W]): the raster index y' * W + x' of the seed that attains it, of several the one with the smallest raster index.  ``metric``:
    a name of GEODESIC_STEPS -- 'cityblock' (1, 0), 'chessboard' (1, 1), 'chamfer' (5, 7) -- or a pair (a, b) of integers with 1 <= a
    <= b <= 2a or b == 0: an axial step costs a, a diagonal one b, b == 0 means no diagonal steps.  ``dist`` is in raw cost units:
    ``dist / a`` is the distance in pixels.  ``connectivity`` 2: a diagonal step needs only its two end points in the domain; 1
    (default): also one of the two pixels it passes between, so a path never squeezes through a corner contact -- the reached pixels
    are exactly the ``connectivity``-components of the domain that hold a seed.  A pixel outside the domain, or one no seed can reach,
    reports GEO_INF (2^31 - 1) and -1.  ``max_distance`` (pixels, float >= 0): pixels whose cost exceeds the largest integer k with
    k / a <= max_distance report GEO_INF and -1, all others are exact.  (b or a) * H * W must stay below 2^31 (ValueError).

    Host syncs: one per batch of relaxation rounds (8, then 16, 32, then 64 rounds each) until a round moves nothing: one when the
    growth crosses at most six edges of the 64 x 64 tiles (any bound of a few pixels), three for 56 rounds.  The number of rounds
    is 2 + the tile edges crossed by the longest shortest path: a serpentine corridor over a whole image is the case to avoid or to
    bound (kernels.KernelSpec.geodesic_transform)."""
    _check_image('geodesic_distance_transform', 'seeds', seeds)
    _check_within('geodesic_distance_transform', within, seeds)
    dist, nearest = _geodesic(seeds, within, metric, connectivity, max_distance, 'max_distance', return_nearest)
    return (dist, nearest) if return_nearest else dist


def expand_labels(labels, distance, within=None, geodesic=False, metric='chamfer', connectivity=1):
    """skimage.segmentation.expand_labels on the GPU, with a stated tie rule.  labels: 2-D bool / integer tensor on the GPU (0 =
    background).  Every background pixel whose nearest labelled pixel lies within ``distance`` (Euclidean, sqrt(dist2) <= distance)
    takes that pixel's value; of several equally near labelled pixels the one with the smallest raster index decides.  ``within``
    (same shape, bool / integer): only background pixels that are also non-zero in ``within`` may be filled.  Nearness stays
    Euclidean, not geodesic: ``within`` selects which pixels are filled, not the paths along which distance is measured, so a label
    can reach across a gap of ``within``.  Labelled pixels never change; the output has the input's dtype.  The distance transform
    underneath is bounded by ``distance``.

    ``geodesic=True``: nearness is geodesic instead -- the seeds are the labelled pixels, the domain is ``within`` (None: the whole
    image), and a background pixel of the domain whose path cost (``metric``, ``connectivity``: see geodesic_distance_transform) is
    within ``distance`` pixels takes the value of the labelled pixel that attains it (ties: the smallest raster index): no label
    crosses a gap of ``within``.  ``distance=None`` (only then) means unbounded: every domain pixel joined to a label is filled.

    Host syncs: none; with ``geodesic=True`` those of geodesic_distance_transform (one for a bound of a few pixels)."""
    _check_image('expand_labels', 'labels', labels)
    _check_within('expand_labels', within, labels)
    if geodesic:
        _, nearest = _geodesic(labels, within, metric, connectivity, distance, 'distance', True)
        fill = nearest >= 0                     # -1: outside the domain, not joined to a label or beyond the bound
    else:
        if distance is None:
            raise ValueError('distance=None (unbounded growth) needs geodesic=True')
        return _grow_euclidean(labels, _d2max(distance, 'distance'), within)[0]
    return _take_nearest(labels, nearest, fill)


def _take_nearest(labels, nearest, fill):
    # a labelled pixel is its own nearest site, so the gather returns it unchanged
    src = labels.reshape(-1)[nearest.clamp_(min=0).reshape(-1).long()].reshape(labels.shape)
    return torch.where(fill, src, labels)


def _grow_euclidean(labels, d2max, within=None):
    """(grown, dist2) of expand_labels' Euclidean growth: one distance transform gives both the cells and every pixel's squared
    distance to its nearest labelled pixel (EDT_INF beyond the bound)."""
    with torch.cuda.device(labels.device):
        dist2, nearest = kernels.get().distance_transform(labels, True, d2max, True)
    fill = nearest >= 0                         # -1: nothing within reach
    if within is not None:
        fill &= (labels != 0) | (within != 0)
    return _take_nearest(labels, nearest, fill), dist2


def reconstruct(marker, mask, method='dilation', connectivity=1):
    """Grayscale morphological reconstruction (Vincent 1993).  marker, mask: 2-D bool / uint8 / int8 / int16 / int32 tensors on the
    same GPU, of the same shape, any strides (int64 is a TypeError: values must fit int32, and checking that would cost a host read).
    Returns the reconstruction in the marker's dtype, contiguous; bool counts as 0 / 1.

    ``method='dilation'``: R0 = min(marker, mask) pointwise (a marker above the mask is clamped, not refused) and R is the fixed
    point of R[p] = min(mask[p], max(R[p], max over the neighbours q of R[q])): R[p] is the largest, over pixels q and paths of
    neighbours from q to p, of min(R0[q], the smallest mask value on the path) -- the marker's peaks spread under the mask as far as
    the mask lets them.  ``connectivity`` 1: 4 neighbours, a diagonal corner contact does not conduct; 2: 8 neighbours, it does.
    ``method='erosion'``: the dual (min and max exchanged; a marker below the mask is raised to it), computed as
    ~dilation(~marker, ~mask) with bitwise NOT, which reverses order on all of int32 and cannot overflow.
    The computation is in int32 and exact (kernels.KernelSpec.morph_reconstruct); the result lies between min(marker, mask) and mask
    (dilation), so it fits the marker's dtype whenever the mask's values do.

    Host syncs: one per batch of relaxation rounds (8, then 16, 32, then 64 rounds each) until a round moves nothing; the number of
    rounds is 2 + the 64 x 64 tile edges crossed by the longest path along which a value has to travel.  A serpentine plateau over
    a whole image is the case to avoid."""
    _check_image('reconstruct', 'marker', marker, _INT32_DTYPES)
    _check_image('reconstruct', 'mask', mask, _INT32_DTYPES)
    if tuple(marker.shape) != tuple(mask.shape) or marker.device != mask.device:
        raise ValueError('reconstruct: marker and mask must have the same shape and device (got %s on %s and %s on %s)'
                         % (tuple(marker.shape), marker.device, tuple(mask.shape), mask.device))
    if method not in ('dilation', 'erosion'):
        raise ValueError("method must be 'dilation' or 'erosion', got %r" % (method,))
    _check_connectivity(connectivity)
    with torch.cuda.device(marker.device):
        out = kernels.get().morph_reconstruct(marker.to(torch.int32), mask.to(torch.int32), int(connectivity), method == 'erosion')
    return out != 0 if marker.dtype == torch.bool else out.to(marker.dtype)


def watershed(height, markers, within=None, metric='chamfer', connectivity=1, return_level=False):
    """Marker-controlled (seeded) watershed.  height: 2-D bool / uint8 / int8 / int16 / int32 tensor on the GPU, any strides (int64 is
    a TypeError: values must fit int32, and checking that would cost a host read); markers, within: 2-D bool / integer tensors of the
    same shape on the same GPU (0 = no marker / outside the domain).  Returns the labels in the markers' dtype and, with
    ``return_level``, level (int32 [H, W]).

    Water rises from the marker pixels over ``height`` inside the domain {within != 0} u {markers != 0} (``within=None``: the whole
    image), along the steps of geodesic_distance_transform (``metric``, ``connectivity``: the same names, pairs and corner rule).  A
    pixel is wetted at level = the lowest, over all paths from any marker pixel, of the highest height on the path after the marker
    (height with its unmarked basins filled to their lowest pass), and on that level by the path that has travelled the least since
    it last rose (kernels.KernelSpec.watershed_flood, items 2 and 3: the definition does not depend on any processing order, so the
    result is a pure function of the input, bit for bit).  Every wetted pixel takes the value of the marker pixel at the root of its
    chain of parents; marker pixels never change; a pixel outside the domain, or one that no marker reaches, is 0 -- the reached
    pixels are exactly the ``connectivity``-components of the domain that hold a marker.  Two basins meet on the pass between
    them: there is no watershed line, every reached pixel has a label.  level is ``height`` on marker and unreached pixels.
    (b or a) * H * W must stay below 2^31 (ValueError).

    Host syncs: one per batch of relaxation rounds (8, then 16, 32, then 64 rounds each) until a round moves nothing, as
    geodesic_distance_transform, then one per batch of 8 pointer jumps until a jump moves nothing (one when no chain of parents is
    longer than 128 pixels): two in all for nuclei-sized basins.  A serpentine valley over a whole image is the case to avoid."""
    _check_image('watershed', 'height', height, _INT32_DTYPES)
    _check_image('watershed', 'markers', markers)
    if tuple(markers.shape) != tuple(height.shape) or markers.device != height.device:
        raise ValueError('watershed: height and markers must have the same shape and device (got %s on %s and %s on %s)'
                         % (tuple(height.shape), height.device, tuple(markers.shape), markers.device))
    _check_within('watershed', within, height)
    a, b = _geodesic_steps(metric)
    _check_connectivity(connectivity)
    with torch.cuda.device(height.device):      # the kernel table refuses path lengths that overflow int32
        level, source = kernels.get().watershed_flood(height.to(torch.int32), markers, within, a, b, int(connectivity))
    # a marker pixel is its own root, so the gather returns it unchanged
    src = markers.reshape(-1)[source.clamp(min=0).reshape(-1).long()].reshape(markers.shape)
    labels = torch.where(source >= 0, src, torch.zeros_like(src))
    return (labels, level) if return_level else labels


def _check_h(h):
    try:
        h = operator.index(h)
    except TypeError:
        raise TypeError('h must be an integer (got %r)' % (h,))
    if not 1 <= h <= INT32_MAX:
        raise ValueError('h must lie in [1, 2^31 - 1] (got %d)' % h)
    return h


def h_maxima(image, h, connectivity=1):
    """The h-maxima markers of an image.  image: 2-D bool / uint8 / int8 / int16 / int32 tensor on the GPU, any strides; ``h``: an
    integer, 1 <= h <= 2^31 - 1.  Returns the bool map (image - reconstruct(image - h, image)) >= h, where image - h saturates at the
    int32 minimum: True exactly on the summit plateaus of those regional maxima whose dynamic -- the height of the summit above the
    highest saddle on a path to any higher pixel -- is at least ``h``.  A maximum that a saddle shallower than ``h`` joins to a higher
    one is not marked.  The highest summit has no higher pixel, so its dynamic is unbounded and it is marked for every ``h`` (where
    skimage's h_maxima returns nothing once ``h`` exceeds max - min) -- except where image - h saturates: a pixel less than ``h``
    above the int32 minimum is never marked, so an ``h`` larger than the room between the image and the int32 minimum gives all
    False.

    Host syncs: those of reconstruct."""
    _check_image('h_maxima', 'image', image, _INT32_DTYPES)
    h = _check_h(h)
    _check_connectivity(connectivity)
    wide = image.to(torch.int64)
    mask = wide.to(torch.int32)
    marker = (wide - h).clamp_(min=INT32_MIN).to(torch.int32)
    with torch.cuda.device(image.device):
        rec = kernels.get().morph_reconstruct(marker, mask, int(connectivity), False)
    return (wide - rec) >= h


def regional_maxima(image, connectivity=1):
    """The regional maxima of an image (arguments as h_maxima): True on every ``connectivity``-connected plateau of equal values that
    has no higher neighbour.  It is h_maxima(image, 1, connectivity).

    Host syncs: those of reconstruct."""
    return h_maxima(image, 1, connectivity)


def fill_holes(image, connectivity=1):
    """Fill the holes of a mask.  image: 2-D bool / uint8 / int8 / int16 / int32 tensor on the GPU, any strides.  A hole is a
    ``connectivity``-component (1: 4 neighbours, 2: 8) of the background {image == 0} that does not touch the image border.  Returns
    a tensor of the input's dtype.
      bool image: the holes become True; with connectivity 1 this is scipy.ndimage.binary_fill_holes, bit for bit.  One reconstruction
        of the marker (background on the border) under the mask (background): what it does not reach are the holes.
      integer image (an instance mask): every hole pixel takes the value of the geodesically nearest labelled pixel along paths
        inside the hole -- expand_labels(image, None, within=holes, geodesic=True, connectivity=connectivity): a ring of one label
        closes with that label, a hole bordered by two labels is shared between them (ties: expand_labels' rule).
    Labelled pixels and the background outside the holes never change.

    Host syncs: those of reconstruct -- the flood starts at the four borders and meets in the middle, so about max(H, W) / 128 rounds
    when the open background is one sheet (three reads for 3584 x 3584), more where it winds -- plus, for an integer image, those of geodesic_distance_transform (one for holes narrower than
    a few tiles)."""
    _check_image('fill_holes', 'image', image, _INT32_DTYPES)
    _check_connectivity(connectivity)
    H, W = image.shape
    if H * W == 0:
        return image.clone()
    background = image == 0
    border = torch.zeros_like(background)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    outside = reconstruct(background & border, background, 'dilation', connectivity)
    holes = background & ~outside
    if image.dtype == torch.bool:
        return image | holes
    return expand_labels(image, None, within=holes, geodesic=True, connectivity=connectivity)


def _eighths(dist2):
    """T (int32): the largest integer with T^2 <= 64 dist2 -- the distance in eighths of a pixel, defined in integers: float64 sqrt
    (64 dist2 < 2^37 is exact in float64, the root is off by at most one), then corrected by +-1 in integer arithmetic."""
    v = dist2.to(torch.int64) * 64
    t = v.to(torch.float64).sqrt_().to(torch.int64)
    t -= (t * t > v).to(torch.int64)
    t += ((t + 1) * (t + 1) <= v).to(torch.int64)
    return t.to(torch.int32)


def split_touching(mask, core_radius, connectivity=1, min_size=0, growth='euclidean', markers='core', h=None):
    """The erode-label-grow split of a foreground mask (2-D bool / integer tensor on the GPU, 0 = background) into instances, for
    nuclei that touch: returns (labels int32 [H, W], n) as ``label_instances`` does, ready for ``nucleus_features(labels, gray,
    max_label=n)``.
      1. dist2 = distance_transform(mask): squared distance of every foreground pixel to the background inside the image;
      2. the cores -- pixels farther than ``core_radius`` from the background -- are labelled (``connectivity``);
      3. the cores grow back by ``core_radius`` + 1 inside the mask (expand_labels(..., within=mask)): the opening of the mask,
         partitioned by nearest core, plus the one-pixel rim that the opening of a digital shape leaves behind (grown by
         ``core_radius`` alone, a disc of radius 10 sheds 24 single-pixel slivers at core_radius 8, each of which would count as a
         nucleus; the mask clips what the extra pixel oversteps);
      4. what is left of the mask (thin bridges, slivers, objects without a core) is labelled on its own: no foreground pixel is lost;
      5. label_instances(combined, connectivity, min_size) splits every value into its connected pieces, applies ``min_size`` and
         numbers the result 1..n by first pixel.
    ``core_radius`` = 0 is label_instances(mask != 0, connectivity, min_size).

    ``growth='geodesic'``: step 3 is expand_labels(cores, None, within=mask, geodesic=True, connectivity=connectivity) instead --
    unbounded, chamfer (5, 7) steps along paths inside the mask: every mask pixel that is connected to a core takes the geodesically
    nearest core, however narrow the part it sits in, and never a core of another object.  Step 4 is then exactly the components
    that hold no core.  The Euclidean growth cannot reach parts narrower than the core radius (tapered tips, necks), which become
    instances of their own, and hands pixels to the nearest core across a gap, which step 5 splits off as fragments.

    ``growth='flood'``: step 3 is watershed(-T, cores, within=mask, connectivity=connectivity) instead, with T = the largest integer
    with T^2 <= 64 dist2 (the distance to the background in eighths of a pixel): water rises from the cores over the negated distance
    map, chamfer (5, 7) steps inside the mask, and two cores' waters meet where the ridge of the distance map between them is lowest
    -- the neck.  What this buys: the cut no longer moves with the sizes of the two nuclei.  Two touching discs of radius 28 and 16
    are cut at the neck, within a pixel or two, and the large one keeps its pixels, where the geodesic growth cuts on the midline
    between the cores, seven columns inside the large disc, and hands 8 % of it to the small one.  Like the geodesic growth it
    reaches every mask pixel that is connected to a core and never a core of another object, so step 4 is again the components that
    hold no core.  What it does not: it decides nothing about which cores exist -- a nucleus with two cores is still cut in two, one
    without a core still merges with its neighbour -- and where there is no neck (two overlapping discs that form a convex blob) the
    pass is flat and the cut is wherever the two waters meet on it, which is no better than the midline.

    ``markers='h_maxima'`` (needs ``growth='geodesic'`` or ``'flood'`` and ``h``, in pixels; ``core_radius`` is ignored): only step 2 changes.  With
    T = the largest integer with T^2 <= 64 dist2 (the distance to the background in eighths of a pixel) and h8 = the largest integer
    with h8 / 8 <= h (at least 1: ValueError otherwise), the cores are label_instances(h_maxima(T, h8, connectivity) & mask,
    connectivity): the summit plateaus of those maxima of the distance map that stand at least ``h`` above the saddle towards any
    higher one (``& mask`` only matters for an image without foreground, whose flat distance map is one plateau).  What this buys:
    one core, hence one node, per nucleus whatever its size -- a global ``core_radius`` large enough to cut the neck between two
    large nuclei erases the cores of the small ones, and one small enough to keep those does not cut the neck -- and ``h`` only asks
    how deep the neck is compared with the lower summit.  What it does not: summit plateaus are a few pixels wide, so growing them
    back by a Euclidean radius has no meaning (hence the geodesic growth), and with ``growth='geodesic'`` the cut between two nuclei
    falls on the geodesic midline between the two summits, which for very unequal nuclei is not the neck (``growth='flood'`` puts it
    there).

    Host syncs: three, the reads of n of the three labelling calls; with ``growth='geodesic'`` plus those of the convergence loop of
    geodesic_distance_transform (one when the longest path inside a nucleus crosses at most six tile edges, two up to 22); with
    ``markers='h_maxima'`` plus those of reconstruct (one when no nucleus spans more than six tile edges); with ``growth='flood'``
    plus those of watershed (two for nuclei-sized basins)."""
    _check_image('split_touching', 'mask', mask)
    if growth not in ('euclidean', 'geodesic', 'flood'):
        raise ValueError("growth must be 'euclidean', 'geodesic' or 'flood', got %r" % (growth,))
    if markers not in ('core', 'h_maxima'):
        raise ValueError("markers must be 'core' or 'h_maxima', got %r" % (markers,))
    if markers == 'h_maxima':
        if growth not in ('geodesic', 'flood'):
            raise ValueError("markers='h_maxima' needs growth='geodesic' or 'flood': summit plateaus cannot be grown back by a Euclidean radius")
        if h is None:
            raise ValueError("markers='h_maxima' needs h, the least dynamic of a marker in pixels")
        h8 = _bound(h, 'h', lambda d: d * 8, lambda k: k / 8, INT32_MAX)
        if h8 < 1:
            raise ValueError('h must be at least 1 / 8 pixel (got %r)' % (h,))
    else:
        if h is not None:
            raise ValueError("h is only used with markers='h_maxima'")
        radius2 = _d2max(core_radius, 'core_radius')
    _check_connectivity(connectivity)
    _check_min_size(min_size)
    fg = mask != 0                          # an empty image goes through every step as an empty tensor, without a host read
    dist2 = distance_transform(fg)
    if markers == 'h_maxima':
        cores, k = label_instances(h_maxima(_eighths(dist2), h8, connectivity) & fg, connectivity)
    else:
        cores, k = label_instances(dist2 > radius2, connectivity)
    if growth == 'flood':
        grown = watershed(-_eighths(dist2), cores, within=fg, connectivity=connectivity)
    elif growth == 'geodesic':
        grown = expand_labels(cores, None, within=fg, geodesic=True, connectivity=connectivity)
    else:
        grown = expand_labels(cores, float(core_radius) + 1.0, within=fg)
    rest, _ = label_instances(fg & (grown == 0), connectivity)
    combined = torch.where(rest > 0, rest + k, grown)
    return label_instances(combined, connectivity, min_size)


def _check_labels32(fn, name, labels):
    """A label image whose values are themselves output: int64 is refused instead of narrowed."""
    _check_image(fn, name, labels)
    if labels.dtype == torch.int64:
        raise TypeError('%s: %s must fit int32, whose values are output: pass %s.to(torch.int32)' % (fn, name, name))


def region_adjacency(labels, connectivity=1, value=None):
    """Which regions of a label image touch, and along how many pixel pairs (csrc/adjacency.hip; the contract item by item:
    kernels.KernelSpec.region_adjacency).  labels: 2-D bool / uint8 / int8 / int16 / int32 tensor on the GPU, any strides, fewer than
    2^29 pixels; 0 = background, every other value (negative ones too) a region, connected or not.  int64 is a TypeError (``labels.to(
    torch.int32)``): the values themselves are output and must fit.  A contact is an unordered pair of neighbouring pixels
    (``connectivity`` 1: horizontal and vertical neighbours, 2: also diagonal ones) that carry two different non-zero values.  Returns
    (pairs int32 [P, 2], count int32 [P]): rows (a, b) with a < b, sorted lexicographically, each pair once, and its number of
    contacts -- e.g. which instances of ``split_touching`` still touch, and along how many pixels.  ``value`` (bool / uint8 / int8 /
    int16 / int32, same shape and device: ValueError otherwise, TypeError for another dtype, as for ``within`` elsewhere): a third
    output min_sum int32 [P], the smallest value[p] + value[q] over the pair's contacts (summed in 64 bits, clamped to int32).  The
    outputs are a pure function of the inputs.  An empty image gives empty tensors without a launch.

    Host syncs: two, the reads of the number of per-tile records and of P; none for an empty image."""
    _check_labels32('region_adjacency', 'labels', labels)
    _check_connectivity(connectivity)
    if value is not None:
        _check_image('region_adjacency', 'value', value, _INT32_DTYPES)
        if tuple(value.shape) != tuple(labels.shape) or value.device != labels.device:
            raise ValueError('region_adjacency: value must have the shape and device of labels (got %s on %s and %s on %s)'
                             % (tuple(value.shape), value.device, tuple(labels.shape), labels.device))
    H, W = labels.shape
    if H * W >= kernels.ADJ_MAX_PIXELS:
        raise ValueError('region_adjacency: images of 2^29 pixels or more are not supported (%d x %d)' % (H, W))
    i32 = dict(dtype=torch.int32, device=labels.device)
    if H * W == 0:
        out = (torch.empty(0, 2, **i32), torch.empty(0, **i32), torch.empty(0, **i32))
    else:
        with torch.cuda.device(labels.device):
            out = kernels.get().region_adjacency(labels.to(torch.int32), int(connectivity), None if value is None else value.to(torch.int32))
    return out[:2] if value is None else out


def voronoi_graph(labels, max_distance, kept_labels=None, connectivity=1, loop=True, max_gap=None, return_attr=False):
    """The cell graph whose edges join nuclei with neighbouring Voronoi cells (the Delaunay / Voronoi construction of the cell-graph
    literature, on the nuclei's shapes instead of their centroids): symmetric, no degree cap, measured from the nuclei's outlines, and
    never across a third nucleus that lies between two.  labels: 2-D bool / uint8 / int8 / int16 / int32 instance mask on the GPU (0 =
    background; int64 is a TypeError), non-negative (ValueError).  Returns edge_index int64 [2, E] and, with ``return_attr``, (edge_index,
    border int32 [E], gap float32 [E]).
      1. Nodes.  Node i is label kept_labels[i]: int32, strictly ascending, positive, on the labels' device, as ``nucleus_features``
         returns it -- edge ends are then row numbers of its feature table.  ``None``: the distinct non-zero labels in ascending order.
         Pixels of labels that are not kept become background before growing: a nucleus that ``min_size`` removed claims no cell.
      2. Cells.  cells = expand_labels(kept, max_distance): Euclidean growth, ties to the smallest raster index; dist2 comes from the
         same distance transform.
      3. Distance plane.  T = the largest integer with T^2 <= 64 dist2 (eighths of a pixel), 0 where no nucleus is within reach.
      4. Adjacency.  pairs, count, min_sum = region_adjacency(cells, connectivity, value=T).
      5. Gap.  gap8 = min_sum + 8: the length, in eighths of a pixel, of the shortest path from one nucleus to the other that crosses
         their common border in one axial step.  It is NOT the true gap between the two outlines: it is at least the true gap minus
         1/4 pixel (two floors) and usually equal to it, but where a third nucleus hides the two closest points from the shared border
         it is larger (on a 300 x 300 synthetic tissue at max_distance 50: median excess 0.05 px, largest 18.9 px), and a purely
         diagonal contact (connectivity 2) is short by 3/8 px.  ``max_gap`` (pixels, float >= 0) keeps the pairs with gap8 <= the
         largest integer k with k / 8 <= max_gap.
      6. Output.  edge_index in ``radius_knn``'s convention: rows are centres in ascending order, then columns in ascending order.
         Both directions of every pair are present; (i, i) is present for every node iff ``loop``.  border = the pair's contacts (0
         on loops), gap = gap8 / 8 (0 on loops).

    Host syncs: one read that checks the labels' sign (and kept_labels' order), one for the distinct labels when kept_labels is None,
    the two of region_adjacency, and one for the pairs ``max_gap`` keeps."""
    _check_labels32('voronoi_graph', 'labels', labels)
    _check_connectivity(connectivity)
    d2max = _d2max(max_distance, 'max_distance')
    g8max = None if max_gap is None else _bound(max_gap, 'max_gap', lambda d: d * 8, lambda k: k / 8, INT32_MAX)
    dev = labels.device
    if kept_labels is not None:
        if not torch.is_tensor(kept_labels) or kept_labels.dtype != torch.int32 or kept_labels.dim() != 1 or kept_labels.device != dev:
            raise ValueError('voronoi_graph: kept_labels must be a 1-D int32 tensor on the device of labels')
    labels = labels.to(torch.int32)
    checks = [labels.min() < 0 if labels.numel() else torch.zeros((), dtype=torch.bool, device=dev)]
    if kept_labels is not None:
        checks.append((kept_labels[:1] <= 0).any() | (kept_labels[1:] <= kept_labels[:-1]).any())
    checks = torch.stack(checks).tolist()            # host sync: the labels' sign, the order of kept_labels
    if checks[0]:
        raise ValueError('voronoi_graph: negative labels in the instance mask')
    if kept_labels is None:
        kept_labels = torch.unique(labels[labels != 0])      # host sync: the distinct labels, ascending
        kept = labels
    else:
        if checks[1]:
            raise ValueError('voronoi_graph: kept_labels must be positive and strictly ascending')
        if kept_labels.numel() == 0:
            kept = torch.zeros_like(labels)
        else:
            slot = torch.searchsorted(kept_labels, labels).clamp_(max=kept_labels.numel() - 1)
            kept = torch.where(kept_labels[slot] == labels, labels, 0)
    n = int(kept_labels.numel())
    i64 = dict(dtype=torch.int64, device=dev)
    src = dst = torch.empty(0, **i64)
    border, gap8 = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, **i64)
    if n > 0 and labels.numel() > 0:
        cells, dist2 = _grow_euclidean(kept, d2max)
        t = torch.where(dist2 == EDT_INF, 0, _eighths(dist2))
        pairs, border, min_sum = region_adjacency(cells, connectivity, value=t)
        gap8 = min_sum.to(torch.int64) + 8
        if g8max is not None:
            keep = gap8 <= g8max
            pairs, border, gap8 = pairs[keep], border[keep], gap8[keep]      # host sync: how many pairs are kept
        ends = torch.searchsorted(kept_labels, pairs).to(torch.int64)       # every cell's label is a kept one
        src, dst = ends[:, 0], ends[:, 1]
    rows, cols = torch.cat([src, dst]), torch.cat([dst, src])
    border, gap8 = torch.cat([border, border]), torch.cat([gap8, gap8])
    if loop:
        nodes = torch.arange(n, **i64)
        rows, cols = torch.cat([rows, nodes]), torch.cat([cols, nodes])
        border, gap8 = torch.cat([border, torch.zeros(n, dtype=torch.int32, device=dev)]), torch.cat([gap8, torch.zeros(n, **i64)])
    order = torch.argsort(rows * max(n, 1) + cols)       # (row, col) pairs are distinct
    edge_index = torch.stack([rows[order], cols[order]])
    if return_attr:
        return edge_index, border[order], (gap8[order].to(torch.float64) / 8).to(torch.float32)
    return edge_index


def nucleus_features(labels, gray, min_size=10, return_info=False, max_label=None):
    """labels: integer [H, W] instance mask on the GPU (0 = background; other integer dtypes are converted to int32), gray: uint8
    [H, W] on the same GPU.  Returns (features f32 [n, 16], centroids f32 [n, 2] as (row, col), kept_labels int32 [n]) -- row k
    describes the k-th surviving label in ascending order -- plus, with ``return_info``, int32 [n, 4]: the traced contour's start
    (row, col) in the crop, its vertex count and the path taken (0 LDS, 1 global workspace).

    Host syncs: one read of the label range (negative labels raise ValueError; the tables are indexed by label value, so very sparse
    label ids cost memory in proportion to the largest) and one read of the row count.  ``max_label`` (an int >= the largest label,
    e.g. the n of ``label_instances``) replaces the read of the label range; pixels outside [0, max_label] then raise ValueError."""
    _check_image('nucleus_features', 'labels', labels, _INT_DTYPES, on_gpu=False)
    if not torch.is_tensor(gray):
        raise TypeError('nucleus_features takes torch tensors on the GPU (gray)')
    if tuple(gray.shape) != tuple(labels.shape):
        raise ValueError('labels and gray must be 2-D images of the same size (got %s and %s)'
                         % (tuple(labels.shape), tuple(gray.shape)))
    if gray.dtype != torch.uint8:
        raise TypeError('gray must be uint8, got %s' % gray.dtype)
    H, W = labels.shape
    dev = labels.device
    if max_label is not None:
        lo, hi = 0, int(max_label)
        if hi < 0:
            raise ValueError('max_label must not be negative (got %d)' % hi)
    elif H * W == 0:
        lo = hi = 0
    else:
        lo, hi = torch.stack([labels.min(), labels.max()]).to(torch.int64).tolist()
    if lo < 0:
        raise ValueError('negative labels in the instance mask (remove_small_objects refuses them)')
    if hi >= 2 ** 31 - 1:
        raise ValueError('label values must fit int32 (largest: %d)' % hi)
    if hi == 0 and (max_label is None or H * W == 0):
        out = (torch.zeros(0, NUM_FEATURES, dtype=torch.float32, device=dev), torch.zeros(0, 2, dtype=torch.float32, device=dev),
               torch.zeros(0, dtype=torch.int32, device=dev))
        return out + (torch.zeros(0, 4, dtype=torch.int32, device=dev),) if return_info else out
    feats, cen, kept, info = kernels.get().nucleus_features(labels.to(torch.int32).contiguous(), gray.contiguous(), int(hi),
                                                            int(min_size), bool(return_info))
    return (feats, cen, kept, info) if return_info else (feats, cen, kept)


def bgr_to_gray(bgr):
    """cv2.cvtColor(image, cv2.COLOR_BGR2GRAY) of a uint8 [H, W, 3] image on the GPU (construct_feature_graph.py:60)."""
    if not torch.is_tensor(bgr) or bgr.dtype != torch.uint8 or bgr.dim() != 3 or bgr.shape[2] != 3:
        raise ValueError('bgr_to_gray takes a uint8 [H, W, 3] tensor')
    return kernels.get().bgr_to_gray(bgr)


def _od_lut():
    """The optical density of every channel value in 1/1024 of a natural-log unit: floor(1024 ln(255 / max(v, 1)) + 0.5).  No entry
    lies within 1e-3 of a rounding boundary (tests/test_stain_ref_cpu.py), so every libm gives the same table."""
    return tuple(int(math.floor(1024.0 * math.log(255.0 / max(v, 1)) + 0.5)) for v in range(256))


OD_LUT = _od_lut()
# unit OD vectors (R, G, B) of haematoxylin, eosin and a residual (Ruifrok and Johnston 2001; rows are normalised by stain_matrix)
DEFAULT_STAINS = ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78))
STAIN_ORDERS = {'bgr': 0, 'rgb': 1}
ANGLE_BINS = kernels.ANGLE_BINS
CONC_BINS = kernels.CONC_BINS
# the reference stains and their robust maxima of Macenko's published implementation: unit OD vectors (R, G, B) of haematoxylin and
# eosin, and the 99th percentiles of their concentrations in natural-log units
TARGET_STAINS = ((0.5626, 0.7201, 0.4062), (0.2159, 0.8012, 0.5581))
TARGET_MAX = (1.9705, 1.0308)


def _exp_lut():
    """The channel value of every optical density in 1/1024 of a natural-log unit: floor(255 exp(-k / 1024) + 0.5) for k = 0..6385,
    from 255 down to the first 0.  No 255 exp(-k / 1024) + 0.5 lies within 1e-6 of an integer (the nearest is 1.79e-5 away, at
    k = 6384; tests/test_normalize_ref_cpu.py), so every libm gives the same table.  EXP_LUT[OD_LUT[v]] = v for v = 1..255."""
    return tuple(int(math.floor(255.0 * math.exp(-k / 1024.0) + 0.5)) for k in range(kernels.EXP_LUT_LEN))


EXP_LUT = _exp_lut()


def _angle_dirs():
    """The K - 1 directions that separate the K angle bins of estimate_stains: (rint(16384 cos t_k), rint(16384 sin t_k)) with
    t_k = -pi/2 + k pi / K in float64, k = 1..K-1.  No entry lies within 1e-6 of a rounding boundary (the nearest is 4.0e-4 away) and
    the angles of the rounded directions increase strictly (tests/test_macenko_ref_cpu.py), so every libm gives the same table."""
    K = ANGLE_BINS
    return tuple((int(round(16384.0 * math.cos(-0.5 * math.pi + k * math.pi / K))),
                  int(round(16384.0 * math.sin(-0.5 * math.pi + k * math.pi / K)))) for k in range(1, K))


ANGLE_DIRS = _angle_dirs()


def stain_matrix(stains=None):
    """The fixed-point deconvolution matrix of three stains: numpy int32 [3, 3], m[c][s] = rint(4096 inv(S)[c][s]), c = 0 R, 1 G, 2 B.
    ``stains``: 3 x 3 numbers, row s = the optical-density vector (R, G, B) of stain s, any positive length (None: DEFAULT_STAINS --
    haematoxylin, eosin, residual).  The rows are normalised to unit length and S is inverted in float64.  ValueError: a shape other
    than 3 x 3, a non-finite entry, a zero row, a singular matrix, or a column with sum_c |m[c][s]| * 5674 >= 2^31 - 2^15 (stains so
    nearly dependent that the int32 arithmetic of separate_stains could overflow)."""
    try:
        S = np.array(DEFAULT_STAINS if stains is None else stains, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('stains must be 3 x 3 numbers')
    if S.shape != (3, 3):
        raise ValueError('stains must be 3 x 3 (got shape %s)' % (S.shape,))
    if not np.isfinite(S).all():
        raise ValueError('stains must be finite')
    norm = np.sqrt((S * S).sum(axis=1))
    if not (norm > 0).all() or not np.isfinite(norm).all():
        raise ValueError('every stain needs a non-zero optical-density vector')
    S = S / norm[:, None]
    try:
        inv = np.linalg.inv(S)
    except np.linalg.LinAlgError:
        raise ValueError('the stain vectors are linearly dependent')
    if not np.isfinite(inv).all() or np.linalg.matrix_rank(S) < 3:
        raise ValueError('the stain vectors are linearly dependent')
    q = np.rint(4096.0 * inv)
    if (np.abs(q).sum(axis=0) * kernels.STAIN_OD_MAX >= 2 ** 31 - 2 ** 15).any():
        raise ValueError('the stain vectors are too nearly dependent: the int32 sum of separate_stains could overflow')
    return q.astype(np.int32)


def _check_color(fn, image):
    """A colour image: a uint8 [H, W, 3] tensor on the GPU of fewer than 2^31 pixels (_check_image on one channel)."""
    if not torch.is_tensor(image):
        raise TypeError('%s takes torch tensors on the GPU (image)' % fn)
    if image.dim() != 3 or image.shape[2] != 3:
        raise ValueError('%s: image must be [H, W, 3] (got %s)' % (fn, tuple(image.shape)))
    _check_image(fn, 'image', image[:, :, 0], (torch.uint8,))


def _check_planes(planes):
    """The bit mask of a sequence of distinct stain indices in ascending order."""
    try:
        idx = [operator.index(s) for s in planes]
    except TypeError:
        raise ValueError('planes must be a sequence of stain indices 0..2 (got %r)' % (planes,))
    if not idx or any(s not in (0, 1, 2) for s in idx) or any(a >= b for a, b in zip(idx, idx[1:])):
        raise ValueError('planes must be distinct stain indices 0..2 in ascending order, at least one (got %r)' % (planes,))
    return sum(1 << s for s in idx)


def _check_radius(radius):
    try:
        radius = operator.index(radius)
    except TypeError:
        raise ValueError('radius must be an integer in 0..%d (got %r)' % (kernels.SMOOTH_MAX_RADIUS, radius))
    if not 0 <= radius <= kernels.SMOOTH_MAX_RADIUS:
        raise ValueError('radius must be an integer in 0..%d (got %r)' % (kernels.SMOOTH_MAX_RADIUS, radius))
    return radius


def separate_stains(image, stains=None, order='bgr', planes=(0, 1, 2)):
    """Colour deconvolution (Ruifrok and Johnston 2001) of a stained tile.  image: uint8 [H, W, 3] tensor on the GPU, any strides;
    ``order``: 'bgr' (cv2, bgr_to_gray) or 'rgb'; ``stains``: as stain_matrix (None: haematoxylin, eosin, residual); ``planes``: the
    wanted stains, distinct indices in ascending order.  Returns uint8 [len(planes), H, W]: the concentration of each wanted stain in
    levels of 1 / 64 of a natural-log unit, clamped to [0, 255] -- a dark nucleus of concentration 2.1 lands at 134.  Fixed-point
    arithmetic with a stated contract (kernels.KernelSpec.stain_separate): the result is exact, a pure function of the input, and
    within one level of the float64 formula.

    Host syncs: none."""
    _check_color('separate_stains', image)
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    mask = _check_planes(planes)
    m = stain_matrix(stains)
    with torch.cuda.device(image.device):
        return kernels.get().stain_separate(image, STAIN_ORDERS[order], OD_LUT, m.tolist(), mask)


def _check_gray(fn, image, within):
    _check_image(fn, 'image', image, (torch.uint8,))
    _check_within(fn, within, image)


def histogram(image, within=None):
    """The 256-bin histogram of a uint8 [H, W] tensor on the GPU (any strides; other dtypes are a TypeError): int64 [256] on the
    device, hist[v] = the number of pixels of value v -- with ``within`` (bool / integer, same shape and device) only those where
    ``within`` is non-zero.

    Host syncs: none."""
    _check_gray('histogram', image, within)
    with torch.cuda.device(image.device):
        return kernels.get().histogram_u8(image, within).to(torch.int64)


def _otsu(counts):
    """Otsu's threshold of 256 counts, in Python integers: the t in 0..254 with 0 < w0(t) < N that maximises the between-class
    variance (w0 S - N s0)^2 / (w0 (N - w0)), compared as exact fractions; ties go to the smallest t."""
    h = [int(c) for c in counts]
    N = sum(h)
    if N == 0:
        return 0
    S = sum(v * c for v, c in enumerate(h))
    best, bn, bd = None, 0, 1
    w0 = s0 = 0
    for t in range(255):
        w0 += h[t]
        s0 += t * h[t]
        if 0 < w0 < N:
            num, den = (w0 * S - N * s0) ** 2, w0 * (N - w0)
            if best is None or num * bd > bn * den:
                best, bn, bd = t, num, den
    if best is None:                        # one value only: no t separates anything
        return max(v for v, c in enumerate(h) if c)
    return best


def otsu_threshold(image, within=None):
    """Otsu's global threshold of a uint8 [H, W] tensor on the GPU (``within``: as histogram): the integer t for which ``image > t``
    is the foreground.  With h the histogram, N = sum h, S = sum v h[v], w0(t) = sum_{v <= t} h[v] and s0(t) = sum_{v <= t} v h[v], it
    is the t in 0..254 with 0 < w0 < N that maximises (w0 S - N s0)^2 / (w0 (N - w0)) -- N^2 times the between-class variance.  The
    comparison is made in Python integers as exact fractions (the numerator reaches 2^140: float64 would not define the result); ties
    go to the smallest t, as skimage's first argmax.  A selection of one value returns that value (nothing is foreground), an empty
    selection 0.

    Host syncs: one, the read of the 256 counts."""
    return _otsu(histogram(image, within).tolist())


def smooth(image, radius):
    """Binomial smoothing of a uint8 [H, W] tensor on the GPU (any strides): weights C(2 r, k) along each axis, the border replicated,
    one rounding at the end (kernels.KernelSpec.binomial_smooth).  ``radius`` r: an integer in 0..5; 0 copies, 5 has standard deviation
    1.58; larger blurs are repeated calls.  Returns uint8 [H, W].

    Host syncs: none."""
    _check_image('smooth', 'image', image, (torch.uint8,))
    radius = _check_radius(radius)
    with torch.cuda.device(image.device):
        return kernels.get().binomial_smooth(image, radius)


RESAMPLE_MAX_SIDE = kernels.RESAMPLE_MAX_SIDE                       # largest side of resize / resize_labels, source and output
RESAMPLE_LABELS_MAX_FACTOR = kernels.RESAMPLE_LABELS_MAX_FACTOR     # largest shrink per axis and call of resize_labels(..., 'majority')


def _check_u8_image(fn, image):
    """A uint8 plane [H, W] or tile [H, W, 3] on the GPU."""
    if torch.is_tensor(image) and image.dim() == 3:
        _check_color(fn, image)
    else:
        _check_image(fn, 'image', image, (torch.uint8,))


def resize(image, size, mode='linear'):
    """A uint8 [H, W] plane or uint8 [H, W, 3] tile on the GPU (any strides) at another pixel size: ``size`` = (H2, W2), every side in
    1..32767.  ``mode`` 'linear': exact rational bilinear interpolation with pixel centres at half-integers, the border replicated, one
    rounding (half up) -- no prefiltering, so it aliases below half size; 'area': the exact mean over the source box of every output
    pixel, pixels weighted by their overlap (shrinking only; for integer factors the rounded block mean).  The channels of a tile are
    resampled independently.  Returns a contiguous uint8 tensor of the new size; ``size == image.shape[:2]`` returns an equal copy.  The
    contract item by item: kernels.KernelSpec.resample_u8.  ``nucleus_features(L, resize(gray, L.shape))`` is the reference's
    dataflow/construct_feature_graph.py:61.

    Host syncs: none."""
    _check_u8_image('resize', image)
    kernels.HipKernels._check_resample('resize', image.shape, size, mode, kernels.RESAMPLE_MODES)
    with torch.cuda.device(image.device):
        return kernels.get().resample_u8(image, size, mode)


def resize_labels(labels, size, mode='nearest'):
    """A bool or integer [H, W] label image on the GPU (any strides) at another pixel size: ``size`` = (H2, W2), every side in 1..32767.
    ``mode`` 'nearest': every output pixel copies the source pixel under its centre (integer upscaling is np.repeat on both axes);
    'majority': it takes the value that covers most of its source box, 0 included, ties to the smallest value -- shrinking only, by at
    most 8 per axis and call.  Returns the input's dtype, contiguous; every output value is one of the input's.  The contract item by
    item: kernels.KernelSpec.resample_labels.  Labels keep their values, so ``max_label`` and ``kept_labels`` stay valid; a nucleus
    thinner than the new pixel can vanish.

    Host syncs: none."""
    _check_image('resize_labels', 'labels', labels)
    kernels.HipKernels._check_resample('resize_labels', labels.shape, size, mode, kernels.RESAMPLE_LABEL_MODES)
    with torch.cuda.device(labels.device):
        return kernels.get().resample_labels(labels, size, mode)


def _exact_factor(fn, f):
    if isinstance(f, bool) or not isinstance(f, (int, Fraction, float)):
        raise TypeError('%s: factor must be an int, a Fraction, a float or a pair (fy, fx) of those, got %r' % (fn, f))
    if isinstance(f, float) and not math.isfinite(f):
        raise ValueError('%s: factor must be finite, got %r' % (fn, f))
    f = Fraction(f)                      # a float is taken as the exact binary fraction it holds
    if f <= 0:
        raise ValueError('%s: factor must be positive, got %r' % (fn, f))
    return f


def _scaled_size(shape, factor, fn='rescale'):
    """The size rescale / rescale_labels give an image of ``shape``: per axis max(1, floor(n * f + 1/2)), in exact fractions."""
    fy, fx = factor if isinstance(factor, (tuple, list)) and len(factor) == 2 else (factor, factor)
    return tuple(max(1, math.floor(int(n) * _exact_factor(fn, f) + Fraction(1, 2))) for n, f in zip(shape[:2], (fy, fx)))


def rescale(image, factor, mode='linear'):
    """resize(image, size, mode) with size = max(1, floor(n * factor + 1/2)) per axis, computed in exact fractions.  ``factor``: an int,
    a Fraction, a pair (fy, fx) of those, or a float taken as its exact Fraction.
    ``normalize_stains(rescale(tile, Fraction(1, 2), 'area'))`` is a 40x tile at 20x.

    Host syncs: none."""
    _check_u8_image('rescale', image)
    return resize(image, _scaled_size(image.shape, factor, 'rescale'), mode)


def rescale_labels(labels, factor, mode='nearest'):
    """resize_labels(labels, size, mode) with rescale's size rule.

    Host syncs: none."""
    _check_image('rescale_labels', 'labels', labels)
    return resize_labels(labels, _scaled_size(labels.shape, factor, 'rescale_labels'), mode)


def scale_points(points, from_size, to_size):
    """Float [N, 2] (row, column) coordinates, such as centroids, from a raster of ``from_size`` = (H, W) to the same image at
    ``to_size`` = (H2, W2), under the pixel-centre convention of resize: c2 = (c + 1/2) * n2 / n - 1/2 per axis, computed in float64
    and returned in the input's dtype.  Plain torch, on whatever device the points live; scale_points(., b, a) inverts
    scale_points(., a, b).

    Host syncs: none."""
    if not torch.is_tensor(points) or not points.is_floating_point():
        raise TypeError('scale_points takes a float tensor [N, 2] (points)')
    if points.dim() != 2 or points.shape[1] != 2:
        raise ValueError('scale_points: points must be [N, 2] (got %s)' % (tuple(points.shape),))
    sizes = []
    for name, size in (('from_size', from_size), ('to_size', to_size)):
        try:
            h, w = (operator.index(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError('scale_points: %s must be a pair of integers, got %r' % (name, size))
        if h < 1 or w < 1:
            raise ValueError('scale_points: %s must be positive, got %r' % (name, size))
        sizes.append((h, w))
    n, n2 = (torch.tensor(v, dtype=torch.float64, device=points.device) for v in sizes)
    return ((points.to(torch.float64) + 0.5) * n2 / n - 0.5).to(points.dtype)


def stain_foreground(image, stain=0, radius=2, stains=None, order='bgr', within=None):
    """From a stained tile to a foreground map: plane = smooth(separate_stains(image, stains, order, (stain,))[0], radius),
    t = otsu_threshold(plane, within), fg = plane > t.  image: uint8 [H, W, 3] on the GPU; ``stain``: 0 haematoxylin (the nuclei),
    1 eosin, 2 residual, of ``stains``; ``within`` (bool / integer [H, W]): the pixels the threshold is taken over, e.g. a tissue
    mask -- fg is still defined everywhere.  Returns (fg bool [H, W], t, plane uint8 [H, W]).  ``stains``: as stain_matrix -- None
    for the fixed DEFAULT_STAINS, or the tile's own vectors: stain_foreground(image, stains=estimate_stains(image)).

    The stage behind it:
        L, n = split_touching(fill_holes(fg), None, markers='h_maxima', growth='flood', h=2.0)
        features, centroids, kept = nucleus_features(L, bgr_to_gray(image), max_label=n)

    With normalisation in front (normalize_stains), ``TARGET_STAINS + residual`` standing for the two target rows plus their cross
    product:
        norm = normalize_stains(tile)
        fg, t, plane = stain_foreground(norm, stains=TARGET_STAINS + residual)
        ...
        nucleus_features(L, bgr_to_gray(norm), max_label=n)

    Host syncs: one, that of otsu_threshold."""
    _check_color('stain_foreground', image)
    _check_planes((stain,))
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    radius = _check_radius(radius)
    _check_within('stain_foreground', within, image[:, :, 0])
    plane = smooth(separate_stains(image, stains, order, (int(stain),))[0], radius)
    t = otsu_threshold(plane, within)
    return plane > t, t, plane


def _check_int_in(name, value, lo, hi):
    if isinstance(value, bool):
        raise ValueError('%s must be an integer in %d..%d (got %r)' % (name, lo, hi, value))
    try:
        value = operator.index(value)
    except TypeError:
        raise ValueError('%s must be an integer in %d..%d (got %r)' % (name, lo, hi, value))
    if not lo <= value <= hi:
        raise ValueError('%s must be an integer in %d..%d (got %r)' % (name, lo, hi, value))
    return value


def _check_window(window):
    return _check_int_in('the window radius', window, 0, kernels.WINDOW_MAX_RADIUS)


def window_sums(image, radius, within=None):
    """Count, sum and sum of squares of the pixels around every pixel of a uint8 [H, W] tensor on the GPU (any strides; other dtypes
    are a TypeError): the window of (y, x) is rows y - radius .. y + radius and columns x - radius .. x + radius, clipped to the image
    -- nothing is replicated, border windows are smaller -- and ``radius`` is an integer in 0..127.  With ``within`` (bool / integer,
    same shape and device) only the pixels where it is non-zero count, which a stock box filter cannot give: statistics over tissue
    only.  Returns (n int32, S int32, Q int64), each [H, W]: mean = S / n, variance = Q / n - mean^2 wherever n > 0
    (kernels.KernelSpec.window_sums).  A ``within`` that selects nothing gives zeros, an empty image empty outputs.

    Host syncs: none."""
    _check_gray('window_sums', image, within)
    radius = _check_window(radius)
    with torch.cuda.device(image.device):
        return kernels.get().window_sums(image, radius, within)


def niblack_k64(k):
    """The integer the local rule uses for a real k: floor(64 k + 1/2), computed exactly (``Fraction``), in -128..128 -- k = 0.2 is
    13 / 64 = 0.203.  ValueError for a bool, a value that is not a real number, a non-finite one, or a result out of range."""
    if isinstance(k, bool) or not isinstance(k, numbers.Real):
        raise ValueError('k must be a real number (got %r)' % (k,))
    try:
        exact = k if isinstance(k, numbers.Rational) else float(k)      # numpy scalars and the like: their exact value as a float
        if isinstance(exact, float) and not math.isfinite(exact):
            raise ValueError
        k64 = math.floor(Fraction(exact) * 64 + Fraction(1, 2))
    except (TypeError, ValueError, OverflowError):
        raise ValueError('k must be a finite real number (got %r)' % (k,))
    if not -128 <= k64 <= 128:
        raise ValueError('k must lie in -2..2 (got %r)' % (k,))
    return k64


def local_threshold(image, radius, k=0.0, offset=0, floor=None, within=None):
    """The local mean / Niblack threshold of a uint8 [H, W] tensor on the GPU (any strides): a pixel of value v is foreground iff
    v > m + k s + offset, with m and s the mean and the standard deviation of the window of ``radius`` (0..127) around it, clipped to
    the image and, with ``within``, taken over its non-zero pixels only (a pixel outside ``within`` is still decided, from the counted
    pixels of its window; where none is counted it is background).  ``k``: a real number in -2..2, used as niblack_k64(k) / 64; k = 0
    is the local mean rule, Niblack's text binarisation uses k < 0, bright objects on a varying background k >= 0 with an ``offset``
    (an integer in -255..255) of about half their contrast.  ``floor``: None or an integer in 0..255 -- also require v > floor.
    Returns bool [H, W].  The decision is made in exact integers (kernels.KernelSpec.local_threshold): the map is a pure function of
    its inputs, and a pixel that sits exactly on the rule is background.

    Host syncs: none."""
    _check_gray('local_threshold', image, within)
    radius = _check_window(radius)
    k64 = niblack_k64(k)
    offset = _check_int_in('offset', offset, -255, 255)
    floor = -1 if floor is None else _check_int_in('floor', floor, 0, 255)
    with torch.cuda.device(image.device):
        return kernels.get().local_threshold(image, radius, k64, offset, floor, within).view(torch.bool)


def local_stain_foreground(image, window, stain=0, radius=2, stains=None, order='bgr', within=None, k=0.0, offset=0, floor=None):
    """stain_foreground with a local threshold: plane = smooth(separate_stains(image, stains, order, (stain,))[0], radius) exactly as
    there, fg = local_threshold(plane, window, k, offset, floor, within).  ``window``: the radius of the statistics' window, 0..127 --
    a few nucleus diameters; ``k``, ``offset``, ``within``: as local_threshold.  ``floor``: None, an integer in 0..255, or 'otsu':
    the floor is otsu_threshold(plane, within), so that the local rule only removes pixels from the global foreground.  Returns
    (fg bool [H, W], the floor used or None, plane uint8 [H, W]); fg goes where stain_foreground's goes:
        L, n = split_touching(fill_holes(fg), None, markers='h_maxima', growth='flood', h=2.0)

    Host syncs: none; one, that of otsu_threshold, with floor='otsu'."""
    _check_color('local_stain_foreground', image)
    _check_planes((stain,))
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    radius = _check_radius(radius)
    window = _check_window(window)
    _check_within('local_stain_foreground', within, image[:, :, 0])
    niblack_k64(k)
    _check_int_in('offset', offset, -255, 255)
    if floor is not None and not (isinstance(floor, str) and floor == 'otsu'):
        floor = _check_int_in('floor', floor, 0, 255)
    plane = smooth(separate_stains(image, stains, order, (int(stain),))[0], radius)
    if floor == 'otsu':
        floor = otsu_threshold(plane, within)
    return local_threshold(plane, window, k, offset, floor, within), floor, plane


MORPH_MAX_RADIUS = kernels.MORPH_MAX_RADIUS
MORPH_FOOTPRINTS = tuple(kernels.MORPH_KINDS)


def _check_flat(fn, image, radius, footprint, within, top=MORPH_MAX_RADIUS):
    """The refusals the flat-morphology functions and the rank filters share, before any launch (``top``: the largest radius):
    returns (the image as uint8 -- a bool image as 0 / 1, without a copy --, radius as an int)."""
    _check_image(fn, 'image', image, (torch.bool, torch.uint8))
    _check_within(fn, within, image)
    radius = _check_int_in('radius', radius, 0, top)
    if not isinstance(footprint, str) or footprint not in kernels.MORPH_KINDS:
        raise ValueError("footprint must be 'disk', 'square' or 'diamond', got %r" % (footprint,))
    return (image.view(torch.uint8) if image.dtype == torch.bool else image), radius


def _morph(x, footprint, radius, op, within, other=None, epilogue=None):
    with torch.cuda.device(x.device):
        return kernels.get().flat_morphology(x, footprint, radius, op, within, other, epilogue)


def erode(image, radius, footprint='disk', within=None):
    """Grey-scale erosion of a uint8 or bool [H, W] tensor on the GPU (any strides) by a flat structuring element: every pixel becomes
    the minimum over its footprint.  ``footprint``: 'disk' (dx^2 + dy^2 <= radius^2, skimage's disk), 'square' (side 2 radius + 1) or
    'diamond' (|dx| + |dy| <= radius); ``radius``: an integer in 0..63, 0 being the single pixel.  The footprint is clipped to the
    image -- nothing is replicated, so the border never lowers a value -- and with ``within`` (bool / integer, same shape and device)
    only the pixels where it is non-zero count; where none counts the result is 255, the neutral value (True for a bool image).  A bool
    image counts as 0 / 1 and gives a bool result: binary erosion.  Other dtypes are a TypeError; int32 images are out of scope.
    Exact, one launch (kernels.KernelSpec.flat_morphology).

    Host syncs: none."""
    x, radius = _check_flat('erode', image, radius, footprint, within)
    out = _morph(x, footprint, radius, 'erode', within)
    return out != 0 if image.dtype == torch.bool else out


def dilate(image, radius, footprint='disk', within=None):
    """Grey-scale dilation: every pixel becomes the maximum over its footprint; image, radius, footprint, within and the result as
    erode.  Where no pixel counts the result is 0.  dilate(x) == 255 - erode(255 - x).

    Host syncs: none."""
    x, radius = _check_flat('dilate', image, radius, footprint, within)
    out = _morph(x, footprint, radius, 'dilate', within)
    return out != 0 if image.dtype == torch.bool else out


def opening(image, radius, footprint='disk', within=None):
    """dilate(erode(image)): removes bright structures that the footprint does not fit into and leaves the rest as it was; never above
    the image, idempotent.  Arguments and result as erode; a bool image is computed as 0 / 1 and converted at the end.  Two launches.

    Host syncs: none."""
    x, radius = _check_flat('opening', image, radius, footprint, within)
    out = _morph(_morph(x, footprint, radius, 'erode', within), footprint, radius, 'dilate', within)
    return out != 0 if image.dtype == torch.bool else out


def closing(image, radius, footprint='disk', within=None):
    """erode(dilate(image)): fills dark gaps that the footprint does not fit into; never below the image, idempotent.  Arguments and
    result as erode.  Two launches.

    Host syncs: none."""
    x, radius = _check_flat('closing', image, radius, footprint, within)
    out = _morph(_morph(x, footprint, radius, 'dilate', within), footprint, radius, 'erode', within)
    return out != 0 if image.dtype == torch.bool else out


def white_tophat(image, radius, footprint='disk', within=None):
    """image - opening(image): what the opening removed -- bright structures smaller than the footprint on a flattened background.
    The standard correction for an unevenly stained tile in front of ``otsu_threshold``.  Arguments as erode; returns uint8 [H, W] (a
    bool image counts as 0 / 1).  Two launches: the subtraction is fused into the dilation, clamped at 0 (without ``within`` the
    opening is never above the image and the clamp never acts).

    Host syncs: none."""
    x, radius = _check_flat('white_tophat', image, radius, footprint, within)
    return _morph(_morph(x, footprint, radius, 'erode', within), footprint, radius, 'dilate', within, x, 'other_minus')


def black_tophat(image, radius, footprint='disk', within=None):
    """closing(image) - image: dark structures smaller than the footprint.  Arguments and result as white_tophat.  Two launches.

    Host syncs: none."""
    x, radius = _check_flat('black_tophat', image, radius, footprint, within)
    return _morph(_morph(x, footprint, radius, 'dilate', within), footprint, radius, 'erode', within, x, 'minus_other')


def morph_gradient(image, radius, footprint='disk', within=None):
    """The morphological gradient dilate(image) - erode(image): the local contrast, large on edges -- a height image for
    ``watershed`` that puts the cut on the stain edge.  Arguments as erode; returns uint8 [H, W]; 0 where no pixel counts.  ONE
    launch: both extrema are found in the same pass.

    Host syncs: none."""
    x, radius = _check_flat('morph_gradient', image, radius, footprint, within)
    return _morph(x, footprint, radius, 'gradient', within)


def open_by_reconstruction(image, radius, footprint='disk', connectivity=1, within=None):
    """reconstruct(erode(image, radius, footprint, within), image, 'dilation', connectivity): like opening it removes what the
    footprint does not fit into, but what survives the erosion gets its exact shape back.  opening <= open_by_reconstruction <= image.
    image, radius, footprint, within: as erode; connectivity: as reconstruct.  Returns the image's dtype.

    Host syncs: those of reconstruct."""
    _check_flat('open_by_reconstruction', image, radius, footprint, within)
    _check_connectivity(connectivity)
    return reconstruct(erode(image, radius, footprint, within), image, 'dilation', connectivity)


def close_by_reconstruction(image, radius, footprint='disk', connectivity=1, within=None):
    """The dual: reconstruct(dilate(image, radius, footprint, within), image, 'erosion', connectivity).
    image <= close_by_reconstruction <= closing.  Arguments and result as open_by_reconstruction.

    Host syncs: those of reconstruct."""
    _check_flat('close_by_reconstruction', image, radius, footprint, within)
    _check_connectivity(connectivity)
    return reconstruct(dilate(image, radius, footprint, within), image, 'erosion', connectivity)


RANK_MAX_RADIUS = kernels.RANK_MAX_RADIUS
ENTROPY_MAX_RADIUS = kernels.ENTROPY_MAX_RADIUS


def rank_q10k(q):
    """The integer the rank filters use for a quantile q in [0, 1]: the nearest integer to 10000 q, decided exactly (``Fraction``),
    halves rounding up -- 0.5 is 5000, 0.05 is 500, Fraction(1, 3) is 3333.  ``q``: an int, float or Fraction.  ValueError for a bool,
    a value that is not a real number, NaN, or anything outside [0, 1]."""
    if isinstance(q, bool) or not isinstance(q, numbers.Real):
        raise ValueError('q must be a real number in [0, 1] (got %r)' % (q,))
    try:
        exact = q if isinstance(q, numbers.Rational) else float(q)      # numpy scalars and the like: their exact value as a float
        if isinstance(exact, float) and not math.isfinite(exact):
            raise ValueError
        q10k = math.floor(Fraction(exact) * 10000 + Fraction(1, 2))
    except (TypeError, ValueError, OverflowError):
        raise ValueError('q must be a finite real number in [0, 1] (got %r)' % (q,))
    if not 0 <= Fraction(exact) <= 1:
        raise ValueError('q must lie in [0, 1] (got %r)' % (q,))
    return q10k


def _rank(x, footprint, radius, op, q_lo, q_hi, within):
    with torch.cuda.device(x.device):
        return kernels.get().rank_filter(x, footprint, radius, op, q_lo, q_hi, within)


def rank_filter(image, radius, q, footprint='disk', within=None):
    """The q-quantile of every window of a uint8 or bool [H, W] tensor on the GPU (any strides): with n the number of counted pixels of
    the window and v[0] <= ... <= v[n-1] their values sorted, the result is v[min(n - 1, floor(n * q10k / 10000))], q10k =
    rank_q10k(q) -- q = 0 is erode, 1 is dilate, 1/2 the median (the upper one when n is even); 0.05 and 0.95 are the erode and dilate
    that one hot pixel does not decide.  ``radius`` (0..63), ``footprint`` and ``within`` as erode: the footprint is clipped to the
    image, and with ``within`` only its non-zero pixels count; where none counts the result is 0 (False).  A bool image counts as
    0 / 1 and gives a bool result.  Exact integers, one launch (kernels.KernelSpec.rank_filter).

    Host syncs: none."""
    x, radius = _check_flat('rank_filter', image, radius, footprint, within, RANK_MAX_RADIUS)
    out = _rank(x, footprint, radius, 'quantile', 0, rank_q10k(q), within)
    return out != 0 if image.dtype == torch.bool else out


def median(image, radius, footprint='disk', within=None):
    """rank_filter(image, radius, 1/2): the median filter, the edge-preserving denoiser in front of a threshold -- it removes bright
    and dark specks smaller than half the footprint and leaves a step edge where it is.  With an even count the upper median is
    taken.  On a bool mask it is the majority filter: True iff at least half of the counted pixels are True -- a tie gives True,
    and a window in which nothing is counted gives False.  Arguments and result as rank_filter.

    Host syncs: none."""
    x, radius = _check_flat('median', image, radius, footprint, within, RANK_MAX_RADIUS)
    out = _rank(x, footprint, radius, 'quantile', 0, 5000, within)
    return out != 0 if image.dtype == torch.bool else out


def quantile_range(image, radius, q_lo, q_hi, footprint='disk', within=None):
    """The q_hi-quantile minus the q_lo-quantile of every window (q_lo <= q_hi, both as rank_filter's q; ValueError otherwise), both
    read off one histogram in ONE launch: the robust local contrast -- quantile_range(x, r, 0, 1) is morph_gradient(x, r), and
    (0.05, 0.95) is the gradient that a single hot or dead pixel does not decide.  Arguments as rank_filter; returns uint8 [H, W] (a
    bool image counts as 0 / 1), 0 where no pixel counts.

    Host syncs: none."""
    x, radius = _check_flat('quantile_range', image, radius, footprint, within, RANK_MAX_RADIUS)
    lo, hi = rank_q10k(q_lo), rank_q10k(q_hi)
    if lo > hi:
        raise ValueError('q_lo <= q_hi (got %r > %r)' % (q_lo, q_hi))
    return _rank(x, footprint, radius, 'range', lo, hi, within)


def local_entropy(image, radius=3, footprint='disk', within=None, raw=False):
    """The Shannon entropy, in bits, of the values under every window: skimage.filters.rank.entropy(image, disk(radius)), with the
    footprint clipped to the image -- 0 on a flat region, log2(n) where all n pixels differ; a texture map to threshold or to flood.
    ``radius``: an integer in 0..15; ``footprint`` and ``within`` as rank_filter (where no pixel counts the result is 0).  Computed
    in integers from a table of c log2 c terms (kernels.KernelSpec.rank_filter, item 7): the result is H16 / 65536 as float32 -- exact,
    H16 < 2^24 -- with |H16 / 65536 - H| <= 2^-15, or, with ``raw=True``, the int32 H16 itself.  One launch; a pure function of its
    inputs.

    Host syncs: none."""
    x, radius = _check_flat('local_entropy', image, radius, footprint, within, ENTROPY_MAX_RADIUS)
    h16 = _rank(x, footprint, radius, 'entropy', 0, 0, within)
    return h16 if raw else h16.to(torch.float32) / 65536.0


def _od_min(beta):
    """The smallest integer k with k / 1024 >= beta (exact: beta as a Fraction)."""
    if isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not 0 <= beta <= Fraction(kernels.STAIN_OD_MAX, 1024):
        raise ValueError('beta must be a number with 0 <= beta <= %d/1024 (got %r)' % (kernels.STAIN_OD_MAX, beta))
    return int(math.ceil(Fraction(beta) * 1024))


def _percentile_bins(bins, alpha):
    """(b_lo, b_hi) of item 4 of estimate_stains, in exact arithmetic; sum(bins) > 0."""
    a, M = Fraction(alpha), sum(bins)
    b_lo = b_hi = None
    cum = 0
    for b, c in enumerate(bins):
        cum += c
        if b_lo is None and cum >= 1 and 100 * cum >= a * M:
            b_lo = b
        if b_hi is None and 100 * cum >= (100 - a) * M:
            b_hi = b
            break
    return b_lo, b_hi


def _plane_of_moments(mom):
    """Item 2 of estimate_stains: (n, eigenvalues ascending, e_1, e_2) of the ten integer moments."""
    n, s, q = mom[0], mom[1:4], mom[4:]
    if n < 2:
        raise ValueError('estimate_stains: too few stained pixels (%d): lower beta or widen within' % n)
    q = ((q[0], q[1], q[2]), (q[1], q[3], q[4]), (q[2], q[4], q[5]))
    C = np.array([[float(n * q[i][j] - s[i] * s[j]) for j in range(3)] for i in range(3)], np.float64)      # exact integers, then rounded once
    lam, vec = np.linalg.eigh(C)
    if not np.isfinite(lam[1]) or not lam[1] > 0:
        raise ValueError('estimate_stains: the optical densities of the stained pixels lie on one line (one stain only): no plane')
    e1, e2 = vec[:, 2].copy(), vec[:, 1].copy()
    if e1.sum() < 0:
        e1 = -e1
    if e2[int(np.argmax(np.abs(e2)))] < 0:
        e2 = -e2
    return n, lam, e1, e2


def _stains_of_bins(e1, e2, b_lo, b_hi):
    """Item 5 of estimate_stains: the unit vectors of haematoxylin, eosin and the residual from the two percentile bins."""
    v = []
    for b in (b_lo, b_hi):
        phi = -0.5 * math.pi + (b + 0.5) * math.pi / ANGLE_BINS
        v.append(e1 * math.cos(phi) + e2 * math.sin(phi))
    h, e = (v[0], v[1]) if v[0][0] > v[1][0] else (v[1], v[0])
    S = np.stack([h, e, np.cross(h, e)])
    norm = np.sqrt((S * S).sum(axis=1))
    if not (norm > 0).all():
        stain_matrix(S)                    # both percentiles in one bin: no residual; stain_matrix words the refusal
    return S / norm[:, None]


def estimate_stains(image, order='bgr', beta=0.15, alpha=1.0, within=None, return_info=False):
    """A tile's own stain vectors by Macenko's method (Macenko et al. 2009), for stain_matrix, separate_stains and stain_foreground:
    numpy float64 [3, 3], the rows the unit optical-density vectors (R, G, B) of haematoxylin, eosin and a residual.  image: uint8
    [H, W, 3] on the GPU, any strides; ``order``: 'bgr' or 'rgb'; ``within`` (bool / integer [H, W]): the pixels that may be used, e.g.
    a tissue mask.  The two passes over the tile are integer reductions with a stated contract (kernels.KernelSpec.od_moments,
    angle_histogram), so the result is a pure function of the tile, of numpy's ``eigh`` and of the platform's cos and sin.

    1.  od_min = the smallest integer k with k / 1024 >= beta (154 for 0.15): a pixel counts as stained when the optical densities
        OD_LUT[.] of all three channels reach od_min.  ``beta`` must be a number with 0 <= beta <= 5674/1024 and ``alpha`` one with
        0 <= alpha < 50 (ValueError otherwise).
    2.  The ten moments n, s_i, q_ij of the stained pixels are read (host sync 1).  n < 2 raises ValueError ("too few stained
        pixels").  In Python integers C[i][j] = n q_ij - s_i s_j, exactly n (n - 1) times the covariance; C goes to float64 and to
        numpy.linalg.eigh.  e_1 = the eigenvector of the largest eigenvalue, its sign such that its components sum to a positive
        number; e_2 = that of the second largest, its sign such that its component of largest magnitude is positive.  A second
        eigenvalue <= 0 or not finite raises ValueError: one stain only, no plane.
    3.  E[j][c] = rint(4096 e_j[c]); angle_histogram bins every stained pixel by the angle of its projection (p_1, p_2) on that plane
        into K = 1024 bins of (-pi/2, pi/2), and the K + 1 counts are read (host sync 2).  M = the sum of the K bins; M = 0 raises
        ValueError.  Pixels with p_1 <= 0 are not binned but counted (``skipped``).
    4.  With a = Fraction(alpha) and cum(b) the running sum of the bins, in exact arithmetic: b_lo = the smallest b with cum(b) >= 1
        and 100 cum(b) >= a M; b_hi = the smallest b with 100 cum(b) >= (100 - a) M.  phi = -pi/2 + (b + 1/2) pi / K, the bin's centre.
    5.  v_lo = e_1 cos phi_lo + e_2 sin phi_lo and v_hi likewise, from the float64 eigenvectors.  The one with the larger R component
        is haematoxylin, the other eosin, their cross product the residual; all three are normalised.  If stain_matrix would refuse
        the result its ValueError is raised.
    6.  ``return_info``: also a dict with n, skipped, od_min, bins = (b_lo, b_hi) and eigenvalues = the three eigenvalues of C in
        ascending order, each divided by n (n - 1) -- those of the covariance of the optical densities in units of 1/1024.

        S = estimate_stains(tile)
        fg, t, plane = stain_foreground(tile, stains=S)

    Host syncs: two, the read of the ten moments and the read of the K + 1 counts."""
    _check_color('estimate_stains', image)
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    od_min = _od_min(beta)
    _check_alpha(alpha)
    _check_within('estimate_stains', within, image[:, :, 0])
    if image.shape[0] * image.shape[1] == 0:
        raise ValueError('estimate_stains: too few stained pixels (0): the image is empty')
    with torch.cuda.device(image.device):
        table = kernels.get()
        mom = table.od_moments(image, STAIN_ORDERS[order], OD_LUT, od_min, within).tolist()
        n, lam, e1, e2 = _plane_of_moments(mom)
        basis = [[int(v) for v in np.rint(4096.0 * e)] for e in (e1, e2)]
        counts = table.angle_histogram(image, STAIN_ORDERS[order], OD_LUT, od_min, basis, ANGLE_DIRS, within).tolist()
    bins, skipped = counts[:ANGLE_BINS], counts[ANGLE_BINS]
    if sum(bins) == 0:
        raise ValueError('estimate_stains: no stained pixel lies on the positive side of the first principal direction')
    b_lo, b_hi = _percentile_bins(bins, alpha)
    S = _stains_of_bins(e1, e2, b_lo, b_hi)
    stain_matrix(S)                        # its refusals are this function's
    if return_info:
        return S, dict(n=n, skipped=skipped, od_min=od_min, bins=(b_lo, b_hi), eigenvalues=tuple(float(v) / (n * (n - 1)) for v in lam))
    return S


def _check_alpha(alpha):
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not 0 <= alpha < 50:
        raise ValueError('alpha must be a number with 0 <= alpha < 50 (got %r)' % (alpha,))


def _top_bin(bins, alpha):
    """The bin of stain_maxima's rule, in exact arithmetic as _percentile_bins: the smallest b with cum(b) >= 1 and
    100 cum(b) >= (100 - alpha) n; sum(bins) = n > 0."""
    a, n = Fraction(alpha), sum(bins)
    cum = 0
    for b, c in enumerate(bins):
        cum += c
        if cum >= 1 and 100 * cum >= (100 - a) * n:
            return b


def _stain_maxima(image, stains, order, alpha, beta, within):
    """stain_maxima behind its checks: (maxima, bins, n)."""
    _check_color('stain_maxima', image)
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    _check_alpha(alpha)
    od_min = _od_min(beta)
    _check_within('stain_maxima', within, image[:, :, 0])
    m = stain_matrix(stains)
    if image.shape[0] * image.shape[1] == 0:
        raise ValueError('stain_maxima: no stained pixel (0): the image is empty')
    with torch.cuda.device(image.device):
        counts = kernels.get().concentration_histogram(image, STAIN_ORDERS[order], OD_LUT, od_min, m.tolist(), within).tolist()
    halves = counts[:CONC_BINS], counts[CONC_BINS:]
    n = sum(halves[0])
    if n == 0:
        raise ValueError('stain_maxima: no stained pixel (0): lower beta or widen within')
    bins = tuple(_top_bin(h, alpha) for h in halves)
    for s, b in enumerate(bins):
        if b == 0:
            raise ValueError('stain_maxima: the tile has none of stain %d (its robust maximum lies in bin 0)' % s)
        if b == CONC_BINS - 1:
            raise ValueError('stain_maxima: the histogram of stain %d is saturated (its robust maximum lies in the last bin, '
                             '%d/128 and up)' % (s, CONC_BINS - 1))
    return tuple(Fraction(b, 128) for b in bins), bins, n


def stain_maxima(image, stains=None, order='bgr', alpha=1.0, beta=0.15, within=None):
    """The robust maxima of a tile's haematoxylin and eosin concentrations (Macenko et al. 2009), for recolor_matrix: two
    ``Fraction``s in natural-log units.  image: uint8 [H, W, 3] on the GPU, any strides; ``stains``: as stain_matrix (None:
    DEFAULT_STAINS), usually estimate_stains(image); ``order``: 'bgr' or 'rgb'; ``within`` (bool / integer [H, W]): the pixels that
    may be used.  One integer reduction with a stated contract (kernels.KernelSpec.concentration_histogram): the result is a pure
    function of the tile and of stain_matrix(stains).

    1.  od_min from ``beta`` and the selection of the stained pixels: item 1 of estimate_stains.  ``beta`` = 0 selects every pixel
        (of ``within``), which is what the published code does; the default selects the stained pixels, as estimate_stains does.
        0 <= alpha < 50 (ValueError otherwise).
    2.  The concentrations C_0, C_1 of every stained pixel are binned in levels of 1/128 of a unit, 512 bins per stain, the last one
        open, and the 1024 counts are read (the host sync).  n = the sum of either half.  n = 0 raises ValueError.
    3.  In exact arithmetic: b_s = the smallest bin with cum(b) >= 1 and 100 cum(b) >= (100 - alpha) n -- the bin of the
        ceil((100 - alpha) n / 100)-th smallest concentration.  The maximum of stain s is b_s / 128.
    4.  b_s = 0 raises ValueError (the tile has none of that stain), and so does b_s = 511 (the histogram is saturated: 3.99 units
        and up).

    Host syncs: one, the read of the 1024 counts."""
    return _stain_maxima(image, stains, order, alpha, beta, within)[0]


def _unit_rows(fn, name, rows, shapes):
    try:
        R = np.array(rows, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s: %s must be numbers' % (fn, name))
    if R.shape not in shapes:
        raise ValueError('%s: %s must be %s (got shape %s)' % (fn, name, ' or '.join('%d x %d' % sh for sh in shapes), R.shape))
    if not np.isfinite(R).all():
        raise ValueError('%s: %s must be finite' % (fn, name))
    norm = np.sqrt((R * R).sum(axis=1))
    if not (norm > 0).all() or not np.isfinite(norm).all():
        raise ValueError('%s: every row of %s needs a non-zero optical-density vector' % (fn, name))
    return R / norm[:, None]


def _positive_pair(fn, name, pair):
    try:
        v = [float(x) for x in pair]
    except (TypeError, ValueError):
        raise ValueError('%s: %s must be two positive numbers' % (fn, name))
    if len(v) != 2 or not all(math.isfinite(x) and x > 0 for x in v):
        raise ValueError('%s: %s must be two positive finite numbers (got %r)' % (fn, name, pair))
    return v


def recolor_matrix(stains, maxima, target_stains=None, target_max=None):
    """The fixed-point matrix that takes a tile's optical densities to those of the normalised tile: numpy int32 [3, 3],
    a[c][d] = rint(4096 A[c][d]) with c the input and d the output channel (0 R, 1 G, 2 B) and, in float64,
        A = inv(S)[:, :2] diag(target_max_s / maxima_s) T[:2].
    S: the unit-normalised rows of ``stains`` (3 x 3, as stain_matrix); T: the first two unit-normalised rows of ``target_stains``
    (2 x 3 or 3 x 3; None: TARGET_STAINS); ``maxima``: two positive numbers, e.g. stain_maxima's Fractions; ``target_max``: two positive
    numbers (None: TARGET_MAX).  The residual is dropped, as Macenko does: because the residual row of estimate_stains is orthogonal
    to the other two, the first two columns of inv(S) are the least-squares concentrations on the two stains alone.
    ValueError: bad shapes, non-finite or zero rows, dependent stains, non-positive or non-finite maxima or targets, or a matrix
    with sum_c |a[c][d]| * 5674 >= 2^31 - 2^11 for some d (recolor's int32 sum could overflow)."""
    S = _unit_rows('recolor_matrix', 'stains', stains, ((3, 3),))
    stain_matrix(S)                        # its refusals of dependent stains are this function's
    T = _unit_rows('recolor_matrix', 'target_stains', TARGET_STAINS if target_stains is None else target_stains, ((2, 3), (3, 3)))[:2]
    mx = _positive_pair('recolor_matrix', 'maxima', maxima)
    tm = _positive_pair('recolor_matrix', 'target_max', TARGET_MAX if target_max is None else target_max)
    A = np.linalg.inv(S)[:, :2] @ np.diag([tm[0] / mx[0], tm[1] / mx[1]]) @ T
    q = np.rint(4096.0 * A)
    if not np.isfinite(q).all() or (np.abs(q).sum(axis=0) * kernels.STAIN_OD_MAX >= 2 ** 31 - 2 ** 11).any():
        raise ValueError('recolor_matrix: the matrix is too large: the int32 sum of recolor could overflow')
    return q.astype(np.int32)


def recolor(image, a, order='bgr'):
    """A linear map in optical-density space: image uint8 [H, W, 3] on the GPU (any strides) -> uint8 [H, W, 3] in the same channel
    order, out_d = EXP_LUT[clamp((sum_c OD_LUT[v_c] a[c][d] + 2^11) >> 12, 0, 6385)] (kernels.KernelSpec.od_recolor).  ``a``: 3 x 3
    integers, 4096 times the matrix, c the input and d the output channel (0 R, 1 G, 2 B): recolor_matrix's, or
    rint(4096 inv(S)[:, s] T[s]) to render stain s alone.  ValueError: a matrix that is not 3 x 3 integers or that fails
    sum_c |a[c][d]| * 5674 < 2^31 - 2^11.  With a = 4096 I the result is the input except that 0 becomes 1.

    Host syncs: none."""
    _check_color('recolor', image)
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    if isinstance(a, np.ndarray):
        if a.dtype.kind not in 'iu':
            raise ValueError('recolor: the matrix must hold integers (got %s)' % a.dtype)
        a = a.tolist()
    kernels.HipKernels._check_od_matrix('recolor', a, 2 ** 11)
    with torch.cuda.device(image.device):
        return kernels.get().od_recolor(image, STAIN_ORDERS[order], OD_LUT, a, EXP_LUT)


def normalize_stains(image, stains=None, order='bgr', target_stains=None, target_max=None, alpha=1.0, beta=0.15, within=None,
                     return_info=False):
    """Stain normalisation by Macenko's method (Macenko et al. 2009): the tile as it would look with the reference stains at the
    reference strength.  image: uint8 [H, W, 3] on the GPU, any strides; returns uint8 [H, W, 3], contiguous, in the input's channel
    order (``order``: 'bgr' or 'rgb').  ``within`` (bool / integer [H, W]): the pixels the statistics are taken over, e.g. a tissue
    mask -- every pixel is recoloured.  All device arithmetic is integer with a stated contract, so the result is a pure function of
    the tile (and, with ``stains`` = None, of what estimate_stains depends on).

    1.  S = ``stains`` (as stain_matrix), or with None the tile's own vectors estimate_stains(image, order, beta, alpha, within).
    2.  maxima = stain_maxima(image, S, order, alpha, beta, within): the robust maxima b_s / 128 of the two concentrations.
    3.  a = recolor_matrix(S, maxima, target_stains, target_max): rint(4096 inv(S)[:, :2] diag(target_max_s / maxima_s) T[:2]),
        T the reference vectors (None: TARGET_STAINS, TARGET_MAX); the residual is dropped.
    4.  The result is recolor(image, a, order): out_d = EXP_LUT[clamp((sum_c OD_LUT[v_c] a[c][d] + 2^11) >> 12, 0, 6385)].
    5.  Every ValueError of the four steps is this function's: too few stained pixels, one stain only, none of a stain, a saturated
        histogram, bad targets, a matrix that could overflow.
    6.  ``return_info``: also a dict with stains (S as float64 [3, 3], as given or as estimated), maxima (two Fractions), bins = (b_0, b_1), n (the stained
        pixels) and matrix (a, int32 [3, 3]).

        norm = normalize_stains(tile)
        fg, t, plane = stain_foreground(norm, stains=TARGET_STAINS + residual)
        ...
        nucleus_features(L, bgr_to_gray(norm), max_label=n)
    (``TARGET_STAINS + residual``: the two target rows plus their cross product.)

    Host syncs: three -- the two of estimate_stains and the read of the 1024 counts -- or one with given stains."""
    _check_color('normalize_stains', image)
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    _check_alpha(alpha)
    _od_min(beta)
    _check_within('normalize_stains', within, image[:, :, 0])
    T = TARGET_STAINS if target_stains is None else target_stains
    tm = TARGET_MAX if target_max is None else target_max
    _unit_rows('normalize_stains', 'target_stains', T, ((2, 3), (3, 3)))      # bad targets are refused before any launch
    _positive_pair('normalize_stains', 'target_max', tm)
    S = estimate_stains(image, order, beta, alpha, within) if stains is None else stains
    maxima, bins, n = _stain_maxima(image, S, order, alpha, beta, within)
    a = recolor_matrix(S, maxima, T, tm)
    out = recolor(image, a, order)
    if return_info:
        return out, dict(stains=np.array(S, dtype=np.float64), maxima=maxima, bins=bins, n=n, matrix=a)
    return out


RegionStats = collections.namedtuple('RegionStats', ('count', 'sum', 'sumsq', 'min', 'max', 'argmin', 'argmax'))
REGION_MAX_QUANTILES = kernels.REGION_MAX_QUANTILES
STAIN_FEATURE_NAMES = tuple('%s%s_%s' % (where, stain, what) for where in ('', 'ring_') for stain in ('hematoxylin', 'eosin')
                            for what in ('mean', 'std', 'median', 'range'))
STAIN_FEATURE_QUANTILES = (1000, 5000, 9000)      # as q10k: the range column is the 90 % minus the 10 % quantile


def _region_args(fn, labels, values, max_label, within, dtypes):
    """The refusals the region functions share, then the label range: returns (max_label, values with bool as uint8).  Without
    ``max_label`` the range is read from the labels (one host sync)."""
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    _check_image(fn, 'values', values, dtypes)
    if tuple(values.shape) != tuple(labels.shape) or values.device != labels.device:
        raise ValueError('%s: values must have the shape and device of labels (got %s on %s and %s on %s)'
                         % (fn, tuple(values.shape), values.device, tuple(labels.shape), labels.device))
    _check_within(fn, within, labels)
    return _label_top(fn, labels, max_label), values.view(torch.uint8) if values.dtype == torch.bool else values


def _label_top(fn, labels, max_label):
    """``max_label`` checked, or read from the labels (one host sync; negative labels raise there).  The kernel table narrows the
    labels to int32 itself; an int64 value that does not fit stays outside [0, max_label] and is refused with the rest."""
    if max_label is not None:
        if isinstance(max_label, bool) or not isinstance(max_label, numbers.Integral):
            raise ValueError('%s: max_label must be an integer (got %r)' % (fn, max_label))
        hi = int(max_label)
        if hi < 0:
            raise ValueError('%s: max_label must not be negative (got %d)' % (fn, hi))
    elif labels.numel() == 0:
        hi = 0
    else:
        lo, hi = torch.stack([labels.min(), labels.max()]).to(torch.int64).tolist()      # host sync: the label range
        if lo < 0:
            raise ValueError('%s: negative labels in the label image' % fn)
    if hi >= INT32_MAX:
        raise ValueError('%s: label values must lie below 2^31 - 1 (largest: %d)' % (fn, hi))
    return hi


def _refuse_labels(fn, refused, max_label):
    if refused:
        raise ValueError('%s: %d pixels carry a label outside [0, %d]' % (fn, refused, max_label))


def region_statistics(labels, values, max_label=None, within=None):
    """Count, sum, sum of squares, extrema and their positions of ``values`` over every region of a label image (csrc/region.hip; the
    contract item by item: kernels.KernelSpec.region_statistics).  labels: 2-D tensor of any integer dtype on the GPU, any strides;
    values: bool / uint8 / int8 / int16 / int32, same shape and device (TypeError for another dtype, ValueError for another shape);
    ``within`` (bool / integer, same shape): only its non-zero pixels are counted.  Returns the named tuple ``RegionStats(count int32,
    sum int64, sumsq int64, min int32, max int32, argmin int32, argmax int32)``, every table [max_label + 1] and indexed by label
    value -- row 0 is the background, a region like any other.  ``sumsq`` is None for int32 values (it would not fit int64).
    ``argmin`` / ``argmax`` are raster indices y * W + x; of equal values the smallest index is reported.  A label without a counted
    pixel has count 0, sum 0, sumsq 0, min = max = 0 and argmin = argmax = -1.  Exact integers, bit-identical from call to call.

    The ``max`` and ``argmax`` of ``region_statistics(L, distance_transform(L != 0))`` are the inscribed radius squared of every
    nucleus and its centre: how thick it is, and where.

    Host syncs: the read of the label range unless ``max_label`` is given (negative labels raise ValueError; the tables are indexed by
    label value, so sparse ids cost memory in proportion to the largest), and the one read of ``meta``: pixels whose label lies
    outside [0, max_label] raise ValueError."""
    hi, values = _region_args('region_statistics', labels, values, max_label, within, _INT32_DTYPES)
    with torch.cuda.device(labels.device):
        tables, meta = kernels.get().region_statistics(labels, values, hi, within)
    _refuse_labels('region_statistics', int(meta.item()), hi)      # host sync: the refused pixels
    return RegionStats(*tables)


def _region_histogram(fn, labels, values, max_label, within):
    hi, values = _region_args(fn, labels, values, max_label, within, (torch.bool, torch.uint8))
    with torch.cuda.device(labels.device):
        hist, meta = kernels.get().region_histogram(labels, values, hi, within)
    return hist, meta, hi


def region_histogram(labels, values, max_label=None, within=None):
    """The 256-bin histogram of a uint8 or bool plane over every region of a label image (kernels.KernelSpec.region_histogram): int32
    [max_label + 1, 256], hist[L][v] = the pixels of label L with value v -- with ``within`` only those where it is non-zero.
    Arguments as region_statistics; its row L is ``histogram(values, within=labels == L)``, all rows in one pass.

    Host syncs: as region_statistics."""
    hist, meta, hi = _region_histogram('region_histogram', labels, values, max_label, within)
    _refuse_labels('region_histogram', int(meta.item()), hi)       # host sync: the refused pixels
    return hist


def _q10k_list(fn, q):
    """(q10k of every quantile, was q a single number)."""
    single = isinstance(q, numbers.Real) or not isinstance(q, (list, tuple))
    qs = [rank_q10k(v) for v in ((q,) if single else q)]
    if not 1 <= len(qs) <= REGION_MAX_QUANTILES:
        raise ValueError('%s: q takes 1 to %d quantiles (got %d)' % (fn, REGION_MAX_QUANTILES, len(qs)))
    return qs, single


def region_quantiles(labels, values, q, max_label=None, within=None):
    """Quantiles of a uint8 or bool plane over every region: uint8 [max_label + 1, len(q)], or [max_label + 1] for a single number
    ``q``.  With n the pixels of a region and v[0] <= ... <= v[n-1] their values sorted, the result is v[min(n - 1, floor(n * q10k /
    10000))], q10k = rank_q10k(q) -- rank_filter's rule: 0 is the minimum, 1 the maximum, 1/2 the median (the upper one when n is
    even); 0 for a region without a pixel.  ``q``: a real number in [0, 1] or a list / tuple of at most 8 (ValueError otherwise).  One
    histogram pass and one wave per region (kernels.KernelSpec.region_histogram, region_quantiles); other arguments as
    region_statistics.

    Host syncs: as region_statistics."""
    qs, single = _q10k_list('region_quantiles', q)
    hist, meta, hi = _region_histogram('region_quantiles', labels, values, max_label, within)
    with torch.cuda.device(hist.device):
        out = kernels.get().region_quantiles(hist, qs)
    _refuse_labels('region_quantiles', int(meta.item()), hi)       # host sync: the refused pixels
    return out[:, 0] if single else out


def region_mean_std(stats):
    """(mean, std) float32 [max_label + 1] of a ``RegionStats`` with ``sumsq``: mean = sum / count and the population standard
    deviation sqrt(max(0, sumsq / count - mean^2)), computed in float64 on the device from the integer tables and rounded once; rows
    with count 0 give 0.  A constant region gives std exactly 0.  ValueError for statistics of int32 values, which carry no sumsq.

    Host syncs: none."""
    if not isinstance(stats, RegionStats):
        raise TypeError('region_mean_std takes the RegionStats of region_statistics')
    if stats.sumsq is None:
        raise ValueError('region_mean_std needs sumsq: statistics of int32 values carry none')
    n = stats.count.to(torch.float64)
    some = n > 0
    n = torch.where(some, n, 1.0)
    mean = stats.sum.to(torch.float64) / n
    var = (stats.sumsq.to(torch.float64) / n - mean * mean).clamp_(min=0.0)
    zero = torch.zeros_like(mean)
    return torch.where(some, mean, zero).to(torch.float32), torch.where(some, var.sqrt(), zero).to(torch.float32)


def ring_labels(labels, distance, within=None):
    """The cytoplasm ring of every nucleus: ``expand_labels(labels, distance, within=within)`` with the pixels of the nuclei
    themselves set to 0 -- each ring pixel carries the label of its nearest nucleus, for statistics around the nucleus
    (``region_statistics(ring_labels(L, 6), plane)``).  Arguments as expand_labels' Euclidean growth.

    Host syncs: none."""
    grown = expand_labels(labels, distance, within=within)
    return torch.where(labels != 0, torch.zeros_like(grown), grown)


def stain_features(labels, tile, kept_labels, stains=None, order='bgr', ring=0, max_label=None):
    """Stain features per nucleus, to put beside ``nucleus_features``' sixteen gray-level columns: float32 [len(kept_labels), 8], or
    16 with ``ring`` > 0; ``STAIN_FEATURE_NAMES`` names the columns.  labels: 2-D integer instance mask on the GPU; tile: the uint8
    [H, W, 3] H&E tile it was made from (``stains``, ``order``: as separate_stains); kept_labels: 1-D int32 or int64 tensor on the
    same device, e.g. the third output of nucleus_features -- row k describes label kept_labels[k].  For the haematoxylin and the
    eosin plane of ``separate_stains`` (levels of 1 / 64 of a natural-log unit) the columns are the mean, the population standard
    deviation (region_mean_std), the median and the 10 % to 90 % quantile range (region_quantiles) over the nucleus' pixels.  With
    ``ring`` > 0 the same eight columns follow for ``ring_labels(labels, ring)``, the cytoplasm around each nucleus; a nucleus
    without a ring pixel has zeros there.

    Host syncs: the label range unless ``max_label`` is given, and one read that brings the refused pixels and the check of
    kept_labels: labels or kept_labels outside [0, max_label] raise ValueError."""
    fn = 'stain_features'
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    _check_color(fn, tile)
    if tuple(tile.shape[:2]) != tuple(labels.shape) or tile.device != labels.device:
        raise ValueError('%s: tile must have the height, width and device of labels (got %s on %s and %s on %s)'
                         % (fn, tuple(tile.shape[:2]), tile.device, tuple(labels.shape), labels.device))
    if not torch.is_tensor(kept_labels) or kept_labels.dtype not in (torch.int32, torch.int64):
        raise TypeError('%s: kept_labels must be an int32 or int64 tensor' % fn)
    if kept_labels.dim() != 1 or kept_labels.device != labels.device:
        raise ValueError('%s: kept_labels must be 1-D and on the device of labels' % fn)
    if isinstance(ring, bool) or not isinstance(ring, numbers.Real) or not ring >= 0:
        raise ValueError('%s: ring must be a distance >= 0 (got %r)' % (fn, ring))
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    hi = _label_top(fn, labels, max_label)
    planes = separate_stains(tile, stains, order, planes=(0, 1))
    with torch.cuda.device(labels.device):
        k = kernels.get()
        columns, meta = [], None
        for regions in (labels,) + ((ring_labels(labels, ring),) if ring > 0 else ()):
            for plane in planes:
                tables, m = k.region_statistics(regions, plane, hi)
                meta = m if meta is None else meta                  # the rings carry labels of the mask (or 0): one check covers both
                mean, std = region_mean_std(RegionStats(*tables))
                q = k.region_quantiles(k.region_histogram(regions, plane, hi)[0], STAIN_FEATURE_QUANTILES).to(torch.float32)
                columns += [mean, std, q[:, 1], q[:, 2] - q[:, 0]]
    table = torch.stack(columns, dim=1)
    kept = kept_labels.to(torch.int64)
    out = table[kept.clamp(0, hi)]
    refused, bad_kept = torch.stack([meta[0].to(torch.int64), ((kept < 0) | (kept > hi)).sum()]).tolist()      # host sync
    _refuse_labels(fn, refused, hi)
    if bad_kept:
        raise ValueError('%s: %d of kept_labels lie outside [0, %d]' % (fn, bad_kept, hi))
    return out


COOC_MAX_OFFSET = kernels.COOC_MAX_OFFSET
COOC_MAX_OFFSETS = kernels.COOC_MAX_OFFSETS
COOC_MAX_LEVELS = kernels.COOC_MAX_LEVELS
COOC_DIRECTIONS = ((0, 1), (1, 1), (1, 0), (1, -1))      # Haralick et al. 1973: 0, 45, 90 and 135 degrees at distance 1
COOC_PROPERTIES = ('contrast', 'dissimilarity', 'homogeneity', 'ASM', 'energy', 'correlation', 'entropy')
TEXTURE_PROPERTIES = ('contrast', 'dissimilarity', 'homogeneity', 'energy', 'correlation', 'entropy')
TEXTURE_FEATURE_NAMES = tuple('hematoxylin_%s_%s' % (prop, what) for prop in TEXTURE_PROPERTIES for what in ('mean', 'range'))


def _check_levels(fn, levels):
    if isinstance(levels, bool) or not isinstance(levels, numbers.Integral) or not 2 <= levels <= COOC_MAX_LEVELS:
        raise ValueError('%s: levels must be an integer in 2..%d (got %r)' % (fn, COOC_MAX_LEVELS, levels))
    return int(levels)


def level_lut(levels, lo=0, hi=255):
    """The table that quantises a uint8 plane to ``levels`` (2..16) grey levels for region_cooccurrence: a tuple of 256 ints.  v <= lo
    maps to 0, v >= hi to levels - 1, and between them the level is floor((v - lo) * levels / (hi - lo + 1)), in exact integers; 0 <=
    lo < hi <= 255 (ValueError otherwise).  The default (lo = 0, hi = 255) is v * levels >> 8 when ``levels`` is a power of two.

    Host syncs: none (no tensor is touched)."""
    levels = _check_levels('level_lut', levels)
    for name, v in (('lo', lo), ('hi', hi)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError('level_lut: %s must be an integer (got %r)' % (name, v))
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi <= 255:
        raise ValueError('level_lut: 0 <= lo < hi <= 255 is required (got lo = %d, hi = %d)' % (lo, hi))
    return tuple(0 if v <= lo else levels - 1 if v >= hi else (v - lo) * levels // (hi - lo + 1) for v in range(256))


def cooc_directions(distance=1):
    """The four directions of COOC_DIRECTIONS at ``distance`` (an integer in 1..16): ((0, d), (d, d), (d, 0), (d, -d)).

    Host syncs: none."""
    if isinstance(distance, bool) or not isinstance(distance, numbers.Integral) or not 1 <= distance <= COOC_MAX_OFFSET:
        raise ValueError('cooc_directions: distance must be an integer in 1..%d (got %r)' % (COOC_MAX_OFFSET, distance))
    return tuple((dy * int(distance), dx * int(distance)) for dy, dx in COOC_DIRECTIONS)


def _cooc_lut(fn, lut, levels):
    """``lut`` as a list for the launch argument: None is level_lut(levels); a tensor on the GPU cannot be one."""
    if lut is None:
        return level_lut(levels)
    if torch.is_tensor(lut):
        if lut.device.type != 'cpu':
            raise TypeError('%s: lut is a launch argument and must live on the host (got a tensor on %s)' % (fn, lut.device))
        if lut.dtype == torch.bool or lut.is_floating_point() or lut.is_complex():
            raise ValueError('%s: lut must hold integers (got %s)' % (fn, lut.dtype))
        lut = lut.reshape(-1).tolist() if lut.dim() == 1 else [None]
    elif isinstance(lut, np.ndarray):
        if lut.dtype.kind not in 'iu':
            raise ValueError('%s: lut must hold integers (got %s)' % (fn, lut.dtype))
        lut = lut.tolist() if lut.ndim == 1 else [None]
    elif not isinstance(lut, (list, tuple)):
        raise TypeError('%s: lut must be None, a list, a tuple, a numpy array or a CPU tensor (got %s)' % (fn, type(lut).__name__))
    if len(lut) != 256:
        raise ValueError('%s: lut must be 256 integers, one per value of the plane' % fn)
    return lut


def _cooc_tables(fn, labels, values, offsets, levels, lut, symmetric, max_label, within):
    """The checks, every one before a launch, and the launch: (tables [R, K, levels, levels], meta, max_label)."""
    levels = _check_levels(fn, levels)
    lut = _cooc_lut(fn, lut, levels)
    try:
        offsets = list(offsets)
    except TypeError:
        raise ValueError('%s: offsets must be a sequence of pairs (dy, dx) (got %r)' % (fn, offsets))
    kernels.HipKernels._check_cooc(lut, levels, offsets)
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    if labels.shape[0] * labels.shape[1] >= kernels.COOC_MAX_PIXELS:
        raise ValueError('%s: images of 2^30 pixels or more are not supported (%d x %d): a count must fit int32'
                         % ((fn,) + tuple(labels.shape)))
    hi, values = _region_args(fn, labels, values, max_label, within, (torch.bool, torch.uint8))
    with torch.cuda.device(labels.device):
        tables, meta = kernels.get().region_cooccurrence(labels, values, hi, lut, levels, offsets, bool(symmetric), within)
    return tables.view(hi + 1, len(offsets), levels, levels), meta, hi


def region_cooccurrence(labels, values, offsets=COOC_DIRECTIONS, levels=16, lut=None, symmetric=True, max_label=None, within=None):
    """The grey-level co-occurrence tables (GLCM) of a uint8 or bool plane over every region of a label image (csrc/region.hip; the
    contract item by item: kernels.KernelSpec.region_cooccurrence): int32 [max_label + 1, len(offsets), levels, levels].  Entry [R, k,
    a, b] is the number of pixel pairs p, q = p + offsets[k] that both lie inside the image, both carry label R, both lie where
    ``within`` is non-zero (if given), and whose levels are a at p and b at q; with ``symmetric`` every pair is also counted the
    other way round, so the table equals its transpose and a pair of equal levels adds 2 to the diagonal (skimage's
    ``graycomatrix(..., symmetric=True)``).  ``offsets``: 1 to 8 pairs (dy, dx), |dy| and |dx| <= 16, not (0, 0); ``levels``: 2..16;
    ``lut``: None (``level_lut(levels)``) or 256 integers below ``levels`` as a list, tuple, numpy array or CPU tensor -- the level
    of a pixel is lut[v]; a tensor on the GPU is a TypeError, because the table is a launch argument.  Row 0, the background, is a
    region like any other: ``within=labels != 0`` leaves it out.  Images of 2^30 pixels or more are refused (a count must fit
    int32).  Other arguments as region_statistics.  Exact integers, bit-identical from call to call.

    Host syncs: as region_statistics."""
    tables, meta, hi = _cooc_tables('region_cooccurrence', labels, values, offsets, levels, lut, symmetric, max_label, within)
    _refuse_labels('region_cooccurrence', int(meta.item()), hi)    # host sync: the refused pixels
    return tables


def _check_props(fn, props):
    try:
        props = tuple(props)
    except TypeError:
        raise ValueError('%s: props must be a sequence of names out of %r' % (fn, COOC_PROPERTIES))
    if not props or any(p not in COOC_PROPERTIES for p in props):
        raise ValueError('%s: props must be names out of %r, at least one (got %r)' % (fn, COOC_PROPERTIES, props))
    return props


def cooccurrence_properties(tables, props=COOC_PROPERTIES):
    """The Haralick properties of co-occurrence tables: float32 [R, K, len(props)] for integer tables [R, K, levels, levels] (those
    of region_cooccurrence), computed in float64 on the tables' device from the integers and rounded once.  With n the total of a
    table and P = C / n: contrast = sum P (i - j)^2; dissimilarity = sum P |i - j|; homogeneity = sum P / (1 + (i - j)^2); ASM = sum
    P^2; energy = sqrt(ASM); entropy = -sum over P > 0 of P log2 P; correlation = sum P (i - mu_i)(j - mu_j) / (sigma_i sigma_j) in
    the centred form.  Correlation is 1 where either marginal of the integer table has a single non-zero level (skimage's rule for
    sigma = 0, decided from the integers, with no threshold).  A table with n = 0 gives 0 for every property.

    Host syncs: none."""
    fn = 'cooccurrence_properties'
    if not torch.is_tensor(tables) or tables.dtype not in _INT_DTYPES:
        raise TypeError('%s takes the integer tables of region_cooccurrence' % fn)
    if tables.dim() != 4 or tables.shape[2] != tables.shape[3] or tables.shape[2] < 1:
        raise ValueError('%s: tables must be [R, K, levels, levels] (got %s)' % (fn, tuple(tables.shape)))
    props = _check_props(fn, props)
    f64 = dict(dtype=torch.float64, device=tables.device)
    lv = tables.shape[2]
    c = tables.to(torch.float64)
    n = c.sum((2, 3))
    some = n > 0
    p = c / torch.where(some, n, torch.ones_like(n))[:, :, None, None]
    i = torch.arange(lv, **f64)
    d = i[:, None] - i[None, :]
    out = {}
    if 'contrast' in props:
        out['contrast'] = (p * (d * d)).sum((2, 3))
    if 'dissimilarity' in props:
        out['dissimilarity'] = (p * d.abs()).sum((2, 3))
    if 'homogeneity' in props:
        out['homogeneity'] = (p / (1.0 + d * d)).sum((2, 3))
    if 'ASM' in props or 'energy' in props:
        out['ASM'] = (p * p).sum((2, 3))
        out['energy'] = out['ASM'].sqrt()
    if 'entropy' in props:
        out['entropy'] = -torch.where(p > 0, p * torch.log2(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p)).sum((2, 3))
    if 'correlation' in props:
        pi, pj = p.sum(3), p.sum(2)                                  # the marginals over the anchor's and the partner's level
        di, dj = i - (pi * i).sum(2, keepdim=True), i - (pj * i).sum(2, keepdim=True)
        var = (pi * di * di).sum(2) * (pj * dj * dj).sum(2)
        cov = (p * di[:, :, :, None] * dj[:, :, None, :]).sum((2, 3))
        flat = ((tables.sum(3) != 0).sum(2) <= 1) | ((tables.sum(2) != 0).sum(2) <= 1)      # one level only: sigma = 0 exactly
        out['correlation'] = torch.where(flat, torch.ones_like(cov), cov / torch.where(flat, torch.ones_like(var), var).sqrt())
    zero = torch.zeros_like(n)
    return torch.stack([torch.where(some, out[name], zero) for name in props], dim=2).to(torch.float32)


def texture_features(labels, tile, kept_labels, stains=None, order='bgr', planes=(0,), levels=16, lo=0, hi=None, distance=1,
                     max_label=None):
    """Chromatin texture per nucleus, to put beside ``nucleus_features`` and ``stain_features``: float32 [len(kept_labels), 12 *
    len(planes)]; ``TEXTURE_FEATURE_NAMES`` names the columns for ``planes=(0,)``, the haematoxylin plane.  labels, tile, stains,
    order, kept_labels: as stain_features; ``planes``: as separate_stains.  Per plane of ``separate_stains`` the symmetric
    co-occurrence tables of every nucleus are taken at the four directions ``cooc_directions(distance)`` over the pixel pairs inside
    the nucleus (``within = labels != 0``: the background is skipped), at ``levels`` levels of ``level_lut(levels, lo, hi)``; for
    each of contrast, dissimilarity, homogeneity, energy, correlation and entropy (cooccurrence_properties, float32) two columns
    follow: the mean over the four directions, ((p0 + p1) + (p2 + p3)) / 4 in float32, and their range, max - min -- the two
    rotation-robust summaries of Haralick et al. 1973.  A nucleus without a pair in a direction contributes 0 there.

    The stain planes are in levels of 1 / 64 of a natural-log unit and rarely pass about 160, so the default ``hi=None``, 255,
    leaves the upper levels nearly empty: the caller chooses ``hi`` for the stain (``hi=159`` for haematoxylin).  No value is read
    off the tile: a ``hi`` that followed the tile would make the columns incomparable between tiles.
        x = torch.cat([features, stain_features(L, tile, kept, max_label=n), texture_features(L, tile, kept, hi=159, max_label=n)], 1)

    Host syncs: the label range unless ``max_label`` is given, and one read that brings the refused pixels and the check of
    kept_labels: labels or kept_labels outside [0, max_label] raise ValueError."""
    fn = 'texture_features'
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    _check_color(fn, tile)
    if tuple(tile.shape[:2]) != tuple(labels.shape) or tile.device != labels.device:
        raise ValueError('%s: tile must have the height, width and device of labels (got %s on %s and %s on %s)'
                         % (fn, tuple(tile.shape[:2]), tile.device, tuple(labels.shape), labels.device))
    if not torch.is_tensor(kept_labels) or kept_labels.dtype not in (torch.int32, torch.int64):
        raise TypeError('%s: kept_labels must be an int32 or int64 tensor' % fn)
    if kept_labels.dim() != 1 or kept_labels.device != labels.device:
        raise ValueError('%s: kept_labels must be 1-D and on the device of labels' % fn)
    if order not in STAIN_ORDERS:
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    _check_planes(planes)
    lut = level_lut(levels, lo, 255 if hi is None else hi)
    offsets = cooc_directions(distance)
    if labels.shape[0] * labels.shape[1] >= kernels.COOC_MAX_PIXELS:
        raise ValueError('%s: images of 2^30 pixels or more are not supported (%d x %d)' % ((fn,) + tuple(labels.shape)))
    top = _label_top(fn, labels, max_label)
    stain_planes = separate_stains(tile, stains, order, planes=planes)
    with torch.cuda.device(labels.device):
        k = kernels.get()
        inside = labels != 0
        columns, meta = [], None
        for plane in stain_planes:
            tables, m = k.region_cooccurrence(labels, plane, top, lut, levels, offsets, True, inside)
            meta = m if meta is None else meta                      # the same labels every time: one check covers all planes
            props = cooccurrence_properties(tables.view(top + 1, len(offsets), levels, levels), TEXTURE_PROPERTIES)
            mean = ((props[:, 0] + props[:, 1]) + (props[:, 2] + props[:, 3])) * 0.25      # float32, in this order
            columns.append(torch.stack([mean, props.max(1)[0] - props.min(1)[0]], dim=2).reshape(top + 1, 2 * len(TEXTURE_PROPERTIES)))
    table = torch.cat(columns, dim=1)
    kept = kept_labels.to(torch.int64)
    out = table[kept.clamp(0, top)]
    refused, bad_kept = torch.stack([meta[0].to(torch.int64), ((kept < 0) | (kept > top)).sum()]).tolist()      # host sync
    _refuse_labels(fn, refused, top)
    if bad_kept:
        raise ValueError('%s: %d of kept_labels lie outside [0, %d]' % (fn, bad_kept, top))
    return out


GEOMETRY_DIRECTIONS = kernels.GEOMETRY_DIRECTIONS
GEOMETRY_MAX_SIDE = kernels.GEOMETRY_MAX_SIDE
RegionGeometry = collections.namedtuple('RegionGeometry', ('count', 'sy', 'sx', 'syy', 'sxy', 'sxx', 'extents', 'quads', 'border'))
RegionShape = collections.namedtuple('RegionShape', (
    'area', 'centroid_y', 'centroid_x', 'var_y', 'var_x', 'cov', 'major_axis', 'minor_axis', 'eccentricity', 'orientation', 'bbox',
    'bbox_fill', 'perimeter_crack', 'perimeter', 'circularity', 'euler4', 'euler8', 'equivalent_diameter', 'feret_max', 'feret_min',
    'polygon_area', 'convexity16', 'border'))
SHAPE_FEATURE_NAMES = ('area', 'major_axis', 'minor_axis', 'eccentricity', 'orientation', 'perimeter', 'circularity', 'convexity16',
                       'feret_max', 'feret_min', 'bbox_fill', 'holes', 'touches_border')


def _geometry_tables(fn, labels, max_label, within):
    """The refusals of the geometry functions, then the launch: (RegionGeometry, meta, max_label); meta is not read."""
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    _check_within(fn, within, labels)
    kernels.HipKernels._check_geometry_dims(fn, *labels.shape)
    hi = _label_top(fn, labels, max_label)
    with torch.cuda.device(labels.device):
        (count, sums, extents, quads, border), meta = kernels.get().region_geometry(labels, hi, within)
    return RegionGeometry(count, sums[0], sums[1], sums[2], sums[3], sums[4], extents, quads, border), meta, hi


def region_geometry(labels, max_label=None, within=None):
    """The shape of every region of a label image as exact integer tables (csrc/region.hip; the contract item by item:
    kernels.KernelSpec.region_geometry).  labels, max_label, within: as region_statistics; sides of at most 32767 pixels and (H + 1)(W
    + 1) < 2^31 (ValueError).  Returns the named tuple ``RegionGeometry``, every table indexed by label value -- row 0 is the
    background, a region like any other:

      count    int32 [R]        the region's pixels
      sy, sx, syy, sxy, sxx     int64 [R] each: sums of the pixels' coordinates and of their products, y = row, x = column
      extents  int32 [R, 8, 2]  minimum and maximum of a x + b y over the pixel centres for (a, b) in ``GEOMETRY_DIRECTIONS``;
                                directions (1, 0) and (0, 1) are the bounding box
      quads    int32 [R, 4]     n1, n2, nd, n3: the 2 x 2 windows (over the image and a frame of one pixel that belongs to nobody) in
                                which the region has one pixel, two that share an edge, the two of a diagonal, three
      border   int32 [R]        the region's pixels in the first or last row or column of the image

    A label without a pixel has zeros everywhere -- its extents (0, 0) are no coordinates: mask by ``count == 0``.  Unlike nine of
    ``nucleus_features``' columns, which keep the reference's crop (neighbours count as foreground there), every number describes the
    pixels of that label and nothing else.  ``region_shape`` turns the tables into the usual properties.  Exact integers,
    bit-identical from call to call.

    Host syncs: as region_statistics."""
    geometry, meta, hi = _geometry_tables('region_geometry', labels, max_label, within)
    _refuse_labels('region_geometry', int(meta.item()), hi)        # host sync: the refused pixels
    return geometry


def region_shape(geometry):
    """Shape properties of every region from a ``RegionGeometry``: the named tuple ``RegionShape`` of tables [R], float32 unless said
    otherwise, computed in float64 on the tables' device from the integers and rounded once.  Rows with count 0 are 0 everywhere.  The
    definitions, tied to no library's version (n = count; n1, n2, nd, n3 = quads; x = column, y = row):

      area                  n
      centroid_y, _x        sy / n, sx / n
      var_y, var_x, cov     the second central moments.  With the sums shifted to the bounding box's corner (in int64; nothing is
                            subtracted at image-coordinate magnitude) A = n suu - su^2, B = n svv - sv^2, C = n suv - su sv: var_x =
                            A / n^2, var_y = B / n^2, cov = C / n^2.  The products are exact while they stay below 2^53 (any nucleus).
      major_axis, minor_axis  4 sqrt(l1), 4 sqrt(l2) of the eigenvalues l1 >= l2 of the covariance: with D = sqrt((A - B)^2 + 4 C^2),
                            l1 = (A + B + D) / (2 n^2) and l2 = max(0, A + B - D) / (2 n^2) -- the axes of the ellipse with these moments
      eccentricity          sqrt(1 - l2 / l1) = sqrt(2 D / (A + B + D)), 0 where l1 = 0
      orientation           atan2(2 cov, var_x - var_y) / 2 = atan2(2 C, A - B) / 2: the angle of the major axis from +x towards +y (y
                            points down the image), in (-pi/2, pi/2]; 0 where both arguments are 0 (a disc, a square, one pixel)
      bbox                  int32 [R, 4]: (y0, x0, y1 + 1, x1 + 1); bbox_fill = n / ((y1 + 1 - y0)(x1 + 1 - x0))
      perimeter_crack       int32: n1 + n2 + n3 + 2 nd, the number of pixel edges between the region and everything else, the image
                            frame included
      perimeter             n2 + (n1 + n3 + 2 nd) / sqrt(2), the bit-quad estimate; circularity = 4 pi n / perimeter^2
      euler4, euler8        int32: (n1 - n3 + 2 nd) / 4 and (n1 - n3 - 2 nd) / 4, components minus holes for 4- and 8-connectivity
      equivalent_diameter   sqrt(4 n / pi)
      feret_max, feret_min  the largest and smallest of the eight widths (max_k - min_k + |a| + |b|) / sqrt(a^2 + b^2) of the pixel
                            SQUARES (not centres) across ``GEOMETRY_DIRECTIONS``
      polygon_area          the area of the 16-gon cut out by the sixteen support lines of the pixel squares in these directions and
                            their opposites: consecutive lines (in angular order) are intersected, the shoelace formula gives the area
      convexity16           n / polygon_area.  The 16-gon CONTAINS the convex hull, so this is a lower bound of solidity (area over
                            hull area), not solidity: equal for shapes whose hull has edges in these directions only
      border                int32: as in the geometry

    Host syncs: none."""
    if not isinstance(geometry, RegionGeometry):
        raise TypeError('region_shape takes the RegionGeometry of region_geometry')
    g = geometry
    f64, i64 = torch.float64, torch.int64
    ni = g.count.to(i64)
    some = ni > 0
    n = torch.where(some, ni, torch.ones_like(ni)).to(f64)
    ext = g.extents.to(i64)
    x0, x1, y0, y1 = ext[:, 0, 0], ext[:, 0, 1], ext[:, 4, 0], ext[:, 4, 1]
    su, sv = g.sx - ni * x0, g.sy - ni * y0                          # int64, shifted to the corner of the bounding box
    suu = g.sxx - 2 * x0 * g.sx + ni * x0 * x0
    svv = g.syy - 2 * y0 * g.sy + ni * y0 * y0
    suv = g.sxy - x0 * g.sy - y0 * g.sx + ni * x0 * y0
    su, sv, suu, svv, suv = (t.to(f64) for t in (su, sv, suu, svv, suv))
    nn = n * n
    A, B, C = n * suu - su * su, n * svv - sv * sv, n * suv - su * sv
    D = ((A - B) * (A - B) + 4.0 * (C * C)).sqrt()
    top = A + B + D
    l1, l2 = top / (2.0 * nn), (A + B - D).clamp(min=0.0) / (2.0 * nn)
    ecc = torch.where(top > 0, (2.0 * D / torch.where(top > 0, top, torch.ones_like(top))).clamp(max=1.0).sqrt(), torch.zeros_like(top))
    q = g.quads.to(i64)
    n1, n2, nd, n3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    diag = n1 + n3 + 2 * nd
    perimeter = n2.to(f64) + diag.to(f64) / math.sqrt(2.0)
    area = ni.to(f64)
    box = ((y1 + 1 - y0) * (x1 + 1 - x0)).to(f64)
    # the sixteen support lines a x + b y <= h of the pixel squares, in angular order, relative to the corner of the bounding box
    ab = torch.tensor(GEOMETRY_DIRECTIONS, dtype=i64, device=ext.device)
    a, b = ab[:, 0], ab[:, 1]
    half = (a.abs() + b.abs()).to(f64) * 0.5
    corner = a[None] * x0[:, None] + b[None] * y0[:, None]
    lo, hi = (ext[:, :, 0] - corner).to(f64), (ext[:, :, 1] - corner).to(f64)
    widths = (hi - lo + 2.0 * half) / (a * a + b * b).to(f64).sqrt()
    h = torch.cat([hi + half, half - lo], dim=1)                    # [R, 16]
    a16, b16 = torch.cat([a, -a]).to(f64), torch.cat([b, -b]).to(f64)
    a_n, b_n, h_n = a16.roll(-1), b16.roll(-1), h.roll(-1, 1)       # every determinant a b' - b a' of consecutive lines is 1
    px, py = h * b_n - b16 * h_n, a16 * h_n - h * a_n
    polygon = 0.5 * (px * py.roll(-1, 1) - px.roll(-1, 1) * py).sum(1)
    one = torch.ones_like(area)

    def f32(t):
        return torch.where(some, t, torch.zeros_like(t)).to(torch.float32)

    def i32(t):
        return torch.where(some if t.dim() == 1 else some[:, None], t, torch.zeros_like(t)).to(torch.int32)

    return RegionShape(
        area=f32(area), centroid_y=f32(y0.to(f64) + sv / n), centroid_x=f32(x0.to(f64) + su / n), var_y=f32(B / nn), var_x=f32(A / nn),
        cov=f32(C / nn), major_axis=f32(4.0 * l1.sqrt()), minor_axis=f32(4.0 * l2.sqrt()), eccentricity=f32(ecc),
        orientation=f32(torch.atan2(2.0 * C, A - B) * 0.5), bbox=i32(torch.stack([y0, x0, y1 + 1, x1 + 1], dim=1)), bbox_fill=f32(area / box),
        perimeter_crack=i32(n1 + n2 + n3 + 2 * nd), perimeter=f32(perimeter),
        circularity=f32(4.0 * math.pi * area / torch.where(some, perimeter * perimeter, one)), euler4=i32((n1 - n3 + 2 * nd) // 4),
        euler8=i32((n1 - n3 - 2 * nd) // 4), equivalent_diameter=f32((4.0 * area / math.pi).sqrt()), feret_max=f32(widths.max(1)[0]),
        feret_min=f32(widths.min(1)[0]), polygon_area=f32(polygon), convexity16=f32(area / torch.where(some, polygon, one)),
        border=i32(g.border.to(i64)))


def _shape_table(shape):
    """float32 [R, len(SHAPE_FEATURE_NAMES)] of a RegionShape."""
    s = shape
    some = (s.area > 0).to(torch.float32)
    return torch.stack([s.area, s.major_axis, s.minor_axis, s.eccentricity, s.orientation, s.perimeter, s.circularity, s.convexity16,
                        s.feret_max, s.feret_min, s.bbox_fill, (1 - s.euler8).to(torch.float32) * some,
                        (s.border > 0).to(torch.float32)], dim=1)


def shape_features(labels, kept_labels, max_label=None, within=None):
    """Shape features per nucleus, to put beside ``nucleus_features``, ``stain_features`` and ``texture_features``: float32
    [len(kept_labels), 13]; ``SHAPE_FEATURE_NAMES`` names the columns.  labels: 2-D integer instance mask on the GPU; kept_labels: as
    stain_features -- row k describes label kept_labels[k]; within: as region_geometry.  The columns are ``region_shape``'s area,
    major_axis, minor_axis, eccentricity, orientation, perimeter, circularity, convexity16, feret_max, feret_min and bbox_fill, then
    ``holes`` = 1 - euler8 (the holes of a connected nucleus, counted with 4-connected background) and ``touches_border`` = 1 where
    the nucleus has a pixel on the image frame (its shape is cut: tiled pipelines drop such rows), else 0.  A label without a pixel
    gives a row of zeros.  Each row describes the pixels of its own label only, also where nuclei touch:

        x = torch.cat([features, stain_features(L, tile, kept, max_label=n), texture_features(L, tile, kept, hi=159, max_label=n),
                       shape_features(L, kept, max_label=n)], 1)

    Host syncs: the label range unless ``max_label`` is given, and one read that brings the refused pixels and the check of
    kept_labels: labels or kept_labels outside [0, max_label] raise ValueError."""
    fn = 'shape_features'
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    if not torch.is_tensor(kept_labels) or kept_labels.dtype not in (torch.int32, torch.int64):
        raise TypeError('%s: kept_labels must be an int32 or int64 tensor' % fn)
    if kept_labels.dim() != 1 or kept_labels.device != labels.device:
        raise ValueError('%s: kept_labels must be 1-D and on the device of labels' % fn)
    geometry, meta, hi = _geometry_tables(fn, labels, max_label, within)
    table = _shape_table(region_shape(geometry))
    kept = kept_labels.to(torch.int64)
    out = table[kept.clamp(0, hi)]
    refused, bad_kept = torch.stack([meta[0].to(torch.int64), ((kept < 0) | (kept > hi)).sum()]).tolist()      # host sync
    _refuse_labels(fn, refused, hi)
    if bad_kept:
        raise ValueError('%s: %d of kept_labels lie outside [0, %d]' % (fn, bad_kept, hi))
    return out


RegionHull = collections.namedtuple('RegionHull', ('count', 'area2', 'diameter2', 'diameter_ends', 'width_cross', 'width_edge', 'perimeter',
                                                   'vertices', 'ptr'))
RegionHull.__new__.__defaults__ = (None, None)
HullShape = collections.namedtuple('HullShape', ('convex_area', 'solidity', 'convex_perimeter', 'feret_max', 'feret_min', 'feret_ratio',
                                                 'feret_angle', 'vertices'))
HULL_FEATURE_NAMES = ('solidity', 'convex_area', 'convex_perimeter', 'feret_max', 'feret_min', 'feret_ratio', 'feret_angle')


def _check_kept(fn, kept_labels, labels):
    if not torch.is_tensor(kept_labels) or kept_labels.dtype not in (torch.int32, torch.int64):
        raise TypeError('%s: kept_labels must be an int32 or int64 tensor' % fn)
    if kept_labels.dim() != 1 or kept_labels.device != labels.device:
        raise ValueError('%s: kept_labels must be 1-D and on the device of labels' % fn)


def _hull_tables(fn, labels, max_label, within, kept_labels=None, tall_rows=0):
    """The refusals of the hull functions, the geometry launch, the ONE host read -- the refused pixels, the rows of all bounding boxes
    and, with kept_labels, how many of them lie outside [0, max_label] -- and the hull launches: (RegionGeometry, the tables of
    kernels.KernelSpec.region_hull, points, ptr, max_label)."""
    geometry, meta, hi = _geometry_tables(fn, labels, max_label, within)
    with torch.cuda.device(labels.device):
        ptr = kernels.get().region_hull_ptr(geometry.count, geometry.extents)
    parts = [meta[0].to(torch.int64), ptr[-1]]
    if kept_labels is not None:
        kept = kept_labels.to(torch.int64)
        parts.append(((kept < 0) | (kept > hi)).sum())
    read = torch.stack(parts).tolist()                                # host sync: the refused pixels, the span rows
    _refuse_labels(fn, read[0], hi)
    if kept_labels is not None and read[2]:
        raise ValueError('%s: %d of kept_labels lie outside [0, %d]' % (fn, read[2], hi))
    with torch.cuda.device(labels.device):
        tables, points = kernels.get().region_hull(labels, hi, geometry.extents, ptr, int(read[1]), within, tall_rows)
    return geometry, tables, points, ptr, hi


def region_hull(labels, max_label=None, within=None, return_vertices=False):
    """The exact convex hull of every region of a label image (csrc/region.hip; the contract item by item:
    kernels.KernelSpec.region_hull).  labels, max_label, within and the limits on the sides: as region_geometry.

    THE HULL of label L is the convex hull of the pixel SQUARES of its counted pixels: the pixel at row y, column x is the square [x, x
    + 1] x [y, y + 1], so hull vertices are lattice corners -- the convention ``region_shape``'s feret_max, feret_min and 16-gon already
    use.  It follows that hull area >= count, and that solidity is 1 for a rectangle.  The definition is tied to no library's version:
    skimage counts the pixels inside a hull, cv2 hulls a contour.  Returns the named tuple ``RegionHull``, every table indexed by label
    value -- row 0 is the background, a region like any other:

      count          int32 [R]        the number of hull vertices (at least 4)
      area2          int64 [R]        twice the hull's area (shoelace)
      diameter2      int64 [R]        the largest squared distance between two vertices: the maximum Feret diameter, squared
      diameter_ends  int32 [R, 2, 2]  its two end points as (y, x).  Of several pairs that attain it, the one with the smallest vertex
                                      indices (i, j), i < j, in hull order
      width_cross    int64 [R]        the minimum width is width_cross / |width_edge|: over the hull's edges e = (dy, dx) the smallest
      width_edge     int32 [R, 2]     of c / |e|, c = the largest dy (x - x_e) - dx (y - y_e) over the vertices; edges are compared
                                      exactly (c_a^2 |e_b|^2 against c_b^2 |e_a|^2 in 128 bits), of equal widths the first in hull order
      perimeter      float64 [R]      the edge lengths sqrt(dy^2 + dx^2) summed in hull order

    and, with ``return_vertices``, ``vertices`` int32 [V, 2] as (y, x) and ``ptr`` int64 [R + 1]: label L's vertices are
    vertices[ptr[L]:ptr[L + 1]], strictly convex (none on the segment between its neighbours), listed from the left end of the top
    lattice line down the left side, along the bottom and up the right side, without repeats -- the list is unique.  Both are None
    otherwise.  A label without a counted pixel has zeros everywhere and no vertices.  Exact integers but for the perimeter (correctly
    rounded square roots, one addition each), bit-identical from call to call.

    Host syncs: as region_geometry -- the label range unless ``max_label`` is given, and ONE read that brings the refused pixels
    (ValueError) and the number of rows of all bounding boxes, which sizes the second launch.  ``return_vertices`` adds one read: V."""
    geometry, tables, points, rows, hi = _hull_tables('region_hull', labels, max_label, within)
    if not return_vertices:
        return RegionHull(*tables)
    count = tables[0].to(torch.int64)
    ptr = torch.zeros(hi + 2, dtype=torch.int64, device=count.device)
    torch.cumsum(count, 0, out=ptr[1:])
    total = int(ptr[-1].item())                                          # host sync: the number of vertices
    first = 2 * (rows[:-1] + torch.arange(hi + 1, device=count.device))  # where each label's vertices start in ``points``
    index = torch.repeat_interleave(first - ptr[:-1], count, output_size=total) + torch.arange(total, device=count.device)
    return RegionHull(*tables, vertices=points[index], ptr=ptr)


def hull_shape(hull, geometry):
    """Shape properties from a ``RegionHull`` and the ``RegionGeometry`` of the same labels: the named tuple ``HullShape`` of tables
    [R], float32, computed in float64 on the tables' device from the integers and rounded once, as ``region_shape`` does.  Rows with
    count 0 are 0 everywhere.  With n = geometry.count:

      convex_area       area2 / 2
      solidity          n / convex_area: area over hull area, at most 1 and 1 for a rectangle -- what ``region_shape``'s convexity16
                        bounds from below
      convex_perimeter  perimeter
      feret_max         sqrt(diameter2): the largest distance between two points of the pixel squares
      feret_min         width_cross / |width_edge|: the smallest distance between two parallel lines that enclose them
      feret_ratio       feret_min / feret_max
      feret_angle       the angle of the diameter from +x towards +y (y points down the image), ``region_shape``'s convention for
                        ``orientation``: atan2(dy, dx) of the vector between diameter_ends turned so that dx > 0, or dx = 0 and dy > 0,
                        in (-pi/2, pi/2]
      vertices          count

    Host syncs: none."""
    if not isinstance(hull, RegionHull) or not isinstance(geometry, RegionGeometry):
        raise TypeError('hull_shape takes the RegionHull of region_hull and the RegionGeometry of region_geometry')
    if hull.count.shape != geometry.count.shape or hull.count.device != geometry.count.device:
        raise ValueError('hull_shape: the hull and the geometry must describe the same labels (%d and %d rows)'
                         % (hull.count.shape[0], geometry.count.shape[0]))
    f64 = torch.float64
    some = hull.count > 0
    one = torch.ones(hull.count.shape, dtype=f64, device=hull.count.device)
    area = hull.area2.to(f64) * 0.5
    fmax = hull.diameter2.to(f64).sqrt()
    e = hull.width_edge.to(f64)
    fmin = hull.width_cross.to(f64) / torch.where(some, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).sqrt(), one)
    d = (hull.diameter_ends[:, 1] - hull.diameter_ends[:, 0]).to(f64)
    flip = (d[:, 1] < 0) | ((d[:, 1] == 0) & (d[:, 0] < 0))
    d = torch.where(flip[:, None], -d, d)

    def f32(t):
        return torch.where(some, t, torch.zeros_like(t)).to(torch.float32)

    return HullShape(convex_area=f32(area), solidity=f32(geometry.count.to(f64) / torch.where(some, area, one)),
                     convex_perimeter=f32(hull.perimeter), feret_max=f32(fmax), feret_min=f32(fmin),
                     feret_ratio=f32(fmin / torch.where(some, fmax, one)), feret_angle=f32(torch.atan2(d[:, 0], d[:, 1])),
                     vertices=f32(hull.count.to(f64)))


def hull_features(labels, kept_labels, max_label=None, within=None):
    """Hull features per nucleus, to put beside ``shape_features``: float32 [len(kept_labels), 7]; ``HULL_FEATURE_NAMES`` names the
    columns -- ``hull_shape``'s solidity, convex_area, convex_perimeter, feret_max, feret_min, feret_ratio and feret_angle.  labels,
    kept_labels, within: as shape_features; row k describes label kept_labels[k], a label without a pixel gives a row of zeros.  Each
    row describes the pixels of its own label only, also where nuclei touch or were cut apart:

        x = torch.cat([..., shape_features(L, kept, max_label=n), hull_features(L, kept, max_label=n)], 1)

    Host syncs: as shape_features -- the label range unless ``max_label`` is given, and one read that brings the refused pixels, the
    check of kept_labels and the rows of the bounding boxes: labels or kept_labels outside [0, max_label] raise ValueError."""
    fn = 'hull_features'
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    _check_kept(fn, kept_labels, labels)
    geometry, tables, _, _, hi = _hull_tables(fn, labels, max_label, within, kept_labels)
    s = hull_shape(RegionHull(*tables), geometry)
    table = torch.stack([getattr(s, name) for name in HULL_FEATURE_NAMES], dim=1)
    return table[kept_labels.to(torch.int64)]


OUTLINE_MODES = kernels.OUTLINE_MODES
OUTLINE_MAX_PIXELS = kernels.OUTLINE_MAX_PIXELS
RegionOutlines = collections.namedtuple('RegionOutlines', ('label_ptr', 'loop_ptr', 'loop_label', 'loop_start', 'loop_cracks', 'loop_area2',
                                                           'vertices', 'meta'))
OutlineTables = collections.namedtuple('OutlineTables', ('outer', 'holes', 'cracks', 'area2'))


def region_outlines(labels, max_label=None, connectivity=1, within=None, mode='corners', background=False):
    """The outline of every region of a label image: its ordered boundary as closed polygons of lattice corners, outer boundaries
    and holes (csrc/outline.hip; the contract item by item: kernels.KernelSpec.region_outlines).  labels, max_label, within: as
    region_geometry, sides of at most 32767 pixels, and H * W < 2^29 (ValueError).  connectivity 1 or 2, mode 'corners' or 'cracks'
    (ValueError otherwise).  Labels 1 .. max_label get outlines; with ``background`` label 0 is a region like any other.

    THE OUTLINE follows the cracks between pixels: the pixel at row y, column x is the square [x, x + 1] x [y, y + 1], and a side of a
    pixel of label v is a crack of v when the pixel across it does not belong to v (the image's frame included) -- the convention of
    ``region_hull`` and of ``region_shape``'s perimeter_crack.  A crack runs with its own pixel on its right (top east, right south,
    bottom west, left north), so an outer boundary runs clockwise on the screen and a hole the other way; its id is 4 (y W + x) + side
    with sides 0 top, 1 right, 2 bottom, 3 left.  Where two pixels of v touch by a corner only, connectivity 1 turns right and keeps them
    apart, connectivity 2 turns left and passes through the corner twice.  Returns the named tuple ``RegionOutlines``, all on the device:

      label_ptr    int64 [R + 1]         label L owns loops label_ptr[L] .. label_ptr[L + 1] - 1, R = max_label + 1
      loop_ptr     int64 [n_loops + 1]   loop j owns vertices[loop_ptr[j] : loop_ptr[j + 1]]
      loop_label   int32 [n_loops]       ascending; the loops of a label are ordered by loop_start
      loop_start   int32 [n_loops]       the id of the loop's smallest crack, where it starts
      loop_cracks  int32 [n_loops]       its number of cracks: its length in pixel sides
      loop_area2   int64 [n_loops]       twice the area it encloses (shoelace): positive for an outer boundary, negative for a hole
      vertices     int32 [n, 2]          corners (y, x), 0 <= y <= H, 0 <= x <= W.  'cracks': the tail of every crack; 'corners': only
                                         where the direction changes -- the first vertex of a hole is then in general not the start
                                         crack's tail
      meta         int32 [1]             0: the refused pixels

    Per label the areas sum to twice its pixel count, the cracks to perimeter_crack, and outer boundaries minus holes is euler4
    (connectivity 1) or euler8 (connectivity 2).  A label without a pixel has no loops.  Exact integers, unique, bit-identical from
    call to call.

    Host syncs: the label range unless ``max_label`` is given, and two reads: the number of cracks with the refused pixels (ValueError),
    then the number of loops and vertices.  An empty image makes neither."""
    fn = 'region_outlines'
    _check_image(fn, 'labels', labels, _INT_DTYPES)
    _check_within(fn, within, labels)
    kernels.HipKernels._check_outline(labels.shape[0], labels.shape[1], connectivity, mode)
    hi = _label_top(fn, labels, max_label)
    with torch.cuda.device(labels.device):
        tables, meta, refused = kernels.get().region_outlines(labels, hi, connectivity, within, mode, bool(background))
    _refuse_labels(fn, refused, hi)
    return RegionOutlines(*tables, meta=meta)


def _check_outlines(fn, outlines):
    if not isinstance(outlines, RegionOutlines):
        raise TypeError('%s takes a RegionOutlines (region_outlines)' % fn)


def outline_tables(outlines):
    """Per-label counts from a ``RegionOutlines``: the named tuple ``OutlineTables(outer, holes, cracks, area2)`` of int32 [R] tables
    on its device -- the number of outer boundaries (loops of positive area), of holes (negative area), the cracks of all loops (=
    region_shape's perimeter_crack) and the sum of loop_area2 (= twice the pixel count).  Integer additions only.

    Host syncs: none."""
    _check_outlines('outline_tables', outlines)
    R = outlines.label_ptr.shape[0] - 1
    index = outlines.loop_label.to(torch.int64)
    out = torch.zeros(4, R, dtype=torch.int64, device=index.device)
    area = outlines.loop_area2
    out[0].index_add_(0, index, (area > 0).to(torch.int64))
    out[1].index_add_(0, index, (area < 0).to(torch.int64))
    out[2].index_add_(0, index, outlines.loop_cracks.to(torch.int64))
    out[3].index_add_(0, index, area)
    return OutlineTables(*out.to(torch.int32))


def _ring_holds(ring, py, px):
    """Whether the rectilinear ring of (y, x) corners encloses the point (py, px), whose coordinates are half-integers: the vertical
    edges right of it that span its row, counted even-odd."""
    y1, x1 = ring[:, 0], ring[:, 1]
    y2 = np.roll(y1, -1)
    spans = (np.minimum(y1, y2) < py) & (py < np.maximum(y1, y2)) & (x1 == np.roll(x1, -1)) & (x1 > px)
    return int(spans.sum()) % 2 == 1


def outline_polygons(outlines, kept_labels=None, scale=None):
    """The outlines as polygons on the host.  Returns a list with one entry per label of ``kept_labels`` (an int32 / int64 tensor or a
    sequence of integers; None: every label 0 .. R - 1): the list of that label's polygons, each a list [outer ring, hole ring, ...] of
    float64 numpy arrays [m, 2] of (x, y) -- x first, as GeoJSON and slide viewers take them; rings are not closed (the first point is
    not repeated).  A label without a pixel gives an empty list.

    scale = (from_size, to_size), pairs (H, W): corners are mapped as ``scale_points`` maps pixel-centre coordinates between the two
    rasters -- a corner c sits half a pixel before centre c, so it goes to c * to / from per axis, the image's frame to the frame.

    HOLES.  A hole (a loop of negative area) goes to the outer ring of the same label that encloses it, the innermost (smallest area)
    if several do (an island inside a hole).  For connectivity 1 a hole never touches an outer ring, and "encloses its first vertex"
    is well defined.  For connectivity 2 a hole can touch its outer ring at a corner, where a vertex test has no answer, so for BOTH the
    point tested is the centre of the pixel across the hole's first crack -- a pixel of the hole itself, strictly inside it and on no
    lattice line; for connectivity 1 this is the same ring the first vertex gives.

    Host syncs: one transfer of the tables (with kept_labels, if they are a tensor)."""
    fn = 'outline_polygons'
    _check_outlines(fn, outlines)
    R = outlines.label_ptr.shape[0] - 1
    n_loops = outlines.loop_label.shape[0]
    sx = sy = 1.0
    if scale is not None:
        try:
            (h, w), (h2, w2) = ((operator.index(v) for v in size) for size in scale)
        except (TypeError, ValueError):
            raise ValueError('%s: scale must be (from_size, to_size), pairs of integers, got %r' % (fn, scale))
        if min(h, w, h2, w2) < 1:
            raise ValueError('%s: the sizes of scale must be positive, got %r' % (fn, scale))
        sy, sx = h2 / float(h), w2 / float(w)
    parts = [outlines.label_ptr, outlines.loop_ptr, outlines.loop_area2, outlines.vertices.reshape(-1)]
    if torch.is_tensor(kept_labels):
        if kept_labels.dtype not in (torch.int32, torch.int64) or kept_labels.dim() != 1:
            raise TypeError('%s: kept_labels must be a 1-D int32 or int64 tensor, or a sequence of integers' % fn)
        parts.append(kept_labels.to(outlines.label_ptr.device))
    flat = torch.cat([p.to(torch.int64) for p in parts]).cpu().numpy()      # host sync: the one transfer
    sizes = np.cumsum([p.numel() for p in parts])
    label_ptr, loop_ptr, area2, vertices = np.split(flat, sizes)[:4]
    vertices = vertices.reshape(-1, 2)
    if torch.is_tensor(kept_labels):
        kept = [int(v) for v in flat[sizes[3]:]]
    elif kept_labels is None:
        kept = list(range(R))
    else:
        try:
            kept = [operator.index(v) for v in kept_labels]
        except TypeError:
            raise TypeError('%s: kept_labels must be a 1-D int32 or int64 tensor, or a sequence of integers' % fn)
    bad = [v for v in kept if not 0 <= v < R]
    if bad:
        raise ValueError('%s: %d of kept_labels lie outside [0, %d]' % (fn, len(bad), R - 1))
    assert len(loop_ptr) == n_loops + 1

    def ring(j):
        return vertices[loop_ptr[j]:loop_ptr[j + 1]]

    def as_xy(r):
        return np.stack([r[:, 1] * sx, r[:, 0] * sy], axis=1).astype(np.float64)

    out = []
    for v in kept:
        loops = range(int(label_ptr[v]), int(label_ptr[v + 1]))
        outer = sorted((j for j in loops if area2[j] > 0), key=lambda j: area2[j])      # the innermost first
        polygons = {j: [as_xy(ring(j))] for j in outer}
        for j in loops:
            if area2[j] >= 0:
                continue
            r = ring(j)
            dy, dx = np.sign(r[1] - r[0])                                 # the first crack; the hole lies on its left, at (-dx, dy)
            py, px = r[0][0] + 0.5 * dy - 0.5 * dx, r[0][1] + 0.5 * dx + 0.5 * dy
            home = next((k for k in outer if _ring_holds(ring(k), py, px)), None)
            if home is None:
                raise ValueError('%s: loop %d of label %d is a hole that no outer loop of the label encloses' % (fn, j, v))
            polygons[home].append(as_xy(r))
        out.append([polygons[j] for j in sorted(outer)])
    return out


def clear_border(labels, max_label=None):
    """``labels`` with every region that has a pixel in the first or last row or column of the image set to 0 (region_geometry's
    ``border`` > 0): the nuclei a tile cuts.  The other labels keep their values; nothing is renumbered.  Same dtype and shape.

    Host syncs: as region_statistics (the label range unless ``max_label`` is given; the refused pixels)."""
    geometry, meta, hi = _geometry_tables('clear_border', labels, max_label, None)
    cut = geometry.border > 0
    out = torch.where(cut[labels.clamp(0, hi).to(torch.int64)], torch.zeros_like(labels), labels)
    _refuse_labels('clear_border', int(meta.item()), hi)           # host sync: the refused pixels
    return out


SLIC_MIN_STEP, SLIC_MAX_STEP = kernels.SLIC_MIN_STEP, kernels.SLIC_MAX_STEP
SLIC_MAX_PLANES = kernels.SLIC_MAX_PLANES
SLIC_MAX_PIXELS = kernels.SLIC_MAX_PIXELS
# superpixel_features' columns for 4 planes; C planes give the first 3 + 2 C
SUPERPIXEL_FEATURE_NAMES = ('area', 'centroid_y', 'centroid_x') + tuple('plane%d_%s' % (c, what) for c in range(SLIC_MAX_PLANES)
                                                                         for what in ('mean', 'std'))


def _check_superpixel_args(planes, step, compactness, n_iter, min_size, within):
    """The refusals of superpixels, all before any launch: returns min_size with its default filled in."""
    fn = 'superpixels'
    if not torch.is_tensor(planes):
        raise TypeError('%s takes torch tensors on the GPU (planes)' % fn)
    if planes.dtype != torch.uint8:
        raise TypeError('%s: planes must be uint8, got %s' % (fn, planes.dtype))
    if planes.dim() != 3:
        raise ValueError('%s: planes must be [C, H, W] (got %s)' % (fn, tuple(planes.shape)))
    kernels.HipKernels._check_slic(planes.shape, step, compactness, n_iter)
    _check_image(fn, 'planes', planes[0], (torch.uint8,))            # on the GPU
    if min_size is None:
        min_size = max(1, step * step // 4)
    if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral) or not 0 <= min_size < 2 ** 31:
        raise ValueError('%s: min_size must be an integer in 0..2^31 - 1, got %r' % (fn, min_size))
    if within is not None:
        _check_image(fn, 'within', within)
        if tuple(within.shape) != tuple(planes.shape[1:]) or within.device != planes.device:
            raise ValueError('%s: within must have the shape and device of a plane (got %s on %s and %s on %s)'
                             % (fn, tuple(within.shape), within.device, tuple(planes.shape[1:]), planes.device))
    return int(min_size)


def _superpixel_numbers(group, piece_blob):
    """Rule (f) of superpixels on tables: group int32 [P + 1] (slic_merge's; 0 = never settled), piece_blob int64 [P + 1] (the
    leftover blob, 1 .., of every piece that never settled; anything elsewhere) or None when every piece settled.  Returns (table
    int32 [P + 1], the number of regions as a 0-d tensor): table[p] = the final number of piece p, table[0] = 0.  Pieces are numbered
    by first pixel, so a region's first pixel belongs to its smallest piece, and regions are numbered in the order of those."""
    P = group.shape[0] - 1
    dev = group.device
    ids = torch.arange(1, P + 1, dtype=torch.int64, device=dev)
    region = group[1:].to(torch.int64)                               # settled: the group's piece, 1 .. P
    if piece_blob is not None:
        region = torch.where(region == 0, P + piece_blob[1:], region)       # leftovers: P + 1 ..
    smallest = torch.full((2 * P + 2,), P + 1, dtype=torch.int64, device=dev)
    smallest.scatter_reduce_(0, region, ids, 'amin')                 # the smallest piece of every region
    lead = smallest[region]                                          # ... seen from each of its pieces
    number = torch.cumsum(lead == ids, 0)                            # at a region's smallest piece: the region's number
    table = torch.zeros(P + 1, dtype=torch.int32, device=dev)
    table[1:] = number[lead - 1].to(torch.int32)
    return table, number[-1] if P > 0 else torch.zeros((), dtype=torch.int64, device=dev)


def superpixels(planes, step, compactness=10, n_iter=10, min_size=None, within=None, return_centres=False):
    """The tile cut into compact, colour-homogeneous, 4-connected regions: SLIC superpixels (Achanta et al. 2012) in exact integers
    (csrc/slic.hip; the contract item by item: kernels.KernelSpec.slic_iterate and slic_merge) -- the nodes of a tissue graph beside
    the cell graph.  planes: uint8 [C, H, W] on the GPU, 1 <= C <= 4, any strides, fewer than 2^29 pixels -- ``separate_stains``'
    planes, or a tile as ``tile.permute(2, 0, 1)``.  step: the grid step S in pixels, 4..256 (a region has about S^2 pixels);
    compactness m: 0..1024, the weight of distance against colour (0: colour alone); n_iter: 1..64 rounds; within (bool / integer
    [H, W], same device): only its non-zero pixels are clustered.  TypeError for another dtype, ValueError for everything else, before
    any launch.  Returns (labels int32 [H, W], n): regions 1 .. n, each 4-connected, numbered by the raster order of their first
    pixels; 0 exactly where ``within`` is zero.  With ``return_centres`` also (centres int32 [K, 2 + C], count int32 [K]) of the
    clustering, before connectivity is enforced.  A pure function of its inputs, bit for bit from call to call.

    The clustering leaves labels that need not be connected.  The rule that connects them is order-free (skimage's depends on the
    scan order):
      (a) pieces, P, sizes = label_instances(clustered, connectivity=1, return_sizes=True).
      (b) A piece is small iff sizes < min_size (default max(1, S * S // 4)); the other pieces are settled, each a group of its own.
      (c) pairs, count = region_adjacency(pieces, 1).
      (d) In round r every unsettled piece with a neighbour settled before round r joins the group of the settled neighbour with the
          largest count, of equal counts the smallest piece number, and is settled from then on; until a round settles nothing.
      (e) Pixels that never settled -- a component of ``within`` made of small pieces only -- become one region per 4-connected blob.
      (f) Groups and blobs are numbered in the raster order of their first pixels; one launch writes the image.

    Host syncs: the one of label_instances, the two of region_adjacency, one per batch of merge rounds (4 rounds, then 8, ...: one
    read for an ordinary tile), one that brings "did every piece settle" and n, and only when rule (e) applies the one of a second
    label_instances and a second read of n.  None for an empty image."""
    min_size = _check_superpixel_args(planes, step, compactness, n_iter, min_size, within)
    C, H, W = planes.shape
    dev = planes.device
    i32 = dict(dtype=torch.int32, device=dev)
    if H * W == 0:
        out = (torch.zeros(H, W, **i32), 0)
        return out + ((torch.zeros(0, 2 + C, **i32), torch.zeros(0, **i32)),) if return_centres else out
    with torch.cuda.device(dev):
        k = kernels.get()
        clustered, centres, count = k.slic_iterate(planes, int(step), int(compactness), int(n_iter), within)
        pieces, P, sizes = label_instances(clustered, 1, return_sizes=True)
        if P == 0:
            final, n = pieces, 0
        else:
            pairs, contacts = region_adjacency(pieces, 1)
            group, _ = k.slic_merge(sizes, pairs, contacts, min_size)
            table, n_t = _superpixel_numbers(group, None)
            left, n = torch.stack([(group[1:] == 0).sum(), n_t]).tolist()        # host sync: pieces that never settled; n
            if left:
                unsettled = (group[pieces.to(torch.int64)] == 0) & (pieces != 0)
                blobs, _ = label_instances(unsettled, 1)
                piece_blob = torch.zeros(P + 1, dtype=torch.int64, device=dev)
                piece_blob[pieces.reshape(-1).to(torch.int64)] = blobs.reshape(-1).to(torch.int64)      # one value per piece
                table, n_t = _superpixel_numbers(group, piece_blob)
                n = int(n_t.item())                                              # host sync: n with the leftover blobs
            final = k.slic_relabel(pieces, table)
    return (final, n, (centres, count)) if return_centres else (final, n)


def _check_superpixel_labels(fn, labels, n):
    _check_labels32(fn, 'labels', labels)
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n < INT32_MAX:
        raise ValueError('%s: n must be an integer in 0..2^31 - 2, got %r' % (fn, n))
    return int(n)


def superpixel_graph(labels, n, loop=True, return_attr=False):
    """The tissue graph of a superpixel image: node i is label i + 1, and two nodes are joined iff their regions share a border
    (``region_adjacency(labels, 1)``).  labels: ``superpixels``' int32 [H, W] (0 = outside), n: its region count.  Returns edge_index
    int64 [2, E] in ``radius_knn``'s convention -- rows are centres in ascending order, then columns in ascending order; both
    directions of every pair, and (i, i) for every node iff ``loop`` -- and with ``return_attr`` also border int32 [E], the pixel pairs
    along which the two regions touch (0 on loops).  It goes into ``graph_item(features, centroids, y, edge_index=...)``.  A label
    above n is a ValueError.

    Host syncs: the two of region_adjacency and one that checks the label range."""
    n = _check_superpixel_labels('superpixel_graph', labels, n)
    dev = labels.device
    i64 = dict(dtype=torch.int64, device=dev)
    pairs, border = region_adjacency(labels, 1)
    if pairs.shape[0]:
        lo, hi = torch.stack([pairs.min(), pairs.max()]).tolist()      # host sync: the label range
        if lo < 1 or hi > n:
            raise ValueError('superpixel_graph: labels outside 1..%d' % n)
    ends = pairs.to(torch.int64) - 1
    rows, cols = torch.cat([ends[:, 0], ends[:, 1]]), torch.cat([ends[:, 1], ends[:, 0]])
    border = torch.cat([border, border])
    if loop:
        nodes = torch.arange(n, **i64)
        rows, cols = torch.cat([rows, nodes]), torch.cat([cols, nodes])
        border = torch.cat([border, torch.zeros(n, dtype=torch.int32, device=dev)])
    order = torch.argsort(rows * max(n, 1) + cols)      # (row, col) pairs are distinct
    edge_index = torch.stack([rows[order], cols[order]])
    return (edge_index, border[order]) if return_attr else edge_index


def superpixel_features(labels, planes, n):
    """The node table of a tissue graph: (features float32 [n, 3 + 2 C], centroids float32 [n, 2]) of regions 1 .. n of a superpixel
    image over uint8 planes [C, H, W] -- row i is label i + 1.  Columns (``SUPERPIXEL_FEATURE_NAMES``, the first 3 + 2 C): the area
    in pixels, the centroid (row, column), then the mean and the population standard deviation of every plane.  From the integer
    tables of ``region_geometry`` and ``region_statistics`` through ``region_mean_std``, computed in float64 and rounded once; a label
    without a pixel gives a row of zeros.

    Host syncs: the refused-pixel reads of region_geometry and of region_statistics, one per plane (a label outside 0..n raises)."""
    n = _check_superpixel_labels('superpixel_features', labels, n)
    if not torch.is_tensor(planes) or planes.dtype != torch.uint8:
        raise TypeError('superpixel_features: planes must be a uint8 tensor [C, H, W]')
    if planes.dim() != 3 or not 1 <= planes.shape[0] <= SLIC_MAX_PLANES or tuple(planes.shape[1:]) != tuple(labels.shape):
        raise ValueError('superpixel_features: planes must be [C, H, W] with 1 <= C <= %d and the shape of labels (got %s and %s)'
                         % (SLIC_MAX_PLANES, tuple(planes.shape), tuple(labels.shape)))
    geometry = region_geometry(labels, max_label=n)
    area = geometry.count[1:].to(torch.float64)
    some = area > 0
    den = torch.where(some, area, 1.0)
    cy, cx = geometry.sy[1:].to(torch.float64) / den, geometry.sx[1:].to(torch.float64) / den
    columns = [area, cy, cx]
    for c in range(planes.shape[0]):
        mean, std = region_mean_std(region_statistics(labels, planes[c], max_label=n))
        columns += [mean[1:], std[1:]]
    features = torch.stack([col.to(torch.float32) for col in columns], 1)
    return features, torch.stack([cy, cx], 1).to(torch.float32)


def regions_at(labels, points):
    """The label under each point: int32 [N] for float (row, column) coordinates [N, 2] on the labels' device, in the pixel-centre
    convention of ``scale_points`` -- pixel (i, j) has its centre at (i, j) and covers [i - 1/2, i + 1/2) x [j - 1/2, j + 1/2), so a
    point falls into pixel floor(c + 1/2) per axis, computed in float64.  0 for a point outside the image (and where the label is 0).
    ``regions_at(superpixel_labels, centroids)`` assigns every nucleus to the tissue node under it.

    Host syncs: none."""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.is_floating_point():
        raise TypeError('regions_at takes an integer label image [H, W] (labels)')
    if not torch.is_tensor(points) or not points.is_floating_point():
        raise TypeError('regions_at takes a float tensor [N, 2] (points)')
    if points.dim() != 2 or points.shape[1] != 2 or points.device != labels.device:
        raise ValueError('regions_at: points must be [N, 2] on the device of labels (got %s on %s)' % (tuple(points.shape), points.device))
    H, W = labels.shape
    out = torch.zeros(points.shape[0], dtype=torch.int32, device=labels.device)
    if H * W == 0 or points.shape[0] == 0:
        return out
    at = torch.floor(points.to(torch.float64) + 0.5)
    inside = (at[:, 0] >= 0) & (at[:, 0] < H) & (at[:, 1] >= 0) & (at[:, 1] < W)      # NaN compares false: outside
    y = torch.where(inside, at[:, 0], 0.0).to(torch.int64)
    x = torch.where(inside, at[:, 1], 0.0).to(torch.int64)
    return torch.where(inside, labels[y, x].to(torch.int32), out)


def graph_item(features, centroids, y, edge_index=None):
    """The ``Data`` of prepare_cv_dataset.py:57-72 (_read_one_raw_graph): x = cat(features, centroids) [n, 18], pos = centroids,
    y = [label], on the host -- ready for ``Batch.from_data_list(items, device=..., knn=(100, 8), mean=..., std=...)``.  With
    ``edge_index`` ([2, E], e.g. ``voronoi_graph``'s) the ``Data`` carries it on the host as int64, and
    ``Batch.from_data_list(items, device=...)`` without ``knn=`` uses it."""
    from .data import Data
    f = torch.as_tensor(features).detach().to('cpu', torch.float32)
    c = torch.as_tensor(centroids).detach().to('cpu', torch.float32)
    item = Data(x=torch.cat([f, c], dim=1), pos=c.clone(), y=torch.tensor([int(y)], dtype=torch.long))
    if edge_index is not None:
        e = torch.as_tensor(edge_index).detach().to('cpu', torch.int64)
        if e.dim() != 2 or e.shape[0] != 2:
            raise ValueError('edge_index must be [2, E] (got %s)' % (tuple(e.shape),))
        item.edge_index = e.contiguous()
    return item


def save_reference_files(root, dataset, label_dir, name, features, centroids):
    """Write ``<root>/feature/<dataset>/<label_dir>/<name>`` and ``<root>/coordinate/...`` as float32 .npy files, the two arrays
    construct_feature_graph.py:121-122 saves (``name`` = the mask's file name, e.g. 'image_001.npy').  Returns the two paths."""
    paths = []
    for kind, arr in (('feature', features), ('coordinate', centroids)):
        d = os.path.join(root, kind, dataset, label_dir)
        os.makedirs(d, exist_ok=True)
        p = os.path.join(d, name if name.endswith('.npy') else name + '.npy')
        a = arr.detach().cpu().numpy() if torch.is_tensor(arr) else np.asarray(arr)
        np.save(p, a.astype(np.float32))
        paths.append(p)
    return tuple(paths)


def synthetic_tissue(H, W, num_nuclei, seed=0):
    """A synthetic instance mask and gray image (numpy int32 [H, W], uint8 [H, W]) that exercises every quirk of the stage: rotated
    ellipses painted over each other (touching, clipped and disconnected labels), label values with gaps in random order, objects
    under 10 pixels, ring nuclei with a nucleus inside the hole, nuclei cut by each of the four image edges, and a smooth background
    plus a per-nucleus level plus noise (some pixels reach 0)."""
    rng = np.random.RandomState(seed)
    labels = np.zeros((H, W), np.int32)
    ids = (rng.permutation(6 * num_nuclei + 64)[:2 * num_nuclei + 16] + 1).astype(np.int32)   # gaps, random order
    nxt = [0]

    def new_id():
        v = ids[nxt[0]]
        nxt[0] += 1
        return v

    def paint(cy, cx, a, b, phi, lab, hole=0.0):
        r = int(np.ceil(max(a, b))) + 1
        y0, y1 = max(int(np.floor(cy)) - r, 0), min(int(np.floor(cy)) + r + 1, H)
        x0, x1 = max(int(np.floor(cx)) - r, 0), min(int(np.floor(cx)) + r + 1, W)
        if y0 >= y1 or x0 >= x1:
            return
        yy, xx = np.mgrid[y0:y1, x0:x1]
        dy, dx = yy - cy, xx - cx
        u = dx * np.cos(phi) + dy * np.sin(phi)
        v = -dx * np.sin(phi) + dy * np.cos(phi)
        q = (u / a) ** 2 + (v / b) ** 2
        m = q <= 1.0
        if hole > 0:
            m &= q > hole * hole
        labels[y0:y1, x0:x1][m] = lab

    edge_sites = [(0.0, W * 0.3), (H - 1.0, W * 0.6), (H * 0.4, 0.0), (H * 0.7, W - 1.0)]   # top, bottom, left, right
    for i in range(num_nuclei):
        kind = rng.rand()
        phi = rng.uniform(0, np.pi)
        if i < len(edge_sites):
            cy, cx = edge_sites[i]
            paint(cy, cx, rng.uniform(5, 9), rng.uniform(3, 5), phi, new_id())
            continue
        cy, cx = rng.uniform(-3, H + 2), rng.uniform(-3, W + 2)
        if kind < 0.06:                                             # under 10 pixels
            paint(cy, cx, rng.uniform(0.6, 1.6), rng.uniform(0.5, 1.2), phi, new_id())
        elif kind < 0.10:                                           # a ring with a nucleus in its hole
            a = rng.uniform(9, 14)
            b = rng.uniform(0.7, 1.0) * a
            paint(cy, cx, a, b, phi, new_id(), hole=0.6)
            paint(cy, cx, 0.3 * a, 0.3 * b, phi, new_id())
        else:
            a = rng.uniform(4, 11)
            paint(cy, cx, a, rng.uniform(0.45, 1.0) * a, phi, new_id())
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bg = 150 + 25 * np.sin(2 * np.pi * yy / max(H / 1.7, 1)) * np.cos(2 * np.pi * xx / max(W / 2.3, 1))
    level = rng.uniform(8, 130, size=int(ids.max()) + 1)
    img = np.where(labels > 0, level[labels], bg) + rng.normal(0, 14, size=(H, W))
    gray = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return labels, gray
