"""Instance masks, then nucleus features and centroids from them, on the GPU: the steps that make the node tables of every graph
(dataflow/construct_feature_graph.py:50-123 + common/nuc_feature.py, then dataflow/prepare_cv_dataset.py:57-72).

``label_instances(image)`` is the step in front: it turns a thresholded foreground map into an instance mask (connected-component
labelling, scipy.ndimage.label's numbering) or splits every value of an integer mask into its connected pieces (csrc/label.hip; the
contract item by item: kernels.KernelSpec.label_components).  Its ``labels`` and ``n`` go straight into
``nucleus_features(labels, gray, max_label=n)``.  The reference starts from finished masks and has no such step.

``nucleus_features(labels, gray)`` returns the reference's ``feature`` / ``coordinate`` arrays of one image (csrc/nuclei.hip; the
arithmetic item by item: kernels.KernelSpec.nucleus_features), ``graph_item`` turns them into the ``Data`` that
``_read_one_raw_graph`` builds, and ``save_reference_files`` writes them where the reference's dataset preparation reads them.

Differences from the reference, all stated: an image without a surviving nucleus gives empty tensors (the reference's
``np.vstack`` raises); labels must be non-negative (``ValueError``, as skimage); gray and mask must have the same size
(``ValueError``; the reference resizes, which is the identity then).  OpenCV, scikit-image and xtract-features are restated from their
documented behaviour, not linked: see DESIGN.md, "Nucleus features".
"""
import os

import numpy as np
import torch

from . import kernels

NUM_FEATURES = 16
FEATURE_NAMES = ('mean_im_out', 'diff', 'var_im', 'skew_im', 'mean_ent', 'glcm_dissimilarity', 'glcm_homogeneity', 'glcm_energy',
                 'glcm_ASM', 'eccentricity', 'area', 'majoraxis_length', 'minoraxis_length', 'perimeter', 'solidity', 'orientation')
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def label_instances(image, connectivity=1, min_size=0, return_sizes=False):
    """image: 2-D bool / uint8 / int8 / int16 / int32 / int64 tensor on the GPU, any strides; 0 = background, every other value
    (negative ones too) foreground.  Returns (labels int32 [H, W], n) and, with ``return_sizes``, int32 [n] pixel counts (sizes[k - 1]
    belongs to label k).  Two pixels share a component iff a path of neighbours (``connectivity`` 1: 4 neighbours, 2: 8) that all
    carry the same value joins them, so a bool or 0/1 image is labelled as scipy.ndimage.label does -- components numbered 1..n by the
    raster order of their first pixels, bit for bit -- and an integer mask has each value split into its connected pieces.  With
    ``min_size`` > 0 components of fewer pixels become background and take no number (skimage's remove_small_objects, then labelling).

    Host syncs: one, the read of n."""
    if not torch.is_tensor(image) or not image.is_cuda:
        raise TypeError('label_instances takes a torch tensor on the GPU')
    if image.dtype != torch.bool and image.dtype not in _INT_DTYPES:
        raise TypeError('image must be a bool or integer image, got %s' % image.dtype)
    if image.dim() != 2:
        raise ValueError('image must be 2-D (got %s)' % (tuple(image.shape),))
    if connectivity not in (1, 2):
        raise ValueError('connectivity must be 1 (4 neighbours) or 2 (8 neighbours), got %r' % (connectivity,))
    if min_size < 0:
        raise ValueError('min_size must not be negative (got %r)' % (min_size,))
    H, W = image.shape
    if H * W >= 2 ** 31:
        raise ValueError('images of 2^31 pixels or more are not supported (%d x %d)' % (H, W))
    if H * W == 0:
        labels, n = torch.zeros(H, W, dtype=torch.int32, device=image.device), 0
        sizes = torch.zeros(0, dtype=torch.int32, device=image.device)
    else:
        with torch.cuda.device(image.device):
            labels, n, sizes = kernels.get().label_components(image.contiguous(), int(connectivity), int(min_size), bool(return_sizes))
    return (labels, n, sizes) if return_sizes else (labels, n)


def nucleus_features(labels, gray, min_size=10, return_info=False, max_label=None):
    """labels: integer [H, W] instance mask on the GPU (0 = background; other integer dtypes are converted to int32), gray: uint8
    [H, W] on the same GPU.  Returns (features f32 [n, 16], centroids f32 [n, 2] as (row, col), kept_labels int32 [n]) -- row k
    describes the k-th surviving label in ascending order -- plus, with ``return_info``, int32 [n, 4]: the traced contour's start
    (row, col) in the crop, its vertex count and the path taken (0 LDS, 1 global workspace).

    Host syncs: one read of the label range (negative labels raise ValueError; the tables are indexed by label value, so very sparse
    label ids cost memory in proportion to the largest) and one read of the row count.  ``max_label`` (an int >= the largest label,
    e.g. the n of ``label_instances``) replaces the read of the label range; pixels outside [0, max_label] then raise ValueError."""
    if not (torch.is_tensor(labels) and torch.is_tensor(gray)):
        raise TypeError('nucleus_features takes torch tensors on the GPU')
    if labels.dim() != 2 or tuple(gray.shape) != tuple(labels.shape):
        raise ValueError('labels and gray must be 2-D images of the same size (got %s and %s)'
                         % (tuple(labels.shape), tuple(gray.shape)))
    if labels.dtype not in _INT_DTYPES:
        raise TypeError('labels must be an integer image, got %s' % labels.dtype)
    if gray.dtype != torch.uint8:
        raise TypeError('gray must be uint8, got %s' % gray.dtype)
    H, W = labels.shape
    if H * W >= 2 ** 31:
        raise ValueError('images of 2^31 pixels or more are not supported (%d x %d)' % (H, W))
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


def graph_item(features, centroids, y):
    """The ``Data`` of prepare_cv_dataset.py:57-72 (_read_one_raw_graph): x = cat(features, centroids) [n, 18], pos = centroids,
    y = [label], on the host -- ready for ``Batch.from_data_list(items, device=..., knn=(100, 8), mean=..., std=...)``."""
    from .data import Data
    f = torch.as_tensor(features).detach().to('cpu', torch.float32)
    c = torch.as_tensor(centroids).detach().to('cpu', torch.float32)
    return Data(x=torch.cat([f, c], dim=1), pos=c.clone(), y=torch.tensor([int(y)], dtype=torch.long))


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
