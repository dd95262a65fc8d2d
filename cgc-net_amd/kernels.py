"""Tensor-level front door of ``libcgc_hip.so`` (the C-ABI declared in include/cgc_hip.h).

``KernelSpec`` documents the exact arithmetic of every entry point -- it is the contract that the
HIP kernels (csrc/*.hip), the op-level checker (oracle/flat_ref.py, tests only) and the autograd
layer (ops.py) share.  ``HipKernels`` marshals torch tensors to raw device pointers and calls the
library through ctypes on torch's current HIP stream.  There is exactly one product implementation:
``get()`` raises if the library cannot be loaded or a tensor is not on the GPU.

All float tensors are fp32, all index tensors int32 unless stated; "ld" = leading dimension in
elements of a row-major matrix.  Kernels never allocate and never synchronise.
"""
import ctypes
import functools
import operator
import os

import torch

ACT_CODES = {'identity': 0, 'relu': 1, 'elu': 2, 'leakyrelu': 3}
L2_EPS = 1e-12       # F.normalize eps
RENORM_EPS = 1e-15   # model/network.py:8
EDT_INF = 2 ** 31 - 1      # CGC_EDT_INF: dist2 of a pixel without a site (within the bound)
EDT_MAX_SIDE = 32767       # 2 * 32766^2 < 2^31 - 1: squared distances fit int32
GEO_INF = 2 ** 31 - 1      # CGC_GEO_INF: dist of a pixel that no seed reaches (within the bound)
GEO_FIRST_BATCH, GEO_MAX_BATCH = 8, 64      # rounds of geodesic_transform per host read: 8, 16, 32, 64, 64, ...
STAIN_OD_MAX = 5674        # floor(1024 ln 255 + 0.5): the largest optical density of stain_separate's table
ANGLE_BINS = 1024          # K of angle_histogram: bins of the half turn (-pi/2, pi/2), separated by K - 1 directions
ANGLE_E_MAX, ANGLE_E_REACH = 4096, 7095      # angle_histogram's basis: |E[j][c]| and sum_c |E[j][c]| (ceil(4096 sqrt 3))
ANGLE_DIR_MAX = 16384      # angle_histogram's directions: |c_k|, |s_k|
CONC_BINS = 512            # concentration_histogram: levels of 1/128 of a natural-log unit per stain, the last one open (3.99 and up)
EXP_LUT_LEN = 6386         # od_recolor's exponential table: floor(255 exp(-k / 1024) + 0.5) is 255 at k = 0 and first 0 at k = 6385
SMOOTH_MAX_RADIUS = 5      # binomial_smooth: 255 * 4^(2 * 5) < 2^31
WINDOW_MAX_RADIUS = 127    # window_sums / local_threshold: n <= 255^2, so that Q <= 255^4 < 2^32 and everything of the rule fits int64
MORPH_MAX_RADIUS = 63      # flat_morphology: a tile plus a halo of r on both sides is one 256-byte LDS row and keeps 128 columns of its own
MORPH_KINDS = {'square': 0, 'disk': 1, 'diamond': 2}              # include/cgc_hip.h: CGC_MORPH_SQUARE / _DISK / _DIAMOND
MORPH_OPS = {'erode': 0, 'dilate': 1, 'gradient': 2}              # CGC_MORPH_ERODE / _DILATE / _GRADIENT
MORPH_EPILOGUES = {None: 0, 'other_minus': 1, 'minus_other': 2}   # CGC_MORPH_PLAIN / _OTHER_MINUS / _MINUS_OTHER
RANK_MAX_RADIUS = 63       # rank_filter: morph's tile geometry; n <= 127^2 = 16129, so n * q10k < 2^31
ENTROPY_MAX_RADIUS = 15    # rank_filter 'entropy': n <= 31^2 = 961, the length of the table of c log2 c terms
RANK_ENTROPY_TERMS = 962   # T[0..961]
RANK_OPS = {'quantile': 0, 'range': 1, 'entropy': 2}              # CGC_RANK_QUANTILE / _RANGE / _ENTROPY
ADJ_MAX_PIXELS = 2 ** 29   # region_adjacency: a pair's count can reach 4 H W and must fit int32
REGION_MAX_QUANTILES = 8   # region_quantiles: quantiles read off one histogram per launch
COOC_MAX_OFFSET = 16       # region_cooccurrence: largest |dy|, |dx| (cgc_region_cooc_max_offset)
COOC_MAX_OFFSETS = 8       # ... offsets per call (cgc_region_cooc_max_offsets)
COOC_MAX_LEVELS = 16       # ... levels: levels^2 bins are the 256 16-bit bins of a slot in LDS
COOC_MAX_PIXELS = 2 ** 30  # ... a symmetric diagonal bin holds at most 2 H W and must fit int32
GEOMETRY_MAX_SIDE = 32767  # region_geometry: largest H, W (cgc_region_geometry_max_side): sum x^2 over 2^31 pixels fits int64
GEOMETRY_DIRECTIONS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1))      # (a, b) of the extents a x + b y
OUTLINE_MAX_PIXELS = 2 ** 29      # region_outlines: a crack id 4 (y W + x) + side and the number of cracks fit int32
OUTLINE_MODES = ('corners', 'cracks')
SLIC_MAX_PIXELS = 2 ** 29         # slic_iterate: as region_adjacency, which reads the result
SLIC_MIN_STEP, SLIC_MAX_STEP = 4, 256      # ... the grid step S (cgc_slic_max_step)
SLIC_MAX_COMPACTNESS = 1024       # ... m: m^2 times a squared distance stays far inside int64
SLIC_MAX_ITER = 64                # ... rounds per call
SLIC_MAX_PLANES = 4               # ... C
SLIC_MERGE_FIRST_BATCH, SLIC_MERGE_MAX_BATCH = 4, 64      # slic_merge: rounds per host read, doubled after each
REGION_VALUE_DTYPES = {torch.uint8: (1, 0), torch.int8: (1, 1), torch.int16: (2, 1), torch.int32: (4, 1)}      # (bytes, signed)
RESAMPLE_MAX_SIDE = 32767  # resample_u8 / resample_labels: largest source and output side (cgc_resample_max_side): (2 d + 1) n < 2^31
RESAMPLE_LABELS_MAX_FACTOR = 8      # resample_labels 'majority': largest n / m per axis (cgc_resample_labels_max_factor): a box spans <= 9 pixels
RESAMPLE_MODES = {'linear': 0, 'area': 1}              # include/cgc_hip.h: CGC_RESAMPLE_LINEAR / _AREA
RESAMPLE_LABEL_MODES = {'nearest': 0, 'majority': 1}   # CGC_RESAMPLE_NEAREST / _MAJORITY (2 = _MAJORITY_UNSIGNED: uint8 and bool)
WS_JUMP_BATCH = 8        # pointer jumps of watershed_flood per host read: resolves parent chains of up to 2^7 pixels in one read


@functools.lru_cache(maxsize=4)
def _checked_dirs(dirs):
    """angle_histogram's refusals of a direction table (a tuple of tuples: the check of nuclei.ANGLE_DIRS is made once): the flat
    tuple c_1, s_1, c_2, s_2, ... of Python integers."""
    try:
        dirs = [[int(v) for v in d] for d in dirs]
    except (TypeError, ValueError):
        raise ValueError('angle_histogram: dirs must be %d x 2 integers' % (ANGLE_BINS - 1))
    if len(dirs) != ANGLE_BINS - 1 or any(len(d) != 2 for d in dirs):
        raise ValueError('angle_histogram: dirs must be %d x 2' % (ANGLE_BINS - 1))
    if any(abs(c) > ANGLE_DIR_MAX or abs(s) > ANGLE_DIR_MAX for c, s in dirs):
        raise ValueError('angle_histogram: every direction must lie in [-%d, %d]' % (ANGLE_DIR_MAX, ANGLE_DIR_MAX))
    if any(c <= 0 for c, _ in dirs) or any(c0 * s1 - s0 * c1 <= 0 for (c0, s0), (c1, s1) in zip(dirs, dirs[1:])):
        raise ValueError('angle_histogram: the directions must lie in the open right half plane (c > 0) with strictly increasing '
                         'angles (c_k s_{k+1} - s_k c_{k+1} > 0): the bin is found by binary search')
    return tuple(v for d in dirs for v in d)


class KernelSpec(object):
    """Semantics of the kernel entry points (all outputs are caller-allocated ``out`` tensors)."""

    # ------------------------------------------------------------------ graph structure (A1)
    def csr_build(self, edge_index, n, add_diag):
        """COO (int64 [2,E], row = aggregating centre) -> CSR + its transpose, both column-sorted.

        Duplicate edges collapse (model/utils.py:28-33 ASSIGNS 1); ``add_diag`` inserts (i,i) for
        every i (needed by edge_renorm, whose result always has a diagonal).  Returns a dict of
        int32 tensors: rowptr[n+1], col[cap], rowidx[cap], t_rowptr[n+1], t_col[cap], t_perm[cap]
        with cap = E (+n); entries at or beyond nnz = rowptr[n] are undefined.  t_col[k] is the
        source row of transposed slot k and t_perm[k] its slot in the forward arrays.  Edges with an id outside [0, n) are
        dropped and counted in ``bad_edges`` (int32 [1] on the device; the reference's dense indexing raises instead).
        """
        raise NotImplementedError

    def collate(self, x, mean, std, gptr, num_graphs, batch_out, edge_index, eptr):
        """Device-side finish of Batch.from_data_list: x [n,F] z-scored in place with mean/std [F] (None: untouched),
        batch_out int64 [n] = graph id per node (None: skipped), edge_index int64 [2,E] with per-graph local ids gets the
        node offset gptr[g] of its graph, the edges of graph g being [eptr[g], eptr[g+1]) (None: skipped)."""
        raise NotImplementedError

    def farthest_point_sample(self, pos, gptr, num_graphs, max_nodes, start, optr, out, table16=False):
        """Farthest-point sampling per graph (FarthestSampler, common/utils.py:187-197, on coordinates instead of the
        distance table): pos [n,2] f32, gptr int32 [B+1], start int32 [B] first pick (local index), optr int32 [B+1]
        offsets of the picks, out int32 [optr[B]] global node ids in pick order; ties -> lowest index.
        table16=False: squared fp64 distances.  table16=True: the reference's table entries int16(sqrt(dx^2+dy^2)) in
        float32 (dataflow/construct_feature_graph.py:17-24) -- the reference's picks index for index."""
        raise NotImplementedError

    def radius_knn(self, pos, gptr, num_graphs, r, k, loop):
        """Cell-graph construction for a batch of graphs (torch_cluster.radius_graph(pos, r, None, loop, k) per graph,
        dataflow/data.py:348): pos [n,2] f32, gptr int32 [B+1].  Per node its <= k nearest others within r (+ itself iff
        loop), restricted to its own graph.  Returns edge_index int64 [2, nnz] (row = centre, ascending; neighbours by
        distance, ties by index) with global node ids."""
        raise NotImplementedError

    def nucleus_features(self, labels, gray, max_label, min_size, with_info=False):
        """Nucleus feature rows and centroids of one instance mask (F4: dataflow/construct_feature_graph.py:50-123 +
        common/nuc_feature.py).  labels int32 [H, W] (0 = background, values in [0, max_label]), gray uint8 [H, W], H * W < 2^31.
        Returns (features f32 [n, 16], centroids f32 [n, 2], kept_labels int32 [n], info int32 [n, 4] or None); reads n on the host.

        1.  remove_small_objects(mask, min_size) of skimage 0.15 on a label image: labels with fewer than min_size pixels in the whole
            image become background; no relabelling, the connectivity is irrelevant.
        2.  One row per surviving label, ascending; a label of several pieces is one row.  centroid = (mean row, mean column) of its
            pixels; bbox = (r0, c0, r1 + 1, c1 + 1).
        3.  Crop (quirk): rows r0 .. r1 + 1, columns c0 .. c1 + 1, clipped at the image edge; crop mask = pixels of ANY surviving
            label (neighbours' pixels count as foreground in everything below).
        4.  mean_im_out = sum fg / (n_fg + 1e-8); diff = |mean_im_out - sum bg / (n_bg + 1e-8)|; var_im = population variance of fg;
            skew_im = m3 / m2^1.5 (biased), 0 when m2 = 0 -- over gray in the crop.
        5.  mean_ent = mean over the crop mask of skimage.filters.rank.entropy(gray, disk(3)): per pixel the histogram of the <= 29
            in-image values with dy^2 + dx^2 <= 9, -sum p log2 p.
        6.  GLCM of gray * mask with offset (0, +1), 256 levels, not symmetric: row and column 0 dropped, normalised by the remaining
            total (0 -> 1); dissimilarity sum P |i - j|, homogeneity sum P / (1 + (i - j)^2), ASM sum P^2, energy sqrt(ASM).
        7.  Contour (quirk, cv2.findContours(RETR_TREE)[0][0]): among the 8-connected components of the crop mask that are top-level
            -- the background pixel left of the raster-first pixel is 4-connected to the outside (the crop is padded by background) --
            the one whose raster-first pixel comes last.  It may be a fragment of a neighbour.
        8.  Suzuki 8-connected border following from that pixel, CHAIN_APPROX_SIMPLE vertices (direction changes; the start kept).
        9.  area = |shoelace| (0 below 3 vertices); hull_area of the vertices (0 -> 1); solidity = area / hull_area; perimeter = closed
            polygon length with float32 edge lengths summed in double; with more than 4 vertices fitEllipse gives major = max, minor =
            min of the box sizes and orientation = the box angle, otherwise 1, 1, 0; eccentricity = sqrt(1 - (minor / major)^2).
        10. fitEllipse = OpenCV 4.1 fitEllipseNoDirect: least squares [-x^2, -y^2, -xy, x, y] g = const on centred points (min-norm),
            centre from [[2 g0, g2], [g2, 2 g1]] c = (g3, g4), refit [(x-cx)^2, (y-cy)^2, (x-cx)(y-cy)] h = 1, theta = -atan2(h2,
            h1 - h0) / 2, t = h2 / sin(-2 theta) (h1 - h0 when |h2| <= 1e-8), radii sqrt(2 / |h0 + h1 -+ t|) (when > 1e-8), box (2 r2, 2 r3),
            swapped with angle 90 + theta in degrees when the width exceeds the height, else angle 0.  Directions whose singular value
            is below 1e-6 of the largest are dropped (OpenCV perturbs such point sets instead: not pinned).
        11. Columns: mean_im_out, diff, var_im, skew_im, mean_ent, glcm_dissimilarity, glcm_homogeneity, glcm_energy, glcm_ASM,
            eccentricity, area, majoraxis_length, minoraxis_length, perimeter, solidity, orientation.
        info (with_info): start row, start column of the contour in the crop, its vertex count, path (0 LDS, 1 global workspace).
        Pixels with a label outside [0, max_label] raise ValueError (the reference raises for negative labels)."""
        raise NotImplementedError

    def label_components(self, image, connectivity, min_size, want_sizes=False):
        """Connected components of one image (F5, in front of nucleus_features; csrc/label.hip).  image: [H, W] of a 1-, 2-, 4- or 8-byte
        integer type or bool, any strides, H * W < 2^31.  Returns (labels int32 [H, W], n, sizes int32 [n] or None); reads n on the host,
        which is the only host read.

        1.  0 is background; every other value, negative ones included, is foreground.
        2.  Two foreground pixels belong to one component iff a path of neighbouring pixels that ALL CARRY THE SAME VALUE joins them:
            connectivity 1 = the 4 edge neighbours, connectivity 2 = the 8 neighbours.  A bool or 0/1 image gets ordinary
            connected-component labelling; an integer image has every value split into its connected pieces, and adjacent pixels of
            different values are never merged.
        3.  labels: 0 for background, components numbered 1..n by the raster (row-major) order of each component's first pixel -- for a
            binary image scipy.ndimage.label's output with the matching structuring element, bit for bit.
        4.  min_size > 0: components of fewer than min_size pixels become background and take no number; the survivors are still
            numbered 1..n by first pixel (skimage.morphology.remove_small_objects on the boolean image, then labelling).
        5.  want_sizes: sizes[k - 1] = pixels of component k.
        6.  H * W = 0 gives empty labels and n = 0; an all-background image zeros and n = 0.
        The result is a pure function of the input: no launch's outcome depends on the order in which workgroups run."""
        raise NotImplementedError

    def distance_transform(self, image, sites_nonzero, d2max, want_nearest=False):
        """Exact Euclidean distance transform of one image with the nearest site of every pixel (F6, beside label_components;
        csrc/edt.hip).  image: [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides, H <= 32767 and W <= 32767 (ValueError
        otherwise: a squared distance must fit int32).  Returns (dist2 int32 [H, W], nearest int32 [H, W] or None); no host read.

        1.  A site is a pixel with value != 0 (sites_nonzero) or value == 0 (not sites_nonzero).
        2.  dist2[p] = the smallest dy^2 + dx^2 from p to a site; 0 on sites.  Integer arithmetic only: every value is exact.
        3.  nearest[p] = the raster index y' * W + x' of the site that attains it; ties go to the SMALLEST raster index.  Only computed
            with want_nearest.
        4.  An image without a site: dist2 = EDT_INF (2^31 - 1) and nearest = -1 everywhere.
        5.  d2max >= 0: pixels whose true dist2 exceeds d2max report EDT_INF and -1, all others are exact; d2max < 0: no bound.
        6.  Distances are measured to sites inside the image only (scipy's convention): the image border is not a site.
        7.  H * W = 0 gives empty outputs.
        The result is a pure function of the input.  Cost per pixel grows with the distance to its nearest site, capped by
        sqrt(d2max): O(W) per pixel where a row's columns hold no site at all."""
        raise NotImplementedError

    def geodesic_transform(self, seeds, within, a, b, connectivity, dmax, want_nearest=False):
        """Geodesic distance transform of one image with the nearest seed of every pixel (F7, beside distance_transform;
        csrc/geodesic.hip): distance is measured along paths that stay inside a domain.  Returns (dist int32 [H, W], nearest int32
        [H, W] or None).  All arithmetic is integer: every result is exact and a pure function of the input.

        1.  seeds, within: [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is read.  The domain is
            D = {within != 0} u {seeds != 0}: a seed always belongs to it.  within = None: every pixel.
        2.  An axial step between two 4-neighbours that are both in D costs a, a diagonal step between two corner neighbours that are
            both in D costs b; b == 0: no diagonal steps.  1 <= a <= b <= 2a or b == 0 (ValueError).  connectivity 2: a diagonal step
            needs only its two end points in D.  connectivity 1: the diagonal step (y, x) -> (y + dy, x + dx) also needs (y + dy, x)
            or (y, x + dx) in D -- a path never squeezes through a corner contact.  So the reached pixels are exactly the pixels of
            those ``connectivity``-components of D that hold a seed (with b == 0: of the connectivity-1 components).
        3.  dist[p] = the smallest path cost from any seed pixel, 0 on seeds; nearest[p] = the raster index y' * W + x' of the seed
            that attains it, ties to the SMALLEST raster index (distance_transform's rule).  A domain pixel that no seed reaches and
            every pixel outside D: GEO_INF (2^31 - 1) and -1.  nearest is only unpacked with want_nearest.
        4.  dmax >= 0: pixels whose true cost exceeds dmax report GEO_INF and -1, all others are exact; dmax < 0: no bound.
        5.  (b or a) * H * W < 2^31, so that no path cost overflows int32 (ValueError otherwise, nothing is launched).  H * W = 0 gives
            empty outputs.
        Why a parallel relaxation gives exactly this: with key = (dist, seed index) packed into 64 bits, the definition is the unique
        fixed point of key[p] = min(key0[p], min over steps q -> p of (key[q].dist + cost, key[q].seed)) -- the predecessor of p on a
        shortest path from the winning seed carries the same seed, costs are positive, keys only decrease -- whatever the order of the
        updates.  Rounds are launches (one 64 x 64 tile per workgroup, relaxed to its own fixed point in LDS; a tile whose keys and
        halo did not move since its last run costs one load), and the loop is here: the host reads the number of tiles that moved in
        the last round of a batch of GEO_FIRST_BATCH (8), then twice as many up to GEO_MAX_BATCH (64), rounds.  Host reads: one per
        batch.  R = 2 + the tile edges that the longest shortest path crosses rounds are needed (the last one moves nothing), so: one
        read when it crosses at most six (a bound of a few pixels, even where a porous domain makes the path weave across an edge),
        otherwise the smallest k with 8 (2^k - 1) >= R (k <= 3), and one more per 64 rounds beyond 56.
        Worst case: a serpentine corridor over a whole image crosses a tile edge per turn and needs hundreds of rounds."""
        raise NotImplementedError

    def morph_reconstruct(self, marker, mask, connectivity, by_erosion=False):
        """Grayscale morphological reconstruction (Vincent 1993) of one image (F8, beside geodesic_transform; csrc/reconstruct.hip).
        Returns R int32 [H, W], contiguous.  All arithmetic is integer comparison: every result is exact and a pure function of the
        input.

        1.  marker, mask: int32 [H, W] of the same shape, any strides, H * W < 2^31; the whole int32 range is allowed.
        2.  connectivity 1: the neighbours of a pixel are its 4 edge neighbours; 2: its 8 neighbours (ValueError otherwise).  With
            connectivity 1 a diagonal corner contact does not conduct, with connectivity 2 it does.
        3.  By dilation: R0 = min(marker, mask) pointwise -- a marker above the mask is clamped, not refused, so nothing is read on
            the host -- and R is the fixed point of R[p] = min(mask[p], max(R[p], max over the neighbours q of R[q])) that is reached
            from R0 by raising values.
        4.  Equivalently R[p] = the largest, over pixels q and over paths of neighbours from q to p (q = p included), of
            min(R0[q], the smallest mask value on the path).  It is unique; R0 <= R <= mask.
        5.  by_erosion: the dual (min and max exchanged), computed as R = ~dilation(~marker, ~mask) with BITWISE NOT, which reverses
            the order of all of int32 and cannot overflow (negation can); mask <= R <= max(marker, mask).
        6.  H * W = 0 gives an empty output.
        Why a parallel relaxation gives exactly this: values only increase, and every stored value is the value of a real path (item
        4), whatever the order of the updates.  Rounds are launches (one 64 x 64 tile per workgroup, relaxed to its own fixed point
        in LDS by forward and backward scans along rows, then columns; a tile that already equals its mask costs one load, a tile
        whose values and halo did not move since its last run nothing), and the loop is here, on geodesic_transform's schedule: the
        host reads the number of tiles that moved in the last round of a batch of GEO_FIRST_BATCH (8), then twice as many up to
        GEO_MAX_BATCH (64), rounds.  Host reads: one per batch.  R = 2 + the tile edges crossed by the longest path along which a
        value has to travel rounds are needed (the last one moves nothing).  Worst case: a serpentine plateau over a whole image
        crosses a tile edge per turn and needs hundreds of rounds.  ``reconstruct_rounds`` holds the rounds launched by the last
        call."""
        raise NotImplementedError

    def watershed_flood(self, height, seeds, within, a, b, connectivity):
        """Seeded watershed flood of one height image (F9, beside morph_reconstruct; csrc/watershed.hip): water rises from the seeds,
        and every pixel learns the level at which it is first wetted and the seed whose water wets it, so that the cut between two
        seeds falls on the pass (the neck) between their basins.  Returns (level int32 [H, W], source int32 [H, W]).  The result is
        defined without reference to any processing order, all arithmetic is integer: every result is exact and a pure function of
        the input.

        1.  height: int32 [H, W], any strides, the whole int32 range allowed.  seeds, within: as items 1 and 2 of geodesic_transform
            -- [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides, only "is zero" is read.  The domain is
            D = {within != 0} u {seeds != 0}; within = None: every pixel.  The steps -- axial and diagonal, their costs a and b
            (b == 0: no diagonal steps; 1 <= a <= b <= 2a otherwise, ValueError) and the connectivity-1 corner rule -- are exactly
            geodesic_transform's.  (b or a) * H * W < 2^31 (ValueError otherwise, nothing is launched).
        2.  The flood key K[p] = (alt, len), compared lexicographically.  A seed has K = (INT32_MIN, 0) and never changes.  Extending
            a path with key (alt, len) by an allowed step of cost w onto a non-seed pixel p gives (height[p], 0) if height[p] > alt
            -- the water rises onto p -- and (alt, len + w) otherwise -- it runs level or downhill; len is the way travelled since
            the last rise.  K[p] is the smallest key over all paths from any seed.  alt is the height image with its unmarked
            basins filled to their lowest pass.
        3.  The parent of a reached non-seed pixel p: among the allowed steps q -> p with q reached, the q that minimises the triple
            (extend_p(K[q]), K[q], raster index of q).  The first component's minimum is K[p], so the parent offers p its key; among
            those offers the earliest-flooded neighbour wins, then the smallest index.  K[parent] < K[p] strictly, so the parents
            form a forest rooted at the seeds.  A rim pixel thereby follows the steepest descent inward; it does not tie between all
            of its lower neighbours.
        4.  source[p] = the raster index of the root of p; a seed is its own root; -1 outside D and on domain pixels that no seed
            reaches.  level[p] = alt of K[p] on reached non-seed pixels and height[p] everywhere else.  H * W = 0 gives empty
            outputs.
        Why a parallel relaxation gives exactly this: the extension is order-preserving and strictly increasing, so K is the unique
        fixed point of K[p] = min over steps q -> p of extend_p(K[q]); every key ever stored is the key of a real path and keys only
        decrease from "not reached", whatever the order of the updates.  Rounds are launches on geodesic_transform's schedule (one
        64 x 64 tile per workgroup, relaxed to its own fixed point in LDS; the host reads the number of tiles that moved in the last
        round of a batch of GEO_FIRST_BATCH (8), then twice as many up to GEO_MAX_BATCH (64), rounds).  Then one launch evaluates
        item 3 and pointer jumping (ptr[p] = ptr[ptr[p]], in place) resolves the roots: the host reads the number of pixels that moved
        in the last jump of a batch of WS_JUMP_BATCH (8) and stops when it is 0; 31 jumps always suffice.  Host reads: one per batch
        of rounds and one per batch of jumps -- two when the flood crosses at most six tile edges and no parent chain exceeds 128
        pixels.  Worst case: a serpentine valley over a whole image crosses a tile edge per turn, needs hundreds of rounds and the
        logarithm of its length in jumps.  ``watershed_rounds`` and ``watershed_jumps`` hold the launches of the last call."""
        raise NotImplementedError

    def bgr_to_gray(self, bgr):
        """cv2.cvtColor(img, COLOR_BGR2GRAY) on uint8 [H, W, 3]: (1868 B + 9617 G + 4899 R + 8192) >> 14 -> uint8 [H, W]."""
        raise NotImplementedError

    def stain_separate(self, image, order, lut, m, planes):
        """Colour deconvolution of one stained tile in fixed point (F10, in front of the foreground map; csrc/stain.hip; Ruifrok and
        Johnston 2001).  Returns uint8 [popcount(planes), H, W], contiguous; no host read.  All arithmetic is integer: every result is
        exact and a pure function of the input.

        1.  image: uint8 [H, W, 3], any strides, H * W < 2^31.  order 0: the channels are B, G, R (cv2, bgr_to_gray); 1: R, G, B.
        2.  lut: 256 integers, the optical density of a channel value in 1/1024 of a natural-log unit:
            lut[v] = floor(1024 ln(255 / max(v, 1)) + 0.5), from 0 (v = 255) to 5674 (v = 0 or 1).  Entries outside [0, 5674] are
            refused (ValueError).
        3.  m: 3 x 3 integers, m[c][s] = rint(4096 inv(S)[c][s]) with c = 0 R, 1 G, 2 B, where the rows of S are the unit-normalised
            OD vectors of the three stains: OD = C S, so C = OD inv(S).
        4.  C_s = lut[R] m[0][s] + lut[G] m[1][s] + lut[B] m[2][s] in int32.  sum_c |m[c][s]| * 5674 < 2^31 - 2^15 for every s
            (ValueError otherwise, nothing is launched): neither the sum nor the rounding term below can overflow.
        5.  out_s = clamp((C_s + 2^15) >> 16, 0, 255) with an arithmetic shift (round half up, also below zero).  One level is 1 / 64
            of a unit of natural-log concentration: 2^-16 * 1024 * 4096 = 64 levels per unit.
        6.  planes: a bit mask, bit s = stain s is wanted, 1..7 (ValueError otherwise); the output holds the wanted planes in ascending
            stain order.
        7.  H * W = 0 gives an empty output.
        Error against the real-number formula 64 ln(255 / max(v, 1)) inv(S): at most 64 (a_s / 2048 + 3 * 5.55 / 8192) + 1/2 levels
        with a_s = sum_c |inv(S)[c][s]| -- the table's rounding times the matrix, the matrix's rounding times the largest OD (5.55),
        and the final rounding; 0.76 for a_s = 4."""
        raise NotImplementedError

    def histogram_u8(self, image, within=None):
        """256-bin histogram of one uint8 image (F10; csrc/stain.hip).  Returns hist int32 [256] on the device; no host read.

        1.  image: uint8 [H, W], any strides, H * W < 2^31, so every count fits int32.
        2.  within: None or [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is read.
        3.  hist[v] = the number of pixels p with image[p] == v and (within is None or within[p] != 0).  sum(hist) = the number of
            selected pixels.
        4.  H * W = 0, or a within that selects nothing, gives zeros.
        Integer counts: the result does not depend on the order of the atomic adds.  A workgroup counts ``histogram_chunk`` (16384)
        consecutive pixels in LDS and flushes its non-empty bins once."""
        raise NotImplementedError

    def od_moments(self, image, order, lut, od_min, within=None):
        """The first and second moments of the optical densities of a tile's stained pixels (stain estimation, Macenko et al. 2009;
        csrc/stain.hip).  Returns int64 [10] on the device; no host read.  All arithmetic is integer: the result is exact and does not
        depend on the order of accumulation.

        1.  image, order, lut: as stain_separate -- uint8 [H, W, 3], any strides, H * W < 2^31; order 0: B, G, R, 1: R, G, B; lut: 256
            integers in [0, 5674] (ValueError otherwise).
        2.  within: as histogram_u8 -- None or [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is
            read.
        3.  od_min: an integer in 0..5674 (ValueError otherwise, before any launch).
        4.  With o = (lut[R], lut[G], lut[B]) a pixel is *selected* iff (within is None or within is non-zero there) and
            lut[R] >= od_min and lut[G] >= od_min and lut[B] >= od_min.
        5.  out = [n, sum oR, sum oG, sum oB, sum oR^2, sum oR oG, sum oR oB, sum oG^2, sum oG oB, sum oB^2] over the selected pixels.
            Everything fits int64: 5674^2 * 2^31 < 2^63.
        6.  H * W = 0, or nothing selected, gives zeros.
        A lane adds at most 64 pixels in uint32 (64 * 5674^2 < 2^32); from the wave's reduction on the sums are 64 bits wide, and a
        workgroup (``scan_chunk`` = 16384 consecutive pixels) adds its ten sums to the result with one 64-bit global atomic each."""
        raise NotImplementedError

    def angle_histogram(self, image, order, lut, od_min, basis, dirs, within=None):
        """The histogram of the angles of a tile's stained pixels in a plane of optical-density space (stain estimation; csrc/stain.hip).
        Returns int32 [K + 1] on the device, K = ANGLE_BINS = 1024; no host read.  All arithmetic is int32 and exact; no transcendental
        function runs on the device.

        1.  image, order, lut, od_min, within and the selection: exactly as od_moments.
        2.  basis: 2 x 3 integers E[j][c], c = 0 R, 1 G, 2 B, |E[j][c]| <= 4096 and sum_c |E[j][c]| <= 7095 (= ceil(4096 sqrt 3)) for
            each j (ValueError otherwise): 4096 times two unit vectors.
        3.  For a selected pixel p_j = (sum_c o_c E[j][c] + 2^11) >> 12, an arithmetic shift in int32: |sum| <= 5674 * 7095 < 2^26,
            so |p_j| <= 9829.
        4.  dirs: (K - 1) x 2 integers (c_k, s_k), k = 1..K-1, each in [-16384, 16384] (ValueError otherwise); the host's table
            (nuclei.ANGLE_DIRS) is (rint(16384 cos t_k), rint(16384 sin t_k)) with t_k = -pi/2 + k pi / K.
        5.  A selected pixel with p_1 <= 0 is not binned: it adds one to out[K], the *skipped* counter.
        6.  Every other selected pixel adds one to out[b], b = #{k : c_k p_2 - s_k p_1 >= 0}, 0 <= b <= K - 1.
            |c_k p_2 - s_k p_1| <= 16384 * 2 * 9829 < 2^31.
        7.  The refusal that makes a binary search equal the count: c_k > 0 for every k and c_k s_{k+1} - s_k c_{k+1} > 0 for
            consecutive k (ValueError otherwise, before any launch; the library repeats it) -- the directions lie in the open right
            half plane and their angles increase strictly.  For p_1 > 0 the sign of c_k p_2 - s_k p_1 is that of
            sin(angle(p) - angle(d_k)) with both angles in (-pi/2, pi/2), so {k : ... >= 0} = {k : angle(d_k) <= angle(p)} is a prefix
            and b is its size; the kernel finds it in 10 steps over the table in LDS.  A table that is not of this kind is refused, not
            counted.
        8.  H * W = 0, or nothing selected, gives zeros.
        A workgroup counts ``scan_chunk`` consecutive pixels into 8 copies of the K + 1 counters in LDS (lane l on copy l mod 8,
        bin-major; a run of equal bins among the 16 pixels a lane takes at a time is one add) and adds its non-empty bins to the result with one global atomic
        each."""
        raise NotImplementedError

    def concentration_histogram(self, image, order, lut, od_min, m, within=None):
        """The histograms of the concentrations of the first two stains over a tile's stained pixels (stain normalisation, Macenko et
        al. 2009; csrc/stain.hip), without writing any plane.  Returns int32 [2 B] on the device, B = CONC_BINS = 512; no host read.
        All arithmetic is int32 and exact; the counts do not depend on the order of the adds.

        1.  image, order, lut, od_min, within and the selection: exactly as od_moments.
        2.  m: exactly as stain_separate, items 3-4 -- 3 x 3 integers, m[c][s] = rint(4096 inv(S)[c][s]), c = 0 R, 1 G, 2 B, with
            sum_c |m[c][s]| * 5674 < 2^31 - 2^15 for every s (ValueError otherwise, before any launch; the library repeats it).
        3.  For a selected pixel and s = 0, 1: C_s = lut[R] m[0][s] + lut[G] m[1][s] + lut[B] m[2][s] in int32.
        4.  b_s = clamp((C_s + 2^14) >> 15, 0, B - 1) with an arithmetic shift (round half up, also below zero).  One level is 1 / 128
            of a unit of natural-log concentration: 2^-15 * 1024 * 4096 = 128 levels per unit; bin B - 1 = 511 collects everything
            from 3.99 units up, bin 0 everything below 1 / 256.
        5.  Every selected pixel adds one to out[b_0] and one to out[B + b_1]: both halves sum to n, the number of selected pixels.
        6.  H * W = 0, or nothing selected, gives zeros.
        The third body of the scan that od_moments and angle_histogram share: a workgroup counts ``scan_chunk`` consecutive pixels into
        8 copies of the 2 B counters in LDS (lane l on copy l mod 8, bin-major; a run of equal bins of one stain among the 16 pixels a
        lane takes at a time is one add) and adds its non-empty bins to the result with one global atomic each."""
        raise NotImplementedError

    def od_recolor(self, image, order, lut, a, exp_lut):
        """A linear map in optical-density space, from a colour tile to a colour tile (stain normalisation; csrc/stain.hip).  Returns
        uint8 [H, W, 3], contiguous, in the channel order of the input; no host read.  All arithmetic is int32 and exact; no
        transcendental function runs on the device.

        1.  image, order, lut: as stain_separate -- uint8 [H, W, 3], any strides, H * W < 2^31; order 0: B, G, R, 1: R, G, B; lut: 256
            integers in [0, 5674] (ValueError otherwise).
        2.  a: 3 x 3 integers, a[c][d] = rint(4096 A[c][d]) with c the input and d the output channel (0 R, 1 G, 2 B): OD_out = OD_in A.
            sum_c |a[c][d]| * 5674 < 2^31 - 2^11 for every d (ValueError otherwise, before any launch; the library repeats it):
            neither the sum nor the rounding term below can overflow.
        3.  exp_lut: EXP_LUT_LEN = 6386 integers, exp_lut[k] = floor(255 exp(-k / 1024) + 0.5) (nuclei.EXP_LUT): 255 at k = 0, first 0
            at k = 6385.  A table of another length, with an entry outside [0, 255], that rises anywhere, or that does not start at
            255 and end at 0 is refused (ValueError, before any launch; the library repeats it).
        4.  O_d = lut[v_R] a[0][d] + lut[v_G] a[1][d] + lut[v_B] a[2][d] in int32, in 1 / (1024 * 4096) of a natural-log unit.
        5.  k_d = clamp((O_d + 2^11) >> 12, 0, 6385) with an arithmetic shift: the optical density in 1/1024, rounded half up.
        6.  out_d = exp_lut[k_d]; the output pixel holds (out_B, out_G, out_R) for order 0 and (out_R, out_G, out_B) for order 1.
        7.  H * W = 0 gives an empty output.
        With a = 4096 I the map is the identity except 0 -> 1: exp_lut[lut[v]] = v for v = 1..255, and lut[0] = lut[1].
        Error against the real-number formula 255 exp(-(ln(255 / max(v, 1)) A)_d): with delta_d = (sum_c |A[c][d]| / 2 + sum_c o_c
        / 8192 + 1 / 2) / 1024 -- the table's rounding through the column, the matrix's rounding times the pixel's densities o_c (in
        natural-log units), the rounding of k -- at most 255 exp(-O_d) (exp(delta_d) - 1) + 1/2 levels.
        A lane takes 4 pixels as three dwords and stores three dwords (bytes on an unaligned base and on the last 1-3 pixels); both
        tables sit in LDS, the exponential one as bytes; the matrix stays in scalar registers.  The exponential table reaches the
        device as angle_histogram's directions do: small launches carry it as kernel arguments into a workspace."""
        raise NotImplementedError

    def resample_u8(self, image, size, mode):
        """The pixel size of one uint8 plane or interleaved tile (F21; csrc/resample.hip).  Returns uint8 [H2, W2] or [H2, W2, 3],
        contiguous; one launch, no workspace, no host read.  Below n is a source side and m the output side of the same axis; the axes
        are independent.

        1.  Sides.  image: uint8 [H, W] or [H, W, 3], any strides; size = (H2, W2); 1 <= n, m <= 32767 (``RESAMPLE_MAX_SIDE``,
            cgc_resample_max_side()) on both axes, anything else is a ValueError before any launch (the library: CGC_EINVAL, nothing
            launched).  A source with H * W = 0 is a ValueError.  size == image.shape[:2] is an ordinary case and returns an equal
            copy in every mode.
        2.  Geometry.  Pixel centres sit at half-integers (cv2, PIL, scipy.ndimage.zoom(grid_mode=True)).  Output index d samples the
            source at s = ((2 d + 1) n - m) / (2 m), clamped to [0, n - 1] (the border is replicated): with num = clamp((2 d + 1) n -
            m, 0, 2 m (n - 1)), i0 = floor(num / (2 m)), i1 = min(i0 + 1, n - 1) and the fraction numerator f = num - i0 * 2 m over
            2 m.  (2 d + 1) n reaches 65533 * 32767 = 2^31 - 163837: it comes within 2 * 10^5 of the int32 limit and is computed in
            uint32, as is 2 m (n - 1) < 2^31.
        3.  mode 'linear'.  out = floor((2 S + D) / (2 D)) with S = sum over the four neighbours of p * wy * wx, wx in {2 W2 - fx, fx},
            wy in {2 H2 - fy, fy}, D = 4 H2 W2: exact rational bilinear interpolation with ONE rounding, half up, in 64 bits (255 *
            2^32 < 2^40).  It does no prefiltering, so it aliases below half size, where 'area' is the mode to use.  cv2.resize's
            INTER_LINEAR works with 11-bit fixed-point weights and can differ from it by one level (the documented reason for stating
            the arithmetic here; not a tested claim).
        4.  mode 'area'.  Requires H2 <= H and W2 <= W (ValueError otherwise).  Output index d owns the source interval [d n / m,
            (d + 1) n / m); in units of 1 / m of a pixel source pixel i has weight o_i = min((d + 1) n, (i + 1) m) - max(d n, i m),
            positive for i = floor(d n / m) .. floor(((d + 1) n - 1) / m); the weights sum to n.  out = floor((2 S + D) / (2 D)) with
            S = sum p * oy * ox and D = H W.  For integer factors this is the rounded block mean.
        5.  Colour.  The three channels of [H, W, 3] are resampled independently, each by items 2 to 4; the tile is read interleaved.
        8.  Purity.  Every result is a pure function of the input and bit-identical from call to call: integers only, no atomics, no
            float arithmetic.
        (Items 6 and 7 are resample_labels'.)  A lane produces 4 adjacent output pixels and stores them as one dword (three for a
        tile); the groups start where the row's address is a multiple of 4, so only the first and last 1-3 pixels of a row's share
        are written as bytes.  'area' walks a box with one lane: neighbouring lanes own neighbouring boxes."""
        raise NotImplementedError

    def resample_labels(self, labels, size, mode):
        """The pixel size of one label image (F21; csrc/resample.hip).  Returns [H2, W2] of the input's dtype, contiguous; one launch,
        no workspace, no host read.  n, m and the geometry as resample_u8.

        1.  Sides.  labels: bool or a 1-, 2-, 4- or 8-byte integer type, [H, W], any strides; size = (H2, W2); 1 <= n, m <= 32767 on
            both axes, a source with H * W = 0 included in the refusal (ValueError before any launch; the library: CGC_EINVAL, nothing
            launched).  size == labels.shape is an ordinary case and returns an equal copy in both modes.
        2.  Geometry.  Pixel centres at half-integers, exactly as resample_u8's item 2; (2 d + 1) n is computed in uint32.
        6.  mode 'nearest'.  out[d] = src[floor((2 d + 1) n / (2 m))] per axis; the index is always in range.  An element of 1, 2, 4
            or 8 bytes is copied as it is.  Upscaling by an integer k is np.repeat along both axes.
        7.  mode 'majority'.  Requires H2 <= H, W2 <= W, H <= 8 H2 and W <= 8 W2 (``RESAMPLE_LABELS_MAX_FACTOR``,
            cgc_resample_labels_max_factor(); ValueError otherwise).  Among the source pixels of the box of resample_u8's item 4 the
            output takes the VALUE with the largest total weight sum oy * ox; the value 0 is a candidate like any other.  Ties go to the
            smallest value: values compare as integers of the dtype (int8 .. int64 signed, uint8 unsigned), bool as 0 / 1.  A box
            spans at most 9 pixels per axis, and its weights sum to H W < 2^30.
        8.  Purity.  A pure function of the input, bit-identical from call to call: integers only, no atomics, no float arithmetic.
        (Items 3 to 5 are resample_u8's.)  The library takes the element size; the unsigned order of uint8 and bool is its mode
        CGC_RESAMPLE_MAJORITY_UNSIGNED.  A box of one value -- the inside of a nucleus, the background -- is decided by one walk over
        it; a mixed box weighs every distinct candidate with a second walk, in registers."""
        raise NotImplementedError

    def binomial_smooth(self, image, radius):
        """Separable binomial smoothing of one uint8 image (F10; csrc/smooth.hip).  Returns uint8 [H, W], contiguous; no host read.

        1.  image: uint8 [H, W], any strides, H * W < 2^31.  radius r: an integer in 0..5 (ValueError otherwise).
        2.  Weights w_k = C(2 r, k), k = 0..2 r; they sum to 4^r.  The kernel w w^T has standard deviation sqrt(r / 2) per axis
            (1.58 at r = 5); larger blurs are repeated calls.
        3.  out[y, x] = (sum_i sum_j w_i w_j image[clamp(y + i - r, 0, H - 1), clamp(x + j - r, 0, W - 1)] + 2^(4 r - 1)) >> 4 r: the
            border is replicated, and there is ONE rounding (half up), after both passes.  Everything is exact in int32: 255 * 2^20 <
            2^31.  r = 0 is a copy (no rounding term).
        4.  H < r or W < r are ordinary shapes: the clamp covers them.  H * W = 0 gives an empty output."""
        raise NotImplementedError

    def window_sums(self, image, radius, within=None):
        """The number, the sum and the sum of squares of the pixels in a square window around every pixel (F14, behind the stain
        plane; csrc/window.hip): the primitive under every local statistic.  Returns (n int32, S int32, Q int64), each [H, W] and
        contiguous; no host read.

        1.  image: uint8 [H, W], any strides, H * W < 2^31.  radius r: an integer in 0..WINDOW_MAX_RADIUS = 127 (ValueError otherwise;
            the library returns CGC_EINVAL and launches nothing).
        2.  The window of pixel (y, x) is rows y - r .. y + r and columns x - r .. x + r, CLIPPED to the image: nothing is replicated
            or reflected, border windows are smaller, and r may exceed either side.
        3.  within: None or [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is read.  A pixel of the
            window is *counted* iff within is None or within is non-zero there.  The centre pixel has no special role: outputs are
            defined at every pixel, selected or not.
        4.  n = the number of counted pixels, S = the sum of their values, Q = the sum of their squares.  Bounds: n <= 255^2 = 65 025,
            S <= 255 n = 16 581 375, Q <= 255^2 n = 4 228 250 625, which is above 2^31 and below 2^32: Q is int64.
        5.  H * W = 0 gives empty outputs; a within that selects nothing gives zeros.
        6.  One launch, no atomics, integer arithmetic: bit-identical from call to call.
        Widths inside the kernel ("Window sums and local thresholds"): a workgroup scans the per-column sums of 1024
        columns in uint32.  The scans of n and S are exact (<= 1024 * 255 and 1024 * 255^2); the scan of Q passes 2^32 and wraps, and a
        window's Q, a difference of two entries and itself below 2^32, is exact modulo 2^32.  A tile is ``window_tile_rows`` (16) rows
        by ``window_strip_cols(r)`` (1024 - 2 * (r rounded up to a multiple of 4)) columns."""
        raise NotImplementedError

    def local_threshold(self, image, radius, k64, offset, floor, within=None):
        """The local mean / Niblack threshold of one uint8 image, fused with the window sums it needs (F14; csrc/window.hip, the same
        kernel as window_sums with another epilogue: n, S and Q are never written to memory).  Returns uint8 [H, W] of 0 / 1,
        contiguous; no host read.

        1.  image, radius, within, n, S, Q: exactly as window_sums, items 1-4.
        2.  k64: an integer in -128..128, 64 times Niblack's k, so |k| <= 2.  offset c: an integer in -255..255.  floor: an integer in
            -1..255, -1 meaning no floor.  (ValueError otherwise, before any launch; the library returns CGC_EINVAL.)
        3.  With v the pixel's own value -- read whatever `within` says there -- m = S / n and s^2 = Q / n - m^2, a pixel is
            foreground iff n >= 1 and v > floor and v > m + k s + c.  A pixel outside `within` is still decided, from the counted
            pixels of its window.
        4.  The decision is made in exact integers, never in floating point.  L = 64 (n v - S - c n), D = n Q - S^2 >= 0 (n^2 times
            the variance).  k64 >= 0: foreground iff L > 0 and L^2 > k64^2 D.  k64 < 0: foreground iff L > 0, or (L = 0 and D > 0),
            or (L < 0 and L^2 < k64^2 D).
        5.  Equality is not foreground: in the 1 x 5 image [0, 0, 0, 0, 200] with r = 4, c = 0 and no floor the last pixel has
            m + 2 s = v exactly; it is 0 at k64 = 128 and 1 at k64 = 127.  A constant window has D = 0: c = 0 gives nothing, c = -1
            everything.
        6.  Everything fits int64: |L| <= 64 * 2 * 255 * 65 025 < 2^31.0, so L^2 < 2^62.0; D <= n^2 * 255^2 / 4 <= 6.874e13, so
            k64^2 D <= 1.13e18 < 2^63 = 9.22e18.
        7.  H * W = 0 gives an empty output; where nothing is counted (n = 0) the pixel is background."""
        raise NotImplementedError

    def flat_morphology(self, image, kind, radius, op, within=None, other=None, epilogue=None):
        """Erosion, dilation or morphological gradient of one uint8 image over a flat structuring element (F15, on the stain plane,
        beside window_sums; csrc/morph.hip): the min / max filter under opening, closing, the top-hats and reconstruction's markers.
        Returns uint8 [H, W], contiguous; no host read.

        1.  image: uint8 [H, W], any strides, H * W < 2^31.  radius r: an integer in 0..MORPH_MAX_RADIUS = 63 (ValueError otherwise;
            the library returns CGC_EINVAL and launches nothing).  kind: 'square', 'disk' or 'diamond'.
        2.  The footprint is the set of offsets (dy, dx) with |dy| <= r and |dx| <= w(dy): w = r for the square, w = r - |dy| for the
            diamond, and for the disk the largest integer with w^2 + dy^2 <= r^2 -- dx^2 + dy^2 <= r^2, skimage's disk(r), decided
            in integers, never with a floating-point root.  r = 0 is the single pixel for every kind.
        3.  The footprint is CLIPPED to the image: nothing is replicated or reflected, border footprints are smaller, and r may exceed
            either side.
        4.  within: None or [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is read.  A pixel of the
            footprint is *counted* iff it lies in the image and within is None or non-zero there.  The centre pixel has no special
            role: outputs are defined at every pixel, selected or not.
        5.  op 'erode': the minimum over the counted pixels, and 255, the neutral value, where none is counted.  'dilate': the
            maximum, and 0 where none is counted.  'gradient': maximum minus minimum, both found in ONE pass, and 0 where none is
            counted.  Bounds: every result lies in 0..255.
        6.  epilogue None: the result is stored.  'other_minus': max(0, other - result).  'minus_other': max(0, result - other).
            other: uint8 [H, W], any strides, read at the output pixel only (ValueError if an epilogue comes without it or it
            without an epilogue).  The white top-hat is erode, then dilate with 'other_minus' against the image; the black
            top-hat dilate, then erode with 'minus_other': two launches each and no subtraction pass.
        7.  H * W = 0 gives an empty output.
        8.  One launch, no workspace, no atomics, integer arithmetic: bit-identical from call to call.
        Inside the kernel ("Flat morphology"): only maxima are taken -- the minimum is 255 - max(255 - v), so 0 is the one
        neutral value -- over a table of run maxima M_k(y, x) = max over [x, x + 2^k) that is doubled in place in LDS; a footprint row
        costs two byte reads per pixel whatever its length.  A tile is ``morph_tile_rows`` (32) rows by ``morph_tile_cols(r)`` (256 -
        2 * (r rounded up to a multiple of 4)) columns."""
        raise NotImplementedError

    def rank_filter(self, image, kind, radius, op, q_lo=0, q_hi=0, within=None):
        """A quantile, a quantile range or the local entropy of one uint8 image over a flat footprint (F16, on the stain plane, beside
        flat_morphology; csrc/rank.hip): the order statistics of the window -- median, robust erode / dilate / gradient, the majority
        filter of a mask -- and the texture measure skimage.filters.rank.entropy.  Returns [H, W], contiguous: uint8 for 'quantile'
        and 'range', int32 for 'entropy'; no host read.

        1.  image: uint8 [H, W], any strides, H * W < 2^31.  kind: 'square', 'disk' or 'diamond'.  radius r: an integer in
            0..RANK_MAX_RADIUS = 63, for 'entropy' in 0..ENTROPY_MAX_RADIUS = 15 (ValueError otherwise; the library returns
            CGC_EINVAL and launches nothing).
        2.  The footprint is flat_morphology's, item 2: offsets (dy, dx) with |dy| <= r and |dx| <= w(dy), the widths decided in
            integers on the host; r = 0 is the single pixel.
        3.  The footprint is CLIPPED to the image: nothing is replicated, border windows are smaller.
        4.  within: None or [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is read.  A footprint
            pixel is *counted* iff it lies in the image and within is None or non-zero there.  The centre has no special role.
            Below, n is the number of counted pixels of a window and v[0] <= ... <= v[n-1] their values sorted.
        5.  op 'quantile', q_hi = q10k, an integer in 0..10000 (q_lo is not used; pass 0): the result is v[k], k = min(n - 1,
            floor(n * q10k / 10000)) in exact integers (n <= 16129: n * q10k < 2^31) -- the smallest value t whose cumulative count
            #{v <= t} exceeds k.  q10k = 0 is the minimum, 10000 the maximum, 5000 the median (the upper one when n is even).  n = 0
            gives 0.  The 1 x 2 image [10, 20] at r = 1 gives [20, 20] at 5000 and [10, 10] at 4999; in the interior of a square
            of r = 2 (n = 25) 2000 takes k = 5 and 1999 takes k = 4.
        6.  op 'range', q_lo <= q_hi (both as q10k; ValueError otherwise): v[k(q_hi)] - v[k(q_lo)] from one histogram in one pass, in
            0..255, and 0 where n = 0.  (0, 10000) is the morphological gradient.
        7.  op 'entropy': the Shannon entropy H = -sum p log2 p of the counted values in bits, in fixed point and integers only.  With
            T[c] = round(c * log2(c) * 2^16) for c = 0..961 (T[0] = T[1] = 0; every entry fits int32; the library's table,
            ``rank_entropy_term``, is the one the kernel reads), E = T[n] - sum over the non-empty bins of T[count], and the result
            is H16 = floor(E / n) as int32, 0 where n = 0.  Derived: E >= 0, and E == 0 iff one bin holds everything (T is the
            rounding of a superadditive function with integer gaps of at least 2 * 2^16 between T[a + b] and T[a] + T[b]); with m
            occupied bins |E - 2^16 n H| <= (m + 1) / 2 (m + 1 roundings of at most 1/2); hence, m <= n and the floor,
            |H16 / 2^16 - H| <= (n + 1) / (2 n 2^16) + 2^-16 <= 2^-15.
        8.  H * W = 0 gives an empty output.
        9.  One launch, NO workspace, no global atomics (the histograms are counters in LDS, and integer sums do not depend on the
            order of their terms), integer arithmetic: bit-identical from call to call.
        Inside the kernel ("Rank filters"): a wave slides one 256-bin histogram along a row of a tile of
        ``rank_tile_rows`` (8) rows by ``rank_tile_cols(r)`` (256 - 2 * (r rounded up to a multiple of 4)) columns, one pixel out
        and one in per footprint row and step, and reads the rank off a scan of the bins."""
        raise NotImplementedError

    def region_adjacency(self, labels, connectivity, value=None):
        """Region adjacency of one label image (F13, behind label_components / distance_transform; csrc/adjacency.hip): which
        regions touch, along how many pixel pairs, and how near they come.  Returns (pairs int32 [P, 2], count int32 [P], min_sum int32
        [P] or None); two host reads, the number of per-tile records and P.

        1.  labels: int32 [H, W], contiguous, H * W < 2^29 (ValueError otherwise; the library returns CGC_EINVAL and launches nothing): a
            pair's count can reach 4 H W and must fit int32.
        2.  0 is background.  Every other value is a region, negative values included.  Regions need not be connected.
        3.  A contact is an unordered pair of neighbouring pixels p, q with labels[p] != labels[q] and both non-zero.  connectivity 1:
            the horizontal and the vertical neighbour; connectivity 2: also the two diagonals.  Each pixel pair is counted once.
        4.  pairs: each row is (a, b) with a < b as signed integers; rows are sorted lexicographically and each pair appears once.
            count: the number of contacts of that pair.
        5.  value (int32 [H, W]): min_sum = the smallest value[p] + value[q] over the pair's contacts, the sum taken in 64 bits and clamped
            to the int32 range, so it is defined for every input.  Without value, min_sum is None.
        6.  H * W = 0, or no contact at all, gives empty outputs.
        7.  The outputs are a pure function of the inputs, bit for bit from call to call: internal tables are filled in any order, and
            the sort and the integer sums and minima make the outputs independent of it.
        8.  No input overflows a table silently.  The per-tile table in LDS has a fallback that is exact: a tile with more distinct
            pairs than the table folds writes one record per contact instead, and which tiles do so depends on their pixels alone.  The
            record buffers are sized from a count launch, the outputs from a count of the sorted records' distinct keys.  An image in
            which every pixel has its own label (2 H (W - 1) + ... distinct pairs, one per contact) is an ordinary input.
        The records are ordered by ``torch.sort`` of their 64-bit keys between two library calls; the scan, the per-tile folding and the
        merge of equal keys are library kernels."""
        raise NotImplementedError

    def region_statistics(self, labels, values, max_label, within=None):
        """Moments and extrema of one plane over the regions of a label image (F17, beside region_adjacency; csrc/region.hip): a
        segmented reduction that joins the planes of the image stage to the instance mask.  Returns ((count int32, sum int64, sumsq
        int64 or None, min int32, max int32, argmin int32, argmax int32), meta int32 [1]), every table [max_label + 1], all on the device;
        no host read.

        1.  labels: [H, W] of any integer dtype, H * W < 2^31; the kernel reads contiguous int32, so other dtypes and strides are
            copied, and an int64 value that does not fit int32 stays outside [0, max_label] (item 4).  max_label: an integer in 0 .. 2^31 - 2 (ValueError otherwise;
            the library returns CGC_EINVAL and launches nothing).  Tables are indexed by label value; row 0, the background, is a
            region like any other.
        2.  values: uint8, int8, int16 or int32 [H, W], any strides (TypeError for another dtype; bool is the caller's to pass as uint8).
        3.  within: None or [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool, any strides; only "is zero" is read.  A pixel p is
            *counted* in row L iff labels[p] == L and within is None or non-zero at p.
        4.  A pixel whose label lies outside [0, max_label] is counted nowhere.  meta[0] = the number of such pixels, whatever within
            says there; the caller reads it and refuses.
        5.  count = the number of counted pixels; sum = their sum (|sum| <= 2^31 * 2^31: it fits int64); sumsq = the sum of their
            squares for values of at most 16 bits (at most 2^31 * 2^30), None for int32 values.
        6.  min, max: the extrema of the counted values; argmin, argmax: the raster index y * W + x at which they are attained, of
            equal values the SMALLEST index -- inside a tile, across tiles and however lanes arrive: value and position travel as one
            64-bit key, (v ^ 2^31) << 32 | i under an unsigned minimum and (v ^ 2^31) << 32 | ~i under an unsigned maximum.
        7.  An empty row has count = sum = sumsq = min = max = 0 and argmin = argmax = -1.  H * W = 0 gives such rows only.
        8.  Exact for every input: a tile with more distinct labels than its table in LDS holds (``region_slots``), down to one
            label per pixel, sends what finds no slot to the global tables directly; nothing is dropped or counted twice, and no
            probe sequence is longer than the table.
        9.  Integer additions and integer minima / maxima only: bit-identical from call to call, whatever the order of arrival.
        Inside the kernel ("Region statistics"): one workgroup per tile of ``region_tile`` x ``region_tile`` (64) pixels; a
        thread sums the run of equal labels down its 16 pixels of a column in registers, folds it into a table of ``region_slots``
        (64) labels in LDS, and the tile's table goes to the global tables with one integer atomic per label and quantity."""
        raise NotImplementedError

    def region_histogram(self, labels, values, max_label, within=None):
        """The 256-bin histogram of a uint8 plane over every region of a label image (F17; csrc/region.hip).  Returns (hist int32
        [max_label + 1, 256], meta int32 [1]) on the device; no host read.

        1.  labels, max_label, within, "counted" and meta: items 1, 3 and 4 of region_statistics.
        2.  values: uint8 [H, W], any strides (TypeError for another dtype).
        3.  hist[L][v] = the number of counted pixels of row L with value v; the table is indexed in 64 bits ((max_label + 1) * 256
            may pass 2^31).  H * W = 0 gives zeros.
        4.  Exact for every input, as item 8 of region_statistics: pixels whose label finds no slot add to hist directly.
        5.  Partial counts are 16-bit bins in LDS, two per dword; a tile has 4096 pixels, so a tile of one label and one value does
            not overflow one.
        6.  Integer additions only: bit-identical from call to call."""
        raise NotImplementedError

    def region_cooccurrence(self, labels, values, max_label, lut, levels, offsets, symmetric, within=None):
        """The grey-level co-occurrence tables (GLCM) of a uint8 plane over every region of a label image, at several offsets (F18,
        beside region_histogram; csrc/region.hip).  Returns (tables int32 [max_label + 1, len(offsets), levels * levels], meta int32
        [1]) on the device; no host read.

        1.  labels, max_label, within, the refused pixels and meta: items 1, 3 and 4 of region_statistics.  meta[0] counts every pixel
            whose label lies outside [0, max_label] once per call, not once per offset.  H * W < 2^30, so that a symmetric diagonal
            bin of at most 2 H W fits int32 (the library returns CGC_EINVAL for a larger image and launches nothing).
        2.  values: uint8 [H, W], any strides (TypeError for another dtype).
        3.  levels: an integer in 2..16.  lut: 256 integers in 0 .. levels - 1 on the host; the level of a pixel is lut[v].  An entry
            >= levels is a ValueError (CGC_EINVAL, nothing launched).  The table travels by value in the kernel argument: nothing
            of the caller's is read after the call returns.
        4.  offsets: 1 to 8 pairs (dy, dx) of integers, |dy| and |dx| <= 16, (0, 0) not allowed (ValueError; CGC_EINVAL, nothing
            launched).
        5.  For offset k, anchor p = (y, x) and partner q = (y + dy, x + dx), the pair is counted in row R iff p and q lie inside the
            image, labels[p] == labels[q] == R, 0 <= R <= max_label, and within is None or non-zero at both p and q.  Row 0, the
            background, is a region like any other; a caller who does not want it passes within = labels != 0.
        6.  A counted pair with levels (a, b) adds 1 to tables[R][k][a * levels + b]; with symmetric it also adds 1 to
            tables[R][k][b * levels + a], so a pair with a == b adds 2 to the diagonal (skimage's symmetric=True).  The table is
            indexed in 64 bits.  H * W = 0 gives zeros.
        7.  Exact for every input, as item 8 of region_statistics: the pairs of a label that finds no slot in the tile's table in
            LDS add to tables directly.  The tile that holds the anchor counts the pair, wherever the partner lies; a partner is
            read through an address clamped into the image, and whether it lies inside is decided from its coordinates.
        8.  Partial counts are 16-bit bins in LDS, two per dword; a tile has 4096 anchors, so a tile of one label and one level,
            symmetric, puts 8192 into one bin and does not overflow it.
        9.  Integer additions only: bit-identical from call to call.
        Inside the kernel ("Region co-occurrence"): one launch per offset over region_histogram's tile, table and walk."""
        raise NotImplementedError

    def region_geometry(self, labels, max_label, within=None):
        """The shape of every region of a label image, from the labels alone (F19, beside region_statistics; csrc/region.hip): one
        segmented integer reduction.  Returns ((count int32 [R], sums int64 [5, R], extents int32 [R, 8, 2], quads int32 [R, 4], border
        int32 [R]), meta int32 [1]) with R = max_label + 1, all on the device; no host read.

        1.  labels, max_label, within, "a pixel *belongs* to row L" (= is counted there), the refused pixels and meta: items 1, 3 and
            4 of region_statistics.  Row 0, the background, is a region like any other.  Also H, W <= GEOMETRY_MAX_SIDE = 32767, so
            that sum x^2 over 2^31 pixels stays inside int64, and (H + 1)(W + 1) < 2^31, so that a quad count fits int32 (ValueError;
            the library returns CGC_EINVAL and launches nothing).
        2.  count = the number of the row's pixels.
        3.  sums = sy, sx, syy, sxy, sxx over the row's pixels, in image coordinates: y = row, x = column.
        4.  extents[L][k] = (minimum, maximum) of a x + b y over the row's pixel centres, (a, b) = GEOMETRY_DIRECTIONS[k] = (1,0)
            (2,1) (1,1) (1,2) (0,1) (-1,2) (-1,1) (-2,1).  Directions (1,0) and (0,1) are the bounding box.
        5.  quads = n1, n2, nd, n3.  A quad is a 2 x 2 window with top-left corner (y, x), y in -1 .. H-1 and x in -1 .. W-1; positions
            outside the image belong to no row.  For a row present in the quad, the pattern of which of the four positions belong
            to it is counted under exactly one of: n1 one pixel, n2 two that share an edge, nd the two of a diagonal, n3 three.  A
            quad adds to every row that occurs in it, so to at most four.  Quads that lie in the row entirely are not stored: n4 =
            (4 count - n1 - 2 n2 - 2 nd - 3 n3) / 4 exactly.
        6.  border = the number of the row's pixels with y in {0, H-1} or x in {0, W-1}.
        7.  An empty row has zeros everywhere, extents (0, 0): a caller masks by count == 0.  H * W = 0 gives empty rows only.
        8.  Exact for every input, as item 8 of region_statistics: what finds no slot in the tile's table in LDS -- a run of pixels,
            a quad's pattern -- goes to the global tables with the same integer atomics.
        9.  Integer additions, minima and maxima only: bit-identical from call to call.
        Inside the kernel ("Region geometry"): region_statistics' tile, column walk and table.  A run of one label down a
        thread's 16 pixels is summed in registers in tile coordinates (32 bits in LDS) and shifted to image coordinates at the flush;
        its extents are attained at its two ends.  The tile that holds a quad's top-left corner counts it, the tiles on the top and
        left edge also own row and column -1; the column to the right and the row below are read through clamped addresses and
        "inside the image" is decided from coordinates.  Only quads whose four positions differ are classified."""
        raise NotImplementedError

    def region_hull_ptr(self, count, extents):
        """Where the row spans of region_hull lie: int64 [R + 1], ptr[0] = 0 and ptr[L + 1] - ptr[L] = the height y1 - y0 + 1 of the
        bounding box of row L (extents[L][4] of region_geometry), 0 for a row with count 0.  A prefix sum on the device; no host
        read.  The caller reads ptr[R] together with region_geometry's meta: the ONE host read of a hull call."""
        raise NotImplementedError

    def region_hull(self, labels, max_label, extents, ptr, span_rows, within=None, tall_rows=0):
        """The exact convex hull of every region of a label image (F20, behind region_geometry; csrc/region.hip).  Returns ((count
        int32 [R], area2 int64 [R], diameter2 int64 [R], diameter_ends int32 [R, 2, 2], width_cross int64 [R], width_edge int32 [R, 2],
        perimeter float64 [R]), points int32 [2 (span_rows + R), 2]) with R = max_label + 1, all on the device; no host read.

        1.  labels, max_label, within, "a pixel is *counted* in row L" and the refused pixels: items 1, 3 and 4 of region_statistics,
            sides as item 1 of region_geometry.  extents: region_geometry's of the same labels and within; ptr: region_hull_ptr's of
            them; span_rows = ptr[R], read by the caller.  span_rows < 0 or > R * H is a ValueError (the library returns CGC_EINVAL
            and launches nothing); a ptr that does not fit the extents writes nothing outside the tables (such rows come out empty
            or wrong, never out of bounds).
        2.  THE HULL of row L is the convex hull of the pixel SQUARES of its counted pixels: the pixel at row y, column x is [x, x +
            1] x [y, y + 1], so vertices are lattice corners (y, x) -- the convention of region_shape's feret_max, feret_min and
            16-gon.  Hence hull area >= count, and a rectangle has solidity 1.  Tied to no library's version: skimage counts the
            pixels inside the hull, cv2 hulls a contour.
        3.  Vertices are strictly convex (none lies on the segment between its neighbours) and listed from the left end of the top
            lattice line y = y0 down the left side, along the bottom line and up the right side, without repeats: the list is
            unique.  count = their number, at least 4.  Row L's vertices are points[2 (ptr[L] + L) : 2 (ptr[L] + L) + count[L]]; the
            rest of ``points`` is workspace.
        4.  area2 = twice the area (shoelace, exact).  perimeter = the edge lengths sqrt(dy^2 + dx^2), each correctly rounded from
            the integer, summed in hull order from vertex 0 in float64.
        5.  diameter2 = the largest squared distance between two vertices; diameter_ends = those vertices (y, x).  TIE RULE: of
            several pairs the one with the smallest vertex indices (i, j), i < j, in hull order (smallest i, then smallest j).
        6.  The width of edge e = (v[e], v[e + 1]) with (dy, dx) = v[e + 1] - v[e] is c / |e|, c = the largest dy (x - x_e) - dx (y -
            y_e) over all vertices (y, x) -- non-negative in this order.  width_cross, width_edge = c and (dy, dx) of the edge of
            smallest width.  Two edges are compared as c_a^2 |e_b|^2 against c_b^2 |e_a|^2 EXACTLY: with sides up to 32767 the
            crosses reach 2^31 and the products 2^93, so they are formed in 128 bits.  TIE RULE: the first edge in hull order.
        7.  A row without a counted pixel has zeros everywhere and no vertices.  H * W = 0 gives such rows only.
        8.  tall_rows: a region of more rows is hulled by a whole wave (each lane a 64th of the lattice lines, one lane merges the
            64 chains), one of at most that many by one lane; 0 = the library's own threshold (``region_hull_tall_rows``); negative
            is a ValueError.  Both routes give identical tables and vertices.
        9.  Stage 1 uses integer minima and maxima only, stage 2 no atomics: bit-identical from call to call.
        Inside the kernels ("Region hull"): stage 1, region_geometry's tile; per row L and image row y of its bounding
        box spans[ptr[L] + y - y0] = (smallest, largest column of its counted pixels); a wave is one row of a tile and only the
        first and last pixel of a run of one label (seen through a lane shuffle; a tile's first and last column always) send an
        atomic.  Stage 2: lattice line j = y0 .. y1 + 1 has the left point (min(xmin[j-1], xmin[j]), j) and the right point
        (max(xmax[j-1], xmax[j]) + 1, j) over the non-empty rows beside it; Andrew's monotone chain with int64 cross products, in
        place in ``points``; then the scans of items 4 to 6."""
        raise NotImplementedError

    def region_outlines(self, labels, max_label, connectivity=1, within=None, mode='corners', background=False):
        """The ordered boundary of every region of a label image as closed polygons of lattice corners (F22, behind region_geometry;
        csrc/outline.hip).  Returns ((label_ptr int64 [R + 1], loop_ptr int64 [n_loops + 1], loop_label int32 [n_loops], loop_start
        int32 [n_loops], loop_cracks int32 [n_loops], loop_area2 int64 [n_loops], vertices int32 [n, 2]), meta int32 [1], refused) with
        R = max_label + 1, every tensor on the device; ``refused`` is meta[0] as the first host read brought it, and where it is not
        0 the tables are None: nothing more is launched and the caller refuses.

        1.  labels, max_label, within, "a pixel is *counted* in row L", the refused pixels and meta: items 1, 3 and 4 of
            region_statistics; sides as item 1 of region_geometry (at most 32767).  Also H * W < 2^29, so that a crack id and the
            number of cracks fit int32 (ValueError; the library returns CGC_EINVAL and launches nothing).  connectivity: 1 or 2; mode:
            'corners' or 'cracks' (ValueError).  background=False: rows 1 .. max_label get outlines; background=True: row 0 is a
            region like any other.
        2.  CRACKS.  The pixel (y, x) is the square [x, x + 1] x [y, y + 1].  A side of a counted pixel of row v is a crack of v
            when the pixel across it is not counted in row v; outside the image counts as "not".  Sides are numbered 0 top, 1
            right, 2 bottom, 3 left; a crack is directed so that its own pixel lies on its right: top east, right south, bottom
            west, left north.  Its id is 4 (y W + x) + side.  Vertices are lattice corners (y, x), 0 <= y <= H and 0 <= x <= W, row
            first.  A border between two rows is cracked from both sides.
        3.  SUCCESSOR, decided at the crack's head from the 2 x 2 block around that vertex alone.  A = the pixel ahead on the
            region's side, B = the pixel ahead on the other side.  TIE RULE, connectivity 1: a right turn (the next side of the same
            pixel) if A is not in v, else straight on (the same side of A) if B is not in v, else a left turn (the previous side of
            B).  TIE RULE, connectivity 2: left if B is in v, else straight if A is in v, else right.  The two differ only where two
            pixels of v touch by a corner: connectivity 1 keeps them apart, connectivity 2 passes through the vertex twice.
        4.  The successor map is a permutation of the cracks; its cycles are the LOOPS.  ORDER: a loop starts at its crack of
            smallest id; the loops of a label are ordered by start id; labels ascend.  The output is therefore unique.  Loops
            label_ptr[L] .. label_ptr[L + 1] - 1 belong to row L, vertices loop_ptr[j] .. loop_ptr[j + 1] - 1 to loop j.
        5.  mode='cracks': one vertex, the tail, per crack, in loop order from the start crack.  mode='corners': the same list
            without every vertex whose incoming and outgoing crack have the same direction -- an even number, at least 4.  The first
            vertex of a hole is then in general NOT the start crack's tail.
        6.  loop_label = the row; loop_start = the id of the start crack; loop_cracks = the number of cracks, whatever the mode;
            loop_area2 = the shoelace sum of x1 y2 - x2 y1 over the loop's cracks (tail 1, head 2): twice the enclosed area, positive
            for an outer boundary and negative for a hole.  Over the loops of a row it sums to twice the row's count.
        7.  An empty image, an image without foreground and labels that do not occur give empty rows: label_ptr[L] = label_ptr[L +
            1].  H * W = 0 makes no host read at all.
        8.  HOST READS: two.  The first brings the number of cracks and the refused pixels; it sizes the compact crack list and
            fixes the doubling rounds.  The second brings the number of loops and, for mode='corners', the number of vertices; it
            sizes the tables.  No cracks: the second is not made.
        9.  Integer work only: bit-identical from call to call.  The one place where an order of arrival exists, the int64 additions
            to loop_area2, does not depend on it.
        Inside the kernels ("Region outlines"): no loop is walked.  A thread per pixel counts its cracks (a prefix sum
        gives the compact list in id order) and writes each crack's successor as a compact index; pointer doubling over all cracks,
        in ceil(log2(n_cracks)) rounds per phase (``region_outline_rounds``), finds first the smallest index of every cycle -- the
        loop's start -- and then, with the cycle cut there, every crack's position and the loop's length; the loops' 64-bit keys
        (label, start) are sorted; one scatter puts every tail at loop_ptr[loop] + position, for 'corners' through a prefix sum over
        the kept vertices in that order.  The prefix sums and the sort are torch's; everything else is a library kernel."""
        raise NotImplementedError

    def slic_iterate(self, planes, step, compactness, n_iter, within=None):
        """SLIC superpixel clustering of one tile in integers (F23, behind stain_separate / od_recolor, in front of label_components
        and region_adjacency; csrc/slic.hip).  Returns (labels int32 [H, W], centres int32 [K, 2 + C], count int32 [K]) on the device;
        no host read.

        1.  planes: uint8 [C, H, W], 1 <= C <= 4, any strides (copied if not contiguous), H * W < 2^29 (TypeError for another dtype,
            ValueError otherwise; the library returns CGC_EINVAL and launches nothing).  step S: an integer in 4..256; compactness m:
            an integer in 0..1024; n_iter: an integer in 1..64 (ValueError).  within: None or [H, W] of a 1-, 2-, 4- or 8-byte
            integer type or bool; only "is zero" is read.
        2.  GRID.  ny = max(1, (2 H + S) // (2 S)), nx likewise from W, K = ny * nx.  Pixel (y, x) has HOME cell (y * ny // H, x * nx //
            W).  Centre k = i * nx + j starts at y = ((2 i + 1) H) // (2 ny), x = ((2 j + 1) W) // (2 nx), with the colour of the pixel
            there, whether or not within holds there.
        3.  ASSIGNMENT.  A pixel where within is non-zero looks at the centres of the up to 9 cells around its home cell (those
            inside the grid) -- at those centres' identities, wherever they have moved -- and takes the one with the smallest D = S^2 *
            sum_c (p_c - c_c)^2 + m^2 * ((y - c_y)^2 + (x - c_x)^2), computed in 64 bits; of equal D the smallest k.  A gather: no
            atomics and no launch order decide anything.
        4.  UPDATE.  Per centre: n, the number of its pixels, and the sums of y, x and every plane over them.  Every coordinate and
            colour becomes (2 * sum + n) // (2 * n): the mean, rounded half up.  A centre with n == 0 keeps its values.
        5.  A call is n_iter rounds of assignment, then update.  labels = k + 1 of the LAST assignment, 0 where within is zero;
            centres = (y, x, colours) after the last update; count = n of the last assignment.
        6.  H * W = 0 gives labels [H, W], centres [0, 2 + C] and count [0] without a launch.
        7.  Integer additions only: bit-identical from call to call.  The regions of one label need not be connected; slic_merge and
            nuclei.superpixels see to that.
        Inside the kernels ("Superpixels"): 1 + 2 n_iter launches.  A round is one launch over tiles of ``slic_tile`` x
        ``slic_tile`` (64) pixels that assigns and accumulates -- a thread sums the run of equal centres down its 16 pixels of a
        column in registers and folds it into a table in LDS of the ``slic_table`` x ``slic_table`` (12) cells around the tile's
        first pixel, which goes to global memory with one integer atomic per centre and quantity -- and one launch of a thread per
        centre that divides and clears.  A tile meets at most 64 // (H // ny) + 4 cells per axis, neighbours included, so the
        table holds them all from cells of 8 pixels up; sums of cells outside it (small steps) go to global memory directly, exactly."""
        raise NotImplementedError

    def slic_merge(self, sizes, pairs, count, min_size):
        """The order-free merge of small pieces into settled neighbours (F23; csrc/slic.hip): what makes superpixels connected.
        Returns (group int32 [P + 1], launched rounds); one host read per batch of rounds.

        1.  sizes: int32 [P], the pixels of pieces 1 .. P (label_components with sizes); pairs int32 [Q, 2] and count int32 [Q]:
            region_adjacency's outputs on the piece image, connectivity 1.  min_size: an integer >= 0.
        2.  A piece is SMALL iff sizes < min_size; the others are SETTLED from the start, each its own group: group[p] = p.
        3.  ROUND r: every unsettled piece that has a neighbour settled BEFORE round r joins the group of the settled neighbour q
            with the largest count; of equal counts the smallest q (one 64-bit key, count << 32 | ~q, under an unsigned maximum).
            Pieces that join are settled from round r + 1 on.  Rounds repeat until one settles nothing.
        4.  group[p] = the piece whose group p ended in, 0 for a piece that never met a settled one (its whole component of the
            mask is made of small pieces); group[0] = 0.
        5.  The result does not depend on the order of the pairs, of arrival, or on how many rounds run past the last useful one;
            they run in batches of SLIC_MERGE_FIRST_BATCH, twice that, ... with one host read after each (_relax_until_still)."""
        raise NotImplementedError

    def slic_relabel(self, pieces, table):
        """out int32 [H, W] = table[pieces] for pieces in 1 .. len(table) - 1, 0 elsewhere (F23; one launch, no host read)."""
        raise NotImplementedError

    def region_quantiles(self, hist, q10k):
        """Quantiles of the rows of a table of 256-bin histograms (F17; csrc/region.hip).  Returns uint8 [R, len(q10k)] on the device;
        no host read.

        1.  hist: int32 [R, 256], contiguous, counts >= 0, every row's total n < 2^31 (region_histogram's are).
        2.  q10k: 1 to REGION_MAX_QUANTILES = 8 integers in 0..10000 (ValueError otherwise; the library returns CGC_EINVAL and
            launches nothing).
        3.  With v[0] <= ... <= v[n-1] the row's values sorted, the result is v[k], k = min(n - 1, floor(n * q10k / 10000)) --
            rank_filter's rule (item 5 there), the product taken in 64 bits: a bin of 2^31 - 1 at q10k = 9999 is not an overflow.
            q10k = 0 is the row's minimum, 10000 its maximum, 5000 the median (the upper one when n is even).
        4.  n = 0 gives 0.  R = 0 gives an empty output.
        5.  One wave per row, four bins per lane, rank_filter's scan in registers; no atomics: bit-identical from call to call."""
        raise NotImplementedError

    def edge_renorm(self, rowptr, col, n, p, val_out):
        """Level-1 ``_re_norm_adj`` (model/network.py:183-191) on a 0/1 CSR that holds its diagonal:
        val[k] = p if col[k]==row else (1/(c+1e-15))*(1-p), c = number of off-diagonal entries of the row."""
        raise NotImplementedError

    def csr_transpose_vals(self, t_rowptr, t_perm, val, n, t_val_out):
        """t_val[k] = val[t_perm[k]] for the live slots of the transposed CSR (entries beyond nnz stay undefined)."""
        raise NotImplementedError

    def csr_invdeg(self, rowptr, val, n, out):
        """out[i] = 1 / max(sum_k val[k] (or the entry count when val is None), 1)  -- DenseSAGEConv's clamp."""
        raise NotImplementedError

    def spmm(self, rowptr, col, perm, val, pre, post, x, out, n, width, gptr=None, num_graphs=0, nmax=0, visit=0, ld=None, gorder=None):
        """out[i,:] = post[i] * sum_{k in row i} w_k * pre[col[k]] * x[col[k],:]
        with w_k = val[perm[k]] / val[k] / 1 and pre/post optional.  x, out: [n, width] contiguous.
        gptr/num_graphs/nmax (optional): the rows are a batch of graphs with block-diagonal adjacency
        (first row of each graph, count, largest graph) -- a layout hint, the result is the same.
        visit (optional, scheduling hint, bits 0-1): 1 = x was just written in ascending row order, 2 = by a ragged batched gemm;
        bit 2 (+4) notes that the nodes of every graph are listed grid cell by grid cell.  Higher bits are ignored.
        ld (optional): row stride of x and out when the rows are padded (wide rows only; needs gptr).
        gorder (optional, scheduling only): int32 [num_graphs] visiting sequence of the graphs (wide rows)."""
        raise NotImplementedError

    # ------------------------------------------------------------------ dense contractions (MFMA fp32)
    def gemm(self, A, B, C, M, N, K, transA, transB, lda, ldb, ldc, alpha=1.0, beta=0.0, bias=None,
             batch=1, strideA=0, strideB=0, strideC=0, gptr=None, ragged=0, max_ragged=0, ragged_total=0, extra=()):
        """C_b = alpha * op(A_b) op(B_b) + beta * C_b (+ bias[N]),  b = 0..batch-1, row-major.

        op(A) is M x K (stored [M,K] or, transA, [K,M]); op(B) is K x N (stored [K,N] or, transB, [N,K]).
        Operand b starts at base + b*stride (+ ragged offset).  ragged=1: M_b = gptr[b+1]-gptr[b], A
        (not transposed) and C advance by gptr[b] rows.  ragged=2: K_b = gptr[b+1]-gptr[b], A (transposed)
        and B (not transposed) advance by gptr[b] rows.  max_ragged bounds the ragged extent (grid size);
        ragged_total = sum of the ragged extents (host-side flop accounting only).
        extra: up to two (A_x, B_x, lda, ldb, K_x, strideA, strideB) pairs whose products are added to op(A)op(B)
        (same orientation, M, N, batch and ragged row offsets): the concatenated-K product without the concatenation.
        """
        raise NotImplementedError

    def reduce_batch_sum(self, ws, out, parts, numel, beta=0.0):
        """out[j] = beta*out[j] + sum_s ws[s*numel + j]  (deterministic split-K combine)."""
        raise NotImplementedError

    def reduce_batched(self, ws, out, outer, parts, numel, beta=0.0):
        """out[o, j] = beta*out[o, j] + sum_s ws[o, s, j]  for ws [outer, parts, numel]."""
        raise NotImplementedError

    # ------------------------------------------------------------------ conv epilogue: L2 norm, activation, BatchNorm (A4, A5)
    def l2norm_act_stats(self, h, n, F, normalize, act, hn_out, rinv_out, stats_out):
        """hn = h / max(||h||_2, 1e-12) row-wise (or hn = h), rinv = that reciprocal;
        stats[0,f] = sum_i act(hn)[i,f], stats[1,f] = sum_i act(hn)[i,f]^2 (None to skip).  ``stats`` is
        FLOAT64 [2,F]: the variance is a difference of these two sums."""
        raise NotImplementedError

    def l2norm_act_bn(self, h, n, F, normalize, act, hn_out, rinv_out, count, eps, momentum, running_mean, running_var,
                      num_batches_tracked, mean_out, istd_out):
        """l2norm_act_stats + bn_finalize as one call (the training forward): also increments num_batches_tracked
        (int64 scalar tensor or None), as nn.BatchNorm1d.forward does."""
        raise NotImplementedError

    def sage_wide_fwd(self, agg, lda, weight, bias, n, Kin, F, normalize, act, hn_out, rinv_out, stats, count, eps, momentum,
                      running_mean, running_var, num_batches_tracked, mean_out, istd_out):
        """hn = l2norm(agg[:, :Kin] @ weight + bias) and (stats) the statistics part of l2norm_act_bn, as one kernel: narrow
        inputs (Kin <= 32) into narrow (F <= 32) or wide (F <= 1664) outputs.  Returns False (nothing done) outside that envelope."""
        raise NotImplementedError

    def bn_finalize(self, stats, count, eps, momentum, running_mean, running_var, mean_out, istd_out):
        """mean = s0/count, var = s1/count - mean^2 (biased), istd = rsqrt(var+eps); running stats get
        momentum updates with the unbiased var*count/(count-1).  ``count`` = B*Nmax INCLUDING the
        zero padding rows of the dense layout (model/network.py:101-107)."""
        raise NotImplementedError

    def bn_act_apply(self, hn, n, F, act, mean, istd, gamma, beta, y_out, ldy):
        """y = (act(hn) - mean) * istd * gamma + beta   (mean None -> y = act(hn))."""
        raise NotImplementedError

    def bn_bwd_reduce(self, dy, ldy, hn, n, F, act, mean, istd, sums_out):
        """sums[0,f] = sum_i dy, sums[1,f] = sum_i dy * xhat, xhat = (act(hn)-mean)*istd."""
        raise NotImplementedError

    def bn_act_l2_bwd(self, dy, ldy, hn, rinv, n, F, act, normalize, mode, mean, istd, gamma, sums, count, dh_out,
                      dh_colsum_out=None):
        """Backward of BN o act o l2norm for one row block (dh_colsum_out[f] = sum_i dh[i,f], optional).
        mode 2 (batch stats): do = gamma*istd*(dy - s0/count - xhat*s1/count); mode 1 (running stats):
        do = gamma*istd*dy; mode 0 (no BN): do = dy.   dhn = do*act'(hn);
        normalize: dh = rinv*(dhn - hn*<hn,dhn>) (dh = dhn*1e12 where the norm clamp was active)."""
        raise NotImplementedError

    def colsum(self, x, ld, n, F, out):
        """out[f] = sum_i x[i,f]."""
        raise NotImplementedError

    def sage_narrow_bwd(self, dy, ldy, hn, rinv, n, F, act, normalize, mode, mean, istd, gamma, sums, count, agg, lda, fin, weight,
                        dagg_out, dwdb_out):
        """bn_act_l2_bwd without writing dh, plus its three consumers: dagg_out [n,fin] = dh @ weight^T (None: skipped) and
        dwdb_out [fin*F + F] = (agg^T dh).ravel() followed by colsum(dh).  Returns False (nothing done) unless fin, F <= 32."""
        raise NotImplementedError

    # ------------------------------------------------------------------ assignment softmax (A8), readout (A9)
    def softmax_fwd(self, x, n, C, out, ld=None):
        raise NotImplementedError

    def softmax_bwd(self, S, dS, n, C, dx_out, dx_colsum_out=None, ld=None):
        """dx = S * (dS - <dS, S>_row);  dx_colsum_out[c] = sum_i dx[i,c] (optional)."""
        raise NotImplementedError

    def segment_max_fwd(self, x, gptr, B, D, nmax, out, arg_out):
        """Per graph b and column d: max over its rows (first index on ties); a graph with fewer than
        nmax rows also competes against the zero padding rows of the dense layout (model/network.py:264):
        if its max is < 0 the result is 0 and arg = -1."""
        raise NotImplementedError

    def segment_max_bwd(self, dout, arg, B, D, dx_zeroed):
        """dx[arg[b,d], d] = dout[b,d] where arg >= 0 (dx arrives zero-filled)."""
        raise NotImplementedError

    def segment_max_bwd_full(self, dout, arg, gptr, B, D, nmax, dx_out):
        """segment_max_bwd that writes every element of dx (no pre-zeroed buffer needed)."""
        raise NotImplementedError

    # ------------------------------------------------------------------ jumping-knowledge attention (A7)
    def jk_supported(self, C):
        """Whether the fused DenseJK kernels exist for this channel count."""
        raise NotImplementedError

    def jk_fwd(self, xs, n, npad, C, lstm, w_att, b_att, out, HS, CS):
        """DenseJK forward (model/network.py:36-52): xs [n,3C] -> out [n,C].  ``lstm`` = 8 tensors
        (w_ih, w_hh, b_ih, b_hh) x (forward, reverse) in torch.nn.LSTM layout, hidden H = 3C/2.
        HS, CS [6H, npad]: hidden / cell state of (direction d, step t, unit j) at row (d*3+t)*H + j.
        npad, here and in the three backward calls: npad >= n and npad % 64 == 0 (include/cgc_hip.h), else the call is refused
        before anything is launched; ``jk_bwd_params`` may need npad % 256 == 0 (see there).  Columns >= n of HS / CS are never
        read: the buffers need not be cleared."""
        raise NotImplementedError

    def jk_bwd(self, xs, dout, n, npad, C, lstm, w_att, b_att, HS, CS, dxs, DGT, INT, DHC):
        """DenseJK backward: dxs [n,3C]; DGT [2, 4H+1, 3*npad] and INT [2, C+2H+1, 3*npad] such that
        G_d = DGT[d] @ INT[d]^T gives dW_ih = G_d[:4H,:C], dW_hh = G_d[:4H,C:C+H], db_ih = db_hh = G_d[:4H,C+H],
        d w_att[dH:(d+1)H] = G_d[4H, C+H+1:], d b_att = G_0[4H, C+H].  DHC [2,2,H,npad] is scratch.
        One kernel for every supported C and any alignment of xs / dout / dxs (the thread-per-direction k_jk_bwd<C>); every
        column of DGT and INT is written, the padded columns n .. npad-1 of each time slot with zeros."""
        raise NotImplementedError

    def jk_bwd_params(self, xs, dout, n, npad, C, lstm, w_att, b_att, HS, CS, dxs, G_out):
        """DenseJK backward with the parameter gradients delivered directly: dxs [n,3C] and G_out [2, 4H+1, C+2H+1] with
        the meaning of ``DGT[d] @ INT[d]^T`` in ``jk_bwd`` (entries of the last row that are not parameter gradients are
        unspecified).  Where the gradients are staged through DGT / INT (channel counts off the matrix cores, buffers that are
        not 16-byte aligned) the product runs over K slices of 768 columns: npad % 256 == 0 there, else ValueError before
        anything is launched.  ops._DenseJK pads to multiples of 1024."""
        raise NotImplementedError

    def jk_unpack_param_grads(self, G, C):
        """G [2, 4H+1, C+2H+1] -> list of CONTIGUOUS gradients in parameter order: (w_ih, w_hh, b_ih, b_hh) forward, the same
        four reverse, att.weight [1, 2H], att.bias [1] -- all slices of one flat buffer."""
        raise NotImplementedError

    # ------------------------------------------------------------------ dense adjacency ops at levels 2-3 (A4, A6)
    def dense_rownorm_fwd(self, A, R, C, out, invd_out, ge1_out):
        """s = rowsum(A); d = max(s,1); out = A/d; invd = 1/d; ge1 = (s >= 1)  (clamp(min=1) of DenseSAGEConv)."""
        raise NotImplementedError

    def dense_rownorm_bwd(self, dOut, Anorm, invd, ge1, R, C, dA_out):
        """dA = invd * (dOut - ge1 * <dOut, Anorm>_row)."""
        raise NotImplementedError

    def dense_renorm_fwd(self, A, R, C, p, out):
        """``_re_norm_adj`` on [B,C,C] viewed as [R=B*C, C]; the diagonal of row i is column i mod C."""
        raise NotImplementedError

    def dense_renorm_bwd(self, A, dOut, R, C, p, dA_out):
        raise NotImplementedError

    def adj_prep_fwd(self, A, R, C, p, At_out, An_out, invd_out, ge1_out):
        """dense_renorm_fwd (skipped when p is None: At_out None) followed by dense_rownorm_fwd of its result, one pass."""
        raise NotImplementedError

    def adj_prep_bwd(self, A, An, invd, ge1, gAn, gAt, R, C, p, dA_out):
        """dAt = dense_rownorm_bwd(gAn) + gAt (gAt may be None); dA = dense_renorm_bwd(A, dAt) (dA = dAt when p is None)."""
        raise NotImplementedError

    # ------------------------------------------------------------------ DiffPool regularisers (csrc/diffpool_reg.hip)
    def diffpool_reg_fwd(self, S, n, C, lds, G, A_out, B, A, A_numel, rowptr, numel, rows, link_out, ent_out, keep_out):
        """link = sqrt(||A||^2 - 2 sum_b tr(A_out_b) + ||G||^2) / numel, ent = sum -S log(S + 1e-15) / rows (0-dim outputs);
        keep[0] = the square root.  A: dense [A_numel] (rowptr None) or the CSR values of rowptr (None: all ones)."""
        raise NotImplementedError

    def diffpool_reg_bwd_prep(self, d_reg, keep, numel, rows, d_ao, dao_out, G, Gs_out, B, C, coef_out):
        """coef = [c_l, c_e] from the upstream gradients d_reg [2]; dao = d_ao (None: 0) - 2 c_l I per graph; Gs = 4 c_l G."""
        raise NotImplementedError

    def diffpool_reg_entropy_bwd(self, S, n, C, lds, coef, ds, ldd):
        """ds[:, :C] += c_e (-log(S + 1e-15) - S / (S + 1e-15))."""
        raise NotImplementedError

    def diffpool_reg_adj_bwd(self, A, m, coef, gA, accumulate):
        """gA (+)= 2 c_l A over m elements."""
        raise NotImplementedError


# ----------------------------------------------------------------------------------------------
_LIB_NAME = 'libcgc_hip.so'
_instance = None


def lib_path():
    # CGC_LIB: another build of the same library (A/B timing of kernel changes on one box); default: the in-tree build
    return os.environ.get('CGC_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', _LIB_NAME)


def get():
    """The process-wide kernel table.  Raises (never falls back) when the HIP library is unusable."""
    global _instance
    if _instance is None:
        _instance = HipKernels()
    return _instance


_EINVAL = -1                            # include/cgc_hip.h: CGC_EINVAL (nothing was launched)
GEMM_EXACT, GEMM_SPLIT_BF16, GEMM_SPLIT_F16 = 0, 1, 2      # include/cgc_hip.h: CGC_GEMM_EXACT / CGC_GEMM_SPLIT_BF16 / CGC_GEMM_SPLIT_F16


def is_native():
    return isinstance(_instance, HipKernels)


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)
if _raw_stream is None or _cur_device is None:          # older / newer torch without the private accessors
    def _raw_stream(_idx):
        return torch.cuda.current_stream().cuda_stream

    def _cur_device():
        return torch.cuda.current_device()


def split_jk_param_grads(flat, C):
    """Views of the flat DenseJK parameter-gradient buffer (layout: cgc_jk_unpack_param_grads, include/cgc_hip.h)."""
    H = 3 * C // 2
    out, o = [], 0
    for _ in range(2):
        for shape in ((4 * H, C), (4 * H, H), (4 * H,), (4 * H,)):
            k = 1
            for d in shape:
                k *= d
            out.append(flat[o:o + k].view(shape))
            o += k
    out.append(flat[o:o + 2 * H].view(1, 2 * H))
    out.append(flat[o + 2 * H:o + 2 * H + 1])
    return out


def _ptr(t):
    # a plain int (None = NULL): every prototype is declared (_abi.py), so ctypes converts it -- building a c_void_p object per
    # argument was ~0.1 ms of a 4 ms step (~950 pointer arguments per step)
    return t.data_ptr() if t is not None else None


def _within_args(within):
    """The (pointer, element size) pair a flat-window entry point takes for ``within``: (NULL, 0) without one."""
    return _ptr(within), within.element_size() if within is not None else 0


class LaunchTimer(object):
    """HIP-event timing of every launch of the dominant 128 x 128 GEMM and of the wide SpMM between ``start()`` and ``stop()``
    (the library's measurement hook, csrc/timing.hip: events on the stream of the launch, whoever issues it -- the per-operator
    path or the step sequencer).  ``records()`` after a synchronize: list of (tag, dims, ms)."""
    TAGS = {1: 'gemm_128x128', 2: 'spmm_wide'}

    def __init__(self, capacity=8192):
        self.lib = get().lib
        self.h = self.lib.cgc_timing_create(int(capacity))
        if not self.h:
            raise RuntimeError('cgc_timing_create failed')

    def start(self):
        self.lib.cgc_timing_attach(self.h)
        return self

    def stop(self):
        self.lib.cgc_timing_attach(None)

    def records(self):
        out = []
        dims, ms = (ctypes.c_int * 8)(), ctypes.c_float()
        for i in range(self.lib.cgc_timing_count(self.h)):
            rc = self.lib.cgc_timing_read(self.h, i, dims, ctypes.byref(ms))
            if rc != 0:
                raise RuntimeError('cgc_timing_read failed with code %d' % rc)
            out.append((self.TAGS.get(dims[0], str(dims[0])), tuple(dims[1:8]), float(ms.value)))
        return out

    def counts(self):
        c = {}
        for i in range(self.lib.cgc_timing_count(self.h)):
            dims, ms = (ctypes.c_int * 8)(), ctypes.c_float()
            self.lib.cgc_timing_read(self.h, i, dims, ctypes.byref(ms))
            c[self.TAGS.get(dims[0], str(dims[0]))] = c.get(self.TAGS.get(dims[0], str(dims[0])), 0) + 1
        return c

    def close(self):
        if self.h:
            self.lib.cgc_timing_destroy(self.h)
            self.h = None

    @staticmethod
    def gemm_flops(dims, ragged_total):
        """Algorithmic flops 2 M N K of a recorded GEMM launch; ``ragged_total`` = the rows the ragged extents add up to (the
        batch's node count: the library does not know it)."""
        M, N, K, batch, ragged, _, xk = dims
        if ragged == 1:
            return 2.0 * ragged_total * N * (K + xk)
        if ragged == 2:
            return 2.0 * M * N * ragged_total
        if ragged == 3:
            parts = -(-K // dims[5])
            return 2.0 * M * N * K * (batch // parts)
        return 2.0 * M * N * (K + xk) * batch


class _NoWorkspace(object):
    @staticmethod
    def data_ptr():
        return None

    @staticmethod
    def numel():
        return 0


_NO_WS = _NoWorkspace()


class HipKernels(KernelSpec):
    tail_split = True   # hand cgc_gemm_f32 its slab workspace (False: every output tile is computed whole; tests / A-B timing)
    # cgc_gemm_f32's `mode` for the products issued through this table (the per-operator path): GEMM_EXACT (default),
    # GEMM_SPLIT_BF16 -- the big products as six bf16 MFMA pairs per fp32 product (csrc/gemm_split.hip) -- or GEMM_SPLIT_F16 -- as
    # three fp16 pairs of operands scaled per output tile's operand panels (csrc/gemm_half.hip).  The encoder sets it from its own ``gemm_mode`` at
    # the top of forward(); the sequencer gets the same choice through cgc_level_desc.flags bits 1 / 2.
    gemm_mode = 0
    # graph structure graph by graph in two launches when the Batch says how its edge list is grouped (cgc_graph_build_local;
    # CGC_GRAPH_LOCAL=0 / False: always the general build -- A-B timing, tests)
    graph_local = os.environ.get('CGC_GRAPH_LOCAL', '1') != '0'
    graph_local_count = 0      # batches built that way by this process (tests: did the route apply?)

    def __init__(self):
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError('%s not built: run `python -c "import __graft_entry__ as g; g.build()"` '
                               '(there is no CPU fallback)' % path)
        if not torch.cuda.is_available():
            raise RuntimeError('cgc_net_amd needs an AMD GPU (gfx950); torch.cuda.is_available() is False '
                               'and there is no CPU fallback')
        self.lib = ctypes.CDLL(path)
        from . import _abi
        _abi.declare(self.lib)
        self._ws_cache = {}
        self._graph_local_max = int(self.lib.cgc_graph_local_max_nodes())
        self.histogram_chunk = int(self.lib.cgc_histogram_chunk_pixels())      # pixels one workgroup of histogram_u8 counts (tests)
        self.window_tile_rows = int(self.lib.cgc_window_tile_rows())          # rows of the tiles of window_sums / local_threshold (tests)
        self.morph_tile_rows = int(self.lib.cgc_morph_tile_rows())            # rows of the tiles of flat_morphology (tests)
        assert int(self.lib.cgc_morph_max_radius()) == MORPH_MAX_RADIUS
        self.rank_tile_rows = int(self.lib.cgc_rank_tile_rows())              # rows of the tiles of rank_filter (tests)
        assert int(self.lib.cgc_rank_max_radius()) == RANK_MAX_RADIUS and int(self.lib.cgc_rank_entropy_max_radius()) == ENTROPY_MAX_RADIUS
        self.adjacency_tile = int(self.lib.cgc_adjacency_tile_side())          # side of the tiles region_adjacency folds in LDS (tests)
        self.region_tile = int(self.lib.cgc_region_tile_side())                # side of the tiles of region_statistics / region_histogram (tests)
        self.region_slots = int(self.lib.cgc_region_table_slots())             # labels such a tile folds in LDS (tests)
        self.region_cooc_max_offset = int(self.lib.cgc_region_cooc_max_offset())      # largest |dy|, |dx| of region_cooccurrence
        self.region_cooc_max_offsets = int(self.lib.cgc_region_cooc_max_offsets())    # offsets per call
        self.region_geometry_max_side = int(self.lib.cgc_region_geometry_max_side())  # largest H, W of region_geometry
        self.region_hull_tall_rows = int(self.lib.cgc_region_hull_tall_rows())        # rows above which a wave hulls a region
        self.slic_tile = int(self.lib.cgc_slic_tile_side())                    # side of the tiles of slic_iterate (tests)
        self.slic_table = int(self.lib.cgc_slic_table_side())                  # cells per axis such a tile folds in LDS (tests)
        assert int(self.lib.cgc_slic_max_step()) == SLIC_MAX_STEP
        self.scan_chunk = int(self.lib.cgc_scan_chunk_pixels())               # ... and of od_moments / angle_histogram
        self._dirs_checked = (None, None)                                      # angle_histogram's last direction table and its C array
        self._exp_checked = (None, None)                                       # od_recolor's last exponential table and its C array
        assert int(self.lib.cgc_angle_bins()) == ANGLE_BINS
        assert int(self.lib.cgc_resample_max_side()) == RESAMPLE_MAX_SIDE
        assert int(self.lib.cgc_resample_labels_max_factor()) == RESAMPLE_LABELS_MAX_FACTOR

    # -- helpers
    @staticmethod
    def _stream():
        # torch's current stream of the current device as a raw hipStream_t (the C call: torch.cuda.current_stream() costs
        # ~8 us of Python per launch, which is what bounds the small-graph regime)
        return _raw_stream(_cur_device())

    @staticmethod
    def _chk(rc, name):
        if rc != 0:
            raise RuntimeError('%s failed with code %d' % (name, rc))

    @staticmethod
    def _dev(*ts):
        # kernels are enqueued on the CURRENT device's current stream (_stream()): tensors living on another GPU would be
        # touched from the wrong device's stream, unordered against torch's work on them -- refuse instead of racing
        cur = _cur_device()
        for t in ts:
            if t is not None:
                if not t.is_cuda:
                    raise RuntimeError('cgc_net_amd kernels take GPU tensors only (got a %s tensor)' % t.device)
                if t.get_device() != cur:
                    raise RuntimeError('tensor on cuda:%d but the current device is cuda:%d: wrap the call in '
                                       'torch.cuda.device(...) / call torch.cuda.set_device first' % (t.get_device(), cur))

    # -- graph structure
    def csr_build(self, edge_index, n, add_diag):
        self._dev(edge_index)
        edge_index = edge_index.to(torch.int64).contiguous()
        E = edge_index.shape[1]
        cap = E + (n if add_diag else 0)
        dev = edge_index.device
        i32 = dict(dtype=torch.int32, device=dev)
        out = {k: torch.empty(n + 1, **i32) for k in ('rowptr', 't_rowptr')}
        out.update({k: torch.empty(max(cap, 1), **i32) for k in ('col', 'rowidx', 't_col', 't_perm')})
        ws = torch.empty(3 * (n + 1) + 2 * max(cap, 1), **i32)
        rc = self.lib.cgc_csr_build(_ptr(edge_index), ctypes.c_int64(E), n, int(add_diag),
                                    _ptr(out['rowptr']), _ptr(out['col']), _ptr(out['rowidx']),
                                    _ptr(out['t_rowptr']), _ptr(out['t_col']), _ptr(out['t_perm']),
                                    _ptr(ws), self._stream())
        self._chk(rc, 'cgc_csr_build')
        out['cap'] = cap
        o = int(self.lib.cgc_csr_bad_edges_offset(ctypes.c_int64(E), n, int(add_diag)))
        out['bad_edges'] = ws[o:o + 1]              # device-side count of dropped out-of-range edges (no sync here)
        return out

    def graph_build(self, edge_index, n, renorm_p, gptr=None, eptr=None, num_graphs=0, nmax=0, emax=0):
        """csr_build (+ edge_renorm + csr_transpose_vals when renorm_p is not None) + csr_invdeg behind ONE library call, all
        outputs carved out of two allocations.  Returns the dict of csr_build plus val / t_val (None without renorm) and inv_d.
        With ``gptr`` / ``eptr`` (int32 [B+1] on the device: node and edge ranges of the graphs, the edge list grouped by graph as
        Batch.from_data_list emits it; ``nmax`` / ``emax``: the largest graph's nodes, the most edges of one graph) the structure is built
        graph by graph in two launches (cgc_graph_build_local: same arrays bit for bit); batches outside its envelope take the general
        build."""
        self._dev(edge_index)
        edge_index = edge_index.to(torch.int64).contiguous()
        E = edge_index.shape[1]
        renorm = renorm_p is not None
        cap = max(E + (n if renorm else 0), 1)
        dev = edge_index.device
        a = lambda k: -(-k // 64) * 64                    # 256-byte aligned pieces
        sizes = [n + 1, n + 1, cap, cap, cap, cap, 3 * (n + 1) + 2 * cap]
        ibuf = torch.empty(sum(a(k) for k in sizes), dtype=torch.int32, device=dev)
        parts, o = [], 0
        for k in sizes:
            parts.append(ibuf[o:o + k])
            o += a(k)
        rowptr, t_rowptr, col, rowidx, t_col, t_perm, ws = parts
        fbuf = torch.empty((2 * a(cap) if renorm else 0) + max(n, 1), dtype=torch.float32, device=dev)
        val = fbuf[:cap] if renorm else None
        t_val = fbuf[a(cap):a(cap) + cap] if renorm else None
        inv_d = fbuf[2 * a(cap):] if renorm else fbuf
        rc = _EINVAL
        if gptr is not None and eptr is not None and self.graph_local and 0 < nmax <= self._graph_local_max:
            self._dev(gptr, eptr)
            rc = self.lib.cgc_graph_build_local(_ptr(edge_index), ctypes.c_int64(E), n, _ptr(gptr), _ptr(eptr), int(num_graphs), int(nmax), int(emax),
                                                ctypes.c_float(-1.0 if renorm_p is None else renorm_p), _ptr(rowptr), _ptr(col), _ptr(rowidx),
                                                _ptr(t_rowptr), _ptr(t_col), _ptr(t_perm), _ptr(val), _ptr(t_val), _ptr(inv_d), _ptr(ws),
                                                self._stream())
            if rc != _EINVAL:
                self._chk(rc, 'cgc_graph_build_local')
                self.graph_local_count += 1
        if rc == _EINVAL:                                  # no graph ranges, or outside the graph-local build's envelope
            self._chk(self.lib.cgc_graph_build(_ptr(edge_index), ctypes.c_int64(E), n, ctypes.c_float(-1.0 if renorm_p is None else renorm_p),
                                               _ptr(rowptr), _ptr(col), _ptr(rowidx), _ptr(t_rowptr), _ptr(t_col), _ptr(t_perm), _ptr(val),
                                               _ptr(t_val), _ptr(inv_d), _ptr(ws), self._stream()), 'cgc_graph_build')
        bo = int(self.lib.cgc_csr_bad_edges_offset(ctypes.c_int64(E), n, int(renorm)))
        return dict(rowptr=rowptr, t_rowptr=t_rowptr, col=col, rowidx=rowidx, t_col=t_col, t_perm=t_perm, cap=E + (n if renorm else 0),
                    bad_edges=ws[bo:bo + 1], val=val, t_val=t_val, inv_d=inv_d)

    def collate(self, x, mean, std, gptr, num_graphs, batch_out, edge_index, eptr):
        self._dev(x, mean, std, gptr, batch_out, edge_index, eptr)
        assert x.is_contiguous() and x.dtype == torch.float32
        E = edge_index.shape[1] if edge_index is not None else 0
        assert edge_index is None or (edge_index.is_contiguous() and edge_index.dtype == torch.int64)
        self._chk(self.lib.cgc_collate(_ptr(x), x.shape[0], x.shape[1], _ptr(mean), _ptr(std), _ptr(gptr), num_graphs,
                                       _ptr(batch_out), _ptr(edge_index), ctypes.c_int64(E), _ptr(eptr), self._stream()),
                  'cgc_collate')

    def farthest_point_sample(self, pos, gptr, num_graphs, max_nodes, start, optr, out, table16=False):
        self._dev(pos, gptr, start, optr, out)
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[1] == 2
        fn = self.lib.cgc_farthest_point_sample_table16 if table16 else self.lib.cgc_farthest_point_sample
        self._chk(fn(_ptr(pos), _ptr(gptr), num_graphs, max_nodes, _ptr(start), _ptr(optr), _ptr(out), self._stream()),
                  'cgc_farthest_point_sample')

    def radius_knn(self, pos, gptr, num_graphs, r, k, loop):
        self._dev(pos, gptr)
        pos = pos.to(torch.float32).contiguous()
        n, dev = pos.shape[0], pos.device
        i32 = dict(dtype=torch.int32, device=dev)
        if n == 0:
            return torch.zeros(2, 0, dtype=torch.int64, device=dev)
        assert pos.dim() == 2 and pos.shape[1] == 2 and gptr.dtype == torch.int32
        nbr, cnt, rowptr = torch.empty(n, k + 1, **i32), torch.empty(n, **i32), torch.empty(n + 1, **i32)
        ws = torch.empty(int(self.lib.cgc_radius_knn_ws_ints(n, num_graphs)), **i32)
        self._chk(self.lib.cgc_radius_knn(_ptr(pos), _ptr(gptr), num_graphs, n, ctypes.c_float(r), k, int(bool(loop)),
                                          _ptr(nbr), _ptr(cnt), _ptr(rowptr), _ptr(ws), self._stream()), 'cgc_radius_knn')
        nnz = int(rowptr[n].item())                    # the one host sync of graph construction: the edge count
        ei = torch.empty(2, nnz, dtype=torch.int64, device=dev)
        self._chk(self.lib.cgc_knn_emit_edges(_ptr(nbr), _ptr(rowptr), n, k, ctypes.c_int64(nnz), _ptr(ei), self._stream()),
                  'cgc_knn_emit_edges')
        return ei

    def nucleus_features(self, labels, gray, max_label, min_size, with_info=False):
        self._dev(labels, gray)
        assert labels.dtype == torch.int32 and gray.dtype == torch.uint8 and labels.dim() == 2 and labels.shape == gray.shape
        labels, gray = labels.contiguous(), gray.contiguous()
        H, W = labels.shape
        dev = labels.device
        u8, i32, f32 = (dict(dtype=d, device=dev) for d in (torch.uint8, torch.int32, torch.float32))
        ws = torch.empty(int(self.lib.cgc_nuclei_ws_bytes(max_label)), **u8)
        kept = torch.empty(max(max_label, 1), **i32)
        meta = torch.empty(4, **i32)
        self._chk(self.lib.cgc_nuclei_label_pass(_ptr(labels), H, W, max_label, int(min_size), _ptr(ws), _ptr(kept), _ptr(meta),
                                                 self._stream()), 'cgc_nuclei_label_pass')
        n, nbig, big_px, refused = meta.tolist()        # the host sync of this stage: the row count
        if refused:
            raise ValueError('%d pixels carry a label outside [0, %d]' % (refused, max_label))
        feats, cen = torch.empty(n, 16, **f32), torch.empty(n, 2, **f32)
        info = torch.empty(n, 4, **i32) if with_info else None
        big_ws = torch.empty(int(self.lib.cgc_nuclei_big_ws_bytes(nbig, ctypes.c_int64(big_px))), **u8) if nbig else None
        self._chk(self.lib.cgc_nuclei_features(_ptr(labels), _ptr(gray), H, W, max_label, int(min_size), _ptr(ws), _ptr(kept), n, nbig,
                                               ctypes.c_int64(big_px), _ptr(big_ws), _ptr(feats), _ptr(cen), _ptr(info), self._stream()),
                  'cgc_nuclei_features')
        return feats, cen, kept[:n], info

    def _image(self, t):
        """An image as the image kernels read it: on the current device, [H, W] of a 1-, 2-, 4- or 8-byte integer type or bool,
        contiguous (copied if not)."""
        self._dev(t)
        assert t is None or (t.dim() == 2 and t.element_size() in (1, 2, 4, 8) and not t.is_floating_point())
        return t if t is None else t.contiguous()

    def label_components(self, image, connectivity, min_size, want_sizes=False):
        image = self._image(image)
        H, W = image.shape
        dev = image.device
        i32 = dict(dtype=torch.int32, device=dev)
        counts = int(min_size > 1 or want_sizes)
        labels, nbuf = torch.empty(H, W, **i32), torch.empty(1, **i32)
        ws = torch.empty(int(self.lib.cgc_label_ws_bytes(H, W, counts)), dtype=torch.uint8, device=dev)
        self._chk(self.lib.cgc_label_components(_ptr(image), image.element_size(), H, W, int(connectivity), int(min_size), counts, _ptr(ws),
                                                _ptr(labels), _ptr(nbuf), self._stream()), 'cgc_label_components')
        n = int(nbuf.item())                            # the host sync of this stage: the component count
        sizes = None
        if want_sizes:
            sizes = torch.empty(n, **i32)
            self._chk(self.lib.cgc_label_sizes(_ptr(ws), H, W, n, _ptr(sizes), self._stream()), 'cgc_label_sizes')
        return labels, n, sizes

    def distance_transform(self, image, sites_nonzero, d2max, want_nearest=False):
        image = self._image(image)
        H, W = image.shape
        if H > EDT_MAX_SIDE or W > EDT_MAX_SIDE:
            raise ValueError('distance_transform takes images of at most %d x %d pixels (got %d x %d)' % (EDT_MAX_SIDE, EDT_MAX_SIDE, H, W))
        i32 = dict(dtype=torch.int32, device=image.device)
        dist2 = torch.empty(H, W, **i32)
        nearest = torch.empty(H, W, **i32) if want_nearest else None
        if H * W == 0:
            return dist2, nearest
        ws = torch.empty(int(self.lib.cgc_edt_ws_bytes(H, W)), dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_edt(_ptr(image), image.element_size(), H, W, int(bool(sites_nonzero)), int(d2max), _ptr(ws), _ptr(dist2),
                                   _ptr(nearest), self._stream()), 'cgc_edt')
        return dist2, nearest

    @staticmethod
    def _check_connectivity(connectivity):
        if connectivity not in (1, 2):
            raise ValueError('connectivity must be 1 or 2, got %r' % (connectivity,))

    @staticmethod
    def _check_steps(name, a, b, connectivity, H, W, what):
        """The refusals of a path relaxation, which need shapes only (before any copy): the step costs, the connectivity, and that no
        path's ``what`` ('cost', 'length') reaches 2^31."""
        if a < 1 or (b != 0 and not a <= b <= 2 * a):
            raise ValueError('%s needs steps 1 <= a <= b <= 2a or b == 0 (got a = %d, b = %d)' % (name, a, b))
        HipKernels._check_connectivity(connectivity)
        if (b or a) * H * W >= 2 ** 31:
            raise ValueError('%s: %d * %d * %d reaches 2^31: a path %s must fit int32' % (name, b or a, H, W, what))

    @staticmethod
    def _relax_until_still(launch, changed, first_batch, max_batch):
        """launch(first, count) enqueues launches first .. first + count - 1 of a stage of csrc/tile_relax.hpp, the last of which
        counts into ``changed`` what it moved.  Batches of first_batch, twice that, ... up to max_batch, one host read (the stage's
        host sync) after each, until a batch ends still.  Returns the launches done."""
        done, batch = 0, first_batch
        while True:
            launch(done, batch)
            done += batch
            if int(changed.item()) == 0:
                return done
            batch = min(2 * batch, max_batch)

    def geodesic_transform(self, seeds, within, a, b, connectivity, dmax, want_nearest=False):
        assert within is None or within.shape == seeds.shape
        H, W = seeds.shape
        a, b = int(a), int(b)
        HipKernels._check_steps('geodesic_transform', a, b, connectivity, H, W, 'cost')
        seeds, within = self._image(seeds), self._image(within)      # after the refusals: may copy
        dev = seeds.device
        i32 = dict(dtype=torch.int32, device=dev)
        dist = torch.empty(H, W, **i32)
        nearest = torch.empty(H, W, **i32) if want_nearest else None
        if H * W == 0:
            return dist, nearest
        ws = torch.empty(int(self.lib.cgc_geodesic_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
        changed = torch.empty(1, **i32)
        st = self._stream()
        self._chk(self.lib.cgc_geodesic_begin(_ptr(seeds), seeds.element_size(), _ptr(within), within.element_size() if within is not None else 0,
                                              H, W, a, b, _ptr(ws), st), 'cgc_geodesic_begin')
        self.geodesic_rounds = self._relax_until_still(                      # rounds launched by the last call (tests, tools)
            lambda first, count: self._chk(self.lib.cgc_geodesic_rounds(H, W, a, b, int(connectivity), int(dmax), _ptr(ws), first, count,
                                                                        _ptr(changed), st), 'cgc_geodesic_rounds'),
            changed, GEO_FIRST_BATCH, GEO_MAX_BATCH)
        self._chk(self.lib.cgc_geodesic_finish(H, W, _ptr(ws), _ptr(dist), _ptr(nearest), st), 'cgc_geodesic_finish')
        return dist, nearest

    def morph_reconstruct(self, marker, mask, connectivity, by_erosion=False):
        assert marker.dtype == torch.int32 and mask.dtype == torch.int32 and marker.shape == mask.shape
        HipKernels._check_connectivity(connectivity)      # by the class: the refusals need no instance
        marker, mask = self._image(marker), self._image(mask)      # after the refusal: may copy
        H, W = marker.shape
        dev = marker.device
        out = torch.empty(H, W, dtype=torch.int32, device=dev)
        self.reconstruct_rounds = 0                     # rounds launched by the last call (tests, tools)
        if H * W == 0:
            return out
        ws = torch.empty(int(self.lib.cgc_reconstruct_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
        changed = torch.empty(1, dtype=torch.int32, device=dev)
        st = self._stream()
        self._chk(self.lib.cgc_reconstruct_begin(_ptr(marker), _ptr(mask), H, W, int(bool(by_erosion)), _ptr(ws), st),
                  'cgc_reconstruct_begin')
        self.reconstruct_rounds = self._relax_until_still(
            lambda first, count: self._chk(self.lib.cgc_reconstruct_rounds(H, W, int(connectivity), _ptr(ws), first, count, _ptr(changed),
                                                                           st), 'cgc_reconstruct_rounds'),
            changed, GEO_FIRST_BATCH, GEO_MAX_BATCH)
        self._chk(self.lib.cgc_reconstruct_finish(H, W, int(bool(by_erosion)), _ptr(ws), _ptr(out), st), 'cgc_reconstruct_finish')
        return out

    def watershed_flood(self, height, seeds, within, a, b, connectivity):
        assert height.dtype == torch.int32 and height.shape == seeds.shape and (within is None or within.shape == seeds.shape)
        H, W = height.shape
        a, b = int(a), int(b)
        HipKernels._check_steps('watershed_flood', a, b, connectivity, H, W, 'length')
        height, seeds, within = self._image(height), self._image(seeds), self._image(within)      # after the refusals: may copy
        dev = height.device
        i32 = dict(dtype=torch.int32, device=dev)
        level, source = torch.empty(H, W, **i32), torch.empty(H, W, **i32)
        self.watershed_rounds = self.watershed_jumps = 0      # launches of the last call (tests, tools)
        if H * W == 0:
            return level, source
        ws = torch.empty(int(self.lib.cgc_watershed_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
        changed = torch.empty(1, **i32)
        st = self._stream()
        self._chk(self.lib.cgc_watershed_begin(_ptr(height), _ptr(seeds), seeds.element_size(), _ptr(within),
                                               within.element_size() if within is not None else 0, H, W, a, b, _ptr(ws), st),
                  'cgc_watershed_begin')
        self.watershed_rounds = self._relax_until_still(
            lambda first, count: self._chk(self.lib.cgc_watershed_rounds(H, W, a, b, int(connectivity), _ptr(ws), first, count,
                                                                         _ptr(changed), st), 'cgc_watershed_rounds'),
            changed, GEO_FIRST_BATCH, GEO_MAX_BATCH)
        self._chk(self.lib.cgc_watershed_parents(H, W, a, b, int(connectivity), _ptr(ws), st), 'cgc_watershed_parents')
        self.watershed_jumps = self._relax_until_still(                      # a constant batch: the entry takes no first jump
            lambda first, count: self._chk(self.lib.cgc_watershed_jumps(H, W, _ptr(ws), count, _ptr(changed), st), 'cgc_watershed_jumps'),
            changed, WS_JUMP_BATCH, WS_JUMP_BATCH)
        self._chk(self.lib.cgc_watershed_finish(H, W, _ptr(ws), _ptr(level), _ptr(source), st), 'cgc_watershed_finish')
        return level, source

    def bgr_to_gray(self, bgr):
        self._dev(bgr)
        assert bgr.dtype == torch.uint8 and bgr.dim() == 3 and bgr.shape[2] == 3
        bgr = bgr.contiguous()
        out = torch.empty(bgr.shape[0], bgr.shape[1], dtype=torch.uint8, device=bgr.device)
        self._chk(self.lib.cgc_bgr_to_gray(_ptr(bgr), ctypes.c_int64(out.numel()), _ptr(out), self._stream()), 'cgc_bgr_to_gray')
        return out

    @staticmethod
    def _check_stain_tables(order, lut, m, planes):
        """The refusals of stain_separate, which need no tensor: returns (lut, m) as flat lists of Python integers."""
        if order not in (0, 1):
            raise ValueError('stain_separate: order must be 0 (BGR) or 1 (RGB), got %r' % (order,))
        if planes not in range(1, 8):
            raise ValueError('stain_separate: planes must be a bit mask in 1..7, got %r' % (planes,))
        lut = [int(v) for v in lut]
        m = [int(v) for row in m for v in row]
        if len(lut) != 256 or min(lut) < 0 or max(lut) > STAIN_OD_MAX:
            raise ValueError('stain_separate: the optical-density table must hold 256 integers in [0, %d]' % STAIN_OD_MAX)
        if len(m) != 9:
            raise ValueError('stain_separate: the matrix must be 3 x 3')
        for s in range(3):
            if sum(abs(m[3 * c + s]) for c in range(3)) * STAIN_OD_MAX >= 2 ** 31 - 2 ** 15:
                raise ValueError('stain_separate: column %d of the matrix lets the int32 sum overflow (near-singular stains)' % s)
        return lut, m

    def stain_separate(self, image, order, lut, m, planes):
        lut, m = HipKernels._check_stain_tables(order, lut, m, planes)      # by the class: the refusals need no instance
        self._dev(image)
        assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
        image = image.contiguous()
        H, W = image.shape[:2]
        out = torch.empty(bin(planes).count('1'), H, W, dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_stain_separate(_ptr(image), ctypes.c_int64(H * W), int(order), (ctypes.c_int * 256)(*lut),
                                              (ctypes.c_int * 9)(*m), int(planes), _ptr(out), self._stream()), 'cgc_stain_separate')
        return out

    def histogram_u8(self, image, within=None):
        assert image.dtype == torch.uint8 and (within is None or within.shape == image.shape)
        image, within = self._image(image), self._image(within)
        hist = torch.empty(256, dtype=torch.int32, device=image.device)
        self._chk(self.lib.cgc_histogram_u8(_ptr(image), ctypes.c_int64(image.numel()), _ptr(within),
                                            within.element_size() if within is not None else 0, _ptr(hist), self._stream()),
                  'cgc_histogram_u8')
        return hist

    @staticmethod
    def _check_scan_tables(fn, order, lut, od_min):
        """The refusals od_moments and angle_histogram share, which need no tensor: returns lut as a list of Python integers."""
        if order not in (0, 1):
            raise ValueError('%s: order must be 0 (BGR) or 1 (RGB), got %r' % (fn, order))
        lut = [int(v) for v in lut]
        if len(lut) != 256 or min(lut) < 0 or max(lut) > STAIN_OD_MAX:
            raise ValueError('%s: the optical-density table must hold 256 integers in [0, %d]' % (fn, STAIN_OD_MAX))
        if isinstance(od_min, bool) or od_min not in range(0, STAIN_OD_MAX + 1):
            raise ValueError('%s: od_min must be an integer in 0..%d, got %r' % (fn, STAIN_OD_MAX, od_min))
        return lut

    @staticmethod
    def _check_basis(basis):
        """The refusals of angle_histogram's basis: returns it as a flat list of Python integers."""
        try:
            basis = [[int(v) for v in row] for row in basis]
        except (TypeError, ValueError):
            raise ValueError('angle_histogram: the basis must be 2 x 3 integers')
        if len(basis) != 2 or any(len(row) != 3 for row in basis):
            raise ValueError('angle_histogram: the basis must be 2 x 3')
        for row in basis:
            if max(abs(v) for v in row) > ANGLE_E_MAX or sum(abs(v) for v in row) > ANGLE_E_REACH:
                raise ValueError('angle_histogram: a basis row needs |E| <= %d and sum |E| <= %d (got %r)' % (ANGLE_E_MAX, ANGLE_E_REACH, row))
        return [v for row in basis for v in row]

    @staticmethod
    def _check_angle_tables(basis, dirs):
        """The refusals of angle_histogram's basis and directions, which need no tensor: returns both as flat lists of integers."""
        basis = HipKernels._check_basis(basis)
        try:
            key = tuple(tuple(d) for d in dirs)
        except TypeError:
            raise ValueError('angle_histogram: dirs must be %d x 2 integers' % (ANGLE_BINS - 1))
        return basis, list(_checked_dirs(key))

    def _scan_images(self, image, within):
        self._dev(image)
        assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
        assert within is None or tuple(within.shape) == tuple(image.shape[:2])
        return image.contiguous(), self._image(within)

    def od_moments(self, image, order, lut, od_min, within=None):
        lut = HipKernels._check_scan_tables('od_moments', order, lut, od_min)
        image, within = self._scan_images(image, within)
        out = torch.empty(10, dtype=torch.int64, device=image.device)
        self._chk(self.lib.cgc_od_moments(_ptr(image), ctypes.c_int64(image.shape[0] * image.shape[1]), int(order),
                                          (ctypes.c_int * 256)(*lut), int(od_min), _ptr(within),
                                          within.element_size() if within is not None else 0, _ptr(out), self._stream()), 'cgc_od_moments')
        return out

    def angle_histogram(self, image, order, lut, od_min, basis, dirs, within=None):
        lut = HipKernels._check_scan_tables('angle_histogram', order, lut, od_min)
        if self is not None and dirs is self._dirs_checked[0]:      # the same deeply immutable table as last time: checked, marshalled
            basis, dirs_c = HipKernels._check_basis(basis), self._dirs_checked[1]
        else:
            basis, flat = HipKernels._check_angle_tables(basis, dirs)
            dirs_c = (ctypes.c_int * len(flat))(*flat)
            if self is not None and type(dirs) is tuple and all(type(d) is tuple and type(d[0]) is int and type(d[1]) is int for d in dirs):
                self._dirs_checked = (dirs, dirs_c)
        image, within = self._scan_images(image, within)
        out = torch.empty(ANGLE_BINS + 1, dtype=torch.int32, device=image.device)
        ws = torch.empty(int(self.lib.cgc_angle_histogram_ws_bytes()), dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_angle_histogram(_ptr(image), ctypes.c_int64(image.shape[0] * image.shape[1]), int(order),
                                               (ctypes.c_int * 256)(*lut), int(od_min), (ctypes.c_int * 6)(*basis),
                                               dirs_c, _ptr(within),
                                               within.element_size() if within is not None else 0, _ptr(ws), _ptr(out), self._stream()),
                  'cgc_angle_histogram')
        return out

    @staticmethod
    def _check_od_matrix(fn, m, slack):
        """A 3 x 3 integer matrix no column of which lets an int32 sum of optical densities overflow: sum_c |m[c][s]| * 5674 <
        2^31 - slack.  Returns it as a flat list of Python integers."""
        try:
            m = [[operator.index(v) for v in row] for row in m]      # no float, however integral: int() would truncate 0.9 to 0
        except TypeError:
            raise ValueError('%s: the matrix must be 3 x 3 integers' % fn)
        if len(m) != 3 or any(len(row) != 3 for row in m):
            raise ValueError('%s: the matrix must be 3 x 3' % fn)
        for s in range(3):
            if sum(abs(m[c][s]) for c in range(3)) * STAIN_OD_MAX >= 2 ** 31 - slack:
                raise ValueError('%s: column %d of the matrix lets the int32 sum overflow' % (fn, s))
        return [v for row in m for v in row]

    @staticmethod
    def _check_concentration_tables(order, lut, od_min, m):
        """The refusals of concentration_histogram, which need no tensor: returns (lut, m) as flat lists of Python integers."""
        lut = HipKernels._check_scan_tables('concentration_histogram', order, lut, od_min)
        return lut, HipKernels._check_od_matrix('concentration_histogram', m, 2 ** 15)

    @staticmethod
    def _check_exp_lut(exp_lut):
        """The refusals of od_recolor's exponential table: returns it as a list of Python integers."""
        try:
            e = [operator.index(v) for v in exp_lut]
        except TypeError:
            raise ValueError('od_recolor: the exponential table must hold %d integers' % EXP_LUT_LEN)
        if len(e) != EXP_LUT_LEN or min(e) < 0 or max(e) > 255:
            raise ValueError('od_recolor: the exponential table must hold %d integers in [0, 255]' % EXP_LUT_LEN)
        if e[0] != 255 or e[-1] != 0 or any(x < y for x, y in zip(e, e[1:])):
            raise ValueError('od_recolor: the exponential table must start at 255, end at 0 and never rise')
        return e

    @staticmethod
    def _check_recolor_map(order, lut, a):
        """The refusals of od_recolor's order, optical-density table and matrix: returns (lut, a) as flat lists of Python integers."""
        if order not in (0, 1):
            raise ValueError('od_recolor: order must be 0 (BGR) or 1 (RGB), got %r' % (order,))
        try:
            lut = [operator.index(v) for v in lut]
        except TypeError:
            raise ValueError('od_recolor: the optical-density table must hold 256 integers in [0, %d]' % STAIN_OD_MAX)
        if len(lut) != 256 or min(lut) < 0 or max(lut) > STAIN_OD_MAX:
            raise ValueError('od_recolor: the optical-density table must hold 256 integers in [0, %d]' % STAIN_OD_MAX)
        return lut, HipKernels._check_od_matrix('od_recolor', a, 2 ** 11)

    @staticmethod
    def _check_recolor_tables(order, lut, a, exp_lut):
        """The refusals of od_recolor, which need no tensor: returns (lut, a, exp_lut) as flat lists of Python integers."""
        return HipKernels._check_recolor_map(order, lut, a) + (HipKernels._check_exp_lut(exp_lut),)

    def concentration_histogram(self, image, order, lut, od_min, m, within=None):
        lut, m = HipKernels._check_concentration_tables(order, lut, od_min, m)
        image, within = self._scan_images(image, within)
        out = torch.empty(2 * CONC_BINS, dtype=torch.int32, device=image.device)
        self._chk(self.lib.cgc_concentration_histogram(_ptr(image), ctypes.c_int64(image.shape[0] * image.shape[1]), int(order),
                                                       (ctypes.c_int * 256)(*lut), int(od_min), (ctypes.c_int * 9)(*m), _ptr(within),
                                                       within.element_size() if within is not None else 0, _ptr(out), self._stream()),
                  'cgc_concentration_histogram')
        return out

    def od_recolor(self, image, order, lut, a, exp_lut):
        if self is not None and exp_lut is self._exp_checked[0]:      # the same deeply immutable table as last time: checked, marshalled
            (lut, a), exp_c = HipKernels._check_recolor_map(order, lut, a), self._exp_checked[1]
        else:
            lut, a, e = HipKernels._check_recolor_tables(order, lut, a, exp_lut)
            exp_c = (ctypes.c_int * EXP_LUT_LEN)(*e)
            if self is not None and type(exp_lut) is tuple and all(type(v) is int for v in exp_lut):
                self._exp_checked = (exp_lut, exp_c)
        self._dev(image)
        assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
        image = image.contiguous()
        H, W = image.shape[:2]
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=image.device)
        ws = torch.empty(int(self.lib.cgc_od_recolor_ws_bytes()), dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_od_recolor(_ptr(image), ctypes.c_int64(H * W), int(order), (ctypes.c_int * 256)(*lut),
                                          (ctypes.c_int * 9)(*a), exp_c, EXP_LUT_LEN, _ptr(ws), _ptr(out), self._stream()),
                  'cgc_od_recolor')
        return out

    @staticmethod
    def _check_resample(fn, shape, size, mode, modes):
        """The refusals of resample_u8 / resample_labels, which need no tensor: returns (H2, W2, the library's mode)."""
        if not isinstance(mode, str) or mode not in modes:
            raise ValueError('%s: mode must be %s, got %r' % (fn, ' or '.join(repr(k) for k in modes), mode))
        try:
            H2, W2 = (operator.index(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError('%s: size must be a pair of integers (H2, W2), got %r' % (fn, size))
        H, W = int(shape[0]), int(shape[1])
        if H < 1 or W < 1:
            raise ValueError('%s: the image must not be empty (got %d x %d)' % (fn, H, W))
        if max(H, W) > RESAMPLE_MAX_SIDE:
            raise ValueError('%s: the image may have sides up to %d (got %d x %d)' % (fn, RESAMPLE_MAX_SIDE, H, W))
        if not (1 <= H2 <= RESAMPLE_MAX_SIDE and 1 <= W2 <= RESAMPLE_MAX_SIDE):
            raise ValueError('%s: size must lie in 1..%d on both axes (got %d x %d)' % (fn, RESAMPLE_MAX_SIDE, H2, W2))
        if mode in ('area', 'majority') and (H2 > H or W2 > W):
            raise ValueError("%s: mode %r only shrinks: size %d x %d exceeds the image's %d x %d" % (fn, mode, H2, W2, H, W))
        if mode == 'majority' and (H > RESAMPLE_LABELS_MAX_FACTOR * H2 or W > RESAMPLE_LABELS_MAX_FACTOR * W2):
            raise ValueError("%s: mode 'majority' shrinks by at most %d per axis (size %d x %d from %d x %d): repeat the call"
                             % (fn, RESAMPLE_LABELS_MAX_FACTOR, H2, W2, H, W))
        return H2, W2, modes[mode]

    def resample_u8(self, image, size, mode):
        H2, W2, code = HipKernels._check_resample('resample_u8', image.shape, size, mode, RESAMPLE_MODES)
        self._dev(image)
        assert image.dtype == torch.uint8 and (image.dim() == 2 or (image.dim() == 3 and image.shape[2] == 3))
        image = image.contiguous()
        H, W = image.shape[:2]
        out = torch.empty((H2, W2) + tuple(image.shape[2:]), dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_resample_u8(_ptr(image), H, W, 1 if image.dim() == 2 else 3, H2, W2, code, _ptr(out), self._stream()),
                  'cgc_resample_u8')
        return out

    def resample_labels(self, labels, size, mode):
        H2, W2, code = HipKernels._check_resample('resample_labels', labels.shape, size, mode, RESAMPLE_LABEL_MODES)
        labels = self._image(labels)
        if code == 1 and labels.dtype in (torch.uint8, torch.bool):
            code = 2                                                            # CGC_RESAMPLE_MAJORITY_UNSIGNED
        H, W = labels.shape
        out = torch.empty(H2, W2, dtype=labels.dtype, device=labels.device)
        self._chk(self.lib.cgc_resample_labels(_ptr(labels), labels.element_size(), H, W, H2, W2, code, _ptr(out), self._stream()),
                  'cgc_resample_labels')
        return out

    def binomial_smooth(self, image, radius):
        if radius not in range(0, SMOOTH_MAX_RADIUS + 1):
            raise ValueError('binomial_smooth: radius must be an integer in 0..%d, got %r' % (SMOOTH_MAX_RADIUS, radius))
        assert image.dtype == torch.uint8
        image = self._image(image)
        H, W = image.shape
        out = torch.empty(H, W, dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_binomial_smooth_u8(_ptr(image), H, W, int(radius), _ptr(out), self._stream()), 'cgc_binomial_smooth_u8')
        return out

    @staticmethod
    def _check_flat_radius(fn, radius, top, what=''):
        """The radius of a flat-window stage: an int (no bool) in 0..top; ``what`` names the case a smaller ``top`` belongs to."""
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= top:
            raise ValueError('%s: radius must be an integer in 0..%d%s, got %r' % (fn, top, what, radius))

    @staticmethod
    def _check_footprint_kind(fn, kind):
        if not isinstance(kind, str) or kind not in MORPH_KINDS:
            raise ValueError("%s: kind must be 'square', 'disk' or 'diamond', got %r" % (fn, kind))

    @staticmethod
    def _check_rule(k64, offset, floor):
        for name, value, lo, hi in (('k64', k64, -128, 128), ('offset', offset, -255, 255), ('floor', floor, -1, 255)):
            if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
                raise ValueError('local_threshold: %s must be an integer in %d..%d, got %r' % (name, lo, hi, value))

    def _window_images(self, image, within):
        assert image.dtype == torch.uint8 and (within is None or within.shape == image.shape)
        return self._image(image), self._image(within)      # after the refusals: may copy

    def window_strip_cols(self, radius):
        """Columns of the tiles of window_sums / local_threshold at this radius (tests place windows across tile edges)."""
        return int(self.lib.cgc_window_strip_cols(int(radius)))

    def window_sums(self, image, radius, within=None):
        HipKernels._check_flat_radius('window_sums', radius, WINDOW_MAX_RADIUS)
        image, within = self._window_images(image, within)
        H, W = image.shape
        n, s = (torch.empty(H, W, dtype=torch.int32, device=image.device) for _ in range(2))
        q = torch.empty(H, W, dtype=torch.int64, device=image.device)
        self._chk(self.lib.cgc_window_sums(_ptr(image), *_within_args(within), H, W, radius,
                                           _ptr(n), _ptr(s), _ptr(q), self._stream()), 'cgc_window_sums')
        return n, s, q

    def local_threshold(self, image, radius, k64, offset, floor, within=None):
        HipKernels._check_flat_radius('local_threshold', radius, WINDOW_MAX_RADIUS)
        HipKernels._check_rule(k64, offset, floor)
        image, within = self._window_images(image, within)
        H, W = image.shape
        out = torch.empty(H, W, dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_local_threshold(_ptr(image), *_within_args(within), H, W,
                                               radius, k64, offset, floor, _ptr(out), self._stream()), 'cgc_local_threshold')
        return out

    @staticmethod
    def _check_morph(kind, radius, op, other, epilogue):
        """The refusals of flat_morphology that need no tensor: returns the library's codes (kind, op, epilogue)."""
        HipKernels._check_footprint_kind('flat_morphology', kind)
        HipKernels._check_flat_radius('flat_morphology', radius, MORPH_MAX_RADIUS)
        if not isinstance(op, str) or op not in MORPH_OPS:
            raise ValueError("flat_morphology: op must be 'erode', 'dilate' or 'gradient', got %r" % (op,))
        if not (epilogue is None or isinstance(epilogue, str)) or epilogue not in MORPH_EPILOGUES:
            raise ValueError("flat_morphology: epilogue must be None, 'other_minus' or 'minus_other', got %r" % (epilogue,))
        if (other is None) != (epilogue is None):
            raise ValueError('flat_morphology: other and epilogue come together or not at all')
        return MORPH_KINDS[kind], MORPH_OPS[op], MORPH_EPILOGUES[epilogue]

    def morph_tile_cols(self, radius):
        """Columns of the tiles of flat_morphology at this radius (tests place footprints across tile edges)."""
        return int(self.lib.cgc_morph_tile_cols(int(radius)))

    def flat_morphology(self, image, kind, radius, op, within=None, other=None, epilogue=None):
        kind, op, epilogue = HipKernels._check_morph(kind, radius, op, other, epilogue)
        assert image.dtype == torch.uint8 and (within is None or within.shape == image.shape)
        assert other is None or (other.dtype == torch.uint8 and other.shape == image.shape)
        image, within, other = self._image(image), self._image(within), self._image(other)      # after the refusals: may copy
        H, W = image.shape
        out = torch.empty(H, W, dtype=torch.uint8, device=image.device)
        self._chk(self.lib.cgc_morph(_ptr(image), *_within_args(within), H, W, kind, radius,
                                     op, _ptr(other), epilogue, _ptr(out), self._stream()), 'cgc_morph')
        return out

    @staticmethod
    def _check_rank(kind, radius, op, q_lo, q_hi):
        """The refusals of rank_filter that need no tensor: returns the library's codes (kind, op)."""
        HipKernels._check_footprint_kind('rank_filter', kind)
        if not isinstance(op, str) or op not in RANK_OPS:
            raise ValueError("rank_filter: op must be 'quantile', 'range' or 'entropy', got %r" % (op,))
        HipKernels._check_flat_radius('rank_filter', radius, ENTROPY_MAX_RADIUS if op == 'entropy' else RANK_MAX_RADIUS, ' for %r' % (op,))
        for name, q in (('q_lo', q_lo), ('q_hi', q_hi)):
            if isinstance(q, bool) or not isinstance(q, int) or not 0 <= q <= 10000:
                raise ValueError('rank_filter: %s must be an integer in 0..10000, got %r' % (name, q))
        if q_lo > q_hi:
            raise ValueError('rank_filter: q_lo <= q_hi (got %d > %d)' % (q_lo, q_hi))
        return MORPH_KINDS[kind], RANK_OPS[op]

    def rank_tile_cols(self, radius):
        """Columns of the tiles of rank_filter at this radius (tests place footprints across tile edges)."""
        return int(self.lib.cgc_rank_tile_cols(int(radius)))

    def rank_entropy_term(self, c):
        """T[c] = round(c log2(c) 2^16) of rank_filter's entropy, c in 0..961, from the library's table (host only)."""
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < RANK_ENTROPY_TERMS:
            raise ValueError('rank_entropy_term: c must be an integer in 0..%d, got %r' % (RANK_ENTROPY_TERMS - 1, c))
        return int(self.lib.cgc_rank_entropy_term(c))

    def rank_filter(self, image, kind, radius, op, q_lo=0, q_hi=0, within=None):
        kind, op = HipKernels._check_rank(kind, radius, op, q_lo, q_hi)
        assert image.dtype == torch.uint8 and (within is None or within.shape == image.shape)
        image, within = self._image(image), self._image(within)               # after the refusals: may copy
        H, W = image.shape
        out = torch.empty(H, W, dtype=torch.int32 if op == RANK_OPS['entropy'] else torch.uint8, device=image.device)
        self._chk(self.lib.cgc_rank_filter(_ptr(image), *_within_args(within), H, W, kind,
                                           radius, op, q_lo, q_hi, _ptr(out), self._stream()), 'cgc_rank_filter')
        return out

    def region_adjacency(self, labels, connectivity, value=None):
        HipKernels._check_connectivity(connectivity)
        labels, value = self._image(labels), self._image(value)
        assert labels.dtype == torch.int32 and (value is None or (value.dtype == torch.int32 and value.shape == labels.shape))
        H, W = labels.shape
        if H * W >= ADJ_MAX_PIXELS:
            raise ValueError('region_adjacency takes images of fewer than 2^29 pixels (got %d x %d): a count must fit int32' % (H, W))
        dev = labels.device
        u8, i32, i64 = (dict(dtype=d, device=dev) for d in (torch.uint8, torch.int32, torch.int64))
        empty = (torch.empty(0, 2, **i32), torch.empty(0, **i32), None if value is None else torch.empty(0, **i32))
        if H * W == 0:
            return empty
        ws = torch.empty(int(self.lib.cgc_adjacency_ws_bytes(H, W)), **u8)
        nbuf = torch.empty(2, **i32)
        self._chk(self.lib.cgc_adjacency_count(_ptr(labels), H, W, int(connectivity), _ptr(ws), _ptr(nbuf), self._stream()),
                  'cgc_adjacency_count')
        nrec = int(nbuf[0].item())                      # host sync 1 of this stage: the records the tiles will write
        if nrec == 0:
            return empty
        keys, cnts = torch.empty(nrec, **i64), torch.empty(nrec, **i32)
        sums = None if value is None else torch.empty(nrec, **i32)
        self._chk(self.lib.cgc_adjacency_records(_ptr(labels), _ptr(value), H, W, int(connectivity), _ptr(ws), ctypes.c_int64(nrec),
                                                 _ptr(keys), _ptr(cnts), _ptr(sums), self._stream()), 'cgc_adjacency_records')
        keys, perm = torch.sort(keys)                   # the order of equal keys does not matter: their records are summed
        mws = torch.empty(int(self.lib.cgc_adjacency_merge_ws_bytes(ctypes.c_int64(nrec))), **u8)
        self._chk(self.lib.cgc_adjacency_heads(_ptr(keys), ctypes.c_int64(nrec), _ptr(mws), _ptr(nbuf[1:]), self._stream()),
                  'cgc_adjacency_heads')
        npairs = int(nbuf[1].item())                    # host sync 2: the distinct pairs
        pairs, count = torch.empty(npairs, 2, **i32), torch.empty(npairs, **i32)
        min_sum = None if value is None else torch.empty(npairs, **i32)
        self._chk(self.lib.cgc_adjacency_merge(_ptr(keys), _ptr(perm), _ptr(cnts), _ptr(sums), ctypes.c_int64(nrec), _ptr(mws), npairs,
                                               _ptr(pairs), _ptr(count), _ptr(min_sum), self._stream()), 'cgc_adjacency_merge')
        return pairs, count, min_sum

    @staticmethod
    def _check_max_label(fn, max_label):
        if isinstance(max_label, bool) or not isinstance(max_label, int) or not 0 <= max_label < 2 ** 31 - 1:
            raise ValueError('%s: max_label must be an integer in 0..2^31 - 2, got %r' % (fn, max_label))

    @staticmethod
    def _check_q10k(q10k):
        """The refusals of region_quantiles that need no tensor: returns the quantiles as a C array."""
        try:
            q10k = list(q10k)
        except TypeError:
            raise ValueError('region_quantiles: q10k must be a sequence of integers in 0..10000, got %r' % (q10k,))
        if not 1 <= len(q10k) <= REGION_MAX_QUANTILES:
            raise ValueError('region_quantiles: q10k takes 1 to %d quantiles, got %d' % (REGION_MAX_QUANTILES, len(q10k)))
        for q in q10k:
            if isinstance(q, bool) or not isinstance(q, int) or not 0 <= q <= 10000:
                raise ValueError('region_quantiles: q10k must hold integers in 0..10000, got %r' % (q,))
        return (ctypes.c_int * len(q10k))(*q10k)

    def _region_inputs(self, labels, values, within, max_label):
        """labels as contiguous int32 (any integer dtype is taken; what does not fit int32 stays outside [0, max_label]), values and
        within contiguous: after the refusals, may copy."""
        assert not labels.is_floating_point() and labels.dtype != torch.bool
        if labels.dtype == torch.int64:
            labels = labels.clamp(-1, max_label + 1)
        labels, values, within = self._image(labels.to(torch.int32)), self._image(values), self._image(within)
        assert values.shape == labels.shape and (within is None or within.shape == labels.shape)
        return labels, values, within

    def region_statistics(self, labels, values, max_label, within=None):
        HipKernels._check_max_label('region_statistics', max_label)
        if values.dtype not in REGION_VALUE_DTYPES:
            raise TypeError('region_statistics: values must be uint8, int8, int16 or int32, got %s' % values.dtype)
        labels, values, within = self._region_inputs(labels, values, within, max_label)
        H, W = labels.shape
        dev = labels.device
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        R = max_label + 1
        ints = torch.empty(5, R, **i32)                                         # count, min, max, argmin, argmax
        wide = torch.empty(1 if values.dtype == torch.int32 else 2, R, **i64)    # sum, sumsq
        sumsq = wide[1] if wide.shape[0] == 2 else None
        meta = torch.empty(1, **i32)
        ws = torch.empty(int(self.lib.cgc_region_ws_bytes(max_label)), dtype=torch.uint8, device=dev)
        vbytes, vsigned = REGION_VALUE_DTYPES[values.dtype]
        self._chk(self.lib.cgc_region_moments(_ptr(labels), _ptr(values), vbytes, vsigned, *_within_args(within), H, W, max_label, _ptr(ws),
                                              _ptr(ints[0]), _ptr(wide[0]), _ptr(sumsq), _ptr(ints[1]), _ptr(ints[2]), _ptr(ints[3]),
                                              _ptr(ints[4]), _ptr(meta), self._stream()), 'cgc_region_moments')
        return (ints[0], wide[0], sumsq, ints[1], ints[2], ints[3], ints[4]), meta

    def region_histogram(self, labels, values, max_label, within=None):
        HipKernels._check_max_label('region_histogram', max_label)
        if values.dtype != torch.uint8:
            raise TypeError('region_histogram: values must be uint8, got %s' % values.dtype)
        labels, values, within = self._region_inputs(labels, values, within, max_label)
        H, W = labels.shape
        hist = torch.empty(max_label + 1, 256, dtype=torch.int32, device=labels.device)
        meta = torch.empty(1, dtype=torch.int32, device=labels.device)
        self._chk(self.lib.cgc_region_histogram(_ptr(labels), _ptr(values), *_within_args(within), H, W, max_label, _ptr(hist), _ptr(meta),
                                                self._stream()), 'cgc_region_histogram')
        return hist, meta

    @staticmethod
    def _check_cooc(lut, levels, offsets):
        """The refusals of region_cooccurrence that need no tensor: returns (the lut as 256 C bytes, the offsets as a C array)."""
        fn = 'region_cooccurrence'
        if isinstance(levels, bool) or not isinstance(levels, int) or not 2 <= levels <= COOC_MAX_LEVELS:
            raise ValueError('%s: levels must be an integer in 2..%d, got %r' % (fn, COOC_MAX_LEVELS, levels))
        try:
            lut = [operator.index(v) for v in lut]
        except TypeError:
            raise ValueError('%s: lut must be a sequence of 256 integers below levels' % fn)
        if len(lut) != 256:
            raise ValueError('%s: lut must hold 256 entries, got %d' % (fn, len(lut)))
        if any(not 0 <= v < levels for v in lut):
            raise ValueError('%s: every entry of lut must lie in 0..%d' % (fn, levels - 1))
        try:
            offsets = [(operator.index(dy), operator.index(dx)) for dy, dx in offsets]
        except (TypeError, ValueError):
            raise ValueError('%s: offsets must be a sequence of pairs (dy, dx) of integers, got %r' % (fn, offsets))
        if not 1 <= len(offsets) <= COOC_MAX_OFFSETS:
            raise ValueError('%s: offsets takes 1 to %d offsets, got %d' % (fn, COOC_MAX_OFFSETS, len(offsets)))
        for dy, dx in offsets:
            if (dy, dx) == (0, 0) or abs(dy) > COOC_MAX_OFFSET or abs(dx) > COOC_MAX_OFFSET:
                raise ValueError('%s: an offset must not be (0, 0) and |dy|, |dx| must not pass %d, got %r' % (fn, COOC_MAX_OFFSET, (dy, dx)))
        return (ctypes.c_uint8 * 256)(*lut), (ctypes.c_int * (2 * len(offsets)))(*[v for o in offsets for v in o])

    def region_cooccurrence(self, labels, values, max_label, lut, levels, offsets, symmetric, within=None):
        HipKernels._check_max_label('region_cooccurrence', max_label)
        lut, offs = HipKernels._check_cooc(lut, levels, offsets)
        if values.dtype != torch.uint8:
            raise TypeError('region_cooccurrence: values must be uint8, got %s' % values.dtype)
        labels, values, within = self._region_inputs(labels, values, within, max_label)
        H, W = labels.shape
        if H * W >= COOC_MAX_PIXELS:
            raise ValueError('region_cooccurrence takes images of fewer than 2^30 pixels (got %d x %d): a count must fit int32' % (H, W))
        noff = len(offs) // 2
        tables = torch.empty(max_label + 1, noff, levels * levels, dtype=torch.int32, device=labels.device)
        meta = torch.empty(1, dtype=torch.int32, device=labels.device)
        self._chk(self.lib.cgc_region_cooccurrence(_ptr(labels), _ptr(values), *_within_args(within), H, W, max_label, lut, levels, offs,
                                                   noff, 1 if symmetric else 0, _ptr(tables), _ptr(meta), self._stream()),
                  'cgc_region_cooccurrence')
        return tables, meta

    @staticmethod
    def _check_geometry_dims(fn, H, W):
        if H > GEOMETRY_MAX_SIDE or W > GEOMETRY_MAX_SIDE:
            raise ValueError('%s takes images of sides up to %d (got %d x %d): the coordinate sums must fit int64' % (fn, GEOMETRY_MAX_SIDE, H, W))
        if (H + 1) * (W + 1) >= 2 ** 31:
            raise ValueError('%s takes images with (H + 1)(W + 1) < 2^31 (got %d x %d): a quad count must fit int32' % (fn, H, W))

    def region_geometry(self, labels, max_label, within=None):
        HipKernels._check_max_label('region_geometry', max_label)
        HipKernels._check_geometry_dims('region_geometry', *labels.shape)
        assert not labels.is_floating_point() and labels.dtype != torch.bool
        if labels.dtype == torch.int64:                                         # as _region_inputs: what does not fit int32 stays refused
            labels = labels.clamp(-1, max_label + 1)
        labels, within = self._image(labels.to(torch.int32)), self._image(within)
        assert within is None or within.shape == labels.shape
        H, W = labels.shape
        dev = labels.device
        R = max_label + 1
        ints = torch.empty(R * 22, dtype=torch.int32, device=dev)                  # count, border, quads, extents
        count, border, quads, extents = ints[:R], ints[R:2 * R], ints[2 * R:6 * R].view(R, 4), ints[6 * R:].view(R, 8, 2)
        sums = torch.empty(5, R, dtype=torch.int64, device=dev)
        meta = torch.empty(1, dtype=torch.int32, device=dev)
        self._chk(self.lib.cgc_region_geometry(_ptr(labels), *_within_args(within), H, W, max_label, _ptr(count), _ptr(sums), _ptr(extents),
                                               _ptr(quads), _ptr(border), _ptr(meta), self._stream()), 'cgc_region_geometry')
        return (count, sums, extents, quads, border), meta

    def region_hull_ptr(self, count, extents):
        self._dev(count, extents)
        e = extents.to(torch.int64)
        rows = torch.where(count > 0, e[:, 4, 1] - e[:, 4, 0] + 1, torch.zeros_like(e[:, 4, 0]))
        ptr = torch.zeros(count.shape[0] + 1, dtype=torch.int64, device=count.device)
        torch.cumsum(rows, 0, out=ptr[1:])
        return ptr

    @staticmethod
    def _check_hull_rows(max_label, H, span_rows, tall_rows):
        for name, v in (('span_rows', span_rows), ('tall_rows', tall_rows)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError('region_hull: %s must be a non-negative integer, got %r' % (name, v))
        if span_rows > (max_label + 1) * H:
            raise ValueError('region_hull: span_rows = %d does not fit %d labels of at most %d rows' % (span_rows, max_label + 1, H))

    def region_hull(self, labels, max_label, extents, ptr, span_rows, within=None, tall_rows=0):
        HipKernels._check_max_label('region_hull', max_label)
        HipKernels._check_geometry_dims('region_hull', *labels.shape)
        HipKernels._check_hull_rows(max_label, labels.shape[0], span_rows, tall_rows)
        assert not labels.is_floating_point() and labels.dtype != torch.bool
        if labels.dtype == torch.int64:                                         # as _region_inputs: what does not fit int32 stays refused
            labels = labels.clamp(-1, max_label + 1)
        labels, within = self._image(labels.to(torch.int32)), self._image(within)
        assert within is None or within.shape == labels.shape
        self._dev(extents, ptr)
        H, W = labels.shape
        dev = labels.device
        R = max_label + 1
        assert extents.dtype == torch.int32 and tuple(extents.shape) == (R, 8, 2) and extents.is_contiguous()
        assert ptr.dtype == torch.int64 and tuple(ptr.shape) == (R + 1,) and ptr.is_contiguous()
        spans = torch.empty(span_rows, 2, dtype=torch.int32, device=dev)
        ws_bytes = int(self.lib.cgc_region_hull_ws_bytes(max_label, ctypes.c_int64(span_rows)))
        assert ws_bytes >= 2 * (span_rows + R) * 8
        points = torch.empty(ws_bytes // 8, 2, dtype=torch.int32, device=dev)
        ints = torch.empty(R * 7, dtype=torch.int32, device=dev)                   # count, width_edge, diameter_ends
        count, width_edge, ends = ints[:R], ints[R:3 * R].view(R, 2), ints[3 * R:].view(R, 2, 2)
        wide = torch.empty(3, R, dtype=torch.int64, device=dev)                    # area2, diameter2, width_cross
        perimeter = torch.empty(R, dtype=torch.float64, device=dev)
        self._chk(self.lib.cgc_region_hull_spans(_ptr(labels), *_within_args(within), H, W, max_label, _ptr(extents), _ptr(ptr),
                                                 ctypes.c_int64(span_rows), _ptr(spans) if span_rows else None, self._stream()),
                  'cgc_region_hull_spans')
        self._chk(self.lib.cgc_region_hull(max_label, H, _ptr(extents), _ptr(ptr), ctypes.c_int64(span_rows),
                                           _ptr(spans) if span_rows else None, _ptr(points), tall_rows, _ptr(count), _ptr(wide[0]),
                                           _ptr(wide[1]), _ptr(ends), _ptr(wide[2]), _ptr(width_edge), _ptr(perimeter), self._stream()),
                  'cgc_region_hull')
        return (count, wide[0], wide[1], ends, wide[2], width_edge, perimeter), points[:2 * (span_rows + R)]

    @staticmethod
    def _check_outline(H, W, connectivity, mode):
        """The refusals of region_outlines that need shapes only."""
        HipKernels._check_geometry_dims('region_outlines', H, W)
        if H * W >= OUTLINE_MAX_PIXELS:
            raise ValueError('region_outlines takes images of fewer than 2^29 pixels (got %d x %d): a crack id must fit int32' % (H, W))
        if isinstance(connectivity, bool) or connectivity not in (1, 2):
            raise ValueError('region_outlines: connectivity must be 1 or 2, got %r' % (connectivity,))
        if mode not in OUTLINE_MODES:
            raise ValueError("region_outlines: mode must be 'corners' or 'cracks', got %r" % (mode,))

    def region_outline_rounds(self, n_cracks):
        """The doubling rounds of each phase for ``n_cracks`` cracks: the smallest r with 2^r >= n_cracks."""
        return int(self.lib.cgc_region_outline_rounds(ctypes.c_int64(n_cracks)))

    def region_outlines(self, labels, max_label, connectivity=1, within=None, mode='corners', background=False):
        HipKernels._check_max_label('region_outlines', max_label)
        HipKernels._check_outline(labels.shape[0], labels.shape[1], connectivity, mode)
        assert not labels.is_floating_point() and labels.dtype != torch.bool
        if labels.dtype == torch.int64:                                         # as _region_inputs: what does not fit int32 stays refused
            labels = labels.clamp(-1, max_label + 1)
        labels, within = self._image(labels.to(torch.int32)), self._image(within)
        assert within is None or within.shape == labels.shape
        H, W = labels.shape
        dev = labels.device
        R = max_label + 1
        i32, i64, u8 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev), dict(dtype=torch.uint8, device=dev)
        L = ctypes.c_int64
        lib, st = self.lib, self._stream()
        image = (_ptr(labels),) + tuple(_within_args(within)) + (H, W, max_label)
        meta = torch.empty(1, **i32)

        def empty_tables():
            return (torch.zeros(R + 1, **i64), torch.zeros(1, **i64), torch.empty(0, **i32), torch.empty(0, **i32), torch.empty(0, **i32),
                    torch.empty(0, **i64), torch.empty(0, 2, **i32))

        if H * W == 0:
            self._chk(lib.cgc_region_outline_count(*image, 1 if background else 0, None, None, _ptr(meta), st), 'cgc_region_outline_count')
            return empty_tables(), meta, 0
        sides = torch.empty(2, H * W, **u8)                                       # mask, count
        self._chk(lib.cgc_region_outline_count(*image, 1 if background else 0, _ptr(sides[0]), _ptr(sides[1]), _ptr(meta), st),
                  'cgc_region_outline_count')
        offsets = torch.cumsum(sides[1], 0, dtype=torch.int32)
        n, refused = torch.stack([offsets[-1], meta[0]]).tolist()                 # host read 1: the cracks, the refused pixels
        if refused:
            return None, meta, refused
        if n == 0:
            return empty_tables(), meta, 0
        lists = torch.empty(4, n, **i32)
        crack, succ, start, steps = lists[0], lists[1], lists[2], lists[3]
        self._chk(lib.cgc_region_outline_cracks(*image, connectivity, _ptr(sides[0]), _ptr(offsets), L(n), _ptr(crack), _ptr(succ), st),
                  'cgc_region_outline_cracks')
        ws = torch.empty(int(lib.cgc_region_outlines_ws_bytes(L(n))), **u8)
        assert ws.numel() >= 16 * n
        self._chk(lib.cgc_region_outline_loops(L(n), _ptr(succ), _ptr(ws), _ptr(start), _ptr(steps), st), 'cgc_region_outline_loops')
        del ws
        rank = torch.cumsum(start == torch.arange(n, **i32), 0, dtype=torch.int32)
        counts = [rank[-1]]
        if mode == 'corners':                                                     # a vertex is kept where the direction changes
            counts.append((((crack ^ crack[succ.to(torch.int64)]) & 3) != 0).sum().to(torch.int32))
        counts = torch.stack(counts).tolist()                                     # host read 2: the loops, the vertices
        n_loops, n_vertices = counts[0], counts[-1] if mode == 'corners' else n
        keys = torch.empty(n_loops, **i64)
        self._chk(lib.cgc_region_outline_keys(L(n), L(n_loops), _ptr(labels), _ptr(crack), _ptr(start), _ptr(rank), _ptr(keys), st),
                  'cgc_region_outline_keys')
        keys = torch.sort(keys).values
        loops = torch.empty(3, n_loops, **i32)
        loop_label, loop_start, loop_cracks = loops[0], loops[1], loops[2]
        area2 = torch.empty(n_loops, **i64)
        loop_of = rank                                                            # no longer read: the loop's number at its start crack
        self._chk(lib.cgc_region_outline_tables(L(n), L(n_loops), _ptr(keys), _ptr(crack), _ptr(steps), _ptr(loop_label), _ptr(loop_start),
                                                _ptr(loop_cracks), _ptr(area2), _ptr(loop_of), st), 'cgc_region_outline_tables')
        crack_ptr = torch.zeros(n_loops + 1, **i64)
        torch.cumsum(loop_cracks, 0, out=crack_ptr[1:])
        slots = torch.empty(n, 2, **i32)
        keep = torch.empty(n, **u8) if mode == 'corners' else None
        self._chk(lib.cgc_region_outline_scatter(L(n), L(n_loops), W, _ptr(crack), _ptr(succ), _ptr(start), _ptr(steps), _ptr(loop_of),
                                                 _ptr(crack_ptr), _ptr(area2), _ptr(slots), _ptr(keep), st), 'cgc_region_outline_scatter')
        if mode == 'cracks':
            loop_ptr, vertices = crack_ptr, slots
        else:
            place = torch.zeros(n + 1, **i32)
            torch.cumsum(keep, 0, dtype=torch.int32, out=place[1:])
            vertices = torch.empty(n_vertices, 2, **i32)
            self._chk(lib.cgc_region_outline_compact(L(n), L(n_vertices), _ptr(keep), _ptr(place[1:]), _ptr(slots), _ptr(vertices), st),
                      'cgc_region_outline_compact')
            loop_ptr = place[crack_ptr].to(torch.int64)
        label_ptr = torch.searchsorted(loop_label.to(torch.int64), torch.arange(R + 1, **i64))
        return (label_ptr, loop_ptr, loop_label, loop_start, loop_cracks, area2, vertices), meta, 0

    @staticmethod
    def _check_slic(shape, step, compactness, n_iter):
        """The refusals of slic_iterate that need shapes only."""
        for name, v, lo, hi in (('step', step, SLIC_MIN_STEP, SLIC_MAX_STEP), ('compactness', compactness, 0, SLIC_MAX_COMPACTNESS),
                                ('n_iter', n_iter, 1, SLIC_MAX_ITER)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError('slic_iterate: %s must be an integer in %d..%d, got %r' % (name, lo, hi, v))
        if len(shape) != 3 or not 1 <= shape[0] <= SLIC_MAX_PLANES:
            raise ValueError('slic_iterate: planes must be [C, H, W] with 1 <= C <= %d (got %s)' % (SLIC_MAX_PLANES, tuple(shape)))
        if shape[1] * shape[2] >= SLIC_MAX_PIXELS:
            raise ValueError('slic_iterate takes images of fewer than 2^29 pixels (got %d x %d)' % (shape[1], shape[2]))

    @staticmethod
    def slic_grid(H, W, step):
        """(ny, nx) of slic_iterate's grid."""
        return max(1, (2 * H + step) // (2 * step)), max(1, (2 * W + step) // (2 * step))

    def slic_iterate(self, planes, step, compactness, n_iter, within=None):
        HipKernels._check_slic(planes.shape, step, compactness, n_iter)
        if planes.dtype != torch.uint8:
            raise TypeError('slic_iterate: planes must be uint8, got %s' % planes.dtype)
        if within is not None and (tuple(within.shape) != tuple(planes.shape[1:]) or within.device != planes.device):
            raise ValueError('slic_iterate: within must have the shape and device of a plane (got %s on %s and %s on %s)'
                             % (tuple(within.shape), within.device, tuple(planes.shape[1:]), planes.device))
        self._dev(planes)
        within = self._image(within)
        planes = planes.contiguous()
        C, H, W = planes.shape
        i32 = dict(dtype=torch.int32, device=planes.device)
        if H * W == 0:
            return torch.empty(H, W, **i32), torch.empty(0, 2 + C, **i32), torch.empty(0, **i32)
        ny, nx = HipKernels.slic_grid(H, W, step)
        labels, centres, count = torch.empty(H, W, **i32), torch.empty(ny * nx, 2 + C, **i32), torch.empty(ny * nx, **i32)
        ws = torch.empty(int(self.lib.cgc_slic_ws_bytes(C, H, W, step)), dtype=torch.uint8, device=planes.device)
        assert ws.numel() >= 8 * ny * nx * (3 + C)
        self._chk(self.lib.cgc_slic_iterate(_ptr(planes), C, H, W, step, compactness, n_iter, *_within_args(within), _ptr(ws), _ptr(labels),
                                            _ptr(centres), _ptr(count), self._stream()), 'cgc_slic_iterate')
        return labels, centres, count

    def slic_merge(self, sizes, pairs, count, min_size):
        if isinstance(min_size, bool) or not isinstance(min_size, int) or not 0 <= min_size < 2 ** 31:
            raise ValueError('slic_merge: min_size must be an integer in 0..2^31 - 1, got %r' % (min_size,))
        self._dev(sizes, pairs, count)
        assert sizes.dtype == pairs.dtype == count.dtype == torch.int32 and sizes.dim() == 1
        assert pairs.dim() == 2 and pairs.shape[1] == 2 and tuple(count.shape) == (pairs.shape[0],)
        sizes, pairs, count = sizes.contiguous(), pairs.contiguous(), count.contiguous()
        P, Q = sizes.shape[0], pairs.shape[0]
        dev = sizes.device
        group = torch.empty(P + 1, dtype=torch.int32, device=dev)
        best = torch.empty(P + 1, dtype=torch.int64, device=dev)
        self._chk(self.lib.cgc_slic_merge_begin(_ptr(sizes), P, min_size, _ptr(group), _ptr(best), self._stream()), 'cgc_slic_merge_begin')
        if P == 0 or Q == 0:
            return group, 0
        changed = torch.empty(1, dtype=torch.int32, device=dev)

        def launch(first, rounds):
            self._chk(self.lib.cgc_slic_merge_rounds(_ptr(pairs), _ptr(count), ctypes.c_int64(Q), P, rounds, _ptr(group), _ptr(best),
                                                     _ptr(changed), self._stream()), 'cgc_slic_merge_rounds')

        return group, HipKernels._relax_until_still(launch, changed, SLIC_MERGE_FIRST_BATCH, SLIC_MERGE_MAX_BATCH)

    def slic_relabel(self, pieces, table):
        self._dev(pieces, table)
        assert pieces.dtype == table.dtype == torch.int32 and pieces.dim() == 2 and table.dim() == 1 and table.numel() >= 1
        pieces, table = pieces.contiguous(), table.contiguous()
        out = torch.empty_like(pieces)
        self._chk(self.lib.cgc_slic_relabel(_ptr(pieces), ctypes.c_int64(pieces.numel()), table.numel() - 1, _ptr(table), _ptr(out),
                                            self._stream()), 'cgc_slic_relabel')
        return out

    def region_quantiles(self, hist, q10k):
        q = HipKernels._check_q10k(q10k)
        self._dev(hist)
        assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.shape[1] == 256
        hist = hist.contiguous()
        out = torch.empty(hist.shape[0], len(q), dtype=torch.uint8, device=hist.device)
        self._chk(self.lib.cgc_region_quantiles(_ptr(hist), ctypes.c_int64(hist.shape[0]), q, len(q), _ptr(out), self._stream()),
                  'cgc_region_quantiles')
        return out

    def edge_renorm(self, rowptr, col, n, p, val_out):
        self._dev(rowptr, col, val_out)
        self._chk(self.lib.cgc_edge_renorm(_ptr(rowptr), _ptr(col), n, ctypes.c_float(p), _ptr(val_out),
                                           self._stream()), 'cgc_edge_renorm')

    def csr_transpose_vals(self, t_rowptr, t_perm, val, n, t_val_out):
        self._dev(t_rowptr, t_perm, val, t_val_out)
        self._chk(self.lib.cgc_csr_transpose_vals(_ptr(t_rowptr), _ptr(t_perm), _ptr(val), n, _ptr(t_val_out), self._stream()),
                  'cgc_csr_transpose_vals')

    def csr_invdeg(self, rowptr, val, n, out):
        self._dev(rowptr, val, out)
        self._chk(self.lib.cgc_csr_invdeg(_ptr(rowptr), _ptr(val), n, _ptr(out), self._stream()), 'cgc_csr_invdeg')

    def spmm(self, rowptr, col, perm, val, pre, post, x, out, n, width, gptr=None, num_graphs=0, nmax=0, visit=0, ld=None, gorder=None):
        self._dev(rowptr, col, perm, val, pre, post, x, out, gptr)
        assert (x.is_contiguous() and out.is_contiguous()) if ld is None else (gptr is not None and x.stride(1) == 1 and out.stride(1) == 1)
        if gptr is not None:
            self._chk(self.lib.cgc_spmm_graphs(_ptr(rowptr), _ptr(col), _ptr(perm), _ptr(val), _ptr(pre), _ptr(post),
                                               _ptr(x), _ptr(out), n, width, width if ld is None else ld, _ptr(gptr),
                                               num_graphs, nmax, int(visit), _ptr(gorder), self._stream()), 'cgc_spmm_graphs')
        else:
            self._chk(self.lib.cgc_spmm(_ptr(rowptr), _ptr(col), _ptr(perm), _ptr(val), _ptr(pre), _ptr(post),
                                        _ptr(x), _ptr(out), n, width, self._stream()), 'cgc_spmm')

    # -- dense contractions
    def _gemm_ws(self, device, stream):
        """The workspace of cgc_gemm_f32 (include/cgc_hip.h): the slabs of the tail split and, at its end, the scale slots of mode
        GEMM_SPLIT_F16; one per (device, stream): products queued on one stream run one after the other and may share it; two
        streams must not.  tail_split = False: no slabs -- mode GEMM_SPLIT_F16 still gets its scale slots (a workspace too small for
        a slab)."""
        if not self.tail_split and int(self.gemm_mode) != GEMM_SPLIT_F16:
            return _NO_WS
        key = (device.index, stream)
        ws = self._ws_cache.get(key)
        if ws is None:
            ws = self._ws_cache[key] = torch.empty(int(self.lib.cgc_gemm_ws_floats()), dtype=torch.float32, device=device)
        return ws if self.tail_split else ws[-int(self.lib.cgc_gemm_half_ws_floats()):]

    def gemm(self, A, B, C, M, N, K, transA, transB, lda, ldb, ldc, alpha=1.0, beta=0.0, bias=None,
             batch=1, strideA=0, strideB=0, strideC=0, gptr=None, ragged=0, max_ragged=0, ragged_total=0, extra=()):
        self._dev(A, B, C, bias, gptr)
        stream = self._stream()
        ws = self._gemm_ws(C.device, stream)
        nx = len(extra)
        segs = (None,) * 7                     # no extra K segments: NULL arrays
        if nx:
            self._dev(*[e[0] for e in extra], *[e[1] for e in extra])
            PA, IA, LA = ctypes.c_void_p * nx, ctypes.c_int * nx, ctypes.c_int64 * nx
            segs = (PA(*[e[0].data_ptr() for e in extra]), IA(*[e[2] for e in extra]), LA(*[e[5] for e in extra]),
                    PA(*[e[1].data_ptr() for e in extra]), IA(*[e[3] for e in extra]), LA(*[e[6] for e in extra]),
                    IA(*[e[4] for e in extra]))
        rc = self.lib.cgc_gemm_f32(int(transA), int(transB), M, N, K, ctypes.c_float(alpha), _ptr(A), lda,
                                   _ptr(B), ldb, ctypes.c_float(beta), _ptr(C), ldc, _ptr(bias), batch,
                                   ctypes.c_int64(strideA), ctypes.c_int64(strideB), ctypes.c_int64(strideC),
                                   _ptr(gptr), ragged, max_ragged, nx, *segs, ws.data_ptr(), ws.numel(), int(self.gemm_mode), stream)
        self._chk(rc, 'cgc_gemm_f32')

    def reduce_batch_sum(self, ws, out, parts, numel, beta=0.0):
        self._dev(ws, out)
        self._chk(self.lib.cgc_reduce_batch_sum(_ptr(ws), _ptr(out), parts, ctypes.c_int64(numel),
                                                ctypes.c_float(beta), self._stream()), 'cgc_reduce_batch_sum')

    def reduce_batched(self, ws, out, outer, parts, numel, beta=0.0):
        self._dev(ws, out)
        self._chk(self.lib.cgc_reduce_batched(_ptr(ws), _ptr(out), outer, parts, numel, ctypes.c_float(beta),
                                              self._stream()), 'cgc_reduce_batched')

    # -- conv epilogue
    def l2norm_act_stats(self, h, n, F, normalize, act, hn_out, rinv_out, stats_out):
        self._dev(h, hn_out, rinv_out, stats_out)
        ws = torch.empty(int(self.lib.cgc_stats_ws_floats(n, F)), dtype=torch.float32, device=h.device) if stats_out is not None else None
        self._chk(self.lib.cgc_l2norm_act_stats(_ptr(h), n, F, int(normalize), act, _ptr(hn_out), _ptr(rinv_out),
                                                _ptr(stats_out), _ptr(ws), self._stream()), 'cgc_l2norm_act_stats')

    def sage_wide_fwd(self, agg, lda, weight, bias, n, Kin, F, normalize, act, hn_out, rinv_out, stats, count, eps, momentum,
                      running_mean, running_var, num_batches_tracked, mean_out, istd_out):
        self._dev(agg, weight, bias, hn_out, rinv_out, running_mean, running_var, num_batches_tracked, mean_out, istd_out)
        ws = None
        if stats:
            ws = torch.empty(int(self.lib.cgc_stats_ws_floats(n, F)), dtype=torch.float32, device=agg.device)
        tail = (int(bool(stats)), _ptr(ws), ctypes.c_double(count), ctypes.c_float(eps), ctypes.c_float(momentum), _ptr(running_mean),
                _ptr(running_var), _ptr(num_batches_tracked), _ptr(mean_out), _ptr(istd_out), self._stream())
        if F <= 32 and hn_out.stride(0) == F:          # narrow output: one wave per 32 rows (csrc/sagenarrow.hip)
            rc = self.lib.cgc_sage_narrow_fwd(_ptr(agg), lda, _ptr(weight), _ptr(bias), n, Kin, F, int(normalize), act, _ptr(hn_out),
                                              _ptr(rinv_out), *tail)
        else:
            rc = self.lib.cgc_sage_wide_fwd(_ptr(agg), lda, _ptr(weight), _ptr(bias), n, Kin, F, int(normalize), act, _ptr(hn_out),
                                            hn_out.stride(0), _ptr(rinv_out), *tail)
        if rc == -1:
            return False
        self._chk(rc, 'cgc_sage_wide_fwd')
        return True

    def bn_finalize(self, stats, count, eps, momentum, running_mean, running_var, mean_out, istd_out):
        self._dev(stats, running_mean, running_var, mean_out, istd_out)
        F = mean_out.numel()
        self._chk(self.lib.cgc_bn_finalize(_ptr(stats), F, ctypes.c_double(count), ctypes.c_float(eps),
                                           ctypes.c_float(momentum), _ptr(running_mean), _ptr(running_var),
                                           _ptr(mean_out), _ptr(istd_out), self._stream()), 'cgc_bn_finalize')

    def bn_act_apply(self, hn, n, F, act, mean, istd, gamma, beta, y_out, ldy):
        self._dev(hn, mean, istd, gamma, beta, y_out)
        self._chk(self.lib.cgc_bn_act_apply(_ptr(hn), n, F, act, _ptr(mean), _ptr(istd), _ptr(gamma), _ptr(beta),
                                            _ptr(y_out), ldy, None, 0, self._stream()), 'cgc_bn_act_apply')

    def l2norm_act_bn(self, h, n, F, normalize, act, hn_out, rinv_out, count, eps, momentum, running_mean, running_var,
                      num_batches_tracked, mean_out, istd_out):
        self._dev(h, hn_out, rinv_out, running_mean, running_var, num_batches_tracked, mean_out, istd_out)
        ws = torch.empty(int(self.lib.cgc_stats_ws_floats(n, F)), dtype=torch.float32, device=h.device)
        assert num_batches_tracked is None or num_batches_tracked.dtype == torch.int64
        self._chk(self.lib.cgc_l2norm_act_bn(_ptr(h), n, F, int(normalize), act, _ptr(hn_out), _ptr(rinv_out), _ptr(ws),
                                             ctypes.c_double(count), ctypes.c_float(eps),
                                             ctypes.c_float(momentum), _ptr(running_mean), _ptr(running_var),
                                             _ptr(num_batches_tracked), _ptr(mean_out), _ptr(istd_out), self._stream()),
                  'cgc_l2norm_act_bn')

    def bn_bwd_reduce(self, dy, ldy, hn, n, F, act, mean, istd, sums_out):
        self._dev(dy, hn, mean, istd, sums_out)
        nblk = self.lib.cgc_stats_blocks(n, F)
        ws = torch.empty(max(nblk, 1) * 2 * F, dtype=torch.float32, device=hn.device)
        self._chk(self.lib.cgc_bn_bwd_reduce(_ptr(dy), ldy, _ptr(hn), n, F, act, _ptr(mean), _ptr(istd),
                                             _ptr(sums_out), _ptr(ws), self._stream()), 'cgc_bn_bwd_reduce')

    def _slots(self, n, F, dev):
        return torch.empty(max(self.lib.cgc_stats_blocks(n, F), 1) * 2 * F, dtype=torch.float32, device=dev)

    def bn_act_l2_bwd(self, dy, ldy, hn, rinv, n, F, act, normalize, mode, mean, istd, gamma, sums, count, dh_out,
                      dh_colsum_out=None):
        self._dev(dy, hn, rinv, mean, istd, gamma, sums, dh_out, dh_colsum_out)
        ws = self._slots(n, F, hn.device) if dh_colsum_out is not None else None
        self._chk(self.lib.cgc_bn_act_l2_bwd(_ptr(dy), ldy, _ptr(hn), _ptr(rinv), n, F, act, int(normalize), mode,
                                             _ptr(mean), _ptr(istd), _ptr(gamma), _ptr(sums),
                                             ctypes.c_double(count), _ptr(dh_out), _ptr(dh_colsum_out), _ptr(ws),
                                             self._stream()), 'cgc_bn_act_l2_bwd')

    def sage_narrow_bwd(self, dy, ldy, hn, rinv, n, F, act, normalize, mode, mean, istd, gamma, sums, count, agg, lda, fin, weight,
                        dagg_out, dwdb_out):
        if F > 32 or fin > 32:
            return False
        self._dev(dy, hn, rinv, mean, istd, gamma, sums, agg, weight, dagg_out, dwdb_out)
        ws = torch.empty(int(self.lib.cgc_sage_narrow_ws_floats(n, fin, F)), dtype=torch.float32, device=hn.device)
        self._chk(self.lib.cgc_sage_narrow_bwd(_ptr(dy), ldy, _ptr(hn), _ptr(rinv), n, F, act, int(normalize), mode, _ptr(mean),
                                               _ptr(istd), _ptr(gamma), _ptr(sums), ctypes.c_double(count), _ptr(agg), lda, fin,
                                               _ptr(weight), _ptr(dagg_out), fin, _ptr(dwdb_out), _ptr(ws), self._stream()),
                  'cgc_sage_narrow_bwd')
        return True

    def colsum(self, x, ld, n, F, out):
        self._dev(x, out)
        nblk = self.lib.cgc_stats_blocks(n, F)
        ws = torch.empty(max(nblk, 1) * 2 * F, dtype=torch.float32, device=x.device)
        self._chk(self.lib.cgc_colsum(_ptr(x), ld, n, F, _ptr(out), _ptr(ws), self._stream()), 'cgc_colsum')

    # -- softmax / readout
    def softmax_fwd(self, x, n, C, out, ld=None):
        self._dev(x, out)
        self._chk(self.lib.cgc_softmax_fwd(_ptr(x), n, C, C if ld is None else ld, _ptr(out), self._stream()), 'cgc_softmax_fwd')

    def softmax_bwd(self, S, dS, n, C, dx_out, dx_colsum_out=None, ld=None):
        self._dev(S, dS, dx_out, dx_colsum_out)
        ws = self._slots(n, C, S.device) if dx_colsum_out is not None else None
        self._chk(self.lib.cgc_softmax_bwd(_ptr(S), _ptr(dS), n, C, C if ld is None else ld, _ptr(dx_out), _ptr(dx_colsum_out), _ptr(ws),
                                           self._stream()), 'cgc_softmax_bwd')

    def segment_max_fwd(self, x, gptr, B, D, nmax, out, arg_out):
        self._dev(x, gptr, out, arg_out)
        self._chk(self.lib.cgc_segment_max_fwd(_ptr(x), _ptr(gptr), B, D, nmax, _ptr(out), _ptr(arg_out),
                                               self._stream()), 'cgc_segment_max_fwd')

    def segment_max_bwd(self, dout, arg, B, D, dx_zeroed):
        self._dev(dout, arg, dx_zeroed)
        self._chk(self.lib.cgc_segment_max_bwd(_ptr(dout), _ptr(arg), B, D, _ptr(dx_zeroed), self._stream()),
                  'cgc_segment_max_bwd')

    def segment_max_bwd_full(self, dout, arg, gptr, B, D, nmax, dx_out):
        self._dev(dout, arg, gptr, dx_out)
        self._chk(self.lib.cgc_segment_max_bwd_full(_ptr(dout), _ptr(arg), _ptr(gptr), B, D, nmax, _ptr(dx_out), self._stream()),
                  'cgc_segment_max_bwd_full')

    # -- jumping knowledge
    def jk_supported(self, C):
        return bool(self.lib.cgc_jk_supported(int(C)))

    @staticmethod
    def _ptr_array(tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def jk_fwd(self, xs, n, npad, C, lstm, w_att, b_att, out, HS, CS):
        self._dev(xs, w_att, b_att, out, HS, CS, *lstm)
        self._chk(self.lib.cgc_jk_lstm_fwd(_ptr(xs), n, npad, C, self._ptr_array(lstm), _ptr(w_att), _ptr(b_att), _ptr(out),
                                           _ptr(HS), _ptr(CS), self._stream()), 'cgc_jk_lstm_fwd')

    def jk_bwd(self, xs, dout, n, npad, C, lstm, w_att, b_att, HS, CS, dxs, DGT, INT, DHC):
        self._dev(xs, dout, w_att, b_att, HS, CS, dxs, DGT, INT, DHC, *lstm)
        self._chk(self.lib.cgc_jk_lstm_bwd(_ptr(xs), _ptr(dout), n, npad, C, self._ptr_array(lstm), _ptr(w_att), _ptr(b_att),
                                           _ptr(HS), _ptr(CS), _ptr(dxs), _ptr(DGT), _ptr(INT), _ptr(DHC), self._stream()),
                  'cgc_jk_lstm_bwd')

    def jk_bwd_params(self, xs, dout, n, npad, C, lstm, w_att, b_att, HS, CS, dxs, G_out):
        self._dev(xs, dout, w_att, b_att, HS, CS, dxs, G_out, *lstm)
        H = 3 * C // 2
        ng, ni, ktot = 4 * H + 1, C + 2 * H + 1, 3 * npad
        ws = torch.empty(int(self.lib.cgc_jk_bwd_ws_floats(C)), dtype=torch.float32, device=xs.device)
        rc = self.lib.cgc_jk_lstm_bwd_params(_ptr(xs), _ptr(dout), n, npad, C, self._ptr_array(lstm), _ptr(w_att), _ptr(b_att),
                                             _ptr(HS), _ptr(CS), _ptr(dxs), _ptr(G_out), _ptr(ws), self._stream())
        if rc == 0:
            return
        if rc != _EINVAL:
            self._chk(rc, 'cgc_jk_lstm_bwd_params')
        # unaligned buffers / other channel counts: staged path -- gate gradients and cell inputs transposed, one batched NT
        # GEMM per direction over K slices of 768 columns, combined deterministically
        kp = 768
        if npad < n or npad % 64 != 0:
            raise ValueError('jk_bwd_params: npad = %d must be a multiple of 64 and at least n = %d' % (npad, n))
        if ktot % kp != 0:          # (columns past the last whole slice would silently drop out of the gradients)
            raise ValueError('jk_bwd_params: the staged parameter gradients (C = %d, or unaligned buffers) take npad %% 256 == 0, '
                             'got %d' % (C, npad))
        dev = xs.device
        DGT = torch.empty(2, ng, ktot, dtype=torch.float32, device=dev)
        INT = torch.empty(2, ni, ktot, dtype=torch.float32, device=dev)
        DHC = torch.empty(2, 2, H, npad, dtype=torch.float32, device=dev)
        self.jk_bwd(xs, dout, n, npad, C, lstm, w_att, b_att, HS, CS, dxs, DGT, INT, DHC)
        parts = ktot // kp
        ws2 = torch.empty(parts, ng * ni, dtype=torch.float32, device=dev)
        for d in range(2):
            self.gemm(DGT[d], INT[d], ws2, ng, ni, kp, False, True, ktot, ktot, ni, 1.0, 0.0, None, parts, kp, kp, ng * ni)
            self.reduce_batch_sum(ws2, G_out[d], parts, ng * ni, 0.0)

    def jk_unpack_param_grads(self, G, C):
        self._dev(G)
        flat = torch.empty(int(self.lib.cgc_jk_param_grad_floats(int(C))), dtype=torch.float32, device=G.device)
        self._chk(self.lib.cgc_jk_unpack_param_grads(_ptr(G), int(C), _ptr(flat), self._stream()), 'cgc_jk_unpack_param_grads')
        return split_jk_param_grads(flat, C)

    # -- dense adjacency ops
    def dense_rownorm_fwd(self, A, R, C, out, invd_out, ge1_out):
        self._dev(A, out, invd_out, ge1_out)
        self._chk(self.lib.cgc_dense_rownorm_fwd(_ptr(A), R, C, _ptr(out), _ptr(invd_out), _ptr(ge1_out),
                                                 self._stream()), 'cgc_dense_rownorm_fwd')

    def dense_rownorm_bwd(self, dOut, Anorm, invd, ge1, R, C, dA_out):
        self._dev(dOut, Anorm, invd, ge1, dA_out)
        self._chk(self.lib.cgc_dense_rownorm_bwd(_ptr(dOut), _ptr(Anorm), _ptr(invd), _ptr(ge1), R, C, _ptr(dA_out),
                                                 self._stream()), 'cgc_dense_rownorm_bwd')

    def dense_renorm_fwd(self, A, R, C, p, out):
        self._dev(A, out)
        self._chk(self.lib.cgc_dense_renorm_fwd(_ptr(A), R, C, ctypes.c_float(p), _ptr(out), self._stream()),
                  'cgc_dense_renorm_fwd')

    def dense_renorm_bwd(self, A, dOut, R, C, p, dA_out):
        self._dev(A, dOut, dA_out)
        self._chk(self.lib.cgc_dense_renorm_bwd(_ptr(A), _ptr(dOut), R, C, ctypes.c_float(p), _ptr(dA_out),
                                                self._stream()), 'cgc_dense_renorm_bwd')

    def adj_prep_fwd(self, A, R, C, p, At_out, An_out, invd_out, ge1_out):
        self._dev(A, At_out, An_out, invd_out, ge1_out)
        self._chk(self.lib.cgc_adj_prep_fwd(_ptr(A), R, C, ctypes.c_float(-1.0 if p is None else p), _ptr(At_out), _ptr(An_out),
                                            _ptr(invd_out), _ptr(ge1_out), self._stream()), 'cgc_adj_prep_fwd')

    def adj_prep_bwd(self, A, An, invd, ge1, gAn, gAt, R, C, p, dA_out):
        self._dev(A, An, invd, ge1, gAn, gAt, dA_out)
        self._chk(self.lib.cgc_adj_prep_bwd(_ptr(A), _ptr(An), _ptr(invd), _ptr(ge1), _ptr(gAn), _ptr(gAt), R, C,
                                            ctypes.c_float(-1.0 if p is None else p), _ptr(dA_out), self._stream()), 'cgc_adj_prep_bwd')

    def diffpool_reg_fwd(self, S, n, C, lds, G, A_out, B, A, A_numel, rowptr, numel, rows, link_out, ent_out, keep_out):
        self._dev(S, G, A_out, A, rowptr, link_out, ent_out, keep_out)
        ws = torch.empty(int(self.lib.cgc_diffpool_reg_ws_floats()), dtype=torch.float32, device=S.device)
        self._chk(self.lib.cgc_diffpool_reg_fwd(_ptr(S), n, C, lds, _ptr(G), _ptr(A_out), B, _ptr(A), A_numel, _ptr(rowptr),
                                                float(numel), float(rows), _ptr(ws), _ptr(link_out), _ptr(ent_out), _ptr(keep_out),
                                                self._stream()), 'cgc_diffpool_reg_fwd')

    def diffpool_reg_bwd_prep(self, d_reg, keep, numel, rows, d_ao, dao_out, G, Gs_out, B, C, coef_out):
        self._dev(d_reg, keep, d_ao, dao_out, G, Gs_out, coef_out)
        self._chk(self.lib.cgc_diffpool_reg_bwd_prep(_ptr(d_reg), _ptr(keep), float(numel), float(rows), _ptr(d_ao), _ptr(dao_out),
                                                     _ptr(G), _ptr(Gs_out), B, C, _ptr(coef_out), self._stream()),
                  'cgc_diffpool_reg_bwd_prep')

    def diffpool_reg_entropy_bwd(self, S, n, C, lds, coef, ds, ldd):
        self._dev(S, coef, ds)
        self._chk(self.lib.cgc_diffpool_reg_entropy_bwd(_ptr(S), n, C, lds, _ptr(coef), _ptr(ds), ldd, self._stream()),
                  'cgc_diffpool_reg_entropy_bwd')

    def diffpool_reg_adj_bwd(self, A, m, coef, gA, accumulate):
        self._dev(A, coef, gA)
        self._chk(self.lib.cgc_diffpool_reg_adj_bwd(_ptr(A), m, _ptr(coef), _ptr(gA), int(accumulate), self._stream()),
                  'cgc_diffpool_reg_adj_bwd')
