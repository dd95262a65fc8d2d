/* libcgc_hip.so -- C ABI of the MI355X (gfx950) CGC-Net hot path.
 *
 * The reference (Amandaynzhou/CGC-Net) is pure Python: its hot path sits behind nn.Module.forward, not behind
 * an FFI.  Each entry point below replaces the dense torch / torch_geometric expression cited next to it
 * (paths relative to the reference checkout); cgc-net_amd/kernels.py binds them with ctypes and
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers; float = fp32, int = int32 unless stated; matrices row-major with an
 *     explicit leading dimension ("ld", in elements) where one is taken, contiguous otherwise
 *   - every call enqueues kernels on `stream` and returns immediately: no allocation, no synchronisation,
 *     no ownership taken (workspaces are passed in); safe for concurrent callers and for hipGraph capture.
 *     The library keeps NO state between calls, with two stated exceptions: (1) the measurement hook at the end of
 *     this header (cgc_timing_*): one process-wide observer pointer, NULL unless a benchmark attaches one -- while one is
 *     attached the GEMM / SpMM launches additionally record HIP events on their stream (do not attach during hipGraph
 *     capture); (2) per-device "dynamic LDS limit already raised" flags for the kernels that need more than 64 KB
 *     (idempotent hipFuncSetAttribute, set on first use per device)
 *   - return value: 0 on success, a hipError_t (>0) from the launch, or a negative CGC_E* argument error
 */
#ifndef CGC_HIP_H
#define CGC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cgc_stream_t; /* hipStream_t */

#define CGC_EINVAL (-1)      /* unsupported argument combination */

/* activation codes (model/network.py:84-91) */
#define CGC_ACT_IDENTITY 0
#define CGC_ACT_RELU 1
#define CGC_ACT_ELU 2
#define CGC_ACT_LEAKYRELU 3  /* slope 0.01 */

/* Bumped whenever an entry point is added, removed or changes its signature / semantics.  Bindings compare their own copy
 * (cgc-net_amd/_abi.py: ABI_VERSION) with cgc_abi_version() of the library they loaded and refuse a mismatch.
 *   1: rounds 1-3 (operators, step sequencer, head, optimiser, measurement hook)
 *   2: round 4 (head: labels outside [0, L) are ignored like F.cross_entropy's ignore_index; forward BatchNorm statistics in double:
 *      cgc_stats_ws_floats; additions listed in DESIGN.md)
 *   3: round 5 (cgc_gemm_f32_ws / cgc_gemm_f32_cat_ws take a `mode`; cgc_level_desc.flags bit 1; head: a label outside [0, L) other
 *      than -100 makes the loss NaN instead of being ignored)
 *   4: round 6 (removed: cgc_adj_prep_fwd2, cgc_adj_grad_operands, cgc_zero_diag and cgc_level_desc.flags bit 0 -- the thin-operand
 *      adjacency gradient; a descriptor with bit 0 set is refused.  Added: cgc_graph_build_local, cgc_graph_local_max_nodes)
 *   5: round 6 (mode CGC_GEMM_SPLIT_F16 of cgc_gemm_f32_ws / cgc_gemm_f32_cat_ws; cgc_level_desc.flags bit 2; cgc_gemm_half_count, cgc_gemm_half_ws_floats, cgc_gemm_half_min_work;
 *      cgc_gemm_ws_floats() grew by the mode's scale slots: workspaces sized by an older library are too small for the tail split)
 *   6: added cgc_sgd_step, cgc_rmsprop_step (one-launch SGD and RMSprop on the tables of cgc_adam_step)
 *   7: DiffPool regularisers: cgc_level_desc.flags bit 3, cgc_level_fwd_reg, cgc_level_bwd_reg, cgc_diffpool_reg_ws_floats,
 *      cgc_diffpool_reg_fwd, cgc_diffpool_reg_bwd_prep, cgc_diffpool_reg_entropy_bwd, cgc_diffpool_reg_adj_bwd
 *   8: one entry point per operation.  Removed: cgc_gemm_f32_ws, cgc_gemm_f32_cat, cgc_gemm_f32_cat_ws, cgc_spmm_graphs_ordered,
 *      cgc_bn_act_apply2, cgc_sage_narrow_bwd_ld, cgc_level_fwd_reg, cgc_level_bwd_reg.  The survivors take the signature of their
 *      widest former sibling: cgc_gemm_f32 (of cgc_gemm_f32_cat_ws), cgc_spmm_graphs (of cgc_spmm_graphs_ordered), cgc_bn_act_apply
 *      (of cgc_bn_act_apply2), cgc_sage_narrow_bwd (of cgc_sage_narrow_bwd_ld), cgc_level_fwd (of cgc_level_fwd_reg), cgc_level_bwd
 *      (of cgc_level_bwd_reg)
 *   9: nucleus features from instance masks: cgc_nuclei_lds_max_pixels, cgc_nuclei_ws_bytes, cgc_nuclei_label_pass,
 *      cgc_nuclei_big_ws_bytes, cgc_nuclei_features, cgc_bgr_to_gray
 *  10: connected-component labelling in front of them: cgc_label_ws_bytes, cgc_label_components, cgc_label_sizes
 *  11: exact distance transform with nearest sites: cgc_edt_ws_bytes, cgc_edt, CGC_EDT_INF
 *  12: geodesic distance transform with nearest seeds: cgc_geodesic_ws_bytes, cgc_geodesic_begin, cgc_geodesic_rounds,
 *      cgc_geodesic_finish, CGC_GEO_INF
 *  13: grayscale morphological reconstruction: cgc_reconstruct_ws_bytes, cgc_reconstruct_begin, cgc_reconstruct_rounds,
 *      cgc_reconstruct_finish
 *  14: seeded watershed flood: cgc_watershed_ws_bytes, cgc_watershed_begin, cgc_watershed_rounds, cgc_watershed_parents,
 *      cgc_watershed_jumps, cgc_watershed_finish
 *  15: from an H&E tile to a foreground map: cgc_stain_separate, cgc_histogram_chunk_pixels, cgc_histogram_u8, cgc_binomial_smooth_u8
 *  16: a tile's own stain vectors (Macenko): cgc_scan_chunk_pixels, cgc_od_moments, cgc_angle_bins, cgc_angle_histogram_ws_bytes,
 *      cgc_angle_histogram
 *  17: stain normalisation: cgc_concentration_bins, cgc_concentration_histogram, cgc_exp_lut_len, cgc_od_recolor_ws_bytes,
 *      cgc_od_recolor
 *  18: region adjacency of a label image: cgc_adjacency_tile_side, cgc_adjacency_ws_bytes, cgc_adjacency_count,
 *      cgc_adjacency_records, cgc_adjacency_merge_ws_bytes, cgc_adjacency_heads, cgc_adjacency_merge
 *  19: window sums and the local (mean / Niblack) threshold: cgc_window_max_radius, cgc_window_tile_rows, cgc_window_strip_cols,
 *      cgc_window_sums, cgc_local_threshold
 *  20: flat grey-scale morphology (erode, dilate, gradient over a square, disk or diamond; fused top-hat subtraction):
 *      cgc_morph_max_radius, cgc_morph_tile_rows, cgc_morph_tile_cols, cgc_morph_footprint_width, cgc_morph, CGC_MORPH_*
 *  21: DenseJK: cgc_jk_lstm_fwd, cgc_jk_lstm_bwd, cgc_jk_lstm_bwd_params and cgc_jk_lstm_bwd_flat refuse an npad that is not a
 *      multiple of 64 (CGC_EINVAL, nothing launched); they took any npad >= n before
 *  22: rank filters (quantile, quantile range, local entropy over a square, disk or diamond): cgc_rank_max_radius,
 *      cgc_rank_entropy_max_radius, cgc_rank_tile_rows, cgc_rank_tile_cols, cgc_rank_entropy_term, cgc_rank_filter, CGC_RANK_*
 *  23: region statistics (per label value: count, sum, sum of squares, extrema with positions; 256-bin histograms; quantiles off
 *      them): cgc_region_tile_side, cgc_region_table_slots, cgc_region_ws_bytes, cgc_region_moments, cgc_region_histogram,
 *      cgc_region_quantiles
 *  24: region co-occurrence (per label value and offset: the grey-level co-occurrence table of a uint8 plane over pairs of pixels of
 *      one region): cgc_region_cooc_max_offset, cgc_region_cooc_max_offsets, cgc_region_cooccurrence
 *  25: region geometry (per label value: count, coordinate sums, extents in eight directions, bit-quad counts, pixels on the image
 *      frame): cgc_region_geometry_max_side, cgc_region_geometry
 *  26: region hull (per label value: the exact convex hull of its pixel squares -- vertices, area, diameter with end points, minimum
 *      width, perimeter): cgc_region_hull_tall_rows, cgc_region_hull_ws_bytes, cgc_region_hull_spans, cgc_region_hull
 *  27: resampling (the pixel size of a uint8 plane or tile -- linear, area -- and of a label image -- nearest, majority):
 *      cgc_resample_max_side, cgc_resample_labels_max_factor, cgc_resample_u8, cgc_resample_labels
 *  28: region outlines (per label value: the ordered boundary of its pixel squares as closed loops of lattice corners, by pointer
 *      doubling over the cracks): cgc_region_outline_rounds, cgc_region_outlines_ws_bytes, cgc_region_outline_count,
 *      cgc_region_outline_cracks, cgc_region_outline_loops, cgc_region_outline_keys, cgc_region_outline_tables,
 *      cgc_region_outline_scatter, cgc_region_outline_compact
 *  29: superpixels (SLIC on integer planes: a gather assignment and an integer centre update per round; the order-free merge of
 *      small connected pieces; one relabel): cgc_slic_max_step, cgc_slic_tile_side, cgc_slic_table_side, cgc_slic_ws_bytes,
 *      cgc_slic_iterate, cgc_slic_merge_begin, cgc_slic_merge_rounds, cgc_slic_relabel */
#define CGC_ABI_VERSION 29
int cgc_abi_version(void);

/* ---- A1: graph structure.  Replaces to_dense_adj (model/utils.py:3-36, called at model/network.py:241).
 * edge_index: int64 [2,E] (row 0 = aggregating centre, row 1 = neighbour), any order, duplicates allowed.
 * Produces column-sorted, de-duplicated CSR (rowptr[n+1], col[cap], rowidx[cap]) and its transpose
 * (t_rowptr[n+1], t_col[cap] = source row, t_perm[cap] = slot in the forward arrays); cap = E + (add_diag? n : 0).
 * nnz = rowptr[n] stays on the device.  ws: int32 workspace of 3*(n+1) + 2*max(cap,1) elements.
 * Edges with an id outside [0, n) are DROPPED (never dereferenced) and counted: after the call
 * ws[cgc_csr_bad_edges_offset(E, n, add_diag)] holds their number (0 for a well-formed batch) -- the device-side
 * counterpart of the IndexError the reference's dense indexing raises (model/utils.py:28-33). */
int64_t cgc_csr_bad_edges_offset(int64_t E, int n, int add_diag);
int cgc_csr_build(const int64_t* edge_index, int64_t E, int n, int add_diag,
                  int* rowptr, int* col, int* rowidx, int* t_rowptr, int* t_col, int* t_perm,
                  int* ws, cgc_stream_t stream);

/* ---- F1 (loader front-end): device-side finish of Batch.from_data_list after ONE host-to-device copy of the packed
 * batch.  x [n,F] is z-scored in place, x = (x - mean[f]) / std[f] (dataflow/data.py:353; mean/std NULL: untouched);
 * batch[i] = graph of node i from gptr [B+1] (NULL: skipped); edge_index [2,E] holds per-graph LOCAL node ids, the edges of
 * graph g at [eptr[g], eptr[g+1]): both rows get + gptr[g] (torch_geometric Batch.from_data_list; NULL: skipped). */
int cgc_collate(float* x, int n, int F, const float* mean, const float* stdv, const int* gptr, int B, int64_t* batch,
                int64_t* edge_index, int64_t E, const int* eptr, cgc_stream_t stream);

/* ---- F3 (node samplers in front of graph construction): farthest-point sampling on the nucleus coordinates for a
 * batch of graphs.  Replaces FarthestSampler (common/utils.py:187-197: k argmax / minimum passes over rows of a
 * precomputed n x n int16 distance table) inside the 'farthest' / 'fuse' samplers (dataflow/data.py:195-225); distances
 * are formed from pos (fp64, ties -> lowest index as numpy.argmax), no table.  pos [n,2] f32; gptr [B+1]; start [B] = first
 * pick of each graph (local index; the reference draws it at random); optr [B+1] = offsets of each graph's picks in out
 * (k_g = optr[g+1]-optr[g] <= n_g); out int32 GLOBAL node ids in pick order.  max_nodes = largest graph (<= 16384). */
int cgc_farthest_point_sample(const float* pos, const int* gptr, int B, int max_nodes, const int* start, const int* optr,
                              int* out, cgc_stream_t stream);
/* Reference-compatible variant: the distance between two nuclei is the entry the reference's table holds,
 * int16(sqrt(dx*dx + dy*dy)) evaluated in float32 on the float32 coordinates (euc_dist,
 * dataflow/construct_feature_graph.py:17-24), recomputed on the fly -- the picks equal FarthestSampler's on the stored table
 * index for index (ties of the truncated distances -> lowest index).  Same arguments. */
int cgc_farthest_point_sample_table16(const float* pos, const int* gptr, int B, int max_nodes, const int* start,
                                      const int* optr, int* out, cgc_stream_t stream);

/* ---- F2 (the step before the path): cell-graph construction.  Replaces torch_cluster.radius_graph(pos, r, None, loop,
 * max_num_neighbors) = cKDTree.query(k+1, distance_upper_bound = r+1e-8) per graph on the host (dataflow/data.py:246,255,
 * 297,348; dataflow/prepare_cv_dataset.py:102) for a whole batch of graphs: pos [n,2] f32, gptr [B+1] first node of each
 * graph (a node only sees its own graph).  Per node the <= k (<= 32) nearest others within r (fp64 distances, ties by
 * index) plus itself iff loop.  Out: nbr [n, k+1] (global node ids, by distance), cnt [n], rowptr [n+1] (exclusive scan of
 * cnt; rowptr[n] = nnz).  ws: cgc_radius_knn_ws_ints(n, B) ints. */
int64_t cgc_radius_knn_ws_ints(int n, int B);
int cgc_radius_knn(const float* pos, const int* gptr, int B, int n, float r, int k, int loop, int* nbr, int* cnt, int* rowptr,
                   int* ws, cgc_stream_t stream);
/* ELL rows of cgc_radius_knn -> edge_index [2, nnz] int64 (row = centre, ascending; col = neighbour), the layout
 * Batch.from_data_list / cgc_csr_build consume (dataflow/data.py:347-353). */
int cgc_knn_emit_edges(const int* nbr, const int* rowptr, int n, int k, int64_t nnz, int64_t* edge_index, cgc_stream_t stream);

/* ---- F4 (the first front-end step): nucleus features and centroids from an instance mask (csrc/nuclei.hip).  Replaces
 * dataflow/construct_feature_graph.py:50-123 + common/nuc_feature.py (remove_small_objects, regionprops, the per-nucleus crop statistics,
 * rank entropy, GLCM, findContours / contourArea / convexHull / arcLength / fitEllipse); the arithmetic item by item:
 * cgc-net_amd/kernels.py KernelSpec.nucleus_features.  labels int32 [H, W] (0 = background), gray uint8 [H, W]; H * W < 2^31.
 * Two calls around ONE host read of meta:
 *   cgc_nuclei_label_pass: ws = cgc_nuclei_ws_bytes(max_label) bytes (tables indexed by label value: max_label >= the largest label);
 *     kept_labels int32 [max_label] receives the surviving labels (count >= min_size) in ascending order; meta int32 [4] (device) =
 *     {n rows, nbig crops above the LDS path, pixels of the largest such crop, refused pixels}.  A pixel whose label is negative or above
 *     max_label is counted in meta[3] and ignored (the reference raises ValueError for a negative label).
 *   cgc_nuclei_features: the same labels / ws / kept_labels, n, nbig and max_big_px = meta[0..2] read on the host; big_ws =
 *     cgc_nuclei_big_ws_bytes(nbig, max_big_px) bytes (NULL when nbig = 0).  Out: features f32 [n, 16] (the reference's column order),
 *     centroids f32 [n, 2] (mean row, mean column), info int32 [n, 4] or NULL: start row / column of the traced contour in the crop,
 *     its vertex count (negative: the trace overran its workspace -- never expected), path (0 LDS, 1 global workspace).
 * A crop of at most cgc_nuclei_lds_max_pixels() (2048) pixels is processed in LDS, a larger one on a slot of big_ws.
 * cgc_bgr_to_gray: cv2.cvtColor(BGR2GRAY) on 8-bit data, gray[i] = (1868 B + 9617 G + 4899 R + 8192) >> 14 for npix pixels of
 * bgr uint8 [npix, 3]; no workspace. */
int cgc_nuclei_lds_max_pixels(void);
int64_t cgc_nuclei_ws_bytes(int max_label);
int cgc_nuclei_label_pass(const int* labels, int H, int W, int max_label, int min_size, void* ws, int* kept_labels, int* meta,
                          cgc_stream_t stream);
int64_t cgc_nuclei_big_ws_bytes(int nbig, int64_t max_big_px);
int cgc_nuclei_features(const int* labels, const uint8_t* gray, int H, int W, int max_label, int min_size, const void* ws,
                        const int* kept_labels, int n, int nbig, int64_t max_big_px, void* big_ws, float* features, float* centroids,
                        int* info, cgc_stream_t stream);
int cgc_bgr_to_gray(const uint8_t* bgr, int64_t npix, uint8_t* gray, cgc_stream_t stream);

/* ---- F5 (in front of F4): connected-component labelling of a binary mask, relabelling of an integer mask (csrc/label.hip).  Replaces
 * scipy.ndimage.label on the host between a segmentation network's thresholded output and cgc_nuclei_label_pass; the contract item by
 * item: cgc-net_amd/kernels.py KernelSpec.label_components.  image [H, W] of pixel_bytes = 1, 2, 4 or 8 bytes per pixel (an integer
 * type of either signedness: only "is zero" and "equals" are used), 0 = background; H * W < 2^31.  connectivity 1 (4 neighbours) or
 * 2 (8 neighbours): two pixels share a component iff a path of neighbours that all carry the SAME value joins them.
 *   cgc_label_components: ws = cgc_label_ws_bytes(H, W, with_counts) bytes.  Out: labels int32 [H, W], 0 = background, components
 *     numbered 1..n by the raster order of their first pixels (for a 0/1 image: scipy.ndimage.label's output); *n_out (device) = n.
 *     with_counts != 0 keeps per-component pixel counts in ws: required for min_size > 1 (components of fewer pixels become
 *     background and take no number) and by cgc_label_sizes.  H * W = 0: only *n_out = 0 is written.
 *   cgc_label_sizes: after the host has read n, sizes int32 [n], sizes[k - 1] = pixels of component k; the same ws, untouched since a
 *     cgc_label_components call with with_counts != 0.
 * No workgroup waits for another one in any of the launches; the result is a pure function of the image. */
int64_t cgc_label_ws_bytes(int H, int W, int with_counts);
int cgc_label_components(const void* image, int pixel_bytes, int H, int W, int connectivity, int min_size, int with_counts, void* ws,
                         int* labels, int* n_out, cgc_stream_t stream);
int cgc_label_sizes(const void* ws, int H, int W, int n, int* sizes, cgc_stream_t stream);

/* ---- F6 (beside F5): exact Euclidean distance transform of a 2-D image with the nearest site of every pixel (csrc/edt.hip).  Replaces
 * scipy.ndimage.distance_transform_edt / skimage.segmentation.expand_labels on the host; the contract item by item:
 * cgc-net_amd/kernels.py KernelSpec.distance_transform.  image [H, W] of elem_bytes = 1, 2, 4 or 8 bytes per pixel (only "is zero" is
 * used); a site is a pixel with value != 0 (sites_nonzero != 0) or value == 0 (sites_nonzero = 0).  H <= 32767 and W <= 32767, so that
 * every squared distance fits int32; otherwise CGC_EINVAL and nothing is launched.  ws = cgc_edt_ws_bytes(H, W) bytes.
 *   dist2 int32 [H, W]: the smallest dy^2 + dx^2 from the pixel to a site INSIDE THE IMAGE (0 on sites).
 *   nearest int32 [H, W] or NULL (skipped): the raster index y' * W + x' of the site that attains it; of several the smallest index.
 *   No site in the image: dist2 = CGC_EDT_INF and nearest = -1 everywhere.  d2max >= 0: pixels whose true dist2 exceeds d2max report
 *   CGC_EDT_INF and -1, all others are exact; d2max < 0: no bound.  H * W = 0: nothing is written.
 * Three launches, no workgroup waits for another one, nothing allocates or synchronises; the result is a pure function of the image.
 * Cost per pixel grows with the distance to its nearest site (bounded by sqrt(d2max)): O(W) where a row's columns hold no site. */
#define CGC_EDT_INF 2147483647
int64_t cgc_edt_ws_bytes(int H, int W);
int cgc_edt(const void* image, int elem_bytes, int H, int W, int sites_nonzero, int d2max, void* ws, int* dist2, int* nearest_or_null,
            cgc_stream_t stream);

/* ---- F7 (beside F6): geodesic distance transform of a 2-D image with the nearest seed of every pixel (csrc/geodesic.hip): distance is
 * measured along paths that stay inside a domain, which F6 cannot do.  The contract item by item: cgc-net_amd/kernels.py
 * KernelSpec.geodesic_transform.  seeds, within_or_null [H, W] of 1, 2, 4 or 8 bytes per pixel (only "is zero" is used); the domain is
 * {within != 0} u {seeds != 0}, every pixel when within is NULL.  An axial step between two domain pixels costs a, a diagonal one b
 * (b = 0: no diagonal steps); 1 <= a <= b <= 2a or b = 0.  connectivity 2: a diagonal step needs its two end points in the domain;
 * connectivity 1: also one of the two pixels it passes between.  (b != 0 ? b : a) * H * W < 2^31, so that no path cost overflows int32;
 * otherwise CGC_EINVAL and nothing is launched.  ws = cgc_geodesic_ws_bytes(H, W) bytes (0: H * W is out of range).
 *   cgc_geodesic_begin: keys and domain into ws (one launch).
 *   cgc_geodesic_rounds: rounds number first_round .. first_round + rounds - 1 of the relaxation, one launch each (plus one 4-byte
 *     fill); the first call after begin passes first_round = 0, every later one the number of rounds already launched.  *changed
 *     (device) = the number of tiles whose keys moved in the LAST of these rounds: 0 means the keys are final (further rounds are
 *     harmless).  dmax >= 0: costs above dmax are never stored; dmax < 0: no bound.  a, b, connectivity as given to begin.
 *   cgc_geodesic_finish: dist int32 [H, W] = the smallest path cost from a seed (0 on seeds), nearest int32 [H, W] or NULL (skipped) =
 *     the raster index y' * W + x' of the seed that attains it, of several the smallest index.  A pixel outside the domain, one that no
 *     seed reaches, or one whose cost exceeds dmax: CGC_GEO_INF and -1.  H * W = 0: nothing is written.
 * No workgroup waits for another one in any launch, nothing allocates or synchronises: the caller reads *changed between batches of
 * rounds.  The result is exact and a pure function of the input.  Worst case: the number of rounds needed is 2 + the number of 64 x 64
 * tile edges that the longest shortest path crosses -- a serpentine corridor over a whole image needs hundreds. */
#define CGC_GEO_INF 2147483647
int64_t cgc_geodesic_ws_bytes(int H, int W);
int cgc_geodesic_begin(const void* seeds, int seed_bytes, const void* within_or_null, int within_bytes, int H, int W, int a, int b,
                       void* ws, cgc_stream_t stream);
int cgc_geodesic_rounds(int H, int W, int a, int b, int connectivity, int dmax, void* ws, int first_round, int rounds, int* changed,
                        cgc_stream_t stream);
int cgc_geodesic_finish(int H, int W, const void* ws, int* dist, int* nearest_or_null, cgc_stream_t stream);

/* ---- F8 (beside F7): grayscale morphological reconstruction of a 2-D int32 image (csrc/reconstruct.hip), the primitive under h-maxima
 * markers and hole filling.  The contract item by item: cgc-net_amd/kernels.py KernelSpec.morph_reconstruct.  marker, mask int32
 * [H, W], contiguous; connectivity 1 (4 neighbours) or 2 (8 neighbours); H * W < 2^31; otherwise CGC_EINVAL and nothing is launched.
 * By dilation (by_erosion = 0): R0 = min(marker, mask) pointwise -- a marker above the mask is clamped, not refused -- and R is the
 * fixed point of R[p] = min(mask[p], max(R[p], max over the neighbours q of R[q])): R[p] = the largest, over pixels q and
 * `connectivity`-paths from q to p, of min(R0[q], the smallest mask value on the path).  By erosion (by_erosion != 0): the dual,
 * ~dilation(~marker, ~mask) with bitwise NOT, which reverses the order of all of int32 and cannot overflow.
 * ws = cgc_reconstruct_ws_bytes(H, W) bytes (0: H * W is out of range).
 *   cgc_reconstruct_begin: the clamped marker and the mask into ws (one launch).
 *   cgc_reconstruct_rounds: rounds number first_round .. first_round + rounds - 1 of the relaxation, one launch each (plus one 4-byte
 *     fill); the first call after begin passes first_round = 0, every later one the number of rounds already launched.  *changed
 *     (device) = the number of tiles whose values moved in the LAST of these rounds: 0 means the values are final (further rounds are
 *     harmless).  connectivity as described above; by_erosion is begin's and finish's business only.
 *   cgc_reconstruct_finish: out int32 [H, W] = the reconstruction (one launch); by_erosion as given to begin.  H * W = 0: nothing is
 *     written.
 * No workgroup waits for another one in any launch, nothing allocates or synchronises: the caller reads *changed between batches of
 * rounds.  The result is exact and a pure function of the input.  Worst case: the number of rounds needed is 2 + the number of 64 x 64
 * tile edges that the longest path along which a value has to travel crosses -- a serpentine plateau over a whole image needs hundreds. */
int64_t cgc_reconstruct_ws_bytes(int H, int W);
int cgc_reconstruct_begin(const int* marker, const int* mask, int H, int W, int by_erosion, void* ws, cgc_stream_t stream);
int cgc_reconstruct_rounds(int H, int W, int connectivity, void* ws, int first_round, int rounds, int* changed, cgc_stream_t stream);
int cgc_reconstruct_finish(int H, int W, int by_erosion, const void* ws, int* out, cgc_stream_t stream);

/* ---- F9 (beside F8): seeded watershed flood of a 2-D int32 height image (csrc/watershed.hip): the level at which water rising from the
 * seeds first wets every pixel of a domain, and the seed that wets it.  The contract item by item: cgc-net_amd/kernels.py
 * KernelSpec.watershed_flood.  height int32 [H, W], contiguous, the whole int32 range; seeds, within_or_null, a, b, connectivity and
 * the size limit exactly as F7's; otherwise CGC_EINVAL and nothing is launched.  The flood key of a pixel is (alt, len), compared
 * lexicographically: (INT32_MIN, 0) on seeds; a step of cost w from a pixel with key (alt, len) onto the non-seed pixel p offers
 * (height[p], 0) if height[p] > alt, else (alt, len + w); a pixel keeps the smallest offer over all paths from any seed.
 * ws = cgc_watershed_ws_bytes(H, W) bytes (0: H * W is out of range).
 *   cgc_watershed_begin: keys, domain and a copy of the heights into ws (one launch).
 *   cgc_watershed_rounds: as cgc_geodesic_rounds (no dmax): *changed (device) = the number of tiles whose keys moved in the LAST of
 *     these rounds; 0 means the keys are final.
 *   cgc_watershed_parents: after the keys are final (one launch): the parent of a reached non-seed pixel p is the neighbour q that
 *     minimises (the offer of q to p, the key of q, the raster index of q) over the allowed steps q -> p from reached pixels; a seed is
 *     its own parent.  The key of a parent is strictly smaller, so the parents form a forest rooted at the seeds.
 *   cgc_watershed_jumps: `jumps` >= 1 pointer jumps parent[p] = parent[parent[p]], in place, one launch each (plus one 4-byte fill).
 *     *changed (device) = the number of pixels whose pointer moved in the LAST of these jumps: 0 means every pointer names its root
 *     (further jumps are harmless).  31 jumps always suffice.
 *   cgc_watershed_finish: level int32 [H, W] = alt on reached non-seed pixels, height elsewhere; source int32 [H, W] = the raster
 *     index of the root (a seed: its own index), -1 outside the domain and where no seed reaches.  H * W = 0: nothing is written.
 * No workgroup waits for another one in any launch, nothing allocates or synchronises: the caller reads *changed between batches.
 * The result is exact and a pure function of the input.  Worst case: as F7's for the rounds -- a serpentine valley over a whole image
 * needs hundreds -- and the logarithm of the longest parent chain for the jumps. */
int64_t cgc_watershed_ws_bytes(int H, int W);
int cgc_watershed_begin(const int* height, const void* seeds, int seed_bytes, const void* within_or_null, int within_bytes, int H, int W,
                        int a, int b, void* ws, cgc_stream_t stream);
int cgc_watershed_rounds(int H, int W, int a, int b, int connectivity, void* ws, int first_round, int rounds, int* changed,
                         cgc_stream_t stream);
int cgc_watershed_parents(int H, int W, int a, int b, int connectivity, void* ws, cgc_stream_t stream);
int cgc_watershed_jumps(int H, int W, void* ws, int jumps, int* changed, cgc_stream_t stream);
int cgc_watershed_finish(int H, int W, const void* ws, int* level, int* source, cgc_stream_t stream);

/* ---- F10 (in front of everything above): from a stained tile to the plane that is thresholded (csrc/stain.hip, csrc/smooth.hip).
 * Replaces skimage.color.separate_stains / rgb2hed, a Gaussian blur and skimage.filters.threshold_otsu's histogram on the host; the
 * contracts item by item: cgc-net_amd/kernels.py KernelSpec.stain_separate, histogram_u8, binomial_smooth.  All arithmetic is integer:
 * every result is exact and a pure function of the input.  No workspace; pixel counts obey H * W < 2^31 (npix < 2^31).
 *   cgc_stain_separate: colour deconvolution (Ruifrok and Johnston) in fixed point.  pix uint8 [npix, 3], interleaved; order 0: B, G, R
 *     (what cgc_bgr_to_gray reads), 1: R, G, B.  lut (HOST, 256 int32): optical density in 1/1024 of a natural-log unit,
 *     lut[v] = floor(1024 ln(255 / max(v, 1)) + 0.5), every entry in [0, 5674].  m (HOST, 9 int32, m[3 c + s], c = 0 R, 1 G, 2 B):
 *     rint(4096 inv(S)[c][s]) for the stain matrix S whose rows are the unit OD vectors of the stains.  Both travel as kernel
 *     arguments.  planes: bit s set = stain s is wanted (1..7); out uint8 [popcount(planes), npix], planar, ascending stain order:
 *       C_s = lut[R] m[0][s] + lut[G] m[1][s] + lut[B] m[2][s] (int32);  out_s = clamp((C_s + 2^15) >> 16, 0, 255), arithmetic shift:
 *     one level = 1 / 64 of a unit of natural-log concentration.  CGC_EINVAL, nothing launched: a NULL table, an order other than 0 / 1,
 *     planes outside 1..7, a table entry outside [0, 5674], or a matrix with sum_c |m[c][s]| * 5674 >= 2^31 - 2^15 for some s (the
 *     int32 sum could overflow: near-singular stains).  npix = 0: nothing is written.
 *   cgc_histogram_u8: hist int32 [256] (device) = the number of pixels i with img[i] = v and within[i] != 0; within_or_null [npix] of
 *     within_bytes = 1, 2, 4 or 8 bytes per pixel (only "is zero" is used), NULL: every pixel counts.  The entry zeroes hist itself
 *     (an asynchronous fill), then one launch: a workgroup counts cgc_histogram_chunk_pixels() (16384) consecutive pixels in LDS and
 *     adds its non-empty bins to hist with one atomic each.  npix = 0: hist is zeroed.
 *   cgc_binomial_smooth_u8: img, out uint8 [H, W], radius r in 0..5, weights w_k = C(2 r, k), k = 0..2 r:
 *       out[y, x] = (sum_i sum_j w_i w_j img[clamp(y + i - r, 0, H - 1), clamp(x + j - r, 0, W - 1)] + 2^(4 r - 1)) >> 4 r
 *     (border replicated; one rounding; exact in int32 since 255 * 2^20 < 2^31; r = 0 copies).  The standard deviation is sqrt(r / 2):
 *     1.58 at r = 5; larger blurs are repeated calls.  One launch; img and out must not overlap.  H * W = 0: nothing is written. */
int cgc_stain_separate(const uint8_t* pix, int64_t npix, int order, const int* lut, const int* m, int planes, uint8_t* out,
                       cgc_stream_t stream);
int cgc_histogram_chunk_pixels(void);
int cgc_histogram_u8(const uint8_t* img, int64_t npix, const void* within_or_null, int within_bytes, int* hist, cgc_stream_t stream);
int cgc_binomial_smooth_u8(const uint8_t* img, int H, int W, int radius, uint8_t* out, cgc_stream_t stream);

/* ---- F11 (beside F10): the two reductions behind an estimate of a tile's own stain vectors (Macenko et al. 2009; csrc/stain.hip;
 * cgc-net_amd/nuclei.py estimate_stains).  The contracts item by item: cgc-net_amd/kernels.py KernelSpec.od_moments, angle_histogram.
 * pix, npix, order and lut (HOST) are those of cgc_stain_separate, within_or_null and within_bytes those of cgc_histogram_u8.  With
 * o = (lut[R], lut[G], lut[B]) a pixel is SELECTED iff within is NULL or non-zero there and o_R, o_G, o_B >= od_min (0..5674).  All
 * arithmetic is integer; every result is exact and independent of the order of the adds.  A workgroup takes cgc_scan_chunk_pixels()
 * (16384) consecutive pixels and adds to the result once.  Each entry zeroes its result itself (an asynchronous fill); npix = 0 or an
 * empty selection leaves zeros.
 *   cgc_od_moments: out int64 [10] (device) = n, sum o_R, sum o_G, sum o_B, sum o_R^2, sum o_R o_G, sum o_R o_B, sum o_G^2, sum o_G o_B,
 *     sum o_B^2 over the selected pixels (5674^2 * 2^31 < 2^63).  One launch.
 *   cgc_angle_histogram: out int32 [K + 1] (device), K = cgc_angle_bins() = 1024.  basis (HOST, 6 int32, E[j][c] = basis[3 j + c],
 *     c = 0 R, 1 G, 2 B): |E[j][c]| <= 4096 and sum_c |E[j][c]| <= 7095 for j = 0, 1.  p_j = (sum_c o_c E[j][c] + 2^11) >> 12 (int32,
 *     arithmetic shift), so |p_j| <= 9829.  dirs (HOST, (K - 1) x 2 int32: c_k, s_k for k = 1 .. K - 1): 0 < c_k <= 16384,
 *     |s_k| <= 16384 and c_k s_{k+1} - s_k c_{k+1} > 0 -- directions in the open right half plane whose angles increase strictly.  A
 *     selected pixel with p_1 <= 0 adds one to out[K] (skipped); every other selected pixel adds one to out[b],
 *     b = #{k : c_k p_2 - s_k p_1 >= 0} (|c_k p_2 - s_k p_1| <= 2 * 16384 * 9829 < 2^31).  For a table that passes the check that set is
 *     a prefix of 1 .. K - 1 and the kernel finds b by binary search; any other table is refused.  ws: cgc_angle_histogram_ws_bytes()
 *     (4096) bytes on the device, 256-byte aligned: the entry puts the packed table there (two small launches whose kernel arguments
 *     carry it), then one launch.
 * CGC_EINVAL, nothing launched: npix outside [0, 2^31), an order other than 0 / 1, a NULL table, basis, dirs or out, a table entry
 * outside [0, 5674], od_min outside [0, 5674], within_bytes other than 1, 2, 4, 8 with a within, a basis or a direction outside the
 * bounds above, directions that do not turn left; with npix > 0 also a NULL pix or ws. */
int cgc_scan_chunk_pixels(void);
int cgc_od_moments(const uint8_t* pix, int64_t npix, int order, const int* lut, int od_min, const void* within_or_null, int within_bytes,
                   int64_t* out, cgc_stream_t stream);
int cgc_angle_bins(void);
int64_t cgc_angle_histogram_ws_bytes(void);
int cgc_angle_histogram(const uint8_t* pix, int64_t npix, int order, const int* lut, int od_min, const int* basis, const int* dirs,
                        const void* within_or_null, int within_bytes, void* ws, int* out, cgc_stream_t stream);

/* ---- F12 (beside F11): the two kernels behind stain normalisation (Macenko et al. 2009; csrc/stain.hip; cgc-net_amd/nuclei.py
 * normalize_stains).  The contracts item by item: cgc-net_amd/kernels.py KernelSpec.concentration_histogram, od_recolor.  All arithmetic
 * is int32 and exact; no transcendental function runs on the device.
 *   cgc_concentration_histogram: pix, npix, order, lut, od_min, within_or_null, within_bytes and the selection are those of
 *     cgc_od_moments; m (HOST, 9 int32, m[3 c + s]) is that of cgc_stain_separate, with its refusal for all three columns.  For a
 *     selected pixel and s = 0, 1: C_s = lut[R] m[0][s] + lut[G] m[1][s] + lut[B] m[2][s], b_s = clamp((C_s + 2^14) >> 15, 0, B - 1)
 *     (arithmetic shift), B = cgc_concentration_bins() = 512: one level = 1 / 128 of a natural-log unit, the last bin open.  out int32
 *     [2 B] (device): one is added to out[b_0] and to out[B + b_1].  The entry zeroes out itself (an asynchronous fill), then one
 *     launch: the third body of the scan of F11, a workgroup per cgc_scan_chunk_pixels() pixels.  No workspace.
 *   cgc_od_recolor: out uint8 [npix, 3] (device, interleaved in the order of pix; must not overlap pix).  a (HOST, 9 int32,
 *     a[3 c + d] = rint(4096 A[c][d]), c the input and d the output channel, 0 R, 1 G, 2 B): sum_c |a[c][d]| * 5674 < 2^31 - 2^11 for
 *     every d.  exp_lut (HOST, exp_len = cgc_exp_lut_len() = 6386 int32): exp_lut[k] = floor(255 exp(-k / 1024) + 0.5); the library
 *     accepts any table of that length with entries in [0, 255] that starts at 255, ends at 0 and never rises.  Per pixel
 *       O_d = sum_c lut[v_c] a[c][d] (int32);  k_d = clamp((O_d + 2^11) >> 12, 0, 6385);  out_d = exp_lut[k_d].
 *     ws: cgc_od_recolor_ws_bytes() (6400) bytes on the device, 256-byte aligned: the entry puts the table there as bytes (two
 *     small launches whose kernel arguments carry it -- the helper that carries cgc_angle_histogram's directions), then one launch.
 * CGC_EINVAL, nothing launched.  cgc_concentration_histogram: what cgc_od_moments refuses (a NULL out included, also at npix = 0,
 * since the entry zeroes it), a NULL m, a matrix beyond its bound; with npix > 0 also a NULL pix.  cgc_od_recolor: what
 * cgc_stain_separate refuses for pix, npix, order and lut, a NULL a or exp_lut, a matrix beyond its bound, exp_len other than 6386, a
 * table of another kind; with npix > 0 also a NULL pix, ws or out -- at npix = 0 the tables are still checked, then the entry
 * returns 0 and touches neither ws nor out, which may be NULL.  out of cgc_od_recolor may start at any byte: three dwords per lane
 * where its base is a multiple of 4, bytes otherwise. */
int cgc_concentration_bins(void);
int cgc_concentration_histogram(const uint8_t* pix, int64_t npix, int order, const int* lut, int od_min, const int* m,
                                const void* within_or_null, int within_bytes, int* out, cgc_stream_t stream);
int cgc_exp_lut_len(void);
int64_t cgc_od_recolor_ws_bytes(void);
int cgc_od_recolor(const uint8_t* pix, int64_t npix, int order, const int* lut, const int* a, const int* exp_lut, int exp_len, void* ws,
                   uint8_t* out, cgc_stream_t stream);

/* ---- F13 (behind F5/F6, in front of A1): region adjacency of a label image (csrc/adjacency.hip): which regions touch, along how many
 * pixel pairs, and the smallest value[p] + value[q] over each pair's contacts -- on the cells of expand_labels, the edges of the Voronoi
 * cell graph (cgc-net_amd/nuclei.py voronoi_graph).  The contract item by item: cgc-net_amd/kernels.py KernelSpec.region_adjacency.
 * labels, value_or_null int32 [H, W], contiguous, 0 = background, every other value (negative ones too) a region; H * W < 2^29, so that a
 * pair's count (at most 4 H W) fits int32 -- otherwise CGC_EINVAL and nothing is launched.  connectivity 1 (right and lower neighbour)
 * or 2 (also the two lower diagonals): every unordered pair of neighbouring pixels is looked at once.  A record is (key, count, sum): key
 * = ((int64)a << 32) | ((uint32)b ^ 0x80000000) for a < b as signed integers, whose int64 order is the lexicographic order of (a, b).
 *   cgc_adjacency_tile_side: the side (64) of the tiles one workgroup folds in LDS.
 *   cgc_adjacency_count: ws = cgc_adjacency_ws_bytes(H, W) bytes.  Counts the records every tile will write -- its distinct pairs, or,
 *     for a tile with more than 512 of them, its contacts -- and scans the counts; *n_records_out (device) = their total.  H * W = 0:
 *     only *n_records_out = 0 is written.
 *   cgc_adjacency_records: after the host has read n_records; the same labels, connectivity and ws.  Out: keys int64 [n_records],
 *     counts int32 [n_records], sums int32 [n_records] (iff value is given: the smallest value[p] + value[q], summed in 64 bits and
 *     clamped to int32), grouped by tile, in any order inside a tile.
 *   cgc_adjacency_heads: sorted_keys = the keys in ascending order; ws = cgc_adjacency_merge_ws_bytes(n_records) bytes;
 *     *n_pairs_out (device) = the number of distinct keys.
 *   cgc_adjacency_merge: after the host has read n_pairs; perm int64 [n_records] = the permutation that sorted the keys (sorted_keys[i] =
 *     keys[perm[i]]), counts / sums as cgc_adjacency_records wrote them, ws untouched since cgc_adjacency_heads.  Out: pairs int32
 *     [n_pairs, 2] ascending, count int32 [n_pairs] = sum of the records' counts, min_sum int32 [n_pairs] = minimum of their sums (iff
 *     sums are given).
 * The library allocates nothing and reads nothing on the host; no workgroup waits for another one; integer sums and minima make the
 * outputs independent of the order in which tables and records are filled. */
int cgc_adjacency_tile_side(void);
int64_t cgc_adjacency_ws_bytes(int H, int W);
int cgc_adjacency_count(const int* labels, int H, int W, int connectivity, void* ws, int* n_records_out, cgc_stream_t stream);
int cgc_adjacency_records(const int* labels, const int* value_or_null, int H, int W, int connectivity, void* ws, int64_t n_records,
                          int64_t* keys, int* counts, int* sums_or_null, cgc_stream_t stream);
int64_t cgc_adjacency_merge_ws_bytes(int64_t n_records);
int cgc_adjacency_heads(const int64_t* sorted_keys, int64_t n_records, void* ws, int* n_pairs_out, cgc_stream_t stream);
int cgc_adjacency_merge(const int64_t* sorted_keys, const int64_t* perm, const int* counts, const int* sums_or_null, int64_t n_records,
                        const void* ws, int n_pairs, int* pairs, int* count, int* min_sum_or_null, cgc_stream_t stream);

/* ---- F14 (behind F10's plane, in front of F5): window sums of a uint8 image and the local threshold on them (csrc/window.hip).  The
 * contract item by item: cgc-net_amd/kernels.py KernelSpec.window_sums / local_threshold.  img uint8 [H, W], contiguous, H * W < 2^31;
 * radius r in 0..127: the window of (y, x) is rows y - r .. y + r and columns x - r .. x + r, clipped to the image.  within_or_null [H, W]
 * of within_bytes (1, 2, 4 or 8) bytes per element, of which only "is zero" is read: only pixels with within != 0 count.
 *   cgc_window_sums: n int32, s int32, q int64, each [H, W]: the number, the sum and the sum of squares of the counted pixels.
 *   cgc_local_threshold: out uint8 [H, W] of 0 / 1.  With v the pixel's own value (read whatever `within` says), L = 64 (n v - s -
 *     offset n) and D = n q - s^2: out = 1 iff n >= 1 and v > floor and
 *       k64 >= 0: L > 0 and L^2 > k64^2 D;      k64 < 0: L > 0, or (L = 0 and D > 0), or (L < 0 and L^2 < k64^2 D)
 *     -- v > m + (k64 / 64) sd + offset with m = s / n, sd^2 = q / n - m^2, in int64; equality is not foreground.  k64 in -128..128,
 *     offset in -255..255, floor in -1..255 (-1: no floor).  n, s and q are never written to memory: one byte read, one written.
 *   cgc_window_max_radius (127), cgc_window_tile_rows (16), cgc_window_strip_cols(radius) (1024 - 2 * (radius rounded up to a multiple
 *     of 4); 0 for a radius out of range): the tile one workgroup owns, for tests that place windows across tile edges.
 * One launch per call, no workspace, no atomics: outputs are bit-identical from call to call.  Bad dims, a radius, k64, offset or floor
 * out of range, within_bytes other than 1, 2, 4, 8 (with a within), or a null pointer with H * W > 0: CGC_EINVAL, nothing launched.
 * H * W = 0: nothing to do, 0. */
int cgc_window_max_radius(void);
int cgc_window_tile_rows(void);
int cgc_window_strip_cols(int radius);
int cgc_window_sums(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int radius, int* n, int* s, int64_t* q,
                    cgc_stream_t stream);
int cgc_local_threshold(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int radius, int k64, int offset,
                        int floor, uint8_t* out, cgc_stream_t stream);

/* ---- F15 (on F10's plane, beside F14): flat grey-scale morphology of a uint8 image (csrc/morph.hip).  The contract item by item:
 * cgc-net_amd/kernels.py KernelSpec.flat_morphology.  img uint8 [H, W], contiguous, H * W < 2^31.  The footprint (kind, radius r in
 * 0..63) is the set of offsets (dy, dx) with |dy| <= r and |dx| <= w(dy): w = r (square), the largest integer with w^2 + dy^2 <= r^2
 * (disk, skimage's disk(r)), r - |dy| (diamond); r = 0 is the single pixel.  It is CLIPPED to the image: nothing is replicated.
 * within_or_null [H, W] of within_bytes (1, 2, 4 or 8) bytes per element, of which only "is zero" is read: a footprint pixel is counted
 * iff it lies in the image and within is non-zero there (or null).  The centre has no special role.
 *   op ERODE: the minimum over the counted pixels, 255 where none is counted.  DILATE: the maximum, 0 where none is.  GRADIENT: maximum
 *     minus minimum in one pass, 0 where none is counted.
 *   epilogue PLAIN: out = result.  OTHER_MINUS: out = max(0, other - result).  MINUS_OTHER: out = max(0, result - other); other uint8
 *     [H, W], read at the output pixel only (it may be the image of an earlier call; out must not overlap img).
 *   cgc_morph_max_radius (63), cgc_morph_tile_rows (32), cgc_morph_tile_cols(radius) (256 - 2 * (radius rounded up to a multiple of 4);
 *     0 for a radius out of range): the tile one workgroup owns, for tests that place footprints across tile edges.
 *   cgc_morph_footprint_width(kind, radius, dy): w(dy) as the kernel uses it (host only); CGC_EINVAL for a bad kind, radius or |dy| > r.
 * One launch per call, no workspace, no atomics: outputs are bit-identical from call to call.  Bad dims, a kind, radius, op or epilogue
 * out of range, within_bytes other than 1, 2, 4, 8 (with a within), or a null img / out (or other, with an epilogue) with H * W > 0:
 * CGC_EINVAL, nothing launched.  H * W = 0: nothing to do, 0. */
#define CGC_MORPH_SQUARE 0
#define CGC_MORPH_DISK 1
#define CGC_MORPH_DIAMOND 2
#define CGC_MORPH_ERODE 0
#define CGC_MORPH_DILATE 1
#define CGC_MORPH_GRADIENT 2
#define CGC_MORPH_PLAIN 0
#define CGC_MORPH_OTHER_MINUS 1
#define CGC_MORPH_MINUS_OTHER 2
int cgc_morph_max_radius(void);
int cgc_morph_tile_rows(void);
int cgc_morph_tile_cols(int radius);
int cgc_morph_footprint_width(int kind, int radius, int dy);
int cgc_morph(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int kind, int radius, int op,
              const uint8_t* other_or_null, int epilogue, uint8_t* out, cgc_stream_t stream);

/* ---- F16 (on F10's plane, beside F15): rank filters of a uint8 image (csrc/rank.hip) -- order statistics and the entropy of the
 * histogram of the counted pixels under a flat footprint.  The contract item by item: cgc-net_amd/kernels.py KernelSpec.rank_filter.
 * img, kind, radius, the widths w(dy), the clipping to the image, within_or_null / within_bytes and "counted" are exactly F15's (kinds
 * are CGC_MORPH_SQUARE / _DISK / _DIAMOND; radius 0..63).  With n the number of counted pixels of a window and v[0] <= ... <= v[n-1]
 * their values sorted, and k(q) = min(n - 1, floor(n * q / 10000)) for an integer q in 0..10000:
 *   op QUANTILE: out uint8 = v[k(q_hi)] (q_lo is not used, but must still be a valid q <= q_hi); 0 where n = 0.
 *   op RANGE:    out uint8 = v[k(q_hi)] - v[k(q_lo)], q_lo <= q_hi, both from one histogram; 0 where n = 0.
 *   op ENTROPY:  radius 0..15 only (n <= 961).  out int32 = floor(E / n), E = T[n] - sum over the non-empty bins of T[count], with
 *                T[c] = round(c * log2(c) * 2^16): the Shannon entropy of the counted values in bits, times 2^16, within 2 of the
 *                real value; 0 where n = 0.  q_lo, q_hi are checked as for the other ops and not used.
 *   cgc_rank_max_radius (63), cgc_rank_entropy_max_radius (15), cgc_rank_tile_rows (8), cgc_rank_tile_cols(radius) (256 - 2 * (radius
 *     rounded up to a multiple of 4); 0 for a radius out of range): the tile one workgroup owns, for tests.
 *   cgc_rank_entropy_term(c): T[c] for c in 0..961 (host only; the one table the kernel reads); CGC_EINVAL outside.
 * One launch per call, no workspace, no global atomics, integers only: outputs are bit-identical from call to call.  Bad dims, a kind,
 * radius or op out of range (radius > 15 with ENTROPY), q_lo or q_hi outside 0..10000, q_lo > q_hi, within_bytes other than 1, 2, 4,
 * 8 (with a within), or a null img / out with H * W > 0: CGC_EINVAL, nothing launched.  H * W = 0: nothing to do, 0. */
#define CGC_RANK_QUANTILE 0
#define CGC_RANK_RANGE 1
#define CGC_RANK_ENTROPY 2
int cgc_rank_max_radius(void);
int cgc_rank_entropy_max_radius(void);
int cgc_rank_tile_rows(void);
int cgc_rank_tile_cols(int radius);
int cgc_rank_entropy_term(int c);
int cgc_rank_filter(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int kind, int radius, int op,
                    int q_lo, int q_hi, void* out, cgc_stream_t stream);

/* ---- F17 (behind F5/F6 and every plane of F10..F16, beside F13): statistics of a second plane over the regions of a label image
 * (csrc/region.hip).  The contract item by item: cgc-net_amd/kernels.py KernelSpec.region_statistics / region_histogram /
 * region_quantiles.  labels int32 [H, W], contiguous, H * W < 2^31; tables are indexed by label value 0 .. max_label (0 <= max_label <
 * 2^31 - 1), row 0 -- the background -- being a region like any other.  within_or_null [H, W] of within_bytes (1, 2, 4 or 8) bytes per
 * element, of which only "is zero" is read.  A pixel p is counted in row L iff labels[p] == L and within is null or non-zero at p.  A
 * pixel whose label lies outside [0, max_label] is counted nowhere; *meta (int32 on the device) = the number of such pixels, whatever
 * within says there.
 *   cgc_region_moments: values [H, W] of value_bytes / value_signed = 1 / 0 (uint8), 1 / 1 (int8), 2 / 1 (int16) or 4 / 1 (int32).
 *     ws = cgc_region_ws_bytes(max_label) bytes.  Out, each [max_label + 1]: count int32; sum int64; sumsq int64 (may be null; must be
 *     null for 4-byte values); min, max int32; argmin, argmax int32 = the raster index y W + x of the extremum, of equal values the
 *     smallest index.  An empty row has count = sum = sumsq = min = max = 0 and argmin = argmax = -1.
 *   cgc_region_histogram: values uint8.  hist int32 [max_label + 1, 256], indexed in 64 bits: hist[L][v] = the counted pixels of row L
 *     with value v.
 *   cgc_region_quantiles: hist int32 [rows, 256], 16-byte aligned, every row's total n < 2^31; q10k: nq (1..8) integers in 0..10000 in
 *     HOST memory.  out uint8 [rows, nq] = v[min(n - 1, floor(n * q10k / 10000))] of the row's values sorted (F16's rule, the product
 *     in 64 bits), 0 where n = 0.  One wave per row.
 *   cgc_region_tile_side (64), cgc_region_table_slots (64): the tile one workgroup owns and the labels it folds in LDS, for tests; a
 *     tile with more labels than that sends the rest to the global tables directly -- exact for every input.
 * Integer adds and integer minima / maxima of (value, index) keys only: outputs are bit-identical from call to call.  No loop waits
 * for another thread.  Bad dims, max_label, value_bytes / value_signed, within_bytes (with a within), nq or q10k out of range, sumsq
 * with 4-byte values, or a null pointer where one is needed: CGC_EINVAL, nothing launched.  H * W = 0: the tables of empty rows. */
int cgc_region_tile_side(void);
int cgc_region_table_slots(void);
int64_t cgc_region_ws_bytes(int max_label);
int cgc_region_moments(const int* labels, const void* values, int value_bytes, int value_signed, const void* within_or_null,
                       int within_bytes, int H, int W, int max_label, void* ws, int* count, int64_t* sum, int64_t* sumsq_or_null, int* min,
                       int* max, int* argmin, int* argmax, int* meta, cgc_stream_t stream);
int cgc_region_histogram(const int* labels, const uint8_t* values, const void* within_or_null, int within_bytes, int H, int W,
                         int max_label, int* hist, int* meta, cgc_stream_t stream);
int cgc_region_quantiles(const int* hist, int64_t rows, const int* q10k, int nq, uint8_t* out, cgc_stream_t stream);

/* ---- F18 (beside F17, csrc/region.hip): grey-level co-occurrence tables of a uint8 plane over the regions of a label image.  The
 * contract item by item: cgc-net_amd/kernels.py KernelSpec.region_cooccurrence.  labels, max_label, within_or_null, the refused pixels
 * and *meta as F17 (*meta counts a refused pixel once per call, not once per offset); H * W < 2^30, so that a symmetric diagonal bin
 * of at most 2 H W fits int32.  values uint8 [H, W]; the level of a pixel is lut256_host[v], 256 bytes in HOST memory, every entry <
 * levels, levels in 2..16; the table travels by value, the buffer may be freed when the call returns.  offsets_host: noff (1 ..
 * cgc_region_cooc_max_offsets() = 8) pairs (dy, dx) in HOST memory, |dy|, |dx| <= cgc_region_cooc_max_offset() = 16, not (0, 0).
 * For offset k, anchor p = (y, x) and partner q = (y + dy, x + dx) the pair is counted in row R iff p and q lie inside the image,
 * labels[p] == labels[q] == R, 0 <= R <= max_label, and within is null or non-zero at both.  tables int32 [max_label + 1, noff,
 * levels * levels], indexed in 64 bits: a counted pair with levels (a, b) adds 1 to bin a * levels + b and, with symmetric != 0, 1 to
 * bin b * levels + a (2 on the diagonal: skimage's symmetric=True).  One launch per offset; pairs of a label that finds no slot in
 * the tile's LDS table add to `tables` directly: exact for every input, integer adds only, bit-identical from call to call.
 * Bad dims, max_label, within_bytes, levels, a lut entry >= levels, noff, an offset out of range or (0, 0), H * W >= 2^30 or a null
 * pointer where one is needed: CGC_EINVAL, nothing launched.  H * W = 0: zeros. */
int cgc_region_cooc_max_offset(void);
int cgc_region_cooc_max_offsets(void);
int cgc_region_cooccurrence(const int* labels, const uint8_t* values, const void* within_or_null, int within_bytes, int H, int W,
                            int max_label, const uint8_t* lut256_host, int levels, const int* offsets_host, int noff, int symmetric,
                            int* tables, int* meta, cgc_stream_t stream);

/* ---- F19 (beside F17, csrc/region.hip): the shape of every region of a label image, from the labels alone.  The contract item by
 * item: cgc-net_amd/kernels.py KernelSpec.region_geometry.  labels, max_label, within_or_null, "a pixel belongs to row L", the refused
 * pixels and *meta as F17.  H, W <= cgc_region_geometry_max_side() = 32767 (sum x^2 over 2^31 pixels fits int64) and (H + 1)(W + 1) <
 * 2^31 (a quad count fits int32).  Per label value 0 .. max_label, R = max_label + 1 rows:
 *   count   int32 [R]         the row's pixels
 *   sums    int64 [5, R]      sy, sx, syy, sxy, sxx over the row's pixels, y = row and x = column of the image
 *   extents int32 [R, 8, 2]   minimum and maximum of a x + b y over the row's pixel centres, (a, b) = (1,0) (2,1) (1,1) (1,2) (0,1)
 *                             (-1,2) (-1,1) (-2,1); (1,0) and (0,1) are the bounding box
 *   quads   int32 [R, 4]      n1, n2, nd, n3: over the 2 x 2 windows with top-left corner (y, x), y in -1 .. H-1, x in -1 .. W-1
 *                             (positions outside the image belong to no row), the windows in which the row has one pixel, two that
 *                             share an edge, the two of a diagonal, three; a window adds to every row that occurs in it
 *   border  int32 [R]         the row's pixels with y in {0, H-1} or x in {0, W-1}
 * An empty row has zeros everywhere, extents (0, 0).  H * W = 0: empty rows only.  What finds no slot in a tile's LDS table goes to
 * the tables directly: exact for every input; integer adds, minima and maxima only, bit-identical from call to call.
 * Bad dims, max_label, within_bytes, a side above 32767, (H + 1)(W + 1) >= 2^31 or a null pointer where one is needed: CGC_EINVAL,
 * nothing launched. */
int cgc_region_geometry_max_side(void);
int cgc_region_geometry(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label, int* count,
                        int64_t* sums, int* extents, int* quads, int* border, int* meta, cgc_stream_t stream);

/* ---- F20 (behind F19, csrc/region.hip): the exact convex hull of every region of a label image.  The per-label form of the
 * hull behind the reference's solidity (cv2.convexHull of one contour, dataflow/construct_feature_graph.py:84-88).  The contract item by item:
 * cgc-net_amd/kernels.py KernelSpec.region_hull.  labels, max_label, within_or_null and "a pixel is counted in row L" as F17, sides
 * as F19.  THE HULL of row L is the convex hull of the pixel SQUARES [x, x + 1] x [y, y + 1] of its counted pixels; vertices are
 * lattice corners (y, x), strictly convex, listed from the left end of the top lattice line down the left side, along the bottom and
 * up the right side, without repeats.  A hull call is three steps on one stream:
 *   cgc_region_geometry first.  extents = its table; ptr int64 [R + 1] = the caller's prefix sum of the bounding boxes' heights (ptr[0] =
 *     0, ptr[L + 1] - ptr[L] = extents[L][4][1] - extents[L][4][0] + 1, or 0 where count[L] = 0); span_rows = ptr[R], which the caller
 *     reads together with F19's *meta.
 *   cgc_region_hull_spans: spans int32 [span_rows, 2]; spans[ptr[L] + y - y0] = (smallest, largest column of the counted pixels of row
 *     L in image row y), (INT32_MAX, INT32_MIN) where it has none.  One workgroup per tile as F17; integer minima and maxima only.
 *   cgc_region_hull: ws = cgc_region_hull_ws_bytes(max_label, span_rows) bytes, 2 (span_rows + R) points (y, x) of two int32; on
 *     return row L's vertices are the first count[L] points from point 2 (ptr[L] + L), the rest is scratch.  Out, per row:
 *       count          int32 [R]        the number of vertices (>= 4), 0 for a row without a counted pixel -- such a row has zeros everywhere
 *       area2          int64 [R]        twice the area (shoelace)
 *       diameter2      int64 [R]        the largest squared distance between two vertices
 *       diameter_ends  int32 [R, 2, 2]  its two ends (y, x); of equal pairs the one with the smallest vertex indices (i, j), i < j, in
 *                                       hull order
 *       width_cross    int64 [R]        c of the edge of smallest width c / |e|, where for the edge e = v[i + 1] - v[i] = (dy, dx) c is
 *                                       the largest dy (x - x_i) - dx (y - y_i) over the vertices (y, x)
 *       width_edge     int32 [R, 2]     (dy, dx) of that edge.  Edges are compared as c_a^2 |e_b|^2 against c_b^2 |e_a|^2 in 128 bits,
 *                                       exactly; of equal widths the first edge in hull order
 *       perimeter      double [R]       the edge lengths sqrt(dy^2 + dx^2), correctly rounded, summed in hull order
 *     tall_rows: a region of more rows than this is hulled by a whole wave, others by one lane; 0 = cgc_region_hull_tall_rows().  Both
 *     routes give identical tables.  H is the image's, as given to cgc_region_hull_spans.
 * Bit-identical from call to call.  Bad dims, max_label, within_bytes, a side above 32767, span_rows < 0 or > R * H, tall_rows < 0 or a
 * null pointer where one is needed: CGC_EINVAL, nothing launched; a ptr that does not fit the extents writes nothing outside the tables.
 * H * W = 0 or span_rows = 0: rows of zeros. */
int cgc_region_hull_tall_rows(void);
int64_t cgc_region_hull_ws_bytes(int max_label, int64_t span_rows);
int cgc_region_hull_spans(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label, const int* extents,
                          const int64_t* ptr, int64_t span_rows, int* spans, cgc_stream_t stream);
int cgc_region_hull(int max_label, int H, const int* extents, const int64_t* ptr, int64_t span_rows, const int* spans, void* ws,
                    int tall_rows, int* count, int64_t* area2, int64_t* diameter2, int* diameter_ends, int64_t* width_cross, int* width_edge,
                    double* perimeter, cgc_stream_t stream);

/* ---- F21 (in front of F10, and between any two steps of the stage): the pixel size of an image (csrc/resample.hip).  The contract
 * item by item: cgc-net_amd/kernels.py KernelSpec.resample_u8 / resample_labels.  src [H, W] (or [H, W, channels] interleaved) and dst
 * [H2, W2] likewise, both contiguous; every side in 1 .. cgc_resample_max_side() = 32767.  Pixel centres sit at half-integers: output
 * index d of an axis of n source and m output pixels samples the source at ((2 d + 1) n - m) / (2 m), clamped to [0, n - 1], and owns
 * the source interval [d n / m, (d + 1) n / m).  One launch per call, no workspace, integers only, no atomics: bit-identical from
 * call to call.
 *   cgc_resample_u8: channels 1 or 3, each channel on its own.  mode CGC_RESAMPLE_LINEAR: exact rational bilinear interpolation of
 *     the four neighbours, one rounding (half up).  CGC_RESAMPLE_AREA: H2 <= H and W2 <= W; the mean over the owned interval of both
 *     axes, pixels weighted by their overlap, one rounding (half up).
 *   cgc_resample_labels: elem_bytes 1, 2, 4 or 8.  mode CGC_RESAMPLE_NEAREST: dst[d] = src[floor((2 d + 1) n / (2 m))] per axis, the
 *     element copied as it is.  CGC_RESAMPLE_MAJORITY: H2 <= H <= 8 H2 and W2 <= W <= 8 W2 (cgc_resample_labels_max_factor() = 8); the
 *     value of the largest total overlap weight among the pixels that meet the owned box, ties to the smallest value, values compared
 *     as signed integers of elem_bytes bytes.  CGC_RESAMPLE_MAJORITY_UNSIGNED: the same with unsigned comparison, elem_bytes 1 only
 *     (uint8, bool).
 * A side outside 1 .. 32767, another channels, elem_bytes or mode, a size the mode refuses or a null pointer: CGC_EINVAL, nothing
 * launched. */
#define CGC_RESAMPLE_LINEAR 0
#define CGC_RESAMPLE_AREA 1
#define CGC_RESAMPLE_NEAREST 0
#define CGC_RESAMPLE_MAJORITY 1
#define CGC_RESAMPLE_MAJORITY_UNSIGNED 2
int cgc_resample_max_side(void);
int cgc_resample_labels_max_factor(void);
int cgc_resample_u8(const uint8_t* src, int H, int W, int channels, int H2, int W2, int mode, uint8_t* dst, cgc_stream_t stream);
int cgc_resample_labels(const void* src, int elem_bytes, int H, int W, int H2, int W2, int mode, void* dst, cgc_stream_t stream);

/* ---- F22 (behind F19, csrc/outline.hip): the ordered boundary of every region of a label image, as closed loops of lattice corners.
 * The per-label form of the reference's contours (cv2.findContours of one nucleus, dataflow/construct_feature_graph.py).  The contract
 * item by item: cgc-net_amd/kernels.py KernelSpec.region_outlines.  labels, max_label, within_or_null and "a pixel is counted in row L"
 * as F17, sides as F19, and H * W < 2^29 so that a crack id 4 (y W + x) + side fits int32.  A crack of row v is a side (0 top, 1 right,
 * 2 bottom, 3 left) of a counted pixel of v across which no pixel counted in v lies; it runs with its pixel on its right.  The
 * successor of a crack is decided from the 2 x 2 block at its head (connectivity 1: right, straight, left; 2: left, straight,
 * right); the successors are a permutation whose cycles are the loops.  A call is these steps on one stream; between them the caller
 * makes prefix sums, one sort of the loop keys, and two host reads (n_cracks; then n_loops and, for corners, n_vertices):
 *   cgc_region_outline_count: mask uint8 [H, W] = the crack sides of each pixel as bits, count uint8 [H, W] = their number (rows 1 ..
 *     max_label, or 0 .. max_label with background != 0); *meta = the refused pixels.  offsets int32 [H, W] = the caller's INCLUSIVE
 *     prefix sum of count; n_cracks = its last entry.
 *   cgc_region_outline_cracks: crack int32 [n_cracks] = the ids in ascending order, succ int32 [n_cracks] = the compact index of each
 *     crack's successor.
 *   cgc_region_outline_loops: ws = cgc_region_outlines_ws_bytes(n_cracks) bytes.  2 cgc_region_outline_rounds(n_cracks) + 3 launches,
 *     rounds = ceil(log2(n_cracks)): start int32 [n_cracks] = the compact index of the smallest crack of each crack's loop, steps int32
 *     [n_cracks] = the cracks that follow it before the loop returns to its start (position = steps[start] - steps, length =
 *     steps[start] + 1).  rank int32 [n_cracks] = the caller's INCLUSIVE prefix sum of (start[k] == k); n_loops = its last entry.
 *   cgc_region_outline_keys: keys int64 [n_loops] = label << 32 | compact index of each loop's start; the caller sorts them ascending.
 *   cgc_region_outline_tables: from the sorted keys loop_label, loop_start (crack ids), loop_cracks int32 [n_loops]; loop_area2 int64
 *     [n_loops] zeroed; loop_of int32 [n_cracks], the loop's number at its start crack (other entries are not written).  crack_ptr int64
 *     [n_loops + 1] = the caller's prefix sum of loop_cracks, crack_ptr[0] = 0.
 *   cgc_region_outline_scatter: slots int32 [n_cracks, 2] = the tail (y, x) of every crack at crack_ptr[loop] + position: the vertex
 *     list of mode 'cracks'.  loop_area2 += x1 y2 - x2 y1 per crack (tail 1, head 2).  keep_or_null uint8 [n_cracks]: keep[t] = 1 iff
 *     the cracks that meet at the vertex of slot t differ in direction.  place int32 [n_cracks] = the caller's INCLUSIVE prefix sum of
 *     keep; n_vertices = its last entry.
 *   cgc_region_outline_compact: vertices int32 [n_vertices, 2] = the kept slots in order: the vertex list of mode 'corners'.
 * Integer work only, bit-identical from call to call.  Bad dims, max_label, within_bytes, connectivity, a side above 32767, H * W >=
 * 2^29, a count outside its range or a null pointer where one is needed: CGC_EINVAL, nothing launched; tables that do not belong
 * together write nothing outside the outputs.  H * W = 0, n_cracks = 0, n_loops = 0 or n_vertices = 0: nothing to do, 0. */
int cgc_region_outline_rounds(int64_t n_cracks);
int64_t cgc_region_outlines_ws_bytes(int64_t n_cracks);
int cgc_region_outline_count(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label, int background,
                             uint8_t* mask, uint8_t* count, int* meta, cgc_stream_t stream);
int cgc_region_outline_cracks(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label,
                              int connectivity, const uint8_t* mask, const int* offsets, int64_t n_cracks, int* crack, int* succ,
                              cgc_stream_t stream);
int cgc_region_outline_loops(int64_t n_cracks, const int* succ, void* ws, int* start, int* steps, cgc_stream_t stream);
int cgc_region_outline_keys(int64_t n_cracks, int64_t n_loops, const int* labels, const int* crack, const int* start, const int* rank,
                            int64_t* keys, cgc_stream_t stream);
int cgc_region_outline_tables(int64_t n_cracks, int64_t n_loops, const int64_t* keys, const int* crack, const int* steps, int* loop_label,
                              int* loop_start, int* loop_cracks, int64_t* loop_area2, int* loop_of, cgc_stream_t stream);
int cgc_region_outline_scatter(int64_t n_cracks, int64_t n_loops, int W, const int* crack, const int* succ, const int* start,
                               const int* steps, const int* loop_of, const int64_t* crack_ptr, int64_t* loop_area2, int* slots,
                               uint8_t* keep_or_null, cgc_stream_t stream);
int cgc_region_outline_compact(int64_t n_cracks, int64_t n_vertices, const uint8_t* keep, const int* place, const int* slots,
                               int* vertices, cgc_stream_t stream);

/* ---- F23 (behind F11 / F12, in front of F13 and F17 .. F19; csrc/slic.hip): superpixels, the tissue regions between the nuclei.  The
 * contract item by item: cgc-net_amd/kernels.py KernelSpec.slic_iterate and KernelSpec.slic_merge.
 *   cgc_slic_iterate: planes uint8 [C, H, W] contiguous, 1 <= C <= 4, H * W < 2^29; 4 <= step <= cgc_slic_max_step() = 256; 0 <=
 *     compactness <= 1024; 1 <= n_iter <= 64; within_or_null as F17 (only "is zero" is read).  ny = max(1, (2 H + S) / (2 S)), nx
 *     likewise, K = ny nx.  Pixel (y, x) has home cell (y ny / H, x nx / W); centre k = i nx + j starts at y = (2 i + 1) H / (2 ny), x =
 *     (2 j + 1) W / (2 nx) with the colour of that pixel.  A round: every counted pixel takes, among the centres of the up to 9 cells
 *     around its home cell, the one with the smallest D = S^2 sum_c (p_c - c_c)^2 + m^2 ((y - c_y)^2 + (x - c_x)^2) (64 bits), of equal
 *     D the smallest k; then every centre with n > 0 pixels moves to (2 sum + n) / (2 n) per coordinate and colour.  n_iter rounds of two
 *     launches (assign + accumulate, finalize) behind one init launch; no host read.  labels int32 [H, W] = k + 1 of the last
 *     assignment, 0 where within is zero; centres int32 [K, 2 + C] = (y, x, colours) after the last update; count int32 [K] = the
 *     pixels of the last assignment.  ws = cgc_slic_ws_bytes(C, H, W, step) bytes (0 for arguments that are refused).  The assign
 *     launch works on tiles of cgc_slic_tile_side() pixels a side and folds the sums of the cgc_slic_table_side()^2 cells around a
 *     tile's first pixel in LDS; sums of other cells go to global memory directly, with the same integer atomics.
 *   cgc_slic_merge_begin: pieces 1 .. n_pieces of sizes int32 [n_pieces]; group int32 [n_pieces + 1] = p where sizes[p - 1] >= min_size
 *     (settled), 0 elsewhere (group[0] = 0); best uint64 [n_pieces + 1] = 0.
 *   cgc_slic_merge_rounds: `rounds` >= 1 rounds over pairs int32 [n_pairs, 2] (a < b, piece numbers) and count int32 [n_pairs] (F13's
 *     outputs): an unsettled piece p with settled neighbours takes group[q] of the neighbour q with the largest count << 32 | ~q.
 *     Two launches per round.  *changed = the pieces the LAST round settled.  Pairs with an end outside 1 .. n_pieces are skipped.
 *   cgc_slic_relabel: out[i] = table[pieces[i]] for pieces[i] in 1 .. n_pieces, else 0; table int32 [n_pieces + 1].
 * Integer work only, bit-identical from call to call.  An argument outside its range or a null pointer where one is needed:
 * CGC_EINVAL, nothing launched.  H * W = 0, n_pieces = 0: nothing to do, 0. */
int cgc_slic_max_step(void);
int cgc_slic_tile_side(void);
int cgc_slic_table_side(void);
int64_t cgc_slic_ws_bytes(int C, int H, int W, int step);
int cgc_slic_iterate(const uint8_t* planes, int C, int H, int W, int step, int compactness, int n_iter, const void* within_or_null,
                     int within_bytes, void* ws, int* labels, int* centres, int* count, cgc_stream_t stream);
int cgc_slic_merge_begin(const int* sizes, int n_pieces, int min_size, int* group, uint64_t* best, cgc_stream_t stream);
int cgc_slic_merge_rounds(const int* pairs, const int* count, int64_t n_pairs, int n_pieces, int rounds, int* group, uint64_t* best,
                          int* changed, cgc_stream_t stream);
int cgc_slic_relabel(const int* pieces, int64_t n_pixels, int n_pieces, const int* table, int* out, cgc_stream_t stream);

/* ---- A6 (level 1): _re_norm_adj on the CSR (model/network.py:183-191): val[k] = p on the diagonal,
 * (1/(c+1e-15))*(1-p) elsewhere, c = off-diagonal entries of the row.  The CSR must hold its diagonal. */
int cgc_edge_renorm(const int* rowptr, const int* col, int n, float p, float* val, cgc_stream_t stream);

/* t_val[k] = val[t_perm[k]] over the live slots of the transpose: the weights the backward aggregations (A^T ...) use, in
 * their own slot order (no per-edge indirection in the gather kernels). */
int cgc_csr_transpose_vals(const int* t_rowptr, const int* t_perm, const float* val, int n, float* t_val, cgc_stream_t stream);

/* out[i] = 1/max(rowsum_i, 1): the clamp(min=1) mean divisor of DenseSAGEConv (PyG 1.2.1; model/network.py:114). val may be NULL (=1). */
int cgc_csr_invdeg(const int* rowptr, const float* val, int n, float* out, cgc_stream_t stream);

/* The four calls above as one (what graph.BatchGraph needs per batch): CSR + transpose, then -- renorm_p >= 0 -- the edge weights of
 * _re_norm_adj in both slot orders (the CSR then holds its diagonal: cap = E + n), then the mean divisor.  val / t_val: [cap] or NULL
 * when renorm_p < 0.  ws as cgc_csr_build. */
int cgc_graph_build(const int64_t* edge_index, int64_t E, int n, float renorm_p, int* rowptr, int* col, int* rowidx, int* t_rowptr,
                    int* t_col, int* t_perm, float* val, float* t_val, float* inv_d, int* ws, cgc_stream_t stream);
/* The same arrays, bit for bit, for a batch whose edge list is GROUPED BY GRAPH -- what Batch.from_data_list emits: the edges of graph
 * g are edge_index[:, eptr[g] .. eptr[g+1]) and both end points lie in its node range gptr[g] .. gptr[g+1] (gptr, eptr: int32
 * [B + 1] on the device; nmax = the largest graph, emax = the most edges of one graph: known on the host).  One workgroup per graph
 * with everything it indexes at random in LDS: TWO launches instead of ~20 (csrc/csr.hip: k_graph_local_rows, k_graph_local_finish).
 * An edge that leaves its own graph's node range is dropped and counted like an out-of-range id (cgc_graph_build would keep an edge
 * between two graphs of the batch; the reference's dense indexing, model/utils.py:28-33, cannot represent one).  Returns CGC_EINVAL
 * -- nothing launched, use cgc_graph_build -- outside its envelope: nmax <= cgc_graph_local_max_nodes() (4095), emax + nmax <= 32767,
 * 20 (nmax + 1) + 4 (emax + nmax) + 4096 bytes of LDS <= 156 KB, B <= 65535, 2 B <= n + 1.  Outputs and ws as cgc_graph_build. */
int cgc_graph_local_max_nodes(void);
int cgc_graph_build_local(const int64_t* edge_index, int64_t E, int n, const int* gptr, const int* eptr, int B, int nmax, int emax,
                          float renorm_p, int* rowptr, int* col, int* rowidx, int* t_rowptr, int* t_col, int* t_perm, float* val,
                          float* t_val, float* inv_d, int* ws, cgc_stream_t stream);

/* ---- A4 / A8: neighbour aggregation.  Replaces torch.matmul(adj, x) inside DenseSAGEConv
 * (model/network.py:114-116) and the inner product of (S^T A) S (model/network.py:207):
 * out[i,:] = post[i] * sum_{k in row i} w_k * pre[col[k]] * x[col[k],:],  w_k = val[perm[k]] | val[k] | 1.
 * perm, val, pre, post may be NULL.  x, out: [n, width] contiguous.  Narrow widths (<=64) and wide widths
 * (cluster counts) take different kernels. */
int cgc_spmm(const int* rowptr, const int* col, const int* perm, const float* val, const float* pre,
             const float* post, const float* x, float* out, int n, int width, cgc_stream_t stream);

/* Same contract when the rows are a batch of graphs (block-diagonal adjacency): gptr[B+1] = first row of each graph,
 * nmax = largest graph.  Wide rows are then swept one (graph, 1 KiB column tile) slab at a time per XCD so that the ~9x
 * re-read of neighbour rows is served by that XCD's L2.  visit = scheduling hint only (results identical): which graphs
 * of x the previous kernel left in the Infinity Cache -- bits 0-1: 0 unknown / ascending, 1 x was written in ascending row order,
 * 2 x was written by cgc_gemm_f32 as a ragged batch.  Bit 2 (+4, round 5): a NOTE that the nodes of every graph are listed grid cell
 * by grid cell (neighbours in space are neighbours in memory: data.spatial_order).  The gather kernel does not read the bit -- it is
 * the node order itself that makes its re-reads hit nearer caches (+3 % at C3, +30 % at C5).  Higher bits are ignored.
 * gorder[B] (NULL: ascending) lists the graphs in the order in which they are swept, the eight XCDs taking consecutive eighths.  For
 * a few LARGE graphs of unequal size (the stress configuration: 32 graphs of 6400..9600 nodes, 4 per XCD) the host deals the graphs
 * to the XCDs by size (graph.BatchGraph.gorder) so that every XCD gets the same number of rows.  The result does not depend on the
 * sequence. */
int cgc_spmm_graphs(const int* rowptr, const int* col, const int* perm, const float* val, const float* pre,
                    const float* post, const float* x, float* out, int n, int width, int ld /* row stride of x and out
                    (>= width): wide rows are kept at a multiple of 32 floats so that a 128-byte line never holds parts
                    of two rows */, const int* gptr, int B, int nmax, int visit, const int* gorder,
                    cgc_stream_t stream);

/* ---- A4/A5/A8: dense contractions on fp32 MFMA (v_mfma_f32_32x32x2_f32).  Replaces torch.matmul / nn.Linear at
 * model/network.py:122 (assignment Linear), :206-207 (S^T X, S^T A S), and the level-2/3 adj@x.
 * C_b = alpha*op(A_b)*op(B_b) + beta*C_b (+ bias[N]);  op(A): M x K (transA: stored [K,M]); op(B): K x N (transB: stored [N,K]).
 * Operand b starts at base + b*stride.  ragged=1: M_b = gptr[b+1]-gptr[b]; A (transA must be 0) and C advance gptr[b] rows.
 * ragged=2: K_b = gptr[b+1]-gptr[b]; A (transA must be 1) and B (transB must be 0) advance gptr[b] rows.
 * max_ragged >= max_b of the ragged extent (sizes the grid).
 * ragged=3 (uniform row chunks: split-K without an offset array): batch = outer * parts items, parts = ceil(K / max_ragged); item
 * (o, p) reduces over rows [o*K + p*max_ragged, o*K + min((p+1)*max_ragged, K)) of A (transA = 1) and B (transB = 0), the
 * flattened [outer*K, .] row blocks (strideA / strideB ignored), and writes C + (o*parts + p)*strideC: partial products for
 * cgc_reduce_batch_sum / cgc_reduce_batched.
 *
 * nx (<= 2) EXTRA operand pairs continue the reduction: C_b = alpha*( op(A_b)op(B_b) + sum_s op(xA[s]_b)op(xB[s]_b) ) + beta*C_b
 * (+bias), i.e. the product of column-concatenated A's with row-concatenated B's without materialising either (assignment Linear
 * over cat[x1,x2,x3], model/network.py:118-122; dS = P dA'^T + X dX'^T in _diff_pool's backward).  Extra pairs share op(), M, N, the
 * batch and (ragged = 1) the row offsets of the main pair; xK[s] = their reduction length.  Host arrays of length nx; nx = 0: none
 * (the arrays may be NULL).  ragged = 2 is not supported with extra pairs.
 *
 * ws: a SLAB WORKSPACE for the tail split of the 128 x 128 pipelined kernel (round 3): T output tiles on the 512 workgroups the chip
 * holds run in ceil(T / 512) rounds, and the last round lasts as long as a full one however few tiles it holds (4140 tiles = 8.09 -> 9
 * rounds for the step's big products at 32 graphs, 522 tiles = 1.02 -> 2 rounds at 4 graphs per GPU).  With ws != NULL the T mod 512
 * tiles of the last round (all tiles when T < 512) are cut along K into up to 12 pieces each, every piece parks its raw fp32
 * accumulators in a slab of ws, and a second kernel adds a tile's slabs IN PIECE ORDER and applies alpha / beta / bias: deterministic
 * (no atomics, no arrival order), no flags, no spinning.  ws: ws_floats >= cgc_gemm_ws_floats() floats, contents irrelevant before
 * and after; products on one stream may share it.  ws = NULL, ws_floats = 0 (or too small, or a product the split does not apply to:
 * short reductions, other tile shapes): every output tile is computed whole.
 *
 * mode (round 5):  CGC_GEMM_EXACT -- the fp32 matrix-core chain (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain), the default of every
 * caller;  CGC_GEMM_SPLIT_BF16 -- products that take the 128 x 128 route (both output extents > 128, reduction > 160, operands fit
 * for 16-byte loads) are computed on the bf16 matrix cores instead: every fp32 element as hi + mid + lo (three bf16 values, exact),
 * the six pairs above 2^-24 multiplied exactly and summed in fp32 (csrc/gemm_split.hip).  Same forms (NN / NT / TN, ragged 1 / 2 / 3,
 * extra K segments, beta, bias, tail split), same determinism; max and rms error against float64 within 1.25 x the exact kernel's
 * (tests/test_kernels_gpu.py::test_split_gemm_*).  Inputs must be finite; magnitudes below ~2^-108 lose the low planes.  Products the
 * mode does not apply to run on the exact kernel.
 * CGC_GEMM_SPLIT_F16 (round 6, csrc/gemm_half.hip) -- the same products on the fp16 matrix cores in THREE passes: a first launch
 * takes max |x| over every output tile's operand panels (256 rows of op(A), 128 columns of op(B), all of K); every element, scaled
 * by the power of two that puts its panel's maximum in [2^14, 2^15), is split into two fp16 values h + l, the pairs l h, h l, h h
 * are summed in fp32 and the tile is descaled.  Same forms, same determinism; needs ws (its scale slots are the last
 * cgc_gemm_half_ws_floats() floats of the workspace; ws = NULL or more panels than slots: the exact kernel runs).  Error against
 * float64 within 1.25 x the exact kernel's -- measured 0.55-1.0 x -- while an element is within 2^17 of its panel's largest; below
 * that the element's ABSOLUTE error stops shrinking at 2^-40 of the panel's maximum (bound and measurements:
 * tests/test_half_gemm_gpu.py, tools/operand_range.py for the step's own operands).  Inputs must be finite (an infinite element
 * makes the tiles of its panel NaN).  1.25 x faster than CGC_GEMM_SPLIT_BF16 on the step's six products, operand pass included; products
 * too small for that (cgc_gemm_half_min_work) run as CGC_GEMM_SPLIT_BF16.  Any other mode, or nx outside [0, 2]: CGC_EINVAL. */
#define CGC_GEMM_EXACT 0
#define CGC_GEMM_SPLIT_BF16 1
#define CGC_GEMM_SPLIT_F16 2
int cgc_gemm_f32(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                 const float* B, int ldb, float beta, float* C, int ldc, const float* bias, int batch,
                 int64_t strideA, int64_t strideB, int64_t strideC, const int* gptr, int ragged, int max_ragged,
                 int nx, const float* const* xA, const int* xlda, const int64_t* xstrideA,
                 const float* const* xB, const int* xldb, const int64_t* xstrideB, const int* xK,
                 float* ws, int64_t ws_floats, int mode, cgc_stream_t stream);
int64_t cgc_gemm_split_count(void);   /* products this process has sent to the split kernel so far (diagnostic: did the mode apply?) */
int64_t cgc_gemm_half_count(void);    /* ... and to the fp16 kernel of mode CGC_GEMM_SPLIT_F16 */
int64_t cgc_gemm_half_ws_floats(void); /* the part of cgc_gemm_ws_floats() that mode CGC_GEMM_SPLIT_F16 needs by itself (scale slots, at the end) */
/* Mode CGC_GEMM_SPLIT_F16 declines products of fewer than this many (256 x 128 output tile) x (16-wide k-tile) steps -- its maximum pass
 * would cost more than the kernel saves -- and they run in mode CGC_GEMM_SPLIT_BF16 instead (default 28000: the six products of a step
 * from 8 graphs of ~1800 nodes up).  Sets the threshold (v >= 0) and returns the previous one; v < 0 only reads.  Tuning hook like
 * cgc_gemm_tuning: process-wide, not meant to be changed while products are in flight. */
int64_t cgc_gemm_half_min_work(int64_t v);
int64_t cgc_gemm_ws_floats(void);
/* Tuning hook for experiments (tools/gemm_cfg_sweep.py): cfg 1..6 forces the tile shape 128x128, 128x64, 64x128, 64x64, 128x32,
 * 32x128 for every following product of this process, +10 the pipelined kernel, +20 the short-K kernel (a call with extra K
 * segments, which that kernel does not walk, takes the pipelined kernel of the forced tile shape instead); 0 restores the automatic
 * selection.  Returns the previous value.  Results do not depend on it (same arithmetic per output element up to tile-edge order). */
int cgc_gemm_tuning(int cfg);

/* out[j] = beta*out[j] + sum_{s<parts} ws[s*numel + j]  (deterministic split-K combine) */
int cgc_reduce_batch_sum(const float* ws, float* out, int parts, int64_t numel, float beta, cgc_stream_t stream);
/* batched form: ws [outer][parts][numel] -> out [outer][numel] (split-K of a strided batch of small products) */
int cgc_reduce_batched(const float* ws, float* out, int outer, int parts, int numel, float beta, cgc_stream_t stream);

/* ---- A4/A5: conv epilogue.  Replaces F.normalize + activation + nn.BatchNorm1d over the padded [B*Nmax, C]
 * view (model/network.py:101-107,114-116).
 * cgc_stats_blocks(n,F): number of partial-sum slots the column reductions use; ws must hold 2*F floats per slot for the
 * backward reductions (cgc_bn_bwd_reduce, cgc_colsum, ...).  The FORWARD statistics (sum of o, sum of o^2 per column, o = act(hn))
 * are accumulated in double from the first addition on -- the variance is a difference of the two, and on the coarsened levels
 * std << |mean| -- and their slots hold doubles: cgc_stats_ws_floats(n,F) floats of workspace (8-byte aligned) for
 * cgc_l2norm_act_stats / cgc_l2norm_act_bn / cgc_sage_wide_fwd / cgc_sage_narrow_fwd.
 * Envelope: cgc_l2norm_act_stats, cgc_l2norm_act_bn, cgc_bn_act_apply, cgc_bn_bwd_reduce, cgc_bn_act_l2_bwd, cgc_colsum and
 * cgc_softmax_bwd hold a row's columns in the lanes' registers: F (C) <= 2048, otherwise CGC_EINVAL and nothing is launched or
 * written.  cgc_softmax_fwd, the dense adjacency transforms and cgc_adj_prep_fwd / cgc_adj_prep_bwd take any width (rows wider than
 * 2048 floats, or wider than 512 floats that cannot be read with 16-byte loads, on a three-pass streaming route). */
int cgc_stats_blocks(int n, int F);
int64_t cgc_stats_ws_floats(int n, int F);
int cgc_l2norm_act_stats(const float* h, int n, int F, int normalize, int act, float* hn, float* rinv,
                         double* stats /*[2,F] fp64 or NULL*/, float* ws, cgc_stream_t stream);
int cgc_bn_finalize(const double* stats /*[2,F] fp64: the variance is a difference of these sums*/, int F, double count, float eps, float momentum,
                    float* running_mean /*NULL ok*/, float* running_var, float* mean, float* istd, cgc_stream_t stream);
/* The two calls above as ONE (what the training forward uses): hn, rinv, batch statistics over `count` rows, mean / istd,
 * running statistics and num_batches_tracked += 1 (NULL ok).  ws: cgc_stats_ws_floats(n,F) floats. */
int cgc_l2norm_act_bn(const float* h, int n, int F, int normalize, int act, float* hn, float* rinv, float* ws, double count,
                      float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      float* mean, float* istd, cgc_stream_t stream);
/* Inference-mode BatchNorm constants from the running statistics: mean[f] = running_mean[f], istd[f] = 1 / sqrt(running_var[f] + eps)
 * (IEEE division and square root), for cgc_bn_act_apply. */
int cgc_bn_running_stats(const float* running_mean, const float* running_var, int F, float eps, float* mean, float* istd,
                         cgc_stream_t stream);
/* y [n, F] (row stride ldy) and, unless y2 is NULL, a second destination y2 [n, F] (row stride ldy2) receive the same values */
int cgc_bn_act_apply(const float* hn, int n, int F, int act, const float* mean /*NULL: no BN*/, const float* istd,
                     const float* gamma, const float* beta, float* y, int ldy, float* y2, int ldy2, cgc_stream_t stream);
int cgc_bn_bwd_reduce(const float* dy, int ldy, const float* hn, int n, int F, int act, const float* mean,
                      const float* istd, float* sums /*[2,F]*/, float* ws, cgc_stream_t stream);
/* mode: 2 batch statistics, 1 running statistics, 0 no BN */
int cgc_bn_act_l2_bwd(const float* dy, int ldy, const float* hn, const float* rinv, int n, int F, int act,
                      int normalize, int mode, const float* mean, const float* istd, const float* gamma,
                      const float* sums, double count, float* dh,
                      float* dh_colsum /*[F] or NULL: fused column sums of dh = bias gradient of the preceding linear*/,
                      float* ws /*cgc_stats_blocks(n,F)*F floats when dh_colsum != NULL*/, cgc_stream_t stream);
int cgc_colsum(const float* x, int ld, int n, int F, float* out, float* ws, cgc_stream_t stream);

/* ---- A8: row softmax of the assignment matrix (model/network.py:200); A9: max readout (model/network.py:264) */
int cgc_softmax_fwd(const float* x, int n, int C, int ld /*row stride of x and out*/, float* out, cgc_stream_t stream);
int cgc_softmax_bwd(const float* S, const float* dS, int n, int C, int ld /*row stride of S, dS, dx*/, float* dx,
                    float* dx_colsum /*[C] or NULL: fused column sums of dx*/, float* ws, cgc_stream_t stream);
/* torch.max over dim 1 of the dense padded [B, nmax, D] layout, from the flat rows x [n, D] (row stride D) of graphs
 * [gptr[b], gptr[b+1]).  out[b,d] = the maximum over the real rows of graph b, and over one zero as well when the graph has fewer
 * than nmax rows; arg[b,d] = the first real row (index into x) that attains it.  arg = -1 when the padding zero wins strictly or the
 * graph is empty (out = 0 then).  A real row that ties with the padding wins, so a real -0.0 comes out as -0.0.  If any real row of
 * the column is NaN, out is NaN and arg the first NaN row, padded or not.  All real rows -inf: without padding out = -inf and
 * arg = gptr[b]; with padding out = 0 and arg = -1.  +inf wins at its first occurrence. */
int cgc_segment_max_fwd(const float* x, const int* gptr, int B, int D, int nmax, float* out, int* arg, cgc_stream_t stream);
int cgc_segment_max_bwd(const float* dout, const int* arg, int B, int D, float* dx_zeroed, cgc_stream_t stream);
/* The same gradient written in full: dx [n,D] need not be zeroed -- every element of every graph's rows is written (dout where
 * the row is the argmax, 0 elsewhere); rows outside [gptr[0], gptr[B]) are not touched.  nmax = largest graph (grid sizing). */
int cgc_segment_max_bwd_full(const float* dout, const int* arg, const int* gptr, int B, int D, int nmax, float* dx,
                             cgc_stream_t stream);

/* ---- A7: DenseJK (model/network.py:11-55): bi-LSTM(C -> H = 3C/2) over a node's 3 layer embeddings + Linear(2H -> 1)
 * attention + softmax-weighted sum, one thread per node.  xs [n, 3C], out [n, C].  lstm = HOST array of 8 device pointers
 * {w_ih[4H,C], w_hh[4H,H], b_ih[4H], b_hh[4H]} for the forward direction, then the same four for the reverse direction
 * (torch.nn.LSTM layout, gate order i,f,g,o).  HS, CS: [6H, npad] saved hidden / cell states.
 * npad (the same value in the forward and the backward of a call pair): npad >= n and npad % 64 == 0, else every entry point
 * below returns CGC_EINVAL before it launches anything.  One rule for all four, so that a pair of HS / CS buffers is valid for
 * every entry point or for none; rows of DGT / INT (3 * npad floats) then start 16-byte aligned (cgc_gemm_f32's 16-byte loads).
 * The forward writes columns < n of HS / CS (the matrix-core forward also the rest of the last 32-node tile: finite values
 * nobody reads); no backward reads a column >= n, so the buffers need not be cleared.  n <= 0 returns 0 at once.
 * cgc_jk_supported(C): 1 if this C is compiled in (every even C <= 32); cgc_jk_matrix_core(C): 1 if cgc_jk_lstm_fwd,
 * cgc_jk_lstm_bwd_params and cgc_jk_lstm_bwd_flat run it on the matrix-core kernels (C in 4, 8, 12, 16, 20, buffers 16-byte
 * aligned); cgc_jk_lstm_fwd otherwise runs the thread-per-direction kernel, which takes any alignment.
 * cgc_jk_lstm_bwd (the staged backward) always runs the thread-per-direction kernel, for every supported C and any alignment.
 * It writes dxs [n, 3C] and, for the parameter gradients, the transposed buffers DGT [2][4H+1][3*npad] and
 * INT [2][C+2H+1][3*npad] (every column written; the padded columns n .. npad-1 of each time slot are zero in both) whose
 * per-direction product DGT_d * INT_d^T (cgc_gemm_f32, NT) holds
 * [dW_ih | dW_hh | db | .] in rows 0..4H-1 and [. | . | d b_att | d w_att[dH:(d+1)H]] in row 4H.  DHC: [2][2][H][npad] scratch
 * (written and read back, for every C). */
int cgc_jk_supported(int C);
int cgc_jk_matrix_core(int C);
int cgc_jk_lstm_fwd(const float* xs, int n, int npad, int C, const float* const* lstm, const float* w_att,
                    const float* b_att, float* out, float* HS, float* CS, cgc_stream_t stream);
int cgc_jk_lstm_bwd(const float* xs, const float* dout, int n, int npad, int C, const float* const* lstm,
                    const float* w_att, const float* b_att, const float* HS, const float* CS, float* dxs, float* DGT,
                    float* INT, float* DHC, cgc_stream_t stream);
/* The same backward with the parameter gradients accumulated in-kernel (no DGT / INT staging, no GEMM):
 * G [2][4H+1][C+2H+1] = what DGT[d] . INT[d]^T would be (rows: gate pre-activations i,f,g,o then the attention score;
 * columns: x_t (C) | h_{t-1} (H) | 1 | h_t (H); of the last row only the entries that are parameter gradients are
 * defined, the rest is 0).  ws: cgc_jk_bwd_ws_floats(C) floats.  Returns CGC_EINVAL (nothing launched) when the buffers
 * are not 16-byte aligned: use cgc_jk_lstm_bwd then. */
int64_t cgc_jk_bwd_ws_floats(int C);
int cgc_jk_lstm_bwd_params(const float* xs, const float* dout, int n, int npad, int C, const float* const* lstm,
                           const float* w_att, const float* b_att, const float* HS, const float* CS, float* dxs, float* G,
                           float* ws, cgc_stream_t stream);
/* cgc_jk_lstm_bwd_params followed by cgc_jk_unpack_param_grads as one call without the intermediate G (matrix-core channel counts
 * only): flat = cgc_jk_param_grad_floats(C) floats in parameter order.  ws as cgc_jk_lstm_bwd_params. */
int cgc_jk_lstm_bwd_flat(const float* xs, const float* dout, int n, int npad, int C, const float* const* lstm,
                         const float* w_att, const float* b_att, const float* HS, const float* CS, float* dxs, float* flat,
                         float* ws, cgc_stream_t stream);
/* G -> the DenseJK parameter gradients as ONE contiguous buffer of cgc_jk_param_grad_floats(C) floats, in parameter order:
 * per direction dW_ih [4H,C] | dW_hh [4H,H] | db_ih [4H] | db_hh [4H], then d att.weight [2H], d att.bias [1]
 * (model/network.py:27-33: nn.LSTM(C, 3C/2, bidirectional) + nn.Linear(3C, 1)). */
int64_t cgc_jk_param_grad_floats(int C);
int cgc_jk_unpack_param_grads(const float* G, int C, float* flat, cgc_stream_t stream);

/* ---- A4 + A5 for the WIDE layer of the assignment block (DenseSAGEConv(hidden, assign_dim) -> act -> BatchNorm,
 * model/network.py:114-116 with out_channels = the cluster count): hn [n,F] (row stride ldh) = agg [n,K] (row stride lda) @
 * W [K,F] + bias, rows L2-normalised (normalize != 0), rinv [n] as cgc_l2norm_act_stats; with stats != 0 also the BatchNorm
 * statistics of act(hn) over `count` rows exactly as cgc_l2norm_act_bn (same ws size).  One matrix-core kernel in which a
 * workgroup owns whole rows, so only hn is written (a third of the HBM traffic of cgc_gemm_f32 + cgc_l2norm_act_bn).
 * Envelope: K <= 32, F <= 1664 -- otherwise CGC_EINVAL and nothing is launched. */
int cgc_sage_wide_fwd(const float* agg, int lda, const float* W, const float* bias, int n, int K, int F, int normalize, int act,
                      float* hn, int ldh, float* rinv, int stats, float* ws, double count, float eps, float momentum,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* istd,
                      cgc_stream_t stream);

/* ---- forward of a NARROW SAGE projection (hidden width -> hidden width): as cgc_sage_wide_fwd, for F <= 32, K <= 32, hn contiguous:
 * one kernel instead of a short-K cgc_gemm_f32 + cgc_l2norm_act_stats.  Otherwise CGC_EINVAL, nothing launched. */
int cgc_sage_narrow_fwd(const float* agg, int lda, const float* W, const float* bias, int n, int K, int F, int normalize, int act,
                        float* hn, float* rinv, int stats, float* ws, double count, float eps, float momentum,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* istd,
                        cgc_stream_t stream);

/* ---- backward of a NARROW SAGE projection y = BN(act(l2norm(agg W + b))) (the 13 hidden-width layers of a step,
 * model/network.py:109-125) in one kernel + one slot reduction: dy [n,F] (row stride ldy), hn, rinv, mode / mean / istd / gamma /
 * sums / count exactly as cgc_bn_act_l2_bwd; agg [n,fin] (row stride lda), W [fin,F].  Out: dagg [n,fin] = dh W^T (row stride
 * ldd >= fin; NULL: skipped), dwdb [fin*F + F] = dW (= agg^T dh, row-major [fin,F]) followed by db (= column sums of dh); dh itself
 * is never written.
 * ws: cgc_sage_narrow_ws_floats(n, fin, F) floats.  Envelope fin <= 32, F <= 32 -- otherwise CGC_EINVAL, nothing launched. */
int64_t cgc_sage_narrow_ws_floats(int n, int fin, int F);
int cgc_sage_narrow_bwd(const float* dy, int ldy, const float* hn, const float* rinv, int n, int F, int act, int normalize,
                        int mode, const float* mean, const float* istd, const float* gamma, const float* sums, double count,
                        const float* agg, int lda, int fin, const float* W, float* dagg, int ldd, float* dwdb, float* ws,
                        cgc_stream_t stream);

/* ---- A4/A6 at levels 2-3 (dense, real-valued adjacency that carries gradient) */
int cgc_dense_rownorm_fwd(const float* A, int R, int C, float* out, float* invd, float* ge1, cgc_stream_t stream);
int cgc_dense_rownorm_bwd(const float* dOut, const float* Anorm, const float* invd, const float* ge1, int R, int C,
                          float* dA, cgc_stream_t stream);
int cgc_dense_renorm_fwd(const float* A, int R, int C, float p, float* out, cgc_stream_t stream);
int cgc_dense_renorm_bwd(const float* A, const float* dOut, int R, int C, float p, float* dA, cgc_stream_t stream);

/* ---- A4 + A6 fused (levels 2-3): At = _re_norm_adj(A, p) (skipped when p < 0: At may be NULL and "At" below means A), then
 * s = rowsum(At), d = max(s,1), An = At/d, invd = 1/d, ge1 = (s >= 1) -- one pass over the [R = B*C, C] adjacency
 * (model/network.py:183-191,259-262 + DenseSAGEConv's clamp(min=1)). */
int cgc_adj_prep_fwd(const float* A, int R, int C, float p, float* At, float* An, float* invd, float* ge1, cgc_stream_t stream);
/* its backward: gAn = gradient w.r.t. An, gAt = gradient that reaches At directly (NULL if none; e.g. from At*S of _diff_pool):
 * dAt = invd*(gAn - ge1*<gAn,An>_row) + gAt, dA = backward of the re-normalisation at dAt (dA = dAt when p < 0). */
int cgc_adj_prep_bwd(const float* A, const float* An, const float* invd, const float* ge1, const float* gAn, const float* gAt,
                     int R, int C, float p, float* dA, cgc_stream_t stream);

/* ---- small layout helpers of the step sequencer (also usable on their own) */
/* dst[r, off_i : off_i + width_i] (=, or += when accumulate != 0) src_i[r, 0:width_i], off_i = width_0 + .. + width_{i-1}: the column
 * concatenation torch.cat(srcs, dim=1) (model/network.py:118) / its gradient scatter, for up to 4 sources with their own row strides. */
int cgc_cat_cols(float* dst, int ldd, int rows, int nsrc, const float* const* srcs, const int* lds, const int* widths,
                 int accumulate, cgc_stream_t stream);
/* dst [cols, rows] (row stride ldd) = src [rows, cols] (row stride lds) transposed */
int cgc_transpose(const float* src, int lds, int rows, int cols, float* dst, int ldd, cgc_stream_t stream);

/* ==== Step sequencer (round 3): one level of SoftPoolingGcnEncoder.forward (model/network.py:258-268 | :270-278 | :279-285) and
 * its backward as ONE call each.  A level = optional adjacency preparation (levels 2-3) -> the embedding block and (levels 1-2)
 * the assignment block run layer by layer in lockstep (GNN_Module.forward, model/network.py:109-125) -> DenseJK -> max readout ->
 * Linear over cat + softmax -> _diff_pool.  The call enqueues the same kernels, in the same order, that the per-operator entry
 * points above would be asked for one by one by a Python autograd graph (328 launches per step) -- without Python, without
 * autograd nodes, without per-launch allocations: activations live in two caller-provided arenas.  Stateless like everything
 * else here: no allocation, no synchronisation, safe for concurrent callers with distinct arenas.
 * Scope: DenseSAGEConv blocks (normalize, add_loop = False), training mode (BatchNorm batch statistics) or no BatchNorm, fixed
 * momentum; anything else stays on the per-operator path.                                                                     */
typedef struct {
  int level;              /* 1: flat rows + CSR; 2, 3: dense [B, C, .] tensors */
  int B;                  /* graphs */
  int n;                  /* rows: total nodes (level 1) or B * rows_per_graph */
  int rows_per_graph;     /* levels 2-3: clusters of the previous level; level 1: 0 */
  int nmax, npad;         /* level 1: largest graph; rows per graph of the reference's dense layout (readout vs zero padding) */
  int fin;                /* input features */
  int H, E;               /* embedding block: hidden width, last-layer width */
  int AH, C;              /* assignment block: hidden width, clusters; C = 0: no assignment block (level 3) */
  int has_bias, has_bn, act, jk, renorm;   /* jk: DenseJK over the embedding block's three outputs (needs H == E) */
  float renorm_p;
  float bn_eps[6], bn_momentum[6];         /* embedding block layers 0..2, assignment block layers 3..5 */
  double count;           /* rows BatchNorm statistics are taken over: B * npad (level 1, padding included), n otherwise */
  int eval;               /* 1: inference forward (model.eval() under no_grad; train.py:21-91): BatchNorm normalises with the running
                           * statistics and leaves them alone, nothing is kept for a backward (`saved` is working memory only);
                           * cgc_level_bwd refuses such a descriptor */
  int flags;              /* bit 0: reserved, must be 0 (rounds 4-5: an opt-in thin-operand form of the dense levels' adjacency gradient;
                           * it missed the 1e-4 gradient bar on two reference fixtures and was removed with ABI 4 -- DESIGN.md section 8);
                           * bit 1: the level's products run with mode CGC_GEMM_SPLIT_BF16 (cgc_gemm_f32): those on the 128 x 128
                           * route as six bf16 MFMA pairs per fp32 product.  Off by default;
                           * bit 2: the same with mode CGC_GEMM_SPLIT_F16 (three fp16 pairs); bits 1 and 2 exclude each other;
                           * bit 3: DiffPool regularisers (link and entropy losses of the level's pooling: cgc_diffpool_reg_fwd below).
                           * Only on a level with an assignment block; needs reg_out / d_reg of cgc_level_fwd / cgc_level_bwd
                           * (NULL: the call is refused).  Bits above 3 are unassigned and refused */
} cgc_level_desc;

typedef struct {          /* one GNN_Module's parameters (DEVICE pointers; unused ones NULL) */
  const float* W[3];      /* DenseSAGEConv.weight [in, out] */
  const float* b[3];
  const float* gamma[3];
  const float* beta[3];
  float* running_mean[3];
  float* running_var[3];
  int64_t* num_batches_tracked[3];
  const float* lin_W;     /* nn.Linear(2 AH + C, C).weight [C, 2 AH + C] (assignment block only) */
  const float* lin_b;
} cgc_block_params;

typedef struct {
  const float* lstm[8];   /* as cgc_jk_lstm_fwd */
  const float* w_att;
  const float* b_att;
} cgc_jk_params;

typedef struct {          /* level 1: what graph.BatchGraph holds */
  const int* rowptr; const int* col; const int* t_rowptr; const int* t_col;
  const float* val; const float* t_val;   /* NULL without _re_norm_adj */
  const float* inv_d;
  const int* gorder;      /* NULL or the visiting sequence of cgc_spmm_graphs */
  int spatial;            /* 1: every graph's nodes are listed grid cell by grid cell (cgc_spmm_graphs: visit bit 2) */
} cgc_graph;

typedef struct {          /* element offsets into the gradient buffer of cgc_level_bwd; -1 = absent */
  int64_t W[6], b[6], bn_weight[6], bn_bias[6];   /* layers 0..2 embedding block, 3..5 assignment block */
  int64_t lin_W, lin_b;
  int64_t jk;             /* cgc_jk_param_grad_floats(H) floats in parameter order */
  int64_t total;
} cgc_level_grad_layout;

int cgc_level_supported(const cgc_level_desc* d);                      /* 1 if the sequencer covers this configuration */
int64_t cgc_level_saved_floats(const cgc_level_desc* d);               /* arena kept from cgc_level_fwd to cgc_level_bwd */
int64_t cgc_level_scratch_floats(const cgc_level_desc* d);             /* arena either call may overwrite */
int cgc_level_grad_layout_of(const cgc_level_desc* d, cgc_level_grad_layout* out);
/* x_in [n, fin]; A_in [B, C, C] (levels 2-3; NULL at level 1); gptr [B+1] first row of every graph.
 * Out: readout [B, D] (D = H with jk, else 2H + E); x_out [B, C, D] and A_out [B, C, C] (levels 1-2); assign_out (optional, may be
 * NULL): receives the address of the assignment matrix S [n, C] inside `saved` and *assign_ld its row stride.  reg_out [2] (device):
 * with flags bit 3, the DiffPool regularisers of the level -- link, entropy loss as PyG's dense_diff_pool defines them
 * (cgc_diffpool_reg_fwd); not read without bit 3 (may be NULL). */
int cgc_level_fwd(const cgc_level_desc* d, const cgc_block_params* emb, const cgc_block_params* pool, const cgc_jk_params* jk,
                  const cgc_graph* g, const int* gptr, const float* x_in, const float* A_in, float* saved, float* scratch,
                  float* readout, float* x_out, float* A_out, const float** assign_out, int* assign_ld, float* reg_out,
                  cgc_stream_t stream);
/* d_readout [B, D]; d_x_out / d_A_out: gradients of x_out / A_out (NULL at level 3); d_reg [2] (device): with flags bit 3, the
 * upstream gradients of reg_out (zeros when a loss does not reach the objective); not read without bit 3 (may be NULL).
 * Out: grads (cgc_level_grad_layout_of), d_x_in [n, fin] and d_A_in [B, C, C] (levels 2-3; NULL at level 1: the input features
 * carry no gradient). */
int cgc_level_bwd(const cgc_level_desc* d, const cgc_block_params* emb, const cgc_block_params* pool, const cgc_jk_params* jk,
                  const cgc_graph* g, const int* gptr, const float* x_in, const float* A_in, const float* saved, float* scratch,
                  const float* d_readout, const float* d_x_out, const float* d_A_out, const float* d_reg, float* grads,
                  float* d_x_in, float* d_A_in, cgc_stream_t stream);

/* ==== DiffPool regularisers (csrc/diffpool_reg.hip), the passes around the products G = S^T S and S G.  For one pooling stage with
 * assignment S [n, C] (row stride lds), the stage's adjacency A, dense padding N, numel = B N N, rows = B N:
 *   link = ||A - S S^T||_F / numel = sqrt(||A||^2 - 2 sum_b tr(A'_b) + sum_b ||G_b||^2) / numel,   A' = S^T A S (A_out of _diff_pool)
 *   ent  = sum_rows sum_j -S log(S + 1e-15) / rows
 * All sums in double over fixed grids, combined in a fixed order (deterministic).  ws: cgc_diffpool_reg_ws_floats() floats, 16-byte
 * aligned.  fwd: G, A_out [B, C, C] contiguous; A = dense adjacency of A_numel floats (rowptr NULL), or rowptr = the CSR's row
 * pointer over n rows with A its values (NULL: all ones).  Writes link, ent (device scalars) and keep[0] = sqrt(T) for the backward.
 * bwd_prep: c_l = d_reg[0] / (2 numel keep[0]), c_e = d_reg[1] / rows -> coef [2]; dao = d_ao - 2 c_l I per graph (d_ao NULL: 0),
 * Gs = 4 c_l G.  entropy_bwd: ds[:, :C] (row stride ldd) += c_e (-log(S + 1e-15) - S / (S + 1e-15)).  adj_bwd: gA (+)= 2 c_l A. */
int64_t cgc_diffpool_reg_ws_floats(void);
int cgc_diffpool_reg_fwd(const float* S, int n, int C, int lds, const float* G, const float* A_out, int B, const float* A, int64_t A_numel,
                         const int* rowptr, double numel, double rows, float* ws, float* link, float* ent, float* keep, cgc_stream_t stream);
int cgc_diffpool_reg_bwd_prep(const float* d_reg, const float* keep, double numel, double rows, const float* d_ao, float* dao,
                              const float* G, float* Gs, int B, int C, float* coef, cgc_stream_t stream);
int cgc_diffpool_reg_entropy_bwd(const float* S, int n, int C, int lds, const float* coef, float* ds, int ldd, cgc_stream_t stream);
int cgc_diffpool_reg_adj_bwd(const float* A, int64_t m, const float* coef, float* gA, int accumulate, cgc_stream_t stream);

/* ==== A10: classification head + loss (model/network.py:220-234, 286-289): logits = Linear2(dropout(act(Linear1(cat(readouts))))),
 * loss = mean cross-entropy(logits, y), one kernel; the backward another.  x: HOST array of nseg (<= 3) device pointers [B, D] (the
 * readouts; never concatenated); W1 [H1, nseg*D], W2 [L, H1] in nn.Linear layout; y int64 [B] (NULL: logits only); drop_p in [0,1):
 * the mask is a counter-based function of (seed, element index).  ws: 3*B*H1 + B floats, passed again to the backward.
 * Backward: dloss = device scalar gradient of the mean loss (NULL = 0), dlogits_ext [B, L] or NULL; scratch: B*L + B*H1 floats;
 * grads = dW1 | db1 | dW2 | db2 back to back; dx: HOST array of nseg device pointers [B, D]. */
int cgc_head_fwd(const float* const* x, int nseg, int B, int D, int H1, int L, int act, const float* W1, const float* b1,
                 const float* W2, const float* b2, const int64_t* y, float drop_p, uint64_t seed, float* ws, float* logits,
                 float* loss, cgc_stream_t stream);
int cgc_head_bwd(const float* const* x, int nseg, int B, int D, int H1, int L, int act, const float* W1, const float* W2,
                 const int64_t* y, const float* ws, const float* logits, const float* dloss, const float* dlogits_ext,
                 float* scratch, float* grads, float* const* dx, cgc_stream_t stream);

/* ==== The optimiser of the training step (common/utils.py:119-121: torch.optim.Adam(lr 1e-3, weight_decay 1e-4); train.py:183
 * optimizer.step()) as ONE launch over all parameters.  The gradients of a level are one flat buffer (cgc_level_grad_layout), the
 * head's another, so every parameter's gradient is (buffer index, offset): the caller builds two DEVICE tables once --
 * segs[nseg] and blocks[nblocks] = (segment, chunk of 1024 elements) pairs covering every segment -- and a step passes the
 * addresses of the (up to four) gradient buffers as a HOST array plus the scalars.  Update rule: Adam with the L2 penalty added to
 * the gradient, bias-corrected with `step` (1, 2, ...); grad_mul scales the gradients first (1 / replicas after a summing
 * all-reduce; 1.0 = none).  Mixed precision as torch's fused kernel (double hyper-parameters, float state). */
typedef struct {
  float* p;               /* parameter */
  float* m;               /* exp_avg */
  float* v;               /* exp_avg_sq */
  int64_t off;            /* first element of the parameter's gradient inside its buffer */
  int64_t n;              /* elements */
  int32_t slot;           /* index into grad_buffers (0..3) */
  int32_t reserved;
} cgc_adam_seg;
int cgc_adam_step(const void* segs, const void* blocks, int nblocks, const float* const* grad_buffers, double lr, double beta1,
                  double beta2, double weight_decay, double eps, float step, float grad_mul, cgc_stream_t stream);

/* ==== The reference's other optimisers (common/utils.py:122-127: torch.optim.SGD / RMSprop, momentum 0.9) as ONE launch each, on the
 * same two tables as cgc_adam_step (no second layout; cgc_opt_seg is another name for the row).  What the two state columns hold:
 *   SGD:     m = momentum_buffer (NULL when momentum is 0), v unused (NULL)
 *   RMSprop: m = square_avg, v = momentum_buffer (NULL when momentum is 0)
 * SGD: weight decay, buf = momentum * buf + (1 - dampening) * g, p -= lr * buf -- torch._fused_sgd_'s arithmetic (double scalars,
 * float state).  RMSprop (not centred): torch.optim.RMSprop(foreach=True)'s sequence of float kernels.  grad_mul scales the
 * gradients first.  nblocks <= 0: nothing to do, 0.  NULL tables or negative momentum: CGC_EINVAL, nothing launched.  A segment
 * whose rule needs a state pointer that is NULL is left untouched. */
typedef cgc_adam_seg cgc_opt_seg;
int cgc_sgd_step(const void* segs, const void* blocks, int nblocks, const float* const* grad_buffers, double lr, double momentum,
                 double dampening, double weight_decay, float grad_mul, cgc_stream_t stream);
int cgc_rmsprop_step(const void* segs, const void* blocks, int nblocks, const float* const* grad_buffers, double lr, double alpha,
                     double eps, double weight_decay, double momentum, float grad_mul, cgc_stream_t stream);

/* ==== Measurement hook (csrc/timing.hip): HIP events around every launch of the dominant 128 x 128 GEMM (tag 1) and of the wide
 * SpMM (tag 2), recorded on the stream of the launch, whoever asked for it (per-operator call or step sequencer).  One observer
 * per process; nothing is recorded -- and nothing costs anything -- unless one is attached.  After the stream has been
 * synchronised, record i gives tag_and_dims[8] = {tag, M, N, K, batch, ragged, ragged extent bound, extra K} (GEMM) or
 * {tag, n, width, ld, weighted, 0, 0, 0} (SpMM) and the elapsed milliseconds. */
void* cgc_timing_create(int max_records);
int cgc_timing_attach(void* handle /* NULL detaches */);
int cgc_timing_count(void* handle);
int cgc_timing_read(void* handle, int i, int* tag_and_dims, float* ms);
int cgc_timing_destroy(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* CGC_HIP_H */
