// Grayscale morphological reconstruction (Vincent 1993) of a 2-D int32 image on gfx950: reconstruction by dilation of a marker under a
// mask, and by erosion as its dual through bitwise NOT.  Integers throughout, so every result is bit for bit.  The (max, min)
// counterpart of geodesic.hip, on the same schedule (tile_relax.hpp).  Contract item by item: cgc-net_amd/kernels.py
// KernelSpec.morph_reconstruct; launches, workspace and the worst case: DESIGN.md, "Morphological reconstruction".
//
// R0 = min(marker, mask); the answer is the unique fixed point of  R[p] = min(mask[p], max(R[p], max over neighbours q of R[q]))  that
// is reached from R0 by raising values: R[p] = the largest, over pixels q and paths from q to p, of min(R0[q], min of mask along the
// path).  Values only ever increase and every stored value is the value of a real path, so the order in which updates arrive does not
// matter.  By erosion: x -> ~x reverses the order of all of int32 without overflow, so begin stores ~marker and ~mask and finish
// stores ~R.  Launches:
//   k_rec_begin   one workgroup per 64 x 64 tile: R = min(marker, mask) and the mask (both complemented for erosion) into the
//                 workspace; stamp[tile] = 0 when some pixel of the tile lies below its mask, else -1
//   k_rec_round   round r, one workgroup per tile, on the schedule of tile_relax.hpp: the tile loads R with a one-pixel halo and its
//                 mask into LDS, returns if R equals the mask on the whole tile (nothing can rise), relaxes in LDS until nothing in
//                 the tile moves (INSIDE A TILE below) and stores the values that moved.
//   k_rec_finish  R (complemented for erosion) -> out
//
// INSIDE A TILE a Jacobi sweep would need one iteration per pixel of path length.  Instead a thread owns 16 consecutive pixels of one
// line and scans them forward and backward in registers, carrying the running value along; the lines are the rows in one phase and
// the columns in the next, with a barrier between phases, so a value travels 16 pixels per phase along a line and the loop ends after
// an iteration (both phases) in which nothing moved -- every pixel has then been compared with all of its neighbours' final values.
// The 64 lanes of a wave hold the 64 lines at the same position, so with connectivity 2 the two diagonal predecessors of a pixel are
// the carries of the lanes next door (a shuffle); the outermost lanes take them from the tile's halo.  The LDS row is 67 words: an odd
// stride keeps the 64 rows that a wave reads in the row phase on distinct banks; the column phase reads consecutive words.
//
// TERMINATION, clause (1) of tile_relax.hpp: values only increase and every stored value is the value of a real path; halo values are
// read and values are stored as single 32-bit relaxed atomics.
#include <stdint.h>

#include "tile_relax.hpp"

namespace {

constexpr int REC_SEG = RELAX_PER_THREAD;         // pixels of a line that one thread scans: 16
constexpr int REC_LW = RELAX_TILE + 3;            // LDS row: the tile, a one-pixel halo and one word that makes the stride odd
constexpr int REC_LPX = (RELAX_TILE + 2) * REC_LW;      // 66 rows * 67 words; R and mask: 2 * 17688 bytes
constexpr int REC_LOW = INT32_MIN;                // neutral for max: outside the image

struct RecWs {
  int* r;                // [H*W] the reconstruction so far (complemented for erosion)
  int* mask;             // [H*W] the mask (complemented for erosion)
  int* stamp;            // [tiles] the last round the tile has been asked to run in
};
static inline RecWs rec_layout(Carver&& c, int H, int W) {      // the one definition of the workspace
  RecWs w;
  w.r = c.take<int>((int64_t)H * W);
  w.mask = c.take<int>((int64_t)H * W);
  w.stamp = c.take<int>((int64_t)relax_tiles(H) * relax_tiles(W));
  return w;
}

// (a) clamp, complement, stamps.  flip = 0 (dilation) or ~0 (erosion).
__global__ void __launch_bounds__(CGC_BLOCK) k_rec_begin(const int* __restrict__ marker, const int* __restrict__ mask, int flip, int H,
                                                         int W, int tiles_x, int* __restrict__ r, int* __restrict__ mk,
                                                         int* __restrict__ stamp) {
  relax_begin_tile(H, W, tiles_x, stamp, [&](int64_t i) {
    const int m = mask[i] ^ flip, v = min(marker[i] ^ flip, m);
    r[i] = v;
    mk[i] = m;
    return v < m;
  });
}

__device__ __forceinline__ int lds_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_put(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// One phase: lane l of wave s scans positions 16 s .. 16 s + 15 of line l forward and backward (lines = rows when ROWS, else columns).
// Returns whether a value of this thread rose.  Every lane is active: the shuffles need that.
template <bool ROWS, bool CONN8>
__device__ __forceinline__ int rec_scan(int* r, const int* m) {
  constexpr int SL = ROWS ? REC_LW : 1, SJ = ROWS ? 1 : REC_LW;      // LDS distance between lines, between positions
  const int l = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int base = REC_LW + 1 + l * SL + seg * REC_SEG * SJ;
  int old[REC_SEG], v[REC_SEG], lim[REC_SEG];
#pragma unroll
  for (int j = 0; j < REC_SEG; ++j) {
    old[j] = v[j] = lds_get(r + base + j * SJ);
    lim[j] = m[base + j * SJ];
  }
  int edge[REC_SEG + 2];                          // lane 0: line -1, lane 63: line 64 (the halo), positions -1 .. 16 of the segment
  if (CONN8) {
    const int eb = base + (l == 0 ? -SL : l == 63 ? SL : 0);
#pragma unroll
    for (int j = 0; j < REC_SEG + 2; ++j) edge[j] = lds_get(r + eb + (j - 1) * SJ);
  }
  int carry = lds_get(r + base - SJ);             // may belong to the thread of the segment before: stale or fresh, both are real
#pragma unroll
  for (int j = 0; j < REC_SEG; ++j) {
    int cand = carry;
    if (CONN8) {
      int a = __shfl_up(carry, 1), b = __shfl_down(carry, 1);
      if (l == 0) a = edge[j];
      if (l == 63) b = edge[j];
      cand = max(cand, max(a, b));
    }
    v[j] = min(lim[j], max(v[j], cand));
    carry = v[j];
  }
  carry = lds_get(r + base + REC_SEG * SJ);
#pragma unroll
  for (int j = REC_SEG - 1; j >= 0; --j) {
    int cand = carry;
    if (CONN8) {
      int a = __shfl_up(carry, 1), b = __shfl_down(carry, 1);
      if (l == 0) a = edge[j + 2];
      if (l == 63) b = edge[j + 2];
      cand = max(cand, max(a, b));
    }
    v[j] = min(lim[j], max(v[j], cand));
    carry = v[j];
  }
  int ch = 0;
#pragma unroll
  for (int j = 0; j < REC_SEG; ++j) {
    if (v[j] != old[j]) {                         // only this thread writes these cells in this phase
      lds_put(r + base + j * SJ, v[j]);
      ch = 1;
    }
  }
  return ch;
}

// (b) one round
template <bool CONN8>
__global__ void __launch_bounds__(CGC_BLOCK) k_rec_round(int* __restrict__ rec, const int* __restrict__ mk, int* __restrict__ stamp, int H,
                                                         int W, int tiles_x, int tiles_y, int round, int* __restrict__ changed) {
  __shared__ int r[REC_LPX];
  __shared__ int m[REC_LPX];
  if (!relax_tile_runs(stamp, round)) return;
  const RelaxTile t = relax_tile(tiles_x);
  const bool open = relax_load_halo<int, REC_LW>(rec, H, W, t, [&](int c, const RelaxCell<int>& cell) {
    int v = REC_LOW, lim = REC_LOW;               // outside the image (and the padding word of a row): never rises, never raises
    if (cell.inside) {
      v = cell.load();
      if (!cell.halo) lim = mk[cell.i];
    }
    r[c] = v;
    m[c] = lim;
    return v < lim;
  });
  if (!open) return;                              // R equals the mask on the whole tile: nothing can rise

  for (;;) {
    int ch = rec_scan<true, CONN8>(r, m);
    __syncthreads();
    ch |= rec_scan<false, CONN8>(r, m);
    if (!__syncthreads_or(ch)) break;             // an iteration in which nothing moved read final values only: the tile's fixed point
  }

  // rec[i] is still what this tile loaded: nobody else stores into it
  const int moved = relax_write_back<int, REC_LW>(rec, r, H, W, t, [&](int, int64_t i, const int& v) { return v != rec[i]; });
  relax_publish(moved, t, tiles_x, tiles_y, stamp, round, changed);
}

// (c) R -> out
__global__ void __launch_bounds__(CGC_BLOCK) k_rec_finish(const int* __restrict__ r, int flip, int64_t npix, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i < npix) out[i] = r[i] ^ flip;
}

}  // namespace

extern "C" int64_t cgc_reconstruct_ws_bytes(int H, int W) {
  if (bad_image_dims(H, W)) return 0;
  return layout_bytes(rec_layout, H, W);
}

extern "C" int cgc_reconstruct_begin(const int* marker, const int* mask, int H, int W, int by_erosion, void* ws, cgc_stream_t stream) {
  if (bad_image_dims(H, W)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (marker == nullptr || mask == nullptr || ws == nullptr) return CGC_EINVAL;
  const RecWs w = rec_layout(Carver(ws), H, W);
  const int tiles_x = relax_tiles(W), tiles_y = relax_tiles(H);
  hipLaunchKernelGGL(k_rec_begin, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), marker, mask, by_erosion ? ~0 : 0, H, W,
                     tiles_x, w.r, w.mask, w.stamp);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_reconstruct_rounds(int H, int W, int connectivity, void* ws, int first_round, int rounds, int* changed,
                                      cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_connectivity(connectivity)) return CGC_EINVAL;
  const RecWs w = rec_layout(Carver(ws), H, W);
  const int tiles_x = relax_tiles(W), tiles_y = relax_tiles(H);
  const auto kernel = connectivity == 2 ? k_rec_round<true> : k_rec_round<false>;
  return relax_batch(H, W, ws, first_round, rounds, changed, stream, [&](int round, int* count) {
    hipLaunchKernelGGL(kernel, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), w.r, w.mask, w.stamp, H, W, tiles_x,
                       tiles_y, round, count);
  });
}

extern "C" int cgc_reconstruct_finish(int H, int W, int by_erosion, const void* ws, int* out, cgc_stream_t stream) {
  if (bad_image_dims(H, W)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr || out == nullptr) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const RecWs w = rec_layout(Carver(const_cast<void*>(ws)), H, W);
  hipLaunchKernelGGL(k_rec_finish, dim3((unsigned)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), w.r, by_erosion ? ~0 : 0,
                     npix, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
