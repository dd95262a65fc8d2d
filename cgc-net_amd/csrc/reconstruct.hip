// Grayscale morphological reconstruction (Vincent 1993) of a 2-D int32 image on gfx950: reconstruction by dilation of a marker under a
// mask, and by erosion as its dual through bitwise NOT.  Integers throughout, so every result is bit for bit.  The (max, min)
// counterpart of geodesic.hip, whose driver pattern it shares.  Contract item by item: cgc-net_amd/kernels.py
// KernelSpec.morph_reconstruct; launches, workspace and the worst case: DESIGN.md, "Morphological reconstruction".
//
// R0 = min(marker, mask); the answer is the unique fixed point of  R[p] = min(mask[p], max(R[p], max over neighbours q of R[q]))  that
// is reached from R0 by raising values: R[p] = the largest, over pixels q and paths from q to p, of min(R0[q], min of mask along the
// path).  Values only ever increase and every stored value is the value of a real path, so the order in which updates arrive does not
// matter.  By erosion: x -> ~x reverses the order of all of int32 without overflow, so begin stores ~marker and ~mask and finish
// stores ~R.  Launches:
//   k_rec_begin   one workgroup per 64 x 64 tile: R = min(marker, mask) and the mask (both complemented for erosion) into the
//                 workspace; stamp[tile] = 0 when some pixel of the tile lies below its mask, else -1
//   k_rec_round   round r, one workgroup per tile.  A tile runs when stamp[tile] >= r: it loads R with a one-pixel halo and its mask
//                 into LDS, returns if R equals the mask on the whole tile (nothing can rise), relaxes in LDS until nothing in the tile
//                 moves, writes the moved values back and, if any moved, sets stamp = r + 1 on its eight neighbours.
//   k_rec_finish  R (complemented for erosion) -> out
// No workgroup ever waits for another one: the only ordering is the launch boundary, and the convergence loop is the caller's (it reads
// the number of tiles that moved in the last round of a batch of rounds).
//
// INSIDE A TILE a Jacobi sweep would need one iteration per pixel of path length.  Instead a thread owns 16 consecutive pixels of one
// line and scans them forward and backward in registers, carrying the running value along; the lines are the rows in one phase and
// the columns in the next, with a barrier between phases, so a value travels 16 pixels per phase along a line and the loop ends after
// an iteration (both phases) in which nothing moved -- every pixel has then been compared with all of its neighbours' final values.
// The 64 lanes of a wave hold the 64 lines at the same position, so with connectivity 2 the two diagonal predecessors of a pixel are
// the carries of the lanes next door (a shuffle); the outermost lanes take them from the tile's halo.  The LDS row is 67 words: an odd
// stride keeps the 64 rows that a wave reads in the row phase on distinct banks; the column phase reads consecutive words.
//
// TERMINATION.  As in geodesic.hip: within a round a tile may read a neighbour's halo values stale or fresh.  That is harmless because
// (1) values only increase and every stored value is the value of a real path, so a stale value is only a weaker bound, never a wrong
// one, and halo values are read and values are stored as single 32-bit relaxed atomics; (2) a tile whose values moved in round r stamps
// its neighbours for round r + 1, where they read what round r stored -- an earlier launch; (3) the caller stops only after a round in
// which no tile stored anything: every tile that ran is at its fixed point with respect to the current values, and a tile that did not
// run has been at its fixed point since its last run.  All tiles at their fixed point is the fixed point above.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

constexpr int REC_TILE = 64;                      // tile edge: 4096 pixels, 16 per thread
constexpr int REC_SEG = REC_TILE * REC_TILE / CGC_BLOCK;      // pixels of a line that one thread scans: 16
constexpr int REC_LW = REC_TILE + 3;              // LDS row: the tile, a one-pixel halo and one word that makes the stride odd
constexpr int REC_LPX = (REC_TILE + 2) * REC_LW;  // 66 rows * 67 words; R and mask: 2 * 17688 bytes
constexpr int REC_LOW = INT32_MIN;                // neutral for max: outside the image
static_assert(REC_TILE == 64 && CGC_BLOCK == 256 && REC_SEG == 16, "a wave holds the 64 lines of a tile, a workgroup its four quarters");

static inline int rec_tiles(int n) { return ceil_div(n, REC_TILE); }

struct RecWs {
  int* r;                // [H*W] the reconstruction so far (complemented for erosion)
  int* mask;             // [H*W] the mask (complemented for erosion)
  int* stamp;            // [tiles] the last round the tile has been asked to run in
};
static inline RecWs rec_layout(Carver&& c, int H, int W) {      // the one definition of the workspace
  RecWs w;
  w.r = c.take<int>((int64_t)H * W);
  w.mask = c.take<int>((int64_t)H * W);
  w.stamp = c.take<int>((int64_t)rec_tiles(H) * rec_tiles(W));
  return w;
}

// (a) clamp, complement, stamps.  flip = 0 (dilation) or ~0 (erosion).  Consecutive threads take consecutive pixels of a tile row.
__global__ void __launch_bounds__(CGC_BLOCK) k_rec_begin(const int* __restrict__ marker, const int* __restrict__ mask, int flip, int H,
                                                         int W, int tiles_x, int* __restrict__ r, int* __restrict__ mk,
                                                         int* __restrict__ stamp) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * REC_TILE, x0 = tx * REC_TILE;
  int open = 0;
  for (int j = 0; j < REC_SEG; ++j) {
    const int p = threadIdx.x + j * CGC_BLOCK;
    const int y = y0 + (p >> 6), x = x0 + (p & 63);
    if (y >= H || x >= W) continue;
    const int64_t i = (int64_t)y * W + x;
    const int m = mask[i] ^ flip, v = min(marker[i] ^ flip, m);
    r[i] = v;
    mk[i] = m;
    open |= v < m;
  }
  open = __syncthreads_or(open);
  if (threadIdx.x == 0) stamp[blockIdx.x] = open ? 0 : -1;
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
  __shared__ int run;
  if (threadIdx.x == 0) run = __hip_atomic_load(stamp + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= round;
  __syncthreads();
  if (!run) return;                               // uniform: one thread read the stamp
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * REC_TILE, x0 = tx * REC_TILE;
  int open = 0;
  for (int c = threadIdx.x; c < REC_LPX; c += CGC_BLOCK) {
    const int ly = c / REC_LW - 1, lx = c % REC_LW - 1;
    const int y = y0 + ly, x = x0 + lx;
    int v = REC_LOW, lim = REC_LOW;               // outside the image (and the padding word of a row): never rises, never raises
    if (lx <= REC_TILE && y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t i = (int64_t)y * W + x;
      // the halo belongs to tiles that may be storing right now; the tile's own values were last stored by an earlier launch
      const bool halo = ly < 0 || ly >= REC_TILE || lx < 0 || lx >= REC_TILE;
      if (halo) {
        v = __hip_atomic_load(rec + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        v = rec[i];
        lim = mk[i];
        open |= v < lim;
      }
    }
    r[c] = v;
    m[c] = lim;
  }
  if (!__syncthreads_or(open)) return;            // R equals the mask on the whole tile: nothing can rise

  for (;;) {
    int ch = rec_scan<true, CONN8>(r, m);
    __syncthreads();
    ch |= rec_scan<false, CONN8>(r, m);
    if (!__syncthreads_or(ch)) break;             // an iteration in which nothing moved read final values only: the tile's fixed point
  }

  int moved = 0;
  for (int j = 0; j < REC_SEG; ++j) {
    const int p = threadIdx.x + j * CGC_BLOCK;
    const int ly = p >> 6, lx = p & 63;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int64_t i = (int64_t)y * W + x;
    const int v = r[(ly + 1) * REC_LW + lx + 1];
    if (v != rec[i]) {                            // rec[i] is still what this tile loaded: nobody else stores into it
      __hip_atomic_store(rec + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      moved = 1;
    }
  }
  if (!__syncthreads_or(moved)) return;
  if (threadIdx.x < 9 && threadIdx.x != 4) {      // the eight neighbours read these values in the next round
    const int ny = ty + (int)threadIdx.x / 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
    if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
      __hip_atomic_store(stamp + ny * tiles_x + nx, round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 4 && changed != nullptr) atomicAdd(changed, 1);
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
  const int tiles_x = rec_tiles(W), tiles_y = rec_tiles(H);
  hipLaunchKernelGGL(k_rec_begin, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), marker, mask, by_erosion ? ~0 : 0, H, W,
                     tiles_x, w.r, w.mask, w.stamp);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_reconstruct_rounds(int H, int W, int connectivity, void* ws, int first_round, int rounds, int* changed,
                                      cgc_stream_t stream) {
  if (bad_image_dims(H, W)) return CGC_EINVAL;
  if ((connectivity != 1 && connectivity != 2) || first_round < 0 || rounds < 1 || first_round > 0x7fffffff - rounds - 1) return CGC_EINVAL;
  if (changed == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  {
    const hipError_t e = hipMemsetAsync(changed, 0, 4, st);
    if (e != hipSuccess) return (int)e;
  }
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr) return CGC_EINVAL;
  const RecWs w = rec_layout(Carver(ws), H, W);
  const int tiles_x = rec_tiles(W), tiles_y = rec_tiles(H);
  for (int r = 0; r < rounds; ++r) {              // only the last round of the batch counts the tiles that moved
    int* count = r == rounds - 1 ? changed : nullptr;
    if (connectivity == 2)
      hipLaunchKernelGGL(k_rec_round<true>, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, st, w.r, w.mask, w.stamp, H, W, tiles_x, tiles_y,
                         first_round + r, count);
    else
      hipLaunchKernelGGL(k_rec_round<false>, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, st, w.r, w.mask, w.stamp, H, W, tiles_x, tiles_y,
                         first_round + r, count);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
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
