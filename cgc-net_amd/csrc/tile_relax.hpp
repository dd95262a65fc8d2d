// The schedule that geodesic.hip, reconstruct.hip and watershed.hip share: a monotone relaxation of one value per pixel to its fixed
// point, one 256-thread workgroup per 64 x 64 tile and one launch per round.  A stage supplies what a value is, how a tile relaxes to
// its own fixed point in LDS, and clause (1) below; the run decision, the halo load, the write-back, the stamps and the host's batch
// of launches are here, once.
//
// stamp[tile] = the last round the tile has been asked to run in (-1: never).  Round r: a tile runs when stamp[tile] >= r.  It loads
// its values and a one-pixel halo into LDS, relaxes there until nothing in the tile moves, stores the values that moved and, if any
// did, sets stamp = r + 1 on its eight neighbours.  An idle tile costs one load.  No workgroup ever waits for another one: the only
// ordering is the launch boundary, and the convergence loop is the caller's (it reads the number of tiles that moved in the last
// round of a batch of rounds).
//
// VISIBILITY / TERMINATION.  Within a round a tile may read a neighbour's halo values stale or fresh (see `VISIBILITY` in label.hip:
// L1s and the per-XCD L2s are not coherent within a launch).  That is harmless because (1) -- the stage's clause, in its own file --
// values are monotone and every value ever stored is the value of a real path, so a stale value is only a weaker bound, never a wrong
// one, and halo values are read and values are stored as single relaxed agent-scope atomics of the value's width, so a value is never
// torn; (2) a tile whose values moved in round r stamps its neighbours for round r + 1, where they read what round r stored -- an
// earlier launch; (3) the caller stops only after a round in which no tile stored anything: every value read in that round was
// written by an earlier launch, every tile that ran is at its fixed point with respect to the current values, and a tile that did not
// run has been at its fixed point since its last run, because nothing in it or around it moved since (or it would have been stamped).
// All tiles at their fixed point is the stage's global fixed point.  A stamp is read while neighbours may be raising it to r + 1: both
// r and r + 1 mean "run" in round r, and one thread reads it for the whole workgroup, so the decision is uniform.
#pragma once
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

constexpr int RELAX_TILE = 64;                    // tile edge: 4096 pixels, 16 per thread
constexpr int RELAX_PER_THREAD = RELAX_TILE * RELAX_TILE / CGC_BLOCK;
static_assert(RELAX_TILE == 64 && CGC_BLOCK == 256 && RELAX_PER_THREAD == 16,
              "a wave holds the 64 columns (or lines) of a tile, a workgroup its four quarters: 16 pixels per thread");

static inline int relax_tiles(int n) { return ceil_div(n, RELAX_TILE); }

struct RelaxTile {
  int ty, tx;            // the tile of this workgroup
  int y0, x0;            // its first pixel
};
__device__ __forceinline__ RelaxTile relax_tile(int tiles_x) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  return {ty, tx, ty * RELAX_TILE, tx * RELAX_TILE};
}

// The j-th pixel of this thread, row and column within the tile: consecutive threads take consecutive pixels of a tile row, so a
// thread owns one column position of 16 rows.
__device__ __forceinline__ int relax_ly(int j) { return (int)(threadIdx.x >> 6) + 4 * j; }
__device__ __forceinline__ int relax_lx() { return (int)(threadIdx.x & 63); }

// A begin kernel: init(i) sets up pixel i of the workspace and returns whether it can ever move; a tile without such a pixel never runs.
template <class Init>
__device__ __forceinline__ void relax_begin_tile(int H, int W, int tiles_x, int* __restrict__ stamp, Init init) {
  const RelaxTile t = relax_tile(tiles_x);
  int any = 0;
  for (int j = 0; j < RELAX_PER_THREAD; ++j) {
    const int y = t.y0 + relax_ly(j), x = t.x0 + relax_lx();
    if (y >= H || x >= W) continue;
    any |= init((int64_t)y * W + x) ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) stamp[blockIdx.x] = any ? 0 : -1;
}

// Whether this tile runs in `round`.  Uniform: one thread reads the stamp.
__device__ __forceinline__ bool relax_tile_runs(const int* stamp, int round) {
  __shared__ int run;
  if (threadIdx.x == 0) run = __hip_atomic_load(stamp + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= round;
  __syncthreads();
  return run;
}

// One cell of the tile-plus-halo square, as the loader hands it to a stage.
template <typename T>
struct RelaxCell {
  const T* g;
  int64_t i;             // the pixel's raster index
  bool inside, halo;     // inside the image; outside the tile
  // The halo belongs to tiles that may be storing right now; the tile's own values were last stored by an earlier launch.
  __device__ __forceinline__ T load() const { return halo ? __hip_atomic_load(g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : g[i]; }
};

// Walks the (RELAX_TILE + 2) rows of LW cells of the LDS image of a tile: the tile, its one-pixel halo and, where LW > RELAX_TILE + 2,
// padding (never inside).  cell(c, RelaxCell) fills LDS cell c and returns whether something there can move; returns the OR over the tile.
template <typename T, int LW, class Cell>
__device__ __forceinline__ bool relax_load_halo(const T* g, int H, int W, const RelaxTile& t, Cell cell) {
  int any = 0;
  for (int c = threadIdx.x; c < (RELAX_TILE + 2) * LW; c += CGC_BLOCK) {
    const int ly = c / LW - 1, lx = c % LW - 1;
    const int y = t.y0 + ly, x = t.x0 + lx;
    RelaxCell<T> rc = {g, (int64_t)y * W + x, lx <= RELAX_TILE && y >= 0 && y < H && x >= 0 && x < W,
                       ly < 0 || ly >= RELAX_TILE || lx < 0 || lx >= RELAX_TILE};
    any |= cell(c, rc) ? 1 : 0;
  }
  return __syncthreads_or(any);
}

// Stores those of this thread's 16 pixels for which moved(j, i, v) holds (v: the LDS cell, read only if used); returns whether any was.
template <typename T, int LW, class Moved>
__device__ __forceinline__ int relax_write_back(T* g, const T* lds, int H, int W, const RelaxTile& t, Moved moved) {
  int any = 0;
#pragma unroll
  for (int j = 0; j < RELAX_PER_THREAD; ++j) {
    const int ly = relax_ly(j), lx = relax_lx();
    if (t.y0 + ly >= H || t.x0 + lx >= W) continue;
    const int64_t i = (int64_t)(t.y0 + ly) * W + t.x0 + lx;
    const T& v = lds[(ly + 1) * LW + lx + 1];
    if (moved(j, i, v)) {
      __hip_atomic_store(g + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      any = 1;
    }
  }
  return any;
}

// After the write-back: if a value of the tile moved, the eight neighbours read it in the next round, and the tile counts.
__device__ __forceinline__ void relax_publish(int moved, const RelaxTile& t, int tiles_x, int tiles_y, int* __restrict__ stamp, int round,
                                              int* __restrict__ changed) {
  if (!__syncthreads_or(moved)) return;
  if (threadIdx.x < 9 && threadIdx.x != 4) {
    const int ny = t.ty + (int)threadIdx.x / 3 - 1, nx = t.tx + (int)threadIdx.x % 3 - 1;
    if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
      __hip_atomic_store(stamp + ny * tiles_x + nx, round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 4 && changed != nullptr) atomicAdd(changed, 1);
}

// Host: launches first .. first + count - 1 of a stage whose caller reads `changed` after the batch.  The stage has checked its own
// arguments; one(index, counter) enqueues one launch.  Only the last launch of the batch gets the counter.
template <class Launch>
int relax_batch(int H, int W, const void* ws, int first, int count, int* changed, cgc_stream_t stream, Launch one) {
  if (bad_launch_range(first, count) || changed == nullptr) return CGC_EINVAL;
  const hipError_t e = hipMemsetAsync(changed, 0, 4, as_stream(stream));
  if (e != hipSuccess) return (int)e;
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr) return CGC_EINVAL;
  for (int r = 0; r < count; ++r) {
    one(first + r, r == count - 1 ? changed : nullptr);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}
