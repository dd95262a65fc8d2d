// Geodesic distance transform of a 2-D image on gfx950 with the nearest seed of every pixel: the smallest cost of a path of axial (cost a)
// and diagonal (cost b) steps that stays inside a domain, integers throughout, so every result is bit for bit.  The geodesic counterpart
// of edt.hip.  Contract item by item: cgc-net_amd/kernels.py KernelSpec.geodesic_transform; launches, workspace and the worst case:
// DESIGN.md, "Geodesic growth".
//
// key[p] = cost << 32 | seed index, one 64-bit word per pixel; (GEO_INF, 0xffffffff) = "not reached".  The answer is the unique fixed
// point of  key[p] = min(key0[p], min over the allowed steps q -> p of key[q] + (cost << 32))  -- the predecessor of p on a shortest
// path from the winning seed carries that same seed (another one there would tie at p with a smaller index or beat it), costs are
// positive, and keys only ever decrease, so the order in which updates arrive does not matter.  Launches:
//   k_geo_begin   one workgroup per 64 x 64 tile: keys (0, own index) on seeds, "not reached" elsewhere; the domain as one byte per
//                 pixel; stamp[tile] = 0 when the tile holds a domain pixel, else -1
//   k_geo_round   round r, one workgroup per tile.  A tile runs when stamp[tile] >= r: it loads its keys, its domain bytes and a
//                 one-pixel halo of both into LDS, relaxes there until nothing in the tile moves, writes the moved keys back and, if any
//                 moved, sets stamp = r + 1 on its eight neighbours.  An idle tile costs one load.
//   k_geo_finish  keys -> dist, nearest
// No workgroup ever waits for another one: the only ordering is the launch boundary, and the convergence loop is the caller's (it reads
// the number of tiles that moved in the last round of a batch of rounds).
//
// TERMINATION.  Within a round a tile may read a neighbour's halo keys stale or fresh (see `VISIBILITY` in label.hip: L1s and the per-XCD
// L2s are not coherent within a launch).  That is harmless because (1) every key ever stored is the cost of a real path from its seed
// and keys are monotone, so a stale value is only a weaker bound, never a wrong one, and halo keys are read and keys are stored as
// single 64-bit relaxed atomics, so a value is never torn; (2) a tile whose keys moved in round r stamps its neighbours for round
// r + 1, where they read what round r stored -- an earlier launch; (3) the caller stops only after a round in which no tile stored
// anything: every value read in that round was written by an earlier launch, every tile that ran is at its fixed point with respect to
// the current keys, and a tile that did not run has been at its fixed point since its last run, because nothing in it or around it
// moved since (or it would have been stamped).  All tiles at their fixed point is the fixed point above.  A stamp is read while
// neighbours may be raising it to r + 1: both r and r + 1 mean "run" in round r, and one thread reads it for the whole workgroup.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

typedef unsigned long long geo_key;

constexpr int GEO_TILE = 64;                      // tile edge: 4096 pixels, 16 per thread
constexpr int GEO_PER_THREAD = GEO_TILE * GEO_TILE / CGC_BLOCK;
constexpr int GEO_LW = GEO_TILE + 2;              // LDS row: the tile plus a one-pixel halo; 66 * 66 * (8 + 1) bytes = 39204 in all
constexpr int GEO_LPX = GEO_LW * GEO_LW;
constexpr geo_key GEO_NONE = ((geo_key)CGC_GEO_INF << 32) | 0xffffffffull;
constexpr geo_key GEO_REACHED = (geo_key)CGC_GEO_INF << 32;      // a key below this one carries a seed

static inline int geo_tiles(int n) { return ceil_div(n, GEO_TILE); }

struct GeoWs {
  geo_key* key;          // [H*W]
  unsigned char* dom;    // [H*W] 1 = in the domain
  int* stamp;            // [tiles] the last round the tile has been asked to run in
};
static inline GeoWs geo_layout(Carver&& c, int H, int W) {      // the one definition of the workspace
  GeoWs w;
  w.key = c.take<geo_key>((int64_t)H * W);
  w.dom = c.take<unsigned char>((int64_t)H * W);
  w.stamp = c.take<int>((int64_t)geo_tiles(H) * geo_tiles(W));
  return w;
}

// (a) keys, domain, stamps.  Consecutive threads take consecutive pixels of a tile row.
__global__ void __launch_bounds__(CGC_BLOCK) k_geo_begin(const void* __restrict__ seeds, int seed_bytes, const void* __restrict__ within,
                                                         int within_bytes, int H, int W, int tiles_x, geo_key* __restrict__ key,
                                                         unsigned char* __restrict__ dom, int* __restrict__ stamp) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * GEO_TILE, x0 = tx * GEO_TILE;
  int any = 0;
  for (int j = 0; j < GEO_PER_THREAD; ++j) {
    const int p = threadIdx.x + j * CGC_BLOCK;
    const int y = y0 + (p >> 6), x = x0 + (p & 63);
    if (y >= H || x >= W) continue;
    const int64_t i = (int64_t)y * W + x;
    const bool seed = image_nonzero(seeds, seed_bytes, i);
    const bool in = seed || within == nullptr || image_nonzero(within, within_bytes, i);
    key[i] = seed ? (geo_key)(unsigned)i : GEO_NONE;
    dom[i] = in ? 1 : 0;
    any |= in ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) stamp[blockIdx.x] = any ? 0 : -1;
}

__device__ __forceinline__ geo_key lds_key(const geo_key* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// One candidate: the step from LDS cell q (cost << 32 = step) into the pixel whose best key so far is `best`.
__device__ __forceinline__ geo_key geo_try(const geo_key* k, int q, geo_key step, geo_key limit, geo_key best) {
  const geo_key kq = lds_key(k + q);
  if (kq >= GEO_REACHED) return best;
  const geo_key cand = kq + step;                 // cost below 2^31 (the size limit): the seed index in the low word is untouched
  return (cand < best && cand < limit) ? cand : best;
}

// (b) one round.  limit = (dmax + 1) << 32: candidates whose cost exceeds dmax are dropped, which loses nothing (every prefix of a
// path within the bound is within the bound).
__global__ void __launch_bounds__(CGC_BLOCK) k_geo_round(geo_key* __restrict__ key, const unsigned char* __restrict__ dom,
                                                         int* __restrict__ stamp, int H, int W, int tiles_x, int tiles_y, unsigned a,
                                                         unsigned b, int conn8, geo_key limit, int round, int* __restrict__ changed) {
  __shared__ geo_key k[GEO_LPX];
  __shared__ unsigned char d[GEO_LPX];
  __shared__ int run;
  if (threadIdx.x == 0) run = __hip_atomic_load(stamp + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= round;
  __syncthreads();
  if (!run) return;                               // uniform: one thread read the stamp
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * GEO_TILE, x0 = tx * GEO_TILE;
  int reached = 0;
  for (int c = threadIdx.x; c < GEO_LPX; c += CGC_BLOCK) {
    const int ly = c / GEO_LW - 1, lx = c % GEO_LW - 1;
    const int y = y0 + ly, x = x0 + lx;
    geo_key v = GEO_NONE;
    unsigned char in = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t i = (int64_t)y * W + x;
      in = dom[i];
      // the halo belongs to tiles that may be storing right now; the tile's own keys were last stored by an earlier launch
      const bool halo = ly < 0 || ly >= GEO_TILE || lx < 0 || lx >= GEO_TILE;
      if (in) v = halo ? __hip_atomic_load(key + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : key[i];
    }
    k[c] = v;
    d[c] = in;
    reached |= v < GEO_REACHED;
  }
  if (!__syncthreads_or(reached)) return;         // no seed has reached the tile or its halo yet: nothing can move

  const geo_key sa = (geo_key)a << 32, sb = (geo_key)b << 32;
  unsigned moved = 0;                             // bit j: this thread's j-th pixel moved
  for (;;) {
    int ch = 0;
    for (int j = 0; j < GEO_PER_THREAD; ++j) {
      const int p = threadIdx.x + j * CGC_BLOCK;
      const int c = ((p >> 6) + 1) * GEO_LW + (p & 63) + 1;
      if (!d[c]) continue;
      const geo_key cur = lds_key(k + c);         // only this thread ever writes k[c]
      geo_key best = cur;
      best = geo_try(k, c - GEO_LW, sa, limit, best);
      best = geo_try(k, c - 1, sa, limit, best);
      best = geo_try(k, c + 1, sa, limit, best);
      best = geo_try(k, c + GEO_LW, sa, limit, best);
      if (b != 0) {
        // connectivity 1: a diagonal step needs one of the two pixels it passes between in the domain (no squeezing through a corner)
        const bool up = conn8 || d[c - GEO_LW], down = conn8 || d[c + GEO_LW], left = d[c - 1], right = d[c + 1];
        if (up || left) best = geo_try(k, c - GEO_LW - 1, sb, limit, best);
        if (up || right) best = geo_try(k, c - GEO_LW + 1, sb, limit, best);
        if (down || left) best = geo_try(k, c + GEO_LW - 1, sb, limit, best);
        if (down || right) best = geo_try(k, c + GEO_LW + 1, sb, limit, best);
      }
      if (best < cur) {
        __hip_atomic_store(k + c, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ch = 1;
        moved |= 1u << j;
      }
    }
    if (!__syncthreads_or(ch)) break;             // a sweep in which nothing moved read final values only: the tile's fixed point
  }

  for (int j = 0; j < GEO_PER_THREAD; ++j) {
    if (!(moved >> j & 1u)) continue;
    const int p = threadIdx.x + j * CGC_BLOCK;
    const int ly = p >> 6, lx = p & 63;           // a moved pixel is in the domain, hence inside the image
    __hip_atomic_store(key + (int64_t)(y0 + ly) * W + x0 + lx, k[(ly + 1) * GEO_LW + lx + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!__syncthreads_or(moved != 0)) return;
  if (threadIdx.x < 9 && threadIdx.x != 4) {      // the eight neighbours read these keys in the next round
    const int ny = ty + (int)threadIdx.x / 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
    if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
      __hip_atomic_store(stamp + ny * tiles_x + nx, round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 4 && changed != nullptr) atomicAdd(changed, 1);
}

// (c) keys -> outputs
__global__ void __launch_bounds__(CGC_BLOCK) k_geo_finish(const geo_key* __restrict__ key, int64_t npix, int* __restrict__ dist,
                                                          int* __restrict__ nearest) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= npix) return;
  const geo_key v = key[i];
  const bool found = v < GEO_REACHED;
  dist[i] = found ? (int)(v >> 32) : CGC_GEO_INF;
  if (nearest != nullptr) nearest[i] = found ? (int)(unsigned)v : -1;
}

}  // namespace

extern "C" int64_t cgc_geodesic_ws_bytes(int H, int W) {
  if (bad_image_dims(H, W)) return 0;
  return layout_bytes(geo_layout, H, W);
}

extern "C" int cgc_geodesic_begin(const void* seeds, int seed_bytes, const void* within, int within_bytes, int H, int W, int a, int b,
                                  void* ws, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b)) return CGC_EINVAL;
  if (bad_elem_bytes(seed_bytes) || (within != nullptr && bad_elem_bytes(within_bytes))) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (seeds == nullptr || ws == nullptr) return CGC_EINVAL;
  const GeoWs w = geo_layout(Carver(ws), H, W);
  const int tiles_x = geo_tiles(W), tiles_y = geo_tiles(H);
  hipLaunchKernelGGL(k_geo_begin, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), seeds, seed_bytes, within, within_bytes,
                     H, W, tiles_x, w.key, w.dom, w.stamp);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_geodesic_rounds(int H, int W, int a, int b, int connectivity, int dmax, void* ws, int first_round, int rounds,
                                   int* changed, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b)) return CGC_EINVAL;
  if ((connectivity != 1 && connectivity != 2) || first_round < 0 || rounds < 1 || first_round > 0x7fffffff - rounds - 1) return CGC_EINVAL;
  if (changed == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  {
    const hipError_t e = hipMemsetAsync(changed, 0, 4, st);
    if (e != hipSuccess) return (int)e;
  }
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr) return CGC_EINVAL;
  const GeoWs w = geo_layout(Carver(ws), H, W);
  const int tiles_x = geo_tiles(W), tiles_y = geo_tiles(H);
  const geo_key limit = dmax < 0 ? GEO_REACHED : ((geo_key)(unsigned)dmax + 1) << 32;
  for (int r = 0; r < rounds; ++r) {              // only the last round of the batch counts the tiles that moved
    hipLaunchKernelGGL(k_geo_round, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, st, w.key, w.dom, w.stamp, H, W, tiles_x, tiles_y,
                       (unsigned)a, (unsigned)b, connectivity == 2 ? 1 : 0, limit, first_round + r, r == rounds - 1 ? changed : nullptr);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_geodesic_finish(int H, int W, const void* ws, int* dist, int* nearest, cgc_stream_t stream) {
  if (bad_image_dims(H, W)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr || dist == nullptr) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const GeoWs w = geo_layout(Carver(const_cast<void*>(ws)), H, W);
  hipLaunchKernelGGL(k_geo_finish, dim3((unsigned)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), w.key, npix, dist,
                     nearest);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
