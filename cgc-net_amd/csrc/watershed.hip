// Seeded watershed flood of a 2-D int32 height image on gfx950: every pixel of a domain learns the level at which water rising from
// the seeds first wets it and the seed that wets it, with the cut between two seeds' basins on the pass (the neck) between them.
// Integers throughout, so every result is bit for bit.  The third relaxation of the family of geodesic.hip and reconstruct.hip, whose
// driver pattern it shares.  Contract item by item: cgc-net_amd/kernels.py KernelSpec.watershed_flood; launches, workspace and the
// worst case: DESIGN.md, "Seeded watershed".
//
// key[p] = (alt ^ 0x80000000) << 32 | len, one 64-bit word per pixel, compared as unsigned: the flood key (alt, len) in lexicographic
// order.  0 = a seed, (INT32_MIN, 0); all ones = "not reached".  Extending a path with key (alt, len) by a step of cost w onto the
// non-seed pixel p gives  ext_p(alt, len) = (height[p], 0) if height[p] > alt  (the water rises onto p), else (alt, len + w)  (it runs
// level or downhill; len is the way travelled since the last rise).  K[p] = the smallest key over all paths from any seed.
// WHY RELAXATION IS EXACT.  ext_p is order-preserving (k <= k' implies ext_p(k) <= ext_p(k')) and strictly increasing (ext_p(k) > k:
// either alt rises or len grows by w >= 1), so K is the unique fixed point of  K[p] = min over the allowed steps q -> p of
// ext_p(K[q])  with K = 0 on seeds: every key ever stored is the key of a real path, hence >= K[p]; and at a fixed point, walking an
// optimal path from its seed, order preservation gives key[p] <= K[p] pixel by pixel.  Keys start at "not reached" and only ever
// decrease, so the order in which updates arrive does not matter.  Launches:
//   k_ws_begin    one workgroup per 64 x 64 tile: key 0 on seeds, "not reached" elsewhere; the domain as one byte per pixel; a copy
//                 of the heights; stamp[tile] = 0 when the tile holds a domain pixel, else -1
//   k_ws_round    round r, one workgroup per tile, k_geo_round's schedule.  A tile runs when stamp[tile] >= r: it loads its keys, its
//                 domain bytes and a one-pixel halo of both into LDS and its threads' 16 heights each into registers, relaxes there
//                 until nothing in the tile moves, writes the moved keys back and, if any moved, sets stamp = r + 1 on its eight
//                 neighbours.  Seeds are never relaxed.  An idle tile costs one load.
//   k_ws_parent   once, after convergence: ptr[p] = the neighbour q that minimises (ext_p(K[q]), K[q], q) over the allowed steps
//                 q -> p from reached pixels -- the first component's minimum is K[p], so the parent offers p its key; of those the
//                 earliest flooded wins, then the smallest index.  ext_p is strictly increasing, so K[parent] < K[p]: the pointers
//                 form a forest rooted at the seeds.  ptr[p] = p on seeds, -1 where not reached.
//   k_ws_jump     ptr[p] = ptr[ptr[p]] in place, 32-bit relaxed atomics: a value read while another thread replaces it is still an
//                 ancestor of p, so a stale read only jumps less far.  Counts the pixels that moved.  Every jump at least halves the
//                 depth of every pixel and the depth is below 2^31, so 31 jumps always suffice.
//   k_ws_finish   keys, roots -> level, source
// No workgroup ever waits for another one: the only ordering is the launch boundary, and both convergence loops are the caller's (it
// reads the number of tiles, or pixels, that moved in the last launch of a batch).
//
// TERMINATION.  Within a round a tile may read a neighbour's halo keys stale or fresh (see `VISIBILITY` in label.hip: L1s and the per-XCD
// L2s are not coherent within a launch).  That is harmless because (1) every key ever stored is the key of a real path from a seed
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

typedef unsigned long long ws_key;

constexpr int WS_TILE = 64;                       // tile edge: 4096 pixels, 16 per thread
constexpr int WS_PER_THREAD = WS_TILE * WS_TILE / CGC_BLOCK;
constexpr int WS_LW = WS_TILE + 2;                // LDS row: the tile plus a one-pixel halo; 66 * 66 * (8 + 1) bytes = 39204 in all
constexpr int WS_LPX = WS_LW * WS_LW;
constexpr ws_key WS_NONE = ~(ws_key)0;            // not reached; no key of a path equals it (len < 2^31)
constexpr ws_key WS_SEED = 0;                     // (INT32_MIN, 0); a non-seed key has a higher alt or a positive len
static_assert(WS_TILE == 64 && CGC_BLOCK == 256 && WS_PER_THREAD == 16, "a thread owns one column position of 16 rows of the tile");

static inline int ws_tiles(int n) { return ceil_div(n, WS_TILE); }

struct WsWs {
  ws_key* key;           // [H*W]
  unsigned char* dom;    // [H*W] 1 = in the domain
  int* height;           // [H*W]
  int* ptr;              // [H*W] parent, then root
  int* stamp;            // [tiles] the last round the tile has been asked to run in
};
static inline WsWs ws_layout(Carver&& c, int H, int W) {      // the one definition of the workspace
  WsWs w;
  w.key = c.take<ws_key>((int64_t)H * W);
  w.dom = c.take<unsigned char>((int64_t)H * W);
  w.height = c.take<int>((int64_t)H * W);
  w.ptr = c.take<int>((int64_t)H * W);
  w.stamp = c.take<int>((int64_t)ws_tiles(H) * ws_tiles(W));
  return w;
}

__device__ __forceinline__ unsigned ws_bias(int h) { return (unsigned)h ^ 0x80000000u; }      // int32 order -> unsigned order

// ext_p of the key kq (reached) for a pixel of biased height hb and a step of cost w.  len + w stays below 2^31 (the size limit).
__device__ __forceinline__ ws_key ws_extend(ws_key kq, unsigned hb, unsigned w) {
  return hb > (unsigned)(kq >> 32) ? (ws_key)hb << 32 : kq + w;
}

// (a) keys, domain, heights, stamps.  Consecutive threads take consecutive pixels of a tile row.
__global__ void __launch_bounds__(CGC_BLOCK) k_ws_begin(const int* __restrict__ height, const void* __restrict__ seeds, int seed_bytes,
                                                        const void* __restrict__ within, int within_bytes, int H, int W, int tiles_x,
                                                        ws_key* __restrict__ key, unsigned char* __restrict__ dom,
                                                        int* __restrict__ hcopy, int* __restrict__ stamp) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * WS_TILE, x0 = tx * WS_TILE;
  int any = 0;
  for (int j = 0; j < WS_PER_THREAD; ++j) {
    const int p = threadIdx.x + j * CGC_BLOCK;
    const int y = y0 + (p >> 6), x = x0 + (p & 63);
    if (y >= H || x >= W) continue;
    const int64_t i = (int64_t)y * W + x;
    const bool seed = image_nonzero(seeds, seed_bytes, i);
    const bool in = seed || within == nullptr || image_nonzero(within, within_bytes, i);
    key[i] = seed ? WS_SEED : WS_NONE;
    dom[i] = in ? 1 : 0;
    hcopy[i] = height[i];
    any |= in ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) stamp[blockIdx.x] = any ? 0 : -1;
}

__device__ __forceinline__ ws_key lds_key(const ws_key* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// One candidate: the step of cost w from LDS cell q into the pixel of biased height hb whose best key so far is `best`.
__device__ __forceinline__ ws_key ws_try(const ws_key* k, int q, unsigned w, unsigned hb, ws_key best) {
  const ws_key kq = lds_key(k + q);
  if (kq == WS_NONE) return best;
  const ws_key cand = ws_extend(kq, hb, w);
  return cand < best ? cand : best;
}

// (b) one round
__global__ void __launch_bounds__(CGC_BLOCK) k_ws_round(ws_key* __restrict__ key, const unsigned char* __restrict__ dom,
                                                        const int* __restrict__ height, int* __restrict__ stamp, int H, int W,
                                                        int tiles_x, int tiles_y, unsigned a, unsigned b, int conn8, int round,
                                                        int* __restrict__ changed) {
  __shared__ ws_key k[WS_LPX];
  __shared__ unsigned char d[WS_LPX];
  __shared__ int run;
  if (threadIdx.x == 0) run = __hip_atomic_load(stamp + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= round;
  __syncthreads();
  if (!run) return;                               // uniform: one thread read the stamp
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * WS_TILE, x0 = tx * WS_TILE;
  int reached = 0;
  for (int c = threadIdx.x; c < WS_LPX; c += CGC_BLOCK) {
    const int ly = c / WS_LW - 1, lx = c % WS_LW - 1;
    const int y = y0 + ly, x = x0 + lx;
    ws_key v = WS_NONE;
    unsigned char in = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t i = (int64_t)y * W + x;
      in = dom[i];
      // the halo belongs to tiles that may be storing right now; the tile's own keys were last stored by an earlier launch
      const bool halo = ly < 0 || ly >= WS_TILE || lx < 0 || lx >= WS_TILE;
      if (in) v = halo ? __hip_atomic_load(key + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : key[i];
    }
    k[c] = v;
    d[c] = in;
    reached |= v != WS_NONE;
  }
  if (!__syncthreads_or(reached)) return;         // no seed has reached the tile or its halo yet: nothing can move

  // this thread's 16 pixels: column threadIdx.x & 63 of rows (threadIdx.x >> 6) + 4 j.  Their heights never change: registers.
  const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
  unsigned hb[WS_PER_THREAD];
  unsigned live = 0;                              // bit j: the j-th pixel is a domain pixel that is no seed -- the ones to relax
#pragma unroll
  for (int j = 0; j < WS_PER_THREAD; ++j) {
    const int ly = ly0 + 4 * j;
    const int c = (ly + 1) * WS_LW + lx + 1;
    hb[j] = 0;
    if (d[c] && k[c] != WS_SEED) {                // a domain pixel lies inside the image
      hb[j] = ws_bias(height[(int64_t)(y0 + ly) * W + x0 + lx]);
      live |= 1u << j;
    }
  }

  unsigned moved = 0;                             // bit j: this thread's j-th pixel moved
  for (;;) {
    int ch = 0;
#pragma unroll
    for (int j = 0; j < WS_PER_THREAD; ++j) {
      if (!(live >> j & 1u)) continue;
      const int c = (ly0 + 4 * j + 1) * WS_LW + lx + 1;
      const ws_key cur = lds_key(k + c);          // only this thread ever writes k[c]
      ws_key best = cur;
      best = ws_try(k, c - WS_LW, a, hb[j], best);
      best = ws_try(k, c - 1, a, hb[j], best);
      best = ws_try(k, c + 1, a, hb[j], best);
      best = ws_try(k, c + WS_LW, a, hb[j], best);
      if (b != 0) {
        // connectivity 1: a diagonal step needs one of the two pixels it passes between in the domain (no squeezing through a corner)
        const bool up = conn8 || d[c - WS_LW], down = conn8 || d[c + WS_LW], left = d[c - 1], right = d[c + 1];
        if (up || left) best = ws_try(k, c - WS_LW - 1, b, hb[j], best);
        if (up || right) best = ws_try(k, c - WS_LW + 1, b, hb[j], best);
        if (down || left) best = ws_try(k, c + WS_LW - 1, b, hb[j], best);
        if (down || right) best = ws_try(k, c + WS_LW + 1, b, hb[j], best);
      }
      if (best < cur) {
        __hip_atomic_store(k + c, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ch = 1;
        moved |= 1u << j;
      }
    }
    if (!__syncthreads_or(ch)) break;             // a sweep in which nothing moved read final values only: the tile's fixed point
  }

#pragma unroll
  for (int j = 0; j < WS_PER_THREAD; ++j) {
    if (!(moved >> j & 1u)) continue;
    const int ly = ly0 + 4 * j;                   // a moved pixel is in the domain, hence inside the image
    __hip_atomic_store(key + (int64_t)(y0 + ly) * W + x0 + lx, k[(ly + 1) * WS_LW + lx + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!__syncthreads_or(moved != 0)) return;
  if (threadIdx.x < 9 && threadIdx.x != 4) {      // the eight neighbours read these keys in the next round
    const int ny = ty + (int)threadIdx.x / 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
    if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
      __hip_atomic_store(stamp + ny * tiles_x + nx, round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 4 && changed != nullptr) atomicAdd(changed, 1);
}

// (c) parents from the final keys.  One thread per pixel; the eight neighbours' keys and domain bytes come through the caches.
// The best offer so far is (ext, from, q) = (ext_p(K[q]), K[q], q), compared lexicographically.  The comparison is written without
// branches, as one predicate and three selects under it: the short-circuit form compiled (ROCm 7, -O3) to code that took ext and
// from of a tying offer but kept the old q.
struct WsOffer {
  ws_key ext, from;
  int q;
};
__device__ __forceinline__ void ws_offer(const ws_key* __restrict__ key, int64_t q, unsigned w, unsigned hb, WsOffer& best) {
  const ws_key kq = key[q];
  const ws_key e = ws_extend(kq, hb, w);
  const bool take = (kq != WS_NONE) &
                    ((e < best.ext) | ((e == best.ext) & ((kq < best.from) | ((kq == best.from) & ((int)q < best.q)))));
  best.ext = take ? e : best.ext;
  best.from = take ? kq : best.from;
  best.q = take ? (int)q : best.q;
}

__global__ void __launch_bounds__(CGC_BLOCK) k_ws_parent(const ws_key* __restrict__ key, const unsigned char* __restrict__ dom,
                                                         const int* __restrict__ height, int H, int W, unsigned a, unsigned b, int conn8,
                                                         int* __restrict__ ptr) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const ws_key kp = key[i];
  if (kp == WS_NONE || kp == WS_SEED) {
    ptr[i] = kp == WS_SEED ? (int)i : -1;
    return;
  }
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const unsigned hb = ws_bias(height[i]);
  const bool iu = y > 0, id = y + 1 < H, il = x > 0, ir = x + 1 < W;      // inside the image
  const bool up = iu && dom[i - W], down = id && dom[i + W], left = il && dom[i - 1], right = ir && dom[i + 1];
  WsOffer best = {WS_NONE, WS_NONE, -1};
  if (up) ws_offer(key, i - W, a, hb, best);
  if (left) ws_offer(key, i - 1, a, hb, best);
  if (right) ws_offer(key, i + 1, a, hb, best);
  if (down) ws_offer(key, i + W, a, hb, best);
  if (b != 0) {                                   // the corner rule of k_ws_round
    if (iu && il && dom[i - W - 1] && (conn8 || up || left)) ws_offer(key, i - W - 1, b, hb, best);
    if (iu && ir && dom[i - W + 1] && (conn8 || up || right)) ws_offer(key, i - W + 1, b, hb, best);
    if (id && il && dom[i + W - 1] && (conn8 || down || left)) ws_offer(key, i + W - 1, b, hb, best);
    if (id && ir && dom[i + W + 1] && (conn8 || down || right)) ws_offer(key, i + W + 1, b, hb, best);
  }
  ptr[i] = best.q;                                // a reached pixel has a reached neighbour that offers it its key
}

// (d) one pointer jump, in place
__global__ void __launch_bounds__(CGC_BLOCK) k_ws_jump(int* __restrict__ ptr, int64_t npix, int* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  int moved = 0;
  if (i < npix) {
    const int q = __hip_atomic_load(ptr + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q >= 0 && q != (int)i) {                  // q: an ancestor of i, so reached, so ptr[q] >= 0
      const int r = __hip_atomic_load(ptr + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r != q) {
        __hip_atomic_store(ptr + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        moved = 1;
      }
    }
  }
  if (changed == nullptr) return;                 // uniform
  const int n = __syncthreads_count(moved);
  if (threadIdx.x == 0 && n != 0) atomicAdd(changed, n);
}

// (e) keys, roots -> outputs
__global__ void __launch_bounds__(CGC_BLOCK) k_ws_finish(const ws_key* __restrict__ key, const int* __restrict__ height,
                                                         const int* __restrict__ ptr, int64_t npix, int* __restrict__ level,
                                                         int* __restrict__ source) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= npix) return;
  const ws_key v = key[i];
  level[i] = (v == WS_NONE || v == WS_SEED) ? height[i] : (int)ws_bias((int)(unsigned)(v >> 32));
  source[i] = v == WS_NONE ? -1 : ptr[i];
}

static inline bool ws_bad_connectivity(int connectivity) { return connectivity != 1 && connectivity != 2; }

}  // namespace

extern "C" int64_t cgc_watershed_ws_bytes(int H, int W) {
  if (bad_image_dims(H, W)) return 0;
  return layout_bytes(ws_layout, H, W);
}

extern "C" int cgc_watershed_begin(const int* height, const void* seeds, int seed_bytes, const void* within, int within_bytes, int H, int W,
                                   int a, int b, void* ws, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b)) return CGC_EINVAL;
  if (bad_elem_bytes(seed_bytes) || (within != nullptr && bad_elem_bytes(within_bytes))) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (height == nullptr || seeds == nullptr || ws == nullptr) return CGC_EINVAL;
  const WsWs w = ws_layout(Carver(ws), H, W);
  const int tiles_x = ws_tiles(W), tiles_y = ws_tiles(H);
  hipLaunchKernelGGL(k_ws_begin, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), height, seeds, seed_bytes, within,
                     within_bytes, H, W, tiles_x, w.key, w.dom, w.height, w.stamp);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_watershed_rounds(int H, int W, int a, int b, int connectivity, void* ws, int first_round, int rounds, int* changed,
                                    cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b)) return CGC_EINVAL;
  if (ws_bad_connectivity(connectivity) || first_round < 0 || rounds < 1 || first_round > 0x7fffffff - rounds - 1) return CGC_EINVAL;
  if (changed == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  {
    const hipError_t e = hipMemsetAsync(changed, 0, 4, st);
    if (e != hipSuccess) return (int)e;
  }
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr) return CGC_EINVAL;
  const WsWs w = ws_layout(Carver(ws), H, W);
  const int tiles_x = ws_tiles(W), tiles_y = ws_tiles(H);
  for (int r = 0; r < rounds; ++r) {              // only the last round of the batch counts the tiles that moved
    hipLaunchKernelGGL(k_ws_round, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, st, w.key, w.dom, w.height, w.stamp, H, W, tiles_x, tiles_y,
                       (unsigned)a, (unsigned)b, connectivity == 2 ? 1 : 0, first_round + r, r == rounds - 1 ? changed : nullptr);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_watershed_parents(int H, int W, int a, int b, int connectivity, void* ws, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b) || ws_bad_connectivity(connectivity)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const WsWs w = ws_layout(Carver(ws), H, W);
  hipLaunchKernelGGL(k_ws_parent, dim3((unsigned)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), w.key, w.dom, w.height,
                     H, W, (unsigned)a, (unsigned)b, connectivity == 2 ? 1 : 0, w.ptr);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_watershed_jumps(int H, int W, void* ws, int jumps, int* changed, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || jumps < 1 || changed == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  {
    const hipError_t e = hipMemsetAsync(changed, 0, 4, st);
    if (e != hipSuccess) return (int)e;
  }
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const WsWs w = ws_layout(Carver(ws), H, W);
  for (int j = 0; j < jumps; ++j) {               // only the last jump of the batch counts the pixels that moved
    hipLaunchKernelGGL(k_ws_jump, dim3((unsigned)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, st, w.ptr, npix,
                       j == jumps - 1 ? changed : nullptr);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_watershed_finish(int H, int W, const void* ws, int* level, int* source, cgc_stream_t stream) {
  if (bad_image_dims(H, W)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (ws == nullptr || level == nullptr || source == nullptr) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const WsWs w = ws_layout(Carver(const_cast<void*>(ws)), H, W);
  hipLaunchKernelGGL(k_ws_finish, dim3((unsigned)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), w.key, w.height, w.ptr,
                     npix, level, source);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
