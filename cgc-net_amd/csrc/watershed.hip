// Seeded watershed flood of a 2-D int32 height image on gfx950: every pixel of a domain learns the level at which water rising from
// the seeds first wets it and the seed that wets it, with the cut between two seeds' basins on the pass (the neck) between them.
// Integers throughout, so every result is bit for bit.  The third relaxation of the family of geodesic.hip and reconstruct.hip, on
// the same schedule (tile_relax.hpp).  Contract item by item: cgc-net_amd/kernels.py KernelSpec.watershed_flood; launches, workspace and the
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
//   k_ws_round    round r, one workgroup per tile, on the schedule of tile_relax.hpp with the sweep of path_relax.hpp; a thread's
//                 16 heights sit in registers.  Seeds are never relaxed.
//   k_ws_parent   once, after convergence: ptr[p] = the neighbour q that minimises (ext_p(K[q]), K[q], q) over the allowed steps
//                 q -> p from reached pixels -- the first component's minimum is K[p], so the parent offers p its key; of those the
//                 earliest flooded wins, then the smallest index.  ext_p is strictly increasing, so K[parent] < K[p]: the pointers
//                 form a forest rooted at the seeds.  ptr[p] = p on seeds, -1 where not reached.
//   k_ws_jump     ptr[p] = ptr[ptr[p]] in place, 32-bit relaxed atomics: a value read while another thread replaces it is still an
//                 ancestor of p, so a stale read only jumps less far.  Counts the pixels that moved.  Every jump at least halves the
//                 depth of every pixel and the depth is below 2^31, so 31 jumps always suffice.
//   k_ws_finish   keys, roots -> level, source
// The convergence loop of the jumps is the caller's too (it reads the number of pixels that moved in the last jump of a batch).
//
// TERMINATION, clause (1) of tile_relax.hpp: every key ever stored is the key of a real path from a seed and keys only decrease (WHY
// RELAXATION IS EXACT above); halo keys are read and keys are stored as single 64-bit relaxed atomics.
#include <stdint.h>

#include "path_relax.hpp"

namespace {

typedef path_key ws_key;

constexpr ws_key WS_NONE = ~(ws_key)0;            // not reached; no key of a path equals it (len < 2^31)
constexpr ws_key WS_SEED = 0;                     // (INT32_MIN, 0); a non-seed key has a higher alt or a positive len

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
  w.stamp = c.take<int>((int64_t)relax_tiles(H) * relax_tiles(W));
  return w;
}

__device__ __forceinline__ unsigned ws_bias(int h) { return (unsigned)h ^ 0x80000000u; }      // int32 order -> unsigned order

// ext_p of the key kq (reached) for a pixel of biased height hb and a step of cost w.  len + w stays below 2^31 (the size limit).
__device__ __forceinline__ ws_key ws_extend(ws_key kq, unsigned hb, unsigned w) {
  return hb > (unsigned)(kq >> 32) ? (ws_key)hb << 32 : kq + w;
}

// (a) keys, domain, heights, stamps
__global__ void __launch_bounds__(CGC_BLOCK) k_ws_begin(const int* __restrict__ height, const void* __restrict__ seeds, int seed_bytes,
                                                        const void* __restrict__ within, int within_bytes, int H, int W, int tiles_x,
                                                        ws_key* __restrict__ key, unsigned char* __restrict__ dom,
                                                        int* __restrict__ hcopy, int* __restrict__ stamp) {
  relax_begin_tile(H, W, tiles_x, stamp, [&](int64_t i) {
    bool in;
    key[i] = path_begin_pixel(seeds, seed_bytes, within, within_bytes, i, dom, in) ? WS_SEED : WS_NONE;
    hcopy[i] = height[i];
    return in;
  });
}

// A thread's 16 pixels are fixed and their heights never change: registers.
struct WsRule {
  static constexpr ws_key NONE = WS_NONE;
  const int* __restrict__ height;
  unsigned axial, diagonal;
  unsigned hb[RELAX_PER_THREAD];
  __device__ __forceinline__ bool setup(int j, ws_key kc, int64_t i) {
    const bool live = kc != WS_SEED;
    hb[j] = live ? ws_bias(height[i]) : 0;
    return live;
  }
  __device__ __forceinline__ ws_key extend(ws_key kq, unsigned w, int j) const { return ws_extend(kq, hb[j], w); }
};

// (b) one round
__global__ void __launch_bounds__(CGC_BLOCK) k_ws_round(ws_key* __restrict__ key, const unsigned char* __restrict__ dom,
                                                        const int* __restrict__ height, int* __restrict__ stamp, int H, int W,
                                                        int tiles_x, int tiles_y, unsigned a, unsigned b, int conn8, int round,
                                                        int* __restrict__ changed) {
  path_relax_round(WsRule{height, a, b, {}}, key, dom, stamp, H, W, tiles_x, tiles_y, conn8, round, changed);
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
  if (b != 0) {                                   // the corner rule of path_relax.hpp
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
  const int tiles_x = relax_tiles(W), tiles_y = relax_tiles(H);
  hipLaunchKernelGGL(k_ws_begin, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), height, seeds, seed_bytes, within,
                     within_bytes, H, W, tiles_x, w.key, w.dom, w.height, w.stamp);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_watershed_rounds(int H, int W, int a, int b, int connectivity, void* ws, int first_round, int rounds, int* changed,
                                    cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b) || bad_connectivity(connectivity)) return CGC_EINVAL;
  const WsWs w = ws_layout(Carver(ws), H, W);
  const int tiles_x = relax_tiles(W), tiles_y = relax_tiles(H);
  return relax_batch(H, W, ws, first_round, rounds, changed, stream, [&](int round, int* count) {
    hipLaunchKernelGGL(k_ws_round, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), w.key, w.dom, w.height, w.stamp, H, W,
                       tiles_x, tiles_y, (unsigned)a, (unsigned)b, connectivity == 2 ? 1 : 0, round, count);
  });
}

extern "C" int cgc_watershed_parents(int H, int W, int a, int b, int connectivity, void* ws, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b) || bad_connectivity(connectivity)) return CGC_EINVAL;
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
  if (bad_image_dims(H, W)) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const WsWs w = ws_layout(Carver(ws), H, W);
  return relax_batch(H, W, ws, 0, jumps, changed, stream, [&](int, int* count) {      // counts the pixels that moved
    hipLaunchKernelGGL(k_ws_jump, dim3((unsigned)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), w.ptr, npix, count);
  });
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
