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
//   k_geo_round   round r, one workgroup per tile, on the schedule of tile_relax.hpp with the sweep of path_relax.hpp
//   k_geo_finish  keys -> dist, nearest
//
// TERMINATION, clause (1) of tile_relax.hpp: every key ever stored is the cost of a real path from its seed and keys only decrease;
// halo keys are read and keys are stored as single 64-bit relaxed atomics.
#include <stdint.h>

#include "path_relax.hpp"

namespace {

typedef path_key geo_key;

constexpr geo_key GEO_NONE = ((geo_key)CGC_GEO_INF << 32) | 0xffffffffull;
constexpr geo_key GEO_REACHED = (geo_key)CGC_GEO_INF << 32;      // a key below this one carries a seed

struct GeoWs {
  geo_key* key;          // [H*W]
  unsigned char* dom;    // [H*W] 1 = in the domain
  int* stamp;            // [tiles] the last round the tile has been asked to run in
};
static inline GeoWs geo_layout(Carver&& c, int H, int W) {      // the one definition of the workspace
  GeoWs w;
  w.key = c.take<geo_key>((int64_t)H * W);
  w.dom = c.take<unsigned char>((int64_t)H * W);
  w.stamp = c.take<int>((int64_t)relax_tiles(H) * relax_tiles(W));
  return w;
}

// (a) keys, domain, stamps
__global__ void __launch_bounds__(CGC_BLOCK) k_geo_begin(const void* __restrict__ seeds, int seed_bytes, const void* __restrict__ within,
                                                         int within_bytes, int H, int W, int tiles_x, geo_key* __restrict__ key,
                                                         unsigned char* __restrict__ dom, int* __restrict__ stamp) {
  relax_begin_tile(H, W, tiles_x, stamp, [&](int64_t i) {
    bool in;
    key[i] = path_begin_pixel(seeds, seed_bytes, within, within_bytes, i, dom, in) ? (geo_key)(unsigned)i : GEO_NONE;
    return in;
  });
}

// Steps are cost << 32: the cost stays below 2^31 (the size limit), so the seed index in the low word is untouched.  limit =
// (dmax + 1) << 32: candidates whose cost exceeds dmax are dropped, which loses nothing (every prefix of a path within the bound is
// within the bound).
struct GeoRule {
  static constexpr geo_key NONE = GEO_NONE;
  geo_key axial, diagonal, limit;
  __device__ __forceinline__ bool setup(int, geo_key, int64_t) { return true; }
  __device__ __forceinline__ geo_key extend(geo_key kq, geo_key step, int) const { return kq + step < limit ? kq + step : PATH_NOTHING; }
};

// (b) one round
__global__ void __launch_bounds__(CGC_BLOCK) k_geo_round(geo_key* __restrict__ key, const unsigned char* __restrict__ dom,
                                                         int* __restrict__ stamp, int H, int W, int tiles_x, int tiles_y, unsigned a,
                                                         unsigned b, int conn8, geo_key limit, int round, int* __restrict__ changed) {
  path_relax_round(GeoRule{(geo_key)a << 32, (geo_key)b << 32, limit}, key, dom, stamp, H, W, tiles_x, tiles_y, conn8, round, changed);
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
  const int tiles_x = relax_tiles(W), tiles_y = relax_tiles(H);
  hipLaunchKernelGGL(k_geo_begin, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), seeds, seed_bytes, within, within_bytes,
                     H, W, tiles_x, w.key, w.dom, w.stamp);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_geodesic_rounds(int H, int W, int a, int b, int connectivity, int dmax, void* ws, int first_round, int rounds,
                                   int* changed, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || bad_step_costs(H, W, a, b) || bad_connectivity(connectivity)) return CGC_EINVAL;
  const GeoWs w = geo_layout(Carver(ws), H, W);
  const int tiles_x = relax_tiles(W), tiles_y = relax_tiles(H);
  const geo_key limit = dmax < 0 ? GEO_REACHED : ((geo_key)(unsigned)dmax + 1) << 32;
  return relax_batch(H, W, ws, first_round, rounds, changed, stream, [&](int round, int* count) {
    hipLaunchKernelGGL(k_geo_round, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, as_stream(stream), w.key, w.dom, w.stamp, H, W, tiles_x,
                       tiles_y, (unsigned)a, (unsigned)b, connectivity == 2 ? 1 : 0, limit, round, count);
  });
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
