// The round of the two path relaxations on tile_relax.hpp's schedule, geodesic.hip and watershed.hip: one 64-bit key per pixel that
// only ever decreases, a domain byte per pixel, axial and diagonal steps between domain pixels, and a Jacobi sweep in LDS until
// nothing in the tile moves.  A Rule says what a key is:
//   Rule::NONE            the "not reached" key; no key of a path is above it
//   rule.axial, diagonal  the two step costs as extend() takes them; diagonal == 0: no diagonal steps
//   rule.setup(j, kc, i)  once per domain pixel of this thread (its j-th, key kc, raster index i): loads what extend() needs of the
//                         pixel into registers and returns whether the pixel is relaxed at all
//   rule.extend(kq, step, j)  the key that a step from a neighbour with key kq offers this thread's j-th pixel, or PATH_NOTHING;
//                         plain arithmetic on any kq: it is also evaluated, and its result dropped, where kq == NONE
#pragma once
#include "tile_relax.hpp"

typedef unsigned long long path_key;

constexpr path_key PATH_NOTHING = ~(path_key)0;  // below no key: an offer that never wins

constexpr int PATH_LW = RELAX_TILE + 2;           // LDS row: the tile plus a one-pixel halo; 66 * 66 * (8 + 1) bytes = 39204 in all
constexpr int PATH_LPX = PATH_LW * PATH_LW;

// The begin kernels' common part: the domain is the seeds and what `within` (null: every pixel) holds.  Returns whether pixel i is a
// seed; a pixel of the domain can move.
__device__ __forceinline__ bool path_begin_pixel(const void* seeds, int seed_bytes, const void* within, int within_bytes, int64_t i,
                                                 unsigned char* __restrict__ dom, bool& in) {
  const bool seed = image_nonzero(seeds, seed_bytes, i);
  in = seed || within == nullptr || image_nonzero(within, within_bytes, i);
  dom[i] = in ? 1 : 0;
  return seed;
}

__device__ __forceinline__ path_key lds_key(const path_key* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// One candidate: the step from LDS cell q into this thread's j-th pixel, whose best key so far is `best`.
template <class Rule, typename Step>
__device__ __forceinline__ path_key path_try(const Rule& rule, const path_key* k, int q, Step step, int j, path_key best) {
  const path_key kq = lds_key(k + q);
  const path_key cand = rule.extend(kq, step, j);
  return ((kq != Rule::NONE) & (cand < best)) ? cand : best;
}

template <class Rule>
__device__ __forceinline__ void path_relax_round(Rule rule, path_key* __restrict__ key, const unsigned char* __restrict__ dom,
                                                 int* __restrict__ stamp, int H, int W, int tiles_x, int tiles_y, int conn8, int round,
                                                 int* __restrict__ changed) {
  __shared__ path_key k[PATH_LPX];
  __shared__ unsigned char d[PATH_LPX];
  if (!relax_tile_runs(stamp, round)) return;
  const RelaxTile t = relax_tile(tiles_x);
  const bool reached = relax_load_halo<path_key, PATH_LW>(key, H, W, t, [&](int c, const RelaxCell<path_key>& cell) {
    const unsigned char in = cell.inside ? dom[cell.i] : 0;
    const path_key v = in ? cell.load() : Rule::NONE;
    k[c] = v;
    d[c] = in;
    return v != Rule::NONE;
  });
  if (!reached) return;                           // no seed has reached the tile or its halo yet: nothing can move

  const int lx = relax_lx();
  unsigned live = 0;                              // bit j: this thread's j-th pixel is relaxed
#pragma unroll
  for (int j = 0; j < RELAX_PER_THREAD; ++j) {
    const int ly = relax_ly(j);
    const int c = (ly + 1) * PATH_LW + lx + 1;
    if (d[c] && rule.setup(j, k[c], (int64_t)(t.y0 + ly) * W + t.x0 + lx)) live |= 1u << j;      // a domain pixel lies inside the image
  }

  unsigned moved = 0;                             // bit j: this thread's j-th pixel moved
  for (;;) {
    int ch = 0;
#pragma unroll
    for (int j = 0; j < RELAX_PER_THREAD; ++j) {
      if (!(live >> j & 1u)) continue;
      const int c = (relax_ly(j) + 1) * PATH_LW + lx + 1;
      const path_key cur = lds_key(k + c);        // only this thread ever writes k[c]
      path_key best = cur;
      best = path_try(rule, k, c - PATH_LW, rule.axial, j, best);
      best = path_try(rule, k, c - 1, rule.axial, j, best);
      best = path_try(rule, k, c + 1, rule.axial, j, best);
      best = path_try(rule, k, c + PATH_LW, rule.axial, j, best);
      if (rule.diagonal != 0) {
        // connectivity 1: a diagonal step needs one of the two pixels it passes between in the domain (no squeezing through a corner)
        const bool up = conn8 || d[c - PATH_LW], down = conn8 || d[c + PATH_LW], left = d[c - 1], right = d[c + 1];
        if (up || left) best = path_try(rule, k, c - PATH_LW - 1, rule.diagonal, j, best);
        if (up || right) best = path_try(rule, k, c - PATH_LW + 1, rule.diagonal, j, best);
        if (down || left) best = path_try(rule, k, c + PATH_LW - 1, rule.diagonal, j, best);
        if (down || right) best = path_try(rule, k, c + PATH_LW + 1, rule.diagonal, j, best);
      }
      if (best < cur) {
        __hip_atomic_store(k + c, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ch = 1;
        moved |= 1u << j;
      }
    }
    if (!__syncthreads_or(ch)) break;             // a sweep in which nothing moved read final values only: the tile's fixed point
  }

  relax_write_back<path_key, PATH_LW>(key, k, H, W, t, [&](int j, int64_t, const path_key&) { return (moved >> j & 1u) != 0; });
  relax_publish(moved != 0, t, tiles_x, tiles_y, stamp, round, changed);
}
