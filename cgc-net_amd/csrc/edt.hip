// Exact Euclidean distance transform of a 2-D image on gfx950, with the nearest site of every pixel: squared distances and raster
// indices, integers throughout, so every result is bit for bit.  Contract item by item: cgc-net_amd/kernels.py
// KernelSpec.distance_transform; layout, launches, the worst-case input and measurements: DESIGN.md, "Distance transform".
//
// A site is a pixel the caller selects (value == 0 or value != 0).  The usual two phases, with the tie rule "smallest raster index of
// the site" carried through both (a site in another row can never beat the nearest one of its own column, and of two sites at equal
// distance in one column the upper one has the smaller index):
//   k_edt_mask    one thread per (64-row segment, column): the segment's sites of that column as one 64-bit word
//   k_edt_column  the same threads: nearest site row above and below the segment from the neighbouring words (the carry), then for
//                 each of the 64 rows the nearest site row of its own column by bit scans, ties to the upper one -> srow int16 [H, W]
//   k_edt_row     one workgroup per image row, its srow in LDS: every pixel searches outwards from its own column, keeps the smallest
//                 (distance^2, site index) pair and stops once k^2 exceeds the best distance^2 (not when it reaches it: an equal
//                 distance with a smaller index may still lie there) or the caller's bound
// No workgroup waits for another one: the only ordering is the launch boundary.  The search window is as wide as the distance to the
// nearest site, so the cost per pixel is O(that distance): a few pixels on nucleus masks, O(W) where a row's columns hold no site.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

constexpr int EDT_SEG = 64;               // rows per column segment: one bit each in a 64-bit word
constexpr int EDT_MAX_SIDE = 32767;       // 2 * 32766^2 < 2^31 - 1: every distance^2 fits int32 below CGC_EDT_INF; rows fit int16

static inline int edt_segments(int H) { return ceil_div(H, EDT_SEG); }
static inline bool edt_bad_dims(int H, int W) { return H < 0 || W < 0 || H > EDT_MAX_SIDE || W > EDT_MAX_SIDE; }

// (a) site words.  Consecutive threads read consecutive pixels of a row.
template <typename T>
__global__ void __launch_bounds__(CGC_BLOCK) k_edt_mask(const T* __restrict__ img, int H, int W, int sites_nonzero,
                                                        unsigned long long* __restrict__ mask) {
  const int x = blockIdx.x * CGC_BLOCK + threadIdx.x, s = blockIdx.y;
  if (x >= W) return;
  const int y0 = s * EDT_SEG, rows = min(EDT_SEG, H - y0);
  const T* p = img + (int64_t)y0 * W + x;
  unsigned long long m = 0;
  for (int ly = 0; ly < rows; ++ly) {
    const bool site = (p[(int64_t)ly * W] != T(0)) == (sites_nonzero != 0);
    m |= (unsigned long long)site << ly;
  }
  mask[(int64_t)s * W + x] = m;
}

// (b) nearest site row of the pixel's own column (-1: the column has no site); of an upper and a lower one at equal distance the upper.
__global__ void __launch_bounds__(CGC_BLOCK) k_edt_column(const unsigned long long* __restrict__ mask, int H, int W, int nseg,
                                                          short* __restrict__ srow) {
  const int x = blockIdx.x * CGC_BLOCK + threadIdx.x, s = blockIdx.y;
  if (x >= W) return;
  const unsigned long long m = mask[(int64_t)s * W + x];
  int up = -1, down = -1;                               // the carry: nearest site row above / below this segment
  for (int t = s - 1; t >= 0; --t) {
    const unsigned long long mm = mask[(int64_t)t * W + x];
    if (mm != 0) { up = t * EDT_SEG + 63 - __builtin_clzll(mm); break; }
  }
  for (int t = s + 1; t < nseg; ++t) {
    const unsigned long long mm = mask[(int64_t)t * W + x];
    if (mm != 0) { down = t * EDT_SEG + __builtin_ctzll(mm); break; }
  }
  const int y0 = s * EDT_SEG, rows = min(EDT_SEG, H - y0);
  short* out = srow + (int64_t)y0 * W + x;
  for (int ly = 0; ly < rows; ++ly) {
    const int y = y0 + ly;
    const unsigned long long ma = m & (~0ull >> (63 - ly)), mb = m >> ly;      // bits 0..ly, bits ly..63
    const int a = ma != 0 ? y0 + 63 - __builtin_clzll(ma) : up;
    const int b = mb != 0 ? y + __builtin_ctzll(mb) : down;
    int r;
    if (a < 0) r = b;
    else if (b < 0) r = a;
    else r = (y - a <= b - y) ? a : b;
    out[(int64_t)ly * W] = (short)r;
  }
}

// (c) one workgroup per row.  key = distance^2 << 32 | site index: its minimum is the nearest site with the tie rule.
__global__ void __launch_bounds__(CGC_BLOCK) k_edt_row(const short* __restrict__ srow, int W, int d2max, int kcap, int* __restrict__ dist2,
                                                       int* __restrict__ nearest) {
  extern __shared__ short row[];
  const int y = blockIdx.x;
  const short* src = srow + (int64_t)y * W;
  for (int x = threadIdx.x; x < W; x += CGC_BLOCK) row[x] = src[x];
  __syncthreads();
  const unsigned long long none = ((unsigned long long)CGC_EDT_INF << 32) | 0xffffffffu;
  for (int x = threadIdx.x; x < W; x += CGC_BLOCK) {
    unsigned long long best = none;
    unsigned bestd = CGC_EDT_INF;
    {
      const int r = row[x];
      if (r >= 0) {
        const int dy = y - r;
        bestd = (unsigned)(dy * dy);
        best = ((unsigned long long)bestd << 32) | (unsigned)(r * W + x);
      }
    }
    const int kl = min(x, kcap), kr = min(W - 1 - x, kcap), kmax = max(kl, kr);
    for (int k = 1; k <= kmax; ++k) {
      const unsigned k2 = (unsigned)(k * k);
      if (k2 > bestd) break;
      if (k <= kl) {
        const int r = row[x - k];
        if (r >= 0) {
          const int dy = y - r;
          const unsigned long long key = ((unsigned long long)(k2 + (unsigned)(dy * dy)) << 32) | (unsigned)(r * W + x - k);
          if (key < best) { best = key; bestd = (unsigned)(key >> 32); }
        }
      }
      if (k <= kr) {
        const int r = row[x + k];
        if (r >= 0) {
          const int dy = y - r;
          const unsigned long long key = ((unsigned long long)(k2 + (unsigned)(dy * dy)) << 32) | (unsigned)(r * W + x + k);
          if (key < best) { best = key; bestd = (unsigned)(key >> 32); }
        }
      }
    }
    const bool found = best != none && (d2max < 0 || bestd <= (unsigned)d2max);
    const int64_t o = (int64_t)y * W + x;
    dist2[o] = found ? (int)bestd : CGC_EDT_INF;
    if (nearest != nullptr) nearest[o] = found ? (int)(unsigned)best : -1;
  }
}

static inline int edt_window(int d2max, int W) {        // min(floor(sqrt(d2max)), W): no site farther away in x can be within the bound
  if (d2max < 0) return W;
  int r = 0;
  while (r < W && (int64_t)(r + 1) * (r + 1) <= d2max) ++r;
  return r;
}

struct EdtWs {
  unsigned long long* mask;      // [segments, W] site words
  short* srow;                   // [H, W] nearest site row of the pixel's own column
};
static inline EdtWs edt_layout(Carver&& c, int H, int W) {      // the one definition of the workspace
  EdtWs w;
  w.mask = c.take<unsigned long long>((int64_t)edt_segments(H) * W);
  w.srow = c.take<short>((int64_t)H * W);
  return w;
}

template <typename T>
int edt_run(const void* image, int H, int W, int sites_nonzero, int d2max, void* ws, int* dist2, int* nearest, hipStream_t st) {
  const EdtWs w = edt_layout(Carver(ws), H, W);
  const int nseg = edt_segments(H);
  const dim3 cols(ceil_div(W, CGC_BLOCK), nseg);
  hipLaunchKernelGGL(k_edt_mask<T>, cols, dim3(CGC_BLOCK), 0, st, static_cast<const T*>(image), H, W, sites_nonzero, w.mask);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_edt_column, cols, dim3(CGC_BLOCK), 0, st, w.mask, H, W, nseg, w.srow);
  CGC_RETURN_IF_LAUNCH_FAILED();
  const int kcap = edt_window(d2max, W);
  hipLaunchKernelGGL(k_edt_row, dim3(H), dim3(CGC_BLOCK), (size_t)W * sizeof(short), st, w.srow, W, d2max, kcap, dist2, nearest);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // namespace

extern "C" int64_t cgc_edt_ws_bytes(int H, int W) {
  if (edt_bad_dims(H, W)) return 0;
  return layout_bytes(edt_layout, H, W);
}

extern "C" int cgc_edt(const void* image, int elem_bytes, int H, int W, int sites_nonzero, int d2max, void* ws, int* dist2, int* nearest,
                       cgc_stream_t stream) {
  if (edt_bad_dims(H, W)) return CGC_EINVAL;
  if (bad_elem_bytes(elem_bytes)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (image == nullptr || ws == nullptr || dist2 == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int sn = sites_nonzero != 0;
  switch (elem_bytes) {
    case 1: return edt_run<uint8_t>(image, H, W, sn, d2max, ws, dist2, nearest, st);
    case 2: return edt_run<uint16_t>(image, H, W, sn, d2max, ws, dist2, nearest, st);
    case 4: return edt_run<uint32_t>(image, H, W, sn, d2max, ws, dist2, nearest, st);
    default: return edt_run<uint64_t>(image, H, W, sn, d2max, ws, dist2, nearest, st);
  }
}
