// Resampling of the image stage ("F21": the pixel size of a tile, a plane or a label image).  ONE kernel template, k_resample<PB, G,
// Op>, for every mode; a pixel of the output has PB bytes (a gray byte, three interleaved channel bytes, a label of 1, 2, 4 or 8
// bytes), a lane produces G adjacent pixels of one output row (G * PB is a multiple of 4) and stores them as dwords.
//   Layout.  A workgroup of four waves owns RS_ROWS output rows x TX = 63 G output columns; wave w takes the rows yb + w, yb + w + 4,
//   ...  In a row whose first byte sits at address a, the groups of G pixels start where the address is a multiple of 4: `lead` pixels
//   (0..3, from a mod 4) in front of them.  Lane l of the wave takes the pixels [xb + lead + G (l - 1), + G) cut to the workgroup's
//   columns: lane 0 the `lead` head pixels, the last lane what is left, every lane between them one full aligned group -- so only
//   the first and last 1-3 pixels of a row's share are written as bytes, whatever the base address and the row length.
//   Tables.  The per-column geometry (an index and a weight, or a box) costs integer divisions; a workgroup computes it once for its
//   TX columns into LDS (one dword per column) and every row reads it from there.  The per-row geometry is uniform over a wave.
//   Ops.  Linear<C>: four byte loads per channel, the 2 x 2 weights from the table, one rounding by an 8-step restoring division in
//   64 bits (the quotient is a byte).  Area<C>: the lane walks the source box of its pixel row by row, a row's weighted sum in uint32
//   (255 * 32767 < 2^23), the rows in uint64; neighbouring lanes own neighbouring boxes, so a wave's loads of one step cover one
//   contiguous stretch of a source row and every cache line is fetched once.  Nearest<T>: one load.  Majority<T>: the box is at most
//   9 x 9; a first walk finds out whether it holds one value only (the usual case inside a nucleus and in the background), otherwise
//   every pixel of the box is a candidate whose total weight is a second walk -- registers only, no table of votes.
// No atomics and no float arithmetic in this file; no scratch.  The arithmetic item by item: kernels.py KernelSpec.resample_u8 /
// resample_labels.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

#define RS_THREADS 256
#define RS_ROWS 8                      // output rows of one workgroup: two per wave
#define RS_LANES 63                    // groups of one wave and row that can be full: lane 0 takes the pixels in front of the first
#define RS_TABLE (4 * RS_LANES)        // columns of one workgroup at G = 4
constexpr int RS_MAX_SIDE = 32767;     // (2 d + 1) n <= 65533 * 32767 < 2^31 and 2 m (n - 1) < 2^31; a table entry holds 15 + 16 bits
constexpr int RS_MAX_FACTOR = 8;       // majority: a box spans at most 9 pixels per axis
enum { RS_LINEAR = 0, RS_AREA = 1 };                                        // CGC_RESAMPLE_LINEAR / _AREA
enum { RS_NEAREST = 0, RS_MAJORITY = 1, RS_MAJORITY_UNSIGNED = 2 };          // CGC_RESAMPLE_NEAREST / _MAJORITY / _MAJORITY_UNSIGNED
static_assert((uint64_t)(2 * (RS_MAX_SIDE - 1) + 1) * RS_MAX_SIDE < ((uint64_t)1 << 32), "(2 d + 1) n fits uint32");
static_assert((uint64_t)2 * RS_MAX_SIDE * (RS_MAX_SIDE - 1) < ((uint64_t)1 << 31), "the clamp 2 m (n - 1) fits");
static_assert(RS_MAX_SIDE < (1 << 15) && 2 * RS_MAX_SIDE < (1 << 16), "an index and a weight share a dword");
static_assert(RS_THREADS == 4 * 64 && RS_ROWS % 4 == 0, "four waves, whole rounds of rows");

namespace {

// Item 2: the source position of output index d on an axis of n source and m output pixels, as (i0 << 16) | f with the weight
// numerator f over 2 m.  All unsigned: (2 d + 1) n comes within 2 * 10^5 of 2^31.
__device__ __forceinline__ uint32_t linear_entry(uint32_t d, uint32_t n, uint32_t m) {
  const uint32_t a = (2u * d + 1u) * n;
  const uint32_t num = min(a > m ? a - m : 0u, 2u * m * (n - 1u));
  const uint32_t i0 = num / (2u * m);
  return (i0 << 16) | (num - i0 * 2u * m);
}

// Item 4: the source pixels lo .. hi that meet the interval [d n / m, (d + 1) n / m), as (lo << 16) | hi.
__device__ __forceinline__ uint32_t box_entry(uint32_t d, uint32_t n, uint32_t m) {
  return ((d * n / m) << 16) | (((d + 1u) * n - 1u) / m);
}

// Item 4's weight of source pixel i in the box of output index d, in units of 1 / m of a pixel.
__device__ __forceinline__ uint32_t box_weight(uint32_t d, uint32_t i, uint32_t n, uint32_t m) {
  return min((d + 1u) * n, (i + 1u) * m) - max(d * n, i * m);
}

// floor((2 s + den) / (2 den)) for s <= 255 den: the quotient is a byte, eight steps of restoring division.
__device__ __forceinline__ uint32_t round_div_byte(uint64_t s, uint64_t den) {
  uint64_t rem = 2 * s + den;
  uint32_t q = 0;
#pragma unroll
  for (int b = 7; b >= 0; --b) {
    const uint64_t t = (2 * den) << b;
    if (rem >= t) {
      rem -= t;
      q |= 1u << b;
    }
  }
  return q;
}

// An op: xentry(x) -- the table entry of output column x; row(y) -- the state of output row y; pixel(x, e) -- the PB bytes of the
// pixel (row, x) with table entry e, little end first.
template <int C>
struct Linear {
  const uint8_t* __restrict__ src;
  int H, W, H2, W2;
  const uint8_t *r0, *r1;
  uint32_t fy;
  __device__ __forceinline__ uint32_t xentry(int x) const { return linear_entry(x, W, W2); }
  __device__ __forceinline__ void row(int y) {
    const uint32_t e = linear_entry(y, H, H2);
    const int y0 = e >> 16;
    fy = e & 0xffffu;
    r0 = src + (int64_t)y0 * W * C;
    r1 = src + (int64_t)min(y0 + 1, H - 1) * W * C;
  }
  __device__ __forceinline__ uint64_t pixel(int, uint32_t e) const {
    const int x0 = (int)(e >> 16) * C, x1 = min((int)(e >> 16) + 1, W - 1) * C;
    const uint32_t fx = e & 0xffffu, gx = 2u * W2 - fx, gy = 2u * H2 - fy;
    const uint64_t den = 4ull * H2 * W2;
    uint64_t v = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const uint32_t top = r0[x0 + c] * gx + r0[x1 + c] * fx, bot = r1[x0 + c] * gx + r1[x1 + c] * fx;      // <= 255 * 2 W2 < 2^24
      v |= (uint64_t)round_div_byte((uint64_t)top * gy + (uint64_t)bot * fy, den) << (8 * c);
    }
    return v;
  }
};

template <int C>
struct Area {
  const uint8_t* __restrict__ src;
  int H, W, H2, W2;
  int y, ylo, yhi;
  __device__ __forceinline__ uint32_t xentry(int x) const { return box_entry(x, W, W2); }
  __device__ __forceinline__ void row(int y_) {
    const uint32_t e = box_entry(y_, H, H2);
    y = y_;
    ylo = e >> 16;
    yhi = e & 0xffffu;
  }
  __device__ __forceinline__ uint64_t pixel(int x, uint32_t e) const {
    const int xlo = e >> 16, xhi = e & 0xffffu;
    uint64_t s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0;
    for (int yy = ylo; yy <= yhi; ++yy) {
      const uint8_t* r = src + (int64_t)yy * W * C;
      uint32_t t[C];
#pragma unroll
      for (int c = 0; c < C; ++c) t[c] = 0;
      for (int xx = xlo; xx <= xhi; ++xx) {
        const uint32_t ox = box_weight(x, xx, W, W2);
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] += r[xx * C + c] * ox;      // a row's sum: <= 255 W < 2^23
      }
      const uint32_t oy = box_weight(y, yy, H, H2);
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] += (uint64_t)oy * t[c];
    }
    uint64_t v = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) v |= (uint64_t)round_div_byte(s[c], (uint64_t)H * W) << (8 * c);
    return v;
  }
};

template <typename T>
struct Nearest {
  const T* __restrict__ src;
  int H, W, H2, W2;
  const T* r;
  __device__ __forceinline__ uint32_t xentry(int x) const { return (2u * x + 1u) * W / (2u * W2); }
  __device__ __forceinline__ void row(int y) { r = src + (int64_t)((2u * y + 1u) * H / (2u * H2)) * W; }
  __device__ __forceinline__ uint64_t pixel(int, uint32_t e) const { return (uint64_t)r[e]; }
};

template <typename T>      // T carries the order of item 7: int8_t .. int64_t signed, uint8_t unsigned
struct Majority {
  const T* __restrict__ src;
  int H, W, H2, W2;
  int y, ylo, yhi;
  __device__ __forceinline__ uint32_t xentry(int x) const { return box_entry(x, W, W2); }
  __device__ __forceinline__ void row(int y_) {
    const uint32_t e = box_entry(y_, H, H2);
    y = y_;
    ylo = e >> 16;
    yhi = e & 0xffffu;
  }
  __device__ __forceinline__ uint64_t pixel(int x, uint32_t e) const {
    const int xlo = e >> 16, xhi = e & 0xffffu;
    T best = src[(int64_t)ylo * W + xlo];
    bool mixed = false;
    for (int yy = ylo; yy <= yhi; ++yy)
      for (int xx = xlo; xx <= xhi; ++xx) mixed |= src[(int64_t)yy * W + xx] != best;
    if (mixed) {
      uint32_t best_w = 0;             // every candidate weighs at least 1: the first one replaces this
      for (int cy = ylo; cy <= yhi; ++cy)
        for (int cx = xlo; cx <= xhi; ++cx) {
          const T cand = src[(int64_t)cy * W + cx];
          if (best_w != 0 && cand == best) continue;      // weighed already
          uint32_t w = 0;              // <= H W < 2^30
          for (int yy = ylo; yy <= yhi; ++yy) {
            const uint32_t oy = box_weight(y, yy, H, H2);
            for (int xx = xlo; xx <= xhi; ++xx)
              if (src[(int64_t)yy * W + xx] == cand) w += oy * box_weight(x, xx, W, W2);
          }
          if (w > best_w || (w == best_w && cand < best)) {
            best = cand;
            best_w = w;
          }
        }
    }
    return (uint64_t)best;
  }
};

template <int PB, int G, typename Op>
__global__ __launch_bounds__(RS_THREADS) void k_resample(Op op, uint8_t* __restrict__ dst, int H2, int W2) {
  static_assert((G * PB) % 4 == 0 && G * RS_LANES <= RS_TABLE && PB <= 8, "whole dwords per lane; the table holds the columns");
  constexpr int TX = G * RS_LANES, WORDS = G * PB / 4;
  __shared__ uint32_t xtab[RS_TABLE];
  const int xb = blockIdx.x * TX, xend = min(xb + TX, W2);
  for (int i = threadIdx.x; xb + i < xend; i += RS_THREADS) xtab[i] = op.xentry(xb + i);
  __syncthreads();
  const int lane = threadIdx.x & 63, yend = min((int)(blockIdx.y + 1) * RS_ROWS, H2);
  for (int y = blockIdx.y * RS_ROWS + (threadIdx.x >> 6); y < yend; y += RS_THREADS / 64) {
    op.row(y);
    uint8_t* orow = dst + (int64_t)y * W2 * PB;
    const int a = (int)(reinterpret_cast<uintptr_t>(orow) & 3u);      // xb * PB is a multiple of 4
    const int lead = PB == 1 ? (4 - a) & 3 : (PB == 2 ? ((4 - a) & 3) >> 1 : (PB == 3 ? a : 0));      // (a + PB * lead) % 4 == 0
    const int x0 = xb + lead + G * (lane - 1);
    if (x0 >= xend || x0 + G <= xb) continue;
    uint32_t packed[WORDS];
#pragma unroll
    for (int k = 0; k < WORDS; ++k) packed[k] = 0u;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = x0 + j;
      if (x < xb || x >= xend) continue;
      const uint64_t v = op.pixel(x, xtab[x - xb]);
#pragma unroll
      for (int k = 0; k < PB; ++k) packed[(j * PB + k) >> 2] |= (uint32_t)((v >> (8 * k)) & 255u) << (8 * ((j * PB + k) & 3));
    }
    uint8_t* o = orow + (int64_t)x0 * PB;
    if (x0 >= xb && x0 + G <= xend && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
#pragma unroll
      for (int k = 0; k < WORDS; ++k) reinterpret_cast<uint32_t*>(o)[k] = packed[k];
    } else {
#pragma unroll
      for (int k = 0; k < G * PB; ++k)
        if (x0 + k / PB >= xb && x0 + k / PB < xend) o[k] = (uint8_t)(packed[k >> 2] >> (8 * (k & 3)));
    }
  }
}

template <int PB, int G, typename Op>
int launch_resample(Op op, void* dst, int H2, int W2, cgc_stream_t stream) {
  const dim3 grid(ceil_div(W2, G * RS_LANES), ceil_div(H2, RS_ROWS));      // <= 521 x 4096
  hipLaunchKernelGGL((k_resample<PB, G, Op>), grid, dim3(RS_THREADS), 0, as_stream(stream), op, static_cast<uint8_t*>(dst), H2, W2);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

template <typename T, int G>
int launch_labels(const void* src, int H, int W, int H2, int W2, bool majority, void* dst, cgc_stream_t stream) {
  if (majority) return launch_resample<(int)sizeof(T), G>(Majority<T>{static_cast<const T*>(src), H, W, H2, W2, 0, 0, 0}, dst, H2, W2, stream);
  return launch_resample<(int)sizeof(T), G>(Nearest<T>{static_cast<const T*>(src), H, W, H2, W2, nullptr}, dst, H2, W2, stream);
}

bool bad_resample_sides(int H, int W, int H2, int W2) {
  return H < 1 || W < 1 || H2 < 1 || W2 < 1 || H > RS_MAX_SIDE || W > RS_MAX_SIDE || H2 > RS_MAX_SIDE || W2 > RS_MAX_SIDE || bad_image_dims(H, W) ||
         bad_image_dims(H2, W2);
}

}  // namespace

extern "C" int cgc_resample_max_side(void) { return RS_MAX_SIDE; }
extern "C" int cgc_resample_labels_max_factor(void) { return RS_MAX_FACTOR; }

extern "C" int cgc_resample_u8(const uint8_t* src, int H, int W, int channels, int H2, int W2, int mode, uint8_t* dst, cgc_stream_t stream) {
  if (bad_resample_sides(H, W, H2, W2) || (channels != 1 && channels != 3) || (mode != RS_LINEAR && mode != RS_AREA) || src == nullptr ||
      dst == nullptr || (mode == RS_AREA && (H2 > H || W2 > W)))
    return CGC_EINVAL;
  if (mode == RS_LINEAR) {
    if (channels == 1) return launch_resample<1, 4>(Linear<1>{src, H, W, H2, W2, nullptr, nullptr, 0u}, dst, H2, W2, stream);
    return launch_resample<3, 4>(Linear<3>{src, H, W, H2, W2, nullptr, nullptr, 0u}, dst, H2, W2, stream);
  }
  if (channels == 1) return launch_resample<1, 4>(Area<1>{src, H, W, H2, W2, 0, 0, 0}, dst, H2, W2, stream);
  return launch_resample<3, 4>(Area<3>{src, H, W, H2, W2, 0, 0, 0}, dst, H2, W2, stream);
}

extern "C" int cgc_resample_labels(const void* src, int elem_bytes, int H, int W, int H2, int W2, int mode, void* dst, cgc_stream_t stream) {
  if (bad_resample_sides(H, W, H2, W2) || bad_elem_bytes(elem_bytes) || mode < RS_NEAREST || mode > RS_MAJORITY_UNSIGNED ||
      (mode == RS_MAJORITY_UNSIGNED && elem_bytes != 1) || src == nullptr || dst == nullptr)
    return CGC_EINVAL;
  const bool majority = mode != RS_NEAREST;
  if (majority && (H2 > H || W2 > W || H > (int64_t)RS_MAX_FACTOR * H2 || W > (int64_t)RS_MAX_FACTOR * W2)) return CGC_EINVAL;
  if (mode == RS_MAJORITY_UNSIGNED)
    return launch_resample<1, 4>(Majority<uint8_t>{static_cast<const uint8_t*>(src), H, W, H2, W2, 0, 0, 0}, dst, H2, W2, stream);
  switch (elem_bytes) {                // the copy of `nearest` does not read the sign
    case 1: return launch_labels<int8_t, 4>(src, H, W, H2, W2, majority, dst, stream);
    case 2: return launch_labels<int16_t, 2>(src, H, W, H2, W2, majority, dst, stream);
    case 4: return launch_labels<int32_t, 1>(src, H, W, H2, W2, majority, dst, stream);
    default: return launch_labels<int64_t, 1>(src, H, W, H2, W2, majority, dst, stream);
  }
}
