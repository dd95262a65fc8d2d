// The front end the flat-window stages share (window.hip, morph.hip, rank.hip): every one of them gives each pixel a result over the
// pixels of a window around it that are *counted* -- inside the image and, with `within`, non-zero there, whatever the element size of
// `within`.  That rule has ONE reader here, flat_fetch, in a fast form (rows as dwords) and a slow one that must agree; beside it the
// halo, the footprint's half widths, the launcher's choice between the two forms, the WITHIN x DWORDS dispatch and the refusals these
// entry points have in common.  What a stage does with the pixels once they are loaded is its own.  DESIGN.md, "Flat-window stages:
// shared front end".
#pragma once
#include <stdint.h>

#include <type_traits>

#include "common.hpp"
#include "image_common.hpp"

// A tile looks `halo` columns past its own on either side: the radius rounded up to a multiple of 4, so that a thread's four
// adjacent columns start on a multiple of 4 relative to the image.
__host__ __device__ constexpr int flat_halo(int r) { return (r + 3) & ~3; }

// The half width of footprint row dy of a CGC_MORPH_* kind, in integers (the disk: the largest w with w^2 + dy^2 <= r^2); kind and
// |dy| <= r have been checked.
static inline int flat_width(int kind, int r, int dy) {
  const int a = dy < 0 ? -dy : dy;
  if (kind == CGC_MORPH_SQUARE) return r;
  if (kind == CGC_MORPH_DIAMOND) return r - a;
  int w = 0;
  while ((w + 1) * (w + 1) + a * a <= r * r) ++w;
  return w;
}

// Four adjacent pixels of a row, as loaded: p their values, q their flags (a non-zero byte = counted), NOT YET LOOKED AT -- a kernel
// may issue the loads of its next row, go on with other work and only then ask what came back (window.hip scans a row while the next
// two are in flight); nothing in flat_fetch waits for a loaded value.
struct FlatRow {
  uint32_t p, q;
  bool ok;       // DWORDS: the row and the four columns lie inside the image; otherwise q says it all
};

// x: the first column, a multiple of 4 (negative in the left halo of the first tile, >= W past the image).  With DWORDS (the
// launcher's choice, flat_dword_rows) the four columns are all inside or all outside the image, and a row is one dword load per plane
// at an address clamped into the image: no branch.  Otherwise pixel by pixel, also at clamped addresses, and a flag byte is 1 or 0.
template <bool WITHIN, bool DWORDS>
__device__ __forceinline__ FlatRow flat_fetch(const uint8_t* __restrict__ img, const void* __restrict__ within, int wbytes, int H, int W,
                                              int64_t x, int64_t y) {
  const bool row = y >= 0 && y < H;
  const int base = row ? (int)y * W : 0;                                // pixel indices fit int32: H W < 2^31
  FlatRow o;
  if (DWORDS) {
    o.ok = row && x >= 0 && x < W;
    const int i = o.ok ? base + (int)x : 0;
    o.p = *reinterpret_cast<const uint32_t*>(img + i);
    o.q = WITHIN ? *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(within) + i) : 0x01010101u;
  } else {
    o.ok = row;
    o.p = o.q = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = row && x + j >= 0 && x + j < W;
      const int i = in ? base + (int)(x + j) : 0;
      const bool counted = in && (!WITHIN || image_nonzero(within, wbytes, i));
      o.p |= (uint32_t)img[i] << (8 * j);
      o.q |= (uint32_t)counted << (8 * j);
    }
  }
  return o;
}

// The look at a row, for a stage that wants the pixels at once (morph.hip, rank.hip): 0xFF in every byte whose pixel is counted.
// Pixel by pixel the flags already say "inside the image"; only a dword of flags needs `ok` beside it.
template <bool DWORDS>
__device__ __forceinline__ uint32_t flat_counted(const FlatRow& o) {
  uint32_t nz = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) nz |= ((o.q >> (8 * j)) & 255u) != 0 ? 255u << (8 * j) : 0u;
  return DWORDS ? (o.ok ? 0xFFFFFFFFu : 0u) & nz : nz;
}

// Rows as dwords: every row starts on a dword boundary, and the flags of `within` are bytes.
static inline bool dword_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
static inline bool flat_dword_rows(const void* img, const void* within, int within_bytes, int W) {
  return (W & 3) == 0 && dword_aligned(img) && (within == nullptr || (within_bytes == 1 && dword_aligned(within)));
}

// Calls f(std::bool_constant<WITHIN>, std::bool_constant<DWORDS>): the one place that turns the two run-time facts into template
// arguments.
template <typename F>
void flat_dispatch(bool within, bool dwords, F&& f) {
  if (within) {
    if (dwords) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
  } else {
    if (dwords) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
  }
}

// The refusals of every flat-window entry point: an image whose raster indices fit int32 and, if there is a `within`, an element size
// that image_nonzero reads ...
static inline bool bad_flat_image(int H, int W, const void* within, int within_bytes) {
  return bad_image_dims(H, W) || (within != nullptr && bad_elem_bytes(within_bytes));
}
// ... a radius in 0 .. top, and where there is a footprint one of the CGC_MORPH_* kinds.
static inline bool bad_flat_radius(int radius, int top) { return radius < 0 || radius > top; }
static inline bool bad_footprint(int kind, int radius, int top) {
  return kind < CGC_MORPH_SQUARE || kind > CGC_MORPH_DIAMOND || bad_flat_radius(radius, top);
}
