// Window sums of a uint8 image on gfx950, and the local (mean / Niblack) threshold that stands on them: for every pixel the number n,
// the sum S and the sum of squares Q of the (selected) pixels of the clipped (2 r + 1)^2 window around it.  Contract item by item:
// cgc-net_amd/kernels.py KernelSpec.window_sums / local_threshold; design and measurements: DESIGN.md, "Window sums and local
// thresholds".
//
// ONE kernel, k_window<WITHIN, DECIDE, DWORDS>, one launch per call, no workspace.  A workgroup owns a tile of WIN_ROWS rows x strip(r)
// columns, strip(r) = WIN_COLS - 2 halo(r), halo(r) = r rounded up to a multiple of 4, and looks at the WIN_COLS = 1024 columns
// [x0 - halo, x0 + strip + halo): thread t keeps, in registers, the sums over the rows y - r .. y + r of its four adjacent columns
// x0 - halo + 4 t .. + 3 (*column sums*; what lies outside the image, or outside `within`, counts as nothing).
//   warm-up    rows y0 - r - 1 .. y0 + r - 1 are added (one dword load per thread and row, nothing else)
//   per row y  + row y + r, - row y - r - 1, both loaded one output row ahead and not looked at before; an inclusive scan of the
//              1024 column sums over the workgroup (four columns in the thread, six DPP moves over the wave, four wave totals
//              through LDS) is written to LDS; the window sum of output column x is P[x + r] - P[x - r - 1], two conflict-free LDS
//              reads per sum (consecutive lanes take consecutive columns)
//   epilogue   DECIDE = false: store n, S, Q.  DECIDE = true: the pixel's own value (loaded before the scan), the rule in integers,
//              one byte stored.
// The halo, the loader of a row (flat_fetch) and the launcher's choice DWORDS are image_window.hpp's, shared with morph.hip and
// rank.hip: with W % 4 == 0, dword-aligned bases and a 1-byte `within` a row of a thread is one dword load per plane; otherwise (odd
// widths, an unaligned view, a `within` of wider elements) pixels are loaded one by one -- same sums, slower.
// WIDTHS.  A column sum holds at most 255 pixels: n <= 255, S <= 65 025, Q <= 255^3 < 2^24.  The scan over 1024 columns keeps n
// (<= 261 120) and S (<= 66 585 600) exactly in uint32.  The scan of Q reaches 1024 * 255^3 > 2^32 and WRAPS; a window's Q is a
// difference of two scan entries and is at most 255^2 * 255^2 = 4 228 250 625 < 2^32, so the difference modulo 2^32 is the sum
// itself.  Subtracting a row from a column sum is exact: the row was added before.  Nothing else is narrower than 64 bits.
// Without `within`, n is not scanned at all: it is the closed form (rows in the image) x (columns in the image).
#include <stdint.h>

#include "common.hpp"
#include "image_window.hpp"

namespace {

constexpr int WIN_MAX_RADIUS = 127;
constexpr int WIN_CPT = 4;                            // adjacent columns per thread
constexpr int WIN_COLS = CGC_BLOCK * WIN_CPT;         // 1024 columns a workgroup looks at
constexpr int WIN_ROWS = 16;                          // rows of a tile
constexpr int WIN_WAVES = CGC_BLOCK / CGC_WAVE;
static_assert(WIN_COLS > 2 * flat_halo(WIN_MAX_RADIUS), "a strip must keep columns of its own at the largest radius");

struct WinRule {
  int k64, offset, floor;
};

// The look at a row that flat_fetch loaded, and the first: the loads of the next row are in flight while this row is scanned, and
// nothing may wait for them before then.  w = 1 iff the pixel is inside the image and counted, v = its value or 0
__device__ __forceinline__ void win_unpack(const FlatRow& o, uint32_t (&v)[WIN_CPT], uint32_t (&w)[WIN_CPT]) {
#pragma unroll
  for (int j = 0; j < WIN_CPT; ++j) {
    w[j] = o.ok && ((o.q >> (8 * j)) & 255u) != 0;
    v[j] = w[j] ? (o.p >> (8 * j)) & 255u : 0u;
  }
}

// Inclusive scan over the 64 lanes of a wave in six register-to-register DPP moves: shifts by 1, 2, 4, 8 inside each row of 16 lanes
// (a lane without a source adds 0), then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t win_dpp(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t win_wave_scan(uint32_t x) {
  x += win_dpp<0x111, 0xF>(x);      // row_shr:1
  x += win_dpp<0x112, 0xF>(x);      // row_shr:2
  x += win_dpp<0x114, 0xF>(x);      // row_shr:4
  x += win_dpp<0x118, 0xF>(x);      // row_shr:8
  x += win_dpp<0x142, 0xA>(x);      // row_bcast:15
  x += win_dpp<0x143, 0xC>(x);      // row_bcast:31
  return x;
}

// v > m + k s + c and v > floor and n >= 1, with m = S / n, s^2 = Q / n - m^2, k = k64 / 64, in int64 (bounds: KernelSpec.local_threshold)
__device__ __forceinline__ bool win_decide(int v, uint32_t n, uint32_t S, uint32_t Q, const WinRule& rule) {
  const bool live = n >= 1 && v > rule.floor;
  const int L = 64 * ((int)n * (v - rule.offset) - (int)S);             // |L| < 2^31: every product below is 32 x 32 -> 64 bits
  if (rule.k64 == 0) return live & (L > 0);                             // uniform, as the branch below: no lane takes another path
  const int64_t D = (int64_t)((uint64_t)n * Q - (uint64_t)S * S);       // 0 <= D < 2^46
  const int64_t L2 = (int64_t)L * L, k2D = (int64_t)(rule.k64 * rule.k64) * D;
  if (rule.k64 > 0) return live & (L > 0) & (L2 > k2D);
  return live & ((L > 0) | ((L == 0) & (D > 0)) | ((L < 0) & (L2 < k2D)));
}

template <bool WITHIN, bool DECIDE, bool DWORDS>
__global__ void __launch_bounds__(CGC_BLOCK) k_window(const uint8_t* __restrict__ img, const void* __restrict__ within, int wbytes, int H,
                                                      int W, int r, int strips, WinRule rule, int* __restrict__ out_n,
                                                      int* __restrict__ out_s, int64_t* __restrict__ out_q, uint8_t* __restrict__ out_fg) {
  constexpr int K = WITHIN ? 3 : 2;                                     // scanned quantities: S, Q and (with `within`) n
  __shared__ uint32_t wave_tot[2][WIN_WAVES][K];
  __shared__ __attribute__((aligned(16))) uint32_t P[2][K][WIN_COLS];   // the scans of two consecutive rows: two barriers per row
  const int strip = blockIdx.x % strips, chunk = blockIdx.x / strips;
  const int halo = flat_halo(r), tw = WIN_COLS - 2 * halo;
  const int64_t x0 = (int64_t)strip * tw;                               // < W
  const int y0 = chunk * WIN_ROWS, y1 = H - y0 < WIN_ROWS ? H : y0 + WIN_ROWS;      // y0 < H
  const int t = threadIdx.x, lane = t & (CGC_WAVE - 1), wave = t / CGC_WAVE;
  const int64_t xc = x0 - halo + WIN_CPT * t;                           // a multiple of 4

  uint32_t c[3][WIN_CPT];                                               // column sums: [0] S, [1] Q, [2] n
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < WIN_CPT; ++j) c[k][j] = 0;
  uint32_t v[WIN_CPT], w[WIN_CPT], lv[WIN_CPT], lw[WIN_CPT];
  {
    const int64_t ya = (int64_t)y0 - r - 1 > 0 ? (int64_t)y0 - r - 1 : 0, yb = (int64_t)y0 + r - 1 < H - 1 ? (int64_t)y0 + r - 1 : H - 1;
#pragma unroll 4
    for (int64_t y = ya; y <= yb; ++y) {
      win_unpack(flat_fetch<WITHIN, DWORDS>(img, within, wbytes, H, W, xc, y), v, w);
#pragma unroll
      for (int j = 0; j < WIN_CPT; ++j) {
        c[0][j] += v[j];
        c[1][j] += v[j] * v[j];
        c[2][j] += w[j];
      }
    }
  }
  // what this thread stores: output columns x0 + j * 256 + t, consecutive lanes on consecutive columns
  bool mine[WIN_CPT];
  int cols_in[WIN_CPT];                                                 // columns of the window inside the image (n without `within`)
#pragma unroll
  for (int j = 0; j < WIN_CPT; ++j) {
    const int col = j * CGC_BLOCK + t;
    const int64_t x = x0 + col;
    mine[j] = col < tw && x < W;
    cols_in[j] = (int)((x + r < W - 1 ? x + r : W - 1) - (x - r > 0 ? x - r : 0)) + 1;
  }
  // the row that enters and the row that leaves are loaded one output row ahead: their latency hides behind the scan
  FlatRow enter = flat_fetch<WITHIN, DWORDS>(img, within, wbytes, H, W, xc, (int64_t)y0 + r);
  FlatRow leave = flat_fetch<WITHIN, DWORDS>(img, within, wbytes, H, W, xc, (int64_t)y0 - r - 1);

  for (int y = y0; y < y1; ++y) {
    const int b = (y - y0) & 1;
    const int row0 = y * W + (int)x0;                                   // index of the tile's first pixel in this row: < H W
    win_unpack(enter, v, w);
    win_unpack(leave, lv, lw);
    enter = flat_fetch<WITHIN, DWORDS>(img, within, wbytes, H, W, xc, (int64_t)y + 1 + r);
    leave = flat_fetch<WITHIN, DWORDS>(img, within, wbytes, H, W, xc, (int64_t)y - r);
    uint32_t own[WIN_CPT];                                              // the pixels this thread decides: needed after the scan
    if (DECIDE) {
#pragma unroll
      for (int j = 0; j < WIN_CPT; ++j) own[j] = img[mine[j] ? row0 + j * CGC_BLOCK + t : 0];
    }
#pragma unroll
    for (int j = 0; j < WIN_CPT; ++j) {
      c[0][j] += v[j] - lv[j];
      c[1][j] += v[j] * v[j] - lv[j] * lv[j];
      c[2][j] += w[j] - lw[j];
    }
    // inclusive scan of the 1024 column sums: in the thread, over the wave, over the four waves
    uint32_t p[K][WIN_CPT], tot[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint32_t run = 0;
#pragma unroll
      for (int j = 0; j < WIN_CPT; ++j) p[k][j] = run += c[k][j];
      tot[k] = win_wave_scan(run);
    }
    if (lane == CGC_WAVE - 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) wave_tot[b][wave][k] = tot[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint32_t base = tot[k] - p[k][WIN_CPT - 1];                       // everything left of this thread's columns
#pragma unroll
      for (int u = 0; u < WIN_WAVES - 1; ++u) base += u < wave ? wave_tot[b][u][k] : 0u;
      *reinterpret_cast<uint4*>(&P[b][k][WIN_CPT * t]) = make_uint4(base + p[k][0], base + p[k][1], base + p[k][2], base + p[k][3]);
    }
    __syncthreads();
    // output column x0 + col reads P at col + halo + r and col + halo - r - 1 (>= -1; -1: nothing to the left)
    const int rows_in = (int)(((int64_t)y + r < H - 1 ? (int64_t)y + r : H - 1) - (y - r > 0 ? y - r : 0)) + 1;
#pragma unroll
    for (int j = 0; j < WIN_CPT; ++j) {
      if (!mine[j]) continue;
      const int col = j * CGC_BLOCK + t;
      const int hi = col + halo + r, lo = col + halo - r - 1;           // hi <= tw - 1 + 2 halo = WIN_COLS - 1
      uint32_t sum[3];
#pragma unroll
      for (int k = 0; k < K; ++k) sum[k] = P[b][k][hi] - (lo >= 0 ? P[b][k][lo] : 0u);
      if (!WITHIN) sum[2] = (uint32_t)(rows_in * cols_in[j]);
      const int i = row0 + col;
      if (DECIDE) {
        out_fg[i] = win_decide((int)own[j], sum[2], sum[0], sum[1], rule) ? 1 : 0;
      } else {
        out_n[i] = (int)sum[2];
        out_s[i] = (int)sum[0];
        out_q[i] = (int64_t)sum[1];
      }
    }
  }
}

template <bool WITHIN, bool DECIDE, bool DWORDS>
void launch_window_as(const uint8_t* img, const void* within, int within_bytes, int H, int W, int radius, WinRule rule, int* n, int* s,
                      int64_t* q, uint8_t* fg, hipStream_t st) {
  const int strips = (int)ceil_div64(W, WIN_COLS - 2 * flat_halo(radius));
  const int64_t blocks = strips * ceil_div64(H, WIN_ROWS);              // < H W / (768 WIN_ROWS) + H / WIN_ROWS + W / 768 + 1 < 2^31
  hipLaunchKernelGGL((k_window<WITHIN, DECIDE, DWORDS>), dim3((unsigned)blocks), dim3(CGC_BLOCK), 0, st, img, within, within_bytes, H, W,
                     radius, strips, rule, n, s, q, fg);
}

template <bool DECIDE>
int launch_window(const uint8_t* img, const void* within, int within_bytes, int H, int W, int radius, WinRule rule, int* n, int* s,
                  int64_t* q, uint8_t* fg, hipStream_t st) {
  flat_dispatch(within != nullptr, flat_dword_rows(img, within, within_bytes, W), [&](auto with, auto dwords) {
    launch_window_as<with.value, DECIDE, dwords.value>(img, within, with.value ? within_bytes : 0, H, W, radius, rule, n, s, q, fg, st);
  });
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // namespace

extern "C" int cgc_window_max_radius(void) { return WIN_MAX_RADIUS; }
extern "C" int cgc_window_tile_rows(void) { return WIN_ROWS; }
extern "C" int cgc_window_strip_cols(int radius) {
  return bad_flat_radius(radius, WIN_MAX_RADIUS) ? 0 : WIN_COLS - 2 * flat_halo(radius);
}

extern "C" int cgc_window_sums(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int radius, int* n, int* s,
                               int64_t* q, cgc_stream_t stream) {
  if (bad_flat_image(H, W, within_or_null, within_bytes) || bad_flat_radius(radius, WIN_MAX_RADIUS)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (img == nullptr || n == nullptr || s == nullptr || q == nullptr) return CGC_EINVAL;
  return launch_window<false>(img, within_or_null, within_bytes, H, W, radius, WinRule{0, 0, -1}, n, s, q, nullptr, as_stream(stream));
}

extern "C" int cgc_local_threshold(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int radius, int k64,
                                   int offset, int floor, uint8_t* out, cgc_stream_t stream) {
  if (bad_flat_image(H, W, within_or_null, within_bytes) || bad_flat_radius(radius, WIN_MAX_RADIUS)) return CGC_EINVAL;
  if (k64 < -128 || k64 > 128 || offset < -255 || offset > 255 || floor < -1 || floor > 255) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (img == nullptr || out == nullptr) return CGC_EINVAL;
  return launch_window<true>(img, within_or_null, within_bytes, H, W, radius, WinRule{k64, offset, floor}, nullptr, nullptr, nullptr, out,
                             as_stream(stream));
}
