// Colour deconvolution and the 256-bin histogram ("F10", in front of the foreground map: an H&E tile -> a stain plane -> its Otsu
// threshold).  Two kernels:
//   1. k_stain_separate: Ruifrok-Johnston colour deconvolution in fixed point.  A lane takes 4 pixels = 12 bytes = three dwords of the
//      interleaved image and writes one dword per requested plane.  The optical-density table (256 int32, 1 KB) arrives as a kernel
//      argument and is copied to LDS, where every lane can index it; the 3 x 3 matrix stays in scalar registers.
//   2. k_histogram_u8: counts per workgroup in LDS, one global atomic per non-empty bin and workgroup at the end.  A flat tile -- every
//      lane on one bin -- is the worst case, so (a) a lane reads 16 consecutive pixels and adds a run of equal values with ONE LDS atomic,
//      and (b) every wave owns HIST_COPIES copies of the table, lane l using copy l % HIST_COPIES, laid out bin-major so that the
//      copies of one bin sit on different banks.  A flat tile then costs one atomic per 16 pixels and 8 lanes per address.
//   3. k_od_scan<MODE>: the reductions of stain estimation and normalisation (Macenko) over the pixels whose optical densities all
//      reach od_min.  One template, three bodies, the same loads as kernel 1 and the same OD table in LDS; a workgroup takes
//      SCAN_CHUNK consecutive pixels, 4 per lane and step, and flushes once.  SCAN_MOMENTS: the ten moments n, sum o_c, sum o_c o_d.  A lane meets at most
//      64 pixels, so its sums fit uint32 (64 * 5674^2 < 2^32); they are widened to 64 bits before the wave's shuffles, and ten lanes
//      add the workgroup's sums to the result with one vector 64-bit global atomic each.  SCAN_ANGLE: every pixel is projected on
//      a plane (two int32 dot products, rounded) and binned by the side of ANGLE_BINS - 1 directions it lies on -- ten steps of a
//      binary search over the table in LDS, integer cross products only.  Counters as in kernel 2: ANGLE_COPIES copies per
//      workgroup, bin-major, lane l on copy l % ANGLE_COPIES, and a lane adds a run of equal bins among the 16 pixels of a batch with
//      one atomic.  The loads of SCAN_BATCH steps are issued together and their 16 searches run side by side.  SCAN_CONC: the
//      concentrations of the first two stains (two int32 dot products each, rounded to 1/128 of a unit and clamped to CONC_BINS
//      levels) into 2 * CONC_BINS counters kept exactly as SCAN_ANGLE keeps its own, one open run per stain.
//   4. k_od_recolor: a 3 x 3 map in optical-density space and back to bytes.  Loads as kernel 1, stores their mirror image (three
//      dwords per lane, bytes on the tail); the OD table and the 6386-entry exponential table (as bytes, 6.4 KB) sit in LDS, the
//      matrix in scalar registers.  The exponential table is too large for kernel arguments: k_put_words carries it, as it carries
//      SCAN_ANGLE's directions, in two pieces of 3.2 KB into the caller's workspace, from where every workgroup copies it to LDS.
// The arithmetic, item by item: kernels.py KernelSpec.stain_separate / histogram_u8 / od_moments / angle_histogram /
// concentration_histogram / od_recolor.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

#define STAIN_THREADS 256
#define STAIN_OD_MAX 5674             // floor(1024 ln 255 + 0.5): the largest entry a table may hold
#define HIST_THREADS 256
#define HIST_LANE_PIXELS 16           // one 16-byte load per lane and step
#define HIST_STEPS 4
#define HIST_CHUNK (HIST_THREADS * HIST_LANE_PIXELS * HIST_STEPS)      // pixels of one workgroup: 16384
#define HIST_COPIES 8                 // private tables per wave
#define SCAN_THREADS 256
#define SCAN_STEPS 16                 // 4 pixels per lane and step: a lane meets 64 pixels
#define SCAN_BATCH 4                  // steps whose loads are issued together
#define SCAN_CHUNK (SCAN_THREADS * 4 * SCAN_STEPS)      // pixels of one workgroup: 16384
#define ANGLE_BINS 1024               // K: bins of the half turn (-pi/2, pi/2); ANGLE_BINS - 1 directions separate them
#define ANGLE_COPIES 8                // copies of the counters per workgroup
#define ANGLE_E_MAX 4096              // |E[j][c]|
#define ANGLE_E_REACH 7095            // sum_c |E[j][c]|: ceil(4096 sqrt 3)
#define ANGLE_DIR_MAX 16384           // |c_k|, |s_k|
#define PUT_WORDS 800                 // dwords one k_put_words launch carries as kernel arguments: 3.2 KB of the 4 KB there are
#define CONC_BINS 512                 // levels of one stain's concentration: 1/128 of a natural-log unit each, the last one open
#define EXP_LEN 6386                  // entries of the exponential table: floor(255 exp(-k / 1024) + 0.5) first reaches 0 at k = 6385
#define EXP_WORDS 1600                // the table as bytes, four to a dword, padded with zeros to whole 256-byte rows
#define RECOLOR_THREADS 256
#define RECOLOR_MAX_BLOCKS 2048       // 8 workgroups per CU: each copies 7.4 KB of tables to LDS once and strides over the tile
enum { SCAN_MOMENTS = 0, SCAN_ANGLE = 1, SCAN_CONC = 2 };
static_assert(4 * EXP_WORDS >= EXP_LEN && EXP_WORDS % 64 == 0, "the padded table holds every entry");
static_assert(PUT_WORDS <= 1024 && 4 * PUT_WORDS + 64 <= 4096 && EXP_WORDS <= 2 * PUT_WORDS && ANGLE_BINS - 1 <= 2 * PUT_WORDS,
              "a piece is one workgroup and fits the kernel arguments; either table is two pieces");
static_assert(2 * CONC_BINS <= ANGLE_BINS + 1, "the concentration counters fit the LDS the angle counters take");
static_assert(SCAN_STEPS % SCAN_BATCH == 0, "whole batches");
static_assert((uint64_t)SCAN_STEPS * 4 * STAIN_OD_MAX * STAIN_OD_MAX < ((uint64_t)1 << 32), "a lane's sums of products fit uint32");
static_assert((int64_t)STAIN_OD_MAX * ANGLE_E_REACH + 2048 < ((int64_t)1 << 26), "a projection fits 26 bits before the shift");
static_assert(2 * (int64_t)ANGLE_DIR_MAX * ((((int64_t)STAIN_OD_MAX * ANGLE_E_REACH + 2048) >> 12) + 1) < ((int64_t)1 << 31),
              "a cross product fits int32");

namespace {

struct StainTables {                   // passed by value: 1060 bytes of kernel arguments
  int lut[256];
  int m[9];                            // m[3 * c + s]: channel c (0 R, 1 G, 2 B) -> stain s
};

__device__ __forceinline__ uint32_t stain_level(int c) {      // (c + 2^15) >> 16, arithmetic, clamped to a byte
  const int v = (c + 32768) >> 16;
  return (uint32_t)min(max(v, 0), 255);
}

// The 12 bytes of the pixels i0 .. i0 + 3 of an interleaved image as three dwords (zeros past the end).
__device__ __forceinline__ void load_pixels4(const uint8_t* __restrict__ pix, int64_t npix, int64_t i0, bool as_dwords, uint32_t w[3]) {
  w[0] = w[1] = w[2] = 0u;
  if (as_dwords) {                     // all four pixels exist and the base is a multiple of 4 bytes
    const uint32_t* p = reinterpret_cast<const uint32_t*>(pix + 3 * i0);
    w[0] = p[0];
    w[1] = p[1];
    w[2] = p[2];
  } else {
    const int64_t nbytes = 3 * (npix - i0) < 12 ? 3 * (npix - i0) : 12;
    for (int k = 0; k < 12; ++k)
      if (k < nbytes) w[k >> 2] |= (uint32_t)pix[3 * i0 + k] << (8 * (k & 3));
  }
}

__device__ __forceinline__ int pixel_byte(const uint32_t w[3], int b) { return (int)((w[b >> 2] >> (8 * (b & 3))) & 255u); }

__global__ __launch_bounds__(STAIN_THREADS) void k_stain_separate(const uint8_t* __restrict__ pix, int64_t npix, int order,
                                                                  const StainTables t, int planes, uint8_t* __restrict__ out) {
  __shared__ int lut[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = t.lut[i];
  __syncthreads();
  const bool in_dwords = (reinterpret_cast<uintptr_t>(pix) & 3u) == 0;
  const int64_t groups = (npix + 3) >> 2;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = 4 * g;
    const bool full = i0 + 4 <= npix;
    uint32_t w[3];
    load_pixels4(pix, npix, i0, full && in_dwords, w);
    uint32_t packed[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int ch[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) ch[k] = pixel_byte(w, 3 * j + k);
      const int odr = lut[order == 0 ? ch[2] : ch[0]], odg = lut[ch[1]], odb = lut[order == 0 ? ch[0] : ch[2]];
#pragma unroll
      for (int s = 0; s < 3; ++s) packed[s] |= stain_level(odr * t.m[s] + odg * t.m[3 + s] + odb * t.m[6 + s]) << (8 * j);
    }
    int slot = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (((planes >> s) & 1) == 0) continue;      // uniform
      uint8_t* o = out + (int64_t)slot * npix + i0;
      ++slot;
      if (full && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(o) = packed[s];
      } else {
        for (int j = 0; j < 4; ++j)
          if (i0 + j < npix) o[j] = (uint8_t)(packed[s] >> (8 * j));
      }
    }
  }
}

// One workgroup counts the pixels [blockIdx.x * HIST_CHUNK, + HIST_CHUNK) into its LDS tables and adds what it found to hist.
__global__ __launch_bounds__(HIST_THREADS) void k_histogram_u8(const uint8_t* __restrict__ img, int64_t npix, const void* __restrict__ within,
                                                               int within_bytes, int* __restrict__ hist) {
  __shared__ int tab[HIST_THREADS / 64][256 * HIST_COPIES];
  for (int i = threadIdx.x; i < (HIST_THREADS / 64) * 256 * HIST_COPIES; i += HIST_THREADS) (&tab[0][0])[i] = 0;
  __syncthreads();
  int* mine = &tab[threadIdx.x >> 6][threadIdx.x & (HIST_COPIES - 1)];      // bin v of this lane's copy: mine[v * HIST_COPIES]
  const bool in_vectors = (reinterpret_cast<uintptr_t>(img) & 15u) == 0;
  const int64_t chunk0 = blockIdx.x * (int64_t)HIST_CHUNK;
  for (int step = 0; step < HIST_STEPS; ++step) {
    const int64_t i0 = chunk0 + ((int64_t)step * HIST_THREADS + threadIdx.x) * HIST_LANE_PIXELS;
    if (i0 >= npix) continue;
    const int n = npix - i0 < HIST_LANE_PIXELS ? (int)(npix - i0) : HIST_LANE_PIXELS;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (n == HIST_LANE_PIXELS && in_vectors) {
      const uint4 v = *reinterpret_cast<const uint4*>(img + i0);
      w[0] = v.x;
      w[1] = v.y;
      w[2] = v.z;
      w[3] = v.w;
    } else {
      for (int k = 0; k < HIST_LANE_PIXELS; ++k)
        if (k < n) w[k >> 2] |= (uint32_t)img[i0 + k] << (8 * (k & 3));
    }
    int cur = -1, run = 0;             // the open run of equal selected values
#pragma unroll
    for (int k = 0; k < HIST_LANE_PIXELS; ++k) {
      const bool counted = k < n && (within == nullptr || image_nonzero(within, within_bytes, i0 + k));
      const int v = counted ? (int)((w[k >> 2] >> (8 * (k & 3))) & 255u) : -1;
      if (v == cur) {
        ++run;
      } else {
        if (cur >= 0) atomicAdd(&mine[cur * HIST_COPIES], run);
        cur = v;
        run = 1;
      }
    }
    if (cur >= 0) atomicAdd(&mine[cur * HIST_COPIES], run);
  }
  __syncthreads();
  int total = 0;                       // thread v sums the copies of bin v
  for (int wv = 0; wv < HIST_THREADS / 64; ++wv)
    for (int c = 0; c < HIST_COPIES; ++c) total += tab[wv][threadIdx.x * HIST_COPIES + c];
  if (total != 0) atomicAdd(&hist[threadIdx.x], total);
}

struct ScanTables {                    // passed by value: 1052 bytes of kernel arguments
  int lut[256];
  int od_min;
  int e[6];                            // e[3 * j + c]: channel c (0 R, 1 G, 2 B) -> axis j of the plane (ANGLE only)
};

struct WordsPiece {                    // PUT_WORDS dwords of a table: packed directions (c & 0xffff) | (s << 16), or four bytes of exp_lut
  uint32_t d[PUT_WORDS];
};

// table[first + i] = piece.d[i]: a host table travels as kernel arguments, in pieces of 3.2 KB, into the caller's workspace.
__global__ __launch_bounds__(PUT_WORDS) void k_put_words(const WordsPiece piece, int first, int count, uint32_t* __restrict__ table) {
  if ((int)threadIdx.x < count) table[first + threadIdx.x] = piece.d[threadIdx.x];
}

// Bit j = pixel i0 + j of `img` is non-zero, j < n <= 4.
__device__ __forceinline__ uint32_t nonzero4(const void* __restrict__ img, int bytes, int64_t i0, int n) {
  const uint8_t* b = static_cast<const uint8_t*>(img) + i0;
  if (bytes == 1 && n == 4 && (reinterpret_cast<uintptr_t>(b) & 3u) == 0) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(b);
    return (uint32_t)((v & 0xffu) != 0) | (uint32_t)((v & 0xff00u) != 0) << 1 | (uint32_t)((v & 0xff0000u) != 0) << 2 |
           (uint32_t)((v & 0xff000000u) != 0) << 3;
  }
  uint32_t m = 0;
  for (int j = 0; j < 4; ++j)
    if (j < n && image_nonzero(img, bytes, i0 + j)) m |= 1u << j;
  return m;
}

typedef short short2v __attribute__((ext_vector_type(2)));
// a.lo * b.lo + a.hi * b.hi + c with the halves of a and b read as int16 (v_dot2c_i32_i16): exact while the sum fits int32
__device__ __forceinline__ int dot2_i16(uint32_t a, uint32_t b, int c) {
  short2v x, y;
  __builtin_memcpy(&x, &a, 4);
  __builtin_memcpy(&y, &b, 4);
  return __builtin_amdgcn_sdot2(x, y, c, false);
}

// One workgroup reduces the pixels [blockIdx.x * SCAN_CHUNK, + SCAN_CHUNK) and adds what it found to `out`: SCAN_MOMENTS int64 [10];
// SCAN_ANGLE int32 [ANGLE_BINS + 1] (bins, then the skipped counter); SCAN_CONC int32 [2 * CONC_BINS] (stain 0, then stain 1).
// dirs: ANGLE_BINS packed directions, entry 0 unused (SCAN_ANGLE only).  t.e: SCAN_ANGLE the basis, SCAN_CONC two columns of m.
template <int MODE>
__global__ __launch_bounds__(SCAN_THREADS) void k_od_scan(const uint8_t* __restrict__ pix, int64_t npix, int order, const ScanTables t,
                                                          const void* __restrict__ within, int within_bytes,
                                                          const uint32_t* __restrict__ dirs, void* __restrict__ out) {
  constexpr bool ANGLE = MODE == SCAN_ANGLE, CONC = MODE == SCAN_CONC;
  constexpr int COUNTERS = ANGLE ? ANGLE_BINS + 1 : (CONC ? 2 * CONC_BINS : 0);      // 0: sums, no counters
  __shared__ int lut[256];
  __shared__ uint32_t dir[ANGLE ? ANGLE_BINS : 1];
  __shared__ int tab[COUNTERS > 0 ? COUNTERS * ANGLE_COPIES : 1];
  __shared__ unsigned long long part[COUNTERS > 0 ? 1 : SCAN_THREADS / 64][10];
  for (int i = threadIdx.x; i < 256; i += SCAN_THREADS) lut[i] = t.lut[i];
  if constexpr (ANGLE)
    for (int i = threadIdx.x; i < ANGLE_BINS; i += SCAN_THREADS) dir[i] = i > 0 ? dirs[i] : 0u;
  if constexpr (COUNTERS > 0)
    for (int i = threadIdx.x; i < COUNTERS * ANGLE_COPIES; i += SCAN_THREADS) tab[i] = 0;
  __syncthreads();
  int* mine = &tab[COUNTERS > 0 ? threadIdx.x & (ANGLE_COPIES - 1) : 0];      // bin b of this lane's copy: mine[b * ANGLE_COPIES]
  uint32_t acc[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};          // moments: n, sR, sG, sB, RR, RG, RB, GG, GB, BB of this lane
  int skipped = 0;
  const bool in_dwords = (reinterpret_cast<uintptr_t>(pix) & 3u) == 0;
  const int64_t group0 = blockIdx.x * (int64_t)(SCAN_CHUNK / 4);
  for (int s0 = 0; s0 < SCAN_STEPS; s0 += SCAN_BATCH) {
    // the loads of SCAN_BATCH steps first, then their arithmetic: a workgroup per 16384 pixels leaves ~3 waves per SIMD, too few to
    // hide a global load per step behind the others' work
    uint32_t w[SCAN_BATCH][3], live[SCAN_BATCH];      // live: bit j = pixel j of the step exists and lies inside `within`
    if (4 * (group0 + (int64_t)s0 * SCAN_THREADS + threadIdx.x) >= npix) break;      // i0 grows with the step
#pragma unroll
    for (int u = 0; u < SCAN_BATCH; ++u) {
      const int64_t i0 = 4 * (group0 + (int64_t)(s0 + u) * SCAN_THREADS + threadIdx.x);
      const int n = npix - i0 >= 4 ? 4 : (npix - i0 > 0 ? (int)(npix - i0) : 0);
      load_pixels4(pix, npix, i0, n == 4 && in_dwords, w[u]);
      live[u] = ((1u << n) - 1u) & (within == nullptr ? 15u : nonzero4(within, within_bytes, i0, n));
    }
    if constexpr (CONC) {
      int cur[2] = {-1, -1}, run[2] = {0, 0};      // the open run of equal bins, per stain
#pragma unroll
      for (int q = 0; q < 4 * SCAN_BATCH; ++q) {
        const uint32_t* wq = w[q >> 2];
        const int j = q & 3;
        const int c0 = pixel_byte(wq, 3 * j), c1 = pixel_byte(wq, 3 * j + 1), c2 = pixel_byte(wq, 3 * j + 2);
        const int odr = lut[order == 0 ? c2 : c0], odg = lut[c1], odb = lut[order == 0 ? c0 : c2];
        const bool sel = ((live[q >> 2] >> j) & 1u) != 0 && min(min(odr, odg), odb) >= t.od_min;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          // |m| < 2^23 and every product and sum fits int32 (the entry's refusal): the 24-bit multiplies are exact
          const int c = __mul24(odr, t.e[3 * s]) + __mul24(odg, t.e[3 * s + 1]) + __mul24(odb, t.e[3 * s + 2]);
          const int v = sel ? CONC_BINS * s + min(max((c + 16384) >> 15, 0), CONC_BINS - 1) : -1;
          if (v == cur[s]) {
            ++run[s];
          } else {
            if (cur[s] >= 0) atomicAdd(&mine[cur[s] * ANGLE_COPIES], run[s]);
            cur[s] = v;
            run[s] = 1;
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (cur[s] >= 0) atomicAdd(&mine[cur[s] * ANGLE_COPIES], run[s]);
    } else if constexpr (!ANGLE) {
#pragma unroll
      for (int q = 0; q < 4 * SCAN_BATCH; ++q) {
        const uint32_t* wq = w[q >> 2];
        const int j = q & 3;
        const int c0 = pixel_byte(wq, 3 * j), c1 = pixel_byte(wq, 3 * j + 1), c2 = pixel_byte(wq, 3 * j + 2);
        const int odr = lut[order == 0 ? c2 : c0], odg = lut[c1], odb = lut[order == 0 ? c0 : c2];
        const bool sel = ((live[q >> 2] >> j) & 1u) != 0 && min(min(odr, odg), odb) >= t.od_min;
        const uint32_t r = sel ? (uint32_t)odr : 0u, g = sel ? (uint32_t)odg : 0u, b = sel ? (uint32_t)odb : 0u;      // < 2^13
        acc[0] += (uint32_t)sel;
        acc[1] += r;
        acc[2] += g;
        acc[3] += b;
        acc[4] += __umul24(r, r);
        acc[5] += __umul24(r, g);
        acc[6] += __umul24(r, b);
        acc[7] += __umul24(g, g);
        acc[8] += __umul24(g, b);
        acc[9] += __umul24(b, b);
      }
    } else {
      int p1[4 * SCAN_BATCH];
      uint32_t side[4 * SCAN_BATCH], lo[4 * SCAN_BATCH];      // side: (-p_2, p_1) as two int16; lo: 4 * the count so far, an LDS offset
      uint32_t chosen = 0;             // bit q = pixel q of the batch is selected
#pragma unroll
      for (int q = 0; q < 4 * SCAN_BATCH; ++q) {
        const uint32_t* wq = w[q >> 2];
        const int j = q & 3;
        const int c0 = pixel_byte(wq, 3 * j), c1 = pixel_byte(wq, 3 * j + 1), c2 = pixel_byte(wq, 3 * j + 2);
        const int odr = lut[order == 0 ? c2 : c0], odg = lut[c1], odb = lut[order == 0 ? c0 : c2];
        if (((live[q >> 2] >> j) & 1u) != 0 && min(min(odr, odg), odb) >= t.od_min) chosen |= 1u << q;
        // every factor fits 24 bits and every sum int32 (the static_asserts above); an unselected pixel is searched like any other
        p1[q] = (__mul24(odr, t.e[0]) + __mul24(odg, t.e[1]) + __mul24(odb, t.e[2]) + 2048) >> 12;
        const int p2 = (__mul24(odr, t.e[3]) + __mul24(odg, t.e[4]) + __mul24(odb, t.e[5]) + 2048) >> 12;
        side[q] = ((uint32_t)(-p2) & 0xffffu) | (uint32_t)p1[q] << 16;      // |p_j| <= 9829: both fit int16
        lo[q] = 0;                     // the directions 1 .. lo / 4 have the pixel on their left: a prefix (the entry checks the table)
      }
#pragma unroll
      for (int half = ANGLE_BINS / 2; half >= 1; half >>= 1) {      // the 16 searches side by side: 16 LDS reads in flight per level
#pragma unroll
        for (int q = 0; q < 4 * SCAN_BATCH; ++q) {
          const uint32_t d = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(dir) + lo[q] + 4 * half);
          // (c, s) . (-p_2, p_1) - 1 = -(c p_2 - s p_1) - 1, exact in int32: negative iff the cross product is >= 0
          const int below = dot2_i16(d, side[q], -1);
          lo[q] |= (uint32_t)(below >> 31) & (uint32_t)(4 * half);
        }
      }
      int cur = -1, run = 0;           // the open run of equal bins
#pragma unroll
      for (int q = 0; q < 4 * SCAN_BATCH; ++q) {
        const bool sel = ((chosen >> q) & 1u) != 0;
        skipped += (int)(sel && p1[q] <= 0);
        const int v = sel && p1[q] > 0 ? (int)(lo[q] >> 2) : -1;
        if (v == cur) {
          ++run;
        } else {
          if (cur >= 0) atomicAdd(&mine[cur * ANGLE_COPIES], run);
          cur = v;
          run = 1;
        }
      }
      if (cur >= 0) atomicAdd(&mine[cur * ANGLE_COPIES], run);
    }
  }
  if constexpr (COUNTERS > 0) {
    if constexpr (ANGLE)
      if (skipped != 0) atomicAdd(&mine[ANGLE_BINS * ANGLE_COPIES], skipped);
    __syncthreads();
    int* hist = static_cast<int*>(out);
    for (int b = threadIdx.x; b < COUNTERS; b += SCAN_THREADS) {
      int total = 0;
      for (int c = 0; c < ANGLE_COPIES; ++c) total += tab[b * ANGLE_COPIES + c];
      if (total != 0) atomicAdd(&hist[b], total);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 10; ++k) {     // 64 bits from here on: a wave's sum of products reaches 2^37
      unsigned long long v = acc[k];
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
      unsigned long long total = 0;
      for (int wv = 0; wv < SCAN_THREADS / 64; ++wv) total += part[wv][threadIdx.x];
      if (total != 0) atomicAdd(static_cast<unsigned long long*>(out) + threadIdx.x, total);      // the sums are >= 0: int64 = uint64
    }
  }
}

// out[i][d] = exp_lut[clamp((sum_c lut[v_c] a[c][d] + 2^11) >> 12, 0, EXP_LEN - 1)], in the channel order of the input.  t.m holds a.
// exp_words: the table as bytes, EXP_WORDS dwords (k_put_words wrote them).
__global__ __launch_bounds__(RECOLOR_THREADS) void k_od_recolor(const uint8_t* __restrict__ pix, int64_t npix, int order, const StainTables t,
                                                                const uint32_t* __restrict__ exp_words, uint8_t* __restrict__ out) {
  __shared__ int lut[256];
  __shared__ uint32_t exp_tab[EXP_WORDS];
  for (int i = threadIdx.x; i < 256; i += RECOLOR_THREADS) lut[i] = t.lut[i];
  for (int i = threadIdx.x; i < EXP_WORDS; i += RECOLOR_THREADS) exp_tab[i] = exp_words[i];
  __syncthreads();
  const uint8_t* exp_lut = reinterpret_cast<const uint8_t*>(exp_tab);
  const bool in_dwords = (reinterpret_cast<uintptr_t>(pix) & 3u) == 0, out_dwords = (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  const int64_t groups = (npix + 3) >> 2;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = 4 * g;
    const bool full = i0 + 4 <= npix;
    uint32_t w[3];
    load_pixels4(pix, npix, i0, full && in_dwords, w);
    uint32_t packed[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int ch[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) ch[k] = pixel_byte(w, 3 * j + k);
      const int odr = lut[order == 0 ? ch[2] : ch[0]], odg = lut[ch[1]], odb = lut[order == 0 ? ch[0] : ch[2]];
      uint32_t lev[3];                 // the output channels R, G, B
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        // |a| < 2^23 and every product and sum fits int32 (the entry's refusal): the 24-bit multiplies are exact
        const int o = __mul24(odr, t.m[d]) + __mul24(odg, t.m[3 + d]) + __mul24(odb, t.m[6 + d]);
        lev[d] = exp_lut[min(max((o + 2048) >> 12, 0), EXP_LEN - 1)];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int b = 3 * j + k;       // byte b of the 12: channel k of pixel j, R and B swapped for the BGR order
        packed[b >> 2] |= (order == 0 ? lev[2 - k] : lev[k]) << (8 * (b & 3));
      }
    }
    uint8_t* o = out + 3 * i0;
    if (full && out_dwords) {
      uint32_t* p = reinterpret_cast<uint32_t*>(o);
      p[0] = packed[0];
      p[1] = packed[1];
      p[2] = packed[2];
    } else {
      const int64_t nbytes = 3 * (npix - i0) < 12 ? 3 * (npix - i0) : 12;
      for (int k = 0; k < 12; ++k)
        if (k < nbytes) o[k] = (uint8_t)(packed[k >> 2] >> (8 * (k & 3)));
    }
  }
}

}  // namespace

static inline bool bad_pixel_count(int64_t npix) { return npix < 0 || npix >= ((int64_t)1 << 31); }      // bad_image_dims, for a flat count

// No int32 sum over a column of a 3 x 3 matrix of optical densities may overflow, its rounding term included:
// sum_c |m[c][s]| * 5674 < 2^31 - slack for every column s.
static bool bad_od_matrix(const int* m, int64_t slack) {
  for (int s = 0; s < 3; ++s) {
    int64_t reach = 0;
    for (int c = 0; c < 3; ++c) reach += (m[3 * c + s] < 0 ? -(int64_t)m[3 * c + s] : (int64_t)m[3 * c + s]) * STAIN_OD_MAX;
    if (reach >= ((int64_t)1 << 31) - slack) return true;
  }
  return false;
}

// table[first + i] = words[i], i < n, on the stream: ceil(n / PUT_WORDS) launches of k_put_words.
static int put_words(const uint32_t* words, int first, int n, uint32_t* table, hipStream_t st) {
  for (int at = 0; at < n; at += PUT_WORDS) {
    WordsPiece piece;
    const int count = n - at < PUT_WORDS ? n - at : PUT_WORDS;
    for (int i = 0; i < PUT_WORDS; ++i) piece.d[i] = i < count ? words[at + i] : 0u;
    hipLaunchKernelGGL(k_put_words, dim3(1), dim3(PUT_WORDS), 0, st, piece, first + at, count, table);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_stain_separate(const uint8_t* pix, int64_t npix, int order, const int* lut, const int* m, int planes, uint8_t* out,
                                  cgc_stream_t stream) {
  if (bad_pixel_count(npix) || (order != 0 && order != 1) || lut == nullptr || m == nullptr || planes < 1 || planes > 7)
    return CGC_EINVAL;
  StainTables t;
  for (int v = 0; v < 256; ++v) {
    if (lut[v] < 0 || lut[v] > STAIN_OD_MAX) return CGC_EINVAL;
    t.lut[v] = lut[v];
  }
  if (bad_od_matrix(m, 32768)) return CGC_EINVAL;
  for (int k = 0; k < 9; ++k) t.m[k] = m[k];
  if (npix == 0) return 0;
  if (pix == nullptr || out == nullptr) return CGC_EINVAL;
  const int64_t nb = ceil_div64(ceil_div64(npix, 4), STAIN_THREADS);
  hipLaunchKernelGGL(k_stain_separate, dim3((int)(nb < 4096 ? nb : 4096)), dim3(STAIN_THREADS), 0, as_stream(stream), pix, npix, order, t,
                     planes, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_histogram_chunk_pixels(void) { return HIST_CHUNK; }

extern "C" int cgc_histogram_u8(const uint8_t* img, int64_t npix, const void* within_or_null, int within_bytes, int* hist,
                                cgc_stream_t stream) {
  if (bad_pixel_count(npix) || hist == nullptr || (within_or_null != nullptr && bad_elem_bytes(within_bytes)) ||
      (npix > 0 && img == nullptr))
    return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(hist, 0, 256 * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (npix == 0) return 0;
  hipLaunchKernelGGL(k_histogram_u8, dim3((int)ceil_div64(npix, HIST_CHUNK)), dim3(HIST_THREADS), 0, st, img, npix, within_or_null,
                     within_bytes, hist);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

// What cgc_od_moments and cgc_angle_histogram share: the image, the table, the threshold, the selection.  Fills t.lut and t.od_min.
static bool bad_scan_args(int64_t npix, int order, const int* lut, int od_min, const void* within_or_null, int within_bytes,
                          const void* out, ScanTables& t) {
  if (bad_pixel_count(npix) || (order != 0 && order != 1) || lut == nullptr || od_min < 0 || od_min > STAIN_OD_MAX || out == nullptr ||
      (within_or_null != nullptr && bad_elem_bytes(within_bytes)))
    return true;
  for (int v = 0; v < 256; ++v) {
    if (lut[v] < 0 || lut[v] > STAIN_OD_MAX) return true;
    t.lut[v] = lut[v];
  }
  t.od_min = od_min;
  for (int k = 0; k < 6; ++k) t.e[k] = 0;
  return false;
}

extern "C" int cgc_scan_chunk_pixels(void) { return SCAN_CHUNK; }

extern "C" int cgc_od_moments(const uint8_t* pix, int64_t npix, int order, const int* lut, int od_min, const void* within_or_null,
                              int within_bytes, int64_t* out, cgc_stream_t stream) {
  ScanTables t;
  if (bad_scan_args(npix, order, lut, od_min, within_or_null, within_bytes, out, t) || (npix > 0 && pix == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(out, 0, 10 * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  if (npix == 0) return 0;
  hipLaunchKernelGGL(k_od_scan<SCAN_MOMENTS>, dim3((int)ceil_div64(npix, SCAN_CHUNK)), dim3(SCAN_THREADS), 0, st, pix, npix, order, t,
                     within_or_null, within_bytes, (const uint32_t*)nullptr, (void*)out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_angle_bins(void) { return ANGLE_BINS; }
extern "C" int64_t cgc_angle_histogram_ws_bytes(void) { return ANGLE_BINS * (int64_t)sizeof(uint32_t); }

extern "C" int cgc_angle_histogram(const uint8_t* pix, int64_t npix, int order, const int* lut, int od_min, const int* basis,
                                   const int* dirs, const void* within_or_null, int within_bytes, void* ws, int* out,
                                   cgc_stream_t stream) {
  ScanTables t;
  if (bad_scan_args(npix, order, lut, od_min, within_or_null, within_bytes, out, t) || basis == nullptr || dirs == nullptr)
    return CGC_EINVAL;
  for (int j = 0; j < 2; ++j) {        // |sum_c o_c E[j][c]| <= 5674 * 7095 < 2^26
    int reach = 0;
    for (int c = 0; c < 3; ++c) {
      const int v = basis[3 * j + c];
      if (v < -ANGLE_E_MAX || v > ANGLE_E_MAX) return CGC_EINVAL;
      reach += v < 0 ? -v : v;
      t.e[3 * j + c] = v;
    }
    if (reach > ANGLE_E_REACH) return CGC_EINVAL;
  }
  // The directions k = 1 .. K - 1 lie in the open right half plane and turn left from one to the next: for a pixel with p_1 > 0 the
  // set {k : c_k p_2 - s_k p_1 >= 0} is then a prefix, and the kernel's binary search finds its size.
  for (int k = 0; k < ANGLE_BINS - 1; ++k) {
    const int c = dirs[2 * k], s = dirs[2 * k + 1];
    if (c <= 0 || c > ANGLE_DIR_MAX || s < -ANGLE_DIR_MAX || s > ANGLE_DIR_MAX) return CGC_EINVAL;
    if (k + 1 < ANGLE_BINS - 1 && (int64_t)c * dirs[2 * k + 3] - (int64_t)s * dirs[2 * k + 2] <= 0) return CGC_EINVAL;
  }
  if (npix > 0 && (pix == nullptr || ws == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(out, 0, (ANGLE_BINS + 1) * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (npix == 0) return 0;
  uint32_t* table = static_cast<uint32_t*>(ws);      // entry k = direction k; entry 0 is never read
  uint32_t packed[ANGLE_BINS - 1];
  for (int k = 0; k < ANGLE_BINS - 1; ++k) packed[k] = ((uint32_t)dirs[2 * k] & 0xffffu) | (uint32_t)dirs[2 * k + 1] << 16;
  const int put = put_words(packed, 1, ANGLE_BINS - 1, table, st);
  if (put != 0) return put;
  hipLaunchKernelGGL(k_od_scan<SCAN_ANGLE>, dim3((int)ceil_div64(npix, SCAN_CHUNK)), dim3(SCAN_THREADS), 0, st, pix, npix, order, t,
                     within_or_null, within_bytes, (const uint32_t*)table, (void*)out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_concentration_bins(void) { return CONC_BINS; }

extern "C" int cgc_concentration_histogram(const uint8_t* pix, int64_t npix, int order, const int* lut, int od_min, const int* m,
                                           const void* within_or_null, int within_bytes, int* out, cgc_stream_t stream) {
  ScanTables t;
  if (bad_scan_args(npix, order, lut, od_min, within_or_null, within_bytes, out, t) || m == nullptr || bad_od_matrix(m, 32768))
    return CGC_EINVAL;
  for (int s = 0; s < 2; ++s)
    for (int c = 0; c < 3; ++c) t.e[3 * s + c] = m[3 * c + s];
  if (npix > 0 && pix == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(out, 0, 2 * CONC_BINS * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (npix == 0) return 0;
  hipLaunchKernelGGL(k_od_scan<SCAN_CONC>, dim3((int)ceil_div64(npix, SCAN_CHUNK)), dim3(SCAN_THREADS), 0, st, pix, npix, order, t,
                     within_or_null, within_bytes, (const uint32_t*)nullptr, (void*)out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_exp_lut_len(void) { return EXP_LEN; }
extern "C" int64_t cgc_od_recolor_ws_bytes(void) { return EXP_WORDS * (int64_t)sizeof(uint32_t); }

extern "C" int cgc_od_recolor(const uint8_t* pix, int64_t npix, int order, const int* lut, const int* a, const int* exp_lut, int exp_len,
                              void* ws, uint8_t* out, cgc_stream_t stream) {
  if (bad_pixel_count(npix) || (order != 0 && order != 1) || lut == nullptr || a == nullptr || exp_lut == nullptr || exp_len != EXP_LEN)
    return CGC_EINVAL;
  StainTables t;
  for (int v = 0; v < 256; ++v) {
    if (lut[v] < 0 || lut[v] > STAIN_OD_MAX) return CGC_EINVAL;
    t.lut[v] = lut[v];
  }
  if (bad_od_matrix(a, 2048)) return CGC_EINVAL;
  for (int k = 0; k < 9; ++k) t.m[k] = a[k];
  // 255 first, 0 last, never rising: a byte for every k the kernel's clamp can reach
  if (exp_lut[0] != 255 || exp_lut[EXP_LEN - 1] != 0) return CGC_EINVAL;
  uint32_t words[EXP_WORDS] = {0u};
  for (int k = 0; k < EXP_LEN; ++k) {
    if (exp_lut[k] < 0 || exp_lut[k] > 255 || (k > 0 && exp_lut[k] > exp_lut[k - 1])) return CGC_EINVAL;
    words[k >> 2] |= (uint32_t)exp_lut[k] << (8 * (k & 3));
  }
  if (npix == 0) return 0;
  if (pix == nullptr || ws == nullptr || out == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  uint32_t* table = static_cast<uint32_t*>(ws);
  const int put = put_words(words, 0, EXP_WORDS, table, st);
  if (put != 0) return put;
  const int64_t nb = ceil_div64(ceil_div64(npix, 4), RECOLOR_THREADS);
  hipLaunchKernelGGL(k_od_recolor, dim3((int)(nb < RECOLOR_MAX_BLOCKS ? nb : RECOLOR_MAX_BLOCKS)), dim3(RECOLOR_THREADS), 0, st, pix, npix,
                     order, t, (const uint32_t*)table, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
