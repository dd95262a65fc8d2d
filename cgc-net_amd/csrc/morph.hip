// Flat grey-scale morphology of a uint8 image on gfx950: the minimum (ERODE), the maximum (DILATE) or both at once (GRADIENT, max - min)
// over a flat structuring element -- square, disk or diamond of radius r <= 63 -- clipped to the image and, if wanted, to the non-zero
// pixels of `within`, with an optional fused subtraction against a second image (the top-hats).  Contract item by item:
// cgc-net_amd/kernels.py KernelSpec.flat_morphology; design and measurements: DESIGN.md, "Flat morphology".
//
// ONE kernel, k_morph<WITHIN, DWORDS, GRADIENT>, one launch per call, no workspace, no atomics.  A workgroup owns a tile of MORPH_ROWS
// rows x cols(r) columns, cols(r) = MORPH_SPAN - 2 halo(r), halo(r) = r rounded up to a multiple of 4, and looks at the MORPH_SPAN = 256
// columns [x0 - halo, x0 - halo + 256) of the rows y0 - r .. y0 + MORPH_ROWS - 1 + r.
//   ONLY MAXIMA.  min v = 255 - max (255 - v): ERODE stores 255 - v in LDS and complements the result, so the table code knows one
//              operation and one neutral value, 0, which is also what a pixel outside the image or outside `within` is stored as.
//              GRADIENT keeps two tables, of v and of 255 - v: max - min = max v + max (255 - v) - 255, and 0 + 0 - 255 clamps to the 0
//              the contract wants where nothing is counted.
//   load       an LDS row is 256 bytes = the 64 dwords of one wave: wave u loads rows u, u + 4, ...  After it the image border and
//              `within` are gone from every later step.
//   levels     a footprint row dy is the run [x - w(dy), x + w(dy)] of row y + dy.  With M_k(y, x) = max over [x, x + 2^k) its maximum is
//              max(M_k(y + dy, x - w), M_k(y + dy, x + w + 1 - 2^k)), k = floor(log2(2 w + 1)).  The table starts as M_0 = the pixels and is
//              doubled IN PLACE, M_{k+1}(x) = max(M_k(x), M_k(x + 2^k)): a row belongs to one wave and is one dword per lane, so the
//              wave reads both operands of the whole row before it writes any of it.  Between two doublings every thread folds the
//              footprint rows of that level into the running maxima of its pixels (registers): two byte reads per footprint row and
//              pixel, consecutive lanes on consecutive bytes.  Entries whose run passes the right end of the 256 columns take 0 there;
//              no output reads them: x + w <= cols - 1 + halo + r <= 255.
//   epilogue   complement (ERODE) or the sum (GRADIENT), the optional subtraction against other[y, x], one byte stored.
// The halo, the loader of four pixels (flat_fetch, looked at straight away with flat_counted) and the launcher's choice DWORDS are
// image_window.hpp's, shared with window.hip and rank.hip: with W % 4 == 0, dword-aligned bases and a 1-byte `within` a lane's four
// pixels are all inside or all outside the image and are one dword load per plane; otherwise pixel by pixel -- same values, slower.
// The widths w(dy) are computed on the host in integers (flat_width there) and travel, sorted by level, as a kernel argument.
#include <stdint.h>

#include "common.hpp"
#include "image_window.hpp"

namespace {

constexpr int MORPH_MAX_RADIUS = 63;
constexpr int MORPH_ROWS = 32;                                  // output rows of a tile
constexpr int MORPH_SPAN = 256;                                 // columns a workgroup looks at = bytes of an LDS row
constexpr int MORPH_DWORDS = MORPH_SPAN / 4;                    // one per lane
constexpr int MORPH_WAVES = CGC_BLOCK / CGC_WAVE;
constexpr int MORPH_PPT = MORPH_ROWS * MORPH_SPAN / CGC_BLOCK;  // output pixels of a thread, at most (at cols = 256)
static_assert(MORPH_DWORDS == CGC_WAVE, "a wave owns whole LDS rows, one dword per lane");
static_assert(MORPH_SPAN - 2 * flat_halo(MORPH_MAX_RADIUS) >= MORPH_SPAN / 2, "the pixel walk below assumes cols >= 128");

__host__ __device__ __forceinline__ int morph_cols(int r) { return MORPH_SPAN - 2 * flat_halo(r); }
static inline int morph_lds_bytes(int r, bool gradient) { return (MORPH_ROWS + 2 * r) * MORPH_SPAN * (gradient ? 2 : 1); }

// The footprint as the kernel walks it: its rows sorted by the level of the table they are read from.  Dwords, so that the (uniform)
// reads of a workgroup are scalar loads from the kernel arguments.
constexpr int MORPH_LEVELS = 7;                                 // run lengths 1 .. 127: levels 0 .. 6
struct MorphFootprint {
  int start[MORPH_LEVELS + 1];                                  // rows of level k: entry[start[k]] .. entry[start[k + 1] - 1]
  uint32_t entry[2 * MORPH_MAX_RADIUS + 1];                     // (dy + r) << 8 | w(dy)
};
static_assert(2 * MORPH_MAX_RADIUS + 1 < (1 << MORPH_LEVELS), "a row's run length has a level");

typedef unsigned short morph_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t morph_pk_max(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(morph_u16x2, a), __builtin_bit_cast(morph_u16x2, b)));
}
// the maximum of four packed bytes, as two packed 16-bit maxima
__device__ __forceinline__ uint32_t morph_byte_max(uint32_t a, uint32_t b) {
  const uint32_t m = 0x00FF00FFu;
  return morph_pk_max(a & m, b & m) | (morph_pk_max((a >> 8) & m, (b >> 8) & m) << 8);
}

// The walk over a thread's output pixels: pixel number t + 256 j of the tile in raster order, j = 0 .. cols / 8 - 1 (32 cols pixels in
// all).  256 = cols + 2 halo and cols >= 128, so a step is one row down and 2 halo columns right, wrapping at most once.
struct MorphWalk {
  int row, col;
  __device__ __forceinline__ MorphWalk(int t, int cols) : row(t >= cols ? 1 : 0), col(t >= cols ? t - cols : t) {}
  __device__ __forceinline__ void step(int cols) {
    col += MORPH_SPAN - cols;
    row += 1;
    if (col >= cols) {
      col -= cols;
      row += 1;
    }
  }
};

// One footprint row, read as two table entries at byte offsets oa and ob from each pixel's base, into the pixels' running maxima.
// The pixels go in batches without a branch inside -- 16, then 8 and 8 more where the tile is wide enough -- so that a batch's LDS reads
// are all in flight together; a batch may run up to 7 pixels past nj: their base is 0, which is inside the table, and nothing stores
// them.
template <int J0, int J1>
__device__ __forceinline__ void morph_fold_batch(const uint8_t* tab, const int (&base)[MORPH_PPT], uint32_t (&acc)[MORPH_PPT], int oa,
                                                 int ob) {
#pragma unroll
  for (int j = J0; j < J1; ++j) {
    const uint32_t a = tab[base[j] + oa], b = tab[base[j] + ob];
    acc[j] = max(acc[j], max(a, b));
  }
}
__device__ __forceinline__ void morph_fold(const uint8_t* tab, const int (&base)[MORPH_PPT], uint32_t (&acc)[MORPH_PPT], int nj, int oa,
                                           int ob) {
  static_assert(MORPH_PPT == 32, "batches of 16 + 8 + 8; nj >= 16");
  morph_fold_batch<0, 16>(tab, base, acc, oa, ob);
  if (nj > 16) morph_fold_batch<16, 24>(tab, base, acc, oa, ob);        // uniform
  if (nj > 24) morph_fold_batch<24, 32>(tab, base, acc, oa, ob);
}

template <bool WITHIN, bool DWORDS, bool GRADIENT>
__global__ void __launch_bounds__(CGC_BLOCK) k_morph(const uint8_t* __restrict__ img, const void* __restrict__ within, int wbytes, int H, int W,
                                                     int r, int tiles_x, uint32_t flip, MorphFootprint fp,
                                                     const uint8_t* __restrict__ other, int epilogue, uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t morph_lds[];   // [tables][rows][64 dwords]
  constexpr int TABLES = GRADIENT ? 2 : 1;
  const int rows = MORPH_ROWS + 2 * r;
  const int halo = flat_halo(r), cols = MORPH_SPAN - 2 * halo;
  const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const int x0 = tile_x * cols, y0 = tile_y * MORPH_ROWS;               // x0 < W, y0 < H
  const int t = threadIdx.x, lane = t & (CGC_WAVE - 1), wave = t / CGC_WAVE;

  // ---- load: wave u takes rows u, u + 4, ...; what is not counted becomes 0
  {
    const int64_t xg = (int64_t)x0 - halo + 4 * lane;
#pragma unroll 4
    for (int row = wave; row < rows; row += MORPH_WAVES) {
      const FlatRow o = flat_fetch<WITHIN, DWORDS>(img, within, wbytes, H, W, xg, (int64_t)y0 - r + row);
      const uint32_t v = o.p, m = flat_counted<DWORDS>(o);             // 0xFF in every byte whose pixel is counted
      if (GRADIENT) {
        morph_lds[row * MORPH_DWORDS + lane] = v & m;
        morph_lds[(rows + row) * MORPH_DWORDS + lane] = ~v & m;
      } else {
        morph_lds[row * MORPH_DWORDS + lane] = (v ^ flip) & m;
      }
    }
  }

  // ---- this thread's pixels: byte offset of (row, col) in a table whose row 0 is image row y0 - r and column 0 image column x0 - halo,
  // taken at footprint offset (dy, dx) = (-r, -halo): adding (dy + r) * 256 + halo + dx reaches the pixel's neighbour.
  const int nj = cols / 8;                                              // 16 .. 32, the same for every thread
  int base[MORPH_PPT];
  uint32_t acc0[MORPH_PPT], acc1[GRADIENT ? MORPH_PPT : 1];             // running maxima of v (ERODE: of 255 - v) and, GRADIENT, of 255 - v
  {
    MorphWalk p(t, cols);
#pragma unroll
    for (int j = 0; j < MORPH_PPT; ++j) {
      base[j] = j < nj ? p.row * MORPH_SPAN + p.col : 0;
      p.step(cols);
      acc0[j] = 0;
      if (GRADIENT) acc1[j] = 0;
    }
  }
  __syncthreads();

  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(morph_lds);
  const int table_bytes = rows * MORPH_SPAN;
  const int kmax = 31 - __builtin_clz(2 * r + 1);
  for (int k = 0;; ++k) {
    const int run = 1 << k;
    // fold the footprint rows whose run length 2 w + 1 lies in [2^k, 2^(k+1)): the host has sorted them by level
    for (int i = fp.start[k]; i < fp.start[k + 1]; ++i) {
      const uint32_t e = fp.entry[i];                                   // uniform: a scalar load
      const int w = (int)(e & 255u);
      const int oa = (int)(e >> 8) * MORPH_SPAN + halo - w;             // >= 0: halo >= r >= w
      const int ob = oa + 2 * w + 1 - run;                              // oa <= ob; ob + run - 1 <= ... + halo + r <= 255 in the row
      morph_fold(bytes, base, acc0, nj, oa, ob);
      if constexpr (GRADIENT) morph_fold(bytes + table_bytes, base, acc1, nj, oa, ob);
    }
    if (k == kmax) break;
    __syncthreads();                                                    // every fold of level k is done
    // M_{k+1}(x) = max(M_k(x), M_k(x + 2^k)), in place: the wave reads a whole row, both operands, before it writes it
    // four rows at a time, every load before any store: the loads of the four rows overlap
    const int nrows = TABLES * rows;
    for (int row0 = wave; row0 < nrows; row0 += 4 * MORPH_WAVES) {
      uint32_t c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = row0 + u * MORPH_WAVES;
        const uint32_t* R = morph_lds + (row < nrows ? row : row0) * MORPH_DWORDS;
        const uint32_t a = R[lane];
        uint32_t b;
        if (run >= 4) {
          const int i = lane + run / 4;
          b = i < MORPH_DWORDS ? R[i < MORPH_DWORDS ? i : 0] : 0u;
        } else {
          const uint32_t next = lane + 1 < MORPH_DWORDS ? R[lane + 1 < MORPH_DWORDS ? lane + 1 : 0] : 0u;
          b = run == 1 ? (a >> 8) | (next << 24) : (a >> 16) | (next << 16);
        }
        c[u] = morph_byte_max(a, b);
      }
      __builtin_amdgcn_wave_barrier();                                  // no store of these rows is moved above their loads
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = row0 + u * MORPH_WAVES;
        if (row < nrows) morph_lds[row * MORPH_DWORDS + lane] = c[u];
      }
    }
    __syncthreads();
  }

  // ---- epilogue
  MorphWalk p(t, cols);
#pragma unroll
  for (int j = 0; j < MORPH_PPT; ++j) {
    const int y = y0 + p.row, x = x0 + p.col;
    if (j < nj && y < H && x < W) {
      const int i = y * W + x;
      int res;
      if (GRADIENT) {
        res = (int)acc0[j] + (int)acc1[GRADIENT ? j : 0] - 255;         // max v + max (255 - v) - 255; -255 where nothing is counted
        res = res > 0 ? res : 0;
      } else {
        res = (int)((acc0[j] ^ flip) & 255u);
      }
      if (epilogue == CGC_MORPH_OTHER_MINUS) res = (int)other[i] - res;
      if (epilogue == CGC_MORPH_MINUS_OTHER) res = res - (int)other[i];
      out[i] = (uint8_t)(res > 0 ? res : 0);
    }
    p.step(cols);
  }
}

struct MorphArgs {
  const uint8_t* img;
  const void* within;
  int within_bytes, H, W, radius, op;
  MorphFootprint fp;
  const uint8_t* other;
  int epilogue;
  uint8_t* out;
};

template <bool WITHIN, bool DWORDS, bool GRADIENT>
void launch_morph_as(const MorphArgs& a, hipStream_t st) {
  const int tiles_x = (int)ceil_div64(a.W, morph_cols(a.radius));
  const int64_t blocks = tiles_x * ceil_div64(a.H, MORPH_ROWS);         // < H W / (128 * 32) + H / 32 + W / 128 + 1 < 2^31
  auto* kernel = k_morph<WITHIN, DWORDS, GRADIENT>;
  if (GRADIENT) {                                                       // two tables pass the 64 KB default from r = 49 on
    static bool allowed[CGC_MAX_DEVICES];
    cgc_allow_lds(reinterpret_cast<const void*>(kernel), morph_lds_bytes(MORPH_MAX_RADIUS, true), allowed);
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CGC_BLOCK), (size_t)morph_lds_bytes(a.radius, GRADIENT), st, a.img, a.within,
                     a.within_bytes, a.H, a.W, a.radius, tiles_x, a.op == CGC_MORPH_ERODE ? 0xFFFFFFFFu : 0u, a.fp, a.other, a.epilogue,
                     a.out);
}

template <bool WITHIN, bool DWORDS>
void launch_morph_op(const MorphArgs& a, hipStream_t st) {
  if (a.op == CGC_MORPH_GRADIENT) launch_morph_as<WITHIN, DWORDS, true>(a, st);
  else launch_morph_as<WITHIN, DWORDS, false>(a, st);
}

}  // namespace

extern "C" int cgc_morph_max_radius(void) { return MORPH_MAX_RADIUS; }
extern "C" int cgc_morph_tile_rows(void) { return MORPH_ROWS; }
extern "C" int cgc_morph_tile_cols(int radius) { return bad_flat_radius(radius, MORPH_MAX_RADIUS) ? 0 : morph_cols(radius); }

extern "C" int cgc_morph_footprint_width(int kind, int radius, int dy) {
  if (bad_footprint(kind, radius, MORPH_MAX_RADIUS) || dy < -radius || dy > radius) return CGC_EINVAL;
  return flat_width(kind, radius, dy);
}

extern "C" int cgc_morph(const uint8_t* img, const void* within_or_null, int within_bytes, int H, int W, int kind, int radius, int op,
                         const uint8_t* other_or_null, int epilogue, uint8_t* out, cgc_stream_t stream) {
  if (bad_flat_image(H, W, within_or_null, within_bytes) || bad_footprint(kind, radius, MORPH_MAX_RADIUS)) return CGC_EINVAL;
  if (op < CGC_MORPH_ERODE || op > CGC_MORPH_GRADIENT || epilogue < CGC_MORPH_PLAIN || epilogue > CGC_MORPH_MINUS_OTHER) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (img == nullptr || out == nullptr || (epilogue != CGC_MORPH_PLAIN && other_or_null == nullptr)) return CGC_EINVAL;
  MorphArgs a{img, within_or_null, within_or_null != nullptr ? within_bytes : 0, H, W, radius, op, {}, other_or_null, epilogue, out};
  int n = 0;
  for (int k = 0; k < MORPH_LEVELS; ++k) {
    a.fp.start[k] = n;
    for (int dy = -radius; dy <= radius; ++dy) {
      const int w = flat_width(kind, radius, dy);
      if (31 - __builtin_clz((unsigned)(2 * w + 1)) == k) a.fp.entry[n++] = (uint32_t)(dy + radius) << 8 | (uint32_t)w;
    }
  }
  a.fp.start[MORPH_LEVELS] = n;                                         // = 2 radius + 1
  flat_dispatch(within_or_null != nullptr, flat_dword_rows(img, within_or_null, within_bytes, W), [&](auto with, auto dwords) {
    launch_morph_op<with.value, dwords.value>(a, as_stream(stream));
  });
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
