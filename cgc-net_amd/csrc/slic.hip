// Superpixels on gfx950: KernelSpec.slic_iterate and KernelSpec.slic_merge; DESIGN.md, "Superpixels".
//
// SLIC (Achanta et al. 2012) restated in integers.  planes uint8 [C, H, W]; a grid of ny x nx cells, ny = max(1, (2 H + S) / (2 S));
// pixel (y, x) has HOME cell (y ny / H, x nx / W); centre k = i nx + j is a row (y, x, colours) of `centres` and starts in the middle
// of cell (i, j).  A ROUND is
//   k_slic_round     a workgroup per tile of SLIC_TILE x SLIC_TILE pixels, a thread 16 rows of one column (region.hip's standing).  A
//                    GATHER: a counted pixel looks at the centres of the up to 9 cells around its home cell, in ascending k, and keeps
//                    the first smallest D = S^2 sum_c (p_c - c_c)^2 + m^2 ((y - c_y)^2 + (x - c_x)^2), 64 bits.  No atomics decide
//                    anything.  The run of equal centres down a thread's column is summed in registers (count, y, x, colours) and
//                    folded into the tile's table in LDS, which goes to `acc` with one integer atomic per centre and quantity.
//   k_slic_finalize  a thread per centre: (2 sum + n) / (2 n) per coordinate and colour where n > 0; count[k] = n; acc[k] = 0 again.
// THE TABLE.  It holds the SLIC_TABLE x SLIC_TABLE cells whose first is one up and left of the home cell of the tile's first pixel,
// both the centres (read by the gather) and their sums (32 bits, coordinates relative to the tile).  A cell has at least H / ny >= 3
// rows, so a tile meets at most SLIC_TILE / (H / ny) + 2 home cells per axis and their neighbours two more: with cells of 8 pixels
// or more everything a tile reads and sums is in the table.  FALLBACK: a cell outside the table -- small steps -- is read from and
// summed into global memory directly, with the same integer additions on the same words, so which route a pixel takes changes no
// result.  `acc` is 64-bit: sum y over a centre's pixels passes 2^31 on a tall image.
//
// THE MERGE (connectivity of the final regions) works on the pieces of label.hip and the pair list of adjacency.hip:
//   k_slic_merge_begin    group[p] = p for a piece of min_size pixels or more (settled), 0 for a small one.
//   k_slic_merge_round    a thread per pair: a settled end offers itself to an unsettled one, key = count << 32 | ~q under an unsigned
//                         maximum: the largest count, of equal counts the smallest piece number q.  group[] is only read.
//   k_slic_merge_resolve  a thread per piece: an unsettled piece with an offer takes group[q]; q was settled before the round, so its
//                         entry does not change in this launch.  A round that settles nothing leaves everything as it was, so rounds
//                         past the last useful one are harmless, and the caller runs them in batches with one host read each.
//   k_slic_relabel        out = table[pieces], one launch.
// Integer work only; the additions and maxima are independent of the order of arrival.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int SLIC_TILE = 64;                                    // tile side (exported: the tests place seams from it)
constexpr int SLIC_BAND = SLIC_TILE * SLIC_TILE / CGC_BLOCK;     // 16 consecutive rows of one column per thread
constexpr int SLIC_TABLE = 12;                                   // cells per axis a tile folds in LDS (exported): 64 / 8 + 4
constexpr int SLIC_CELLS = SLIC_TABLE * SLIC_TABLE;
constexpr int SLIC_MAX_C = 4;
constexpr int SLIC_MIN_STEP = 4, SLIC_MAX_STEP = 256;            // (exported)
constexpr int SLIC_MAX_M = 1024, SLIC_MAX_ITER = 64;
constexpr int64_t SLIC_MAX_PIXELS = (int64_t)1 << 29;
constexpr int SLIC_CEN = 2 + SLIC_MAX_C, SLIC_ACC = 3 + SLIC_MAX_C;      // row widths in LDS; in global memory 2 + C and 3 + C
static_assert(SLIC_TILE == CGC_WAVE && SLIC_BAND * (CGC_BLOCK / CGC_WAVE) == SLIC_TILE, "a wave is one row of a tile, four bands");
static_assert(255 * SLIC_TILE * SLIC_TILE < (1 << 30), "a tile's sums of one centre fit int32");

struct SlicGrid {
  int C, H, W, ny, nx, K;
  int64_t s2, m2;                        // S^2, m^2
};

static inline int slic_cells(int n, int S) {                      // max(1, (2 n + S) / (2 S))
  const int64_t c = (2 * (int64_t)n + S) / (2 * (int64_t)S);
  return c < 1 ? 1 : (int)c;
}

__device__ __forceinline__ int slic_home(int p, int cells, int n) { return (int)((int64_t)p * cells / n); }      // 0 <= p < n

__global__ void __launch_bounds__(CGC_BLOCK) k_slic_init(const uint8_t* __restrict__ planes, SlicGrid g, int* __restrict__ centres,
                                                         u64* __restrict__ acc) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= g.K) return;
  const int i = k / g.nx, j = k - i * g.nx;
  const int y = (int)((2 * (int64_t)i + 1) * g.H / (2 * (int64_t)g.ny)), x = (int)((2 * (int64_t)j + 1) * g.W / (2 * (int64_t)g.nx));
  int* c = centres + (int64_t)k * (2 + g.C);
  c[0] = y;
  c[1] = x;
  const int64_t plane = (int64_t)g.H * g.W, at = (int64_t)y * g.W + x;      // y < H, x < W
  for (int q = 0; q < g.C; ++q) c[2 + q] = planes[q * plane + at];
  u64* a = acc + (int64_t)k * (3 + g.C);
  for (int q = 0; q < 3 + g.C; ++q) a[q] = 0;
}

struct SlicRun {                         // pixels of one centre down a thread's column
  int ci, cj, n, sy, sc[SLIC_MAX_C];     // sy: the sum of the rows, relative to the tile (the column is the thread's own)
};

template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_slic_round(const uint8_t* __restrict__ planes, const void* __restrict__ within, int wbytes,
                                                          SlicGrid g, int tiles_x, const int* __restrict__ centres, u64* __restrict__ acc,
                                                          int* __restrict__ labels) {      // labels: null but in the last round
  __shared__ int t_cen[SLIC_CELLS][SLIC_CEN];
  __shared__ int t_acc[SLIC_CELLS][SLIC_ACC];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy = ty * SLIC_TILE, ox = tx * SLIC_TILE;               // inside the image: the grid covers it exactly
  const int ci0 = slic_home(oy, g.ny, g.H) - 1, cj0 = slic_home(ox, g.nx, g.W) - 1;      // the table's first cell; may be -1
  const int C = g.C;
  for (int e = threadIdx.x; e < SLIC_CELLS; e += CGC_BLOCK) {
    const int ci = ci0 + e / SLIC_TABLE, cj = cj0 + e % SLIC_TABLE;
    if ((unsigned)ci < (unsigned)g.ny && (unsigned)cj < (unsigned)g.nx) {
      const int* c = centres + ((int64_t)ci * g.nx + cj) * (2 + C);
      for (int q = 0; q < 2 + C; ++q) t_cen[e][q] = c[q];
    }
    for (int q = 0; q < SLIC_ACC; ++q) t_acc[e][q] = 0;
  }
  __syncthreads();

  const int ly0 = (threadIdx.x / SLIC_TILE) * SLIC_BAND, lx = threadIdx.x & (SLIC_TILE - 1);
  const int y0 = oy + ly0, x = ox + lx;
  const int64_t plane = (int64_t)g.H * g.W;
  SlicRun run;
  run.n = 0;
  auto fold = [&]() {                                              // run.n > 0
    const unsigned wi = (unsigned)(run.ci - ci0), wj = (unsigned)(run.cj - cj0);
    if (wi < (unsigned)SLIC_TABLE && wj < (unsigned)SLIC_TABLE) {
      int* a = t_acc[wi * SLIC_TABLE + wj];
      atomicAdd(&a[0], run.n);
      atomicAdd(&a[1], run.sy);
      atomicAdd(&a[2], run.n * lx);
      for (int q = 0; q < C; ++q) atomicAdd(&a[3 + q], run.sc[q]);
    } else {                                                       // the fallback: the same sums, in image coordinates
      u64* a = acc + ((int64_t)run.ci * g.nx + run.cj) * (3 + C);
      atomicAdd(&a[0], (u64)run.n);
      atomicAdd(&a[1], (u64)((int64_t)run.sy + (int64_t)run.n * oy));
      atomicAdd(&a[2], (u64)((int64_t)run.n * x));
      for (int q = 0; q < C; ++q) atomicAdd(&a[3 + q], (u64)run.sc[q]);
    }
    run.n = 0;
  };
  if (x < g.W && y0 < g.H) {
    const int hx = slic_home(x, g.nx, g.W);
    int hy = slic_home(y0, g.ny, g.H);
    for (int r = 0; r < SLIC_BAND; ++r) {
      const int y = y0 + r;
      if (y >= g.H) break;
      while ((int64_t)(hy + 1) * g.H <= (int64_t)y * g.ny) ++hy;    // hy = y ny / H: it grows by at most one per row
      const int64_t at = (int64_t)y * g.W + x;
      const bool on = !WITHIN || image_nonzero(within, wbytes, at);
      int bi = 0, bj = 0;
      if (on) {
        int p[SLIC_MAX_C];
        for (int q = 0; q < C; ++q) p[q] = planes[q * plane + at];
        int64_t best = INT64_MAX;
        for (int ci = hy - 1; ci <= hy + 1; ++ci) {
          if ((unsigned)ci >= (unsigned)g.ny) continue;
          for (int cj = hx - 1; cj <= hx + 1; ++cj) {              // ascending k = ci nx + cj: of equal D the first one stays
            if ((unsigned)cj >= (unsigned)g.nx) continue;
            const unsigned wi = (unsigned)(ci - ci0), wj = (unsigned)(cj - cj0);
            int64_t dc = 0, dy, dx;
            if (wi < (unsigned)SLIC_TABLE && wj < (unsigned)SLIC_TABLE) {
              const int* c = t_cen[wi * SLIC_TABLE + wj];
              dy = y - c[0], dx = x - c[1];
              for (int q = 0; q < C; ++q) dc += (p[q] - c[2 + q]) * (p[q] - c[2 + q]);
            } else {
              const int* c = centres + ((int64_t)ci * g.nx + cj) * (2 + C);
              dy = y - c[0], dx = x - c[1];
              for (int q = 0; q < C; ++q) dc += (p[q] - c[2 + q]) * (p[q] - c[2 + q]);
            }
            const int64_t D = g.s2 * dc + g.m2 * (dy * dy + dx * dx);
            if (D < best) best = D, bi = ci, bj = cj;
          }
        }
        if (run.n != 0 && (run.ci != bi || run.cj != bj)) fold();
        if (run.n == 0) {
          run.ci = bi, run.cj = bj, run.sy = 0;
          for (int q = 0; q < SLIC_MAX_C; ++q) run.sc[q] = 0;
        }
        ++run.n;
        run.sy += ly0 + r;
        for (int q = 0; q < C; ++q) run.sc[q] += p[q];
      } else if (run.n != 0) {
        fold();
      }
      if (labels != nullptr) labels[at] = on ? bi * g.nx + bj + 1 : 0;
    }
    if (run.n != 0) fold();
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SLIC_CELLS; e += CGC_BLOCK) {
    const int n = t_acc[e][0];
    if (n == 0) continue;                                          // also every cell of the table that lies outside the grid
    const int ci = ci0 + e / SLIC_TABLE, cj = cj0 + e % SLIC_TABLE;
    u64* a = acc + ((int64_t)ci * g.nx + cj) * (3 + C);
    atomicAdd(&a[0], (u64)n);
    atomicAdd(&a[1], (u64)((int64_t)t_acc[e][1] + (int64_t)n * oy));
    atomicAdd(&a[2], (u64)((int64_t)t_acc[e][2] + (int64_t)n * ox));
    for (int q = 0; q < C; ++q) atomicAdd(&a[3 + q], (u64)t_acc[e][3 + q]);
  }
}

__global__ void __launch_bounds__(CGC_BLOCK) k_slic_finalize(SlicGrid g, u64* __restrict__ acc, int* __restrict__ centres,
                                                             int* __restrict__ count) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= g.K) return;
  u64* a = acc + (int64_t)k * (3 + g.C);
  const int64_t n = (int64_t)a[0];
  count[k] = (int)n;                                              // n <= H W < 2^29
  a[0] = 0;
  int* c = centres + (int64_t)k * (2 + g.C);
  for (int q = 0; q < 2 + g.C; ++q) {
    if (n > 0) c[q] = (int)((2 * (int64_t)a[1 + q] + n) / (2 * n));
    a[1 + q] = 0;
  }
}

__device__ __forceinline__ u64 merge_key(int count, int q) { return (u64)(uint32_t)count << 32 | (uint32_t)~q; }

__global__ void __launch_bounds__(CGC_BLOCK) k_slic_merge_begin(int n_pieces, const int* __restrict__ sizes, int min_size,
                                                                int* __restrict__ group, u64* __restrict__ best) {
  const int p = blockIdx.x * CGC_BLOCK + threadIdx.x;              // 0 .. n_pieces
  if (p > n_pieces) return;
  group[p] = p >= 1 && sizes[p - 1] >= min_size ? p : 0;
  best[p] = 0;
}

__global__ void __launch_bounds__(CGC_BLOCK) k_slic_merge_round(int64_t n_pairs, int n_pieces, const int* __restrict__ pairs,
                                                                const int* __restrict__ count, const int* __restrict__ group,
                                                                u64* __restrict__ best) {
  const int64_t t = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (t >= n_pairs) return;
  const int a = pairs[2 * t], b = pairs[2 * t + 1], n = count[t];
  if (a < 1 || a > n_pieces || b < 1 || b > n_pieces || n < 1) return;
  const bool sa = group[a] != 0, sb = group[b] != 0;
  if (sa && !sb) atomicMax(&best[b], merge_key(n, a));            // a key is never 0: n >= 1
  if (sb && !sa) atomicMax(&best[a], merge_key(n, b));
}

__global__ void __launch_bounds__(CGC_BLOCK) k_slic_merge_resolve(int n_pieces, int* __restrict__ group, u64* __restrict__ best,
                                                                  int* changed) {      // changed: null but in the last round
  const int p = blockIdx.x * CGC_BLOCK + threadIdx.x;
  bool moved = false;
  if (p >= 1 && p <= n_pieces) {
    const u64 k = best[p];
    if (k != 0) {
      const int q = (int)~(uint32_t)k;                             // settled before this round: 1 <= q <= n_pieces, group[q] != 0
      group[p] = group[q];
      best[p] = 0;
      moved = true;
    }
  }
  if (changed != nullptr) {
    const int m = (int)__popcll(__ballot(moved));
    if (m != 0 && (threadIdx.x & (CGC_WAVE - 1)) == 0) atomicAdd(changed, m);
  }
}

__global__ void __launch_bounds__(CGC_BLOCK) k_slic_relabel(int64_t n_pixels, int n_pieces, const int* __restrict__ pieces,
                                                            const int* __restrict__ table, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= n_pixels) return;
  const int p = pieces[i];
  out[i] = p >= 1 && p <= n_pieces ? table[p] : 0;
}

struct SlicWs {
  u64* acc;                              // [K, 3 + C] count, sum y, sum x, sums of the colours
};
static inline SlicWs slic_layout(Carver&& c, int64_t K, int C) {
  SlicWs w;
  w.acc = c.take<u64>(K * (3 + C));
  return w;
}

static inline bool bad_slic_image(int C, int H, int W, int step) {
  if (C < 1 || C > SLIC_MAX_C || step < SLIC_MIN_STEP || step > SLIC_MAX_STEP) return true;
  return bad_image_dims(H, W) || (int64_t)H * W >= SLIC_MAX_PIXELS;
}
static inline bool bad_piece_count(int n_pieces) { return n_pieces < 0 || n_pieces == 0x7fffffff; }
static inline dim3 slic_grid1(int64_t n) { return dim3((unsigned)ceil_div64(n, CGC_BLOCK)); }      // n < 2^31

}  // namespace

extern "C" int cgc_slic_max_step(void) { return SLIC_MAX_STEP; }
extern "C" int cgc_slic_tile_side(void) { return SLIC_TILE; }
extern "C" int cgc_slic_table_side(void) { return SLIC_TABLE; }

extern "C" int64_t cgc_slic_ws_bytes(int C, int H, int W, int step) {
  if (bad_slic_image(C, H, W, step)) return 0;
  return layout_bytes(slic_layout, (int64_t)slic_cells(H, step) * slic_cells(W, step), C);
}

extern "C" int cgc_slic_iterate(const uint8_t* planes, int C, int H, int W, int step, int compactness, int n_iter,
                                const void* within_or_null, int within_bytes, void* ws, int* labels, int* centres, int* count,
                                cgc_stream_t stream) {
  if (bad_slic_image(C, H, W, step) || compactness < 0 || compactness > SLIC_MAX_M || n_iter < 1 || n_iter > SLIC_MAX_ITER)
    return CGC_EINVAL;
  if (within_or_null != nullptr && bad_elem_bytes(within_bytes)) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (planes == nullptr || ws == nullptr || labels == nullptr || centres == nullptr || count == nullptr) return CGC_EINVAL;
  SlicGrid g;
  g.C = C, g.H = H, g.W = W, g.ny = slic_cells(H, step), g.nx = slic_cells(W, step);
  g.K = g.ny * g.nx;                                               // <= H W
  g.s2 = (int64_t)step * step, g.m2 = (int64_t)compactness * compactness;
  const SlicWs w = slic_layout(Carver(ws), g.K, C);
  hipStream_t st = as_stream(stream);
  const int tiles_x = ceil_div(W, SLIC_TILE);
  const dim3 tiles((unsigned)((int64_t)tiles_x * ceil_div(H, SLIC_TILE))), cells = slic_grid1(g.K), block(CGC_BLOCK);
  hipLaunchKernelGGL(k_slic_init, cells, block, 0, st, planes, g, centres, w.acc);
  CGC_RETURN_IF_LAUNCH_FAILED();
  for (int r = 0; r < n_iter; ++r) {
    int* out = r == n_iter - 1 ? labels : nullptr;
    if (within_or_null != nullptr)
      hipLaunchKernelGGL(k_slic_round<true>, tiles, block, 0, st, planes, within_or_null, within_bytes, g, tiles_x, centres, w.acc, out);
    else
      hipLaunchKernelGGL(k_slic_round<false>, tiles, block, 0, st, planes, within_or_null, 0, g, tiles_x, centres, w.acc, out);
    CGC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(k_slic_finalize, cells, block, 0, st, g, w.acc, centres, count);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_slic_merge_begin(const int* sizes, int n_pieces, int min_size, int* group, uint64_t* best, cgc_stream_t stream) {
  if (bad_piece_count(n_pieces) || min_size < 0 || group == nullptr || best == nullptr || (n_pieces > 0 && sizes == nullptr))
    return CGC_EINVAL;
  hipLaunchKernelGGL(k_slic_merge_begin, slic_grid1((int64_t)n_pieces + 1), dim3(CGC_BLOCK), 0, as_stream(stream), n_pieces, sizes,
                     min_size, group, reinterpret_cast<u64*>(best));
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_slic_merge_rounds(const int* pairs, const int* count, int64_t n_pairs, int n_pieces, int rounds, int* group,
                                     uint64_t* best, int* changed, cgc_stream_t stream) {
  if (bad_piece_count(n_pieces) || n_pairs < 0 || n_pairs >= ((int64_t)1 << 31) || rounds < 1 || rounds > 4096 || changed == nullptr)
    return CGC_EINVAL;
  if (n_pairs > 0 && (pairs == nullptr || count == nullptr || group == nullptr || best == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(changed, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (n_pairs == 0 || n_pieces == 0) return 0;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(k_slic_merge_round, slic_grid1(n_pairs), dim3(CGC_BLOCK), 0, st, n_pairs, n_pieces, pairs, count, group,
                       reinterpret_cast<u64*>(best));
    CGC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(k_slic_merge_resolve, slic_grid1((int64_t)n_pieces + 1), dim3(CGC_BLOCK), 0, st, n_pieces, group,
                       reinterpret_cast<u64*>(best), r == rounds - 1 ? changed : nullptr);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_slic_relabel(const int* pieces, int64_t n_pixels, int n_pieces, const int* table, int* out, cgc_stream_t stream) {
  if (bad_piece_count(n_pieces) || n_pixels < 0 || n_pixels >= ((int64_t)1 << 31)) return CGC_EINVAL;
  if (n_pixels == 0) return 0;
  if (pieces == nullptr || table == nullptr || out == nullptr) return CGC_EINVAL;
  hipLaunchKernelGGL(k_slic_relabel, slic_grid1(n_pixels), dim3(CGC_BLOCK), 0, as_stream(stream), n_pixels, n_pieces, pieces, table, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
