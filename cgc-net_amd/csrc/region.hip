// Region statistics of a label image on gfx950: per label value the count, sum, sum of squares, extrema with their positions
// (MOMENTS) or the 256-bin histogram (HISTOGRAM) of a second plane over the label's pixels, and quantiles read off such histograms
// (QUANTILES).  Contract item by item: cgc-net_amd/kernels.py KernelSpec.region_statistics / region_histogram / region_quantiles;
// design and measurements: DESIGN.md, "Region statistics".
//
// A pixel p is *counted* in row L iff labels[p] == L, 0 <= L <= max_label, and within is null or non-zero at p.  A pixel whose label
// lies outside [0, max_label] is counted nowhere and adds one to *meta, whatever `within` says there.
// Launches of one MOMENTS call:
//   k_region_init      count = sum = sumsq = 0, the two key tables of the workspace to "nothing yet", *meta = 0
//   k_region_moments   one 64 x 64 tile per workgroup.  A thread owns 16 consecutive rows of one column: all its loads are issued
//                      before the first is looked at, and a run of equal labels down the column is summed in registers.  A finished run
//                      is folded into an LDS table keyed by label (REGION_SLOTS slots, LDS atomics); after a barrier every claimed slot
//                      goes to the global tables with one integer atomic per quantity.
//   k_region_finish    keys -> min, max, argmin, argmax; the values of an empty row
// HISTOGRAM: hipMemsetAsync, then k_region_hist -- the same tile, table and walk, with 256 16-bit bins per slot (two per dword; a bin
// holds at most the 4096 pixels of a tile) and one LDS atomic per counted pixel; a claimed slot is flushed as 256 consecutive counters.
// COOCCURRENCE (KernelSpec.region_cooccurrence; DESIGN.md, "Region co-occurrence"): hipMemsetAsync, then one k_region_cooc per offset
// -- k_region_hist with a pair of pixels (anchor, partner) where the histogram has one, and a bin per pair of levels.
// GEOMETRY (KernelSpec.region_geometry; DESIGN.md, "Region geometry"): k_geometry_init, k_region_geometry -- the same tile and table;
// the labels alone, staged in LDS with a frame of one position; runs folded by closed forms in tile coordinates, quads classified
// where their four positions differ -- and k_geometry_finish for the extents of empty rows.
// OVERFLOW.  region_slot() probes at most REGION_PROBES <= REGION_SLOTS slots and never waits: a label that finds neither itself nor
// an empty slot there is sent to the global tables directly (a run at a time in MOMENTS, a pixel at a time in HISTOGRAM).  Both routes
// end in the same integer atomics on the same global words, so which pixels take which route -- it depends on the order in which lanes
// arrive -- changes no result: integer sums, and minima / maxima of 64-bit keys, are independent of order.  A tile in which every pixel
// has its own label is an ordinary input: 64 labels fold, the rest go direct.
// EXTREMA.  The value and its position travel as one key: min key = (v ^ 0x80000000) << 32 | i, combined by unsigned min; max key =
// (v ^ 0x80000000) << 32 | ~i, combined by unsigned max -- of equal values the smallest raster index i wins in both, in a thread's
// run (i grows down the column, strict comparisons), in LDS and in global memory.  No key equals the initial ~0 / 0: i < 2^31.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"
#include "rank_scan.hpp"

namespace {

constexpr int REGION_TILE = 64;                                  // tile side (exported: the tests place seams from it)
constexpr int REGION_BAND = REGION_TILE * REGION_TILE / CGC_BLOCK;      // 16 consecutive rows of one column per thread
constexpr int REGION_SLOT_BITS = 6;
constexpr int REGION_SLOTS = 1 << REGION_SLOT_BITS;              // labels a tile folds in LDS (exported)
constexpr int REGION_PROBES = 8;                                 // slots a label looks at before it goes to global memory
constexpr int REGION_EMPTY = -1;                                 // no label: only labels in [0, max_label] reach the table
constexpr int REGION_MAX_Q = 8;
constexpr int REGION_INIT_BLOCKS = 4096;
constexpr unsigned long long REGION_NO_MIN = ~0ull, REGION_NO_MAX = 0ull;
static_assert(REGION_PROBES <= REGION_SLOTS, "a probe sequence is bounded by the slot count");
static_assert(REGION_TILE * REGION_TILE < (1 << 16), "a 16-bit bin holds a whole tile of one label and one value");
constexpr int COOC_MAX_OFFSET = 16;                              // largest |dy|, |dx| of COOCCURRENCE (exported)
constexpr int COOC_MAX_OFFSETS = 8;                              // offsets per call (exported)
constexpr int COOC_MAX_LEVELS = 16;
constexpr int COOC_MAX_PIXELS = 1 << 30;                         // a symmetric diagonal bin holds at most 2 H W, which must fit int32
static_assert(2 * REGION_TILE * REGION_TILE < (1 << 16), "a 16-bit bin holds a whole tile of symmetric pairs of one label and one level");
static_assert(COOC_MAX_LEVELS * COOC_MAX_LEVELS <= 256, "a co-occurrence table fits the 256 bins of a slot");
static_assert(REGION_TILE == CGC_WAVE && REGION_BAND * (CGC_BLOCK / CGC_WAVE) == REGION_TILE, "a wave is one row of a tile, four bands");

typedef unsigned long long u64;

struct RegionWs {
  u64* kmin;      // [max_label + 1] the smallest (value, index) key of a row
  u64* kmax;      // [max_label + 1] the largest (value, ~index) key
};
static inline RegionWs region_layout(Carver&& c, int64_t rows) {
  RegionWs w;
  w.kmin = c.take<u64>(rows);
  w.kmax = c.take<u64>(rows);
  return w;
}

__device__ __forceinline__ u64 region_min_key(int v, int i) { return ((u64)((uint32_t)v ^ 0x80000000u) << 32) | (uint32_t)i; }
__device__ __forceinline__ u64 region_max_key(int v, int i) { return ((u64)((uint32_t)v ^ 0x80000000u) << 32) | (uint32_t)~i; }

// The slot of label L in an LDS table of REGION_SLOTS keys, claimed if need be; -1 if REGION_PROBES slots hold other labels.  A key
// only ever changes from REGION_EMPTY to a label, so a slot that once answered L answers L for the rest of the tile.
__device__ __forceinline__ int region_slot(int* key, int L) {
  const unsigned h = ((unsigned)L * 0x9E3779B1u) >> (32 - REGION_SLOT_BITS);
  for (int p = 0; p < REGION_PROBES; ++p) {
    const int s = (int)((h + p) & (REGION_SLOTS - 1));
    int k = __hip_atomic_load(&key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == REGION_EMPTY) {
      k = atomicCAS(&key[s], REGION_EMPTY, L);
      if (k == REGION_EMPTY) return s;
    }
    if (k == L) return s;
  }
  return -1;
}

// The 16 pixels of a thread: labels, values and the bits "counted" and "refused" (label outside [0, max_label]).  Addresses are clamped
// into the image, so that no load needs a branch; what lies outside is neither counted nor refused.
template <typename T, bool WITHIN>
struct RegionColumn {
  int lab[REGION_BAND], val[REGION_BAND];
  unsigned counted, refused;
  int first;                                                     // raster index of the thread's first pixel (meaningful if inside)
  __device__ __forceinline__ void load(const int* __restrict__ labels, const T* __restrict__ values, const void* __restrict__ within,
                                       int wbytes, int H, int W, int tiles_x, int max_label) {
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = tx * REGION_TILE + (threadIdx.x & (REGION_TILE - 1));
    const int y0 = ty * REGION_TILE + (threadIdx.x / REGION_TILE) * REGION_BAND;
    const int xc = x < W ? x : W - 1;
    unsigned on = 0;
#pragma unroll
    for (int k = 0; k < REGION_BAND; ++k) {
      const int yc = y0 + k < H ? y0 + k : H - 1;
      const int64_t i = (int64_t)yc * W + xc;
      lab[k] = labels[i];
      val[k] = (int)values[i];
      if (WITHIN) on |= (unsigned)image_nonzero(within, wbytes, i) << k;
    }
    counted = refused = 0;
#pragma unroll
    for (int k = 0; k < REGION_BAND; ++k) {
      const bool inside = x < W && y0 + k < H;
      const bool bad = lab[k] < 0 || lab[k] > max_label;
      refused |= (unsigned)(inside && bad) << k;
      counted |= (unsigned)(inside && !bad && (!WITHIN || (on >> k & 1u))) << k;
    }
    first = (int)((int64_t)y0 * W + x);                          // < H W < 2^31 whenever a bit of `counted` is set
  }
};

struct RegionMoments {
  int key[REGION_SLOTS];
  int cnt[REGION_SLOTS];
  u64 sum[REGION_SLOTS], sq[REGION_SLOTS], kmin[REGION_SLOTS], kmax[REGION_SLOTS];
};

struct RegionTables {
  int* count;
  u64 *sum, *sumsq, *kmin, *kmax;      // sumsq may be null
};

template <typename T, bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_moments(const int* __restrict__ labels, const T* __restrict__ values,
                                                              const void* __restrict__ within, int wbytes, int H, int W, int tiles_x,
                                                              int max_label, RegionTables g, int* meta) {
  __shared__ RegionMoments t;
  for (int i = threadIdx.x; i < REGION_SLOTS; i += CGC_BLOCK) {
    t.key[i] = REGION_EMPTY;
    t.cnt[i] = 0;
    t.sum[i] = t.sq[i] = 0;
    t.kmin[i] = REGION_NO_MIN;
    t.kmax[i] = REGION_NO_MAX;
  }
  RegionColumn<T, WITHIN> c;
  c.load(labels, values, within, wbytes, H, W, tiles_x, max_label);
  __syncthreads();
  const bool with_sq = g.sumsq != nullptr;

  // the run in flight: label rl (REGION_EMPTY: none), rc pixels, their sum and sum of squares, the first smallest and first largest
  int rl = REGION_EMPTY, rc = 0, vmin = 0, imin = 0, vmax = 0, imax = 0;
  int64_t rs = 0, rq = 0;
  auto fold = [&]() {
    const u64 kmn = region_min_key(vmin, imin), kmx = region_max_key(vmax, imax);
    const int s = region_slot(t.key, rl);
    if (s >= 0) {
      atomicAdd(&t.cnt[s], rc);
      atomicAdd(&t.sum[s], (u64)rs);
      if (with_sq) atomicAdd(&t.sq[s], (u64)rq);
      atomicMin(&t.kmin[s], kmn);
      atomicMax(&t.kmax[s], kmx);
    } else {
      atomicAdd(&g.count[rl], rc);
      atomicAdd(&g.sum[rl], (u64)rs);
      if (with_sq) atomicAdd(&g.sumsq[rl], (u64)rq);
      atomicMin(&g.kmin[rl], kmn);
      atomicMax(&g.kmax[rl], kmx);
    }
  };
#pragma unroll
  for (int k = 0; k <= REGION_BAND; ++k) {
    const bool on = k < REGION_BAND && (c.counted >> k & 1u);
    const int L = on ? c.lab[k < REGION_BAND ? k : 0] : REGION_EMPTY;
    if (rl != REGION_EMPTY && (L != rl || k == REGION_BAND)) {      // the run ends: at another label, at a pixel not counted, at the end
      fold();
      rl = REGION_EMPTY;
    }
    if (on) {
      const int v = c.val[k < REGION_BAND ? k : 0], i = c.first + k * W;
      if (rl == REGION_EMPTY) {
        rl = L;
        rc = 0;
        rs = rq = 0;
        vmin = vmax = v;
        imin = imax = i;
      }
      ++rc;
      rs += v;
      rq += (int64_t)v * v;                                       // used for values of at most 16 bits only: 16 * 2^30
      if (v < vmin) vmin = v, imin = i;
      if (v > vmax) vmax = v, imax = i;
    }
  }
  if (c.refused != 0) atomicAdd(meta, (int)__builtin_popcount(c.refused));
  __syncthreads();
  for (int s = threadIdx.x; s < REGION_SLOTS; s += CGC_BLOCK) {
    const int L = t.key[s];
    if (L == REGION_EMPTY) continue;
    atomicAdd(&g.count[L], t.cnt[s]);
    atomicAdd(&g.sum[L], t.sum[s]);
    if (with_sq) atomicAdd(&g.sumsq[L], t.sq[s]);
    atomicMin(&g.kmin[L], t.kmin[s]);
    atomicMax(&g.kmax[L], t.kmax[s]);
  }
}

__global__ void __launch_bounds__(CGC_BLOCK) k_region_init(int rows, RegionTables g, int* meta) {
  for (int64_t r = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * CGC_BLOCK) {
    g.count[r] = 0;
    g.sum[r] = 0;
    if (g.sumsq != nullptr) g.sumsq[r] = 0;
    g.kmin[r] = REGION_NO_MIN;
    g.kmax[r] = REGION_NO_MAX;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *meta = 0;
}

__global__ void __launch_bounds__(CGC_BLOCK) k_region_finish(int rows, const int* __restrict__ count, const u64* __restrict__ kmin,
                                                             const u64* __restrict__ kmax, int* __restrict__ mn, int* __restrict__ mx,
                                                             int* __restrict__ amin, int* __restrict__ amax) {
  for (int64_t r = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * CGC_BLOCK) {
    const bool any = count[r] != 0;
    const u64 a = kmin[r], b = kmax[r];
    mn[r] = any ? (int)((uint32_t)(a >> 32) ^ 0x80000000u) : 0;
    mx[r] = any ? (int)((uint32_t)(b >> 32) ^ 0x80000000u) : 0;
    amin[r] = any ? (int)(uint32_t)a : -1;
    amax[r] = any ? (int)~(uint32_t)b : -1;
  }
}

struct RegionHist {
  int key[REGION_SLOTS];
  uint32_t bins[REGION_SLOTS * 128];      // slot s, value v: the half v & 1 of dword 128 s + (v >> 1)
};

template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_hist(const int* __restrict__ labels, const uint8_t* __restrict__ values,
                                                           const void* __restrict__ within, int wbytes, int H, int W, int tiles_x,
                                                           int max_label, int* hist, int* meta) {
  __shared__ RegionHist t;
  for (int i = threadIdx.x; i < REGION_SLOTS; i += CGC_BLOCK) t.key[i] = REGION_EMPTY;
  for (int i = threadIdx.x; i < REGION_SLOTS * 128; i += CGC_BLOCK) t.bins[i] = 0;
  RegionColumn<uint8_t, WITHIN> c;
  c.load(labels, values, within, wbytes, H, W, tiles_x, max_label);
  __syncthreads();
  int cl = REGION_EMPTY, cs = -1;                                 // the label of the pixel above and its slot
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) {
    if (!(c.counted >> k & 1u)) continue;
    const int L = c.lab[k], v = c.val[k];
    if (L != cl) {
      cl = L;
      cs = region_slot(t.key, L);
    }
    if (cs >= 0) atomicAdd(&t.bins[cs * 128 + (v >> 1)], 1u << ((v & 1) * 16));
    else atomicAdd(&hist[(int64_t)L * 256 + v], 1);
  }
  if (c.refused != 0) atomicAdd(meta, (int)__builtin_popcount(c.refused));
  __syncthreads();
  const int v = threadIdx.x;                                      // CGC_BLOCK == 256: a thread flushes one value of every claimed slot
  for (int s = 0; s < REGION_SLOTS; ++s) {
    const int L = t.key[s];                                       // uniform
    if (L == REGION_EMPTY) continue;
    const int n = (int)(t.bins[s * 128 + (v >> 1)] >> ((v & 1) * 16) & 0xffffu);
    if (n != 0) atomicAdd(&hist[(int64_t)L * 256 + v], n);
  }
}

struct RegionQuantiles {
  int n;
  int q[REGION_MAX_Q];
};

// one wave per row: four bins per lane, rank.hip's scan and search
__global__ void __launch_bounds__(CGC_BLOCK) k_region_quantiles(const uint32_t* __restrict__ hist, int64_t rows, RegionQuantiles q,
                                                                uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & (CGC_WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * (CGC_BLOCK / CGC_WAVE) + threadIdx.x / CGC_WAVE;
  if (row >= rows) return;                                        // the whole wave
  const uint4 c = reinterpret_cast<const uint4*>(hist + row * 256)[lane];
  const uint32_t incl = rank_wave_scan(c.x + c.y + c.z + c.w);
  const uint32_t n = __builtin_amdgcn_readlane(incl, CGC_WAVE - 1);
  for (int j = 0; j < q.n; ++j) {
    int value = 0;
    if (n > 0) {
      const uint64_t k = (uint64_t)n * (uint32_t)q.q[j] / 10000u;   // n q10k < 2^46
      value = rank_value(c, incl, k < n - 1 ? (uint32_t)k : n - 1);
    }
    if (lane == 0) out[row * q.n + j] = (uint8_t)value;
  }
}

static inline bool bad_region(int H, int W, int max_label, const void* within, int wbytes) {
  return bad_image_dims(H, W) || max_label < 0 || max_label == 0x7fffffff || (within != nullptr && bad_elem_bytes(wbytes));
}
static inline int region_blocks(int64_t rows) {
  const int64_t b = ceil_div64(rows, CGC_BLOCK);
  return (int)(b < REGION_INIT_BLOCKS ? b : REGION_INIT_BLOCKS);
}

struct CoocLut {
  uint32_t w[64];                        // the level of value v: byte v & 3 of dword v >> 2
};

struct RegionCooc {
  int key[REGION_SLOTS];
  uint32_t bins[REGION_SLOTS * 128];      // slot s, bin a * levels + b: as RegionHist's value
  uint32_t level[64];                    // the lut, for lookups by lane
};

// One offset (dy, dx) of COOCCURRENCE: k_region_hist with a pair of pixels where the histogram has one.  The anchor p is the thread's
// pixel, the partner q = p + (dy, dx) is loaded from global memory through an address clamped into the image; whether q lies inside the
// image is decided from its coordinates, never from what the clamped address returned.  The tile that holds p counts the pair, wherever
// q lies.  `out` is the table of this offset, tables + k * levels^2; a row is `row_stride` = noff * levels^2 counters further on.
template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_cooc(const int* __restrict__ labels, const uint8_t* __restrict__ values,
                                                           const void* __restrict__ within, int wbytes, int H, int W, int tiles_x,
                                                           int max_label, CoocLut lut, int levels, int dy, int dx, int symmetric,
                                                           int count_refused, int* out, int64_t row_stride, int* meta) {
  __shared__ RegionCooc t;
  for (int i = threadIdx.x; i < REGION_SLOTS; i += CGC_BLOCK) t.key[i] = REGION_EMPTY;
  for (int i = threadIdx.x; i < REGION_SLOTS * 128; i += CGC_BLOCK) t.bins[i] = 0;
  if (threadIdx.x < 64) t.level[threadIdx.x] = lut.w[threadIdx.x];
  RegionColumn<uint8_t, WITHIN> c;
  c.load(labels, values, within, wbytes, H, W, tiles_x, max_label);
  // the partners: same column for all 16, rows y0 + dy ..
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int qx = tx * REGION_TILE + (threadIdx.x & (REGION_TILE - 1)) + dx;
  const int qy0 = ty * REGION_TILE + (threadIdx.x / REGION_TILE) * REGION_BAND + dy;
  const int qxc = qx < 0 ? 0 : (qx < W ? qx : W - 1);
  int plab[REGION_BAND], pval[REGION_BAND];
  unsigned pon = 0;
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) {
    const int qy = qy0 + k;
    const int qyc = qy < 0 ? 0 : (qy < H ? qy : H - 1);
    const int64_t i = (int64_t)qyc * W + qxc;
    plab[k] = labels[i];
    pval[k] = (int)values[i];
    if (WITHIN) pon |= (unsigned)image_nonzero(within, wbytes, i) << k;
  }
  unsigned pair = 0;                                              // bit k: anchor k and its partner are a counted pair
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) {
    const int qy = qy0 + k;
    const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
    pair |= (unsigned)(inside && plab[k] == c.lab[k] && (!WITHIN || (pon >> k & 1u))) << k;
  }
  pair &= c.counted;
  __syncthreads();
  const uint8_t* level = reinterpret_cast<const uint8_t*>(t.level);
  int cl = REGION_EMPTY, cs = -1;                                 // the label of the pair above and its slot
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) {
    if (!(pair >> k & 1u)) continue;
    const int L = c.lab[k];
    const int a = level[c.val[k]], b = level[pval[k]];
    const int ab = a * levels + b, ba = b * levels + a;            // < levels^2 <= 256: the host checked every entry of the lut
    if (L != cl) {
      cl = L;
      cs = region_slot(t.key, L);
    }
    if (cs >= 0) {
      atomicAdd(&t.bins[cs * 128 + (ab >> 1)], 1u << ((ab & 1) * 16));
      if (symmetric) atomicAdd(&t.bins[cs * 128 + (ba >> 1)], 1u << ((ba & 1) * 16));
    } else {
      int* row = out + (int64_t)L * row_stride;
      atomicAdd(&row[ab], 1);
      if (symmetric) atomicAdd(&row[ba], 1);
    }
  }
  if (count_refused && c.refused != 0) atomicAdd(meta, (int)__builtin_popcount(c.refused));
  __syncthreads();
  const int v = threadIdx.x;                                      // CGC_BLOCK == 256: a thread flushes one bin of every claimed slot
  if (v >= levels * levels) return;                               // after the last barrier
  for (int s = 0; s < REGION_SLOTS; ++s) {
    const int L = t.key[s];                                       // uniform
    if (L == REGION_EMPTY) continue;
    const int n = (int)(t.bins[s * 128 + (v >> 1)] >> ((v & 1) * 16) & 0xffffu);
    if (n != 0) atomicAdd(&out[(int64_t)L * row_stride + v], n);
  }
}

// GEOMETRY (KernelSpec.region_geometry; DESIGN.md, "Region geometry"): the shape of every region from the label image alone.  A pixel
// *belongs* to row L as it is counted above; a position outside the image, with a refused label or outside `within` belongs to none.
constexpr int GEOM_NONE = REGION_EMPTY;
constexpr int GEOM_DIRS = 8;                                     // directions (a, b) of the extents a x + b y; every b >= 0 (exported order)
constexpr int GEOM_MAX_SIDE = 32767;                             // sum x^2 over 2^31 pixels stays inside int64 (exported)
constexpr int GEOM_SIDE = REGION_TILE + 2;                       // a tile and the frame of one position its quads reach into

struct GeomTables {
  int* count;                            // [R]
  u64 *sy, *sx, *syy, *sxy, *sxx;        // [R] each, image coordinates
  int* ext;                              // [R, 8, 2] min, max of a x + b y
  int* quad;                             // [R, 4] n1, n2, nd, n3
  int* border;                           // [R]
};

struct GeomTile {                        // sums and extents in tile coordinates, shifted to the image at the flush
  int key[REGION_SLOTS];
  int cnt[REGION_SLOTS], border[REGION_SLOTS];
  uint32_t sy[REGION_SLOTS], sx[REGION_SLOTS], syy[REGION_SLOTS], sxy[REGION_SLOTS], sxx[REGION_SLOTS];      // at most 4096 * 63 * 63
  int ext[REGION_SLOTS][GEOM_DIRS][2];
  int quad[REGION_SLOTS][4];
};

__device__ __forceinline__ int geom_a(int d) { return d == 0 ? 1 : d == 1 ? 2 : d == 2 ? 1 : d == 3 ? 1 : d == 4 ? 0 : d == 5 ? -1 : d == 6 ? -1 : -2; }
__device__ __forceinline__ int geom_b(int d) { return d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 1 : d == 3 ? 2 : d == 4 ? 1 : d == 5 ? 2 : d == 6 ? 1 : 1; }

// A minimum or maximum into a word that only ever falls (rises).  The word is read first and the atomic is skipped where it would
// change nothing: whatever the read returns was written by somebody, so the final value is beyond it.  A whole image of background
// would otherwise send sixteen atomics per tile to the one cache line that holds its extents.
template <int SCOPE>
__device__ __forceinline__ void geom_min(int* p, int v) {
  if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE)) atomicMin(p, v);
}
template <int SCOPE>
__device__ __forceinline__ void geom_max(int* p, int v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE)) atomicMax(p, v);
}

// One tile.  The label every position of the tile and of a frame of one position around it belongs to (GEOM_NONE: to none) is staged
// in LDS, so that runs and quads are walked by loops over k, not by unrolled copies of their bodies: a fold is 23 atomics and a slot
// lookup, and sixteen copies of it per thread do not fit the instruction cache.
template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_geometry(const int* __restrict__ labels, const void* __restrict__ within, int wbytes,
                                                               int H, int W, int tiles_x, int max_label, GeomTables g, int* meta) {
  __shared__ GeomTile t;
  __shared__ int e[GEOM_SIDE][GEOM_SIDE];                          // position (ly, lx) of the tile, -1 .. REGION_TILE, at [ly + 1][lx + 1]
  for (int i = threadIdx.x; i < REGION_SLOTS; i += CGC_BLOCK) {
    t.key[i] = REGION_EMPTY;
    t.cnt[i] = t.border[i] = 0;
    t.sy[i] = t.sx[i] = t.syy[i] = t.sxy[i] = t.sxx[i] = 0;
  }
  for (int i = threadIdx.x; i < REGION_SLOTS * GEOM_DIRS; i += CGC_BLOCK) {
    (&t.ext[0][0][0])[2 * i] = 0x7fffffff;
    (&t.ext[0][0][0])[2 * i + 1] = (int)0x80000000;
  }
  (&t.quad[0][0])[threadIdx.x] = 0;                               // CGC_BLOCK == REGION_SLOTS * 4
  if (threadIdx.x < GEOM_SIDE) e[0][threadIdx.x] = e[threadIdx.x][0] = GEOM_NONE;      // row and column -1: only the image's frame is ever read
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ox = tx * REGION_TILE, oy = ty * REGION_TILE;
  const int lx = threadIdx.x & (REGION_TILE - 1), ly0 = (threadIdx.x / REGION_TILE) * REGION_BAND;
  const int x = ox + lx, y0 = oy + ly0;
  const bool last_band = ly0 + REGION_BAND == REGION_TILE, last_lane = lx == REGION_TILE - 1;
  // The row position (py, px) belongs to.  The address is clamped into the image; whether the position lies inside is decided from
  // its coordinates.  `bad`: inside, and the label is outside [0, max_label].
  auto belongs = [&](int py, int px, bool& bad) -> int {
    const int64_t i = (int64_t)(py < H ? py : H - 1) * W + (px < W ? px : W - 1);
    const int L = labels[i];
    const bool on = !WITHIN || image_nonzero(within, wbytes, i);
    const bool inside = py < H && px < W;
    bad = inside && (L < 0 || L > max_label);
    return inside && !bad && on ? L : GEOM_NONE;
  };
  unsigned on = 0, brk = 0, refused = 0;                          // bit k: pixel k belongs somewhere; not where pixel k - 1 does; is refused
  {
    int prev = GEOM_NONE;
    bool bad;
#pragma unroll
    for (int k = 0; k < REGION_BAND; ++k) {
      const int L = belongs(y0 + k, x, bad);
      refused |= (unsigned)bad << k;
      on |= (unsigned)(L != GEOM_NONE) << k;
      brk |= (unsigned)(L != prev) << k;
      prev = L;
      e[ly0 + k + 1][lx + 1] = L;
    }
    if (last_band) e[REGION_TILE + 1][lx + 1] = belongs(oy + REGION_TILE, x, bad);      // the row below the tile
    if (last_lane) {                                              // the column to its right
#pragma unroll
      for (int k = 0; k < REGION_BAND; ++k) e[ly0 + k + 1][REGION_TILE + 1] = belongs(y0 + k, x + 1, bad);
      if (last_band) e[REGION_TILE + 1][REGION_TILE + 1] = belongs(oy + REGION_TILE, x + 1, bad);
    }
  }
  __syncthreads();

  // pixels: the runs of one label down the thread's 16 pixels, rows ya .. yb of the tile, by their closed forms
  unsigned starts = on & brk;
  for (int r = 0; r < REGION_BAND && starts != 0; ++r) {
    const int ka = __builtin_ctz(starts);
    starts &= starts - 1;
    const int kb = __builtin_ctz((starts | ~on) & (~0u << ka)) - 1;      // the run ends before the next start or pixel of no row; ~on has bit 16
    const int L = e[ly0 + ka + 1][lx + 1];
    const int n = kb - ka + 1, ya = ly0 + ka, yb = ly0 + kb;
    const int rsy = n * (ya + yb) / 2;
    const int rsyy = (yb * (yb + 1) * (2 * yb + 1) - (ya - 1) * ya * (2 * ya - 1)) / 6;
    const int rb = x == 0 || x == W - 1 ? n : (int)(oy + ya == 0) + (int)(oy + yb == H - 1 && H > 1);
    const int s = region_slot(t.key, L);
    if (s >= 0) {
      atomicAdd(&t.cnt[s], n);
      if (rb != 0) atomicAdd(&t.border[s], rb);
      atomicAdd(&t.sy[s], (uint32_t)rsy);
      atomicAdd(&t.sx[s], (uint32_t)(n * lx));
      atomicAdd(&t.syy[s], (uint32_t)rsyy);
      atomicAdd(&t.sxy[s], (uint32_t)(rsy * lx));
      atomicAdd(&t.sxx[s], (uint32_t)(n * lx * lx));
#pragma unroll
      for (int d = 0; d < GEOM_DIRS; ++d) {                       // b >= 0: the run's extents are attained at its two ends
        geom_min<__HIP_MEMORY_SCOPE_WORKGROUP>(&t.ext[s][d][0], geom_a(d) * lx + geom_b(d) * ya);
        geom_max<__HIP_MEMORY_SCOPE_WORKGROUP>(&t.ext[s][d][1], geom_a(d) * lx + geom_b(d) * yb);
      }
    } else {                                                      // no slot: the same atomics on the global tables, in image coordinates
      const int64_t sy = (int64_t)rsy + (int64_t)n * oy, syy = (int64_t)rsyy + 2 * (int64_t)oy * rsy + (int64_t)n * oy * oy;
      atomicAdd(&g.count[L], n);
      if (rb != 0) atomicAdd(&g.border[L], rb);
      atomicAdd(&g.sy[L], (u64)sy);
      atomicAdd(&g.sx[L], (u64)((int64_t)n * x));
      atomicAdd(&g.syy[L], (u64)syy);
      atomicAdd(&g.sxy[L], (u64)(sy * x));
      atomicAdd(&g.sxx[L], (u64)((int64_t)n * x * x));
      int* ext = g.ext + (int64_t)L * (GEOM_DIRS * 2);
#pragma unroll
      for (int d = 0; d < GEOM_DIRS; ++d) {
        geom_min<__HIP_MEMORY_SCOPE_AGENT>(&ext[2 * d], geom_a(d) * x + geom_b(d) * (oy + ya));
        geom_max<__HIP_MEMORY_SCOPE_AGENT>(&ext[2 * d + 1], geom_a(d) * x + geom_b(d) * (oy + yb));
      }
    }
  }

  // quads: pass 0, those whose top-left corner is one of the thread's pixels -- and, in the tiles of the top edge, the one above
  // them in row -1; pass 1, for the first lane of the tiles of the left edge, the same in column -1
  int cl = GEOM_NONE, cs = -1;                                    // the label last looked up and its slot
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0 ? x >= W : !(tx == 0 && lx == 0)) continue;
    const int qx = pass == 0 ? lx : -1;
    const int k0 = ty == 0 && ly0 == 0 ? -1 : 0;
    int tl = e[ly0 + k0 + 1][qx + 1], tr = e[ly0 + k0 + 1][qx + 2];
    for (int k = k0; k < REGION_BAND; ++k) {
      const int bl = e[ly0 + k + 2][qx + 1], br = e[ly0 + k + 2][qx + 2];
      if (y0 + k < H && !(tl == tr && tl == bl && tl == br)) {     // the pattern of every row present in the quad
        const int p[4] = {tl, tr, bl, br};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int L = p[i];
          bool first = L != GEOM_NONE;
          unsigned m = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < i && p[j] == L) first = false;
            m |= (unsigned)(p[j] == L) << j;
          }
          if (!first) continue;
          const int c = __builtin_popcount(m);                    // 1 .. 3: the four are not all equal
          const int cls = c == 1 ? 0 : c == 3 ? 3 : (m == 9u || m == 6u) ? 2 : 1;
          if (L != cl) {
            cl = L;
            cs = region_slot(t.key, L);
          }
          if (cs >= 0) atomicAdd(&t.quad[cs][cls], 1);
          else atomicAdd(&g.quad[(int64_t)L * 4 + cls], 1);
        }
      }
      tl = bl;
      tr = br;
    }
  }
  if (refused != 0) atomicAdd(meta, (int)__builtin_popcount(refused));
  __syncthreads();

  // flush: a wave per quarter of a slot's words, shifted to image coordinates
  const int s = threadIdx.x & (REGION_SLOTS - 1), part = threadIdx.x / REGION_SLOTS;
  const int L = t.key[s];
  if (L == REGION_EMPTY) return;                                  // after the last barrier
  if (part == 0) {
    const int64_t n = t.cnt[s], sy = t.sy[s], sx = t.sx[s];
    if (n == 0) return;                                           // a slot claimed by a quad alone
    atomicAdd(&g.count[L], (int)n);
    if (t.border[s] != 0) atomicAdd(&g.border[L], t.border[s]);
    atomicAdd(&g.sy[L], (u64)(sy + n * oy));
    atomicAdd(&g.sx[L], (u64)(sx + n * ox));
    atomicAdd(&g.syy[L], (u64)((int64_t)t.syy[s] + 2 * oy * sy + n * oy * oy));
    atomicAdd(&g.sxy[L], (u64)((int64_t)t.sxy[s] + ox * sy + oy * sx + n * ox * oy));
    atomicAdd(&g.sxx[L], (u64)((int64_t)t.sxx[s] + 2 * ox * sx + n * ox * ox));
  } else if (part == 3) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (t.quad[s][c] != 0) atomicAdd(&g.quad[(int64_t)L * 4 + c], t.quad[s][c]);
  } else if (t.cnt[s] != 0) {                                      // a slot claimed by a quad alone has no extents
    int* ext = g.ext + (int64_t)L * (GEOM_DIRS * 2);
    // A row that fills half a tile is likely to fill others (the background does): their extents meet on one cache line, and the
    // read first spares it most of the atomics.  A nucleus has its line to itself, and the read would only be a round trip more.
    const bool shared = t.cnt[s] >= REGION_TILE * REGION_TILE / 2;
#pragma unroll
    for (int i = 0; i < GEOM_DIRS / 2; ++i) {
      const int d = (part - 1) * (GEOM_DIRS / 2) + i;
      const int shift = geom_a(d) * ox + geom_b(d) * oy;
      const int lo = t.ext[s][d][0] + shift, hi = t.ext[s][d][1] + shift;
      if (shared) {
        geom_min<__HIP_MEMORY_SCOPE_AGENT>(&ext[2 * d], lo);
        geom_max<__HIP_MEMORY_SCOPE_AGENT>(&ext[2 * d + 1], hi);
      } else {
        atomicMin(&ext[2 * d], lo);
        atomicMax(&ext[2 * d + 1], hi);
      }
    }
  }
}
static_assert(CGC_BLOCK == REGION_SLOTS * 4, "the flush of k_region_geometry gives a slot four threads, one per wave");

__global__ void __launch_bounds__(CGC_BLOCK) k_geometry_init(int rows, GeomTables g, int* meta) {
  for (int64_t r = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * CGC_BLOCK) {
    g.count[r] = g.border[r] = 0;
    g.sy[r] = g.sx[r] = g.syy[r] = g.sxy[r] = g.sxx[r] = 0;
#pragma unroll
    for (int d = 0; d < GEOM_DIRS; ++d) {
      g.ext[r * (GEOM_DIRS * 2) + 2 * d] = 0x7fffffff;
      g.ext[r * (GEOM_DIRS * 2) + 2 * d + 1] = (int)0x80000000;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) g.quad[r * 4 + c] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *meta = 0;
}

__global__ void __launch_bounds__(CGC_BLOCK) k_geometry_finish(int rows, const int* __restrict__ count, int* __restrict__ ext) {      // the extents of an empty row
  for (int64_t r = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * CGC_BLOCK) {
    if (count[r] != 0) continue;
#pragma unroll
    for (int i = 0; i < GEOM_DIRS * 2; ++i) ext[r * (GEOM_DIRS * 2) + i] = 0;
  }
}

template <typename T>
void launch_moments(const int* labels, const void* values, const void* within, int wbytes, int H, int W, int max_label,
                    const RegionTables& g, int* meta, hipStream_t st) {
  const int tiles_x = ceil_div(W, REGION_TILE);
  const dim3 grid((unsigned)((int64_t)tiles_x * ceil_div(H, REGION_TILE)));      // < 2^31 / 4096 + H / 64 + W / 64 + 1
  if (within != nullptr)
    hipLaunchKernelGGL((k_region_moments<T, true>), grid, dim3(CGC_BLOCK), 0, st, labels, static_cast<const T*>(values), within, wbytes, H, W,
                       tiles_x, max_label, g, meta);
  else
    hipLaunchKernelGGL((k_region_moments<T, false>), grid, dim3(CGC_BLOCK), 0, st, labels, static_cast<const T*>(values), within, 0, H, W,
                       tiles_x, max_label, g, meta);
}

}  // namespace

extern "C" int cgc_region_tile_side(void) { return REGION_TILE; }
extern "C" int cgc_region_table_slots(void) { return REGION_SLOTS; }

extern "C" int64_t cgc_region_ws_bytes(int max_label) {
  if (max_label < 0 || max_label == 0x7fffffff) return 0;
  return layout_bytes(region_layout, (int64_t)max_label + 1);
}

extern "C" int cgc_region_moments(const int* labels, const void* values, int value_bytes, int value_signed, const void* within_or_null,
                                  int within_bytes, int H, int W, int max_label, void* ws, int* count, int64_t* sum,
                                  int64_t* sumsq_or_null, int* min, int* max, int* argmin, int* argmax, int* meta, cgc_stream_t stream) {
  if (bad_region(H, W, max_label, within_or_null, within_bytes)) return CGC_EINVAL;
  const bool u8 = value_bytes == 1 && value_signed == 0, i8 = value_bytes == 1 && value_signed == 1;
  const bool i16 = value_bytes == 2 && value_signed == 1, i32 = value_bytes == 4 && value_signed == 1;
  if (!(u8 || i8 || i16 || i32) || (i32 && sumsq_or_null != nullptr)) return CGC_EINVAL;
  if (ws == nullptr || count == nullptr || sum == nullptr || min == nullptr || max == nullptr || argmin == nullptr || argmax == nullptr ||
      meta == nullptr)
    return CGC_EINVAL;
  const bool empty = (int64_t)H * W == 0;
  if (!empty && (labels == nullptr || values == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int rows = max_label + 1;
  const RegionWs w = region_layout(Carver(ws), rows);
  const RegionTables g{count, reinterpret_cast<u64*>(sum), reinterpret_cast<u64*>(sumsq_or_null), w.kmin, w.kmax};
  hipLaunchKernelGGL(k_region_init, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, g, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  if (!empty) {
    if (u8) launch_moments<uint8_t>(labels, values, within_or_null, within_bytes, H, W, max_label, g, meta, st);
    else if (i8) launch_moments<int8_t>(labels, values, within_or_null, within_bytes, H, W, max_label, g, meta, st);
    else if (i16) launch_moments<int16_t>(labels, values, within_or_null, within_bytes, H, W, max_label, g, meta, st);
    else launch_moments<int32_t>(labels, values, within_or_null, within_bytes, H, W, max_label, g, meta, st);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  hipLaunchKernelGGL(k_region_finish, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, count, w.kmin, w.kmax, min, max, argmin, argmax);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_histogram(const int* labels, const uint8_t* values, const void* within_or_null, int within_bytes, int H, int W,
                                    int max_label, int* hist, int* meta, cgc_stream_t stream) {
  if (bad_region(H, W, max_label, within_or_null, within_bytes) || hist == nullptr || meta == nullptr) return CGC_EINVAL;
  const bool empty = (int64_t)H * W == 0;
  if (!empty && (labels == nullptr || values == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  hipError_t e = hipMemsetAsync(hist, 0, ((size_t)max_label + 1) * 256 * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (empty) return 0;
  const int tiles_x = ceil_div(W, REGION_TILE);
  const dim3 grid((unsigned)((int64_t)tiles_x * ceil_div(H, REGION_TILE)));
  if (within_or_null != nullptr)
    hipLaunchKernelGGL(k_region_hist<true>, grid, dim3(CGC_BLOCK), 0, st, labels, values, within_or_null, within_bytes, H, W, tiles_x, max_label,
                       hist, meta);
  else
    hipLaunchKernelGGL(k_region_hist<false>, grid, dim3(CGC_BLOCK), 0, st, labels, values, within_or_null, 0, H, W, tiles_x, max_label, hist,
                       meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_cooc_max_offset(void) { return COOC_MAX_OFFSET; }
extern "C" int cgc_region_cooc_max_offsets(void) { return COOC_MAX_OFFSETS; }

extern "C" int cgc_region_cooccurrence(const int* labels, const uint8_t* values, const void* within_or_null, int within_bytes, int H, int W,
                                       int max_label, const uint8_t* lut256_host, int levels, const int* offsets_host, int noff,
                                       int symmetric, int* tables, int* meta, cgc_stream_t stream) {
  if (bad_region(H, W, max_label, within_or_null, within_bytes) || (int64_t)H * W >= COOC_MAX_PIXELS) return CGC_EINVAL;
  if (tables == nullptr || meta == nullptr || lut256_host == nullptr || offsets_host == nullptr) return CGC_EINVAL;
  if (levels < 2 || levels > COOC_MAX_LEVELS || noff < 1 || noff > COOC_MAX_OFFSETS) return CGC_EINVAL;
  CoocLut lut{};
  for (int v = 0; v < 256; ++v) {
    if (lut256_host[v] >= levels) return CGC_EINVAL;
    lut.w[v >> 2] |= (uint32_t)lut256_host[v] << ((v & 3) * 8);
  }
  for (int k = 0; k < noff; ++k) {
    const int dy = offsets_host[2 * k], dx = offsets_host[2 * k + 1];
    if (dy < -COOC_MAX_OFFSET || dy > COOC_MAX_OFFSET || dx < -COOC_MAX_OFFSET || dx > COOC_MAX_OFFSET || (dy == 0 && dx == 0))
      return CGC_EINVAL;
  }
  const bool empty = (int64_t)H * W == 0;
  if (!empty && (labels == nullptr || values == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int bins = levels * levels;
  const int64_t row_stride = (int64_t)noff * bins;
  hipError_t e = hipMemsetAsync(tables, 0, ((size_t)max_label + 1) * (size_t)row_stride * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (empty) return 0;
  const int tiles_x = ceil_div(W, REGION_TILE);
  const dim3 grid((unsigned)((int64_t)tiles_x * ceil_div(H, REGION_TILE)));
  for (int k = 0; k < noff; ++k) {                                // one launch per offset; the first counts the refused pixels
    const int dy = offsets_host[2 * k], dx = offsets_host[2 * k + 1];
    if (within_or_null != nullptr)
      hipLaunchKernelGGL(k_region_cooc<true>, grid, dim3(CGC_BLOCK), 0, st, labels, values, within_or_null, within_bytes, H, W, tiles_x,
                         max_label, lut, levels, dy, dx, (int)(symmetric != 0), (int)(k == 0), tables + (int64_t)k * bins, row_stride, meta);
    else
      hipLaunchKernelGGL(k_region_cooc<false>, grid, dim3(CGC_BLOCK), 0, st, labels, values, within_or_null, 0, H, W, tiles_x, max_label,
                         lut, levels, dy, dx, (int)(symmetric != 0), (int)(k == 0), tables + (int64_t)k * bins, row_stride, meta);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_region_geometry_max_side(void) { return GEOM_MAX_SIDE; }

extern "C" int cgc_region_geometry(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label, int* count,
                                   int64_t* sums, int* extents, int* quads, int* border, int* meta, cgc_stream_t stream) {
  if (bad_region(H, W, max_label, within_or_null, within_bytes)) return CGC_EINVAL;
  if (H > GEOM_MAX_SIDE || W > GEOM_MAX_SIDE || ((int64_t)H + 1) * ((int64_t)W + 1) >= ((int64_t)1 << 31)) return CGC_EINVAL;
  if (count == nullptr || sums == nullptr || extents == nullptr || quads == nullptr || border == nullptr || meta == nullptr) return CGC_EINVAL;
  const bool empty = (int64_t)H * W == 0;
  if (!empty && labels == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int rows = max_label + 1;
  u64* s = reinterpret_cast<u64*>(sums);                          // [5, rows]: sy, sx, syy, sxy, sxx
  const GeomTables g{count, s, s + rows, s + 2 * (int64_t)rows, s + 3 * (int64_t)rows, s + 4 * (int64_t)rows, extents, quads, border};
  hipLaunchKernelGGL(k_geometry_init, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, g, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  if (!empty) {
    const int tiles_x = ceil_div(W, REGION_TILE);
    const dim3 grid((unsigned)((int64_t)tiles_x * ceil_div(H, REGION_TILE)));
    if (within_or_null != nullptr)
      hipLaunchKernelGGL(k_region_geometry<true>, grid, dim3(CGC_BLOCK), 0, st, labels, within_or_null, within_bytes, H, W, tiles_x, max_label, g,
                         meta);
    else
      hipLaunchKernelGGL(k_region_geometry<false>, grid, dim3(CGC_BLOCK), 0, st, labels, within_or_null, 0, H, W, tiles_x, max_label, g, meta);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  hipLaunchKernelGGL(k_geometry_finish, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, count, extents);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_quantiles(const int* hist, int64_t rows, const int* q10k, int nq, uint8_t* out, cgc_stream_t stream) {
  if (rows < 0 || rows >= ((int64_t)1 << 31) || nq < 1 || nq > REGION_MAX_Q || q10k == nullptr) return CGC_EINVAL;
  RegionQuantiles q{nq, {}};
  for (int j = 0; j < nq; ++j) {
    if (q10k[j] < 0 || q10k[j] > 10000) return CGC_EINVAL;
    q.q[j] = q10k[j];
  }
  if (rows == 0) return 0;
  if (hist == nullptr || out == nullptr || !aligned16(hist)) return CGC_EINVAL;
  hipLaunchKernelGGL(k_region_quantiles, dim3((unsigned)ceil_div64(rows, CGC_BLOCK / CGC_WAVE)), dim3(CGC_BLOCK), 0, as_stream(stream),
                     reinterpret_cast<const uint32_t*>(hist), rows, q, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
