// Tables of a label image on gfx950, indexed by label value.  MOMENTS (count, sum, sum of squares, extrema with their positions),
// HISTOGRAM (the 256 bins of a uint8 plane) and QUANTILES read off such histograms: KernelSpec.region_statistics / region_histogram /
// region_quantiles; DESIGN.md, "Region statistics".  COOCCURRENCE (pairs of levels per offset): KernelSpec.region_cooccurrence; "Region
// co-occurrence".  GEOMETRY (count, second-order sums, extents, quads, frame pixels): KernelSpec.region_geometry; "Region geometry".
// HULL (the exact convex hull of a row's pixel squares, behind GEOMETRY): KernelSpec.region_hull; "Region hull".
//
// A pixel p is *counted* in row L (*belongs* to it) iff labels[p] == L, 0 <= L <= max_label, and within is null or non-zero at p.  A
// pixel whose label lies outside [0, max_label] is *refused*: counted nowhere, one more in *meta (region_refused), `within` or not.
//
// WHAT THE FOUR TILE KERNELS SHARE, each written once:
//   RegionSpot      where a thread stands: a 64 x 64 tile per workgroup, a wave is one row of it, a thread owns 16 rows of one column.
//   region_index,   a position on any side of the image is read through an address clamped into it, so that no load sits behind a
//   region_judge    branch; whether it is inside is decided from its coordinates, never from what the clamped address returned.
//                   RegionColumn::fetch issues the 16 loads of a column (labels, values, `within`), ::judge looks at them afterwards.
//   region_slot     an LDS table of REGION_SLOTS rows keyed by label, filled with LDS atomics and flushed after a barrier with one
//                   integer atomic per word.  OVERFLOW: a label looks at no more than REGION_PROBES <= REGION_SLOTS slots and never
//                   waits; one that finds neither itself nor an empty slot there goes to the global tables directly.  Both routes end
//                   in the same integer atomics on the same global words, so which pixels take which route -- it depends on the order
//                   in which lanes arrive -- changes no result: integer sums, minima and maxima are independent of order.  A tile in
//                   which every pixel has its own label is an ordinary input: 64 labels fold, the rest go direct.
//   RegionBins      the table of HISTOGRAM and COOCCURRENCE: 256 16-bit bins per slot, two per dword; the walk down a thread's pixels
//                   that keeps the slot of the label above and probes only when the label changes; the flush, a thread per bin.
//   region_call     the host side: the refusals that depend on the image alone, the empty image, the grid; region_launch picks WITHIN.
// WHAT EACH MODE ADDS:
//   MOMENTS         k_region_init, k_region_moments, k_region_finish.  A run of equal labels down the column is summed in registers
//                   and folded a run at a time (region_add: the same five quantities in LDS, on the direct route and in the flush).
//                   EXTREMA: the value and its position travel as one key: min key = (v ^ 0x80000000) << 32 | i under an unsigned
//                   min, max key = (v ^ 0x80000000) << 32 | ~i under an unsigned max -- of equal values the smallest raster index i
//                   wins in both, in a thread's run (i grows down the column, strict comparisons), in LDS and in global memory.  No
//                   key equals the initial ~0 / 0: i < 2^31.
//   HISTOGRAM       hipMemsetAsync, k_region_hist: the bin of a counted pixel is its value; a slot is flushed as 256 consecutive counters.
//   COOCCURRENCE    hipMemsetAsync, then one k_region_cooc per offset: a second column, the partners, loaded at (dy, dx) from the
//                   anchors; the bin of a counted pair is its pair of levels, both orders when symmetric.
//   GEOMETRY        k_geometry_init, k_region_geometry, k_geometry_finish.  The label every position belongs to is staged in LDS with
//                   a frame of one position; runs are folded by closed forms in tile coordinates and shifted to the image on the way
//                   to global memory (geom_add: the flush and the direct route), quads classified where their four positions differ.
//   HULL            k_hull_spans_init, k_region_hull_spans, k_region_hull.  No table in LDS: per image row of a label's bounding box the
//                   smallest and largest column, two atomics per run of a tile row; then a lane (a wave for a tall region) per label.
#include <stdint.h>
#include <type_traits>

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

struct RegionImage {                     // what every tile kernel is given
  const int* labels;
  const void* within;                    // null: every pixel
  int wbytes, H, W, tiles_x, max_label;
};

struct RegionSpot {                      // where a thread stands
  int ty, tx, oy, ox;                    // the tile of the workgroup and its first pixel
  int ly0, lx;                           // the first of the thread's 16 rows and its column, in the tile
  int y0, x;                             // ... and in the image
  bool last_band, last_lane;             // the thread's rows end the tile; its column does
};
__device__ __forceinline__ RegionSpot region_spot(int tiles_x) {
  RegionSpot s;
  s.ty = blockIdx.x / tiles_x, s.tx = blockIdx.x - s.ty * tiles_x;
  s.oy = s.ty * REGION_TILE, s.ox = s.tx * REGION_TILE;
  s.ly0 = (threadIdx.x / REGION_TILE) * REGION_BAND, s.lx = threadIdx.x & (REGION_TILE - 1);
  s.y0 = s.oy + s.ly0, s.x = s.ox + s.lx;
  s.last_band = s.ly0 + REGION_BAND == REGION_TILE, s.last_lane = s.lx == REGION_TILE - 1;
  return s;
}

// The raster index position (py, px) is read through: clamped into the image on every side, so that no load needs a branch.
__device__ __forceinline__ int64_t region_index(const RegionImage& im, int py, int px) {
  const int yc = py < 0 ? 0 : (py < im.H ? py : im.H - 1), xc = px < 0 ? 0 : (px < im.W ? px : im.W - 1);
  return (int64_t)yc * im.W + xc;
}
// What was read there: label L, and `on`, the bit of `within`.  Inside the image or not is decided from the coordinates; what lies
// outside is neither counted nor refused.
struct RegionVerdict { bool refused, counted; };
template <bool WITHIN>
__device__ __forceinline__ RegionVerdict region_judge(const RegionImage& im, int py, int px, int L, bool on) {
  const bool inside = (unsigned)py < (unsigned)im.H && (unsigned)px < (unsigned)im.W;      // 0 <= py < H, 0 <= px < W
  const bool bad = (unsigned)L > (unsigned)im.max_label;                                    // L < 0 or L > max_label
  return {inside && bad, inside && !bad && (!WITHIN || on)};
}

// 16 positions of one column, (dy, dx) from the thread's own: labels, values and the bits "counted" and "refused".  Two passes, so
// that a kernel can issue the loads of all its columns before it looks at the first: fetch() loads, judge() decides.
template <typename T, bool WITHIN>
struct RegionColumn {
  int lab[REGION_BAND], val[REGION_BAND];
  unsigned on, counted, refused;                                 // bit k: `within` is non-zero at position k; it is counted; refused
  int py0, px, first;                                            // the first position, and its raster index (meaningful if inside)
  __device__ __forceinline__ void fetch(const RegionImage& im, const T* __restrict__ values, const RegionSpot& s, int dy, int dx) {
    py0 = s.y0 + dy, px = s.x + dx, on = 0;
#pragma unroll
    for (int k = 0; k < REGION_BAND; ++k) {
      const int64_t i = region_index(im, py0 + k, px);
      lab[k] = im.labels[i];
      val[k] = (int)values[i];
      if (WITHIN) on |= (unsigned)image_nonzero(im.within, im.wbytes, i) << k;
    }
  }
  __device__ __forceinline__ void judge(const RegionImage& im) {
    counted = refused = 0;
#pragma unroll
    for (int k = 0; k < REGION_BAND; ++k) {
      const RegionVerdict v = region_judge<WITHIN>(im, py0 + k, px, lab[k], on >> k & 1u);
      refused |= (unsigned)v.refused << k;
      counted |= (unsigned)v.counted << k;
    }
    first = (int)((int64_t)py0 * im.W + px);                     // < H W < 2^31 whenever a bit of `counted` is set
  }
};

__device__ __forceinline__ void region_refused(int* meta, unsigned refused) {      // bit k: the thread's pixel k is refused
  if (refused != 0) atomicAdd(meta, (int)__builtin_popcount(refused));
}

struct RegionMoments {
  int key[REGION_SLOTS], cnt[REGION_SLOTS];
  u64 sum[REGION_SLOTS], sq[REGION_SLOTS], kmin[REGION_SLOTS], kmax[REGION_SLOTS];
};

struct RegionTables {
  int* count;
  u64 *sum, *sumsq, *kmin, *kmax;      // sumsq may be null
};

// The five quantities of a run or of a slot into row i of five tables, in LDS or in global memory.  Inlined, so that every caller's
// atomics are those of its address space.
__device__ __forceinline__ void region_add(const RegionTables& p, bool with_sq, int i, int n, u64 sum, u64 sq, u64 kmn, u64 kmx) {
  atomicAdd(&p.count[i], n);
  atomicAdd(&p.sum[i], sum);
  if (with_sq) atomicAdd(&p.sumsq[i], sq);
  atomicMin(&p.kmin[i], kmn);
  atomicMax(&p.kmax[i], kmx);
}

template <typename T, bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_moments(RegionImage im, const T* __restrict__ values, RegionTables g, int* meta) {
  __shared__ RegionMoments t;
  for (int i = threadIdx.x; i < REGION_SLOTS; i += CGC_BLOCK) {
    t.key[i] = REGION_EMPTY;
    t.cnt[i] = 0;
    t.sum[i] = t.sq[i] = 0;
    t.kmin[i] = REGION_NO_MIN;
    t.kmax[i] = REGION_NO_MAX;
  }
  RegionColumn<T, WITHIN> c;
  c.fetch(im, values, region_spot(im.tiles_x), 0, 0);
  c.judge(im);
  __syncthreads();
  const bool with_sq = g.sumsq != nullptr;

  // the run in flight: label rl (REGION_EMPTY: none), rc pixels, their sum and sum of squares, the first smallest and first largest
  int rl = REGION_EMPTY, rc = 0, vmin = 0, imin = 0, vmax = 0, imax = 0;
  int64_t rs = 0, rq = 0;
  auto fold = [&]() {
    const u64 kmn = region_min_key(vmin, imin), kmx = region_max_key(vmax, imax);
    const int s = region_slot(t.key, rl);
    if (s >= 0) region_add(RegionTables{t.cnt, t.sum, t.sq, t.kmin, t.kmax}, with_sq, s, rc, (u64)rs, (u64)rq, kmn, kmx);
    else region_add(g, with_sq, rl, rc, (u64)rs, (u64)rq, kmn, kmx);
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
      const int v = c.val[k < REGION_BAND ? k : 0], i = c.first + k * im.W;
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
  region_refused(meta, c.refused);
  __syncthreads();
  for (int s = threadIdx.x; s < REGION_SLOTS; s += CGC_BLOCK) {
    const int L = t.key[s];
    if (L != REGION_EMPTY) region_add(g, with_sq, L, t.cnt[s], t.sum[s], t.sq[s], t.kmin[s], t.kmax[s]);
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

// The table of HISTOGRAM and COOCCURRENCE, in LDS: per slot 256 bins of 16 bits.  `out` is a global table of int32 counters whose row L
// starts `row_stride` counters after row L - 1.
struct RegionBins {
  int key[REGION_SLOTS];
  uint32_t bins[REGION_SLOTS * 128];      // slot s, bin b: the half b & 1 of dword 128 s + (b >> 1)
  __device__ __forceinline__ void clear() {
    for (int i = threadIdx.x; i < REGION_SLOTS; i += CGC_BLOCK) key[i] = REGION_EMPTY;
    for (int i = threadIdx.x; i < REGION_SLOTS * 128; i += CGC_BLOCK) bins[i] = 0;
  }
  __device__ __forceinline__ void add(int s, int b) { atomicAdd(&bins[s * 128 + (b >> 1)], 1u << ((b & 1) * 16)); }
  // Down a thread's 16 positions: where bit k of `mask` is set, label lab[k] gains one in each of the bins that bins_of(k, b) writes
  // to b[0 .. its result - 1], one or two: in its slot, or, where it has none, in its row of `out` (the direct route).  The slot of
  // the label above is kept; a label is looked up only where it changes.
  template <typename BinsOf>
  __device__ __forceinline__ void walk(const int (&lab)[REGION_BAND], unsigned mask, int* out, int64_t row_stride, BinsOf&& bins_of) {
    int cl = REGION_EMPTY, cs = -1;
#pragma unroll
    for (int k = 0; k < REGION_BAND; ++k) {
      if (!(mask >> k & 1u)) continue;
      const int L = lab[k];
      int b[2];
      const int nb = bins_of(k, b);
      if (L != cl) {
        cl = L;
        cs = region_slot(key, L);
      }
      if (cs >= 0) {
        add(cs, b[0]);
        if (nb == 2) add(cs, b[1]);
      } else {
        int* row = out + (int64_t)L * row_stride;
        atomicAdd(&row[b[0]], 1);
        if (nb == 2) atomicAdd(&row[b[1]], 1);
      }
    }
  }
  // Behind the caller's last barrier: thread v < nbins <= CGC_BLOCK adds bin v of every claimed slot to its row, where it is not zero.
  __device__ __forceinline__ void flush(int* out, int64_t row_stride, int nbins) const {
    const int v = threadIdx.x;
    if (v >= nbins) return;
    for (int s = 0; s < REGION_SLOTS; ++s) {
      const int L = key[s];                                       // uniform
      if (L == REGION_EMPTY) continue;
      const int n = (int)(bins[s * 128 + (v >> 1)] >> ((v & 1) * 16) & 0xffffu);
      if (n != 0) atomicAdd(&out[(int64_t)L * row_stride + v], n);
    }
  }
};

template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_hist(RegionImage im, const uint8_t* __restrict__ values, int* hist, int* meta) {
  __shared__ RegionBins t;
  t.clear();
  RegionColumn<uint8_t, WITHIN> c;
  c.fetch(im, values, region_spot(im.tiles_x), 0, 0);
  c.judge(im);
  __syncthreads();
  t.walk(c.lab, c.counted, hist, 256, [&](int k, int (&b)[2]) { b[0] = c.val[k]; return 1; });      // one bin: the value
  region_refused(meta, c.refused);
  __syncthreads();
  t.flush(hist, 256, 256);
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

struct RegionCall {                      // the host side that the four tile kernels share
  RegionImage im;                        // wbytes is 0 where within is null
  dim3 grid;                             // a workgroup per tile
  bool empty;                            // H W = 0: no tile launch, the tables of empty rows
};
// False: the call is refused.  `planes`: every plane the mode reads was given; an empty image needs none.
static inline bool region_call(RegionCall& c, const int* labels, bool planes, const void* within, int wbytes, int H, int W, int max_label) {
  if (bad_image_dims(H, W) || max_label < 0 || max_label == 0x7fffffff || (within != nullptr && bad_elem_bytes(wbytes))) return false;
  c.empty = (int64_t)H * W == 0;
  if (!c.empty && !planes) return false;
  const int tiles_x = ceil_div(W, REGION_TILE);
  c.im = RegionImage{labels, within, within != nullptr ? wbytes : 0, H, W, tiles_x, max_label};
  c.grid = dim3((unsigned)((int64_t)tiles_x * ceil_div(H, REGION_TILE)));      // < 2^31 / 4096 + H / 64 + W / 64 + 1
  return true;
}
// launch(std::true_type{}) where the call has a `within`, launch(std::false_type{}) where not: the WITHIN of the kernel to launch
template <typename Launch>
static inline void region_launch(const RegionCall& c, Launch&& launch) {
  if (c.im.within != nullptr) launch(std::true_type{});
  else launch(std::false_type{});
}
static inline int region_blocks(int64_t rows) {
  const int64_t b = ceil_div64(rows, CGC_BLOCK);
  return (int)(b < REGION_INIT_BLOCKS ? b : REGION_INIT_BLOCKS);
}

struct CoocLut {
  uint32_t w[64];                        // the level of value v: byte v & 3 of dword v >> 2
};

// One offset (dy, dx) of COOCCURRENCE.  The anchor p is the thread's pixel, the partner q = p + (dy, dx) a second column loaded beside
// the first; a pair is counted where both are counted and their labels agree.  The tile that holds p counts the pair, wherever q
// lies.  `out` is the table of this offset, tables + k * levels^2; a row is `row_stride` = noff * levels^2 counters further on.
template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_cooc(RegionImage im, const uint8_t* __restrict__ values, CoocLut lut, int levels, int dy,
                                                           int dx, int symmetric, int count_refused, int* out, int64_t row_stride, int* meta) {
  __shared__ RegionBins t;
  __shared__ uint32_t level_words[64];                           // the lut, for lookups by lane
  t.clear();
  if (threadIdx.x < 64) level_words[threadIdx.x] = lut.w[threadIdx.x];
  const RegionSpot s = region_spot(im.tiles_x);
  RegionColumn<uint8_t, WITHIN> c, q;                             // the anchors, the partners
  c.fetch(im, values, s, 0, 0);
  q.fetch(im, values, s, dy, dx);
  c.judge(im);
  q.judge(im);
  unsigned pair = 0;                                              // bit k: anchor k and its partner are a counted pair
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) pair |= (unsigned)(q.lab[k] == c.lab[k]) << k;
  pair &= c.counted & q.counted;
  __syncthreads();
  const uint8_t* level = reinterpret_cast<const uint8_t*>(level_words);
  t.walk(c.lab, pair, out, row_stride, [&](int k, int (&b)[2]) {
    const int lc = level[c.val[k]], lq = level[q.val[k]];
    b[0] = lc * levels + lq, b[1] = lq * levels + lc;             // < levels^2 <= 256: the host checked every entry of the lut
    return symmetric ? 2 : 1;
  });
  if (count_refused) region_refused(meta, c.refused);
  __syncthreads();
  t.flush(out, row_stride, levels * levels);
}

constexpr int GEOM_NONE = REGION_EMPTY;                          // GEOMETRY: the row of a position that belongs to none
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

// n pixels of row L, `border` of them on the image's frame, and their five sums in the coordinates of the tile at (ox, oy): shifted to
// image coordinates, in 64 bits, and added to the global tables.  A slot at the flush; on the direct route a run, a table of one.
__device__ __forceinline__ void geom_add(const GeomTables& g, int L, int ox, int oy, int64_t n, int border, int64_t sy, int64_t sx, int64_t syy,
                                         int64_t sxy, int64_t sxx) {
  atomicAdd(&g.count[L], (int)n);
  if (border != 0) atomicAdd(&g.border[L], border);
  atomicAdd(&g.sy[L], (u64)(sy + n * oy));
  atomicAdd(&g.sx[L], (u64)(sx + n * ox));
  atomicAdd(&g.syy[L], (u64)(syy + 2 * oy * sy + n * oy * oy));
  atomicAdd(&g.sxy[L], (u64)(sxy + ox * sy + oy * sx + n * ox * oy));
  atomicAdd(&g.sxx[L], (u64)(sxx + 2 * ox * sx + n * ox * ox));
}

// One tile.  The label every position of the tile and of a frame of one position around it belongs to (GEOM_NONE: to none) is staged
// in LDS, so that runs and quads are walked by loops over k, not by unrolled copies of their bodies: a fold is 23 atomics and a slot
// lookup, and sixteen copies of it per thread do not fit the instruction cache.
template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_geometry(RegionImage im, GeomTables g, int* meta) {
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
  const RegionSpot sp = region_spot(im.tiles_x);
  const int H = im.H, W = im.W, ty = sp.ty, tx = sp.tx, ox = sp.ox, oy = sp.oy, lx = sp.lx, ly0 = sp.ly0, x = sp.x, y0 = sp.y0;
  auto belongs = [&](int py, int px, bool& bad) -> int {          // the row position (py, px) belongs to; `bad`: it is refused
    const int64_t i = region_index(im, py, px);
    const int L = im.labels[i];
    const RegionVerdict v = region_judge<WITHIN>(im, py, px, L, WITHIN && image_nonzero(im.within, im.wbytes, i));
    bad = v.refused;
    return v.counted ? L : GEOM_NONE;
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
    if (sp.last_band) e[REGION_TILE + 1][lx + 1] = belongs(oy + REGION_TILE, x, bad);      // the row below the tile
    if (sp.last_lane) {                                              // the column to its right
#pragma unroll
      for (int k = 0; k < REGION_BAND; ++k) e[ly0 + k + 1][REGION_TILE + 1] = belongs(y0 + k, x + 1, bad);
      if (sp.last_band) e[REGION_TILE + 1][REGION_TILE + 1] = belongs(oy + REGION_TILE, x + 1, bad);
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
    } else {                                                      // no slot: the run goes to the global tables as a slot of its own would
      geom_add(g, L, ox, oy, n, rb, rsy, n * lx, rsyy, rsy * lx, n * lx * lx);
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
  region_refused(meta, refused);
  __syncthreads();

  // flush: a wave per quarter of a slot's words, shifted to image coordinates
  const int s = threadIdx.x & (REGION_SLOTS - 1), part = threadIdx.x / REGION_SLOTS;
  const int L = t.key[s];
  if (L == REGION_EMPTY) return;                                  // after the last barrier
  if (part == 0) {
    if (t.cnt[s] == 0) return;                                    // a slot claimed by a quad alone
    geom_add(g, L, ox, oy, t.cnt[s], t.border[s], t.sy[s], t.sx[s], t.syy[s], t.sxy[s], t.sxx[s]);
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
static_assert(CGC_BLOCK == 256 && CGC_BLOCK == REGION_SLOTS * 4, "a flush: RegionBins, a thread per bin; k_region_geometry, a wave per quarter of a slot");

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

// HULL: the convex hull of the pixel SQUARES of every row (KernelSpec.region_hull; DESIGN.md, "Region hull").  Stage 1, a tile kernel:
// per row L and image row y of its bounding box, the smallest and largest column of its pixels, spans[ptr[L] + y - y0[L]] = (xmin,
// xmax); y0 is the extent (0, 1) of GEOMETRY, ptr the prefix sum of the bounding boxes' heights.  Stage 2, per region: the points of
// the lattice lines, Andrew's monotone chain down the left side and up the right, then area, diameter, width and perimeter.
constexpr int HULL_NONE = REGION_EMPTY;
constexpr int HULL_NO_MIN = 0x7fffffff, HULL_NO_MAX = (int)0x80000000;      // an image row in which the label has no pixel
// Rows above which a region is hulled by a whole wave, not by one lane (exported).  Measured on an MI355X (tools/hull_bench.py,
// profiles/hull_bench.json), the two hull launches on an image that is ONE region of H rows, lane / wave, ms:
//   every pixel        H = 64: 0.096 / 0.081   128: 0.134 / 0.092   256: 0.216 / 0.101   512: 0.393 / 0.110   1024: 0.743 / 0.119   4096: 3.05 / 0.227
//   inscribed ellipse  H = 64: 0.434 / 0.143   128: 0.852 / 0.192   256: 1.203 / 0.240   512: 2.245 / 0.290   1024: 3.056 / 0.342   4096: 47.4 / 1.38
// A lone region is never slower on the wave: the other 63 lanes had nothing to do anyway.  But a wave takes its tall regions one
// after another, 0.06 to 0.15 ms each at 64 to 256 rows, where 64 lanes hull 64 such regions at once in 0.35 to 1.1 ms: the
// threshold belongs above everything that comes in crowds -- a nucleus is tens of rows high -- and it bounds what one lane can cost,
// 1.2 ms at 256 rows and twice that at 512.
constexpr int HULL_TALL_ROWS = 256;

struct HullPoint { int y, x; };          // a lattice corner, as the vertices are returned

struct HullSpans {
  const int64_t* ptr;                    // [R + 1]
  const int* ext;                        // [R, 8, 2] of GEOMETRY
  int* spans;                            // [total, 2]
  int64_t total;
};

__global__ void __launch_bounds__(CGC_BLOCK) k_hull_spans_init(int64_t total, int* __restrict__ spans) {
  for (int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * CGC_BLOCK) {
    spans[2 * i] = HULL_NO_MIN;
    spans[2 * i + 1] = HULL_NO_MAX;
  }
}

// One tile.  A wave is one row of it: a pixel is the first of a run where the lane to its left holds another row (or is none, or is
// the tile's first column) and the last where the lane to its right does; only these send an atomic, two per run and tile row.
template <bool WITHIN>
__global__ void __launch_bounds__(CGC_BLOCK) k_region_hull_spans(RegionImage im, HullSpans hs) {
  const RegionSpot sp = region_spot(im.tiles_x);
  RegionColumn<int, WITHIN> c;
  c.fetch(im, im.labels, sp, 0, 0);      // no second plane: the labels stand in for the values
  c.judge(im);
  unsigned lo = 0, hi = 0;               // bit k: pixel k starts a run of its image row; ends one
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) {
    const int L = (c.counted >> k & 1u) ? c.lab[k] : HULL_NONE;
    const int left = __shfl_up(L, 1), right = __shfl_down(L, 1);
    lo |= (unsigned)(L != HULL_NONE && (sp.lx == 0 || left != L)) << k;
    hi |= (unsigned)(L != HULL_NONE && (sp.last_lane || right != L)) << k;
  }
#pragma unroll
  for (int k = 0; k < REGION_BAND; ++k) {                           // unrolled: lab[k] stays in registers
    if (!((lo | hi) >> k & 1u)) continue;
    const int L = c.lab[k];
    const int64_t p0 = hs.ptr[L], p1 = hs.ptr[L + 1];
    const int64_t i = p0 + (sp.y0 + k - hs.ext[(int64_t)L * (GEOM_DIRS * 2) + 8]);
    if (i < p0 || i >= p1 || i < 0 || i >= hs.total) continue;      // a ptr that does not fit the extents: nothing is written outside
    if (lo >> k & 1u) atomicMin(&hs.spans[2 * i], sp.x);
    if (hi >> k & 1u) atomicMax(&hs.spans[2 * i + 1], sp.x);
  }
}

struct HullJob {
  const int64_t* ptr;
  const int* ext;
  const int* spans;
  HullPoint* points;                     // [2 (total + rows)]: row L owns 2 (h + 1) from 2 (ptr[L] + L), its vertices first
  int64_t total;
  int rows, tall;
};
struct HullTables {
  int* count;                            // [R]
  long long *area2, *diameter2;          // [R]
  int* ends;                             // [R, 2, 2]
  long long* width_cross;                // [R]
  int* width_edge;                       // [R, 2]
  double* perimeter;                     // [R]
};

// (a - o) x (b - o) with x to the right and y down the image: negative at every vertex of a hull listed down its left side first
__device__ __forceinline__ long long hull_cross(HullPoint o, HullPoint a, HullPoint b) {
  return (long long)(a.x - o.x) * (b.y - o.y) - (long long)(a.y - o.y) * (b.x - o.x);
}
// p onto the stack st[0 .. top): what p makes reflex or collinear is dropped first
__device__ __forceinline__ void hull_push(HullPoint* st, int& top, HullPoint p) {
  for (; top >= 2; --top)
    if (hull_cross(st[top - 2], st[top - 1], p) < 0) break;
  st[top++] = p;
}
// The chain of the points t0 .. t1 - 1 of one side, in hull order: point t of the left side lies on lattice line r = t (down the
// image), of the right side on r = h - t (up).  Line r has the rows r - 1 and r of the label's h rows beside it; the point is the
// outermost corner of both, and there is none between two rows without a pixel.  Returns the number of points left in st.
template <bool LEFT>
__device__ __forceinline__ int hull_side(const int* __restrict__ spans, int h, int y0, int t0, int t1, HullPoint* st) {
  constexpr int NO = LEFT ? HULL_NO_MIN : HULL_NO_MAX, word = LEFT ? 0 : 1;
  int top = 0;
  for (int t = t0; t < t1; ++t) {
    const int r = LEFT ? t : h - t;
    const int a = r > 0 ? spans[2 * (r - 1) + word] : NO, b = r < h ? spans[2 * r + word] : NO;
    const int x = LEFT ? (a < b ? a : b) : (a > b ? a : b);
    if (x != NO) hull_push(st, top, HullPoint{y0 + r, LEFT ? x : x + 1});
  }
  return top;
}

// is ca / sqrt(la) < cb / sqrt(lb)?  ca^2 lb against cb^2 la, exactly: crosses reach 2^31 and squared lengths 2^31, the products 2^93
__device__ __forceinline__ bool hull_narrower(u64 ca, u64 la, u64 cb, u64 lb) {
  const u64 pa = ca * ca, pb = cb * cb;
  const u64 ha = __umul64hi(pa, lb), hb = __umul64hi(pb, la);
  return ((int)(ha < hb) | ((int)(ha == hb) & (int)(pa * lb < pb * la))) != 0;      // no branch: see hull_measure
}

// The tables of row L from its k >= 4 vertices v, by one lane (WAVE false) or by the 64 lanes of a wave.  Diameter and width are
// scans over all pairs: a lattice polygon inside a square of side n has O(n^(2/3)) vertices, a nucleus some twenty.
template <bool WAVE>
__device__ __forceinline__ void hull_measure(const HullPoint* v, int k, int lane, const HullTables& out, int64_t L) {
  constexpr int NL = WAVE ? CGC_WAVE : 1;
  // the diameter: of equal pairs the smallest (i, j), i < j -- in a lane by the strict comparison, between lanes by i
  long long bd = -1;
  int bi = 0, bj = 0;
  for (int i = lane; i < k; i += NL) {
    const HullPoint a = v[i];
    for (int j = i + 1; j < k; ++j) {
      const long long dy = v[j].y - a.y, dx = v[j].x - a.x, d = dy * dy + dx * dx;
      const bool far = d > bd;
      bd = far ? d : bd, bi = far ? i : bi, bj = far ? j : bj;
    }
  }
  // the width: per edge the farthest vertex, of equal widths the first edge
  // The best edge travels as (c, |e|^2, e) through selects, and (dy, dx) is read off the vertices at the end: with the update
  // written as a branch around five assignments, hipcc -O3 (ROCm 7) kept the OLD (dy, dx) on the path where the high halves of the
  // two 128-bit products are equal and the low halves decide -- both are 0 for any nucleus -- while c and e were updated.
  u64 bc = 0, bl = 0;
  int be = -1;
  for (int e = lane; e < k; e += NL) {
    const HullPoint a = v[e], b = v[e + 1 < k ? e + 1 : 0];
    const int dy = b.y - a.y, dx = b.x - a.x;
    long long c = 0;
    for (int j = 0; j < k; ++j) {
      const long long cj = (long long)dy * (v[j].x - a.x) - (long long)dx * (v[j].y - a.y);
      c = cj > c ? cj : c;
    }
    const u64 len = (u64)((long long)dy * dy + (long long)dx * dx);
    const bool take = ((int)(be < 0) | (int)hull_narrower((u64)c, len, bc, bl)) != 0;
    bc = take ? (u64)c : bc, bl = take ? len : bl, be = take ? e : be;
  }
  if (WAVE) {
#pragma unroll
    for (int m = 1; m < CGC_WAVE; m <<= 1) {
      const long long od = __shfl_xor(bd, m);
      const int oi = __shfl_xor(bi, m), oj = __shfl_xor(bj, m);
      const bool far = ((int)(od > bd) | ((int)(od == bd) & (int)(oi < bi))) != 0;
      bd = far ? od : bd, bi = far ? oi : bi, bj = far ? oj : bj;
      const u64 oc = __shfl_xor(bc, m), ol = __shfl_xor(bl, m);
      const int oe = __shfl_xor(be, m);
      const int first = (int)!hull_narrower(bc, bl, oc, ol) & (int)(oe < be);      // as narrow, and earlier in hull order
      const bool take = ((int)(oe >= 0) & ((int)(be < 0) | (int)hull_narrower(oc, ol, bc, bl) | first)) != 0;
      bc = take ? oc : bc, bl = take ? ol : bl, be = take ? oe : be;
    }
  }
  if (lane != 0) return;
  long long s = 0;
  double per = 0.0;
  for (int i = 0; i < k; ++i) {                                     // in hull order
    const HullPoint a = v[i], b = v[i + 1 < k ? i + 1 : 0];
    s += (long long)a.x * b.y - (long long)b.x * a.y;
    const long long dy = b.y - a.y, dx = b.x - a.x;
    per += sqrt((double)(dy * dy + dx * dx));
  }
  out.count[L] = k;
  out.area2[L] = -s;
  out.diameter2[L] = bd;
  out.ends[4 * L] = v[bi].y, out.ends[4 * L + 1] = v[bi].x, out.ends[4 * L + 2] = v[bj].y, out.ends[4 * L + 3] = v[bj].x;
  const HullPoint ea = v[be < 0 ? 0 : be], eb = v[be + 1 < k ? be + 1 : 0];
  out.width_cross[L] = (long long)bc;
  out.width_edge[2 * L] = eb.y - ea.y, out.width_edge[2 * L + 1] = eb.x - ea.x;
  out.perimeter[L] = per;
}

// A tall region, by a whole wave (uniform arguments): each lane hulls a 64th of the lines of both sides in place, lane 0 merges the 64
// chains -- a chain of chains is hulled like a chain of points -- and the wave measures.  What one lane wrote is read by another
// only behind a fence.
__device__ __forceinline__ void hull_tall(const HullJob& job, const HullTables& out, int64_t L, int h, int64_t p0, int lane) {
  HullPoint* st = job.points + 2 * (p0 + L);
  const int* spans = job.spans + 2 * p0;
  const int y0 = job.ext[L * (GEOM_DIRS * 2) + 8];
  const int n = h + 1, per = (n + CGC_WAVE - 1) / CGC_WAVE;
  const int t0 = lane * per < n ? lane * per : n, t1 = t0 + per < n ? t0 + per : n;
  const int cl = hull_side<true>(spans, h, y0, t0, t1, st + t0);
  const int cr = hull_side<false>(spans, h, y0, t0, t1, st + n + t0);
  __threadfence();
  int nl = 0, nr = 0;
  for (int c = 0; c < CGC_WAVE; ++c) {                              // the stack never passes the point it reads: top <= c per + p
    const int cnt = __shfl(cl, c);
    if (lane == 0)
      for (int p = 0; p < cnt; ++p) hull_push(st, nl, st[c * per + p]);
  }
  nl = __shfl(nl, 0);
  for (int c = 0; c < CGC_WAVE; ++c) {                              // ... and nl <= n: the right side lands behind the left
    const int cnt = __shfl(cr, c);
    if (lane == 0)
      for (int p = 0; p < cnt; ++p) hull_push(st + nl, nr, st[n + c * per + p]);
  }
  nr = __shfl(nr, 0);
  __threadfence();
  hull_measure<true>(st, nl + nr, lane, out, L);
}

// A lane per region up to job.tall rows; then the wave takes the taller ones among its 64 one after the other.
__global__ void __launch_bounds__(CGC_BLOCK) k_region_hull(HullJob job, HullTables out) {
  const int lane = threadIdx.x & (CGC_WAVE - 1);
  const int64_t L = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  int h = 0;
  int64_t p0 = 0;
  if (L < job.rows) {
    const int64_t a = job.ptr[L], b = job.ptr[L + 1];
    if (a >= 0 && b >= a && b <= job.total && b - a <= GEOM_MAX_SIDE) p0 = a, h = (int)(b - a);      // else: an empty row
  }
  const bool tall = h > job.tall;
  if (L < job.rows && !tall) {
    if (h == 0) {
      out.count[L] = 0;
      out.area2[L] = out.diameter2[L] = out.width_cross[L] = 0;
      out.ends[4 * L] = out.ends[4 * L + 1] = out.ends[4 * L + 2] = out.ends[4 * L + 3] = 0;
      out.width_edge[2 * L] = out.width_edge[2 * L + 1] = 0;
      out.perimeter[L] = 0.0;
    } else {
      HullPoint* st = job.points + 2 * (p0 + L);
      const int y0 = job.ext[L * (GEOM_DIRS * 2) + 8];
      const int nl = hull_side<true>(job.spans + 2 * p0, h, y0, 0, h + 1, st);
      const int nr = hull_side<false>(job.spans + 2 * p0, h, y0, 0, h + 1, st + nl);
      hull_measure<false>(st, nl + nr, 0, out, L);
    }
  }
  u64 todo = __ballot(tall);
  for (int round = 0; round < CGC_WAVE && todo != 0; ++round) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    hull_tall(job, out, L - lane + src, __shfl(h, src), __shfl(p0, src), lane);
  }
}

struct HullWs {
  HullPoint* points;
};
static inline HullWs hull_layout(Carver&& c, int64_t rows, int64_t span_rows) {
  HullWs w;
  w.points = c.take<HullPoint>(2 * (span_rows + rows));
  return w;
}
// span_rows = ptr[R], read by the caller: no label has more rows than the image
static inline bool bad_hull_rows(int max_label, int H, int64_t span_rows) {
  return max_label < 0 || max_label == 0x7fffffff || H < 0 || H > GEOM_MAX_SIDE || span_rows < 0 || span_rows > ((int64_t)max_label + 1) * H;
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
  RegionCall c;
  if (!region_call(c, labels, labels != nullptr && values != nullptr, within_or_null, within_bytes, H, W, max_label)) return CGC_EINVAL;
  const bool u8 = value_bytes == 1 && value_signed == 0, i8 = value_bytes == 1 && value_signed == 1;
  const bool i16 = value_bytes == 2 && value_signed == 1, i32 = value_bytes == 4 && value_signed == 1;
  if (!(u8 || i8 || i16 || i32) || (i32 && sumsq_or_null != nullptr)) return CGC_EINVAL;
  if (ws == nullptr || count == nullptr || sum == nullptr || min == nullptr || max == nullptr || argmin == nullptr || argmax == nullptr ||
      meta == nullptr)
    return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int rows = max_label + 1;
  const RegionWs w = region_layout(Carver(ws), rows);
  const RegionTables g{count, reinterpret_cast<u64*>(sum), reinterpret_cast<u64*>(sumsq_or_null), w.kmin, w.kmax};
  hipLaunchKernelGGL(k_region_init, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, g, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  if (!c.empty) {
    region_launch(c, [&](auto within) {
      auto of = [&](auto v) {                                     // v: a value of the plane's type
        hipLaunchKernelGGL((k_region_moments<decltype(v), decltype(within)::value>), c.grid, dim3(CGC_BLOCK), 0, st, c.im,
                           static_cast<const decltype(v)*>(values), g, meta);
      };
      if (u8) of(uint8_t{});
      else if (i8) of(int8_t{});
      else if (i16) of(int16_t{});
      else of(int32_t{});
    });
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  hipLaunchKernelGGL(k_region_finish, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, count, w.kmin, w.kmax, min, max, argmin, argmax);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_histogram(const int* labels, const uint8_t* values, const void* within_or_null, int within_bytes, int H, int W,
                                    int max_label, int* hist, int* meta, cgc_stream_t stream) {
  RegionCall c;
  if (!region_call(c, labels, labels != nullptr && values != nullptr, within_or_null, within_bytes, H, W, max_label)) return CGC_EINVAL;
  if (hist == nullptr || meta == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  hipError_t e = hipMemsetAsync(hist, 0, ((size_t)max_label + 1) * 256 * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (c.empty) return 0;
  region_launch(c, [&](auto within) {
    hipLaunchKernelGGL(k_region_hist<decltype(within)::value>, c.grid, dim3(CGC_BLOCK), 0, st, c.im, values, hist, meta);
  });
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_cooc_max_offset(void) { return COOC_MAX_OFFSET; }
extern "C" int cgc_region_cooc_max_offsets(void) { return COOC_MAX_OFFSETS; }

extern "C" int cgc_region_cooccurrence(const int* labels, const uint8_t* values, const void* within_or_null, int within_bytes, int H, int W,
                                       int max_label, const uint8_t* lut256_host, int levels, const int* offsets_host, int noff,
                                       int symmetric, int* tables, int* meta, cgc_stream_t stream) {
  RegionCall c;
  if (!region_call(c, labels, labels != nullptr && values != nullptr, within_or_null, within_bytes, H, W, max_label)) return CGC_EINVAL;
  if ((int64_t)H * W >= COOC_MAX_PIXELS) return CGC_EINVAL;
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
  hipStream_t st = as_stream(stream);
  const int bins = levels * levels;
  const int64_t row_stride = (int64_t)noff * bins;
  hipError_t e = hipMemsetAsync(tables, 0, ((size_t)max_label + 1) * (size_t)row_stride * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (c.empty) return 0;
  for (int k = 0; k < noff; ++k) {                                // one launch per offset; the first counts the refused pixels
    region_launch(c, [&](auto within) {
      hipLaunchKernelGGL(k_region_cooc<decltype(within)::value>, c.grid, dim3(CGC_BLOCK), 0, st, c.im, values, lut, levels, offsets_host[2 * k],
                         offsets_host[2 * k + 1], (int)(symmetric != 0), (int)(k == 0), tables + (int64_t)k * bins, row_stride, meta);
    });
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_region_geometry_max_side(void) { return GEOM_MAX_SIDE; }

extern "C" int cgc_region_geometry(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label, int* count,
                                   int64_t* sums, int* extents, int* quads, int* border, int* meta, cgc_stream_t stream) {
  RegionCall c;
  if (!region_call(c, labels, labels != nullptr, within_or_null, within_bytes, H, W, max_label)) return CGC_EINVAL;
  if (H > GEOM_MAX_SIDE || W > GEOM_MAX_SIDE || ((int64_t)H + 1) * ((int64_t)W + 1) >= ((int64_t)1 << 31)) return CGC_EINVAL;
  if (count == nullptr || sums == nullptr || extents == nullptr || quads == nullptr || border == nullptr || meta == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int rows = max_label + 1;
  u64* s = reinterpret_cast<u64*>(sums);                          // [5, rows]: sy, sx, syy, sxy, sxx
  const GeomTables g{count, s, s + rows, s + 2 * (int64_t)rows, s + 3 * (int64_t)rows, s + 4 * (int64_t)rows, extents, quads, border};
  hipLaunchKernelGGL(k_geometry_init, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, g, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  if (!c.empty) {
    region_launch(c, [&](auto within) {
      hipLaunchKernelGGL(k_region_geometry<decltype(within)::value>, c.grid, dim3(CGC_BLOCK), 0, st, c.im, g, meta);
    });
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  hipLaunchKernelGGL(k_geometry_finish, dim3(region_blocks(rows)), dim3(CGC_BLOCK), 0, st, rows, count, extents);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_hull_tall_rows(void) { return HULL_TALL_ROWS; }

extern "C" int64_t cgc_region_hull_ws_bytes(int max_label, int64_t span_rows) {
  if (bad_hull_rows(max_label, GEOM_MAX_SIDE, span_rows)) return 0;
  return layout_bytes(hull_layout, (int64_t)max_label + 1, span_rows);
}

extern "C" int cgc_region_hull_spans(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label,
                                     const int* extents, const int64_t* ptr, int64_t span_rows, int* spans, cgc_stream_t stream) {
  RegionCall c;
  if (!region_call(c, labels, labels != nullptr, within_or_null, within_bytes, H, W, max_label)) return CGC_EINVAL;
  if (W > GEOM_MAX_SIDE || bad_hull_rows(max_label, H, span_rows)) return CGC_EINVAL;
  if (extents == nullptr || ptr == nullptr || (span_rows > 0 && spans == nullptr)) return CGC_EINVAL;
  if (span_rows == 0) return 0;                                    // an empty image, or no label with a pixel
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_hull_spans_init, dim3(region_blocks(span_rows)), dim3(CGC_BLOCK), 0, st, span_rows, spans);
  CGC_RETURN_IF_LAUNCH_FAILED();
  const HullSpans hs{ptr, extents, spans, span_rows};
  region_launch(c, [&](auto within) {
    hipLaunchKernelGGL(k_region_hull_spans<decltype(within)::value>, c.grid, dim3(CGC_BLOCK), 0, st, c.im, hs);
  });
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_hull(int max_label, int H, const int* extents, const int64_t* ptr, int64_t span_rows, const int* spans, void* ws,
                               int tall_rows, int* count, int64_t* area2, int64_t* diameter2, int* diameter_ends, int64_t* width_cross,
                               int* width_edge, double* perimeter, cgc_stream_t stream) {
  if (bad_hull_rows(max_label, H, span_rows) || tall_rows < 0) return CGC_EINVAL;
  if (extents == nullptr || ptr == nullptr || (span_rows > 0 && spans == nullptr) || ws == nullptr) return CGC_EINVAL;
  if (count == nullptr || area2 == nullptr || diameter2 == nullptr || diameter_ends == nullptr || width_cross == nullptr ||
      width_edge == nullptr || perimeter == nullptr)
    return CGC_EINVAL;
  const int rows = max_label + 1;
  const HullWs w = hull_layout(Carver(ws), rows, span_rows);
  const HullJob job{ptr, extents, spans, w.points, span_rows, rows, tall_rows > 0 ? tall_rows : HULL_TALL_ROWS};
  const HullTables out{count, reinterpret_cast<long long*>(area2), reinterpret_cast<long long*>(diameter2), diameter_ends,
                       reinterpret_cast<long long*>(width_cross), width_edge, perimeter};
  hipLaunchKernelGGL(k_region_hull, dim3((unsigned)ceil_div64(rows, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), job, out);
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
