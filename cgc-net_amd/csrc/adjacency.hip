// Region adjacency of a label image on gfx950: which regions touch, along how many pixel pairs, and (with a value plane) the smallest
// value[p] + value[q] over each pair's contacts.  Contract item by item: cgc-net_amd/kernels.py KernelSpec.region_adjacency; table
// design, launches and measurements: DESIGN.md, "Region adjacency and Voronoi graphs".
//
// A contact is owned by the earlier of its two pixels in raster order: pixel (y, x) looks right, down and (connectivity 2) down-right
// and down-left, so every unordered pixel pair is seen once.  Launches of one call:
//   k_adj_tiles<false>  one 64 x 64 tile per workgroup (+ a one-pixel halo left, right and below): labels in LDS, contacts folded into
//                       an LDS hash table keyed by (a, b); per tile the number of records it will write
//   k_adj_scan          ONE workgroup: exclusive scan of the per-tile counts, the total to device memory     -- host read 1: records
//   k_adj_tiles<true>   the same fold again; each tile writes its distinct (key, count, min) records at its offset
//   (the caller sorts the 64-bit keys)
//   k_adj_heads         first records of runs of equal keys, counted per block of 2048 sorted records
//   k_adj_scan          their exclusive scan, the total to device memory                                   -- host read 2: pairs
//   k_adj_init, k_adj_merge   count = 0, min = INT32_MAX; every record adds its count to and takes the minimum into the row of its run
// OVERFLOW.  The LDS table has ADJ_SLOTS slots and a tile may use ADJ_LIMIT of them.  A tile with more distinct pairs than ADJ_LIMIT is
// `dense`: it writes one record PER CONTACT instead (count 1), and its record count is its contact count.  Whether a tile is dense
// depends only on its pixels, not on the order in which lanes reach the table: `distinct` counts claimed slots, it passes ADJ_LIMIT iff
// the tile has more distinct keys than that, and the table cannot fill up before the flag is seen -- every thread claims at most one
// slot between two looks at the flag, so at most ADJ_LIMIT + CGC_BLOCK < ADJ_SLOTS slots are ever claimed.  The two tile launches
// therefore agree on every tile's record count, and all integer sums and minima are independent of arrival order.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

constexpr int ADJ_TILE = 64;                      // tile side (exported: the tests place seams from it)
constexpr int ADJ_ROWS = ADJ_TILE + 1;            // + the row below
constexpr int ADJ_COLS = ADJ_TILE + 2;            // + the columns left and right
constexpr int ADJ_BAND = ADJ_TILE * ADJ_TILE / CGC_BLOCK;      // 16 consecutive rows of one column per thread
constexpr int ADJ_LOADS = (ADJ_ROWS * ADJ_COLS + CGC_BLOCK - 1) / CGC_BLOCK;      // 17 staged labels per thread
constexpr int ADJ_SLOTS = 1024;
constexpr int ADJ_LIMIT = 512;                    // distinct pairs a tile may fold; ADJ_LIMIT + CGC_BLOCK < ADJ_SLOTS (see OVERFLOW)
constexpr int ADJ_SCAN = 2048;                    // sorted records per merge block, 8 consecutive ones per thread
constexpr int ADJ_PER_THREAD = ADJ_SCAN / CGC_BLOCK;
constexpr int INT32_MAX_ = 0x7fffffff;
static_assert(ADJ_LIMIT + CGC_BLOCK < ADJ_SLOTS, "the table must outlast the threads that have not yet seen the dense flag");

// (a, b), a < b as signed integers, as one int64 whose signed order is the lexicographic order of (a, b)
__host__ __device__ __forceinline__ int64_t adj_key(int a, int b) {
  return (int64_t)(((uint64_t)(uint32_t)a << 32) | (uint32_t)((uint32_t)b ^ 0x80000000u));
}
constexpr unsigned long long ADJ_EMPTY = 0x80000000ull;      // adj_key(0, 0): no pair, 0 is background

struct AdjWs {
  int* tile_off;     // [tiles + 1] records per tile, then their exclusive scan
  int* dense;        // [tiles] 1: the tile writes one record per contact
};
static inline int64_t adj_tiles(int H, int W) { return (int64_t)ceil_div(H, ADJ_TILE) * ceil_div(W, ADJ_TILE); }
static inline AdjWs adj_layout(Carver&& c, int64_t tiles) {
  AdjWs w;
  w.tile_off = c.take<int>(tiles + 1);
  w.dense = c.take<int>(tiles);
  return w;
}
struct MergeWs {
  int* blocks;       // [nblocks] run heads per block of sorted records, then their exclusive scan
};
static inline int64_t merge_blocks(int64_t n) { return ceil_div64(n, ADJ_SCAN); }
static inline MergeWs merge_layout(Carver&& c, int64_t n) {
  MergeWs w;
  w.blocks = c.take<int>(merge_blocks(n));
  return w;
}

__device__ __forceinline__ int clamp_sum(int u, int v) {
  const int64_t s = (int64_t)u + v;
  return s > INT32_MAX_ ? INT32_MAX_ : s < -(int64_t)INT32_MAX_ - 1 ? -INT32_MAX_ - 1 : (int)s;
}

struct AdjTable {
  unsigned long long key[ADJ_SLOTS];
  int cnt[ADJ_SLOTS];
  int mn[ADJ_SLOTS];
  int claimed[ADJ_SLOTS];      // the slots in the order they were claimed: what the write launch walks instead of the whole table
  int distinct, dense, contacts, wpos;
};

// fold (k, c contacts, smallest sum s) into the table; gives up once the tile is known to be dense
__device__ __forceinline__ void adj_insert(AdjTable& t, unsigned long long k, int c, int s, bool with_value) {
  unsigned h = ((unsigned)(k >> 32) * 0x9E3779B1u) ^ ((unsigned)k * 0x85EBCA6Bu);
  h = (h ^ (h >> 15)) & (ADJ_SLOTS - 1);
  for (;;) {
    if (__hip_atomic_load(&t.dense, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
    const unsigned long long prev = atomicCAS(&t.key[h], ADJ_EMPTY, k);
    if (prev == ADJ_EMPTY) {
      const int n = atomicAdd(&t.distinct, 1);
      if (n < ADJ_SLOTS) t.claimed[n] = (int)h;      // always true: at most ADJ_LIMIT + CGC_BLOCK claims (see OVERFLOW)
      if (n >= ADJ_LIMIT) __hip_atomic_store(&t.dense, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (prev == ADJ_EMPTY || prev == k) {
      atomicAdd(&t.cnt[h], c);
      if (with_value) atomicMin(&t.mn[h], s);
      return;
    }
    h = (h + 1) & (ADJ_SLOTS - 1);
  }
}

// The contacts pixel (ly, lx) of the tile owns, in a fixed order: f(key, q) with q = the raster offset of the partner from the pixel.
template <typename F>
__device__ __forceinline__ void adj_contacts(const int* lab, int ly, int lx, int W, int conn8, F&& f) {
  const int* p = lab + ly * ADJ_COLS + lx + 1;
  const int v = p[0];
  if (v == 0) return;
  const int r = p[1], d = p[ADJ_COLS];
  if (r != 0 && r != v) f(v < r ? adj_key(v, r) : adj_key(r, v), 1);
  if (d != 0 && d != v) f(v < d ? adj_key(v, d) : adj_key(d, v), W);
  if (conn8) {
    const int dr = p[ADJ_COLS + 1], dl = p[ADJ_COLS - 1];
    if (dr != 0 && dr != v) f(v < dr ? adj_key(v, dr) : adj_key(dr, v), W + 1);
    if (dl != 0 && dl != v) f(v < dl ? adj_key(v, dl) : adj_key(dl, v), W - 1);
  }
}

// Count launch (WRITE = false): tile_off[tile] = records of the tile, dense[tile].  Write launch (WRITE = true): tile_off holds the
// exclusive scan; the tile's records go to [tile_off[tile], tile_off[tile + 1]).  A thread walks 16 consecutive rows of one column and
// keeps the last key in registers: along a vertical border the key repeats, and one table update stands for the run.
template <bool WRITE>
__global__ void __launch_bounds__(CGC_BLOCK) k_adj_tiles(const int* __restrict__ labels, const int* __restrict__ value, int H, int W,
                                                         int tiles_x, int conn8, int* __restrict__ tile_off, int* __restrict__ dense,
                                                         int64_t* __restrict__ keys, int* __restrict__ cnts, int* __restrict__ sums) {
  __shared__ int lab[ADJ_ROWS * ADJ_COLS];
  __shared__ AdjTable t;
  const int tile = blockIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * ADJ_TILE, x0 = tx * ADJ_TILE;
  const bool with_value = value != nullptr;
  // Every load of the thread is issued before the first one is waited for: the address is clamped into the image, so that the load
  // needs no branch, and what lies outside the image becomes background (no contact) afterwards.
  int staged[ADJ_LOADS];
#pragma unroll
  for (int k = 0; k < ADJ_LOADS; ++k) {
    const int i = threadIdx.x + k * CGC_BLOCK;
    const int ly = i / ADJ_COLS, lx = i - ly * ADJ_COLS;
    const int y = y0 + ly, x = x0 + lx - 1;
    const int yc = y < H ? y : H - 1, xc = x < 0 ? 0 : x < W ? x : W - 1;      // y0 < H and H, W >= 1: inside the image
    staged[k] = labels[(int64_t)yc * W + xc];
  }
#pragma unroll
  for (int k = 0; k < ADJ_LOADS; ++k) {
    const int i = threadIdx.x + k * CGC_BLOCK;
    const int ly = i / ADJ_COLS, lx = i - ly * ADJ_COLS;
    const int y = y0 + ly, x = x0 + lx - 1;
    if (i < ADJ_ROWS * ADJ_COLS) lab[i] = (y < H && x >= 0 && x < W) ? staged[k] : 0;
  }
  for (int i = threadIdx.x; i < ADJ_SLOTS; i += CGC_BLOCK) {
    t.key[i] = ADJ_EMPTY;
    t.cnt[i] = 0;
    t.mn[i] = INT32_MAX_;
  }
  if (threadIdx.x == 0) t.distinct = t.dense = t.contacts = t.wpos = 0;
  __syncthreads();

  const int lx = threadIdx.x & (ADJ_TILE - 1), band = threadIdx.x / ADJ_TILE;
  const int64_t pix0 = (int64_t)(y0 + band * ADJ_BAND) * W + x0 + lx;      // only dereferenced at contacts, which lie inside the image
  const int first = WRITE ? tile_off[tile] : 0;
  const int room = WRITE ? tile_off[tile + 1] - first : 0;
  const bool raw = WRITE && dense[tile] != 0;                              // uniform: the count launch found the tile dense

  if (!raw) {
    unsigned long long ck = ADJ_EMPTY;
    int cc = 0, cm = INT32_MAX_, mine = 0;
    for (int k = 0; k < ADJ_BAND; ++k) {
      const int64_t pix = pix0 + (int64_t)k * W;
      adj_contacts(lab, band * ADJ_BAND + k, lx, W, conn8, [&](int64_t key, int q) {
        const int s = with_value ? clamp_sum(value[pix], value[pix + q]) : 0;
        ++mine;
        if ((unsigned long long)key == ck) {
          ++cc;
          cm = s < cm ? s : cm;
        } else {
          if (cc) adj_insert(t, ck, cc, cm, with_value);
          ck = (unsigned long long)key;
          cc = 1;
          cm = s;
        }
      });
    }
    if (cc) adj_insert(t, ck, cc, cm, with_value);
    if (!WRITE && mine) atomicAdd(&t.contacts, mine);
    __syncthreads();
    if (!WRITE) {
      if (threadIdx.x == 0) {
        dense[tile] = t.dense;
        tile_off[tile] = t.dense ? t.contacts : t.distinct;
      }
      return;
    }
    const int found = t.distinct < room ? t.distinct : room;               // equal (see OVERFLOW): never write past the tile's share
    for (int pos = threadIdx.x; pos < found; pos += CGC_BLOCK) {
      const int i = t.claimed[pos];
      keys[first + pos] = (int64_t)t.key[i];
      cnts[first + pos] = t.cnt[i];
      if (with_value) sums[first + pos] = t.mn[i];
    }
    return;
  }
  if (WRITE) {
    for (int k = 0; k < ADJ_BAND; ++k) {
      const int64_t pix = pix0 + (int64_t)k * W;
      adj_contacts(lab, band * ADJ_BAND + k, lx, W, conn8, [&](int64_t key, int q) {
        const int pos = atomicAdd(&t.wpos, 1);
        if (pos >= room) return;
        keys[first + pos] = key;
        cnts[first + pos] = 1;
        if (with_value) sums[first + pos] = clamp_sum(value[pix], value[pix + q]);
      });
    }
  }
}

// inclusive scan of one int per thread over the 256 threads of the workgroup
__device__ __forceinline__ int adj_block_scan_incl(int v, int* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 1; s < CGC_BLOCK; s <<= 1) {
    const int add = (int)threadIdx.x >= s ? sh[threadIdx.x - s] : 0;
    __syncthreads();
    v += add;
    sh[threadIdx.x] = v;
    __syncthreads();
  }
  return v;
}

// ONE workgroup: a[0 .. n) -> its exclusive scan in place, the total to a[n] (when `tail`) and to *total.  No total reaches 2^31: a
// call has fewer than 4 H W < 2^31 contacts.
__global__ void __launch_bounds__(CGC_BLOCK) k_adj_scan(int* a, int64_t n, int tail, int* __restrict__ total) {
  __shared__ int sh[CGC_BLOCK];
  const int64_t per = (n + CGC_BLOCK - 1) / CGC_BLOCK;
  const int64_t lo = per * threadIdx.x < n ? per * threadIdx.x : n, hi = lo + per < n ? lo + per : n;
  int s = 0;
  for (int64_t i = lo; i < hi; ++i) s += a[i];
  const int incl = adj_block_scan_incl(s, sh);
  int run = incl - s;
  for (int64_t i = lo; i < hi; ++i) {
    const int c = a[i];
    a[i] = run;
    run += c;
  }
  if (threadIdx.x == CGC_BLOCK - 1) {
    if (tail) a[n] = incl;
    *total = incl;
  }
}

__device__ __forceinline__ bool adj_is_head(const int64_t* __restrict__ sorted, int64_t i) { return i == 0 || sorted[i] != sorted[i - 1]; }

__global__ void __launch_bounds__(CGC_BLOCK) k_adj_heads(const int64_t* __restrict__ sorted, int64_t n, int* __restrict__ blocks) {
  __shared__ int wsum[CGC_BLOCK / 64];
  const int64_t base = (int64_t)blockIdx.x * ADJ_SCAN;
  int c = 0;
  for (int k = 0; k < ADJ_PER_THREAD; ++k) {
    const int64_t i = base + k * CGC_BLOCK + threadIdx.x;
    if (i < n && adj_is_head(sorted, i)) ++c;
  }
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blocks[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(CGC_BLOCK) k_adj_init(int n_pairs, int* __restrict__ count, int* __restrict__ min_sum) {
  const int i = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= n_pairs) return;
  count[i] = 0;
  if (min_sum != nullptr) min_sum[i] = INT32_MAX_;
}

// Thread t of a block owns the sorted records base + 8 t .. + 7.  The row of a record is the number of heads up to and including it,
// minus one; a thread folds the records of one row in registers and sends one atomic add / min per row it touches.
__global__ void __launch_bounds__(CGC_BLOCK) k_adj_merge(const int64_t* __restrict__ sorted, const int64_t* __restrict__ perm,
                                                         const int* __restrict__ cnts, const int* __restrict__ sums, int64_t n,
                                                         const int* __restrict__ blocks, int n_pairs, int* __restrict__ pairs,
                                                         int* count, int* min_sum) {
  __shared__ int sh[CGC_BLOCK];
  const int64_t base = (int64_t)blockIdx.x * ADJ_SCAN + (int64_t)threadIdx.x * ADJ_PER_THREAD;
  unsigned heads = 0;
  for (int k = 0; k < ADJ_PER_THREAD; ++k)
    if (base + k < n && adj_is_head(sorted, base + k)) heads |= 1u << k;
  const int c = __builtin_popcount(heads);
  int row = blocks[blockIdx.x] + adj_block_scan_incl(c, sh) - c - 1;      // the row of the run that reaches into this thread's records
  int acc = 0, mn = INT32_MAX_;
  bool any = false;
  for (int k = 0; k < ADJ_PER_THREAD; ++k) {
    const int64_t i = base + k;
    if (i >= n) break;
    if (heads >> k & 1) {
      if (any && row >= 0 && row < n_pairs) {
        atomicAdd(count + row, acc);
        if (min_sum != nullptr) atomicMin(min_sum + row, mn);
      }
      ++row;
      acc = 0;
      mn = INT32_MAX_;
      if (row < n_pairs) {
        const int64_t key = sorted[i];
        pairs[2 * (int64_t)row] = (int)(key >> 32);
        pairs[2 * (int64_t)row + 1] = (int)((uint32_t)key ^ 0x80000000u);
      }
    }
    const int64_t src = perm[i];
    if (src < 0 || src >= n) continue;                                    // a permutation of 0 .. n - 1: never taken
    acc += cnts[src];
    if (sums != nullptr) {
      const int s = sums[src];
      mn = s < mn ? s : mn;
    }
    any = true;
  }
  if (any && row >= 0 && row < n_pairs) {
    atomicAdd(count + row, acc);
    if (min_sum != nullptr) atomicMin(min_sum + row, mn);
  }
}

static inline bool bad_adjacency_dims(int H, int W) { return H < 0 || W < 0 || (int64_t)H * W >= ((int64_t)1 << 29); }      // 4 H W fits int32

}  // namespace

extern "C" int cgc_adjacency_tile_side(void) { return ADJ_TILE; }

extern "C" int64_t cgc_adjacency_ws_bytes(int H, int W) {
  if (bad_adjacency_dims(H, W)) return 0;
  return layout_bytes(adj_layout, adj_tiles(H, W));
}

extern "C" int cgc_adjacency_count(const int* labels, int H, int W, int connectivity, void* ws, int* n_records_out, cgc_stream_t stream) {
  if (bad_adjacency_dims(H, W) || bad_connectivity(connectivity) || n_records_out == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  if ((int64_t)H * W == 0) {
    const hipError_t e = hipMemsetAsync(n_records_out, 0, 4, st);
    return e == hipSuccess ? 0 : (int)e;
  }
  if (labels == nullptr || ws == nullptr) return CGC_EINVAL;
  const int64_t tiles = adj_tiles(H, W);
  const AdjWs w = adj_layout(Carver(ws), tiles);
  hipLaunchKernelGGL(k_adj_tiles<false>, dim3((unsigned)tiles), dim3(CGC_BLOCK), 0, st, labels, (const int*)nullptr, H, W,
                     ceil_div(W, ADJ_TILE), connectivity == 2, w.tile_off, w.dense, (int64_t*)nullptr, (int*)nullptr, (int*)nullptr);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_adj_scan, dim3(1), dim3(CGC_BLOCK), 0, st, w.tile_off, tiles, 1, n_records_out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_adjacency_records(const int* labels, const int* value_or_null, int H, int W, int connectivity, void* ws,
                                     int64_t n_records, int64_t* keys, int* counts, int* sums_or_null, cgc_stream_t stream) {
  if (bad_adjacency_dims(H, W) || bad_connectivity(connectivity) || n_records < 0 || n_records > 4 * (int64_t)H * W) return CGC_EINVAL;
  if (n_records == 0) return 0;
  if (labels == nullptr || ws == nullptr || keys == nullptr || counts == nullptr) return CGC_EINVAL;
  if ((value_or_null == nullptr) != (sums_or_null == nullptr)) return CGC_EINVAL;
  const int64_t tiles = adj_tiles(H, W);
  const AdjWs w = adj_layout(Carver(ws), tiles);
  hipLaunchKernelGGL(k_adj_tiles<true>, dim3((unsigned)tiles), dim3(CGC_BLOCK), 0, as_stream(stream), labels, value_or_null, H, W,
                     ceil_div(W, ADJ_TILE), connectivity == 2, w.tile_off, w.dense, keys, counts, sums_or_null);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int64_t cgc_adjacency_merge_ws_bytes(int64_t n_records) {
  if (n_records < 0 || n_records >= ((int64_t)1 << 31)) return 0;
  return layout_bytes(merge_layout, n_records);
}

extern "C" int cgc_adjacency_heads(const int64_t* sorted_keys, int64_t n_records, void* ws, int* n_pairs_out, cgc_stream_t stream) {
  if (n_records < 0 || n_records >= ((int64_t)1 << 31) || n_pairs_out == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  if (n_records == 0) {
    const hipError_t e = hipMemsetAsync(n_pairs_out, 0, 4, st);
    return e == hipSuccess ? 0 : (int)e;
  }
  if (sorted_keys == nullptr || ws == nullptr) return CGC_EINVAL;
  const MergeWs w = merge_layout(Carver(ws), n_records);
  const int64_t nb = merge_blocks(n_records);
  hipLaunchKernelGGL(k_adj_heads, dim3((unsigned)nb), dim3(CGC_BLOCK), 0, st, sorted_keys, n_records, w.blocks);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_adj_scan, dim3(1), dim3(CGC_BLOCK), 0, st, w.blocks, nb, 0, n_pairs_out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_adjacency_merge(const int64_t* sorted_keys, const int64_t* perm, const int* counts, const int* sums_or_null,
                                   int64_t n_records, const void* ws, int n_pairs, int* pairs, int* count, int* min_sum_or_null,
                                   cgc_stream_t stream) {
  if (n_records < 0 || n_records >= ((int64_t)1 << 31) || n_pairs < 0 || (int64_t)n_pairs > n_records) return CGC_EINVAL;
  if ((sums_or_null == nullptr) != (min_sum_or_null == nullptr)) return CGC_EINVAL;
  if (n_pairs == 0) return 0;
  if (sorted_keys == nullptr || perm == nullptr || counts == nullptr || ws == nullptr || pairs == nullptr || count == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const MergeWs w = merge_layout(Carver(const_cast<void*>(ws)), n_records);
  hipLaunchKernelGGL(k_adj_init, dim3(ceil_div(n_pairs, CGC_BLOCK)), dim3(CGC_BLOCK), 0, st, n_pairs, count, min_sum_or_null);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_adj_merge, dim3((unsigned)merge_blocks(n_records)), dim3(CGC_BLOCK), 0, st, sorted_keys, perm, counts, sums_or_null,
                     n_records, w.blocks, n_pairs, pairs, count, min_sum_or_null);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
