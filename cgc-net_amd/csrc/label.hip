// Connected-component labelling of a 2-D image on gfx950: binary masks (scipy.ndimage.label, bit for bit) and integer masks (every
// value split into its connected pieces).  Contract item by item: cgc-net_amd/kernels.py KernelSpec.label_components; layout,
// launches and measurements: DESIGN.md, "Instance labelling".
//
// One union-find over the pixels, parent[p] <= p always, so the root of a component is its smallest raster index = its first pixel in
// raster order, and the numbering 1..n is an exclusive scan over root flags.  Launches of one call:
//   k_label_tile    one 64 x 64 tile per workgroup: values and the tile's union-find in LDS, all links inside the tile resolved there;
//                   parent[p] = raster index of p's tile-local root (-1 for background)
//   k_label_merge   the pixel pairs that cross a tile edge (the diagonal ones across tile corners with connectivity 2): lock-free union
//                   with agent-scope atomics only (see `VISIBILITY` below)
//   k_label_flatten root[p] = find(p), written into the labels buffer; per-root pixel counts when min_size > 1 or sizes are wanted
//   k_label_count   surviving-root flags counted per block of 2048 consecutive raster indices
//   k_label_scan    ONE workgroup: exclusive scan of the block counts, n to device memory
//   k_label_number  number[root] = 1 + its rank in raster order (0 for a removed one), into the parent array
//   k_label_apply   labels[p] = number[root[p]]
// and, after the host has read n, k_label_sizes gathers sizes[number - 1] = count.  No workgroup ever waits for another one: the
// retries of the union are bounded because parents only decrease, and the scan is launches, not a look-back chain.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

constexpr int LBL_TILE = 64;                      // tile edge: 4096 pixels, 16 per thread
constexpr int LBL_TILE_PX = LBL_TILE * LBL_TILE;
constexpr int LBL_SCAN_PX = 2048;                 // consecutive raster indices per numbering block, 8 per thread
constexpr int LBL_PER_THREAD = LBL_SCAN_PX / CGC_BLOCK;

struct LabelWs {
  int* parent;     // [H*W] union-find parents, then the numbers of the roots
  int* blocks;     // [nblocks] root counts per numbering block, then their exclusive scan
  int* count;      // [H*W] pixels per root (only with counts)
};
static inline int64_t label_blocks(int64_t npix) { return ceil_div64(npix, LBL_SCAN_PX); }
static inline LabelWs label_layout(Carver&& c, int64_t npix, bool counts) {     // the one definition of the workspace
  LabelWs w;
  w.parent = c.take<int>(npix);
  w.blocks = c.take<int>(label_blocks(npix));
  w.count = counts ? c.take<int>(npix) : nullptr;
  return w;
}

// ---- union-find in LDS (tile pass).  Other lanes update the array while this one walks it: every access is an atomic.
__device__ __forceinline__ int lds_find(int* par, int x) {
  int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  return x;
}
__device__ __forceinline__ void lds_unite(int* par, int a, int b) {
  for (;;) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == b) return;    // b was still a root: linked
    b = old;                 // somebody linked b first (to `old` < b): a must now join old's set as well
  }
}

// (a) tile pass.  The pairs each pixel is responsible for are its "backward" neighbours: left, up and (connectivity 2) up-left,
// up-right.  Pairs that already follow from two others are skipped: `up` when left, up-left and up all carry the value; a diagonal
// when `up` carries it (the diagonal pixel is then a 4-neighbour of `up`), up-left also when `left` does.
template <typename T>
__global__ void __launch_bounds__(CGC_BLOCK) k_label_tile(const T* __restrict__ img, int H, int W, int tiles_x, int conn8,
                                                          int* __restrict__ parent) {
  __shared__ T val[LBL_TILE_PX];
  __shared__ int par[LBL_TILE_PX];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * LBL_TILE, x0 = tx * LBL_TILE;
  for (int i = threadIdx.x; i < LBL_TILE_PX; i += CGC_BLOCK) {
    const int ly = i >> 6, lx = i & 63;
    const int y = y0 + ly, x = x0 + lx;
    const T v = (y < H && x < W) ? img[(int64_t)y * W + x] : T(0);
    val[i] = v;
    par[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LBL_TILE_PX; i += CGC_BLOCK) {
    const T v = val[i];
    if (v == T(0)) continue;
    const int ly = i >> 6, lx = i & 63;
    const bool l = lx > 0 && val[i - 1] == v;
    const bool u = ly > 0 && val[i - LBL_TILE] == v;
    const bool ul = lx > 0 && ly > 0 && val[i - LBL_TILE - 1] == v;
    if (l) lds_unite(par, i, i - 1);
    if (u && !(l && ul)) lds_unite(par, i, i - LBL_TILE);
    if (conn8 && !u) {
      if (ul && !l) lds_unite(par, i, i - LBL_TILE - 1);
      if (lx < LBL_TILE - 1 && ly > 0 && val[i - LBL_TILE + 1] == v) lds_unite(par, i, i - LBL_TILE + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LBL_TILE_PX; i += CGC_BLOCK) {
    const int ly = i >> 6, lx = i & 63;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    int out = -1;
    if (val[i] != T(0)) {
      const int r = lds_find(par, i);
      out = (y0 + (r >> 6)) * W + x0 + (r & 63);
    }
    parent[(int64_t)y * W + x] = out;
  }
}

// ---- VISIBILITY.  In k_label_merge other workgroups, on other XCDs, rewrite parents while this one walks them.  A CU's L1 is never
// refreshed by another CU's stores and the per-XCD L2s are not coherent with each other, so a plain load could keep returning a parent
// that was replaced long ago -- and two tiles' pieces of one component would silently stay apart.  Every read of `parent` in that
// kernel is a relaxed agent-scope atomic load and every update an agent-scope atomic min.  The kernels before and after it are
// separate launches and use plain accesses.
__device__ __forceinline__ int g_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(int* parent, int x) {
  int p = g_load(parent + x);
  while (p != x) {
    x = p;
    p = g_load(parent + x);
  }
  return x;
}
__device__ void g_unite(int* parent, int a, int b) {
  const int a0 = a, b0 = b;
  for (;;) {
    a = g_find(parent, a);
    b = g_find(parent, b);
    if (a == b) break;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(parent + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == b) break;
    b = old;
  }
  // shorten the two walked chains: the root found is an ancestor of both starts, and a min can only move a parent towards it
  const int r = a < b ? a : b;
  if (r < a0) __hip_atomic_fetch_min(parent + a0, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r < b0) __hip_atomic_fetch_min(parent + b0, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (b) border merge.  Items [0, nh * W): pixel (x, 64 (k + 1)) of horizontal edge k against the row above it (up; with connectivity 2
// up-left and up-right unless `up` links them already).  Items after those: row y of vertical edge k, the pixels (64 (k + 1) - 1, y)
// and (64 (k + 1), y); with connectivity 2 and y not on a horizontal edge also the two diagonals between rows y - 1 and y (on a
// horizontal edge the first group has them: that is where a corner pair touches four tiles).
template <typename T>
__global__ void __launch_bounds__(CGC_BLOCK) k_label_merge(const T* __restrict__ img, int H, int W, int nh, int nv, int conn8,
                                                           int* parent) {
  const int64_t n_h = (int64_t)nh * W, total = n_h + (int64_t)nv * H;
  for (int64_t it = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x; it < total; it += (int64_t)gridDim.x * CGC_BLOCK) {
    if (it < n_h) {
      const int k = (int)(it / W), x = (int)(it - (int64_t)k * W);
      const int p = (k + 1) * LBL_TILE * W + x, q = p - W;
      const T v = img[p];
      if (v == T(0)) continue;
      if (img[q] == v) {
        g_unite(parent, p, q);
      } else if (conn8) {
        if (x > 0 && img[q - 1] == v) g_unite(parent, p, q - 1);
        if (x + 1 < W && img[q + 1] == v) g_unite(parent, p, q + 1);
      }
    } else {
      const int64_t j = it - n_h;
      const int k = (int)(j / H), y = (int)(j - (int64_t)k * H);
      const int p = y * W + (k + 1) * LBL_TILE;      // (x, y); p - 1 = (x - 1, y)
      const T a = img[p], b = img[p - 1];
      const bool ab = a != T(0) && a == b;
      if (ab) g_unite(parent, p, p - 1);
      if (conn8 && (y & (LBL_TILE - 1)) != 0) {
        const T c = img[p - W], d = img[p - W - 1];    // (x, y - 1), (x - 1, y - 1)
        if (a != T(0) && a == d && !ab && a != c) g_unite(parent, p, p - W - 1);
        if (b != T(0) && b == c && !ab && b != d) g_unite(parent, p - 1, p - W);
      }
    }
  }
}

// (c) flatten, out of place: root[p] = find(p) (-1 for background).  Counts: the lanes of a wave hold 64 consecutive pixels, which share
// few roots -- one atomic per distinct root of the wave.
__global__ void __launch_bounds__(CGC_BLOCK) k_label_flatten(const int* __restrict__ parent, int64_t npix, int* __restrict__ root,
                                                             int* count) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  int r = -1;
  if (i < npix) {
    r = parent[i];
    if (r >= 0) {
      int p = parent[r];
      while (p != r) {
        r = p;
        p = parent[r];
      }
    }
    root[i] = r;
  }
  if (count == nullptr) return;
  bool todo = r >= 0;
  while (todo) {      // lanes that are done have left the loop: the first active lane names the root of this round
    const int lead = __builtin_amdgcn_readfirstlane(r);
    const bool mine = r == lead;
    const unsigned long long m = __ballot(mine);
    if (mine) {
      if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(count + lead, __builtin_popcountll(m));
      todo = false;
    }
  }
}

__device__ __forceinline__ bool is_kept_root(const int* __restrict__ root, const int* __restrict__ count, int min_size, int64_t i) {
  return root[i] == (int)i && (count == nullptr || count[i] >= min_size);
}

// (d1) surviving roots per numbering block
__global__ void __launch_bounds__(CGC_BLOCK) k_label_count(const int* __restrict__ root, const int* __restrict__ count, int min_size,
                                                           int64_t npix, int* __restrict__ blocks) {
  __shared__ int wsum[CGC_BLOCK / 64];
  const int64_t base = (int64_t)blockIdx.x * LBL_SCAN_PX;
  int c = 0;
  for (int k = 0; k < LBL_PER_THREAD; ++k) {
    const int64_t i = base + k * CGC_BLOCK + threadIdx.x;
    if (i < npix && is_kept_root(root, count, min_size, i)) ++c;
  }
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blocks[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// inclusive scan of one int per thread over the 256 threads of the workgroup
__device__ __forceinline__ int block_scan_incl(int v, int* sh) {
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

// (d2) ONE workgroup: blocks[] -> its exclusive scan in place, the total to *n_out.  Each thread owns a run of consecutive entries.
__global__ void __launch_bounds__(CGC_BLOCK) k_label_scan(int* blocks, int64_t nblocks, int* __restrict__ n_out) {
  __shared__ int sh[CGC_BLOCK];
  const int64_t per = (nblocks + CGC_BLOCK - 1) / CGC_BLOCK;
  const int64_t lo = per * threadIdx.x, hi = lo + per < nblocks ? lo + per : nblocks;
  int s = 0;
  for (int64_t i = lo; i < hi; ++i) s += blocks[i];
  const int incl = block_scan_incl(s, sh);
  int run = incl - s;
  for (int64_t i = lo; i < hi; ++i) {
    const int c = blocks[i];
    blocks[i] = run;
    run += c;
  }
  if (threadIdx.x == CGC_BLOCK - 1) *n_out = incl;
}

// (d3) number[p] for the roots of a block: thread t owns the 8 consecutive indices base + 8 t .. + 7, so ranks follow raster order.
// Roots get their number (0 when removed); with `all` every other index gets 0 too, which is what k_label_sizes reads.
__global__ void __launch_bounds__(CGC_BLOCK) k_label_number(const int* __restrict__ root, const int* __restrict__ count, int min_size,
                                                            int64_t npix, const int* __restrict__ blocks, int all,
                                                            int* __restrict__ number) {
  __shared__ int sh[CGC_BLOCK];
  const int64_t base = (int64_t)blockIdx.x * LBL_SCAN_PX + (int64_t)threadIdx.x * LBL_PER_THREAD;
  unsigned isroot = 0, kept = 0;
  for (int k = 0; k < LBL_PER_THREAD; ++k) {
    const int64_t i = base + k;
    if (i < npix && root[i] == (int)i) {
      isroot |= 1u << k;
      if (count == nullptr || count[i] >= min_size) kept |= 1u << k;
    }
  }
  const int c = __builtin_popcount(kept);
  int next = blocks[blockIdx.x] + block_scan_incl(c, sh) - c + 1;
  for (int k = 0; k < LBL_PER_THREAD; ++k) {
    const int64_t i = base + k;
    if (i >= npix) break;
    if (kept >> k & 1) number[i] = next++;
    else if (all || (isroot >> k & 1)) number[i] = 0;
  }
}

// (e) relabel in place: labels holds root[], number[] sits in the parent array
__global__ void __launch_bounds__(CGC_BLOCK) k_label_apply(const int* __restrict__ number, int64_t npix, int* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= npix) return;
  const int r = labels[i];
  labels[i] = r >= 0 ? number[r] : 0;
}

__global__ void __launch_bounds__(CGC_BLOCK) k_label_sizes(const int* __restrict__ number, const int* __restrict__ count, int64_t npix,
                                                           int n, int* __restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= npix) return;
  const int k = number[i];
  if (k > 0 && k <= n) sizes[k - 1] = count[i];
}

template <typename T>
int label_run(const void* image, int H, int W, int conn8, int min_size, bool counts, bool all, const LabelWs& w, int* labels, int* n_out,
              hipStream_t st) {
  const T* img = static_cast<const T*>(image);
  const int64_t npix = (int64_t)H * W;
  const int tiles_x = ceil_div(W, LBL_TILE), tiles_y = ceil_div(H, LBL_TILE);
  hipLaunchKernelGGL(k_label_tile<T>, dim3(tiles_x * tiles_y), dim3(CGC_BLOCK), 0, st, img, H, W, tiles_x, conn8, w.parent);
  CGC_RETURN_IF_LAUNCH_FAILED();
  const int nh = (H - 1) / LBL_TILE, nv = (W - 1) / LBL_TILE;
  const int64_t items = (int64_t)nh * W + (int64_t)nv * H;
  if (items > 0) {
    const int64_t mb = ceil_div64(items, CGC_BLOCK);
    hipLaunchKernelGGL(k_label_merge<T>, dim3((int)(mb < 65536 ? mb : 65536)), dim3(CGC_BLOCK), 0, st, img, H, W, nh, nv, conn8, w.parent);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  int* count = w.count;                          // null without counts
  if (counts) {
    const hipError_t e = hipMemsetAsync(w.count, 0, (size_t)npix * 4, st);
    if (e != hipSuccess) return (int)e;
  }
  const int pb = (int)ceil_div64(npix, CGC_BLOCK), nb = (int)label_blocks(npix);
  hipLaunchKernelGGL(k_label_flatten, dim3(pb), dim3(CGC_BLOCK), 0, st, w.parent, npix, labels, count);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_label_count, dim3(nb), dim3(CGC_BLOCK), 0, st, labels, count, min_size, npix, w.blocks);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_label_scan, dim3(1), dim3(CGC_BLOCK), 0, st, w.blocks, (int64_t)nb, n_out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_label_number, dim3(nb), dim3(CGC_BLOCK), 0, st, labels, count, min_size, npix, w.blocks, all ? 1 : 0, w.parent);
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_label_apply, dim3(pb), dim3(CGC_BLOCK), 0, st, w.parent, npix, labels);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // namespace

extern "C" int64_t cgc_label_ws_bytes(int H, int W, int with_counts) {
  if (bad_image_dims(H, W)) return 0;
  return layout_bytes(label_layout, (int64_t)H * W, with_counts != 0);
}

extern "C" int cgc_label_components(const void* image, int pixel_bytes, int H, int W, int connectivity, int min_size, int with_counts,
                                    void* ws, int* labels, int* n_out, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || (connectivity != 1 && connectivity != 2) || min_size < 0 || n_out == nullptr) return CGC_EINVAL;
  if (bad_elem_bytes(pixel_bytes)) return CGC_EINVAL;
  if (min_size > 1 && !with_counts) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int64_t npix = (int64_t)H * W;
  if (npix == 0) {
    const hipError_t e = hipMemsetAsync(n_out, 0, 4, st);
    return e == hipSuccess ? 0 : (int)e;
  }
  if (image == nullptr || ws == nullptr || labels == nullptr) return CGC_EINVAL;
  const bool counts = with_counts != 0, all = with_counts != 0;
  const LabelWs w = label_layout(Carver(ws), npix, counts);
  const int conn8 = connectivity == 2;
  switch (pixel_bytes) {
    case 1: return label_run<uint8_t>(image, H, W, conn8, min_size, counts, all, w, labels, n_out, st);
    case 2: return label_run<uint16_t>(image, H, W, conn8, min_size, counts, all, w, labels, n_out, st);
    case 4: return label_run<uint32_t>(image, H, W, conn8, min_size, counts, all, w, labels, n_out, st);
    default: return label_run<uint64_t>(image, H, W, conn8, min_size, counts, all, w, labels, n_out, st);
  }
}

extern "C" int cgc_label_sizes(const void* ws, int H, int W, int n, int* sizes, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || n < 0 || (int64_t)n > (int64_t)H * W) return CGC_EINVAL;
  if (n == 0) return 0;
  if (ws == nullptr || sizes == nullptr) return CGC_EINVAL;
  const int64_t npix = (int64_t)H * W;
  const LabelWs w = label_layout(Carver(const_cast<void*>(ws)), npix, true);      // sizes come from a call that counted
  hipLaunchKernelGGL(k_label_sizes, dim3((int)ceil_div64(npix, CGC_BLOCK)), dim3(CGC_BLOCK), 0, as_stream(stream), w.parent, w.count, npix, n,
                     sizes);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
