// Ordered boundary polygons of the regions of a label image on gfx950: KernelSpec.region_outlines; DESIGN.md, "Region outlines".
//
// A pixel (y, x) is the square [x, x + 1] x [y, y + 1].  Its VALUE is its label where it is counted (labels[p] in [0, max_label] and
// `within` null or non-zero at p) and -1 where not, also outside the image; a pixel with a label outside [0, max_label] is refused
// (one more in *meta).  Side s of a pixel of value v that gets outlines (v >= 1, or v >= 0 with `background`) is a CRACK of v when the
// pixel across it has another value.  Sides: 0 top, 1 right, 2 bottom, 3 left; a crack runs with its pixel on the right (east, south,
// west, north); its id is 4 (y W + x) + s.
//
// NO LOOP IS WALKED.  Following one contour is sequential and one region may own 10^5 cracks, so the order along a loop comes from
// pointer doubling over all cracks at once, in rounds = ceil(log2(n_cracks)) launches per phase:
//   k_outline_count    a thread per pixel: the 4-bit mask of its cracks and their number (the caller's prefix sum makes the offsets).
//   k_outline_cracks   a thread per pixel: writes its cracks into the compact list (id order = pixel order, then side) and, from the
//                      2 x 2 block at each crack's head, the compact index of its successor.  The successors are a permutation.
//   k_outline_min_*    phase 1: (smallest compact index seen, pointer) per crack, doubled; ends with the loop's start in every crack.
//   k_outline_rank_*   phase 2: the cycle is cut in front of its start; (steps to the loop's end, pointer) per crack, doubled.  The
//                      position of crack k in its loop is steps[start] - steps[k], the loop's length steps[start] + 1.
//   k_outline_keys     a 64-bit key (label << 32 | compact index) per loop start, packed by the caller's prefix sum over the starts;
//                      the caller sorts them: loops ordered by (label, start id).
//   k_outline_tables   a thread per sorted loop: label, start id, cracks; and the loop's number, written at its start crack.
//   k_outline_scatter  a thread per crack: its tail to slot crack_ptr[loop] + position; its shoelace term to the loop's area2 (int64
//                      atomics; a wave whose cracks share a loop adds once); for 'corners' the flag "the vertex at my head is kept".
//   k_outline_compact  'corners': a thread per slot, the kept vertices to their places (the caller's prefix sum over the flags).
// Two buffers of n_cracks 64-bit pairs (the workspace) are read and written alternately, so no round reads what it writes.
// Integer work only; the one place where order of arrival exists, the int64 additions to area2, is independent of it.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int OUTLINE_MAX_SIDE = 32767;                          // as region_geometry
constexpr int64_t OUTLINE_MAX_PIXELS = (int64_t)1 << 29;         // 4 H W < 2^31: a crack id and a crack count fit int32

struct OutlineImage {
  const int* labels;
  const void* within;                    // null: every pixel
  int wbytes, H, W, max_label, lowest;   // lowest: the smallest value that gets outlines (0 with `background`, else 1)
};

// The value of position (y, x): its label where it is counted, -1 where not (outside the image, refused, or `within` is zero there).
__device__ __forceinline__ int outline_value(const OutlineImage& im, int y, int x) {
  if ((unsigned)y >= (unsigned)im.H || (unsigned)x >= (unsigned)im.W) return -1;
  const int64_t i = (int64_t)y * im.W + x;
  const int L = im.labels[i];
  if ((unsigned)L > (unsigned)im.max_label) return -1;
  if (im.within != nullptr && !image_nonzero(im.within, im.wbytes, i)) return -1;
  return L;
}

__device__ __forceinline__ int outline_dy(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }      // the direction of a crack of side s
__device__ __forceinline__ int outline_dx(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
__device__ __forceinline__ int outline_below(unsigned mask, int s) { return __builtin_popcount(mask & ((1u << s) - 1u)); }

__global__ void __launch_bounds__(CGC_BLOCK) k_outline_count(OutlineImage im, int npix, uint8_t* __restrict__ mask, uint8_t* __restrict__ cnt,
                                                             int* meta) {
  const int i = blockIdx.x * CGC_BLOCK + threadIdx.x;              // npix < 2^29
  const bool in = i < npix;
  unsigned m = 0;
  bool bad = false;
  if (in) {
    const int y = i / im.W, x = i - y * im.W;
    bad = (unsigned)im.labels[i] > (unsigned)im.max_label;
    const int v = outline_value(im, y, x);
    if (v >= im.lowest) {
      m = (unsigned)(outline_value(im, y - 1, x) != v) | (unsigned)(outline_value(im, y, x + 1) != v) << 1 |
          (unsigned)(outline_value(im, y + 1, x) != v) << 2 | (unsigned)(outline_value(im, y, x - 1) != v) << 3;
    }
    mask[i] = (uint8_t)m;
    cnt[i] = (uint8_t)__builtin_popcount(m);
  }
  const int refused = (int)__popcll(__ballot(bad));
  if (refused != 0 && (threadIdx.x & (CGC_WAVE - 1)) == 0) atomicAdd(meta, refused);
}

// off: the INCLUSIVE prefix sum of the counts, so the first crack of pixel j has compact index off[j] - popcount(mask[j]).
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_cracks(OutlineImage im, int npix, int connectivity, const uint8_t* __restrict__ mask,
                                                              const int* __restrict__ off, int n, int* __restrict__ crack,
                                                              int* __restrict__ succ) {
  const int i = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (i >= npix) return;
  const unsigned m = mask[i];
  if (m == 0) return;
  const int y = i / im.W, x = i - y * im.W;
  const int v = im.labels[i];                                      // counted: its mask is not empty
  const int base = off[i] - __builtin_popcount(m);
  for (int s = 0; s < 4; ++s) {
    if ((m >> s & 1u) == 0) continue;
    const int k = base + outline_below(m, s);
    if ((unsigned)k >= (unsigned)n) continue;                      // an `off` that does not belong to `mask` writes nothing outside
    const int ay = y + outline_dy(s), ax = x + outline_dx(s);     // A: ahead on the region's side
    const int by = ay + outline_dy((s + 3) & 3), bx = ax + outline_dx((s + 3) & 3);      // B: ahead on the other side
    const bool a = outline_value(im, ay, ax) == v, b = outline_value(im, by, bx) == v;
    int py, px, ps;                                                // the successor: side ps of pixel (py, px), which has value v
    if (connectivity == 1 ? !a : (!b && !a)) py = y, px = x, ps = (s + 1) & 3;           // right turn
    else if (!b) py = ay, px = ax, ps = s;                                                // straight
    else py = by, px = bx, ps = (s + 3) & 3;                                              // left turn
    const int j = py * im.W + px;
    const unsigned mj = mask[j];
    int t = off[j] - __builtin_popcount(mj) + outline_below(mj, ps);
    if ((unsigned)t >= (unsigned)n) t = k;
    crack[k] = 4 * i + s;
    succ[k] = t;
  }
}

__device__ __forceinline__ u64 outline_pair(int a, int b) { return (u64)(uint32_t)a << 32 | (uint32_t)b; }
__device__ __forceinline__ int outline_hi(u64 p) { return (int)(uint32_t)(p >> 32); }
__device__ __forceinline__ int outline_lo(u64 p) { return (int)(uint32_t)p; }

// Phase 1.  A pair is (the smallest compact index among the cracks from k up to the pointer, the pointer).
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_min_init(int n, const int* __restrict__ succ, u64* __restrict__ out) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= n) return;
  const int j = succ[k];
  out[k] = outline_pair(k, (unsigned)j < (unsigned)n ? j : k);
}
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_min_round(int n, const u64* __restrict__ in, u64* __restrict__ out) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= n) return;
  const u64 a = in[k], b = in[outline_lo(a)];
  out[k] = outline_pair(min(outline_hi(a), outline_hi(b)), outline_lo(b));
}
// ... its end: start[k]; and the first pair of phase 2, (steps to the loop's end so far, pointer or -1 at the end).
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_rank_init(int n, const u64* __restrict__ in, const int* __restrict__ succ,
                                                                 int* __restrict__ start, u64* __restrict__ out) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= n) return;
  const int s = outline_hi(in[k]);
  const int j = succ[k];
  const bool last = j == s || (unsigned)j >= (unsigned)n;
  start[k] = s;
  out[k] = outline_pair(last ? 0 : 1, last ? -1 : j);
}
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_rank_round(int n, const u64* __restrict__ in, u64* __restrict__ out) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= n) return;
  u64 a = in[k];
  const int j = outline_lo(a);
  if (j >= 0) {
    const u64 b = in[j];
    a = outline_pair(outline_hi(a) + outline_hi(b), outline_lo(b));
  }
  out[k] = a;
}
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_rank_end(int n, const u64* __restrict__ in, int* __restrict__ steps) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k < n) steps[k] = outline_hi(in[k]);
}

// rank: the INCLUSIVE prefix sum of "start[k] == k".
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_keys(int n, int n_loops, const int* __restrict__ labels, const int* __restrict__ crack,
                                                            const int* __restrict__ start, const int* __restrict__ rank,
                                                            long long* __restrict__ keys) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (k >= n || start[k] != k) return;
  const int r = rank[k] - 1;
  if ((unsigned)r < (unsigned)n_loops) keys[r] = (long long)outline_pair(labels[crack[k] >> 2], k);      // labels are >= 0: a positive key
}

__global__ void __launch_bounds__(CGC_BLOCK) k_outline_tables(int n, int n_loops, const long long* __restrict__ keys,
                                                              const int* __restrict__ crack, const int* __restrict__ steps,
                                                              int* __restrict__ loop_label, int* __restrict__ loop_start,
                                                              int* __restrict__ loop_cracks, int* __restrict__ loop_of) {
  const int p = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (p >= n_loops) return;
  const u64 key = (u64)keys[p];
  int k = outline_lo(key);
  if ((unsigned)k >= (unsigned)n) k = 0;                           // keys that are not k_outline_keys' stay inside the tables
  loop_label[p] = outline_hi(key);
  loop_start[p] = crack[k];
  loop_cracks[p] = steps[k] + 1;
  loop_of[k] = p;
}

struct OutlinePoint { int y, x; };

// crack_ptr: int64 [n_loops + 1], the prefix sum of loop_cracks.  slots: the tails in output order.  keep (or null): keep[t] = the
// vertex of slot t lies between two cracks of different direction.
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_scatter(int n, int n_loops, int W, const int* __restrict__ crack,
                                                               const int* __restrict__ succ, const int* __restrict__ start,
                                                               const int* __restrict__ steps, const int* __restrict__ loop_of,
                                                               const long long* __restrict__ crack_ptr, long long* area2,
                                                               OutlinePoint* __restrict__ slots, uint8_t* __restrict__ keep) {
  const int k = blockIdx.x * CGC_BLOCK + threadIdx.x;
  bool valid = k < n;
  int p = -1;
  long long term = 0;
  if (valid) {
    const int s0 = start[k];
    valid = (unsigned)s0 < (unsigned)n;
    if (valid) p = loop_of[s0];
    valid = valid && (unsigned)p < (unsigned)n_loops;
    if (valid) {
      const int len = steps[s0] + 1, pos = steps[s0] - steps[k];
      const long long first = crack_ptr[p];
      const int id = crack[k], s = id & 3, i = id >> 2;
      const int y = i / W, x = i - y * W;
      const int ty = y + (s >= 2), tx = x + (s == 1 || s == 2);    // the tail
      term = (long long)tx * outline_dy(s) - (long long)outline_dx(s) * ty;      // x1 y2 - x2 y1 with (x2, y2) = (x1 + dx, y1 + dy)
      valid = pos >= 0 && pos < len && first >= 0 && first + len <= n;
      if (valid) {
        slots[first + pos] = OutlinePoint{ty, tx};
        const int j = succ[k];
        if (keep != nullptr) keep[first + (pos + 1 == len ? 0 : pos + 1)] = (uint8_t)((unsigned)j < (unsigned)n && (crack[j] & 3) != s);
      } else {
        term = 0;
      }
    }
  }
  if (!valid) p = -1;
  // lane 0 of a wave is valid unless the whole wave is not (k grows with the lane and invalid cracks come from bad tables only)
  const int p0 = __shfl(p, 0);
  if (__all(p == p0 || !valid)) {
    for (int d = CGC_WAVE / 2; d > 0; d >>= 1) term += __shfl_down(term, d);
    if ((threadIdx.x & (CGC_WAVE - 1)) == 0 && p0 >= 0 && term != 0) atomicAdd(reinterpret_cast<u64*>(area2) + p0, (u64)term);
  } else if (valid && term != 0) {
    atomicAdd(reinterpret_cast<u64*>(area2) + p, (u64)term);
  }
}

// place: the INCLUSIVE prefix sum of keep.
__global__ void __launch_bounds__(CGC_BLOCK) k_outline_compact(int n, int n_vertices, const uint8_t* __restrict__ keep,
                                                               const int* __restrict__ place, const OutlinePoint* __restrict__ slots,
                                                               OutlinePoint* __restrict__ vertices) {
  const int t = blockIdx.x * CGC_BLOCK + threadIdx.x;
  if (t >= n || keep[t] == 0) return;
  const int q = place[t] - 1;
  if ((unsigned)q < (unsigned)n_vertices) vertices[q] = slots[t];
}

struct OutlineWs {
  u64* a;      // [n_cracks] the pairs of a doubling round
  u64* b;      // [n_cracks] ... and of the next
};
static inline OutlineWs outline_layout(Carver&& c, int64_t n) {
  OutlineWs w;
  w.a = c.take<u64>(n);
  w.b = c.take<u64>(n);
  return w;
}

static inline bool bad_outline_image(int H, int W, int max_label, const void* within, int wbytes) {
  if (bad_image_dims(H, W) || H > OUTLINE_MAX_SIDE || W > OUTLINE_MAX_SIDE || (int64_t)H * W >= OUTLINE_MAX_PIXELS) return true;
  return max_label < 0 || max_label == 0x7fffffff || (within != nullptr && bad_elem_bytes(wbytes));
}
static inline bool bad_outline_count(int64_t n) { return n < 0 || n >= ((int64_t)1 << 31); }
static inline int outline_rounds(int64_t n) {                     // the smallest r with 2^r >= n
  int r = 0;
  for (; r < 31 && ((int64_t)1 << r) < n; ++r) {
  }
  return r;
}
static inline dim3 outline_grid(int64_t n) { return dim3((unsigned)ceil_div64(n, CGC_BLOCK)); }      // n < 2^31

}  // namespace

extern "C" int cgc_region_outline_rounds(int64_t n_cracks) { return bad_outline_count(n_cracks) ? CGC_EINVAL : outline_rounds(n_cracks); }

extern "C" int64_t cgc_region_outlines_ws_bytes(int64_t n_cracks) {
  if (bad_outline_count(n_cracks)) return 0;
  return layout_bytes(outline_layout, n_cracks);
}

extern "C" int cgc_region_outline_count(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label,
                                        int background, uint8_t* mask, uint8_t* count, int* meta, cgc_stream_t stream) {
  if (bad_outline_image(H, W, max_label, within_or_null, within_bytes) || meta == nullptr) return CGC_EINVAL;
  const int npix = H * W;
  if (npix > 0 && (labels == nullptr || mask == nullptr || count == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(meta, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (npix == 0) return 0;
  const OutlineImage im{labels, within_or_null, within_or_null != nullptr ? within_bytes : 0, H, W, max_label, background != 0 ? 0 : 1};
  hipLaunchKernelGGL(k_outline_count, outline_grid(npix), dim3(CGC_BLOCK), 0, st, im, npix, mask, count, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_outline_cracks(const int* labels, const void* within_or_null, int within_bytes, int H, int W, int max_label,
                                         int connectivity, const uint8_t* mask, const int* offsets, int64_t n_cracks, int* crack, int* succ,
                                         cgc_stream_t stream) {
  if (bad_outline_image(H, W, max_label, within_or_null, within_bytes) || bad_connectivity(connectivity)) return CGC_EINVAL;
  const int npix = H * W;
  if (bad_outline_count(n_cracks) || n_cracks > 4 * (int64_t)npix) return CGC_EINVAL;
  if (n_cracks == 0) return 0;
  if (labels == nullptr || mask == nullptr || offsets == nullptr || crack == nullptr || succ == nullptr) return CGC_EINVAL;
  const OutlineImage im{labels, within_or_null, within_or_null != nullptr ? within_bytes : 0, H, W, max_label, 0};
  hipLaunchKernelGGL(k_outline_cracks, outline_grid(npix), dim3(CGC_BLOCK), 0, as_stream(stream), im, npix, connectivity, mask, offsets,
                     (int)n_cracks, crack, succ);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_outline_loops(int64_t n_cracks, const int* succ, void* ws, int* start, int* steps, cgc_stream_t stream) {
  if (bad_outline_count(n_cracks)) return CGC_EINVAL;
  if (n_cracks == 0) return 0;
  if (succ == nullptr || ws == nullptr || start == nullptr || steps == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const int n = (int)n_cracks, rounds = outline_rounds(n_cracks);
  const dim3 grid = outline_grid(n_cracks), block(CGC_BLOCK);
  const OutlineWs w = outline_layout(Carver(ws), n_cracks);
  u64 *in = w.a, *out = w.b;
  hipLaunchKernelGGL(k_outline_min_init, grid, block, 0, st, n, succ, in);
  CGC_RETURN_IF_LAUNCH_FAILED();
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(k_outline_min_round, grid, block, 0, st, n, in, out);
    CGC_RETURN_IF_LAUNCH_FAILED();
    std::swap(in, out);
  }
  hipLaunchKernelGGL(k_outline_rank_init, grid, block, 0, st, n, in, succ, start, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  std::swap(in, out);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(k_outline_rank_round, grid, block, 0, st, n, in, out);
    CGC_RETURN_IF_LAUNCH_FAILED();
    std::swap(in, out);
  }
  hipLaunchKernelGGL(k_outline_rank_end, grid, block, 0, st, n, in, steps);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_outline_keys(int64_t n_cracks, int64_t n_loops, const int* labels, const int* crack, const int* start,
                                       const int* rank, int64_t* keys, cgc_stream_t stream) {
  if (bad_outline_count(n_cracks) || n_loops < 0 || n_loops > n_cracks) return CGC_EINVAL;
  if (n_loops == 0) return 0;
  if (labels == nullptr || crack == nullptr || start == nullptr || rank == nullptr || keys == nullptr) return CGC_EINVAL;
  hipLaunchKernelGGL(k_outline_keys, outline_grid(n_cracks), dim3(CGC_BLOCK), 0, as_stream(stream), (int)n_cracks, (int)n_loops, labels, crack,
                     start, rank, reinterpret_cast<long long*>(keys));
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_outline_tables(int64_t n_cracks, int64_t n_loops, const int64_t* keys, const int* crack, const int* steps,
                                         int* loop_label, int* loop_start, int* loop_cracks, int64_t* loop_area2, int* loop_of,
                                         cgc_stream_t stream) {
  if (bad_outline_count(n_cracks) || n_loops < 0 || n_loops > n_cracks) return CGC_EINVAL;
  if (n_loops == 0) return 0;
  if (keys == nullptr || crack == nullptr || steps == nullptr || loop_label == nullptr || loop_start == nullptr || loop_cracks == nullptr ||
      loop_area2 == nullptr || loop_of == nullptr)
    return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(loop_area2, 0, (size_t)n_loops * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_outline_tables, outline_grid(n_loops), dim3(CGC_BLOCK), 0, st, (int)n_cracks, (int)n_loops,
                     reinterpret_cast<const long long*>(keys), crack, steps, loop_label, loop_start, loop_cracks, loop_of);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_outline_scatter(int64_t n_cracks, int64_t n_loops, int W, const int* crack, const int* succ, const int* start,
                                          const int* steps, const int* loop_of, const int64_t* crack_ptr, int64_t* loop_area2, int* slots,
                                          uint8_t* keep_or_null, cgc_stream_t stream) {
  if (bad_outline_count(n_cracks) || n_loops < 0 || n_loops > n_cracks || W < 1 || W > OUTLINE_MAX_SIDE) return CGC_EINVAL;
  if (n_loops == 0) return 0;
  if (crack == nullptr || succ == nullptr || start == nullptr || steps == nullptr || loop_of == nullptr || crack_ptr == nullptr ||
      loop_area2 == nullptr || slots == nullptr)
    return CGC_EINVAL;
  hipLaunchKernelGGL(k_outline_scatter, outline_grid(n_cracks), dim3(CGC_BLOCK), 0, as_stream(stream), (int)n_cracks, (int)n_loops, W, crack,
                     succ, start, steps, loop_of, reinterpret_cast<const long long*>(crack_ptr), reinterpret_cast<long long*>(loop_area2),
                     reinterpret_cast<OutlinePoint*>(slots), keep_or_null);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_region_outline_compact(int64_t n_cracks, int64_t n_vertices, const uint8_t* keep, const int* place, const int* slots,
                                          int* vertices, cgc_stream_t stream) {
  if (bad_outline_count(n_cracks) || n_vertices < 0 || n_vertices > n_cracks) return CGC_EINVAL;
  if (n_vertices == 0) return 0;
  if (keep == nullptr || place == nullptr || slots == nullptr || vertices == nullptr) return CGC_EINVAL;
  hipLaunchKernelGGL(k_outline_compact, outline_grid(n_cracks), dim3(CGC_BLOCK), 0, as_stream(stream), (int)n_cracks, (int)n_vertices, keep,
                     place, reinterpret_cast<const OutlinePoint*>(slots), reinterpret_cast<OutlinePoint*>(vertices));
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
