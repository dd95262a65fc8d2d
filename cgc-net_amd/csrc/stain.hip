// Colour deconvolution and the 256-bin histogram ("F10", in front of the foreground map: an H&E tile -> a stain plane -> its Otsu
// threshold).  Two kernels:
//   1. k_stain_separate: Ruifrok-Johnston colour deconvolution in fixed point.  A lane takes 4 pixels = 12 bytes = three dwords of the
//      interleaved image and writes one dword per requested plane.  The optical-density table (256 int32, 1 KB) arrives as a kernel
//      argument and is copied to LDS, where every lane can index it; the 3 x 3 matrix stays in scalar registers.
//   2. k_histogram_u8: counts per workgroup in LDS, one global atomic per non-empty bin and workgroup at the end.  A flat tile -- every
//      lane on one bin -- is the worst case, so (a) a lane reads 16 consecutive pixels and adds a run of equal values with ONE LDS atomic,
//      and (b) every wave owns HIST_COPIES copies of the table, lane l using copy l % HIST_COPIES, laid out bin-major so that the
//      copies of one bin sit on different banks.  A flat tile then costs one atomic per 16 pixels and 8 lanes per address.
// The arithmetic, item by item: kernels.py KernelSpec.stain_separate / histogram_u8.
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

namespace {

struct StainTables {                   // passed by value: 1060 bytes of kernel arguments
  int lut[256];
  int m[9];                            // m[3 * c + s]: channel c (0 R, 1 G, 2 B) -> stain s
};

__device__ __forceinline__ uint32_t stain_level(int c) {      // (c + 2^15) >> 16, arithmetic, clamped to a byte
  const int v = (c + 32768) >> 16;
  return (uint32_t)min(max(v, 0), 255);
}

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
    uint32_t w[3] = {0u, 0u, 0u};      // the 12 bytes of pixels i0 .. i0 + 3 (zeros past the end)
    if (full && in_dwords) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(pix + 3 * i0);
      w[0] = p[0];
      w[1] = p[1];
      w[2] = p[2];
    } else {
      const int64_t nbytes = 3 * (npix - i0) < 12 ? 3 * (npix - i0) : 12;
      for (int k = 0; k < 12; ++k)
        if (k < nbytes) w[k >> 2] |= (uint32_t)pix[3 * i0 + k] << (8 * (k & 3));
    }
    uint32_t packed[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int ch[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int b = 3 * j + k;
        ch[k] = (int)((w[b >> 2] >> (8 * (b & 3))) & 255u);
      }
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

}  // namespace

static inline bool bad_pixel_count(int64_t npix) { return npix < 0 || npix >= ((int64_t)1 << 31); }      // bad_image_dims, for a flat count

extern "C" int cgc_stain_separate(const uint8_t* pix, int64_t npix, int order, const int* lut, const int* m, int planes, uint8_t* out,
                                  cgc_stream_t stream) {
  if (bad_pixel_count(npix) || (order != 0 && order != 1) || lut == nullptr || m == nullptr || planes < 1 || planes > 7)
    return CGC_EINVAL;
  StainTables t;
  for (int v = 0; v < 256; ++v) {
    if (lut[v] < 0 || lut[v] > STAIN_OD_MAX) return CGC_EINVAL;
    t.lut[v] = lut[v];
  }
  for (int s = 0; s < 3; ++s) {        // no int32 sum may overflow: sum_c |m[c][s]| * 5674 < 2^31 - 2^15
    int64_t reach = 0;
    for (int c = 0; c < 3; ++c) reach += (m[3 * c + s] < 0 ? -(int64_t)m[3 * c + s] : (int64_t)m[3 * c + s]) * STAIN_OD_MAX;
    if (reach >= ((int64_t)1 << 31) - 32768) return CGC_EINVAL;
  }
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
