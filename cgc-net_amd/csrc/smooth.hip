// Separable binomial smoothing of a uint8 image ("F10", between the stain plane and its threshold).  One launch: a workgroup loads a
// 64 x 64 tile plus a halo of `radius` pixels (border replicated: coordinates are clamped, so images narrower than the halo need no
// special case) into LDS as 32-bit values, filters its rows there, then its columns, rounds once and stores 4 pixels per lane.
// A wave works on one row of 64 columns in the row pass and on four rows of 16 x 4 columns (one 16-byte LDS read per lane and tap) in
// the column pass: consecutive lanes read consecutive banks in both.
// The arithmetic: kernels.py KernelSpec.binomial_smooth.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

#define SMOOTH_TILE 64
#define SMOOTH_THREADS 256
#define SMOOTH_MAX_RADIUS 5

namespace {

template <int R>
struct Binomial {                      // w[k] = C(2 R, k)
  int w[2 * R + 1];
  constexpr Binomial() : w() {
    w[0] = 1;
    for (int k = 1; k <= 2 * R; ++k) w[k] = w[k - 1] * (2 * R - k + 1) / k;
  }
};

template <int R>
__global__ __launch_bounds__(SMOOTH_THREADS) void k_binomial_smooth(const uint8_t* __restrict__ img, int H, int W, int tiles_x,
                                                                    uint8_t* __restrict__ out) {
  constexpr int T = SMOOTH_TILE, IN_H = T + 2 * R, IN_W = T + 2 * R, LD = IN_W;
  constexpr Binomial<R> B;
  __shared__ int in[IN_H * LD];
  __shared__ __attribute__((aligned(16))) int rows[IN_H * T];
  const int ty0 = (blockIdx.x / tiles_x) * T, tx0 = (blockIdx.x % tiles_x) * T;
  for (int i = threadIdx.x; i < IN_H * IN_W; i += SMOOTH_THREADS) {
    const int r = i / IN_W, c = i - r * IN_W;
    const int y = min(max(ty0 - R + r, 0), H - 1), x = min(max(tx0 - R + c, 0), W - 1);
    in[r * LD + c] = img[(int64_t)y * W + x];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < IN_H * T; i += SMOOTH_THREADS) {
    const int r = i / T, c = i % T;
    int s = 0;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) s += B.w[j] * in[r * LD + c + j];
    rows[i] = s;
  }
  __syncthreads();
  const bool out_dwords = (reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (W & 3) == 0;      // then every row's tile start is aligned
  constexpr int ROUND = R > 0 ? 1 << (4 * R - 1) : 0;
  for (int i = threadIdx.x; i < T * T / 4; i += SMOOTH_THREADS) {
    const int r = i / (T / 4), c = 4 * (i % (T / 4));
    const int y = ty0 + r, x = tx0 + c;
    if (y >= H || x >= W) continue;
    int s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {
      const int4 v = *reinterpret_cast<const int4*>(&rows[(r + k) * T + c]);
      s[0] += B.w[k] * v.x;
      s[1] += B.w[k] * v.y;
      s[2] += B.w[k] * v.z;
      s[3] += B.w[k] * v.w;
    }
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) packed |= (uint32_t)((s[j] + ROUND) >> (4 * R)) << (8 * j);
    uint8_t* o = out + (int64_t)y * W + x;
    if (out_dwords && x + 4 <= W) {
      *reinterpret_cast<uint32_t*>(o) = packed;
    } else {
      for (int j = 0; j < 4; ++j)
        if (x + j < W) o[j] = (uint8_t)(packed >> (8 * j));
    }
  }
}

template <int R>
int launch_smooth(const uint8_t* img, int H, int W, uint8_t* out, hipStream_t st) {
  const int tiles_x = ceil_div(W, SMOOTH_TILE);
  const int64_t tiles = (int64_t)tiles_x * ceil_div(H, SMOOTH_TILE);      // < 2^31 / 64 + 2^25
  hipLaunchKernelGGL(k_binomial_smooth<R>, dim3((unsigned)tiles), dim3(SMOOTH_THREADS), 0, st, img, H, W, tiles_x, out);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // namespace

extern "C" int cgc_binomial_smooth_u8(const uint8_t* img, int H, int W, int radius, uint8_t* out, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || radius < 0 || radius > SMOOTH_MAX_RADIUS) return CGC_EINVAL;
  if ((int64_t)H * W == 0) return 0;
  if (img == nullptr || out == nullptr) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  switch (radius) {
    case 0: return launch_smooth<0>(img, H, W, out, st);
    case 1: return launch_smooth<1>(img, H, W, out, st);
    case 2: return launch_smooth<2>(img, H, W, out, st);
    case 3: return launch_smooth<3>(img, H, W, out, st);
    case 4: return launch_smooth<4>(img, H, W, out, st);
    default: return launch_smooth<5>(img, H, W, out, st);
  }
}
