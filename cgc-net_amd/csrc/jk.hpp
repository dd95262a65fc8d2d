// Shared declarations of the DenseJK kernels (jk.hip: thread-per-direction VALU kernels; jk_mfma.hip: matrix-core kernels).
#pragma once
#include "common.hpp"

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

template <int C>
struct JkDims {
  static constexpr int H = 3 * C / 2;
  static constexpr int KIN = C + H;
  static constexpr size_t lds_bytes = sizeof(float4) * (2 * H * KIN + 2 * H) + sizeof(float) * (2 * H + 4);
};

struct JkWeights {            // PyTorch nn.LSTM layout, gate order i,f,g,o; [0] forward direction, [1] reverse
  const float* w_ih[2];       // [4H, C]
  const float* w_hh[2];       // [4H, H]
  const float* b_ih[2];       // [4H]
  const float* b_hh[2];       // [4H]
  const float* w_att;         // [2H]
  const float* b_att;         // [1]
};

// Channel counts the fused kernels are compiled for: every even C up to 32 (hidden H = 3C/2 <= 48; model/network.py:27-33 needs C
// even for the bidirectional split) ...
#define JK_FOR_EACH_C(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28) X(30) X(32)
// ... and those of them that run on the matrix-core kernels of jk_mfma.hip (C % 4 == 0: 16-byte x fragments; H <= 30: one
// 32-row tile per gate with a column left for the bias).  The only place that lists them.
#define JK_FOR_EACH_MFMA_C(X) X(4) X(8) X(12) X(16) X(20)
// ... when the row buffers they read and write as 16-byte fragments (xs, out; xs, dout, dxs) are aligned
static inline bool jk_aligned16(const void* a, const void* b, const void* c = nullptr) { return aligned16(a) && aligned16(b) && aligned16(c); }

// Matrix-core entries (jk_mfma.hip).  Each returns CGC_EINVAL, with nothing launched, for a C outside JK_FOR_EACH_MFMA_C or
// buffers that fail jk_aligned16.
int jk_mfma_fwd(const float* xs, int n, int npad, int C, const JkWeights& w, float* out, float* HS, float* CS, hipStream_t st);
// backward with the parameter gradients accumulated in-kernel: G [2][4H+1][C+2H+1] (same layout as DGT . INT^T)
int64_t jk_mfma_bwd_ws_floats(int C);
int jk_mfma_bwd_params(const float* xs, const float* dout, int n, int npad, int C, const JkWeights& w, const float* HS,
                       const float* CS, float* dxs, float* G, float* ws, hipStream_t st);
// the same with the gradients written straight into the flat parameter-order buffer of cgc_jk_unpack_param_grads
int jk_mfma_bwd_flat(const float* xs, const float* dout, int n, int npad, int C, const JkWeights& w, const float* HS, const float* CS,
                     float* dxs, float* flat, float* ws, hipStream_t st);
