// DiffPool regularisers: the link-prediction and entropy losses that PyG's dense_diff_pool returns next to (out, out_adj)
// (the reference's _diff_pool, model/network.py:194-208, drops them).  Per pooling stage, with s = the assignment matrix (masked
// softmax), A = the adjacency _diff_pool receives, N = the dense padding, numel = B N N, rows = B N:
//   link = ||A - s s^T||_F / numel          ent = (1 / rows) sum_rows sum_j -s_ij log(s_ij + 1e-15)
// Never forming s s^T: per graph ||A_b - S_b S_b^T||^2 = ||A_b||^2 - 2 tr(S_b^T A_b S_b) + ||G_b||^2 with G_b = S_b^T S_b, and
// S_b^T A_b S_b is A'_b, which _diff_pool produces anyway.  The products (G = S^T S, S G) are the GEMM family's; this file holds the
// passes around them.  Padded rows of the dense layout have s = 0: they add nothing to either sum and only count in numel / rows.
// Deterministic: every sum is a fixed grid of per-workgroup partials in double, combined in a fixed order by one workgroup; no atomics.
#include "common.hpp"

#define REG_BLOCK 256
#define REG_PARTS 512            // partial slots per sum (the grid of a pass is at most this many workgroups)
#define REG_EPS 1e-15f

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the workgroup in a fixed order; thread 0 gets the result
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < REG_BLOCK / 64; ++i) r += sh[i];
  return r;
}

__device__ __forceinline__ float ent_term(float s) { return -s * logf(s + REG_EPS); }
__device__ __forceinline__ float ent_grad(float s) { return -logf(s + REG_EPS) - s / (s + REG_EPS); }

// one wave per row: part[block] = sum over the block's rows of sum_j -s log(s + eps)
template <int VEC>
__global__ __launch_bounds__(REG_BLOCK) void k_reg_entropy(const float* __restrict__ S, int n, int C, int ld, double* __restrict__ part) {
  __shared__ double sh[REG_BLOCK / 64];
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (REG_BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (REG_BLOCK / 64);
  double acc = 0.0;
  for (int r = wave; r < n; r += nwaves) {
    const float* row = S + (size_t)r * ld;
    float t = 0.f;
    for (int c = lane * VEC; c < C; c += 64 * VEC) {
      if constexpr (VEC == 4) {
        Vec<4> x;
        x.load_stream(row + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) t += ent_term(x.v[k]);
      } else {
        t += ent_term(row[c]);
      }
    }
    acc += (double)t;
  }
  const double r = block_sum_d(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// part[block] = sum of x[i]^2 over a grid-stride share of x[0, m); m_dev (optional) holds m as an int on the device (the CSR's
// rowptr[n]); x == nullptr: every element is 1 (a CSR without values)
__global__ __launch_bounds__(REG_BLOCK) void k_reg_sumsq(const float* __restrict__ x, int64_t m, const int* __restrict__ m_dev,
                                                         double* __restrict__ part) {
  __shared__ double sh[REG_BLOCK / 64];
  if (m_dev != nullptr) m = (int64_t)*m_dev;
  double acc = 0.0;
  if (x == nullptr) {
    acc = (blockIdx.x == 0 && threadIdx.x == 0) ? (double)m : 0.0;
  } else {
    const int64_t stride = (int64_t)gridDim.x * REG_BLOCK;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
    const int64_t m4 = vec ? m / 4 : 0;
    for (int64_t i = blockIdx.x * (int64_t)REG_BLOCK + threadIdx.x; i < m4; i += stride) {
      Vec<4> v;
      v.load_stream(x + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)v.v[k] * (double)v.v[k];
    }
    for (int64_t i = 4 * m4 + blockIdx.x * (int64_t)REG_BLOCK + threadIdx.x; i < m; i += stride) acc += (double)x[i] * (double)x[i];
  }
  const double r = block_sum_d(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// part[0] = sum_b tr(A'_b), A' [B, C, C] contiguous; one workgroup
__global__ __launch_bounds__(REG_BLOCK) void k_reg_trace(const float* __restrict__ Ap, int B, int C, double* __restrict__ part) {
  __shared__ double sh[REG_BLOCK / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < B * C; i += REG_BLOCK) {
    const int b = i / C, j = i - b * C;
    acc += (double)Ap[((size_t)b * C + j) * C + j];
  }
  const double r = block_sum_d(acc, sh);
  if (threadIdx.x == 0) part[0] = r;
}

// sums the partials (fixed order), then link = sqrt(T) / numel, ent = sum / rows, keep[0] = sqrt(T)
struct RegParts {
  const double *ent, *a2, *g2, *tr;
  int n_ent, n_a2, n_g2;
};
__device__ __forceinline__ double sum_parts(const double* p, int np, double* sh) {
  double v = 0.0;
  for (int i = threadIdx.x; i < np; i += REG_BLOCK) v += p[i];
  const double r = block_sum_d(v, sh);
  __syncthreads();                     // sh is reused by the next sum
  return r;
}
__global__ __launch_bounds__(REG_BLOCK) void k_reg_finalize(const RegParts p, double numel, double rows, float* __restrict__ link,
                                                            float* __restrict__ ent, float* __restrict__ keep) {
  __shared__ double sh[REG_BLOCK / 64];
  const double e = sum_parts(p.ent, p.n_ent, sh);
  const double a2 = sum_parts(p.a2, p.n_a2, sh);
  const double g2 = sum_parts(p.g2, p.n_g2, sh);
  if (threadIdx.x == 0) {
    const double T = a2 - 2.0 * p.tr[0] + g2;
    const double r = T > 0.0 ? sqrt(T) : 0.0;
    *link = (float)(r / numel);
    *ent = (float)(e / rows);
    keep[0] = (float)r;
  }
}

// the coefficients of the backward from the upstream gradients (device memory: no host synchronisation)
__device__ __forceinline__ float link_coef(const float* d_reg, const float* keep, double numel) {
  const double r = (double)keep[0];
  return r > 0.0 ? (float)((double)d_reg[0] / (2.0 * numel * r)) : 0.f;
}

// dao = d_ao - 2 c_l I per graph (d_ao == nullptr: 0), Gs = 4 c_l G; coef = [c_l, c_e].  A workgroup per row of the [B C, C] matrices.
__global__ __launch_bounds__(REG_BLOCK) void k_reg_bwd_prep(const float* __restrict__ d_reg, const float* __restrict__ keep, double numel,
                                                            double rows, const float* __restrict__ d_ao, float* __restrict__ dao,
                                                            const float* __restrict__ G, float* __restrict__ Gs, int B, int C,
                                                            float* __restrict__ coef) {
  const float cl = link_coef(d_reg, keep, numel);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    coef[0] = cl;
    coef[1] = (float)((double)d_reg[1] / rows);
  }
  const float two = 2.f * cl, four = 4.f * cl;
  for (int r = blockIdx.x; r < B * C; r += gridDim.x) {
    const int diag = r % C;
    const size_t o = (size_t)r * C;
    for (int j = threadIdx.x; j < C; j += REG_BLOCK) {
      const float v = d_ao != nullptr ? d_ao[o + j] : 0.f;
      dao[o + j] = j == diag ? v - two : v;
      Gs[o + j] = four * G[o + j];
    }
  }
}

// ds[r, :C] += c_e (-log(s + eps) - s / (s + eps)), one wave per row
template <int VEC>
__global__ __launch_bounds__(REG_BLOCK) void k_reg_entropy_bwd(const float* __restrict__ S, int n, int C, int ld, const float* __restrict__ coef,
                                                               float* __restrict__ ds, int ldd) {
  const float ce = coef[1];
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (REG_BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (REG_BLOCK / 64);
  for (int r = wave; r < n; r += nwaves) {
    const float* srow = S + (size_t)r * ld;
    float* drow = ds + (size_t)r * ldd;
    for (int c = lane * VEC; c < C; c += 64 * VEC) {
      if constexpr (VEC == 4) {
        Vec<4> s, d;
        s.load_stream(srow + c);
        d.load(drow + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) d.v[k] += ce * ent_grad(s.v[k]);
        d.store(drow + c);
      } else {
        drow[c] += ce * ent_grad(srow[c]);
      }
    }
  }
}

// gA (+)= 2 c_l A over m elements
__global__ __launch_bounds__(REG_BLOCK) void k_reg_adj_bwd(const float* __restrict__ A, int64_t m, const float* __restrict__ coef,
                                                           float* __restrict__ gA, int accumulate) {
  const float two = 2.f * coef[0];
  for (int64_t i = blockIdx.x * (int64_t)REG_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * REG_BLOCK) {
    const float v = two * A[i];
    gA[i] = accumulate ? gA[i] + v : v;
  }
}

inline int grid_for(int64_t work, int cap) {
  const int64_t b = (work + REG_BLOCK - 1) / REG_BLOCK;
  return (int)(b < 1 ? 1 : b > cap ? cap : b);
}
inline bool row_vec(const float* a, int C, int ld) { return C % 4 == 0 && ld % 4 == 0 && aligned16(a); }

}  // namespace

extern "C" int64_t cgc_diffpool_reg_ws_floats(void) { return (int64_t)2 * (3 * REG_PARTS + 1); }

extern "C" int cgc_diffpool_reg_fwd(const float* S, int n, int C, int lds, const float* G, const float* A_out, int B, const float* A,
                                    int64_t A_numel, const int* rowptr, double numel, double rows, float* ws, float* link, float* ent,
                                    float* keep, cgc_stream_t stream) {
  if (n < 0 || C < 1 || lds < C || B < 1 || S == nullptr || G == nullptr || A_out == nullptr || ws == nullptr || link == nullptr ||
      ent == nullptr || keep == nullptr || !(numel > 0.0) || !(rows > 0.0))
    return CGC_EINVAL;
  if (A == nullptr && rowptr == nullptr) return CGC_EINVAL;                      // dense A, or the CSR (values or all ones)
  if (rowptr == nullptr && A_numel < 0) return CGC_EINVAL;
  if (!aligned16(ws)) return CGC_EINVAL;
  hipStream_t s = as_stream(stream);
  double* p = reinterpret_cast<double*>(ws);
  RegParts rp;
  rp.ent = p;
  rp.a2 = p + REG_PARTS;
  rp.g2 = p + 2 * REG_PARTS;
  rp.tr = p + 3 * REG_PARTS;
  // entropy: one wave per row
  rp.n_ent = grid_for((int64_t)(n > 0 ? n : 1) * 64, REG_PARTS);
  if (row_vec(S, C, lds))
    hipLaunchKernelGGL(k_reg_entropy<4>, dim3(rp.n_ent), dim3(REG_BLOCK), 0, s, S, n, C, lds, const_cast<double*>(rp.ent));
  else
    hipLaunchKernelGGL(k_reg_entropy<1>, dim3(rp.n_ent), dim3(REG_BLOCK), 0, s, S, n, C, lds, const_cast<double*>(rp.ent));
  CGC_RETURN_IF_LAUNCH_FAILED();
  // ||A||^2: dense [A_numel] floats, or the CSR's values (rowptr[n] of them; A == nullptr: all ones)
  const int64_t a_work = rowptr != nullptr ? (int64_t)REG_PARTS * REG_BLOCK * 4 : A_numel / 4;
  rp.n_a2 = grid_for(a_work, REG_PARTS);
  hipLaunchKernelGGL(k_reg_sumsq, dim3(rp.n_a2), dim3(REG_BLOCK), 0, s, A, A_numel, rowptr != nullptr ? rowptr + n : nullptr,
                     const_cast<double*>(rp.a2));
  CGC_RETURN_IF_LAUNCH_FAILED();
  const int64_t g_numel = (int64_t)B * C * C;
  rp.n_g2 = grid_for(g_numel / 4, REG_PARTS);
  hipLaunchKernelGGL(k_reg_sumsq, dim3(rp.n_g2), dim3(REG_BLOCK), 0, s, G, g_numel, (const int*)nullptr, const_cast<double*>(rp.g2));
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_reg_trace, dim3(1), dim3(REG_BLOCK), 0, s, A_out, B, C, const_cast<double*>(rp.tr));
  CGC_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(k_reg_finalize, dim3(1), dim3(REG_BLOCK), 0, s, rp, numel, rows, link, ent, keep);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_diffpool_reg_bwd_prep(const float* d_reg, const float* keep, double numel, double rows, const float* d_ao, float* dao,
                                         const float* G, float* Gs, int B, int C, float* coef, cgc_stream_t stream) {
  if (d_reg == nullptr || keep == nullptr || dao == nullptr || G == nullptr || Gs == nullptr || coef == nullptr || B < 1 || C < 1 ||
      !(numel > 0.0) || !(rows > 0.0))
    return CGC_EINVAL;
  const int rows_bc = B * C;
  hipLaunchKernelGGL(k_reg_bwd_prep, dim3(rows_bc < 8192 ? rows_bc : 8192), dim3(REG_BLOCK), 0, as_stream(stream), d_reg, keep, numel, rows, d_ao, dao,
                     G, Gs, B, C, coef);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_diffpool_reg_entropy_bwd(const float* S, int n, int C, int lds, const float* coef, float* ds, int ldd, cgc_stream_t stream) {
  if (C < 1 || lds < C || ldd < C || coef == nullptr) return CGC_EINVAL;
  if (n <= 0) return 0;
  const int blocks = grid_for((int64_t)n * 64, 4096);
  if (row_vec(S, C, lds) && ldd % 4 == 0 && aligned16(ds))
    hipLaunchKernelGGL(k_reg_entropy_bwd<4>, dim3(blocks), dim3(REG_BLOCK), 0, as_stream(stream), S, n, C, lds, coef, ds, ldd);
  else
    hipLaunchKernelGGL(k_reg_entropy_bwd<1>, dim3(blocks), dim3(REG_BLOCK), 0, as_stream(stream), S, n, C, lds, coef, ds, ldd);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_diffpool_reg_adj_bwd(const float* A, int64_t m, const float* coef, float* gA, int accumulate, cgc_stream_t stream) {
  if (A == nullptr || gA == nullptr || coef == nullptr || m < 0) return CGC_EINVAL;
  if (m == 0) return 0;
  hipLaunchKernelGGL(k_reg_adj_bwd, dim3(grid_for(m, 4096)), dim3(REG_BLOCK), 0, as_stream(stream), A, m, coef, gA, accumulate);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
