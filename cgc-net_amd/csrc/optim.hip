// The reference's other two optimisers (common/utils.py:119-127: init_optim 'sgd' and 'rmsprop', both with momentum 0.9) as ONE
// launch over all parameter tensors, on the same tables as cgc_adam_step (adam.hip): a device table of cgc_adam_seg rows
// {parameter, state 0, state 1, offset, length, gradient buffer index} and a device table of (segment, 1024-element chunk) pairs,
// one per 256-thread workgroup, both built once by the caller.
//
// Arithmetic, bit for bit what cgc_net_amd.optim's cached-list level calls:
//   * SGD = torch._fused_sgd_ (torch.optim.SGD(fused=True)): the hyper-parameters are doubles, every intermediate is rounded to
//     float, and torch's gfx950 build of that kernel contracts each a + b * c into a double FMA:
//       g = fma(wd, p, g);  buf = fma(momentum, buf, (1 - dampening) * g);  p = fma(-lr, buf, p)
//   * RMSprop = the foreach sequence of torch.optim.RMSprop(foreach=True) (torch/optim/rmsprop.py: _multi_tensor_rmsprop): one
//     torch kernel per line, each rounding to float, scalars rounded to float first; torch's gfx950 foreach kernels contract
//     add(alpha) / addcmul / addcdiv into a float FMA:
//       g = fma(wd, p, g);  sq = sq * alpha;  sq = fma(1 - alpha, g * g, sq);  avg = sqrt(sq) + eps;
//       buf = buf * momentum;  buf = buf + g / avg;  p = fma(-lr, buf, p)          (momentum 0: p = fma(-lr, g / avg, p))
// Those forms were read from torch's own code objects and are held bit for bit by tests/test_optim_gpu.py.  Both kernels switch
// contraction off (#pragma clang fp contract(off): the __f*_rn intrinsics alone do not stop the compiler fusing a product into a
// following add) and write each FMA torch's kernels use as an explicit fma / fmaf, so no compiler choice can move the rounding.
// sqrtf and division are IEEE-rounded (-fhip-fp32-correctly-rounded-divide-sqrt, csrc/Makefile), as in torch's build; the
// __fsqrt_rn intrinsic is not (it compiles to the ~1-ulp v_sqrt_f32).  grad_mul scales the gradient first (a float product), as in
// k_adam_segments.
#include "common.hpp"

struct OptSeg {           // == cgc_adam_seg (alias cgc_opt_seg)
  float* p;
  float* m;               // SGD: momentum_buffer (null when momentum is 0); RMSprop: square_avg
  float* v;               // SGD: unused; RMSprop: momentum_buffer (null when momentum is 0)
  long long off;
  long long n;
  int slot;
  int reserved;
};

__device__ __forceinline__ const float* seg_grad(const OptSeg& sg, const float* g0, const float* g1, const float* g2, const float* g3) {
  const float* gb = sg.slot == 0 ? g0 : (sg.slot == 1 ? g1 : (sg.slot == 2 ? g2 : g3));
  return gb + sg.off;
}

__global__ __launch_bounds__(256) void k_sgd_segments(const OptSeg* __restrict__ segs, const int2* __restrict__ blocks, const float* g0,
                                                      const float* g1, const float* g2, const float* g3, double lr, double momentum,
                                                      double dampening, double wd, float grad_mul) {
#pragma clang fp contract(off)
  const int2 bc = blocks[blockIdx.x];
  const OptSeg sg = segs[bc.x];
  const float* g = seg_grad(sg, g0, g1, g2, g3);
  const bool use_buf = momentum != 0.0;
  if (use_buf && sg.m == nullptr) return;          // (a segment without its buffer: see cgc_sgd_step)
  const double one_minus_d = 1.0 - dampening;
  const long long base = (long long)bc.y * 1024 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = base + k * 256;
    if (i < sg.n) {
      const float param = sg.p[i];
      float grad = g[i];
      if (grad_mul != 1.f) grad *= grad_mul;
      if (wd != 0.0) grad = (float)fma(wd, (double)param, (double)grad);
      if (use_buf) {
        grad = (float)fma(momentum, (double)sg.m[i], one_minus_d * (double)grad);
        sg.m[i] = grad;
      }
      sg.p[i] = (float)fma(-lr, (double)grad, (double)param);
    }
  }
}

__global__ __launch_bounds__(256) void k_rmsprop_segments(const OptSeg* __restrict__ segs, const int2* __restrict__ blocks,
                                                          const float* g0, const float* g1, const float* g2, const float* g3, double lr,
                                                          double alpha, double eps, double wd, double momentum, float grad_mul) {
#pragma clang fp contract(off)
  const int2 bc = blocks[blockIdx.x];
  const OptSeg sg = segs[bc.x];
  const float* g = seg_grad(sg, g0, g1, g2, g3);
  const bool use_buf = momentum > 0.0;
  if (sg.m == nullptr || (use_buf && sg.v == nullptr)) return;      // (a segment without its state: see cgc_sgd_step)
  // the scalars as torch hands them to its float kernels: each rounded to float once
  const float wd_f = (float)wd, alpha_f = (float)alpha, one_minus_alpha_f = (float)(1.0 - alpha), eps_f = (float)eps;
  const float momentum_f = (float)momentum, neg_lr_f = (float)(-lr);
  const long long base = (long long)bc.y * 1024 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = base + k * 256;
    if (i < sg.n) {
      const float param = sg.p[i];
      float grad = g[i];
      if (grad_mul != 1.f) grad *= grad_mul;
      if (wd != 0.0) grad = fmaf(wd_f, param, grad);
      float sq = sg.m[i] * alpha_f;
      sq = fmaf(one_minus_alpha_f, grad * grad, sq);
      sg.m[i] = sq;
      const float avg = sqrtf(sq) + eps_f;
      const float q = grad / avg;
      if (use_buf) {
        const float buf = sg.v[i] * momentum_f + q;
        sg.v[i] = buf;
        sg.p[i] = fmaf(neg_lr_f, buf, param);
      } else {
        sg.p[i] = fmaf(neg_lr_f, q, param);
      }
    }
  }
}

// A segment without the state its rule reads (a null pointer where momentum needs a buffer) is skipped by the kernels, never written
// through: the tables live on the device, so the check is per segment there.  optim.py builds no such table.
extern "C" int cgc_sgd_step(const void* segs, const void* blocks, int nblocks, const float* const* grad_buffers, double lr, double momentum,
                            double dampening, double weight_decay, float grad_mul, cgc_stream_t stream) {
  if (nblocks <= 0) return 0;
  if (segs == nullptr || blocks == nullptr || grad_buffers == nullptr || momentum < 0.0) return CGC_EINVAL;
  hipLaunchKernelGGL(k_sgd_segments, dim3((unsigned)nblocks), dim3(256), 0, as_stream(stream), static_cast<const OptSeg*>(segs),
                     static_cast<const int2*>(blocks), grad_buffers[0], grad_buffers[1], grad_buffers[2], grad_buffers[3], lr, momentum,
                     dampening, weight_decay, grad_mul);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_rmsprop_step(const void* segs, const void* blocks, int nblocks, const float* const* grad_buffers, double lr, double alpha,
                                double eps, double weight_decay, double momentum, float grad_mul, cgc_stream_t stream) {
  if (nblocks <= 0) return 0;
  if (segs == nullptr || blocks == nullptr || grad_buffers == nullptr || momentum < 0.0) return CGC_EINVAL;
  hipLaunchKernelGGL(k_rmsprop_segments, dim3((unsigned)nblocks), dim3(256), 0, as_stream(stream), static_cast<const OptSeg*>(segs),
                     static_cast<const int2*>(blocks), grad_buffers[0], grad_buffers[1], grad_buffers[2], grad_buffers[3], lr, alpha, eps,
                     weight_decay, momentum, grad_mul);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
