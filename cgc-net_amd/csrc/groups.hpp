// Launch groups: up to two layers of EQUAL shape -- the embedding and the assignment block of a level run layer by layer in
// lockstep (network.run_blocks_paired / csrc/exec.hip) -- share one launch of each narrow-layer kernel; blockIdx.y picks the
// pointer set.  At 4 graphs per GPU those kernels are 5 us of pure launch + drain each: halving their number is what the pairing buys.
#pragma once
#include "common.hpp"

struct SnFwdPtrs {           // cgc_sage_narrow_fwd
  const float *agg, *W, *bias;
  float *hn, *rinv, *ws;
};
struct SnFwdBn {             // BatchNorm side of a forward layer
  float eps, momentum;
  float *running_mean, *running_var;
  int64_t* nbt;
  float *mean, *istd;
};
struct SnBwdPtrs {           // cgc_sage_narrow_bwd
  const float *dy, *hn, *rinv, *mean, *istd, *gamma, *sums, *agg, *W;
  float *dagg, *ws;
};
struct StatsFinPtrs {        // slots in, BatchNorm vectors out
  const float* ws;
  float *running_mean, *running_var, *mean, *istd;
  long long* nbt;
  float eps, momentum;
};
struct BnApplyPtrs {         // cgc_bn_act_apply
  const float *hn, *mean, *istd, *gamma, *beta;
  float *y, *y2;
  int ldy2;
};
struct BnRedPtrs {           // cgc_bn_bwd_reduce
  const float *dy, *hn, *mean, *istd;
  float* ws;
};

int sage_narrow_fwd_groups(const SnFwdPtrs* g, const SnFwdBn* bn, int ng, int lda, int n, int K, int F, int normalize, int act, int stats,
                           double count, hipStream_t st);
int sage_narrow_bwd_groups(const SnBwdPtrs* g, float* const* dwdb, int ng, int ldy, int n, int F, int act, int normalize, int mode, double count,
                           int lda, int fin, int ldd, hipStream_t st);
int bn_act_apply_groups(const BnApplyPtrs* g, int ng, int n, int F, int act, int ldy, hipStream_t stream);
int bn_bwd_reduce_groups(const BnRedPtrs* g, float* const* sums, int ng, int ldy, int n, int F, int act, hipStream_t stream);
int launch_stats_finalize_groups(const StatsFinPtrs* g, int ng, int slots, int F, double count, hipStream_t stream);
int launch_stats_finalize(const float* ws, int slots, int F, double count, float eps, float momentum, float* running_mean,
                          float* running_var, float* mean, float* istd, int64_t* nbt, hipStream_t stream);
// out_i[c] = sum over the slots of ws_i[slot * width + c] for ng = 1 or 2 slot areas (rowops.hip; instantiated there for float)
template <typename OUT, typename IN>
int launch_reduce_slots(const IN* ws0, OUT* out0, const IN* ws1, OUT* out1, int ng, int slots, int width, hipStream_t stream);
int reduce_batch_sum_rows(const float* ws, float* out, int parts, int rows, int width, int ldo, float beta, hipStream_t stream);   // gemm.hip
