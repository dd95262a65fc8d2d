// Neighbour aggregation on the CSR:  out[i,:] = post[i] * sum_{k in row i} w_k * pre[col[k]] * x[col[k],:]
//
// Replaces torch.matmul(adj, x) of DenseSAGEConv at level 1 (model/network.py:114-116; narrow widths 16..64) and the
// inner product A*S of (S^T A) S (model/network.py:207; width = cluster count, "K4").  HBM-bound gather kernel:
//   * a row group of `lpr` lanes owns one row x one column tile; every lane holds VEC (=4 -> 16-byte) consecutive columns,
//     so each neighbour row is fetched as one contiguous, fully coalesced segment (1 KiB per wave for wide rows);
//   * the row's (col, weight) pairs are read ONCE by the group's lanes (coalesced) and staged in registers; they reach the
//     other lanes through wavefront shuffles -- no per-edge scalar re-reads, no atomics (the row owner writes its result);
//   * gathers are issued four at a time before the first FMA so that ~4 KiB per wave is in flight;
//   * wide rows are cut into column tiles and the block index is remapped so that one XCD (private 4 MiB L2) works on a
//     contiguous range of rows (= a few whole graphs): the ~9x re-read of neighbour rows is then served by that L2.
#include "common.hpp"

constexpr int GATHER_U = 9;   // neighbour rows requested before the first FMA: one batch covers a k-NN(8)+self row

template <int VEC>
__global__ __launch_bounds__(256) void k_spmm(const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ perm,
                                              const float* __restrict__ val, const float* __restrict__ pre,
                                              const float* __restrict__ post, const float* __restrict__ x, float* __restrict__ out,
                                              int n, int W, int ld, int lpr, int n_ctiles, int rows_per_block, int blocks_per_ct,
                                              int n_chunks, int nt_store, const int* __restrict__ gptr) {
  // XCD-contiguous virtual block id (blocks are dealt round-robin to the 8 XCDs; speed only, never correctness)
  const int nb = gridDim.x, b = blockIdx.x;
  const int vb = (nb % 8 == 0) ? (b % 8) * (nb / 8) + b / 8 : b;
  const int per_chunk = blocks_per_ct * n_ctiles;
  const int chunk = vb / per_chunk;
  if (chunk >= n_chunks) return;
  const int rem = vb - chunk * per_chunk;
  const int ct = rem / blocks_per_ct, rb = rem - ct * blocks_per_ct;
  // chunk = rows whose neighbour rows one XCD should keep in its L2 while it sweeps the column tiles: a whole graph
  // when the caller told us the graph boundaries, a fixed row range otherwise
  int row0, row_end;
  if (gptr != nullptr) {
    const int g0 = gptr[chunk], g1 = gptr[chunk + 1];
    row0 = g0 + rb * rows_per_block;
    if (row0 >= g1) return;
    row_end = min(row0 + rows_per_block, g1);
  } else {
    row0 = (chunk * blocks_per_ct + rb) * rows_per_block;
    row_end = min(row0 + rows_per_block, n);
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sl = lane & (lpr - 1), sub = lane / lpr, rpw = 64 / lpr;
  const int c0 = (ct * lpr + sl) * VEC;
  const bool colok = c0 < W;

  for (int rbase = row0 + wave * rpw; rbase < row_end; rbase += 4 * rpw) {
    const int r = rbase + sub;
    const bool valid = r < row_end;
    int s = 0, e = 0;
    if (valid) { s = rowptr[r]; e = rowptr[r + 1]; }
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    for (int k0 = s; k0 < e; k0 += lpr) {
      // stage up to lpr (col, weight) pairs of this row in the group's lanes
      const int kk = k0 + sl;
      int myc = 0;
      float myw = 0.f;
      if (kk < e) {
        myc = col[kk];
        float w = val != nullptr ? val[perm != nullptr ? perm[kk] : kk] : 1.f;
        if (pre != nullptr) w *= pre[myc];
        myw = w;
      }
      const int cnt = min(lpr, e - k0);
      for (int t = 0; t < cnt; t += GATHER_U) {
        Vec<VEC> xv[GATHER_U];
        float ww[GATHER_U];
#pragma unroll
        for (int u = 0; u < GATHER_U; ++u) {
          const int tt = t + u;
          const int cc = __shfl(myc, tt & (lpr - 1), lpr);
          ww[u] = __shfl(myw, tt & (lpr - 1), lpr);
          if (tt < cnt && colok) {
            xv[u].load(x + (size_t)cc * ld + c0);
          } else {
            ww[u] = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) xv[u].v[v] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < GATHER_U; ++u)
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = fmaf(ww[u], xv[u].v[v], acc[v]);
      }
    }
    if (valid && colok) {
      const float ps = post != nullptr ? post[r] : 1.f;
      float* op = out + (size_t)r * ld + c0;
      if (nt_store && VEC == 4) {   // streaming result: keep it from evicting the re-read neighbour rows out of L2
        typedef float f4v __attribute__((ext_vector_type(4)));
        f4v o4 = {acc[0] * ps, acc[VEC > 1 ? 1 : 0] * ps, acc[VEC > 2 ? 2 : 0] * ps, acc[VEC > 3 ? 3 : 0] * ps};
        __builtin_nontemporal_store(o4, reinterpret_cast<f4v*>(op));
      } else {
        Vec<VEC> o;
#pragma unroll
        for (int v = 0; v < VEC; ++v) o.v[v] = acc[v] * ps;
        o.store(op);
      }
    }
  }
}

// Wide rows (> 32 sixteen-byte chunks, "K4"): one WAVE owns (row, 1 KiB column tile), so everything about the sparsity
// pattern is wave-uniform.  Row extents, neighbour ids and edge weights are fetched with SCALAR loads into SGPRs (no lane
// staging, no ds_bpermute shuffles; each gather is one global_load_dwordx4 off a scalar row base), U gathers are in
// flight before the first FMA.  Workgroups are short (4 waves x RUN rows) and dispatched in (graph, column tile, row)
// order on XCD-contiguous ids, so the rows in flight on one XCD stay inside ONE (graph, column tile) slab
// (1800 rows x 1 KiB = 1.8 MB) and the ~9x re-read of neighbour rows is served by that XCD's 4 MiB L2.  (A persistent,
// strided schedule with index prefetch was measured 1.5-1.9x slower: waves drift apart and several slabs compete for L2.)
typedef float wide_f4 __attribute__((ext_vector_type(4)));

// CNT neighbour rows of one (row, column tile): ids and weights through the scalar unit, CNT gathers in flight, then FMAs.
template <int CNT, bool VAL, bool PERM, bool PRE>
__device__ __forceinline__ void wide_batch(const int* __restrict__ col, const int* __restrict__ perm,
                                           const float* __restrict__ val, const float* __restrict__ pre,
                                           const float* __restrict__ xl, int W, int k, wide_f4& acc) {
  int cc[CNT];
  wide_f4 xv[CNT];
  float ww[CNT];
#pragma unroll
  for (int u = 0; u < CNT; ++u) cc[u] = col[k + u];
#pragma unroll
  for (int u = 0; u < CNT; ++u) xv[u] = *reinterpret_cast<const wide_f4*>(xl + (size_t)cc[u] * W);   // (nt loads: 2.1x slower, they skip L2)
#pragma unroll
  for (int u = 0; u < CNT; ++u) ww[u] = 1.f;
  if (VAL) {
    int pi[CNT];
#pragma unroll
    for (int u = 0; u < CNT; ++u) pi[u] = PERM ? perm[k + u] : k + u;
#pragma unroll
    for (int u = 0; u < CNT; ++u) ww[u] = val[pi[u]];
  }
  if (PRE) {
    float pr[CNT];
#pragma unroll
    for (int u = 0; u < CNT; ++u) pr[u] = pre[cc[u]];
#pragma unroll
    for (int u = 0; u < CNT; ++u) ww[u] *= pr[u];
  }
#pragma unroll
  for (int u = 0; u < CNT; ++u) acc += ww[u] * xv[u];
}

// row tail (wave-uniform count 0..N): dispatch to the batch of exactly that size
template <int N, bool VAL, bool PERM, bool PRE>
__device__ __forceinline__ void wide_tail(int cnt, const int* __restrict__ col, const int* __restrict__ perm,
                                          const float* __restrict__ val, const float* __restrict__ pre,
                                          const float* __restrict__ xl, int W, int k, wide_f4& acc) {
  if constexpr (N > 0) {
    if (cnt == N) wide_batch<N, VAL, PERM, PRE>(col, perm, val, pre, xl, W, k, acc);
    else wide_tail<N - 1, VAL, PERM, PRE>(cnt, col, perm, val, pre, xl, W, k, acc);
  }
}

template <int U, bool VAL, bool PERM, bool PRE>
__global__ __launch_bounds__(256) void k_spmm_wide(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                   const int* __restrict__ perm, const float* __restrict__ val,
                                                   const float* __restrict__ pre, const float* __restrict__ post,
                                                   const float* __restrict__ x, float* __restrict__ out, int n, int W, int ld,
                                                   int n_ctiles, int run, int blocks_per_ct, int n_chunks,
                                                   const int* __restrict__ gptr, int order, const int* __restrict__ gorder) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const int nb = gridDim.x, b = blockIdx.x;
  const int vb = (nb % 8 == 0) ? (b % 8) * (nb / 8) + b / 8 : b;
  const int per_chunk = blocks_per_ct * n_ctiles;
  const int chunk = vb / per_chunk;
  if (chunk >= n_chunks) return;
  const int rem = vb - chunk * per_chunk;
  const int ct = rem / blocks_per_ct, rb = rem - ct * blocks_per_ct;
  const int rows_per_block = 4 * run;
  int row0, row_end;
  if (gptr != nullptr) {
    // Graph visited by this dispatch slot (a hint about what the 256 MB Infinity Cache still holds of x, which was just
    // written by the previous kernel).  1: x was written in ascending row order (row kernels) -- the 8 XCDs start together
    // on the last 8 graphs and walk down.  2: x was written by a batched GEMM whose XCD-contiguous tile order left the tail
    // of every eighth of the batch in cache -- every XCD walks its own eighth backwards.  0: ascending.
    int gi = chunk;
    if (gorder != nullptr) {              // caller-supplied visiting sequence (size-balanced over the XCDs: large graphs)
      gi = gorder[chunk];
    } else if (order == 1) {
      const int per_x = n_chunks >> 3;
      gi = ((n_chunks & 7) == 0 && (nb & 7) == 0) ? (per_x - 1 - chunk % per_x) * 8 + chunk / per_x : n_chunks - 1 - chunk;
    } else if (order == 2) {
      const int per_x = n_chunks >> 3;
      gi = ((n_chunks & 7) == 0 && (nb & 7) == 0) ? (chunk / per_x) * per_x + (per_x - 1 - chunk % per_x) : n_chunks - 1 - chunk;
    }
    const int g0 = gptr[gi], g1 = gptr[gi + 1];
    row0 = g0 + rb * rows_per_block;
    row_end = min(row0 + rows_per_block, g1);
  } else {
    row0 = (chunk * blocks_per_ct + rb) * rows_per_block;
    row_end = min(row0 + rows_per_block, n);
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = (ct * 64 + lane) * 4;
  if (c0 >= W) return;                       // lanes past the row end (last column tile) retire; indices stay scalar
  const float* __restrict__ xl = x + c0;
  int r = row0 + wave * run;
  const int r_end = min(r + run, row_end);
  if (r >= r_end) return;
  int s = rowptr[r];
  for (; r < r_end; ++r) {
    const int e = rowptr[r + 1];
    f4v acc = {0.f, 0.f, 0.f, 0.f};
    int k = s;
    for (; k + U <= e; k += U) wide_batch<U, VAL, PERM, PRE>(col, perm, val, pre, xl, ld, k, acc);
    wide_tail<U - 1, VAL, PERM, PRE>(e - k, col, perm, val, pre, xl, ld, k, acc);   // exactly as many gathers as entries left
    if (post != nullptr) acc *= post[r];
    __builtin_nontemporal_store(acc, reinterpret_cast<f4v*>(out + (size_t)r * ld + c0));
    s = e;
  }
}

// Launch geometry (the measured best for ~1800-node cell graphs): k_spmm blocks hold 4 waves x (64 / lpr) rows x PASSES rows;
// row-range chunks (graph boundaries unknown) are CHUNK rows; a k_spmm_wide workgroup is 4 waves x RUN rows.
constexpr int SPMM_PASSES = 2, SPMM_CHUNK = 2048, SPMM_RUN = 2;

static int launch_gather(const int* rowptr, const int* col, const int* perm, const float* val, const float* pre, const float* post,
                         const float* x, float* out, int n, int width, int ld, const int* gptr, int B, int nmax, int order,
                         hipStream_t stream, const int* gorder = nullptr) {
  const bool vec = (width % 4 == 0) && (ld % 4 == 0) && aligned16(x) && aligned16(out);
  const int chunks = vec ? width / 4 : width;        // per-lane column chunks in a row
  const int lpr = pick_lpr(chunks);
  const int n_ctiles = ceil_div(chunks, lpr);         // > 1 only for rows wider than 64 chunks (lpr == 64)
  const int rpw = 64 / lpr;
  const int rows_per_block = 4 * rpw * SPMM_PASSES;
  int blocks_per_ct, n_chunks;
  if (gptr != nullptr && n_ctiles > 1) {              // graph-aligned chunks (only matters when rows are tiled)
    blocks_per_ct = ceil_div(nmax, rows_per_block);
    n_chunks = B;
  } else {
    gptr = nullptr;
    const int chunk_rows = ceil_div(SPMM_CHUNK, rows_per_block) * rows_per_block;
    blocks_per_ct = chunk_rows / rows_per_block;
    n_chunks = ceil_div(n, chunk_rows);
  }
  if (vec && lpr == 64) {                             // wave-per-row: scalar index path
    const int rpb = 4 * SPMM_RUN;
    if (gptr != nullptr) {
      blocks_per_ct = ceil_div(nmax, rpb);
    } else {
      const int chunk_rows = ceil_div(SPMM_CHUNK, rpb) * rpb;
      blocks_per_ct = chunk_rows / rpb;
      n_chunks = ceil_div(n, chunk_rows);
    }
    const int nbw = ceil_div(n_chunks * blocks_per_ct * n_ctiles, 8) * 8;
#define WIDE_LAUNCH(V, P, Q)                                                                                              \
  hipLaunchKernelGGL((k_spmm_wide<GATHER_U, V, P, Q>), dim3(nbw), dim3(CGC_BLOCK), 0, stream, rowptr, col, perm, val, pre, \
                     post, x, out, n, width, ld, n_ctiles, SPMM_RUN, blocks_per_ct, n_chunks, gptr, order, gorder)
    const bool hv = val != nullptr, hp = hv && perm != nullptr, hq = pre != nullptr;
    if (!hv && !hq) WIDE_LAUNCH(false, false, false);
    else if (!hv) WIDE_LAUNCH(false, false, true);
    else if (!hp && !hq) WIDE_LAUNCH(true, false, false);
    else if (!hp) WIDE_LAUNCH(true, false, true);
    else if (!hq) WIDE_LAUNCH(true, true, false);
    else WIDE_LAUNCH(true, true, true);
#undef WIDE_LAUNCH
    CGC_RETURN_IF_LAUNCH_FAILED();
    return 0;
  }
  int nb = n_chunks * blocks_per_ct * n_ctiles;
  nb = ceil_div(nb, 8) * 8;
  dim3 grid(nb), block(CGC_BLOCK);
  const int nt = n_ctiles > 1 ? 1 : 0;                // streaming stores only when the rows are tiled
  if (vec)
    hipLaunchKernelGGL(k_spmm<4>, grid, block, 0, stream, rowptr, col, perm, val, pre, post, x, out, n, width, ld, lpr,
                       n_ctiles, rows_per_block, blocks_per_ct, n_chunks, nt, gptr);
  else
    hipLaunchKernelGGL(k_spmm<1>, grid, block, 0, stream, rowptr, col, perm, val, pre, post, x, out, n, width, ld, lpr,
                       n_ctiles, rows_per_block, blocks_per_ct, n_chunks, nt, gptr);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int cgc_spmm(const int* rowptr, const int* col, const int* perm, const float* val, const float* pre, const float* post,
                        const float* x, float* out, int n, int width, cgc_stream_t stream) {
  if (n <= 0 || width <= 0) return 0;
  return launch_gather(rowptr, col, perm, val, pre, post, x, out, n, width, width, nullptr, 0, 0, 0, as_stream(stream));
}

// Graph-aware entry point: gptr[B+1] = first row of each graph (every row's neighbours lie inside its own graph),
// nmax = largest graph.  visit bits 0-1: the visiting-order hint of k_spmm_wide; the other bits are not read.
// gorder (optional, B ints, a permutation of the graphs): the sequence in which the graphs are visited; the eight XCDs take
// consecutive eighths of it.  Scheduling only -- the result does not depend on it.
extern "C" int cgc_spmm_graphs(const int* rowptr, const int* col, const int* perm, const float* val, const float* pre,
                               const float* post, const float* x, float* out, int n, int width, int ld, const int* gptr, int B,
                               int nmax, int visit, const int* gorder, cgc_stream_t stream) {
  if (n <= 0 || width <= 0) return 0;
  if (ld < width) return CGC_EINVAL;
  const int trec = width > 64 ? cgc_timing_begin(CGC_TAG_SPMM_WIDE, n, width, ld, val != nullptr, 0, 0, 0, as_stream(stream)) : -1;
  const int rc = launch_gather(rowptr, col, perm, val, pre, post, x, out, n, width, ld, gptr, B, nmax, visit & 3, as_stream(stream), gorder);
  cgc_timing_end(trec, as_stream(stream));
  return rc;
}
