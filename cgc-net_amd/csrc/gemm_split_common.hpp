// Shared by the kernels that run an fp32 product on the 16-bit matrix cores of gfx950 from operands split in registers
// (gemm_split.hip: three bf16 planes, six pairs; gemm_half.hip: two fp16 planes, three pairs): the 256 x 128 x 16 tile's loaders
// (global -> registers -> [plane][row][16 k] in LDS, the transposition of an operand stored [K, .] done by register naming), the
// 16-byte fragment read, and the PIPELINE itself -- device body, kernel entry, host launch -- stated once over a mode type that
// supplies what the two number formats do differently (SplitPlanes and the list in front of split_gemm_body).
#pragma once
#include <type_traits>

#include "gemm_common.hpp"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

#define SBK 16                          // k-tile
#define SROW 48                         // bytes per LDS row of a plane: 16 bf16 + 16 bytes of padding (16-byte-aligned rows for ds_read_b128)
constexpr int S_BM = 256, S_BN = 128;

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {      // v_cvt_pk_bf16_f32: round to nearest even, a in the low half
  float2v t;
  t[0] = a;
  t[1] = b;
  return __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2));
}
__device__ __forceinline__ float comp(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// Everything below is written so that, once the per-tile loops are fully unrolled, every array index is a constant (the register
// arrays then live in registers) and no closure survives: free functions with explicit arguments, no lambda inside a lambda (a
// by-reference lambda nested in another kept its closure -- a struct of pointers to locals -- in scratch memory: gemm.hip).

// Operand whose K index is the contiguous one in memory (A stored [M, K]; B stored [N, K]).  ROWS x 16 tile = ROWS * 4 units of
// 16 bytes; thread t: unit q = t & 3 of rows row_of(i), i = 0 .. ROWS / 64 - 1.  A unit is one "group": four consecutive k of one row.
template <int ROWS, int RS = SROW>
struct SplitLoaderK {
  static constexpr int NF = ROWS / 64, NG = NF;
  // row of unit i: 64 i + 16 wave + r16 with r16 = ((t >> 4) & 1) + 8 ((t >> 5) & 1) + 2 ((t >> 2) & 3): the 16 lanes of an LDS write group
  // (8-byte writes) hold rows b, b + 2, b + 4, b + 6 -- on the 48-byte row stride their 32-byte windows start 96 = -32 (mod 128) bytes
  // apart and tile the 128-byte bank window exactly (consecutive rows overlap: a quarter of the LDS cycles of the first version of
  // this kernel were bank conflicts)
  static __device__ __forceinline__ int row_of(int i) {
    const int t = (int)threadIdx.x;
    static_assert(RS == 48, "the row mapping tiles the bank window for 48-byte rows");
    return 64 * i + 16 * (t >> 6) + ((t >> 4) & 1) + 8 * ((t >> 5) & 1) + 2 * ((t >> 2) & 3);
  }
  static __device__ __forceinline__ void offsets(unsigned (&off)[NF], int ld, int row0, int row_last) {
#pragma unroll
    for (int i = 0; i < NF; ++i) off[i] = (unsigned)min(row0 + row_of(i), row_last) * (unsigned)ld * 4u + (threadIdx.x & 3u) * 16u;
  }
  static __device__ __forceinline__ unsigned soffset(int /*ld*/, int k0) { return (unsigned)k0 * 4u; }
  // any tile of any segment: units past the end of K re-read the last valid 16 bytes of their row (the split zeroes them)
  static __device__ __forceinline__ float4 load_any(int i, const float* __restrict__ base, int ld, int row0, int row_last, int k0, int klim) {
    const int row = min(row0 + row_of(i), row_last);
    const int k = min(k0 + (int)(threadIdx.x & 3) * 4, (klim - 1) & ~3);
    return *reinterpret_cast<const float4*>(base + (size_t)row * ld + k);
  }
  static __device__ __forceinline__ void get(const float4 (&reg)[NF], int u, float (&x)[4]) {
    x[0] = reg[u].x; x[1] = reg[u].y; x[2] = reg[u].z; x[3] = reg[u].w;
  }
  static __device__ __forceinline__ int kof(int /*u*/, int e) { return (int)(threadIdx.x & 3) * 4 + e; }      // k of element e inside the tile
  static __device__ __forceinline__ unsigned wbase() { return (unsigned)row_of(0) * RS + (threadIdx.x & 3u) * 8u; }
  static __device__ __forceinline__ void put(unsigned char* st, int u, int plane_off, unsigned w0, unsigned w1) {   // st = stage + region + wbase()
    *reinterpret_cast<uint2*>(st + u * 64 * RS + plane_off) = make_uint2(w0, w1);
  }
};

// Operand whose M / N index is the contiguous one (A stored [K, M]; B stored [K, N]).  16 x COLS tile; a thread owns a KH x 4 block
// (KH = 4 for the 256-wide operand, 2 for the 128-wide one): lane -> (kgrp = t % (16 / KH), g = t / (16 / KH)); float4 j of the block is
// row k = KH * kgrp + j, columns 4 g .. 4 g + 3.  The 16 lanes of an LDS write group then cover 4 column groups x 4 k groups (KH = 4:
// 8-byte writes) or the 32 lanes 4 x 8 (KH = 2: 4-byte writes): at most two lanes per bank on the 48-byte stride (free for 4-byte writes).
// Groups: KH = 4: column c of the block (its four k); KH = 2: columns 2u, 2u + 1 (two k each).  The transposition is a choice of
// register names.
template <int COLS, int RS = SROW>
struct SplitLoaderMN {
  static constexpr int KH = COLS / 64, NF = KH, NG = KH == 4 ? 4 : 2, KG = 16 / KH;
  static __device__ __forceinline__ int kgrp() { return (int)threadIdx.x % KG; }
  static __device__ __forceinline__ int g() { return (int)threadIdx.x / KG; }
  static __device__ __forceinline__ void offsets(unsigned (&off)[NF], int ld, int col0, int col_last4) {
#pragma unroll
    for (int j = 0; j < NF; ++j)
      off[j] = (unsigned)(KH * kgrp() + j) * (unsigned)ld * 4u + (unsigned)min(col0 + 4 * g(), col_last4) * 4u;
  }
  static __device__ __forceinline__ unsigned soffset(int ld, int k0) { return (unsigned)k0 * (unsigned)ld * 4u; }
  // rows (k) past the end re-read row klim - 1 (the split zeroes them)
  static __device__ __forceinline__ float4 load_any(int j, const float* __restrict__ base, int ld, int col0, int col_last4, int k0, int klim) {
    const int k = min(k0 + KH * kgrp() + j, klim - 1);
    return *reinterpret_cast<const float4*>(base + (size_t)k * ld + min(col0 + 4 * g(), col_last4));
  }
  static __device__ __forceinline__ void get(const float4 (&reg)[NF], int u, float (&x)[4]) {
    if constexpr (KH == 4) {
      x[0] = comp(reg[0], u); x[1] = comp(reg[1], u); x[2] = comp(reg[2], u); x[3] = comp(reg[3], u);
    } else {
      x[0] = comp(reg[0], 2 * u); x[1] = comp(reg[1], 2 * u); x[2] = comp(reg[0], 2 * u + 1); x[3] = comp(reg[1], 2 * u + 1);
    }
  }
  static __device__ __forceinline__ int kof(int /*u*/, int e) { return KH == 4 ? 4 * kgrp() + e : 2 * kgrp() + (e & 1); }
  static __device__ __forceinline__ unsigned wbase() { return (unsigned)g() * 4u * RS + (unsigned)kgrp() * (KH == 4 ? 8u : 4u); }
  static __device__ __forceinline__ void put(unsigned char* st, int u, int plane_off, unsigned w0, unsigned w1) {
    if constexpr (KH == 4) {
      *reinterpret_cast<uint2*>(st + u * RS + plane_off) = make_uint2(w0, w1);
    } else {
      *reinterpret_cast<unsigned*>(st + (2 * u) * RS + plane_off) = w0;
      *reinterpret_cast<unsigned*>(st + (2 * u + 1) * RS + plane_off) = w1;
    }
  }
};

__device__ __forceinline__ uint4v frag16(const unsigned char* p) { return *reinterpret_cast<const uint4v*>(p); }

// LDS of a mode with NP planes per operand: two stages of [NP planes][256 + 128 rows][16 k]
template <int NP_>
struct SplitPlanes {
  static constexpr int NP = NP_, PLA = S_BM * SROW, PLB = S_BN * SROW, STAGE = NP * (PLA + PLB), LDS = 2 * STAGE;
};

// One tile (HALF: a tile of <= 128 valid rows: 64 x 64 per wave) or one K piece of a tail tile.  Two instantiations per kernel, chosen
// per workgroup: as two loop nests inside ONE body the accumulators, fragments and operand registers had to agree at every merge point
// and the allocator spilled 107-124 registers; as two bodies that share nothing but the arguments it spills none.
//
// Pipeline (gemm_split.hip's header has the reasons): global -> registers two k-tiles ahead of the split (two register sets; buffer
// loads, no vector address arithmetic in the loop), split in registers -> LDS two k-tiles ahead of the MFMAs (two stages), fragments
// read one k-tile ahead; one micro-step of the split behind every MFMA with a scheduling fence after it; ONE barrier per k-tile.
// Mode (Bf16x3: gemm_split.hip, F16x2: gemm_half.hip) supplies, as static members with explicit arguments:
//   NP, PLA, PLB, STAGE, LDS  SplitPlanes
//   STEPS                     micro-steps of the split of one group of four values; six groups = 6 STEPS MFMAs per k-tile (8 per pair)
//   Group, micro<>()          state of a group's split; micro-step sidx = STEPS * group + step (groups 0-3: operand A, 4-5: operand B)
//   Frags, mfma<>()           fragment registers of a wave; MFMA of sub-tile (i, j) for pair t of the mode's pair order
//   read_first<>(), read_next<>(), end_tile<>()   all fragments of tile 0; what is read of the next tile behind MFMA m; the hand-over
//   LOAD_A, LOAD_B            MFMA index behind which the A / B global loads of the tile after next start (its registers are free
//                             once the split's last group of that operand has taken its values)
//   Scale                     per-tile operand scales: loaded from (a, b, tile_m, tile_n), applied by micro(), descale() of an accumulator
template <class Mode, bool TA, bool TB, bool HALF>
__device__ __forceinline__ void split_gemm_body(const GemmArgs& a, const int b, const int tile_id, const int piece, const int S, const unsigned tj,
                                                unsigned char* const slds) {
  constexpr int TM = 4, TN = 2, WGN = 2, NA = HALF ? 2 : 4, NM = 6 * Mode::STEPS;
  constexpr int NP = Mode::NP, PLA = Mode::PLA, STAGE = Mode::STAGE, LOAD_A = Mode::LOAD_A, LOAD_B = Mode::LOAD_B;
  const TileBase tb(a, b);
  const int M = tb.M, K = tb.K, N = a.N;
  const float* A = tb.A;
  const float* B = tb.B;
  float* C = tb.C;
  const int tile_m = tile_id / a.tiles_n, tile_n = tile_id - tile_m * a.tiles_n;
  const int m0 = tile_m * S_BM, n0 = tile_n * S_BN;
  if (m0 >= M) return;

  const typename Mode::Scale sc(a, b, tile_m, tile_n);

  typedef typename std::conditional<TA, SplitLoaderMN<S_BM, SROW>, SplitLoaderK<S_BM, SROW>>::type LoaderA;
  typedef typename std::conditional<TB, SplitLoaderK<S_BN, SROW>, SplitLoaderMN<S_BN, SROW>>::type LoaderB;
  static_assert(LoaderA::NG == 4 && LoaderB::NG == 2, "six groups of four values per thread and k-tile");
  constexpr int NFA = LoaderA::NF, NFB = LoaderB::NF;
  static_assert(LOAD_A + NFA <= NM && LOAD_B + NFB <= NM, "the loads of a k-tile are issued behind its MFMAs");
  float4 ra[2][NFA], rb[2][NFB];            // two register sets: tile t lives in set t % 2 from its request until its split

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WGN, wn = wave - wm * WGN;
  const int l31 = lane & 31, lhi = lane >> 5;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk_main = (K + SBK - 1) / SBK, nk_full = K / SBK;
  SegTable seg;
  seg.A0 = A; seg.B0 = B; seg.lda0 = a.lda; seg.ldb0 = a.ldb; seg.K0 = K;
  seg.A1 = seg.A2 = A; seg.B1 = seg.B2 = B; seg.lda1 = seg.lda2 = a.lda; seg.ldb1 = seg.ldb2 = a.ldb; seg.K1 = seg.K2 = K;
  seg.nk_main = nk_main;
  seg.nkx0 = 0;
  int nkx1 = 0;
  if (a.nx > 0) {
    const size_t roff = a.ragged == 1 ? (size_t)a.gptr[b] : 0;
    seg.A1 = a.xA[0] + (size_t)b * a.xsA[0] + roff * a.xlda[0];
    seg.B1 = a.xB[0] + (size_t)b * a.xsB[0];
    seg.lda1 = a.xlda[0]; seg.ldb1 = a.xldb[0]; seg.K1 = a.xK[0];
    seg.nkx0 = (a.xK[0] + SBK - 1) / SBK;
    if (a.nx > 1) {
      seg.A2 = a.xA[1] + (size_t)b * a.xsA[1] + roff * a.xlda[1];
      seg.B2 = a.xB[1] + (size_t)b * a.xsB[1];
      seg.lda2 = a.xlda[1]; seg.ldb2 = a.xldb[1]; seg.K2 = a.xK[1];
      nkx1 = (a.xK[1] + SBK - 1) / SBK;
    }
  }
  const int nk = nk_main + seg.nkx0 + nkx1;
  const int kbeg = S > 1 ? (int)(((long long)nk * piece) / S) : 0;
  const int kend = S > 1 ? (int)(((long long)nk * (piece + 1)) / S) : nk;
  const int n = kend - kbeg;
  const int a_last = TA ? ((M - 1) & ~3) : M - 1, b_last = TB ? N - 1 : ((N - 1) & ~3);

  unsigned offA[NFA], offB[NFB];
  LoaderA::offsets(offA, a.lda, m0, a_last);
  LoaderB::offsets(offB, a.ldb, n0, b_last);
  const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, 0xffffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrcB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(B), 0, 0xffffffff, 0x00020000);

  const unsigned fa_off = (unsigned)((HALF ? wm * 64 : wm * 128) + l31) * SROW + lhi * 16, fb_off = NP * PLA + (unsigned)(wn * 64 + l31) * SROW + lhi * 16;
  const unsigned wa_off = LoaderA::wbase(), wb_off = NP * PLA + LoaderB::wbase();

  typename Mode::Frags fr;
  // ---- prologue: tiles 0, 1 split into stages 0, 1; tiles 2, 3 in flight in the two sets; all fragments of tile 0 in registers.
  // An EMPTY k range (an empty graph of a ragged-K batch; a tail-split piece of a graph with fewer k-tiles than pieces) loads
  // nothing -- there is no valid tile to clamp to (kbeg - 1 would be rows of the previous graph, or in front of the operand) --
  // and goes straight to the epilogue / its slab with zero accumulators, as k_gemm_f32 does (gemm.hip: `if (kend > kbeg)`).
  if (n > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {             // q: 0, 1 request tiles 0, 1; 2: split 0, request 2; 3: split 1, request 3
      const int set = q & 1;
      if (q >= 2) {
        const SegTile t = seg_tile<SBK>(seg, kbeg + (q - 2 < n ? q - 2 : n - 1));
        typename Mode::Group gs[6];
#pragma unroll
        for (int sidx = 0; sidx < NM; ++sidx)
          Mode::template micro<LoaderA, LoaderB, true>(sidx, gs, ra[set], rb[set], slds + (q - 2) * STAGE + wa_off,
                                                       slds + (q - 2) * STAGE + wb_off, t.k0, t.klim, sc);
      }
      const SegTile t = seg_tile<SBK>(seg, kbeg + (q < n ? q : n - 1));
#pragma unroll
      for (int i = 0; i < NFA; ++i) ra[set][i] = LoaderA::load_any(i, t.A, t.lda, m0, a_last, t.k0, t.klim);
#pragma unroll
      for (int i = 0; i < NFB; ++i) rb[set][i] = LoaderB::load_any(i, t.B, t.ldb, n0, b_last, t.k0, t.klim);
    }
    __syncthreads();
    Mode::template read_first<HALF>(fr, slds, fa_off, fb_off);
    __syncthreads();                          // (step 0 writes tile 2 into stage 0: everybody has read tile 0 out of it)
  }

  auto tile_step = [&](auto pos_c, auto full_c, int lt) {
    constexpr int POS = decltype(pos_c)::value;          // local tile index mod 2: its stage, its register sets
    constexpr bool FULL = decltype(full_c)::value;
    const unsigned char* rstage = slds + (POS ^ 1) * STAGE;        // tile lt + 1
    unsigned char* wa = slds + POS * STAGE + wa_off;               // tile lt + 2 goes where tile lt was
    unsigned char* wb = slds + POS * STAGE + wb_off;
    typename Mode::Group gs[6];
    int k0s = 0, klims = 0;
    SegTile tnext;
    unsigned soffA = 0, soffB = 0;
    if constexpr (!FULL) {
      const SegTile ts = seg_tile<SBK>(seg, kbeg + (lt + 2 < n ? lt + 2 : n - 1));
      k0s = ts.k0;
      klims = ts.klim;
      tnext = seg_tile<SBK>(seg, kbeg + (lt + 4 < n ? lt + 4 : n - 1));
    } else {
      tnext.A = A; tnext.B = B; tnext.lda = a.lda; tnext.ldb = a.ldb; tnext.klim = K; tnext.k0 = 0;
      const int tl = min(kbeg + lt + 4, nk_full - 1);
      soffA = LoaderA::soffset(a.lda, tl * SBK);
      soffB = LoaderB::soffset(a.ldb, tl * SBK);
    }
#pragma clang loop unroll(full)
    for (int m = 0; m < NM; ++m) {
      const int t = m / 8, ij = m % 8, i = ij >> 1, j = ij & 1;
      if (!HALF || i < 2) acc[i][j] = Mode::template mfma<POS>(fr, t, i, j, acc[i][j]);      // (HALF: sub-tiles i >= 2 of the wave do not exist)
      Mode::template read_next<POS, HALF>(fr, m, rstage, fa_off, fb_off);
      Mode::template micro<LoaderA, LoaderB, !FULL>(m, gs, ra[POS], rb[POS], wa, wb, k0s, klims, sc);
      if (m >= LOAD_A && m < LOAD_A + NFA) {
        if constexpr (FULL) ra[POS][m - LOAD_A] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrcA, offA[m - LOAD_A], soffA, 0));
        else ra[POS][m - LOAD_A] = LoaderA::load_any(m - LOAD_A, tnext.A, tnext.lda, m0, a_last, tnext.k0, tnext.klim);
      }
      if (m >= LOAD_B && m < LOAD_B + NFB) {
        if constexpr (FULL) rb[POS][m - LOAD_B] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrcB, offB[m - LOAD_B], soffB, 0));
        else rb[POS][m - LOAD_B] = LoaderB::load_any(m - LOAD_B, tnext.B, tnext.ldb, n0, b_last, tnext.k0, tnext.klim);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    Mode::template end_tile<HALF>(fr);
    __syncthreads();
  };
  typedef std::true_type FULL_;
  typedef std::false_type ANY_;
#define SPLIT_POS(P_) std::integral_constant<int, P_>()
  int lt = 0;
  const int last_special = nk - nk_full;
  const int full_steps = min(last_special > 0 && kend > nk_full ? nk_full - 4 - kbeg : nk_full - 2 - kbeg, n);
  for (; lt + 2 <= full_steps; lt += 2) {
    tile_step(SPLIT_POS(0), FULL_(), lt);
    tile_step(SPLIT_POS(1), FULL_(), lt + 1);
  }
  for (; lt < n; ++lt) {
    if ((lt & 1) == 0) tile_step(SPLIT_POS(0), ANY_(), lt);
    else tile_step(SPLIT_POS(1), ANY_(), lt);
  }
#undef SPLIT_POS

#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = sc.descale(acc[i][j]);

  float* const lds_f = reinterpret_cast<float*>(slds);
  if (S > 1) {
    float* slab = a.ws + ((size_t)tj * S + piece) * (size_t)(S_BM * S_BN) + (size_t)wave * (TM * TN * 16 * 64) + lane * 4;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(slab + ((i * TN + j) * 4 + g) * 256) =
              make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
    return;
  }
  if constexpr (HALF) {
    floatx16 ah[2][TN];                    // (by value: a reference to a part of acc would put the accumulators in memory)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) ah[i][j] = acc[i][j];
    gemm_epilogue<2, TN>(a, C, M, N, m0 + wm * 64, n0 + wn * TN * 32, ah, lds_f + wave * 32 * (TN * 32 + 4), lane);
  } else {
    gemm_epilogue<TM, TN>(a, C, M, N, m0 + wm * TM * 32, n0 + wn * TN * 32, acc, lds_f + wave * 32 * (TN * 32 + 4), lane);
  }
}

// Kernel entry: which tile or tail piece this workgroup computes (wave-uniform: in scalar registers), then one of the two bodies
template <class Mode, bool TA, bool TB>
__device__ __forceinline__ void split_gemm_tile(const GemmArgs& a, unsigned char* const slds) {
  int b, tile_id, piece, S;
  unsigned tj;
  {
    TileMap<S_BM> map;
    map.init(a, threadIdx.x & 63);
    if (!map.select(a, blockIdx.x, threadIdx.x & 63, b, tile_id, tj, piece, S)) return;
  }
  b = __builtin_amdgcn_readfirstlane(b);
  tile_id = __builtin_amdgcn_readfirstlane(tile_id);
  piece = __builtin_amdgcn_readfirstlane(piece);
  S = __builtin_amdgcn_readfirstlane(S);
  tj = __builtin_amdgcn_readfirstlane(tj);
  const TileBase tb(a, b);
  const int rows_left = tb.M - (tile_id / a.tiles_n) * S_BM;
  if (S == 1 && rows_left <= 128) {
    split_gemm_body<Mode, TA, TB, true>(a, b, tile_id, piece, S, tj, slds);
    return;
  }
  split_gemm_body<Mode, TA, TB, false>(a, b, tile_id, piece, S, tj, slds);
}

// Workgroups the chip holds at once: one per CU (256 threads = 4 waves, one per SIMD, 512 registers each)
static const int kSplitResident = 256;

// Launch kern[NN, NT, TN] for a product that qualifies (gemm.hip: gemm_dispatch decided: 128 x 128 route, every operand segment fit for
// unguarded 16-byte loads) and count it.  CGC_EINVAL when the shape is outside what the kernel indexes or the mode declines
// (Mode::prepare, which may also keep the end of the workspace for itself); the caller then runs another kernel.  Mode::before
// enqueues what the mode needs in front of the product kernel.
template <class Mode>
int split_gemm_launch(const void* const (&kern)[3], int64_t& count, const GemmArgs& a0, int transA, int transB, int batch, int m_extent,
                      int k_extent, float* ws, int64_t ws_floats, hipStream_t stream) {
  if (transA && transB) return CGC_EINVAL;
  // (k offsets are 32-bit scalar byte offsets, 16 k rows of an [K, .] operand at a time: same limits as the exact kernel checked)
  GemmPlan<2, 2, 4, 2> plan;
  if (!plan.init(a0, batch, m_extent, k_extent, SBK)) return CGC_EINVAL;
  if (!Mode::prepare(plan, batch, m_extent, ws, ws_floats)) return CGC_EINVAL;
  if (ws != nullptr) plan.tail_split(ws, ws_floats, 8, kSplitResident);      // a piece keeps >= 8 k-tiles: the pipeline is five deep
  plan.timing_begin(m_extent, k_extent, stream);
  const int form = transA ? 2 : transB ? 1 : 0;
  const int e = Mode::before(plan.a, form, batch, m_extent, stream);
  if (e != 0) return e;
  static bool attr[3][CGC_MAX_DEVICES] = {};
  cgc_allow_lds(kern[form], Mode::LDS, attr[form]);
  void* args[] = {&plan.a};
  (void)hipLaunchKernel(kern[form], plan.grid(), dim3(256), args, Mode::LDS, stream);
  CGC_RETURN_IF_LAUNCH_FAILED();
  __atomic_fetch_add(&count, 1, __ATOMIC_RELAXED);
  return plan.finish(stream);
}
