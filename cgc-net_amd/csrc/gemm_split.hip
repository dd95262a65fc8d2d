// fp32 products on the bf16 matrix cores of gfx950: C = op(A) op(B) with every fp32 operand element split into three bf16 values
// (hi + mid + lo = x exactly: 8 + 8 + 8 mantissa bits, round-to-nearest at every level, both residuals exact in fp32) and the product
// formed as the SIX most significant bf16 x bf16 pairs -- hh, hm, mh, hl, mm, lh; every partial product is exact in fp32 and the sums
// run in the matrix core's fp32 accumulator.  The three dropped pairs (ml, lm, ll) are below 2^-26 of |a||b| each: the result is
// indistinguishable from the fp32 MFMA chain of gemm.hip (max / rms error against float64 measured per form by
// tests/test_kernels_gpu.py::test_split_gemm_*; profiles/r04_bf16_split_probe.txt has the probe that motivated this).
// v_mfma_f32_32x32x16_bf16 issues in 32 cycles per SIMD where the eight v_mfma_f32_32x32x2_f32 of the same k range take 512: six
// pairs are 192 matrix-pipe cycles per 32 x 32 x 16 block against 512.
//
// This is an opt-in MODE of the same entry point (cgc_gemm_f32, mode = CGC_GEMM_SPLIT_BF16; the step
// sequencer: cgc_level_desc.flags bit 1) for the products that take the 128 x 128 route of gemm.hip -- the assignment Linear
// (model/network.py:121-122), S^T (A S), P dA'^T, S dA' of _diff_pool and its backward (:206-207) -- in all their forms: NN / NT / TN,
// ragged M, ragged K, uniform K chunks, extra K segments, beta = 1, tail split.  Everything else stays on the exact kernel.
//
// Domain: finite inputs.  x = hi + mid + lo needs |x| >= 2^-108 or so for lo to be a normal bf16 (below that the low planes lose bits
// gradually and the product degrades towards bf16 x 2 accuracy; zeros are exact); an infinite or > 3.39e38 input gives NaN where the
// exact kernel gives inf (hi = inf, x - hi = NaN).  The network's activations and gradients live in 1e-12 .. 1e3.
//
// Structure (one workgroup per CU: 256 threads = 4 waves, one per SIMD, 512 registers each):
//   tile 256 x 128, wave tile 128 x 64 (4 x 2 accumulators of 32 x 32), k-tiles of 16;
//   LDS: two stages of [3 planes][256 + 128 rows][16 k bf16], rows of 32 B on a 48 B stride (108 KB): a fragment is ONE ds_read_b128
//   (conflict-free: 3 is coprime with the 16 sixteen-byte slots of a bank row), and the 8-byte writes of a k-contiguous operand tile
//   the bank window exactly;
//   global -> registers two k-tiles ahead of the split (two register sets; buffer loads, no vector address arithmetic in the loop),
//   split in registers -> LDS two k-tiles ahead of the MFMAs, fragments read one k-tile ahead, plane by plane into the registers the
//   pair order frees (Bf16x3::Frags below): a wave never waits for LDS or memory inside a k-tile, and there is ONE barrier per k-tile;
//   an operand whose k index is the memory row (A stored [K, M], B stored [K, N]) is transposed in registers for free: a thread loads a
//   4 (k) x 4 (m) block -- 2 x 4 for the 128-wide operand -- and packs along k;
//   the ~130 vector instructions of a k-tile's split are dealt out by hand behind its 48 MFMAs (one micro-step of 2-4 instructions per
//   MFMA, a scheduling fence after each): behind a bf16 MFMA up to ~5 plain vector instructions of the SAME wave issue for free
//   (tools/pipe_overlap_probe.hip), another wave's do not.  What costs is every LDS instruction (~6 cycles of issue) and every
//   buffer load (~27): 36 + 6 per k-tile here (the first version of this kernel: 54 + 6 with 8-byte fragment reads on 40-byte rows and
//   three stages -- 2 % slower).
#include "gemm_split_common.hpp"

// What the pipeline of gemm_split_common.hpp (split_gemm_body) does in this number format
struct Bf16x3 : SplitPlanes<3> {                      // LDS: 110592 bytes
  // ---- the split of one group of four values in eight micro-steps (sidx = 8 * group + step; groups 0-3: operand A, 4-5: operand B)
  static constexpr int STEPS = 8;
  struct Group {
    float x[4], r1[4], r2[4];
    unsigned hp[2], mp[2], lp[2];
  };
  struct Scale {                                      // none: bf16 has the exponent range of fp32
    __device__ __forceinline__ Scale(const GemmArgs&, int, int, int) {}
    __device__ __forceinline__ floatx16 descale(floatx16 v) const { return v; }
  };
  template <class LoaderA, class LoaderB, bool MASKED>
  static __device__ __forceinline__ void micro(int sidx, Group (&gs)[6], const float4 (&ra)[LoaderA::NF], const float4 (&rb)[LoaderB::NF],
                                               unsigned char* wa, unsigned char* wb, int k0, int klim, const Scale&) {
    const int u = sidx >> 3, st = sidx & 7;
    Group& s = gs[u];
    if (st == 0) {
      if (u < 4) LoaderA::get(ra, u, s.x); else LoaderB::get(rb, u - 4, s.x);
      if (MASKED) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ke = k0 + (u < 4 ? LoaderA::kof(u, e) : LoaderB::kof(u - 4, e));
          s.x[e] = ke < klim ? s.x[e] : 0.f;
        }
      }
      s.hp[0] = pack_bf16(s.x[0], s.x[1]);
      s.hp[1] = pack_bf16(s.x[2], s.x[3]);
    } else if (st == 1 || st == 2) {
      const int h = st - 1;
      const float e0 = __builtin_bit_cast(float, s.hp[h] << 16), e1 = __builtin_bit_cast(float, s.hp[h] & 0xffff0000u);
      s.r1[2 * h] = s.x[2 * h] - e0;
      s.r1[2 * h + 1] = s.x[2 * h + 1] - e1;
      asm volatile("" : "+v"(s.r1[2 * h]), "+v"(s.r1[2 * h + 1]));
    } else if (st == 3) {
      s.mp[0] = pack_bf16(s.r1[0], s.r1[1]);
      s.mp[1] = pack_bf16(s.r1[2], s.r1[3]);
    } else if (st == 4 || st == 5) {
      const int h = st - 4;
      const float e0 = __builtin_bit_cast(float, s.mp[h] << 16), e1 = __builtin_bit_cast(float, s.mp[h] & 0xffff0000u);
      s.r2[2 * h] = s.r1[2 * h] - e0;
      s.r2[2 * h + 1] = s.r1[2 * h + 1] - e1;
      asm volatile("" : "+v"(s.r2[2 * h]), "+v"(s.r2[2 * h + 1]));
    } else if (st == 6) {
      s.lp[0] = pack_bf16(s.r2[0], s.r2[1]);
      s.lp[1] = pack_bf16(s.r2[2], s.r2[3]);
    } else {
      if (u < 4) {
        LoaderA::put(wa, u, 0, s.hp[0], s.hp[1]);
        LoaderA::put(wa, u, PLA, s.mp[0], s.mp[1]);
        LoaderA::put(wa, u, 2 * PLA, s.lp[0], s.lp[1]);
      } else {
        LoaderB::put(wb, u - 4, 0, s.hp[0], s.hp[1]);
        LoaderB::put(wb, u - 4, PLB, s.mp[0], s.mp[1]);
        LoaderB::put(wb, u - 4, 2 * PLB, s.lp[0], s.lp[1]);
      }
    }
  }

  // Fragment registers of a wave: one set (the k-tile being multiplied) + a second copy of the two hi planes.  The pair order of a
  // tile -- lh, mm, mh, hl, hm, hh -- retires the planes one after the other, and the NEXT tile's copy of a plane is read (16 bytes per
  // lane and sub-tile: 18 ds_read_b128 per k-tile, 12 for a half tile) as soon as this tile's is dead: A.lo after pair 0, A.mid after
  // pair 2, B.lo after pair 3, B.mid after pair 4; A.hi and B.hi live to the end, so the next tile's go into the second copies (24
  // registers) during pair 0.  96 fragment registers instead of the 144 of a full double buffer -- with two register sets of raw
  // operands (48) and the split's temporaries everything but the accumulators has to fit 256 architectural registers (a full double
  // buffer spilled 1194).  No fragment of the tile being multiplied is read from LDS any more, so its stage is free for the tile after
  // next: TWO stages.
  struct Frags {
    uint4v a[4][3], b[2][3], a0n[4], b0n[2];
  };
  template <int POS>
  static __device__ __forceinline__ floatx16 mfma(const Frags& fr, int t, int i, int j, floatx16 acc) {
    constexpr int PA_[6] = {2, 1, 1, 0, 0, 0}, PB_[6] = {0, 1, 0, 2, 1, 0};      // lh, mm, mh, hl, hm, hh
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fr.b[j][PB_[t]]), __builtin_bit_cast(bf16x8, fr.a[i][PA_[t]]), acc, 0, 0, 0);
  }
  template <bool HALF>
  static __device__ __forceinline__ void read_first(Frags& fr, const unsigned char* st, unsigned fa_off, unsigned fb_off) {
#pragma unroll
    for (int i = 0; i < (HALF ? 2 : 4); ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) fr.a[i][p] = frag16(st + fa_off + i * 32 * SROW + p * PLA);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p) fr.b[j][p] = frag16(st + fb_off + j * 32 * SROW + p * PLB);
  }
  template <int POS, bool HALF>
  static __device__ __forceinline__ void read_next(Frags& fr, int m, const unsigned char* rstage, unsigned fa_off, unsigned fb_off) {
    constexpr int NA = HALF ? 2 : 4;
    if (m < 4) { if (m < NA) fr.a0n[m] = frag16(rstage + fa_off + m * 32 * SROW); }                          // A.hi' (second copy)
    else if (m < 6) fr.b0n[m - 4] = frag16(rstage + fb_off + (m - 4) * 32 * SROW);                         // B.hi' (second copy)
    else if (m >= 8 && m < 12) { if (m - 8 < NA) fr.a[m - 8][2] = frag16(rstage + fa_off + (m - 8) * 32 * SROW + 2 * PLA); }   // A.lo (pair 0 only)
    else if (m >= 24 && m < 28) { if (m - 24 < NA) fr.a[m - 24][1] = frag16(rstage + fa_off + (m - 24) * 32 * SROW + PLA); }   // A.mid (pairs 1, 2)
    else if (m >= 32 && m < 34) fr.b[m - 32][2] = frag16(rstage + fb_off + (m - 32) * 32 * SROW + 2 * PLB);   // B.lo (pair 3)
    else if (m >= 40 && m < 42) fr.b[m - 40][1] = frag16(rstage + fb_off + (m - 40) * 32 * SROW + PLB);   // B.mid (pairs 1, 4)
  }
  template <bool HALF>
  static __device__ __forceinline__ void end_tile(Frags& fr) {
#pragma unroll
    for (int i = 0; i < (HALF ? 2 : 4); ++i) fr.a[i][0] = fr.a0n[i];
    fr.b[0][0] = fr.b0n[0];
    fr.b[1][0] = fr.b0n[1];
  }
  // the registers of set POS are free once group 3 of A (m = 24) and group 1 of B (m = 40) have taken their values
  static constexpr int LOAD_A = 28, LOAD_B = 44;

  static bool prepare(GemmPlan<2, 2, 4, 2>&, int, int, float*, int64_t&) { return true; }
  static int before(const GemmArgs&, int, int, int, hipStream_t) { return 0; }
};

template <bool TA, bool TB>
__global__ __launch_bounds__(256, 1) void k_gemm_split(const GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char slds[];
  split_gemm_tile<Bf16x3, TA, TB>(a, slds);
}

// how many products this process has sent to the split kernel (tests: "did the mode apply to this product?")
static int64_t g_split_launches = 0;
extern "C" int64_t cgc_gemm_split_count(void) { return __atomic_load_n(&g_split_launches, __ATOMIC_RELAXED); }

// Returns CGC_EINVAL when the shape is outside what the kernel indexes (the caller then runs the exact kernel).
int gemm_split_launch(const GemmArgs& a0, int transA, int transB, int batch, int m_extent, int k_extent, float* ws, int64_t ws_floats,
                      hipStream_t stream) {
  static const void* const kern[3] = {reinterpret_cast<const void*>(&k_gemm_split<false, false>), reinterpret_cast<const void*>(&k_gemm_split<false, true>),
                                      reinterpret_cast<const void*>(&k_gemm_split<true, false>)};
  return split_gemm_launch<Bf16x3>(kern, g_split_launches, a0, transA, transB, batch, m_extent, k_extent, ws, ws_floats, stream);
}
