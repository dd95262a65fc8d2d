// fp32 products on the fp16 matrix cores of gfx950 in THREE passes: every operand element, scaled by a power of two chosen per OUTPUT
// TILE from the largest magnitude of the tile's operand panel, is split into two fp16 values  s x = h + l  (h = fp16(s x), l = fp16(s x - h), both
// round-to-nearest; the residual is exact in fp32), and the product is formed as the three most significant pairs  l h + h l + h h  in
// the matrix core's fp32 accumulator, descaled in registers before the epilogue.  h + l carries 22-23 of the 24 significand bits
// (|s x - h - l| <= 2^-23 |s x| while l is a normal fp16) and the dropped pair l l is below 2^-22 |a||b|: with fp32 accumulation over
// K >= 160 terms the difference to the exact chain of gemm.hip is a fraction of that chain's own rounding (measured per form by
// tests/test_split_gemm_gpu.py; tools/f16_split_model.py is the numpy model that motivated it).  v_mfma_f32_32x32x16_f16 runs at the
// bf16 rate: three pairs are 96 matrix-pipe cycles per 32 x 32 x 16 block against the 192 of gemm_split.hip's six and the 512 of the
// fp32 chain.
//
// What fp16 costs is RANGE, and that is what the scale is for: 5 exponent bits, normal from 2^-14.  A first launch (k_gemm_absmax)
// takes max |x| over the 256 rows of op(A) that an output tile multiplies (all of K, every segment) and over its 128 columns of
// op(B) -- one streaming pass over both operands: the price of the mode, ~50 us per 263 MB operand -- and the product kernel places
// each panel's maximum in [2^14, 2^15).  Elements down to 2^-17 of their panel's maximum then keep both planes normal; below, l and
// finally h go subnormal and the element's ABSOLUTE error stops shrinking at 2^-25 / s = 2^-40 of the panel's maximum (fp32 itself:
// 2^-24 of the element).  Zeros are exact; a panel that is all zero takes s = 1.  (One scale per batch item was the first version:
// the gradient of a 32-graph batch, one item of 58 k rows, had 46 % of its elements below 2^-17 of the tensor's maximum.)
// Domain: finite inputs (an infinite element makes the tiles of its panel NaN; the exact kernel confines it to its row / column).
//
// Third MODE of the same entry points (CGC_GEMM_SPLIT_F16; cgc_level_desc.flags bit 2), for the same products and forms as
// gemm_split.hip, and with its structure: tile 256 x 128, one wave per SIMD with a 128 x 64 wave tile, k-tiles of 16, two LDS stages
// of [2 planes][256 + 128 rows][16 k], global -> registers two k-tiles ahead of the split, split -> LDS two ahead of the MFMAs, a full
// second set of fragment registers (two planes instead of three leave room for it: no retirement order to respect), one barrier per
// k-tile, half tiles.  Per k-tile a wave issues 24 MFMAs (768 pipe cycles) + 12 fragment reads + 12-16 LDS writes + 6 buffer loads +
// ~75 vector instructions.
#include "gemm_split_common.hpp"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// scale slots at the end of the caller's workspace (floats reserved: cgc_gemm_ws_floats() counts them): max |A| per (batch item, 256-row
// tile), max |B| per (batch item, 128-column tile)
constexpr int H_SCALE_FLOATS = 65536;

__device__ __forceinline__ unsigned pack_f16(float a, float b) {      // round to nearest even, a in the low half
  float2v t;
  t[0] = a;
  t[1] = b;
  return __builtin_bit_cast(unsigned, __builtin_convertvector(t, f16x2));
}

// x - float(h) for the low / high fp16 of a packed pair, one instruction each: v_fma_mix_f32 reads the half in place (the compiler
// converts and subtracts: 8 instead of 4 vector instructions per group of four values).  Exact: the residual of a rounding is a float.
__device__ __forceinline__ float resid_lo(unsigned h, float x) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
  return r;
}
__device__ __forceinline__ float resid_hi(unsigned h, float x) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
  return r;
}

// the scale of an operand from the bits of its largest magnitude: 2^(14 - floor(log2 max)), kept inside the normal floats together
// with its reciprocal; 1 for an operand that is all zero
__device__ __forceinline__ void half_scale(unsigned maxbits, float& s, float& inv) {
  const int e = (int)((maxbits >> 23) & 0xffu);
  int ex = 127 + 14 - (e - 127);
  ex = ex < 1 ? 1 : ex > 253 ? 253 : ex;
  if (maxbits == 0u) ex = 127;
  s = __builtin_bit_cast(float, (unsigned)ex << 23);
  inv = __builtin_bit_cast(float, (unsigned)(254 - ex) << 23);
}

// What the pipeline of gemm_split_common.hpp (split_gemm_body; gemm_split.hip's header has its reasons) does in this number format:
// two planes, 24 MFMAs per k-tile
struct F16x2 : SplitPlanes<2> {                       // LDS: 73728 bytes
  // the scales of the tile's two operand panels and their reciprocals
  struct Scale {
    float sa, sb, isa, isb;
    __device__ __forceinline__ Scale(const GemmArgs& a, int b, int tile_m, int tile_n) {
      const int ta = a.per_batch / a.tiles_n;                    // row tiles of the largest item: the slot layout of k_gemm_absmax
      const unsigned* sc = a.scale + (size_t)b * (ta + a.tiles_n);
      half_scale(sc[tile_m], sa, isa);
      half_scale(sc[ta + tile_n], sb, isb);
    }
    // two multiplications (1 / (sa sb) alone may leave the normal range)
    __device__ __forceinline__ floatx16 descale(floatx16 v) const {
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = (v[r] * isa) * isb;
      return v;
    }
  };
  // ---- the split of one group of four values in four micro-steps (sidx = 4 * group + step; groups 0-3: operand A, 4-5: operand B)
  static constexpr int STEPS = 4;
  struct Group {
    float x[4], r[4];
    unsigned hp[2], lp[2];
  };
  template <class LoaderA, class LoaderB, bool MASKED>
  static __device__ __forceinline__ void micro(int sidx, Group (&gs)[6], const float4 (&ra)[LoaderA::NF], const float4 (&rb)[LoaderB::NF],
                                               unsigned char* wa, unsigned char* wb, int k0, int klim, const Scale& sc) {
    const int u = sidx >> 2, st = sidx & 3;
    Group& s = gs[u];
    if (st == 0) {
      if (u < 4) LoaderA::get(ra, u, s.x); else LoaderB::get(rb, u - 4, s.x);
      const float scl = u < 4 ? sc.sa : sc.sb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s.x[e] *= scl;
        if (MASKED) {
          const int ke = k0 + (u < 4 ? LoaderA::kof(u, e) : LoaderB::kof(u - 4, e));
          s.x[e] = ke < klim ? s.x[e] : 0.f;
        }
      }
      s.hp[0] = pack_f16(s.x[0], s.x[1]);
      s.hp[1] = pack_f16(s.x[2], s.x[3]);
    } else if (st == 1) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        s.r[2 * h] = resid_lo(s.hp[h], s.x[2 * h]);
        s.r[2 * h + 1] = resid_hi(s.hp[h], s.x[2 * h + 1]);
      }
      asm volatile("" : "+v"(s.r[0]), "+v"(s.r[1]), "+v"(s.r[2]), "+v"(s.r[3]));
    } else if (st == 2) {
      s.lp[0] = pack_f16(s.r[0], s.r[1]);
      s.lp[1] = pack_f16(s.r[2], s.r[3]);
    } else {
      if (u < 4) {
        LoaderA::put(wa, u, 0, s.hp[0], s.hp[1]);
        LoaderA::put(wa, u, PLA, s.lp[0], s.lp[1]);
      } else {
        LoaderB::put(wb, u - 4, 0, s.hp[0], s.hp[1]);
        LoaderB::put(wb, u - 4, PLB, s.lp[0], s.lp[1]);
      }
    }
  }

  // a full second set of fragment registers: the next tile's 12 reads of 16 bytes (8 for a half tile) go into the other set
  struct Frags {
    uint4v a[2][4][2], b[2][2][2];            // [set = tile parity][sub-tile][plane h, l]
  };
  template <int POS>
  static __device__ __forceinline__ floatx16 mfma(const Frags& fr, int t, int i, int j, floatx16 acc) {
    constexpr int PA_[3] = {1, 0, 0}, PB_[3] = {0, 1, 0};          // l h, h l, h h: the small pairs first
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fr.b[POS][j][PB_[t]]), __builtin_bit_cast(f16x8, fr.a[POS][i][PA_[t]]), acc, 0, 0, 0);
  }
  template <bool HALF>
  static __device__ __forceinline__ void read_first(Frags& fr, const unsigned char* st, unsigned fa_off, unsigned fb_off) {
#pragma unroll
    for (int i = 0; i < (HALF ? 2 : 4); ++i)
#pragma unroll
      for (int p = 0; p < 2; ++p) fr.a[0][i][p] = frag16(st + fa_off + i * 32 * SROW + p * PLA);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) fr.b[0][j][p] = frag16(st + fb_off + j * 32 * SROW + p * PLB);
  }
  template <int POS, bool HALF>
  static __device__ __forceinline__ void read_next(Frags& fr, int m, const unsigned char* rstage, unsigned fa_off, unsigned fb_off) {
    if (m < 8) { if ((m >> 1) < (HALF ? 2 : 4)) fr.a[POS ^ 1][m >> 1][m & 1] = frag16(rstage + fa_off + (m >> 1) * 32 * SROW + (m & 1) * PLA); }
    else if (m < 12) fr.b[POS ^ 1][(m - 8) >> 1][m & 1] = frag16(rstage + fb_off + ((m - 8) >> 1) * 32 * SROW + (m & 1) * PLB);
  }
  template <bool HALF>
  static __device__ __forceinline__ void end_tile(Frags&) {}
  // (group 3 of A took its values at m = 12, group 1 of B at m = 20)
  static constexpr int LOAD_A = 13, LOAD_B = 21;

  static bool prepare(GemmPlan<2, 2, 4, 2>& plan, int batch, int m_extent, float* ws, int64_t& ws_floats);
  static int before(const GemmArgs& a, int form, int batch, int m_extent, hipStream_t stream);
};

template <bool TA, bool TB>
__global__ __launch_bounds__(256, 1) void k_gemm_half(const GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char slds[];
  split_gemm_tile<F16x2, TA, TB>(a, slds);
}

// ---- max |x| per OUTPUT TILE's operand panel: for batch item b, scale[b * (ta + tn) + t] = the bits of max |x| over rows
// 256 t .. 256 t + 255 of op(A) (all of K, every segment) and scale[b * (ta + tn) + ta + t] over columns 128 t .. 128 t + 127 of op(B)
// (bits of a non-negative float: unsigned order is magnitude order; the caller zeroes the slots).  grid (panels x their sub-ranges,
// batch items): a workgroup streams a share of one panel's rows -- stored rows of 16-byte units, one or two per wave-load.
__device__ __forceinline__ float rect_absmax(const float* __restrict__ p, int rows, int cols, int ld, int w, int nw, int lane) {
  float m0 = 0.f, m1 = 0.f;
  const int cv = cols & ~3;
  const int lpr = cols > 128 ? 64 : 32, rpl = 64 / lpr;      // lanes per stored row, stored rows per wave-load
  const int l = lane % lpr, step = nw * rpl;
  int r = w * rpl + lane / lpr;
  for (; r + step < rows; r += 2 * step) {                    // two trips' loads in flight
    const float* q0 = p + (size_t)r * ld;
    const float* q1 = p + (size_t)(r + step) * ld;
#pragma unroll 5
    for (int c = l * 4; c < cv; c += lpr * 4) {
      const float4 u = *reinterpret_cast<const float4*>(q0 + c), v = *reinterpret_cast<const float4*>(q1 + c);
      m0 = fmaxf(m0, fmaxf(fmaxf(fabsf(u.x), fabsf(u.y)), fmaxf(fabsf(u.z), fabsf(u.w))));
      m1 = fmaxf(m1, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    if (l < cols - cv) {                                      // (the padding behind the panel's last column is not the operand's)
      m0 = fmaxf(m0, fabsf(q0[cv + l]));
      m1 = fmaxf(m1, fabsf(q1[cv + l]));
    }
  }
  if (r < rows) {
    const float* q0 = p + (size_t)r * ld;
    for (int c = l * 4; c < cv; c += lpr * 4) {
      const float4 u = *reinterpret_cast<const float4*>(q0 + c);
      m0 = fmaxf(m0, fmaxf(fmaxf(fabsf(u.x), fabsf(u.y)), fmaxf(fabsf(u.z), fabsf(u.w))));
    }
    if (l < cols - cv) m0 = fmaxf(m0, fabsf(q0[cv + l]));
  }
  return fmaxf(m0, m1);
}
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_gemm_absmax(const GemmArgs a, unsigned* __restrict__ scale, int ta, int sub_a, int sub_b) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const TileBase tb(a, b);
  const int M = tb.M, K = tb.K, N = a.N;
  const bool is_a = (int)blockIdx.x < ta * sub_a;
  const int id = is_a ? (int)blockIdx.x : (int)blockIdx.x - ta * sub_a;
  const int sub = is_a ? sub_a : sub_b, t = id / sub, w = (id - t * sub) * 4 + wave, nw = sub * 4;
  const int lo = t * (is_a ? S_BM : S_BN), ext = is_a ? M : N;
  if (lo >= ext) return;
  const int len = min(is_a ? S_BM : S_BN, ext - lo);
  const size_t roff = a.ragged == 1 ? (size_t)a.gptr[b] : 0;
  float m = 0.f;
  for (int i = -1; i < a.nx; ++i) {            // the main pair, then the extra K segments
    const float* base = is_a ? (i < 0 ? tb.A : a.xA[i] + (size_t)b * a.xsA[i] + roff * a.xlda[i]) : (i < 0 ? tb.B : a.xB[i] + (size_t)b * a.xsB[i]);
    const int ld = is_a ? (i < 0 ? a.lda : a.xlda[i]) : (i < 0 ? a.ldb : a.xldb[i]);
    const int kk = i < 0 ? K : a.xK[i];
    const bool k_is_row = is_a ? TA : !TB;     // the operand is stored [K, .]: the panel is a column window of it
    m = fmaxf(m, k_is_row ? rect_absmax(base + lo, kk, len, ld, w, nw, lane) : rect_absmax(base + (size_t)lo * ld, len, kk, ld, w, nw, lane));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  // one atomic per WORKGROUP, and only when it would raise the slot: thousands of atomics on one address execute one after the other
  // at the memory side (the first version -- two per wave, 16 k per launch on two addresses -- spent two thirds of its time there)
  __shared__ float red[4];
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned bits = __builtin_bit_cast(unsigned, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
    unsigned* slot = scale + (size_t)b * (ta + a.tiles_n) + (is_a ? t : ta + t);
    if (bits > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, bits);
  }
}

static int64_t g_half_launches = 0;
// tile x k-tile steps below which gemm_half_launch declines (tuning hook, tests: 0 = never decline)
static int64_t g_half_min_work = 28000;
extern "C" int64_t cgc_gemm_half_min_work(int64_t v) {
  const int64_t old = __atomic_load_n(&g_half_min_work, __ATOMIC_RELAXED);
  if (v >= 0) __atomic_store_n(&g_half_min_work, v, __ATOMIC_RELAXED);
  return old;
}
extern "C" int64_t cgc_gemm_half_count(void) { return __atomic_load_n(&g_half_launches, __ATOMIC_RELAXED); }
int64_t gemm_half_scale_floats() { return H_SCALE_FLOATS; }
extern "C" int64_t cgc_gemm_half_ws_floats(void) { return H_SCALE_FLOATS; }

// false: no workspace for the scales / more panels than slots / a product too small for the mode to pay.  Otherwise the scale slots
// are taken from the end of the workspace.
bool F16x2::prepare(GemmPlan<2, 2, 4, 2>& plan, int batch, int m_extent, float* ws, int64_t& ws_floats) {
  if (ws == nullptr || ws_floats < H_SCALE_FLOATS || batch > 65535) return false;
  const long long slots = (long long)batch * (ceil_div(m_extent, S_BM) + plan.a.tiles_n);
  if (slots > H_SCALE_FLOATS) return false;
  // The mode pays once the product kernel's saving (~30 % of the bf16 kernel's time) exceeds its own fixed cost (the slot fill, the
  // maximum pass: two launches and one more trip over the operands).  Measured on the step's six products at 32 / 16 / 8 / 4 graphs
  // (profiles/r06_configurations.txt): ahead of the bf16 mode by 18 / 17 / 10 % down to 8 graphs (37-47 k tile x k-tile steps per
  // product), behind it by 6 % at 4 (19-23 k) and at C1 = 180 (5 k).  Below 28 k steps the caller runs the bf16 kernel instead.
  if (plan.tiles * plan.kt < __atomic_load_n(&g_half_min_work, __ATOMIC_RELAXED)) return false;
  ws_floats -= H_SCALE_FLOATS;
  plan.a.scale = reinterpret_cast<unsigned*>(ws + ws_floats);
  return true;
}
// the slot fill and the maximum pass
int F16x2::before(const GemmArgs& a, int form, int batch, int m_extent, hipStream_t stream) {
  unsigned* scale = const_cast<unsigned*>(a.scale);
  int ta = ceil_div(m_extent, S_BM);
  const hipError_t e = hipMemsetAsync(scale, 0, sizeof(unsigned) * (size_t)batch * (ta + a.tiles_n), stream);
  if (e != hipSuccess) return (int)e;
  // ~4 workgroups per CU for each operand, a panel's rows shared by up to 64 of them
  auto subs = [&](int panels) { const long long n = (long long)batch * panels; const int v = n >= 1024 ? 1 : ceil_div(1024, (int)n); return v > 64 ? 64 : v; };
  int sub_a = subs(ta), sub_b = subs(a.tiles_n);
  static const void* const kern[3] = {reinterpret_cast<const void*>(&k_gemm_absmax<false, false>), reinterpret_cast<const void*>(&k_gemm_absmax<false, true>),
                                      reinterpret_cast<const void*>(&k_gemm_absmax<true, false>)};
  void* args[] = {const_cast<GemmArgs*>(&a), &scale, &ta, &sub_a, &sub_b};
  (void)hipLaunchKernel(kern[form], dim3((unsigned)(ta * sub_a + a.tiles_n * sub_b), (unsigned)batch), dim3(256), args, 0, stream);
  return 0;
}

// CGC_EINVAL: the mode declines (F16x2::prepare) or the shape is outside what the kernel indexes -- the caller then tries the bf16
// kernel and, failing that, the exact one.
int gemm_half_launch(const GemmArgs& a0, int transA, int transB, int batch, int m_extent, int k_extent, float* ws, int64_t ws_floats,
                     hipStream_t stream) {
  static const void* const kern[3] = {reinterpret_cast<const void*>(&k_gemm_half<false, false>), reinterpret_cast<const void*>(&k_gemm_half<false, true>),
                                      reinterpret_cast<const void*>(&k_gemm_half<true, false>)};
  return split_gemm_launch<F16x2>(kern, g_half_launches, a0, transA, transB, batch, m_extent, k_extent, ws, ws_floats, stream);
}
